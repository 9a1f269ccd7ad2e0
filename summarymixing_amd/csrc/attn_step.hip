// attn_step.hip - the pieces of one KV-cached seq2seq decoding step (include/smx.h: smx_attn_step, smx_s2s_embed_step,
// smx_s2s_select), gfx950 only.  Every position of the search lives on the device (pos / n_keys / n_tok / done), so the host issues the
// same launches at every step and one captured step serves every position.
//
//   a. attn_step_kernel     one query row per (batch row, head) over a (B, cap, H, D) cache.  A memory-bound read of K and V: 16-byte
//                           loads from global memory straight into registers, no LDS tiles, no MFMA.  LPK = min(64, D / N) lanes
//                           share a key (N = elements per 16 bytes), so a wave walks 64 / LPK keys at once; each such lane group keeps
//                           an online (max, sum, accumulator) triple over its keys, the groups of a wave meet in a butterfly, the four
//                           waves through LDS in wave order.  The keys of a row are cut into `nsplit` contiguous chunks, one workgroup
//                           each (nsplit depends on cap alone, never on B or n_keys); with nsplit > 1 the workgroups write their
//                           triples to the workspace and attn_step_combine_kernel folds them in chunk order.  No atomics.
//                           Self-attention: the workgroup of chunk 0 stores k_new / v_new into slot n - 1, and EVERY workgroup reads
//                           that key from k_new / v_new, never from the cache, so no workgroup waits for another's store.
//   b. s2s_embed_step_kernel  Y[b] = table[tok[b]] sqrt(D) + pe[pos[b]], then pos[b] += 1 (one workgroup owns a row: read the
//                           counter, barrier, one lane writes).
//   c. s2s_select_kernel    one wave per row of logits (row_scan.h): arg-max, log-probability, append to the hypothesis.
// A NaN never wins a comparison; every sum has one fixed order: two runs agree bit for bit.
#include "row_scan.h"

#include <limits.h>

namespace smx {

static constexpr int AS_THREADS = 256;
static constexpr int AS_WAVES = AS_THREADS / 64;
static constexpr int AS_UNROLL = 4;                     // keys a lane group has in flight
static constexpr int AS_SPLIT_KEYS = 64;                // a workgroup per this many keys of cap ...
static constexpr int AS_MAX_SPLIT = 16;                 // ... up to this many
static constexpr int AS_MAX_CAP = 1 << 16;

static int as_nsplit(int cap) {
  const int n = (cap + AS_SPLIT_KEYS - 1) / AS_SPLIT_KEYS;
  return n < 1 ? 1 : (n > AS_MAX_SPLIT ? AS_MAX_SPLIT : n);
}
static int as_chunk(int cap) { const int ns = as_nsplit(cap); return (cap + ns - 1) / ns; }

// (m, s, acc) meets (om, os, oacc): both sides rescaled to the common maximum; an empty side (max -inf) contributes nothing
template <int E>
__device__ __forceinline__ void as_meet(float& m, float& s, float (&acc)[E], float om, float os, const float (&oacc)[E]) {
  const float M = fmaxf(m, om);
  const float fa = m == NEG_INF ? 0.f : expf(m - M), fb = om == NEG_INF ? 0.f : expf(om - M);
  s = s * fa + os * fb;
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = acc[e] * fa + oacc[e] * fb;
  m = M;
}

// what smx_attn_step_rows adds to the descriptor (read by the ROWS instantiations alone)
struct AsRows {
  const int32_t* anc; long ld_anc;      // (B, cap): the cache row that holds key j of query row b, or null
  int kv_div;                           // query row b reads cache row (and n_keys entry) b / kv_div
  int rows;                             // cache rows: an anc entry outside [0, rows) is a key that contributes nothing
};

// grid = (nsplit, H, B), block = 256.  ws (nsplit > 1): per (b, h, split) D + 2 floats [max, sum, acc (D)].
// ROWS (smx_attn_step_rows): the cache row of a key is looked up, not b - one 4-byte load per key per lane group, all AS_UNROLL of
// them requested before the first K / V load that depends on one.  The arithmetic is the same code either way.
template <typename T, int D, bool ROWS>
__global__ __launch_bounds__(AS_THREADS) void attn_step_kernel(smx_attn_step_args a, AsRows x, int nsplit, int chunk) {
  constexpr int N = Grp16<T>::N;
  constexpr int LPK = (D / N) < 64 ? (D / N) : 64;      // lanes that share a key
  constexpr int G = D / (N * LPK);                      // 16-byte groups a lane holds of it
  constexpr int KPW = 64 / LPK;                         // keys a wave walks at once
  constexpr int E = G * N;
  __shared__ float red[AS_WAVES][D + 2];
  const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l = lane % LPK, ks = lane / LPK;
  const int bk = ROWS ? b / x.kv_div : b;               // the cache row (and key count) of this query row
  int n = a.n_keys ? a.n_keys[bk] : a.cap;
  if (n < 1 || n > a.cap) n = 0;                        // outside [1, cap]: a zero row, no store, no access
  const T* q = (const T*)a.q.p + (long)b * a.q.sb + (long)h * a.q.sh;
  const T* Kh = (const T*)a.K.p + (long)h * a.K.sh;
  const T* Vh = (const T*)a.V.p + (long)h * a.V.sh;
  const T* K = Kh + (long)bk * a.K.sb;
  const T* V = Vh + (long)bk * a.V.sb;
  const int32_t* anc = ROWS && x.anc ? x.anc + (long)b * x.ld_anc : nullptr;
  const T* kn = a.k_new.p ? (const T*)a.k_new.p + (long)b * a.k_new.sb + (long)h * a.k_new.sh : nullptr;
  const T* vn = a.k_new.p ? (const T*)a.v_new.p + (long)b * a.v_new.sb + (long)h * a.v_new.sh : nullptr;
  const int last = kn && n > 0 ? n - 1 : -1;            // the key that is read from k_new / v_new
  if (last >= 0 && split == 0) {                        // the step's own key / value row -> cache slot n - 1
    for (int c = t * N; c < D; c += AS_THREADS * N) {
      float f[N];
      Grp16<T>::load(kn + c, f);
      Grp16<T>::store(const_cast<T*>(K) + (long)last * a.K.sr + c, f);
      Grp16<T>::load(vn + c, f);
      Grp16<T>::store(const_cast<T*>(V) + (long)last * a.V.sr + c, f);
    }
  }
  float qv[E];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float f[N];
    Grp16<T>::load(q + (g * LPK + l) * N, f);
#pragma unroll
    for (int j = 0; j < N; ++j) qv[g * N + j] = f[j];
  }
  float m = NEG_INF, s = 0.f, acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.f;
  const int j_lo = split * chunk, j_hi = min(n, j_lo + chunk);
  // lane group (wave, ks) walks keys j_lo + wave KPW + ks, + AS_WAVES KPW, ...; AS_UNROLL of them are requested before the first is used
  // (the trip count is the wave's, so every lane of a wave reaches the shuffles below)
  for (int jw = j_lo + wave * KPW; jw < j_hi; jw += AS_WAVES * KPW * AS_UNROLL) {
    const int j0 = jw + ks;
    float kf[AS_UNROLL][E], vf[AS_UNROLL][E];
    int row[AS_UNROLL];                                 // ROWS: the cache row of key u, -1: the key contributes nothing
    if constexpr (ROWS) {
#pragma unroll
      for (int u = 0; u < AS_UNROLL; ++u) {
        const int j = j0 + u * AS_WAVES * KPW;
        row[u] = j < j_hi ? (anc && j != last ? anc[j] : bk) : -1;
        if (row[u] < 0 || row[u] >= x.rows) row[u] = -1;  // compared BEFORE it becomes an address
      }
    }
#pragma unroll
    for (int u = 0; u < AS_UNROLL; ++u) {
      const int j = j0 + u * AS_WAVES * KPW;
      if (ROWS ? row[u] >= 0 : j < j_hi) {
        const T* kr = j == last ? kn : (ROWS ? Kh + (long)row[u] * a.K.sb : K) + (long)j * a.K.sr;
        const T* vr = j == last ? vn : (ROWS ? Vh + (long)row[u] * a.V.sb : V) + (long)j * a.V.sr;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float f[N];
          Grp16<T>::load(kr + (g * LPK + l) * N, f);
#pragma unroll
          for (int i = 0; i < N; ++i) kf[u][g * N + i] = f[i];
          Grp16<T>::load(vr + (g * LPK + l) * N, f);
#pragma unroll
          for (int i = 0; i < N; ++i) vf[u][g * N + i] = f[i];
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) { kf[u][e] = 0.f; vf[u][e] = 0.f; }
      }
    }
#pragma unroll
    for (int u = 0; u < AS_UNROLL; ++u) {
      const int j = j0 + u * AS_WAVES * KPW;
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) d = fmaf(qv[e], kf[u][e], d);
#pragma unroll
      for (int off = LPK / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);     // (every lane of the wave takes part)
      if (ROWS ? row[u] >= 0 : j < j_hi) {
        const float sc = d * a.scale;
        const float M = fmaxf(m, sc);
        const float f = m == NEG_INF ? 0.f : expf(m - M), p = expf(sc - M);
        s = s * f + p;
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = fmaf(p, vf[u][e], acc[e] * f);
        m = M;
      }
    }
  }
  // the lane groups of the wave meet in a butterfly over the key slot; only the ks == 0 group's result is used below (under
  // -ffast-math the two partners of a stage may contract their sums differently, so the other groups need not hold the same bits)
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
    const float om = __shfl_xor(m, off, 64), os = __shfl_xor(s, off, 64);
    float oacc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) oacc[e] = __shfl_xor(acc[e], off, 64);
    as_meet<E>(m, s, acc, om, os, oacc);
  }
  if (ks == 0) {
    if (l == 0) { red[wave][D] = m; red[wave][D + 1] = s; }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int i = 0; i < N; ++i) red[wave][(g * LPK + l) * N + i] = acc[g * N + i];
  }
  __syncthreads();
  // the waves meet in wave order
  float M = NEG_INF;
#pragma unroll
  for (int w = 0; w < AS_WAVES; ++w) M = fmaxf(M, red[w][D]);
  float fw[AS_WAVES], S = 0.f;
#pragma unroll
  for (int w = 0; w < AS_WAVES; ++w) {
    fw[w] = red[w][D] == NEG_INF ? 0.f : expf(red[w][D] - M);
    S += red[w][D + 1] * fw[w];
  }
  float* part = a.workspace ? (float*)a.workspace + (((long)b * a.H + h) * nsplit + split) * (D + 2) : nullptr;
  T* o = (T*)a.o.p + (long)b * a.o.sb + (long)h * a.o.sh;
  for (int c = t; c < D; c += AS_THREADS) {
    float A = 0.f;
#pragma unroll
    for (int w = 0; w < AS_WAVES; ++w) A += red[w][c] * fw[w];
    if (nsplit > 1) part[c] = A;
    else o[c] = from_f32<T>(S > 0.f ? A / S : 0.f);
  }
  if (nsplit > 1 && t == 0) { part[D] = M; part[D + 1] = S; }
}

// grid = (H, B), block = 256: the chunks of a row in chunk order
template <typename T>
__global__ __launch_bounds__(AS_THREADS) void attn_step_combine_kernel(smx_attn_step_args a, int nsplit) {
  const int h = blockIdx.x, b = blockIdx.y, D = a.D;
  const float* part = (const float*)a.workspace + ((long)b * a.H + h) * nsplit * (D + 2);
  float M = NEG_INF;
  for (int p = 0; p < nsplit; ++p) M = fmaxf(M, part[(long)p * (D + 2) + D]);
  float S = 0.f;
  for (int p = 0; p < nsplit; ++p) {
    const float mp = part[(long)p * (D + 2) + D];
    S += mp == NEG_INF ? 0.f : part[(long)p * (D + 2) + D + 1] * expf(mp - M);
  }
  T* o = (T*)a.o.p + (long)b * a.o.sb + (long)h * a.o.sh;
  for (int c = threadIdx.x; c < D; c += AS_THREADS) {
    float A = 0.f;
    for (int p = 0; p < nsplit; ++p) {
      const float mp = part[(long)p * (D + 2) + D];
      A += mp == NEG_INF ? 0.f : part[(long)p * (D + 2) + c] * expf(mp - M);
    }
    o[c] = from_f32<T>(S > 0.f ? A / S : 0.f);
  }
}

// grid = B, block = threads (a multiple of 64 covering D / 8 where it can): a thread owns 8 consecutive columns per trip
template <typename T>
__global__ __launch_bounds__(256) void s2s_embed_step_kernel(const int32_t* __restrict__ tok, const float* __restrict__ table, long ldt,
                                                             const float* __restrict__ pe, long ldpe, T* __restrict__ Y, long ldy,
                                                             int32_t* __restrict__ pos, uint8_t* __restrict__ done, int V, int D,
                                                             int max_pos, float scale) {
  const int b = blockIdx.x;
  const int p = pos[b];
  const int k = tok[b];
  const bool in = k >= 0 && k < V;                      // compared BEFORE the table is indexed
  const bool at = p >= 0 && p < max_pos;                // ... and the position before the positional table
  for (int c = threadIdx.x * 8; c < D; c += blockDim.x * 8) {
    float e0[4] = {0.f, 0.f, 0.f, 0.f}, e1[4] = {0.f, 0.f, 0.f, 0.f}, r0[4] = {0.f, 0.f, 0.f, 0.f}, r1[4] = {0.f, 0.f, 0.f, 0.f};
    if (in) {
      load4<float>(table + (long)k * ldt + c, e0);
      load4<float>(table + (long)k * ldt + c + 4, e1);
    }
    if (at && pe) {
      load4<float>(pe + (long)p * ldpe + c, r0);
      load4<float>(pe + (long)p * ldpe + c + 4, r1);
    }
    float y[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      y[i] = fmaf(e0[i], scale, r0[i]);
      y[4 + i] = fmaf(e1[i], scale, r1[i]);
    }
    T* yr = Y + (long)b * ldy + c;
    if constexpr (sizeof(T) == 2) {
      Grp16<bf16_t>::store(yr, y);
    } else {
      const float lo[4] = {y[0], y[1], y[2], y[3]}, hi[4] = {y[4], y[5], y[6], y[7]};
      store4<float>(yr, lo);
      store4<float>(yr + 4, hi);
    }
  }
  __syncthreads();                                      // every thread has read pos[b]
  if (threadIdx.x == 0) {
    if (!at) done[b] = 1;                               // the table (and the cache) end here: the row ends, it is not advanced
    else if (done[b] == 0) pos[b] = p + 1;
  }
}

// grid = ceil(B / 4), block = 256: wave w of a block owns row 4 blockIdx.x + w
template <typename T>
__global__ __launch_bounds__(256) void s2s_select_kernel(smx_s2s_select_args a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  if (a.done[b]) return;                                // a finished row changes nothing
  const T* x = (const T*)a.logits + (long)b * a.ldz;
  const int n = a.n_tok[b];
  const double inv_temp = a.inv_temp;
  const int skip = (n < a.min_steps) ? a.eos : -1;      // eos stays out of the arg-max below min_steps
  SelRow r = {NEG_INF, INT_MAX, NEG_INF, 0.f, 0};
  row_scan(x, a.V, lane, [&](const auto& g, int c0) { sel_row_take(r, g, c0, skip, inv_temp); });
  float bv = r.bv;
  int bi = r.bi, nan = r.nan;
  argmax_meet<64>(bv, bi);
  const float m = wave_max(r.m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nan |= __shfl_xor(nan, o, 64);
  const double s = wave_sum_f64(r.m == NEG_INF ? 0.0 : (double)r.s * exp((double)(r.m - m) * inv_temp));
  if (lane != 0) return;
  int k = bi == INT_MAX ? -1 : bi;                      // (no entry is a number: every comparison failed)
  if (a.forced) k = a.forced[b];
  float lp;
  if (nan || m == NEG_INF) lp = __builtin_nanf("");
  else if (k < 0 || k >= a.V) lp = NEG_INF;             // a forced token outside the vocabulary has no probability
  else lp = (float)(((double)to_f32(x[k]) - (double)m) * inv_temp - log(s));
  int cnt = n;
  if (n >= 0 && n < a.cap) {
    a.tokens[(long)b * a.cap + n] = k;
    a.logp_tok[(long)b * a.cap + n] = lp;
    a.score[b] += lp;
    cnt = n + 1;
    a.n_tok[b] = cnt;
  }
  if (k == a.eos || cnt >= a.cap) a.done[b] = 1;
  a.tok[b] = k;
}

static bool as_d_ok(int D) { return D == 64 || D == 128 || D == 256 || D == 512; }

// one (B, H, D) operand or a (B, cap, H, D) cache; `rows` says whether sr is read
static int as_check_op(const char* name, const smx_attn_operand& o, int es, bool needed, bool rows) {
  if (!o.p) return needed ? fail(SMX_EINVAL, "smx_attn_step: %s is NULL", name) : SMX_OK;
  if (o.sd != 1) return fail(SMX_EUNSUPPORTED, "smx_attn_step: %s has stride %lld along D (must be contiguous)", name, (long long)o.sd);
  if (!aligned16(o.p) || (o.sb * es) % 16 || (o.sh * es) % 16 || (rows && (o.sr * es) % 16))
    return fail(SMX_EUNSUPPORTED, "smx_attn_step: %s rows are not 16-byte aligned", name);
  return SMX_OK;
}

// cache_rows: the rows K / V hold (smx_attn_step: B; the indexed entry: ceil(B / kv_div))
static int as_check(const smx_attn_step_args* a, bool need, int cache_rows = 0) {
  SMX_REQUIRE(a, "smx_attn_step: null descriptor");
  SMX_REQUIRE(a->B >= 1 && a->H >= 1 && a->D >= 1 && a->cap >= 1, "smx_attn_step: bad sizes B=%d H=%d D=%d cap=%d", a->B, a->H, a->D, a->cap);
  if (a->dtype != SMX_F32 && a->dtype != SMX_BF16) return fail(SMX_EUNSUPPORTED, "smx_attn_step: dtype %d (F32 or BF16)", a->dtype);
  if (!as_d_ok(a->D)) return fail(SMX_EUNSUPPORTED, "smx_attn_step: head dimension %d (64, 128, 256 or 512)", a->D);
  if (a->cap > AS_MAX_CAP) return fail(SMX_EUNSUPPORTED, "smx_attn_step: cap %d exceeds %d keys", a->cap, AS_MAX_CAP);
  if (a->B > 65535 || a->H > 65535) return fail(SMX_EUNSUPPORTED, "smx_attn_step: B %d, H %d exceed the grid", a->B, a->H);
  const int es = a->dtype == SMX_BF16 ? 2 : 4;
  int rc;
  if ((rc = as_check_op("q", a->q, es, need, false))) return rc;
  if ((rc = as_check_op("K", a->K, es, need, true))) return rc;
  if ((rc = as_check_op("V", a->V, es, need, true))) return rc;
  if ((rc = as_check_op("o", a->o, es, need, false))) return rc;
  if ((rc = as_check_op("k_new", a->k_new, es, false, false))) return rc;
  if ((rc = as_check_op("v_new", a->v_new, es, false, false))) return rc;
  SMX_REQUIRE((a->k_new.p == nullptr) == (a->v_new.p == nullptr), "smx_attn_step: k_new and v_new come together");
  if (need) {
    SMX_REQUIRE((cache_rows ? cache_rows : a->B) == 1 || (a->K.sb >= (int64_t)a->D && a->V.sb >= (int64_t)a->D),
                "smx_attn_step: cache batch stride smaller than a row");
    SMX_REQUIRE(a->cap == 1 || (a->K.sr >= a->D && a->V.sr >= a->D), "smx_attn_step: cache row stride smaller than a row");
    SMX_REQUIRE(as_nsplit(a->cap) == 1 || a->workspace, "smx_attn_step: workspace is NULL (smx_attn_step_plan_query: workspace_bytes)");
    if (a->workspace && !aligned16(a->workspace)) return fail(SMX_EUNSUPPORTED, "smx_attn_step: workspace is not 16-byte aligned");
  }
  return SMX_OK;
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

static int as_plan(const smx_attn_step_args* a, smx_attn_step_plan* plan) {
  const int n16 = a->dtype == SMX_BF16 ? 8 : 4;
  memset(plan, 0, sizeof(*plan));
  plan->lanes_per_key = a->D / n16 < 64 ? a->D / n16 : 64;
  plan->keys_per_wave = 64 / plan->lanes_per_key;
  plan->waves = AS_WAVES;
  plan->threads = AS_THREADS;
  plan->splits = as_nsplit(a->cap);
  plan->chunk = as_chunk(a->cap);
  plan->launches = plan->splits > 1 ? 2 : 1;
  plan->lds_bytes = AS_WAVES * (a->D + 2) * 4;
  plan->grid[0] = plan->splits;
  plan->grid[1] = a->H;
  plan->grid[2] = a->B;
  plan->workspace_bytes = plan->splits > 1 ? (int64_t)a->B * a->H * plan->splits * (a->D + 2) * 4 : 0;
  return SMX_OK;
}

template <bool ROWS>
static void as_launch(const smx_attn_step_args* a, const AsRows& x, hipStream_t st) {
  const int nsplit = as_nsplit(a->cap), chunk = as_chunk(a->cap);
  smx_attn_step_args k = *a;
  if (nsplit == 1) k.workspace = nullptr;
  const dim3 grid(nsplit, a->H, a->B);
  dispatch_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    switch (a->D) {
      case 64: hipLaunchKernelGGL((attn_step_kernel<T, 64, ROWS>), grid, dim3(AS_THREADS), 0, st, k, x, nsplit, chunk); break;
      case 128: hipLaunchKernelGGL((attn_step_kernel<T, 128, ROWS>), grid, dim3(AS_THREADS), 0, st, k, x, nsplit, chunk); break;
      case 256: hipLaunchKernelGGL((attn_step_kernel<T, 256, ROWS>), grid, dim3(AS_THREADS), 0, st, k, x, nsplit, chunk); break;
      default: hipLaunchKernelGGL((attn_step_kernel<T, 512, ROWS>), grid, dim3(AS_THREADS), 0, st, k, x, nsplit, chunk); break;
    }
    if (nsplit > 1) hipLaunchKernelGGL(attn_step_combine_kernel<T>, dim3(a->H, a->B), dim3(AS_THREADS), 0, st, k, nsplit);
  });
}

// what the indexed entry adds to as_check: -> the kernel's AsRows
static int as_check_rows(const smx_attn_step_rows_args* r, bool need, AsRows* x) {
  SMX_REQUIRE(r, "smx_attn_step_rows: null descriptor");
  SMX_REQUIRE(r->kv_div >= 1, "smx_attn_step_rows: kv_div %d (must be >= 1)", r->kv_div);
  const int rc = as_check(&r->s, need, r->s.B >= 1 ? (r->s.B + r->kv_div - 1) / r->kv_div : 0);
  if (rc) return rc;
  SMX_REQUIRE(r->kv_div == 1 || !r->anc, "smx_attn_step_rows: anc and kv_div %d do not combine (anc names cache rows itself)", r->kv_div);
  SMX_REQUIRE(r->kv_div == 1 || !r->s.k_new.p, "smx_attn_step_rows: k_new / v_new with kv_div %d (the rows of a cache row would store into one slot)", r->kv_div);
  SMX_REQUIRE(!r->anc || r->ld_anc >= r->s.cap, "smx_attn_step_rows: ld_anc %lld smaller than cap %d", (long long)r->ld_anc, r->s.cap);
  x->anc = r->anc; x->ld_anc = (long)r->ld_anc; x->kv_div = r->kv_div;
  x->rows = (r->s.B + r->kv_div - 1) / r->kv_div;
  return SMX_OK;
}

extern "C" int smx_attn_step_plan_query(const smx_attn_step_args* a, smx_attn_step_plan* plan) {
  SMX_REQUIRE(plan, "smx_attn_step_plan_query: plan is NULL");
  const int rc = as_check(a, false);
  return rc ? rc : as_plan(a, plan);
}

extern "C" int smx_attn_step_rows_plan_query(const smx_attn_step_rows_args* r, smx_attn_step_plan* plan) {
  SMX_REQUIRE(plan, "smx_attn_step_rows_plan_query: plan is NULL");
  AsRows x;
  const int rc = as_check_rows(r, false, &x);
  return rc ? rc : as_plan(&r->s, plan);
}

extern "C" int smx_attn_step_rows(const smx_attn_step_rows_args* r, void* stream) {
  AsRows x;
  const int rc = as_check_rows(r, true, &x);
  if (rc) return rc;
  as_launch<true>(&r->s, x, STREAM);
  return check_launch("smx_attn_step_rows");
}

extern "C" int smx_attn_step(const smx_attn_step_args* a, void* stream) {
  const int rc = as_check(a, true);
  if (rc) return rc;
  as_launch<false>(a, AsRows{nullptr, 0, 1, a->B}, STREAM);
  return check_launch("smx_attn_step");
}

extern "C" int smx_s2s_embed_step(int out_dtype, const int32_t* tok, const float* table, int64_t ldt, const float* pe, int64_t ldpe,
                                  void* Y, int64_t ldy, int32_t* pos, uint8_t* done, int B, int V, int D, int max_pos, void* stream) {
  SMX_REQUIRE(out_dtype == SMX_F32 || out_dtype == SMX_BF16, "smx_s2s_embed_step: bad output dtype %d", out_dtype);
  SMX_REQUIRE(tok && table && Y && pos && done, "smx_s2s_embed_step: null pointer");
  SMX_REQUIRE(B >= 1 && V >= 1 && D >= 1 && max_pos >= 1 && ldt >= D && ldy >= D && (!pe || ldpe >= D),
              "smx_s2s_embed_step: bad sizes B=%d V=%d D=%d max_pos=%d ldt=%lld ldpe=%lld ldy=%lld", B, V, D, max_pos, (long long)ldt,
              (long long)ldpe, (long long)ldy);
  if (D % 8 != 0 || ldt % 8 != 0 || (pe && ldpe % 8 != 0) || ldy % 8 != 0 || !aligned16(table) || !aligned16(pe) || !aligned16(Y))
    return fail(SMX_EUNSUPPORTED, "smx_s2s_embed_step: d and the leading dimensions must be multiples of 8 elements, the bases 16-byte aligned (d=%d)", D);
  const int need = (D / 8 + 63) / 64 * 64;
  const int threads = need < 256 ? need : 256;
  const float scale = sqrtf((float)D);
  dispatch_dtype(out_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(s2s_embed_step_kernel<T>, dim3(B), dim3(threads), 0, STREAM, tok, table, (long)ldt, pe, (long)ldpe, (T*)Y, (long)ldy,
                       pos, done, V, D, max_pos, scale);
  });
  return check_launch("smx_s2s_embed_step");
}

extern "C" int smx_s2s_select(const smx_s2s_select_args* a, void* stream) {
  SMX_REQUIRE(a, "smx_s2s_select: null descriptor");
  SMX_REQUIRE(a->dtype == SMX_F32 || a->dtype == SMX_BF16, "smx_s2s_select: dtype %d", a->dtype);
  SMX_REQUIRE(a->B >= 1 && a->V >= 1 && a->cap >= 1 && a->ldz >= a->V, "smx_s2s_select: bad sizes B=%d V=%d cap=%d ldz=%lld", a->B, a->V,
              a->cap, (long long)a->ldz);
  SMX_REQUIRE(a->inv_temp > 0.0 && a->inv_temp < __builtin_inf(), "smx_s2s_select: the inverse temperature must be positive and finite");
  SMX_REQUIRE(a->logits && a->tok && a->done && a->n_tok && a->score && a->tokens && a->logp_tok, "smx_s2s_select: null pointer");
  const dim3 grid((unsigned)((a->B + 3) / 4));
  dispatch_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(s2s_select_kernel<T>, grid, dim3(256), 0, STREAM, *a);
  });
  return check_launch("smx_s2s_select");
}
