// rowwise.hip — HBM-bound row-wise kernels of the SummaryMixing path (gfx950, wave64):
//   masked mean over time (split-T, fixed-order combine) + broadcast backward, DynChunk window mean,
//   activation/mask backward with fused bias / per-utterance column sums,
//   axpby, casts, fused AdamW, sum of squares, clip factor.
// Every kernel moves 8-16 bytes per lane per access along the feature dim (coalesced 512 B - 1 KiB per
// wave instruction) and accumulates in fp32.
#include <stdlib.h>

#include "smx_common.h"

namespace smx {

template <typename T> struct VT;                       // elements per 16-byte lane access
template <> struct VT<float>  { static constexpr int N = 4; };
template <> struct VT<bf16_t> { static constexpr int N = 8; };

template <typename T, bool VEC>
__device__ __forceinline__ void loadv(const T* p, int nvalid, float (&f)[VT<T>::N]) {
  constexpr int N = VT<T>::N;
  if constexpr (VEC) {
    // whole aligned vectors only (host-checked): callers never issue this for an out-of-range column block
    if constexpr (sizeof(T) == 2) {
      uint4 r = *reinterpret_cast<const uint4*>(p);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) { f[2 * i] = bf16_bits_to_f32(w[i] & 0xffffu); f[2 * i + 1] = bf16_bits_to_f32(w[i] >> 16); }
    } else {
      float4 r = *reinterpret_cast<const float4*>(p);
      f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) f[i] = (i < nvalid) ? to_f32(p[i]) : 0.f;
  }
}
template <typename T, bool VEC>
__device__ __forceinline__ void storev(T* p, int nvalid, const float (&f)[VT<T>::N]) {
  constexpr int N = VT<T>::N;
  if (VEC && nvalid >= N) {
    if constexpr (sizeof(T) == 2) {
      uint4 r;
      r.x = pack_bf16x2(f[0], f[1]);
      r.y = pack_bf16x2(f[2], f[3]);
      r.z = pack_bf16x2(f[4], f[5]);
      r.w = pack_bf16x2(f[6], f[7]);
      *reinterpret_cast<uint4*>(p) = r;
    } else {
      *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < nvalid) p[i] = from_f32<T>(f[i]);
  }
}

static inline bool vec_ok(const void* p, int64_t ld, int D, int n, size_t es) {
  return p == nullptr || (aligned16(p) && ld % n == 0 && D % n == 0 && (ld * es) % 16 == 0);
}

// =================================================================================================
// masked mean over time.  stage 1: grid (DC, TS, B); 4 waves of a block interleave over the rows of the
// block's time range; each lane owns VT<T>::N consecutive features (16-byte loads, 4 rows in flight).
// =================================================================================================
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void masked_sum_stage1(const T* S, long lds, const uint8_t* mask, float* partial,
                                                         float* pcount, int T_, int D, int TR, int TS) {
  constexpr int N = VT<T>::N;
  __shared__ float red[3][64 * N];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.z, ts = blockIdx.y;
  const int col = (blockIdx.x * 64 + lane) * N;
  const int nvalid = D - col;
  const int t0 = ts * TR, t1 = min(T_, t0 + TR);
  float acc[N];
  float cnt = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.f;
  const T* base = S + ((long)b * T_) * lds + (nvalid > 0 ? col : 0);   // idle lanes re-read column 0 (discarded)
  const uint8_t* mrow = mask ? mask + (long)b * T_ : nullptr;
  // every pass keeps 8 independent 16-byte loads in flight per lane (128 B/lane, 8 KiB/wave); rows past the end of
  // the block's range re-read its last row with weight 0, so there is no scalar tail
  const int tlast = t1 - 1;
  for (int t = t0 + w; t < t1; t += 32) {
    float f[8][N], m[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) loadv<T, VEC>(base + (long)min(t + 4 * u, tlast) * lds, nvalid, f[u]);
    {
      const int tt = t + 4 * (lane & 7);                 // lane u (0..7) fetches the mask byte of row slot u
      const float mv = tt < t1 ? (mrow ? (mrow[tt] ? 1.f : 0.f) : 1.f) : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) { m[u] = __shfl(mv, u, 64); cnt += m[u]; }
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
      acc[i] += ((f[0][i] * m[0] + f[1][i] * m[1]) + (f[2][i] * m[2] + f[3][i] * m[3])) +
                ((f[4][i] * m[4] + f[5][i] * m[5]) + (f[6][i] * m[6] + f[7][i] * m[7]));
  }
  __shared__ float cred[4];
  if (lane == 0) cred[w] = cnt;
  if (w > 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[w - 1][lane * N + i] = acc[i];
  }
  __syncthreads();
  if (w == 0 && nvalid > 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = ((acc[i] + red[0][lane * N + i]) + red[1][lane * N + i]) + red[2][lane * N + i];
    float* o = partial + ((long)b * TS + ts) * D + col;
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < nvalid) o[i] = acc[i];
  }
  if (threadIdx.x == 0 && blockIdx.x == 0) pcount[(long)b * TS + ts] = (cred[0] + cred[1]) + (cred[2] + cred[3]);
}

// stage 2: fixed-order sum of the TS partials, divide by the number of valid frames.  grid (ceil(D/256), B)
__global__ __launch_bounds__(256) void masked_sum_stage2(const float* partial, const float* pcount, float* out,
                                                         float* inv_count, int T_, int D, int TS, int scale) {
  const int b = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
  float c = 0.f;
  for (int ts = 0; ts < TS; ++ts) c += pcount[(long)b * TS + ts];   // every thread sums the same TS counts (L1 hits)
  const float inv = 1.f / c;   // zero valid frames -> inf, 0*inf = NaN, as the reference (summary_mixing.py:264-266)
  if (inv_count && blockIdx.x == 0 && threadIdx.x == 0) inv_count[b] = inv;
  if (col >= D) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int ts = 0;
  for (; ts + 3 < TS; ts += 4) {
    s0 += partial[((long)b * TS + ts) * D + col]; s1 += partial[((long)b * TS + ts + 1) * D + col];
    s2 += partial[((long)b * TS + ts + 2) * D + col]; s3 += partial[((long)b * TS + ts + 3) * D + col];
  }
  for (; ts < TS; ++ts) s0 += partial[((long)b * TS + ts) * D + col];
  const float s = (s0 + s1) + (s2 + s3);
  out[(long)b * D + col] = scale ? s * inv : s;
}

static void mm_plan(int B, int T, int D, int nvec, int& DC, int& TS, int& TR) {
  DC = (D + 64 * nvec - 1) / (64 * nvec);
  const long target = 512;                                 // workgroup target (swept 256 / 512 / 1024 / 2048: +-0.1 % of a step)
  long want = (target + (long)B * DC - 1) / ((long)B * DC);   // ~1024 workgroups (4 per CU) when the rows allow it
  long maxts = (T + 127) / 128;                             // >= 128 rows per block (32 per wave)
  TS = (int)(want < 1 ? 1 : (want > maxts ? maxts : want));
  if (TS < 1) TS = 1;
  TR = (T + TS - 1) / TS;
  TS = (T + TR - 1) / TR;
  if (TS < 1) TS = 1;
}

// dS[b,t,:] = g[b,:] * inv_count[b]   (broadcast over t).  grid (DC, ceil(T/RPB), B)
// Optional fusions: the dropout of the merge input (forward `repeat`), or - in the backward - the activation / mask
// backward of the projection that produced the summary columns: dS = g * inv * act'(Z[b,t,:]) * mask[b,t], so that the
// broadcast gradient is never written and re-read by a separate act_mask_bwd pass.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void bcast_rows_kernel(const float* g, const float* inv_count, T* dS, long ldds,
                                                         int T_, int D, int RPB, uint32_t dthresh, float dscale,
                                                         uint64_t dseed_, const uint64_t* ep, const T* __restrict__ Z, long ldz,
                                                         const uint8_t* __restrict__ mask, int act, int LPR) {
  const uint64_t dseed = dthresh ? epoch_seed(dseed_, ep) : 0;
  constexpr int N = VT<T>::N;
  // LPR lanes cover the columns of a row (a power of two <= 64): for narrow rows (D = 256 in bf16: 32 lanes) a wave
  // writes 64 / LPR rows per pass instead of leaving half its lanes idle
  const int lane = threadIdx.x & 63, b = blockIdx.z;
  const int RPW = 64 / LPR, w = (threadIdx.x >> 6) * RPW + lane / LPR, WS = 4 * RPW;
  const int col = (blockIdx.x * LPR + (lane & (LPR - 1))) * N;
  const int nvalid = D - col;
  if (nvalid <= 0) return;
  float v[N];
  const float sc = inv_count ? inv_count[b] : 1.f;
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = (i < nvalid) ? g[(long)b * D + col + i] * sc : 0.f;
  const int t0 = blockIdx.y * RPB, t1 = min(T_, t0 + RPB);
  if (Z || mask) {                                       // backward through act(.) * mask of the producing projection
    dispatch_act(Z ? act : SMX_ACT_NONE, [&](auto act_tag) {
      constexpr int ACT = decltype(act_tag)::value;
      for (int t = t0 + w; t < t1; t += WS) {
        const long n = (long)b * T_ + t;
        const float mk = mask ? (mask[n] ? 1.f : 0.f) : 1.f;
        float o[N];
        if (ACT != SMX_ACT_NONE) {
          float z[N];
          loadv<T, VEC>(Z + n * ldz + col, nvalid, z);
#pragma unroll
          for (int i = 0; i < N; ++i) o[i] = v[i] * mk * act_grad_c<ACT>(z[i]);
        } else {
#pragma unroll
          for (int i = 0; i < N; ++i) o[i] = v[i] * mk;
        }
        storev<T, VEC>(dS + n * ldds + col, nvalid, o);
      }
    });
  } else if (dthresh == 0) {
    for (int t = t0 + w; t < t1; t += WS) storev<T, VEC>(dS + ((long)b * T_ + t) * ldds + col, nvalid, v);
  } else {                                               // fused inverted dropout, mask = f(seed, row * D + col)
    for (int t = t0 + w; t < t1; t += WS) {
      const uint64_t base = ((uint64_t)b * T_ + t) * (uint64_t)D + col;
      float o[N];
#pragma unroll
      for (int i = 0; i < N; ++i) o[i] = v[i];
      dropout_apply_any<N>(o, dseed, base, dthresh, dscale);
      storev<T, VEC>(dS + ((long)b * T_ + t) * ldds + col, nvalid, o);
    }
  }
}

// =================================================================================================
// DynChunk window mean (O(T)).  chunk sums -> window combine.
// =================================================================================================
// csum[b,c,:] = scale_c * sum_{t in chunk c} X[b,t,:]   (scale_c = 1 or 1/wlen(c)).  grid (DC, NC, B)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void chunk_sum_kernel(const T* X, long ldx, float* csum, int T_, int D, int chunk,
                                                        int NC, int left, int scale_by_wlen, int c_off) {
  constexpr int N = VT<T>::N;
  __shared__ float red[3][64 * N];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.z, c = blockIdx.y;
  const int col = (blockIdx.x * 64 + lane) * N;
  const int nvalid = D - col;
  const int t0 = c * chunk, t1 = min(T_, t0 + chunk);
  float acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.f;
  for (int t = t0 + w; t < t1; t += 4) {
    float f[N];
    loadv<T, VEC>(X + ((long)b * T_ + t) * ldx + (nvalid > 0 ? col : 0), nvalid, f);
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] += f[i];
  }
  if (w > 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[w - 1][lane * N + i] = acc[i];
  }
  __syncthreads();
  if (w == 0 && nvalid > 0) {
    float sc = 1.f;
    if (scale_by_wlen) {                                  // (c_off: chunks of earlier sequence-parallel shards in front of this one)
      const int lo = left < 0 ? 0 : max(0, (c + c_off - left) * chunk);
      sc = 1.f / (float)(t1 + c_off * chunk - lo);
    }
    float* o = csum + ((long)b * NC + c) * D + col;
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < nvalid) o[i] = sc * (((acc[i] + red[0][lane * N + i]) + red[1][lane * N + i]) + red[2][lane * N + i]);
  }
}
// Unlimited left context: the window of chunk c is the whole prefix 0..c (reverse: the suffix c..NC-1), which the window
// kernel used to add up chunk by chunk - a dependent chain of up to NC loads per workgroup (237 us at NC = 32 against ~10 us of
// bytes).  One pass turns csum into its running sums in place instead (thread = one column of one utterance, the NC loads
// are independent and unrolled), and the window kernel reads ONE row.  Fixed order: bit-reproducible.
__global__ __launch_bounds__(256) void chunk_prefix_kernel(float* csum, int D, int NC, int reverse) {
  const int col = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (col >= D) return;
  float* p = csum + (long)b * NC * D + col;
  float acc = 0.f;
  if (!reverse) {
#pragma unroll 8
    for (int c = 0; c < NC; ++c) { acc += p[(long)c * D]; p[(long)c * D] = acc; }
  } else {
#pragma unroll 8
    for (int c = NC - 1; c >= 0; --c) { acc += p[(long)c * D]; p[(long)c * D] = acc; }
  }
}
// fwd: out rows of chunk c = (sum_{c'=lo..c} csum[c']) / wlen(c);  bwd (reverse=1): rows of chunk c =
// sum_{c'=c..hi} csum[c'] (csum already scaled by 1/wlen).  grid (DC, NC, B)
// Sequence-parallel shards (c_off chunks in front of this one; carry): the window sums that reach into other shards arrive as
// `carry` rows - chunk c adds carry[b][c - carry_c0] for carry_c0 <= c < carry_c0 + carry_n (carry_n == 0 with a non-null carry: ONE
// row per utterance for every chunk: the totals of all earlier / later shards with unlimited left context).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void chunk_window_kernel(const float* csum, T* out, long ldo, int T_, int D,
                                                           int chunk, int NC, int left, int reverse, int c_off,
                                                           const float* __restrict__ carry, int carry_c0, int carry_n) {
  constexpr int N = VT<T>::N;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.z, c = blockIdx.y;
  const int col = (blockIdx.x * 64 + lane) * N;
  const int nvalid = D - col;
  if (nvalid <= 0) return;
  int clo, chi;
  if (left < 0) { clo = c; chi = c; }                    // (csum holds running sums already: chunk_prefix_kernel)
  else if (!reverse) { clo = max(0, c - left); chi = c; }
  else { clo = c; chi = min(NC - 1, c + left); }
  float acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.f;
  for (int cc = clo; cc <= chi; ++cc) {
    const float* p = csum + ((long)b * NC + cc) * D + col;
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < nvalid) acc[i] += p[i];
  }
  if (carry) {
    const float* cp = nullptr;
    if (carry_n == 0) cp = carry + (long)b * D + col;
    else if (c >= carry_c0 && c < carry_c0 + carry_n) cp = carry + ((long)b * carry_n + (c - carry_c0)) * D + col;
    if (cp) {
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (i < nvalid) acc[i] += cp[i];
    }
  }
  const int t0 = c * chunk, t1 = min(T_, t0 + chunk);
  if (!reverse) {
    const int lo = left < 0 ? 0 : max(0, (c + c_off - left) * chunk);
    float sc = 1.f / (float)(t1 + c_off * chunk - lo);
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] *= sc;
  }
  for (int t = t0 + w; t < t1; t += 4) storev<T, VEC>(out + ((long)b * T_ + t) * ldo + col, nvalid, acc);
}

// =================================================================================================
// SummaryMixing-expdecay in O(T).  The reference builds the (T,T) Laplace matrix
// M_ij = gamma^|i-j| (summary_mixing.py:316-365) and evaluates (M s) / rowsum(M) (:233-235): O(T^2).  M s is a two-sided
// exponential filter:  f_t = s_t + gamma f_{t-1},  g_t = s_t + gamma g_{t+1},  (M s)_t = f_t + g_t - s_t,  and
// rowsum(M)_t = (2 - gamma^(t+1) - gamma^(T-t)) / (1 - gamma) - 1 in closed form (the denominator ignores padding like
// the reference's).  Chunked scan over T: (1) per 16-row chunk the local end values of both recurrences, (2) carries
// across the chunks (a short sequential loop per column), (3) per chunk both local scans out of registers + carries.
// mode 0 (forward):  out = (M s) / rowsum(M);   mode 1 (backward, M symmetric): out = M (s / rowsum(M)).
// =================================================================================================
constexpr int ED_CH = 16;                                // rows per chunk

// 1 - gamma^n is formed as -expm1f(n ln gamma): 2 - gamma^(t+1) - gamma^(T-t) loses every digit the powers share with 1 (at the
// recipe's gamma = 0.995 and T = 1 the denominator came out 3.6e-5 off, 1.5e-5 at T = 2, 8.8e-6 at T = 3 - the first frames of a short
// utterance or streaming chunk).  lng = ln gamma comes from the host (rounded once from double): the relative error of the small
// differences is that of lng, and the device's fast logf is only absolutely accurate near 1.
__device__ __forceinline__ float ed_inv_den(int t, int T_, float lng, float inv1mg) {
  const float den = (-expm1f((float)(t + 1) * lng) - expm1f((float)(T_ - t) * lng)) * inv1mg - 1.f;
  return 1.f / den;
}

// grid (DC, ceil(NC/4), B); a wave owns one chunk; lane owns 4 columns.  ws[b][c][0][D] = F_c, ws[b][c][1][D] = G_c
template <typename T>
__global__ __launch_bounds__(256) void expdecay_chunk_kernel(const T* __restrict__ X, long ldx, float* __restrict__ ws,
                                                             int T_, int D, int NC, float gamma, float lng, int mode, int t_off, int T_glob) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.z;
  const int c = blockIdx.y * 4 + w, col = (blockIdx.x * 64 + lane) * 4;
  if (c >= NC || col >= D) return;
  const float inv1mg = 1.f / (1.f - gamma);
  const int t0 = c * ED_CH;
  float F[4] = {0.f, 0.f, 0.f, 0.f}, G[4] = {0.f, 0.f, 0.f, 0.f};
  float v[ED_CH][4];
#pragma unroll
  for (int i = 0; i < ED_CH; ++i) {
    const int t = t0 + i;
    if (t < T_) load4<T>(X + ((long)b * T_ + t) * ldx + col, v[i]);
    else v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f;
  }
  float pw = 1.f;
#pragma unroll
  for (int i = 0; i < ED_CH; ++i) {
    const int t = t0 + i;
    const float sc = (mode == 1 && t < T_) ? ed_inv_den(t + t_off, T_glob, lng, inv1mg) : 1.f;   // (t_off / T_glob: a sequence-parallel shard)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float x = v[i][q] * sc;
      F[q] = x + gamma * F[q];                           // = sum_t gamma^(last - t) x_t  (rows past T count as zeros)
      G[q] += pw * x;                                    // = sum_t gamma^(t - first) x_t
    }
    pw *= gamma;
  }
  float* o = ws + (((long)b * NC + c) * 2) * D + col;
  *reinterpret_cast<float4*>(o) = make_float4(F[0], F[1], F[2], F[3]);
  *reinterpret_cast<float4*>(o + D) = make_float4(G[0], G[1], G[2], G[3]);
}

// in place: ws[b][c][0] <- f entering chunk c from the left, ws[b][c][1] <- g entering chunk c from the right.
// One thread per (b, column); the chunk values are independent of the recurrence, so 8 are fetched ahead.
// f_in / g_in (B, D; sequence-parallel shards): the states entering the shard from its left / right neighbours, else zero.
// ends (2, B, D; optional, then NOTHING is written to ws): the states LEAVING the shard - f at its last frame, g at its first -
// with zero entering states: what the shards exchange before the second call.
__global__ __launch_bounds__(256) void expdecay_carry_kernel(float* __restrict__ ws, int D, int NC, int B, float gamma,
                                                             const float* __restrict__ f_in, const float* __restrict__ g_in,
                                                             float* __restrict__ ends, int T_) {
  const long idx = blockIdx.x * 256L + threadIdx.x;
  if (idx >= (long)B * D) return;
  const int b = (int)(idx / D), col = (int)(idx % D);
  float* base = ws + (long)b * NC * 2 * D + col;
  const float gch = expf((float)ED_CH * logf(gamma));    // every chunk is ED_CH rows long (the tail is zero padded)
  // both directions advance in the same loop (two independent chains), 16 chunk values of each fetched ahead
  float cf = f_in ? f_in[idx] : 0.f, cg = g_in ? g_in[idx] : 0.f;
  // The last chunk is zero padded to ED_CH rows.  g_in is g at the frame after the shard's LAST one, but it seeds the scan at the end of
  // the padded chunk: the carry step (gch) and the descending scan of expdecay_apply_kernel then decay it through the pad rows as well.
  // Scale it up by gamma^-pad first (the mirror of `ends` below; pad < 16, finite in float32 for gamma >= ~0.01).  pad == 0 and the
  // unsharded call (g_in == nullptr) are untouched.
  const int pad = NC * ED_CH - T_;
  if (g_in && pad > 0) cg *= expf(-(float)pad * logf(gamma));
  for (int c0 = 0; c0 < NC; c0 += 16) {
    float f[16], g[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int c = c0 + u;
      f[u] = c < NC ? base[(long)c * 2 * D] : 0.f;
      g[u] = c < NC ? base[(long)(NC - 1 - c) * 2 * D + D] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int c = c0 + u;
      if (c < NC) {
        if (!ends) base[(long)c * 2 * D] = cf;
        cf = f[u] + gch * cf;
        if (!ends) base[(long)(NC - 1 - c) * 2 * D + D] = cg;
        cg = g[u] + gch * cg;
      }
    }
  }
  if (ends) {
    // the padded last chunk's end value is gamma^pad times f at the shard's last frame
    ends[idx] = cf * expf(-(float)pad * logf(gamma));
    ends[(long)B * D + idx] = cg;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void expdecay_apply_kernel(const T* __restrict__ X, long ldx, const float* __restrict__ ws,
                                                             T* __restrict__ Y, long ldy, int T_, int D, int NC, float gamma,
                                                             float lng, int mode, int t_off, int T_glob) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.z;
  const int c = blockIdx.y * 4 + w, col = (blockIdx.x * 64 + lane) * 4;
  if (c >= NC || col >= D) return;
  const float inv1mg = 1.f / (1.f - gamma);
  const int t0 = c * ED_CH;
  float v[ED_CH][4], a[ED_CH][4];
#pragma unroll
  for (int i = 0; i < ED_CH; ++i) {
    const int t = t0 + i;
    if (t < T_) load4<T>(X + ((long)b * T_ + t) * ldx + col, v[i]);
    else v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f;
  }
  const float* cw = ws + (((long)b * NC + c) * 2) * D + col;
  const float4 cf4 = *reinterpret_cast<const float4*>(cw), cg4 = *reinterpret_cast<const float4*>(cw + D);
  float f[4] = {cf4.x, cf4.y, cf4.z, cf4.w}, g[4] = {cg4.x, cg4.y, cg4.z, cg4.w};
#pragma unroll
  for (int i = 0; i < ED_CH; ++i) {                      // ascending: a_t = gamma f_{t-1}  (= f_t - x_t)
    const int t = t0 + i;
    const float sc = (mode == 1 && t < T_) ? ed_inv_den(t + t_off, T_glob, lng, inv1mg) : 1.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[i][q] *= sc;
      a[i][q] = gamma * f[q];
      f[q] = v[i][q] + a[i][q];
    }
  }
#pragma unroll
  for (int i = ED_CH - 1; i >= 0; --i) {                 // descending: g_t = x_t + gamma g_{t+1};  out = a_t + g_t
    const int t = t0 + i;
    float o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      g[q] = v[i][q] + gamma * g[q];
      o[q] = a[i][q] + g[q];
    }
    if (t < T_) {
      if (mode == 0) {
        const float sc = ed_inv_den(t + t_off, T_glob, lng, inv1mg);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] *= sc;
      }
      store4<T>(Y + ((long)b * T_ + t) * ldy + col, o);
    }
  }
}

// =================================================================================================
// dZ = alpha * dY * mask * act'(Z);  dbias[m] += colsum;  dgroup[n/div, m] += per-group colsum.
// VEC kernel: a lane owns VT<T>::N consecutive columns (16-byte accesses); LPR lanes span a row chunk of up to
// 64*N columns, the remaining 64/LPR lanes of a wave take further rows; 4 rows are in flight per lane.
// =================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void act_mask_bwd_vec_kernel(const T* __restrict__ dY, long lddy, const T* __restrict__ Z,
                                                               long ldz, const uint8_t* __restrict__ mask, T* __restrict__ dZ,
                                                               long lddz, int N_, int M, int act, float alpha, float* dbias,
                                                               float* dgroup, long lddg, int gdiv, int RS, int LPR,
                                                               float* __restrict__ partial, uint32_t dthresh, float dscale,
                                                               uint64_t dseed_, const uint64_t* ep) {
  constexpr int N = VT<T>::N;
  const uint64_t dseed = dthresh ? epoch_seed(dseed_, ep) : 0;
  __shared__ float red[256][N];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lc = lane % LPR, lr = lane / LPR;          // column chunk / row slot inside the wave
  const int RPW = 64 / LPR;                            // rows per wave instruction
  const int col = (blockIdx.x * LPR + lc) * N;
  const bool cok = col < M;
  const int colc = cok ? col : 0;
  float bsum[N], gsum[N];
#pragma unroll
  for (int q = 0; q < N; ++q) bsum[q] = gsum[q] = 0.f;
  int cur_g = -1;
  const int rstep = 4 * RPW;                           // rows advanced per pass of the block's 4 waves
  dispatch_act(Z ? act : SMX_ACT_NONE, [&](auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;
    // a workgroup strides over row strips: gridDim.y (<= ACT_BWD_YMAX) partial rows for the bias reduction however long N is
    for (int r0 = blockIdx.y * RS; r0 < N_; r0 += gridDim.y * RS) {
    const int r1 = min(N_, r0 + RS);
    for (int nb = r0 + w * RPW + lr; nb < r1; nb += 4 * rstep) {
      float fdy[4][N], fz[4][N];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = min(nb + u * rstep, N_ - 1);
        loadv<T, true>(dY + (long)n * lddy + colc, N, fdy[u]);
        if (ACT != SMX_ACT_NONE) loadv<T, true>(Z + (long)n * ldz + colc, N, fz[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = nb + u * rstep;
        if (n >= r1 || !cok) continue;
        const float mk = (mask ? (mask[n] ? 1.f : 0.f) : 1.f) * alpha;
        float o[N];
#pragma unroll
        for (int q = 0; q < N; ++q) o[q] = fdy[u][q] * mk * (ACT != SMX_ACT_NONE ? act_grad_c<ACT>(fz[u][q]) : 1.f);
        if (dthresh) dropout_apply_any<N>(o, dseed, (uint64_t)n * M + col, dthresh, dscale);
        if (dZ) storev<T, true>(dZ + (long)n * lddz + col, N, o);
#pragma unroll
        for (int q = 0; q < N; ++q) bsum[q] += o[q];
        if (dgroup) {
          const int g = n / gdiv;
          if (g != cur_g) {
            if (cur_g >= 0) { for (int q = 0; q < N; ++q) atomicAdd(dgroup + (long)cur_g * lddg + col + q, gsum[q]); }
            cur_g = g;
#pragma unroll
            for (int q = 0; q < N; ++q) gsum[q] = 0.f;
          }
#pragma unroll
          for (int q = 0; q < N; ++q) gsum[q] += o[q];
        }
      }
    }
    }
  });
  if (dgroup && cur_g >= 0 && cok) { for (int q = 0; q < N; ++q) atomicAdd(dgroup + (long)cur_g * lddg + col + q, gsum[q]); }
  if (dbias) {                                         // fold the 256 threads that share a column chunk
#pragma unroll
    for (int q = 0; q < N; ++q) red[threadIdx.x][q] = bsum[q];
    __syncthreads();
    if (threadIdx.x < LPR && cok) {
      float tot[N];
#pragma unroll
      for (int q = 0; q < N; ++q) tot[q] = 0.f;
      for (int k = threadIdx.x; k < 256; k += LPR) {
#pragma unroll
        for (int q = 0; q < N; ++q) tot[q] += red[k][q];
      }
      // one partial row per row strip (no atomics: ~100 ns each when thousands of blocks hit the same address)
#pragma unroll
      for (int q = 0; q < N; ++q) partial[(long)blockIdx.y * M + col + q] = tot[q];
    }
  }
}

// dst[c] += sum_b partial[b][c]  (fixed order).  block = 32 columns x 8 row groups
__global__ __launch_bounds__(256) void colsum_partials_kernel(const float* __restrict__ partial, int nrows, int W, float* dst) {
  __shared__ float red[16][16];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cx;
  const bool ok = c < W;
  const int col = ok ? c : 0;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int b = ry;
  for (; b + 48 < nrows; b += 64) {
    s0 += partial[(long)b * W + col]; s1 += partial[(long)(b + 16) * W + col];
    s2 += partial[(long)(b + 32) * W + col]; s3 += partial[(long)(b + 48) * W + col];
  }
  for (; b < nrows; b += 16) s0 += partial[(long)b * W + col];
  red[ry][cx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ry == 0 && ok) {
    float tot = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot += red[r][cx];
    dst[col] += tot;
  }
}

void launch_colsum_partials(const float* partial, int nrows, int W, float* dst, hipStream_t stream) {
  hipLaunchKernelGGL(colsum_partials_kernel, dim3((W + 15) / 16), dim3(256), 0, stream, partial, nrows, W, dst);
}

// generic (ragged / unaligned) variant: 4 columns per thread, scalar accesses
template <typename T>
__global__ __launch_bounds__(256) void act_mask_bwd_kernel(const T* dY, long lddy, const T* Z, long ldz,
                                                           const uint8_t* mask, T* dZ, long lddz, int N_, int M, int act,
                                                           float alpha, float* dbias, float* dgroup, long lddg, int gdiv,
                                                           int RS, uint32_t dthresh, float dscale, uint64_t dseed_,
                                                           const uint64_t* ep) {
  const uint64_t dseed = dthresh ? epoch_seed(dseed_, ep) : 0;
  __shared__ float red[3][64][4];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + cx) * 4;
  const int nvalid = M - col;
  const int r0 = blockIdx.y * RS, r1 = min(N_, r0 + RS);
  float bsum[4] = {0.f, 0.f, 0.f, 0.f}, gsum[4] = {0.f, 0.f, 0.f, 0.f};
  int cur_g = -1;
  if (nvalid > 0) {
    for (int n = r0 + ry; n < r1; n += 4) {
      float fdy[4], fz[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
      for (int q = 0; q < 4; ++q) fdy[q] = q < nvalid ? to_f32(dY[(long)n * lddy + col + q]) : 0.f;
      if (Z) { for (int q = 0; q < 4; ++q) fz[q] = q < nvalid ? to_f32(Z[(long)n * ldz + col + q]) : 0.f; }
      const float mk = (mask ? (mask[n] ? 1.f : 0.f) : 1.f) * alpha;
      for (int q = 0; q < 4; ++q) o[q] = fdy[q] * mk * (Z ? act_grad(act, fz[q]) : 1.f);
      if (dthresh) dropout_apply_any<4>(o, dseed, (uint64_t)n * M + col, dthresh, dscale);
      if (dZ) { for (int q = 0; q < 4; ++q) if (q < nvalid) dZ[(long)n * lddz + col + q] = from_f32<T>(o[q]); }
      for (int q = 0; q < 4; ++q) bsum[q] += o[q];
      if (dgroup) {
        int g = n / gdiv;
        if (g != cur_g) {
          if (cur_g >= 0) { for (int q = 0; q < 4; ++q) if (q < nvalid) atomicAdd(dgroup + (long)cur_g * lddg + col + q, gsum[q]); }
          cur_g = g;
          for (int q = 0; q < 4; ++q) gsum[q] = 0.f;
        }
        for (int q = 0; q < 4; ++q) gsum[q] += o[q];
      }
    }
    if (dgroup && cur_g >= 0) { for (int q = 0; q < 4; ++q) if (q < nvalid) atomicAdd(dgroup + (long)cur_g * lddg + col + q, gsum[q]); }
  }
  if (dbias) {
    if (ry > 0) { for (int q = 0; q < 4; ++q) red[ry - 1][cx][q] = bsum[q]; }
    __syncthreads();
    if (ry == 0 && nvalid > 0) {
      for (int q = 0; q < 4; ++q)
        if (q < nvalid) atomicAdd(dbias + col + q, ((bsum[q] + red[0][cx][q]) + red[1][cx][q]) + red[2][cx][q]);
    }
  }
}

// y = a*x + b*y0
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void axpby_kernel(float a, const T* X, long ldx, float b, const T* Y0, long ldy0, T* Y,
                                                    long ldy, int N_, int D) {
  const int cv = (D + 3) / 4;
  long total = (long)N_ * cv;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int n = (int)(i / cv), col = (int)(i % cv) * 4, nvalid = D - col;
    float fx[4], fy[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (VEC && nvalid >= 4) load4<T>(X + (long)n * ldx + col, fx);
    else { for (int q = 0; q < 4; ++q) fx[q] = q < nvalid ? to_f32(X[(long)n * ldx + col + q]) : 0.f; }
    if (Y0) {
      if (VEC && nvalid >= 4) load4<T>(Y0 + (long)n * ldy0 + col, fy);
      else { for (int q = 0; q < 4; ++q) fy[q] = q < nvalid ? to_f32(Y0[(long)n * ldy0 + col + q]) : 0.f; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = a * fx[q] + b * fy[q];
    if (VEC && nvalid >= 4) store4<T>(Y + (long)n * ldy + col, o);
    else { for (int q = 0; q < 4; ++q) if (q < nvalid) Y[(long)n * ldy + col + q] = from_f32<T>(o[q]); }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void cast_from_f32_kernel(const float* src, T* dst, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = from_f32<T>(src[i]);
}
template <typename T>
__global__ __launch_bounds__(256) void cast_to_f32_kernel(const T* src, float* dst, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = to_f32(src[i]);
}

// fused AdamW (torch.optim.AdamW semantics: p *= 1 - lr*wd; m,v EMA; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps))
__global__ __launch_bounds__(256) void adamw_kernel(float* p, const float* g, float* m, float* v, uint16_t* shadow, long n,
                                                    float lr, float b1, float b2, float eps, float wd, float bc1,
                                                    float bc2_sqrt, float gscale, const float* gscale_dev,
                                                    const uint64_t* step_dev, const float* lr_dev) {
  // a clip factor of exactly 0 is smx_clip_factor's "non-finite gradient norm" verdict: skip the whole update
  // (no weight decay, no moment update, shadows untouched) like SpeechBrain's check_gradients does
  if (gscale_dev && gscale_dev[0] == 0.f) return;
  const float gs = gscale * (gscale_dev ? gscale_dev[0] : 1.f);
  if (lr_dev) lr = lr_dev[0];                            // the rate smx_lr_schedule wrote for this update
  if (step_dev) {                                        // bias correction from the device step counter (graph replay)
    const float t = (float)step_dev[0];
    bc1 = 1.f - powf(b1, t);
    bc2_sqrt = sqrtf(1.f - powf(b2, t));
  }
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float gi = g[i] * gs, pi = p[i], mi = m[i], vi = v[i];
    pi *= 1.f - lr * wd;
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    pi -= (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if (shadow) shadow[i] = (uint16_t)f32_to_bf16_bits(pi);
  }
}

// Global gradient norm in a FIXED order (no atomics): per-block partial sums, then one block folds them.  Data-parallel
// ranks hold bit-identical all-reduced gradients; an order-dependent norm would give them clip factors that differ in the
// last bits and let their weights drift apart.
constexpr int SUMSQ_BLOCKS = 1024;
__global__ __launch_bounds__(256) void sumsq_kernel(const float* x, long n, float* partial) {
  __shared__ float red[4];
  float s = 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) s += x[i] * x[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* partial, int np, float* out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < np; i += 256) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] += (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void clip_factor_kernel(const float* sumsq, float max_norm, float inv_scale, float* out) {
  const float ss = sumsq[0];
  if (!(ss >= 0.f && ss < __builtin_inff())) {           // NaN or Inf gradient norm: factor 0 = "skip this step"
    out[0] = 0.f;
    out[1] += 1.f;                                        // skipped-step counter
    return;
  }
  float nrm = sqrtf(ss) * inv_scale;
  float f = max_norm / (nrm + 1e-6f);
  out[0] = f < 1.f ? f : 1.f;
}

template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(const T* X, long ldx, T* Y, long ldy, int N_, int D, uint32_t thresh,
                                                      float scale, uint64_t seed_, const uint64_t* ep) {
  const uint64_t seed = epoch_seed(seed_, ep);
  const int cv = (D + 3) / 4;
  const long total = (long)N_ * cv;
  const bool vec = (D & 3) == 0 && (ldx & 3) == 0 && (ldy & 3) == 0 && ((uintptr_t)X % (4 * sizeof(T))) == 0 &&
                   ((uintptr_t)Y % (4 * sizeof(T))) == 0;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i / cv), col = (int)(i % cv) * 4, nvalid = D - col;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) load4<T>(X + (long)n * ldx + col, f);
    else { for (int q = 0; q < 4; ++q) if (q < nvalid) f[q] = to_f32(X[(long)n * ldx + col + q]); }
    dropout_apply_any<4>(f, seed, (uint64_t)n * D + col, thresh, scale);
    if (vec) store4<T>(Y + (long)n * ldy + col, f);
    else { for (int q = 0; q < 4; ++q) if (q < nvalid) Y[(long)n * ldy + col + q] = from_f32<T>(f[q]); }
  }
}
// Y[n, :] += table[n % R, :]   (fp32 table; the abs-sine positional encoding added after the input dropout)
template <typename T>
__global__ __launch_bounds__(256) void add_rowtable_kernel(T* Y, long ldy, const float* table, int R, int N_, int D) {
  const long total = (long)N_ * D;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i / D), c = (int)(i % D);
    Y[(long)n * ldy + c] = from_f32<T>(to_f32(Y[(long)n * ldy + c]) + table[(long)(n % R) * D + c]);
  }
}

static inline int grid1d(long n) {
  long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" size_t smx_masked_mean_workspace(int B, int T, int D) {
  int DC, TS, TR;
  mm_plan(B, T, D, 4, DC, TS, TR);  // fp32 plan has the most splits; bf16 needs no more
  int DC2, TS2, TR2;
  mm_plan(B, T, D, 8, DC2, TS2, TR2);
  int ts = TS > TS2 ? TS : TS2;
  return (size_t)B * ts * (D + 1) * sizeof(float);
}

extern "C" int smx_masked_mean_fwd(int dtype, const void* S, int64_t lds, const uint8_t* mask, float* out,
                                   float* inv_count, int B, int T, int D, int scale_by_count, void* workspace,
                                   void* stream) {
  SMX_REQUIRE(S && out && workspace, "smx_masked_mean_fwd: null pointer");
  SMX_REQUIRE(B > 0 && T > 0 && D > 0, "smx_masked_mean_fwd: bad sizes");
  const int nvec = dtype == SMX_BF16 ? 8 : 4;
  int DC, TS, TR;
  mm_plan(B, T, D, nvec, DC, TS, TR);
  dim3 g1(DC, TS, B);
  float* partial = reinterpret_cast<float*>(workspace);
  float* pcount = partial + (size_t)B * TS * D;
  const bool vec = vec_ok(S, lds, D, nvec, dtype == SMX_BF16 ? 2 : 4);
  if (dtype == SMX_BF16) {
    if (vec) hipLaunchKernelGGL((masked_sum_stage1<bf16_t, true>), g1, dim3(256), 0, STREAM, (const bf16_t*)S, lds, mask, partial, pcount, T, D, TR, TS);
    else hipLaunchKernelGGL((masked_sum_stage1<bf16_t, false>), g1, dim3(256), 0, STREAM, (const bf16_t*)S, lds, mask, partial, pcount, T, D, TR, TS);
  } else if (dtype == SMX_F32) {
    if (vec) hipLaunchKernelGGL((masked_sum_stage1<float, true>), g1, dim3(256), 0, STREAM, (const float*)S, lds, mask, partial, pcount, T, D, TR, TS);
    else hipLaunchKernelGGL((masked_sum_stage1<float, false>), g1, dim3(256), 0, STREAM, (const float*)S, lds, mask, partial, pcount, T, D, TR, TS);
  } else return fail(SMX_EINVAL, "smx_masked_mean_fwd: bad dtype");
  hipLaunchKernelGGL(masked_sum_stage2, dim3((D + 255) / 256, B), dim3(256), 0, STREAM, partial, pcount, out, inv_count, T, D, TS, scale_by_count);
  return check_launch("smx_masked_mean_fwd");
}

#ifndef SMX_BCAST_RPB
#define SMX_BCAST_RPB 64       // rows per workgroup of the broadcast kernels that also read (act / mask backward)
#endif
#ifndef SMX_BCAST_RPB_ST
#define SMX_BCAST_RPB_ST 128   // ... of the store-only ones (repeat, repeat + dropout)
#endif
static int bcast_impl(int dtype, const float* g, const float* inv_count, void* dS, int64_t ldds, int B, int T, int D,
                      float drop_p, uint64_t drop_seed, const uint64_t* epoch, const void* Z, int64_t ldz, const uint8_t* mask, int act, void* stream,
                      const char* what) {
  const uint32_t dthresh = (uint32_t)((double)drop_p * 4294967296.0);
  const float dscale = 1.f / (1.f - drop_p);
  const int nvec = dtype == SMX_BF16 ? 8 : 4;
  int LPR = 1;
  while (LPR < 64 && LPR * nvec < D) LPR <<= 1;           // lanes per row (power of two)
  const int DC = (D + LPR * nvec - 1) / (LPR * nvec);
  int RPB = (Z || mask) ? SMX_BCAST_RPB : SMX_BCAST_RPB_ST;
  while (RPB > 8 && (long)DC * ((T + RPB - 1) / RPB) * B < 512) RPB >>= 1;   // small batches: more, shorter workgroups (the recipe's 10 x 375 frames ran on 30)
  dim3 grid(DC, (T + RPB - 1) / RPB, B);
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  const bool vec = vec_ok(dS, ldds, D, nvec, es) && (Z == nullptr || vec_ok(Z, ldz, D, nvec, es));
  if (dtype == SMX_BF16) {
    if (vec) hipLaunchKernelGGL((bcast_rows_kernel<bf16_t, true>), grid, dim3(256), 0, STREAM, g, inv_count, (bf16_t*)dS, ldds, T, D, RPB, dthresh, dscale, drop_seed, epoch, (const bf16_t*)Z, ldz, mask, act, LPR);
    else hipLaunchKernelGGL((bcast_rows_kernel<bf16_t, false>), grid, dim3(256), 0, STREAM, g, inv_count, (bf16_t*)dS, ldds, T, D, RPB, dthresh, dscale, drop_seed, epoch, (const bf16_t*)Z, ldz, mask, act, LPR);
  } else {
    if (vec) hipLaunchKernelGGL((bcast_rows_kernel<float, true>), grid, dim3(256), 0, STREAM, g, inv_count, (float*)dS, ldds, T, D, RPB, dthresh, dscale, drop_seed, epoch, (const float*)Z, ldz, mask, act, LPR);
    else hipLaunchKernelGGL((bcast_rows_kernel<float, false>), grid, dim3(256), 0, STREAM, g, inv_count, (float*)dS, ldds, T, D, RPB, dthresh, dscale, drop_seed, epoch, (const float*)Z, ldz, mask, act, LPR);
  }
  return check_launch(what);
}

extern "C" int smx_masked_mean_bwd(int dtype, const float* g, const float* inv_count, void* dS, int64_t ldds, int B,
                                   int T, int D, float drop_p, uint64_t drop_seed, const uint64_t* epoch, void* stream) {
  SMX_REQUIRE(g && dS, "smx_masked_mean_bwd: null pointer");
  SMX_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "smx_masked_mean_bwd: 0 <= drop_p < 1");
  return bcast_impl(dtype, g, inv_count, dS, ldds, B, T, D, drop_p, drop_seed, epoch, nullptr, 0, nullptr, SMX_ACT_NONE, stream,
                    "smx_masked_mean_bwd");
}

extern "C" int smx_masked_mean_bwd_act(int dtype, const float* g, const float* inv_count, void* dS, int64_t ldds,
                                       const void* Z, int64_t ldz, const uint8_t* row_mask, int act, int B, int T, int D,
                                       void* stream) {
  SMX_REQUIRE(g && dS && (Z || row_mask), "smx_masked_mean_bwd_act: null pointer");
  return bcast_impl(dtype, g, inv_count, dS, ldds, B, T, D, 0.f, 0, nullptr, Z, ldz, row_mask, Z ? act : SMX_ACT_NONE, stream,
                    "smx_masked_mean_bwd_act");
}

// =================================================================================================
// Round 6, small batches: the masked mean AND its broadcast in ONE launch.  The per-utterance summary is three launches on the big
// path (split-T partial sums, their fixed-order fold, the broadcast back over t) because 64 000 frames want thousands of
// workgroups; the recipe's 10 x 375 frames or one utterance want neither - every launch of a replayed step costs >= 4.5 us
// whatever it does (profiles/r06_seq_c2a_recipe_batch_v0_baseline.txt: 6.6 + 4.8 + 6.3 us for 3.8 MB in, 3.8 MB out).
// One workgroup owns (utterance b, a group of 8 lanes x VT::N columns): its 32 row slots walk the T frames (4 rows in flight each),
// fold through LDS in a FIXED order (bit-reproducible, no atomics), then the same threads write the broadcast with the options of
// bcast_rows_kernel: inverted dropout (forward `repeat`, summary_mixing.py:222,237-239,267) or the act / mask backward of the
// projection that produced the summary columns (backward of summary_mixing.py:210,257).
// =================================================================================================
// CL lanes x VT::N columns per row and workgroup, RS = 256 / CL row slots (chosen at launch: narrower groups = more workgroups
// and more rows in flight for the 10-utterance recipe batch or a single utterance - the first version, 8 lanes and 4 rows in flight
// on 80 workgroups, took 10-15 us: three dependent round trips per slot).
#ifndef SMX_PB_UB
#define SMX_PB_UB 4      // rows in flight of the backward's write phase
#endif
template <typename T, bool VEC, int CL>
__global__ __launch_bounds__(256) void pool_bcast_kernel(const T* __restrict__ S, long lds, const uint8_t* __restrict__ mask_in,
                                                         float* mean_out, const float* __restrict__ inv_in, float* inv_out,
                                                         T* dS, long ldds, int T_, int D, int scale, uint32_t dthresh, float dscale,
                                                         uint64_t dseed_, const uint64_t* ep, const T* __restrict__ Z, long ldz,
                                                         const uint8_t* __restrict__ mask_out, int act) {
  constexpr int N = VT<T>::N, RS = 256 / CL, U = 8, G = 8, RG = RS / G;   // columns per lane, row slots, rows in flight, fold groups
  __shared__ float red[RS][CL * N + 1];
  __shared__ float cred[RS];
  const uint64_t dseed = dthresh ? epoch_seed(dseed_, ep) : 0;
  const int cl = threadIdx.x % CL, rs = threadIdx.x / CL, b = blockIdx.y;
  const int col = (blockIdx.x * CL + cl) * N;
  const int nvalid = D - col;                              // (<= 0: an idle lane of the last column group - it still joins the barriers)
  const T* base = S + (long)b * T_ * lds + (nvalid > 0 ? col : 0);
  const uint8_t* mrow = mask_in ? mask_in + (long)b * T_ : nullptr;
  float acc[N], cnt = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.f;
  const int tlast = T_ - 1;
  for (int t = rs; t < T_; t += U * RS) {                  // U rows in flight per slot; rows past the end: the last row, weight 0
    float f[U][N], m[U];
#pragma unroll
    for (int u = 0; u < U; ++u) loadv<T, VEC>(base + (long)min(t + RS * u, tlast) * lds, nvalid > 0 ? nvalid : 1, f[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int tt = t + RS * u;
      m[u] = tt < T_ ? (mrow ? (mrow[tt] ? 1.f : 0.f) : 1.f) : 0.f;
      cnt += m[u];
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
      acc[i] += ((f[0][i] * m[0] + f[1][i] * m[1]) + (f[2][i] * m[2] + f[3][i] * m[3])) +
                ((f[4][i] * m[4] + f[5][i] * m[5]) + (f[6][i] * m[6] + f[7][i] * m[7]));
  }
#pragma unroll
  for (int i = 0; i < N; ++i) red[rs][cl * N + i] = acc[i];
  if (cl == 0) cred[rs] = cnt;
  __syncthreads();
  // fixed-order fold in two levels: slot g of the first G folds slots g * RG .. g * RG + RG - 1, then everybody folds the G results
  if (rs < G) {
    float c0 = 0.f, w[N];
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = 0.f;
    for (int k = rs * RG; k < rs * RG + RG; ++k) {
      c0 += cred[k];
#pragma unroll
      for (int i = 0; i < N; ++i) w[i] += red[k][cl * N + i];
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);                    // (lgkmcnt(0): the reads above are done before the slot is overwritten)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < N; ++i) red[rs * RG][cl * N + i] = w[i];
    if (cl == 0) cred[rs * RG] = c0;
  }
  __syncthreads();
  float v[N], c = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    c += cred[g * RG];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += red[g * RG][cl * N + i];
  }
  const float inv = 1.f / c;   // zero valid frames -> inf, 0 * inf = NaN, as the reference (summary_mixing.py:264-266)
  if (inv_out && blockIdx.x == 0 && threadIdx.x == 0) inv_out[b] = inv;
  const float sc = (scale ? inv : 1.f);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] *= sc;
  if (nvalid <= 0) return;
  if (mean_out && rs == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < nvalid) mean_out[(long)b * D + col + i] = v[i];
  }
  if (!dS) return;
  if (inv_in) {
    const float si = inv_in[b];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] *= si;
  }
  if (Z || mask_out) {                                     // backward through act(.) * mask of the producing projection
    dispatch_act(Z ? act : SMX_ACT_NONE, [&](auto act_tag) {
      constexpr int ACT = decltype(act_tag)::value;
      constexpr int UB = SMX_PB_UB;                         // rows in flight
      for (int t = rs; t < T_; t += UB * RS) {
        float z[UB][N], mk[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const long n = (long)b * T_ + min(t + u * RS, tlast);
          mk[u] = mask_out ? (mask_out[n] ? 1.f : 0.f) : 1.f;
          if (ACT != SMX_ACT_NONE) loadv<T, VEC>(Z + n * ldz + col, nvalid, z[u]);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          if (t + u * RS >= T_) break;
          float o[N];
#pragma unroll
          for (int i = 0; i < N; ++i) o[i] = ACT != SMX_ACT_NONE ? v[i] * mk[u] * act_grad_c<ACT>(z[u][i]) : v[i] * mk[u];
          storev<T, VEC>(dS + ((long)b * T_ + t + u * RS) * ldds + col, nvalid, o);
        }
      }
    });
  } else if (dthresh == 0) {
    for (int t = rs; t < T_; t += RS) storev<T, VEC>(dS + ((long)b * T_ + t) * ldds + col, nvalid, v);
  } else {                                                 // fused inverted dropout, mask = f(seed, row * D + col)
    for (int t = rs; t < T_; t += RS) {
      const uint64_t ix = ((uint64_t)b * T_ + t) * (uint64_t)D + col;
      float o[N];
#pragma unroll
      for (int i = 0; i < N; ++i) o[i] = v[i];
      dropout_apply_any<N>(o, dseed, ix, dthresh, dscale);
      storev<T, VEC>(dS + ((long)b * T_ + t) * ldds + col, nvalid, o);
    }
  }
}

extern "C" int smx_pool_bcast_ok(int B, int T, int D) {
  // a workgroup per (utterance, 64 bf16 / 32 fp32 columns) walks all T frames: small batches - and big ones of ordinary utterances whose
  // (utterance, column group) pairs alone fill the chip (same-box A/B of the steps with it on: C2b B = 128 18.02 -> 17.90 ms, B = 64
  // 12.00 -> 11.88, C2a 45.36 -> 45.16, C4 38.51 -> 38.00).  Long utterances (config 5: T = 30 000) keep the split-T kernels, whose
  // thousands of workgroups stream at 0.72 of the HBM roof.  SMX_POOL_FUSE_MAX_ROWS: the frame count up to which few pairs are enough.
  if (!(B >= 1 && T >= 1 && D >= 1 && T <= 4096)) return 0;
  return (long)B * T <= (long)cfg().pool_fuse_max_rows || (long)B * ((D + 63) / 64) >= 256;
}

extern "C" int smx_pool_bcast(int dtype, const void* S, int64_t lds, const uint8_t* mask_in, float* mean_out, const float* inv_in,
                              float* inv_out, void* dS, int64_t ldds, int B, int T, int D, int scale_by_count, float drop_p,
                              uint64_t drop_seed, const uint64_t* epoch, const void* Z, int64_t ldz, const uint8_t* mask_out, int act,
                              void* stream) {
  SMX_REQUIRE(S && (mean_out || dS), "smx_pool_bcast: null pointer");
  SMX_REQUIRE(B > 0 && T > 0 && D > 0, "smx_pool_bcast: bad sizes");
  SMX_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "smx_pool_bcast: 0 <= drop_p < 1");
  SMX_REQUIRE(!(drop_p > 0.f && (Z || mask_out)), "smx_pool_bcast: dropout (forward) and the act / mask backward exclude each other");
  if (!smx_pool_bcast_ok(B, T, D)) return fail(SMX_EUNSUPPORTED, "smx_pool_bcast: built for small batches (smx_pool_bcast_ok); use smx_masked_mean_fwd + smx_masked_mean_bwd");
  const uint32_t dthresh = (uint32_t)((double)drop_p * 4294967296.0);
  const float dscale = 1.f / (1.f - drop_p);
  const int nvec = dtype == SMX_BF16 ? 8 : 4;
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  const bool vec = vec_ok(S, lds, D, nvec, es) && (dS == nullptr || vec_ok(dS, ldds, D, nvec, es)) && (Z == nullptr || vec_ok(Z, ldz, D, nvec, es));
  const int a = Z ? act : SMX_ACT_NONE;
  // lanes per row: the widest group (whole 128-byte row segments) that still gives ~half a workgroup per CU
  int CL = 8;
  while (CL > 2 && (long)B * ((D + CL * nvec - 1) / (CL * nvec)) < 128) CL >>= 1;
  dim3 grid((D + CL * nvec - 1) / (CL * nvec), B);
#define SMX_PB_LAUNCH(TT, VV, CC) hipLaunchKernelGGL((pool_bcast_kernel<TT, VV, CC>), grid, dim3(256), 0, STREAM, (const TT*)S, lds, mask_in, mean_out, inv_in, inv_out, (TT*)dS, ldds, T, D, scale_by_count, dthresh, dscale, drop_seed, epoch, (const TT*)Z, ldz, mask_out, a)
#define SMX_PB_CL(TT, VV) do { if (CL == 8) SMX_PB_LAUNCH(TT, VV, 8); else if (CL == 4) SMX_PB_LAUNCH(TT, VV, 4); else SMX_PB_LAUNCH(TT, VV, 2); } while (0)
  if (dtype == SMX_BF16) {
    if (vec) SMX_PB_CL(bf16_t, true); else SMX_PB_CL(bf16_t, false);
  } else if (dtype == SMX_F32) {
    if (vec) SMX_PB_CL(float, true); else SMX_PB_CL(float, false);
  } else return fail(SMX_EINVAL, "smx_pool_bcast: bad dtype");
#undef SMX_PB_CL
#undef SMX_PB_LAUNCH
  return check_launch("smx_pool_bcast");
}

extern "C" size_t smx_chunk_mean_workspace(int B, int T, int D, int chunk) {
  int NC = (T + chunk - 1) / chunk;
  return (size_t)B * NC * D * sizeof(float);
}

// phase: 3 = the whole operator (one shard = the whole sequence); 1 = chunk sums (+ running sums) only - the shard's exchange
// values are then rows of the workspace; 2 = the window combine, with the other shards' contributions in `carry`
template <typename T>
static int chunk_mean_impl(const void* X, int64_t ldx, void* out, int64_t ldo, int B, int T_, int D, int chunk, int left,
                           int reverse, void* ws, hipStream_t s, int phase = 3, int c_off = 0, const float* carry = nullptr,
                           int carry_c0 = 0, int carry_n = 0) {
  const int nvec = VT<T>::N;
  const int NC = (T_ + chunk - 1) / chunk, DC = (D + 64 * nvec - 1) / (64 * nvec);
  dim3 grid(DC, NC, B);
  float* csum = reinterpret_cast<float*>(ws);
  const bool v1 = vec_ok(X, ldx, D, nvec, sizeof(T)), v2 = vec_ok(out, ldo, D, nvec, sizeof(T));
  if (phase & 1) {
    if (v1) hipLaunchKernelGGL((chunk_sum_kernel<T, true>), grid, dim3(256), 0, s, (const T*)X, ldx, csum, T_, D, chunk, NC, left, reverse, c_off);
    else hipLaunchKernelGGL((chunk_sum_kernel<T, false>), grid, dim3(256), 0, s, (const T*)X, ldx, csum, T_, D, chunk, NC, left, reverse, c_off);
    if (left < 0) hipLaunchKernelGGL(chunk_prefix_kernel, dim3((unsigned)((D + 255) / 256), (unsigned)B), dim3(256), 0, s, csum, D, NC, reverse);
  }
  if (phase & 2) {
    if (v2) hipLaunchKernelGGL((chunk_window_kernel<T, true>), grid, dim3(256), 0, s, csum, (T*)out, ldo, T_, D, chunk, NC, left, reverse, c_off, carry, carry_c0, carry_n);
    else hipLaunchKernelGGL((chunk_window_kernel<T, false>), grid, dim3(256), 0, s, csum, (T*)out, ldo, T_, D, chunk, NC, left, reverse, c_off, carry, carry_c0, carry_n);
  }
  return check_launch("smx_chunk_mean");
}

extern "C" int smx_chunk_mean_fwd(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, int B, int T, int D,
                                  int chunk, int left, void* workspace, void* stream) {
  SMX_REQUIRE(S && out && workspace && chunk > 0, "smx_chunk_mean_fwd: bad arguments");
  if (dtype == SMX_BF16) return chunk_mean_impl<bf16_t>(S, lds, out, ldo, B, T, D, chunk, left, 0, workspace, STREAM);
  return chunk_mean_impl<float>(S, lds, out, ldo, B, T, D, chunk, left, 0, workspace, STREAM);
}
extern "C" int smx_chunk_mean_bwd(int dtype, const void* dOut, int64_t ldo, void* dS, int64_t lds, int B, int T, int D,
                                  int chunk, int left, void* workspace, void* stream) {
  SMX_REQUIRE(dOut && dS && workspace && chunk > 0, "smx_chunk_mean_bwd: bad arguments");
  if (dtype == SMX_BF16) return chunk_mean_impl<bf16_t>(dOut, ldo, dS, lds, B, T, D, chunk, left, 1, workspace, STREAM);
  return chunk_mean_impl<float>(dOut, ldo, dS, lds, B, T, D, chunk, left, 1, workspace, STREAM);
}

// Sequence-parallel shards of whole chunks (sequence_parallel.py; summary_mixing.py:224-235 with the mask of TransformerASR.py:85-110):
// the shard holds chunks [c_off, c_off + T / chunk) of the sequence.  phase 1: chunk sums into the workspace (B, T / chunk, D) float32
// - reverse: scaled by 1 / window length of the GLOBAL chunk; left < 0: turned into running sums - whose rows are what the shards
// exchange (the last `left` rows / the last running sum forward, the first ones in reverse).  phase 2: the window combine; chunk c
// adds carry[b][c - carry_c0] (float32 (B, carry_n, D); carry_n == 0: one (B, D) row for every chunk), forward divides by the
// GLOBAL window length.  No elementwise pass over the activations happens outside these kernels.
extern "C" int smx_chunk_mean_sharded(int dtype, const void* X, int64_t ldx, void* out, int64_t ldo, int B, int T, int D, int chunk,
                                      int left, int reverse, int c_off, int phase, const float* carry, int carry_c0, int carry_n,
                                      void* workspace, void* stream) {
  SMX_REQUIRE(workspace && chunk > 0 && T % chunk == 0 && c_off >= 0 && (phase == 1 || phase == 2) && carry_n >= 0 && carry_c0 >= 0,
              "smx_chunk_mean_sharded: shards hold whole chunks; phase 1 or 2");
  SMX_REQUIRE(phase == 1 ? X != nullptr : out != nullptr, "smx_chunk_mean_sharded: null pointer");
  if (B <= 0 || T <= 0 || D <= 0) return SMX_OK;
  if (dtype == SMX_BF16) return chunk_mean_impl<bf16_t>(X, ldx, out, ldo, B, T, D, chunk, left, reverse, workspace, STREAM, phase, c_off, carry, carry_c0, carry_n);
  return chunk_mean_impl<float>(X, ldx, out, ldo, B, T, D, chunk, left, reverse, workspace, STREAM, phase, c_off, carry, carry_c0, carry_n);
}

extern "C" size_t smx_expdecay_mean_workspace(int B, int T, int D) {
  return (size_t)B * ((T + ED_CH - 1) / ED_CH) * 2 * D * sizeof(float);
}

// phase 3: the whole operator; 1: chunk states + the shard's LEAVING states into `ends` (2, B, D); 2: carries (from the ENTERING states
// in `ends`) + both scans out (the workspace of phase 1 must still hold the chunk states)
template <typename T>
static int expdecay_impl(const void* X, int64_t ldx, void* Y, int64_t ldy, int B, int T_, int D, float gamma, int mode,
                         void* ws, hipStream_t s, int phase = 3, int t_off = 0, int T_glob = 0, float* ends = nullptr) {
  const int NC = (T_ + ED_CH - 1) / ED_CH;
  if (T_glob <= 0) T_glob = T_;
  dim3 grid((D + 255) / 256, (NC + 3) / 4, B);
  const dim3 gc((unsigned)(((long)B * D + 255) / 256));
  float* w = reinterpret_cast<float*>(ws);
  const float lng = (float)log((double)gamma);             // (ed_inv_den: the denominators are as accurate as this logarithm)
  if (phase & 1) hipLaunchKernelGGL((expdecay_chunk_kernel<T>), grid, dim3(256), 0, s, (const T*)X, ldx, w, T_, D, NC, gamma, lng, mode, t_off, T_glob);
  if (phase == 1) hipLaunchKernelGGL(expdecay_carry_kernel, gc, dim3(256), 0, s, w, D, NC, B, gamma, (const float*)nullptr, (const float*)nullptr, ends, T_);
  if (phase & 2) {
    const float* fin = phase == 2 ? ends : nullptr;
    hipLaunchKernelGGL(expdecay_carry_kernel, gc, dim3(256), 0, s, w, D, NC, B, gamma, fin, fin ? fin + (long)B * D : nullptr, (float*)nullptr, T_);
    hipLaunchKernelGGL((expdecay_apply_kernel<T>), grid, dim3(256), 0, s, (const T*)X, ldx, w, (T*)Y, ldy, T_, D, NC, gamma, lng, mode, t_off, T_glob);
  }
  return check_launch("smx_expdecay_mean");
}

static int expdecay_check(const void* X, int64_t ldx, const void* Y, int64_t ldy, int D, float gamma, const void* ws, size_t es) {
  SMX_REQUIRE(X && Y && ws, "smx_expdecay_mean: null pointer");
  SMX_REQUIRE(gamma > 0.f && gamma < 1.f, "smx_expdecay_mean: 0 < decay < 1 (got %f)", (double)gamma);
  SMX_REQUIRE(D % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(X) % (4 * es)) == 0 &&
                  (reinterpret_cast<uintptr_t>(Y) % (4 * es)) == 0 && aligned16(ws),
              "smx_expdecay_mean: needs D, leading dimensions multiples of 4 and aligned pointers");
  return SMX_OK;
}

extern "C" int smx_expdecay_mean_fwd(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, int B, int T, int D,
                                     float decay, void* workspace, void* stream) {
  int rc = expdecay_check(S, lds, out, ldo, D, decay, workspace, dtype == SMX_BF16 ? 2 : 4);
  if (rc != SMX_OK) return rc;
  if (B <= 0 || T <= 0 || D <= 0) return SMX_OK;
  if (dtype == SMX_BF16) return expdecay_impl<bf16_t>(S, lds, out, ldo, B, T, D, decay, 0, workspace, STREAM);
  return expdecay_impl<float>(S, lds, out, ldo, B, T, D, decay, 0, workspace, STREAM);
}
extern "C" int smx_expdecay_mean_bwd(int dtype, const void* dOut, int64_t ldo, void* dS, int64_t lds, int B, int T, int D,
                                     float decay, void* workspace, void* stream) {
  int rc = expdecay_check(dOut, ldo, dS, lds, D, decay, workspace, dtype == SMX_BF16 ? 2 : 4);
  if (rc != SMX_OK) return rc;
  if (B <= 0 || T <= 0 || D <= 0) return SMX_OK;
  if (dtype == SMX_BF16) return expdecay_impl<bf16_t>(dOut, ldo, dS, lds, B, T, D, decay, 1, workspace, STREAM);
  return expdecay_impl<float>(dOut, ldo, dS, lds, B, T, D, decay, 1, workspace, STREAM);
}

// The expdecay summary on a sequence-parallel shard (frames [t_off, t_off + T) of T_glob): the filter crosses the boundary through ONE
// (B, D) state per direction.  phase 1: ends (2, B, D) <- the states LEAVING the shard (f at its last frame, g at its first) for zero
// entering states; the caller gathers them and folds f_in = ends_q[0] + decay^T f_in over the earlier shards (g_in over the later
// ones) - (B, D) arithmetic - into `ends`; phase 2 (same workspace): out = the operator with those ENTERING states and the
// denominators of the GLOBAL frame index (summary_mixing.py:316-365; mode 0 forward, 1 the transposed operator M (s / rowsum(M))).
extern "C" int smx_expdecay_mean_sharded(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, int B, int T, int D, float decay,
                                         int mode, int t_off, int T_glob, int phase, float* ends, void* workspace, void* stream) {
  SMX_REQUIRE(S && workspace && ends && (phase == 1 || phase == 2) && (mode == 0 || mode == 1) && t_off >= 0 && T_glob >= t_off + T,
              "smx_expdecay_mean_sharded: bad arguments");
  SMX_REQUIRE(decay > 0.f && decay < 1.f, "smx_expdecay_mean_sharded: 0 < decay < 1");
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  SMX_REQUIRE(D % 4 == 0 && lds % 4 == 0 && (reinterpret_cast<uintptr_t>(S) % (4 * es)) == 0 && aligned16(workspace) && aligned16(ends) &&
                  (phase == 1 || (out && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) % (4 * es)) == 0)),
              "smx_expdecay_mean_sharded: needs D, leading dimensions multiples of 4 and aligned pointers");
  if (B <= 0 || T <= 0 || D <= 0) return SMX_OK;
  if (dtype == SMX_BF16) return expdecay_impl<bf16_t>(S, lds, out, ldo, B, T, D, decay, mode, workspace, STREAM, phase, t_off, T_glob, ends);
  return expdecay_impl<float>(S, lds, out, ldo, B, T, D, decay, mode, workspace, STREAM, phase, t_off, T_glob, ends);
}

static const int ACT_BWD_RS = 32;
static const int ACT_BWD_YMAX = 512;   // row-strip workgroups per column block (= partial rows of the bias reduction)
extern "C" size_t smx_act_mask_bwd_workspace(int N, int M) { return (size_t)((N + ACT_BWD_RS - 1) / ACT_BWD_RS) * M * sizeof(float); }

extern "C" int smx_act_mask_bwd(int dtype, const void* dY, int64_t lddy, const void* Z, int64_t ldz,
                                const uint8_t* row_mask, void* dZ, int64_t lddz, int N, int M, int act, float alpha,
                                float* dbias, float* dgroup, int64_t lddgroup, int group_div, float drop_p,
                                uint64_t drop_seed, const uint64_t* epoch, void* workspace, void* stream) {
  SMX_REQUIRE(dY && N >= 0 && M > 0, "smx_act_mask_bwd: bad arguments");
  SMX_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "smx_act_mask_bwd: 0 <= drop_p < 1");
  const uint32_t dthresh = (uint32_t)((double)drop_p * 4294967296.0);
  const float dscale = 1.f / (1.f - drop_p);
  SMX_REQUIRE(!dgroup || group_div > 0, "smx_act_mask_bwd: group_div must be > 0");
  if (N == 0) return SMX_OK;
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  const int nv = dtype == SMX_BF16 ? 8 : 4;
  auto ok = [&](const void* p, int64_t ld) { return p == nullptr || (aligned16(p) && (ld * (int64_t)es) % 16 == 0); };
  const bool vec = M % nv == 0 && ok(dY, lddy) && ok(Z, ldz) && ok(dZ, lddz) && (!dbias || workspace);
  if (vec) {
    int chunks = M / nv, LPR = 1;
    while (LPR < 64 && LPR < chunks) LPR <<= 1;       // lanes per row chunk (power of two <= 64)
    const int RS = ACT_BWD_RS;
    float* partial = reinterpret_cast<float*>(workspace);
    const int ny = min((N + RS - 1) / RS, ACT_BWD_YMAX);
    dim3 grid((chunks + LPR - 1) / LPR, ny);
    if (dtype == SMX_BF16) hipLaunchKernelGGL((act_mask_bwd_vec_kernel<bf16_t>), grid, dim3(256), 0, STREAM, (const bf16_t*)dY, lddy, (const bf16_t*)Z, ldz, row_mask, (bf16_t*)dZ, lddz, N, M, act, alpha, dbias, dgroup, lddgroup, group_div, RS, LPR, partial, dthresh, dscale, drop_seed, epoch);
    else hipLaunchKernelGGL((act_mask_bwd_vec_kernel<float>), grid, dim3(256), 0, STREAM, (const float*)dY, lddy, (const float*)Z, ldz, row_mask, (float*)dZ, lddz, N, M, act, alpha, dbias, dgroup, lddgroup, group_div, RS, LPR, partial, dthresh, dscale, drop_seed, epoch);
    if (dbias) hipLaunchKernelGGL(colsum_partials_kernel, dim3((M + 15) / 16), dim3(256), 0, STREAM, partial, ny, M, dbias);
  } else {
    const int RS = 128;
    dim3 grid((M + 255) / 256, (N + RS - 1) / RS);
    if (dtype == SMX_BF16) hipLaunchKernelGGL((act_mask_bwd_kernel<bf16_t>), grid, dim3(256), 0, STREAM, (const bf16_t*)dY, lddy, (const bf16_t*)Z, ldz, row_mask, (bf16_t*)dZ, lddz, N, M, act, alpha, dbias, dgroup, lddgroup, group_div, RS, dthresh, dscale, drop_seed, epoch);
    else hipLaunchKernelGGL((act_mask_bwd_kernel<float>), grid, dim3(256), 0, STREAM, (const float*)dY, lddy, (const float*)Z, ldz, row_mask, (float*)dZ, lddz, N, M, act, alpha, dbias, dgroup, lddgroup, group_div, RS, dthresh, dscale, drop_seed, epoch);
  }
  return check_launch("smx_act_mask_bwd");
}

extern "C" int smx_axpby(int dtype, float a, const void* X, int64_t ldx, float b, const void* Y0, int64_t ldy0, void* Y,
                         int64_t ldy, int N, int D, void* stream) {
  SMX_REQUIRE(X && Y, "smx_axpby: null pointer");
  if (N <= 0 || D <= 0) return SMX_OK;
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  auto ok = [&](const void* p, int64_t ld) { return p == nullptr || ((reinterpret_cast<uintptr_t>(p) % (4 * es)) == 0 && ld % 4 == 0); };
  const bool vec = ok(X, ldx) && ok(Y0, ldy0) && ok(Y, ldy);
  int grid = grid1d((long)N * ((D + 3) / 4));
  if (dtype == SMX_BF16) {
    if (vec) hipLaunchKernelGGL((axpby_kernel<bf16_t, true>), dim3(grid), dim3(256), 0, STREAM, a, (const bf16_t*)X, ldx, b, (const bf16_t*)Y0, ldy0, (bf16_t*)Y, ldy, N, D);
    else hipLaunchKernelGGL((axpby_kernel<bf16_t, false>), dim3(grid), dim3(256), 0, STREAM, a, (const bf16_t*)X, ldx, b, (const bf16_t*)Y0, ldy0, (bf16_t*)Y, ldy, N, D);
  } else {
    if (vec) hipLaunchKernelGGL((axpby_kernel<float, true>), dim3(grid), dim3(256), 0, STREAM, a, (const float*)X, ldx, b, (const float*)Y0, ldy0, (float*)Y, ldy, N, D);
    else hipLaunchKernelGGL((axpby_kernel<float, false>), dim3(grid), dim3(256), 0, STREAM, a, (const float*)X, ldx, b, (const float*)Y0, ldy0, (float*)Y, ldy, N, D);
  }
  return check_launch("smx_axpby");
}

extern "C" int smx_dropout(int dtype, const void* X, int64_t ldx, void* Y, int64_t ldy, int N, int D, float p,
                           uint64_t seed, const uint64_t* epoch, void* stream) {
  SMX_REQUIRE(X && Y && p >= 0.f && p < 1.f, "smx_dropout: bad arguments (0 <= p < 1)");
  if (N <= 0 || D <= 0) return SMX_OK;
  const uint32_t thresh = (uint32_t)((double)p * 4294967296.0);
  const float scale = 1.f / (1.f - p);
  int grid = grid1d((long)N * ((D + 3) / 4));
  if (dtype == SMX_BF16) hipLaunchKernelGGL((dropout_kernel<bf16_t>), dim3(grid), dim3(256), 0, STREAM, (const bf16_t*)X, ldx, (bf16_t*)Y, ldy, N, D, thresh, scale, seed, epoch);
  else hipLaunchKernelGGL((dropout_kernel<float>), dim3(grid), dim3(256), 0, STREAM, (const float*)X, ldx, (float*)Y, ldy, N, D, thresh, scale, seed, epoch);
  return check_launch("smx_dropout");
}

extern "C" int smx_add_rowtable(int dtype, void* Y, int64_t ldy, const float* table, int R, int N, int D, void* stream) {
  SMX_REQUIRE(Y && table && R > 0, "smx_add_rowtable: bad arguments");
  if (N <= 0 || D <= 0) return SMX_OK;
  int grid = grid1d((long)N * D);
  if (dtype == SMX_BF16) hipLaunchKernelGGL((add_rowtable_kernel<bf16_t>), dim3(grid), dim3(256), 0, STREAM, (bf16_t*)Y, ldy, table, R, N, D);
  else hipLaunchKernelGGL((add_rowtable_kernel<float>), dim3(grid), dim3(256), 0, STREAM, (float*)Y, ldy, table, R, N, D);
  return check_launch("smx_add_rowtable");
}

extern "C" int smx_cast_from_f32(int dtype, const float* src, void* dst, int64_t n, void* stream) {
  SMX_REQUIRE(src && dst, "smx_cast_from_f32: null pointer");
  if (n <= 0) return SMX_OK;
  if (dtype == SMX_BF16) hipLaunchKernelGGL((cast_from_f32_kernel<bf16_t>), dim3(grid1d(n)), dim3(256), 0, STREAM, src, (bf16_t*)dst, n);
  else hipLaunchKernelGGL((cast_from_f32_kernel<float>), dim3(grid1d(n)), dim3(256), 0, STREAM, src, (float*)dst, n);
  return check_launch("smx_cast_from_f32");
}
extern "C" int smx_cast_to_f32(int dtype, const void* src, float* dst, int64_t n, void* stream) {
  SMX_REQUIRE(src && dst, "smx_cast_to_f32: null pointer");
  if (n <= 0) return SMX_OK;
  if (dtype == SMX_BF16) hipLaunchKernelGGL((cast_to_f32_kernel<bf16_t>), dim3(grid1d(n)), dim3(256), 0, STREAM, (const bf16_t*)src, dst, n);
  else hipLaunchKernelGGL((cast_to_f32_kernel<float>), dim3(grid1d(n)), dim3(256), 0, STREAM, (const float*)src, dst, n);
  return check_launch("smx_cast_to_f32");
}

extern "C" int smx_adamw_step_lr(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                 int64_t n, float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                 int step, float grad_scale, const float* gscale_dev, const uint64_t* step_dev, void* stream) {
  SMX_REQUIRE(param && grad && exp_avg && exp_avg_sq, "smx_adamw_step: bad arguments");
  if (n <= 0) return SMX_OK;
  SMX_REQUIRE(step > 0 || step_dev, "smx_adamw_step: step <= 0 needs the device step counter (step_dev)");
  float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(adamw_kernel, dim3(grid1d(n)), dim3(256), 0, STREAM, param, grad, exp_avg, exp_avg_sq,
                     (uint16_t*)shadow_bf16, n, lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2), grad_scale, gscale_dev,
                     step > 0 ? nullptr : step_dev, lr_dev);
  return check_launch("smx_adamw_step");
}
extern "C" int smx_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                              int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                              float grad_scale, const float* gscale_dev, const uint64_t* step_dev, void* stream) {
  return smx_adamw_step_lr(param, grad, exp_avg, exp_avg_sq, shadow_bf16, n, lr, nullptr, beta1, beta2, eps, weight_decay, step,
                           grad_scale, gscale_dev, step_dev, stream);
}
extern "C" size_t smx_sumsq_workspace(void) { return SUMSQ_BLOCKS * sizeof(float); }
extern "C" int smx_sumsq(const float* x, int64_t n, float* out, void* workspace, void* stream) {
  SMX_REQUIRE(x && out && workspace, "smx_sumsq: null pointer");
  if (n <= 0) return SMX_OK;
  int g = grid1d(n);
  if (g > SUMSQ_BLOCKS) g = SUMSQ_BLOCKS;
  hipLaunchKernelGGL(sumsq_kernel, dim3(g), dim3(256), 0, STREAM, x, n, reinterpret_cast<float*>(workspace));
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, STREAM, reinterpret_cast<const float*>(workspace), g, out);
  return check_launch("smx_sumsq");
}
extern "C" int smx_clip_factor(const float* sumsq, float max_norm, float inv_scale, float* out, void* stream) {
  SMX_REQUIRE(sumsq && out, "smx_clip_factor: null pointer");
  hipLaunchKernelGGL(clip_factor_kernel, dim3(1), dim3(1), 0, STREAM, sumsq, max_norm, inv_scale, out);
  return check_launch("smx_clip_factor");
}
