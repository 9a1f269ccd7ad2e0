// attention.hip — scaled-dot-product attention for speechbrain.nnet.attention.MultiheadAttention (regularMHA), gfx950 only.
//   the decoder layer's two attentions   speechbrain/lobes/models/transformer/Transformer.py:745-751, :811-840
// One descriptor-driven problem (smx_attn_args, include/smx.h): Q (B, L, H, D), K / V (B, S, H, D), O (B, L, H, D), every operand a
// base pointer with element strides for batch, row and head (D contiguous, 16-byte aligned): the operands are read in place out of
// the packed (B, L, 3, H, D) / (B, S, 2, H, D) projection outputs and the gradients land in the packed gradient buffers.
//   s[b,h,i,j] = scale <q_i, k_j> + bias[i,j];  masked (-inf) where j > i + (S - L) (causal), key_pad[b,j] != 0 or bias == -inf
//   p = softmax_j(s) in fp32 with the row maximum subtracted;  p~ = keep(seed, ((b H + h) L + i) S + j) ? p / (1 - drop_p) : 0
//   O = p~ V;  lse = log sum_j exp(s)
// A row whose keys are all masked gives O = 0, lse = -inf and zero gradients (torch gives NaN there).
//
// Arithmetic.  Every product runs on the 16 x 16 MFMA with an fp32 accumulator: F32 operands on v_mfma_f32_16x16x4_f32 (exact fp32
// products, a k-ordered fma chain), BF16 operands on v_mfma_f32_16x16x32_bf16.  Scores, softmax, lse, delta and the accumulators are
// fp32.  What the second product of a pass reads goes through LDS in the operand dtype: for BF16 p~ (forward, dV) and dS (dQ, dK)
// are rounded to bf16 ONCE there; nothing else is rounded before the output store.  That single rounding (2^-9 relative per
// probability) is the BF16 error of this file beyond the bf16 inputs and outputs themselves.
//
// Structure.  A workgroup is 4 waves; a "row tile" is 16 rows (one MFMA tile), a "column tile" 64.
//   dot_block   one wave: a 16 x 16 block of X Y^T for two operands whose rows are D-contiguous in global memory (Q K^T, dO V^T and
//               their transposes), fragments loaded 16 bytes per lane straight from global memory / L2, two accumulator chains.
//   acc_staged  the workgroup: acc (16 x D) += A (16 x 64, LDS) X (64 x D, global).  X is summed over its ROW index, so it is
//               staged through LDS transposed ([d][row], chunks of up to 128 columns of D); each wave owns a quarter of D.
//   forward     grid (ceil(L / 16), H, B): per 64-key tile the four waves write a 16 x 64 score tile, 16 lanes per row run the
//               online softmax (running max / sum in registers, rescale factor through LDS), p~ -> LDS, acc_staged with V.
//   backward    two launches.  dQ: grid (ceil(L / 16), H, B), two sweeps over the key tiles with S and dP = dO V^T from dot_block:
//               the first sums delta_i = sum_j p_ij D(dP)_ij (mathematically rowsum(dO O); taken from the dP bits themselves, so that
//               dS = p (dP - delta) cancels exactly for a row with one visible key, as torch's softmax backward does) and stores it,
//               the second writes dS -> LDS and runs acc_staged with K.  dK / dV: grid (ceil(S / 16), H, B), a workgroup owns 16 keys
//               and walks the queries 64 at a time: S^T and dP^T from dot_block (the same fma chains, operands swapped), p~^T and
//               dS^T -> LDS, acc_staged with dO and with Q.  Probabilities come back from lse, the keep mask from the seed.
//               No atomics, one fixed summation order.
//   weights     grid (ceil(L / 16), ceil(S / 64), B): sum over heads, in index order, of exp(s - lse) (dropped as in forward) / H.
#include "smx_common.h"

namespace smx {

typedef __attribute__((ext_vector_type(4))) float at_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 at_bf16x8;
static constexpr float AT_NEG_INF = -__builtin_inff();
enum { AT_ROWS = 16, AT_COLS = 64, AT_THREADS = 256 };

// E: elements in 16 bytes; KSTEP: elements of the summed index one 16-byte fragment pair of the wave covers (4 lane groups x E);
// LDT: row stride (elements) of a 64-wide LDS image, padded, rows 16-byte aligned
template <typename T>
struct AtT;
template <>
struct AtT<float> { static constexpr int E = 4, KSTEP = 16, LDT = 68; };
template <>
struct AtT<bf16_t> { static constexpr int E = 8, KSTEP = 32, LDT = 72; };

constexpr int at_dchunk(int D) { return D < 128 ? D : 128; }
constexpr int at_lds_bytes(int es, int D, int pass) {
  const int ldt = es == 4 ? 68 : 72;
  const int img = AT_ROWS * ldt * es, xt = at_dchunk(D) * ldt * es;
  return pass == SMX_ATTN_PASS_FWD ? AT_ROWS * 68 * 4 + img + xt + 3 * AT_ROWS * 4 : pass == SMX_ATTN_PASS_BWD_DQ ? img + xt + 4 * AT_ROWS * 4 : pass == SMX_ATTN_PASS_BWD_DKV ? 2 * img + xt : 0;
}

// acc (16 x 16) += A (16 rows x KSTEP) B (16 rows x KSTEP)^T.  pa / pb: this lane's 16 bytes, row (lane & 15), lane group
// g = lane >> 4 at element g E of the step.  Result register r of lane (c = lane & 15, g): row 4 g + r of A, row c of B.
// F32: component x of the four lane groups is one 16x16x4 product, so the summed index runs 0, 4, 8, 12, 1, 5, ... inside a step -
// the same permutation for both operands.
__device__ __forceinline__ void mma16(at_f32x4& acc, const float* pa, const float* pb) {
  const float4 a = *reinterpret_cast<const float4*>(pa), b = *reinterpret_cast<const float4*>(pb);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma16(at_f32x4& acc, const bf16_t* pa, const bf16_t* pb) {
  const uint4 a = *reinterpret_cast<const uint4*>(pa), b = *reinterpret_cast<const uint4*>(pb);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(at_bf16x8, a), __builtin_bit_cast(at_bf16x8, b), acc, 0, 0, 0);
}

// 16 x 16 block of X Y^T over D (rows D-contiguous in global memory); xrow / yrow carry the lane's row and its g E offset
template <typename T, int D>
__device__ __forceinline__ at_f32x4 dot_block(const T* __restrict__ xrow, const T* __restrict__ yrow) {
  constexpr int KS = AtT<T>::KSTEP;
  at_f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int s = 0; s < D / KS; s += 2) {
    mma16(a0, xrow + s * KS, yrow + s * KS);
    mma16(a1, xrow + (s + 1) * KS, yrow + (s + 1) * KS);
  }
  return a0 + a1;
}

// X rows [0, 64) x columns [0, DC) at X (row stride ld) -> Xt[d][row]; rows at and beyond nvalid are zeros
template <typename T, int DC>
__device__ __forceinline__ void stage_t(T* __restrict__ Xt, const T* __restrict__ X, long ld, int nvalid) {
  constexpr int E = AtT<T>::E, LDT = AtT<T>::LDT, NP = AT_COLS * DC / E;
  static_assert(NP % AT_THREADS == 0, "whole rounds");
#pragma unroll
  for (int p0 = 0; p0 < NP; p0 += AT_THREADS) {
    const int p = p0 + (int)threadIdx.x, row = p & 63, dp = p >> 6;
    union { uint4 u; T t[E]; } raw;
    raw.u = make_uint4(0u, 0u, 0u, 0u);
    if (row < nvalid) raw.u = *reinterpret_cast<const uint4*>(X + (long)row * ld + dp * E);
#pragma unroll
    for (int e = 0; e < E; ++e) Xt[(dp * E + e) * LDT + row] = raw.t[e];
  }
}

// acc[D / 64] (this wave's 16-column tiles of a 16 x D result: chunk ch, tile t -> columns ch DC + (w NT + t) 16 ...) += A X,
// A (16 x 64) in LDS with row stride LDT, X = 64 rows of D columns in global memory.  Ends on a barrier: A and Xt are free after it.
template <typename T, int D>
__device__ __forceinline__ void acc_staged(at_f32x4 (&acc)[D / 64], const T* __restrict__ A, const T* __restrict__ X, long ld,
                                           int nvalid, T* __restrict__ Xt) {
  constexpr int DC = at_dchunk(D), NT = DC / 64, NCH = D / DC, KS = AtT<T>::KSTEP, LDT = AtT<T>::LDT, E = AtT<T>::E;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    stage_t<T, DC>(Xt, X + ch * DC, ld, nvalid);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const T* pa = A + c * LDT + g * E;
      const T* pb = Xt + ((w * NT + t) * 16 + c) * LDT + g * E;
#pragma unroll
      for (int s = 0; s < AT_COLS / KS; ++s) mma16(acc[ch * NT + t], pa + s * KS, pb + s * KS);
    }
    __syncthreads();
  }
}

template <typename T>
__device__ __forceinline__ const T* at_base(const smx_attn_operand& o, int b, int h) {
  return reinterpret_cast<const T*>(o.p) + (long)b * o.sb + (long)h * o.sh;
}

// the masked score of (query i, key j); i may be a padding row (>= L: the caller discards it), j may be >= S (masked)
__device__ __forceinline__ float at_score(const smx_attn_args& a, float dot, int b, int i, int j) {
  if (j >= a.S) return AT_NEG_INF;
  if (a.causal && j > i + (a.S - a.L)) return AT_NEG_INF;
  if (a.key_pad && a.key_pad[(long)b * a.ldpad + j]) return AT_NEG_INF;
  float s = dot * a.scale;
  if (a.attn_bias) s += a.attn_bias[(long)(i < a.L ? i : a.L - 1) * a.ldbias + j];
  return s;
}
__device__ __forceinline__ uint64_t at_idx(const smx_attn_args& a, int b, int h, int i, int j) {
  return (((uint64_t)b * a.H + h) * a.L + i) * (uint64_t)a.S + j;
}
__device__ __forceinline__ uint32_t at_thresh(const smx_attn_args& a) {
  return a.drop_p > 0.f ? (uint32_t)((double)a.drop_p * 4294967296.0) : 0u;
}
// the last key (exclusive) any row of the query tile at i0 can see / the first query any key of the tile at j0 is seen by
__device__ __forceinline__ int at_key_end(const smx_attn_args& a, int i0) {
  if (!a.causal) return a.S;
  const int e = i0 + AT_ROWS + (a.S - a.L);
  return e < 0 ? 0 : (e < a.S ? e : a.S);
}

// store this wave's tiles of a 16 x D result (rows r0 .. r0 + 15 below nrows) scaled per row
template <typename T, int D>
__device__ __forceinline__ void at_store(const at_f32x4 (&acc)[D / 64], const smx_attn_operand& o, int b, int h, int r0, int nrows,
                                         const float (&rs)[4]) {
  constexpr int DC = at_dchunk(D), NT = DC / 64, NCH = D / DC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  T* base = reinterpret_cast<T*>(o.p) + (long)b * o.sb + (long)h * o.sh;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + 4 * g + r;
        if (row < nrows) base[(long)row * o.sr + ch * DC + (w * NT + t) * 16 + c] = from_f32<T>(acc[ch * NT + t][r] * rs[r]);
      }
}

template <typename T, int D>
__global__ __launch_bounds__(AT_THREADS) void attn_fwd_kernel(const smx_attn_args a) {
  using C = AtT<T>;
  constexpr int E = C::E, LDT = C::LDT, DC = at_dchunk(D);
  __shared__ __attribute__((aligned(16))) float Ss[AT_ROWS * 68];
  __shared__ __attribute__((aligned(16))) T Ps[AT_ROWS * LDT];
  __shared__ __attribute__((aligned(16))) T Xt[DC * LDT];
  __shared__ float al[AT_ROWS], lrow[AT_ROWS], mrow[AT_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * AT_ROWS, h = blockIdx.y, b = blockIdx.z;
  const T* Q = at_base<T>(a.q, b, h);
  const T* K = at_base<T>(a.k, b, h);
  const T* V = at_base<T>(a.v, b, h);
  const int qi = i0 + c < a.L ? i0 + c : a.L - 1;
  const T* qrow = Q + (long)qi * a.q.sr + g * E;
  const int r = tid >> 4, sub = tid & 15;                // softmax: 16 lanes per row, 4 consecutive keys each
  const uint32_t thresh = at_thresh(a);
  const uint64_t seed = thresh ? epoch_seed(a.drop_seed, a.epoch) : 0;
  const float inv_keep = 1.0f / (1.0f - a.drop_p);
  at_f32x4 o[D / 64];
#pragma unroll
  for (int t = 0; t < D / 64; ++t) o[t] = at_f32x4{0.f, 0.f, 0.f, 0.f};
  float m = AT_NEG_INF, l = 0.f;
  const int kend = at_key_end(a, i0);
  for (int j0 = 0; j0 < kend; j0 += AT_COLS) {
    {
      const int j = j0 + 16 * w + c, kj = j < a.S ? j : a.S - 1;
      const at_f32x4 acc = dot_block<T, D>(qrow, K + (long)kj * a.k.sr + g * E);
#pragma unroll
      for (int q = 0; q < 4; ++q) Ss[(4 * g + q) * 68 + 16 * w + c] = at_score(a, acc[q], b, i0 + 4 * g + q, j);
    }
    __syncthreads();
    {
      const float4 sv = *reinterpret_cast<const float4*>(&Ss[r * 68 + 4 * sub]);
      const float s[4] = {sv.x, sv.y, sv.z, sv.w};
      float tm = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
#pragma unroll
      for (int x = 8; x > 0; x >>= 1) tm = fmaxf(tm, __shfl_xor(tm, x, 16));
      const float mn = fmaxf(m, tm);
      float alpha = 1.f, p[4] = {0.f, 0.f, 0.f, 0.f};
      if (mn != AT_NEG_INF) {                            // (a row with no visible key so far keeps m = -inf, l = 0, O = 0)
        alpha = m == AT_NEG_INF ? 0.f : expf(m - mn);
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = s[e] == AT_NEG_INF ? 0.f : expf(s[e] - mn);
      }
      float ps = (p[0] + p[1]) + (p[2] + p[3]);
#pragma unroll
      for (int x = 8; x > 0; x >>= 1) ps += __shfl_xor(ps, x, 16);
      l = l * alpha + ps;
      m = mn;
      const int i = i0 + r;
      if (thresh && i < a.L) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = j0 + 4 * sub + e;
          if (j < a.S) p[e] = dropout_keep(seed, at_idx(a, b, h, i, j), thresh) ? p[e] * inv_keep : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) Ps[r * LDT + 4 * sub + e] = from_f32<T>(p[e]);
      if (sub == 0) al[r] = alpha;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float f = al[4 * g + q];
#pragma unroll
      for (int t = 0; t < D / 64; ++t) o[t][q] *= f;
    }
    acc_staged<T, D>(o, Ps, V + (long)j0 * a.v.sr, a.v.sr, a.S - j0, Xt);
  }
  if (sub == 0) { lrow[r] = l; mrow[r] = m; }
  __syncthreads();
  if (tid < AT_ROWS && i0 + tid < a.L)
    a.lse[((long)b * a.H + h) * a.L + i0 + tid] = lrow[tid] > 0.f ? mrow[tid] + logf(lrow[tid]) : AT_NEG_INF;
  float rs[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) rs[q] = lrow[4 * g + q] > 0.f ? 1.0f / lrow[4 * g + q] : 0.f;
  at_store<T, D>(o, a.o, b, h, i0, a.L, rs);
}

// One (query i, key j) of the backward from the recomputed score, the saved lse, dP = <dO_i, v_j> and delta: p, p~, the dropped dP
// (rounded once, by a multiply the compiler may not fuse: the delta sweep and both gradient kernels must see the same bits) and dS
__device__ __forceinline__ void at_bwd_entry(const smx_attn_args& a, float s, float lse, float delta, float dp, bool live, bool keep,
                                             float inv_keep, float& p, float& pt, float& dpd, float& ds) {
  p = (live && s != AT_NEG_INF && lse != AT_NEG_INF) ? expf(s - lse) : 0.f;
  pt = keep ? p * inv_keep : 0.f;
  dpd = keep ? __fmul_rn(dp, inv_keep) : 0.f;
  ds = p * __fsub_rn(dpd, delta) * a.scale;
}

template <typename T, int D>
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_dq_kernel(const smx_attn_args a) {
  using C = AtT<T>;
  constexpr int E = C::E, LDT = C::LDT, DC = at_dchunk(D);
  __shared__ __attribute__((aligned(16))) T Ps[AT_ROWS * LDT];
  __shared__ __attribute__((aligned(16))) T Xt[DC * LDT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * AT_ROWS, h = blockIdx.y, b = blockIdx.z;
  const T* K = at_base<T>(a.k, b, h);
  const T* V = at_base<T>(a.v, b, h);
  const int qi = i0 + c < a.L ? i0 + c : a.L - 1;
  const T* qrow = at_base<T>(a.q, b, h) + (long)qi * a.q.sr + g * E;
  const T* grow = at_base<T>(a.dO, b, h) + (long)qi * a.dO.sr + g * E;
  const uint32_t thresh = at_thresh(a);
  const uint64_t seed = thresh ? epoch_seed(a.drop_seed, a.epoch) : 0;
  const float inv_keep = 1.0f / (1.0f - a.drop_p);
  __shared__ float red[4][AT_ROWS];
  float lse[4], delta[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = i0 + 4 * g + q;
    lse[q] = a.lse[((long)b * a.H + h) * a.L + (i < a.L ? i : a.L - 1)];
  }
  at_f32x4 dq[D / 64];
#pragma unroll
  for (int t = 0; t < D / 64; ++t) dq[t] = at_f32x4{0.f, 0.f, 0.f, 0.f};
  const int kend = at_key_end(a, i0);
  // first sweep: delta_i = sum_j p_ij D(dP)_ij, D = the dropout (= rowsum(dO O)), from the very dP and p bits the second sweep and the dK / dV kernel
  // recompute, so p (dP - delta) cancels EXACTLY where a row sees a single key; keys in ascending order per lane, then the 16 lanes
  // of a row by butterfly and the four waves in index order
  for (int j0 = 0; j0 < kend; j0 += AT_COLS) {
    const int j = j0 + 16 * w + c, kj = j < a.S ? j : a.S - 1;
    const at_f32x4 as = dot_block<T, D>(qrow, K + (long)kj * a.k.sr + g * E);
    const at_f32x4 ap = dot_block<T, D>(grow, V + (long)kj * a.v.sr + g * E);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + 4 * g + q;
      const bool live = i < a.L && j < a.S;
      const bool keep = !thresh || !live || dropout_keep(seed, at_idx(a, b, h, i, j), thresh);
      float p, pt, dpd, ds;
      at_bwd_entry(a, at_score(a, as[q], b, i, j), lse[q], 0.f, ap[q], live, keep, thresh ? inv_keep : 1.f, p, pt, dpd, ds);
      delta[q] = fmaf(p, dpd, delta[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int x = 8; x > 0; x >>= 1) delta[q] += __shfl_xor(delta[q], x, 16);
    if (c == 0) red[w][4 * g + q] = delta[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) delta[q] = ((red[0][4 * g + q] + red[1][4 * g + q]) + red[2][4 * g + q]) + red[3][4 * g + q];
  if (w == 0 && c == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i0 + 4 * g + q < a.L) a.delta[((long)b * a.H + h) * a.L + i0 + 4 * g + q] = delta[q];
  }
  for (int j0 = 0; j0 < kend; j0 += AT_COLS) {
    const int j = j0 + 16 * w + c, kj = j < a.S ? j : a.S - 1;
    const at_f32x4 as = dot_block<T, D>(qrow, K + (long)kj * a.k.sr + g * E);
    const at_f32x4 ap = dot_block<T, D>(grow, V + (long)kj * a.v.sr + g * E);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + 4 * g + q;
      const bool live = i < a.L && j < a.S;
      const bool keep = !thresh || !live || dropout_keep(seed, at_idx(a, b, h, i, j), thresh);
      float p, pt, dpd, ds;
      at_bwd_entry(a, at_score(a, as[q], b, i, j), lse[q], delta[q], ap[q], live, keep, thresh ? inv_keep : 1.f, p, pt, dpd, ds);
      Ps[(4 * g + q) * LDT + 16 * w + c] = from_f32<T>(ds);
    }
    acc_staged<T, D>(dq, Ps, K + (long)j0 * a.k.sr, a.k.sr, a.S - j0, Xt);
  }
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  at_store<T, D>(dq, a.dq, b, h, i0, a.L, one);
}

template <typename T, int D>
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_dkv_kernel(const smx_attn_args a) {
  using C = AtT<T>;
  constexpr int E = C::E, LDT = C::LDT, DC = at_dchunk(D);
  __shared__ __attribute__((aligned(16))) T Pt[AT_ROWS * LDT];
  __shared__ __attribute__((aligned(16))) T St[AT_ROWS * LDT];
  __shared__ __attribute__((aligned(16))) T Xt[DC * LDT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int j0 = blockIdx.x * AT_ROWS, h = blockIdx.y, b = blockIdx.z;
  const T* Q = at_base<T>(a.q, b, h);
  const T* G = at_base<T>(a.dO, b, h);
  const int kj = j0 + c < a.S ? j0 + c : a.S - 1;
  const T* krow = at_base<T>(a.k, b, h) + (long)kj * a.k.sr + g * E;
  const T* vrow = at_base<T>(a.v, b, h) + (long)kj * a.v.sr + g * E;
  const uint32_t thresh = at_thresh(a);
  const uint64_t seed = thresh ? epoch_seed(a.drop_seed, a.epoch) : 0;
  const float inv_keep = 1.0f / (1.0f - a.drop_p);
  at_f32x4 dk[D / 64], dv[D / 64];
#pragma unroll
  for (int t = 0; t < D / 64; ++t) dk[t] = dv[t] = at_f32x4{0.f, 0.f, 0.f, 0.f};
  int qs = 0;                                            // causal: key j is seen by the queries i >= j - (S - L)
  if (a.causal && j0 - (a.S - a.L) > 0) qs = (j0 - (a.S - a.L)) / AT_COLS * AT_COLS;
  for (int q0 = qs; q0 < a.L; q0 += AT_COLS) {
    const int i = q0 + 16 * w + c, qi = i < a.L ? i : a.L - 1;
    const at_f32x4 as = dot_block<T, D>(krow, Q + (long)qi * a.q.sr + g * E);      // register q: key 4 g + q, query i
    const at_f32x4 ap = dot_block<T, D>(vrow, G + (long)qi * a.dO.sr + g * E);
    const long at = ((long)b * a.H + h) * a.L + qi;
    const float lse = a.lse[at], delta = a.delta[at];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + 4 * g + q;
      const bool live = i < a.L && j < a.S;
      const bool keep = !thresh || !live || dropout_keep(seed, at_idx(a, b, h, i, j), thresh);
      float p, pt, dpd, ds;
      at_bwd_entry(a, at_score(a, as[q], b, i, j), lse, delta, ap[q], live, keep, thresh ? inv_keep : 1.f, p, pt, dpd, ds);
      Pt[(4 * g + q) * LDT + 16 * w + c] = from_f32<T>(pt);
      St[(4 * g + q) * LDT + 16 * w + c] = from_f32<T>(ds);
    }
    acc_staged<T, D>(dv, Pt, G + (long)q0 * a.dO.sr, a.dO.sr, a.L - q0, Xt);
    acc_staged<T, D>(dk, St, Q + (long)q0 * a.q.sr, a.q.sr, a.L - q0, Xt);
  }
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  at_store<T, D>(dk, a.dk, b, h, j0, a.S, one);
  at_store<T, D>(dv, a.dv, b, h, j0, a.S, one);
}

template <typename T, int D>
__global__ __launch_bounds__(AT_THREADS) void attn_weights_kernel(const smx_attn_args a) {
  constexpr int E = AtT<T>::E;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * AT_ROWS, j = blockIdx.y * AT_COLS + 16 * w + c, b = blockIdx.z;
  const int qi = i0 + c < a.L ? i0 + c : a.L - 1, kj = j < a.S ? j : a.S - 1;
  const uint32_t thresh = at_thresh(a);
  const uint64_t seed = thresh ? epoch_seed(a.drop_seed, a.epoch) : 0;
  const float inv_keep = 1.0f / (1.0f - a.drop_p);
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int h = 0; h < a.H; ++h) {
    const at_f32x4 acc = dot_block<T, D>(at_base<T>(a.q, b, h) + (long)qi * a.q.sr + g * E, at_base<T>(a.k, b, h) + (long)kj * a.k.sr + g * E);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + 4 * g + q;
      if (i >= a.L || j >= a.S) continue;
      const float s = at_score(a, acc[q], b, i, j), lse = a.lse[((long)b * a.H + h) * a.L + i];
      float p = (s != AT_NEG_INF && lse != AT_NEG_INF) ? expf(s - lse) : 0.f;
      if (thresh) p = dropout_keep(seed, at_idx(a, b, h, i, j), thresh) ? p * inv_keep : 0.f;
      sum[q] += p;
    }
  }
  const float inv_h = 1.0f / (float)a.H;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = i0 + 4 * g + q;
    if (i < a.L && j < a.S) a.weights[(long)b * a.w_sb + (long)i * a.ldw + j] = sum[q] * inv_h;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static bool at_d_ok(int D) { return D == 64 || D == 128 || D == 256 || D == 512; }

static int at_check_op(const char* fn, const char* name, const smx_attn_operand& o, int es, bool needed) {
  if (!o.p) return needed ? fail(SMX_EINVAL, "%s: %s is NULL", fn, name) : SMX_OK;
  if (o.sd != 1) return fail(SMX_EUNSUPPORTED, "%s: %s has stride %lld along D (must be contiguous)", fn, name, (long long)o.sd);
  if (!aligned16(o.p) || (o.sb * es) % 16 || (o.sr * es) % 16 || (o.sh * es) % 16)
    return fail(SMX_EUNSUPPORTED, "%s: %s rows are not 16-byte aligned", fn, name);
  return SMX_OK;
}

// which entry point validates (NOT the `pass` of smx_attn_plan_query, which names a launch: SMX_ATTN_PASS_*)
enum AtCall { AT_CALL_FWD, AT_CALL_BWD, AT_CALL_WEIGHTS, AT_CALL_PLAN };
// sizes, dtype, masks and the operands the call reads or writes; AT_CALL_PLAN requires no pointer.  The backward does not read o:
// it is neither required nor checked there.
static int at_check(const char* fn, const smx_attn_args* a, AtCall call) {
  SMX_REQUIRE(a, "%s: null descriptor", fn);
  SMX_REQUIRE(a->B >= 1 && a->L >= 1 && a->S >= 1 && a->H >= 1 && a->D >= 1, "%s: bad sizes", fn);
  SMX_REQUIRE(a->drop_p >= 0.f && a->drop_p < 1.f, "%s: 0 <= drop_p < 1", fn);
  if (a->dtype != SMX_F32 && a->dtype != SMX_BF16) return fail(SMX_EUNSUPPORTED, "%s: dtype %d (F32 or BF16)", fn, a->dtype);
  if (!at_d_ok(a->D)) return fail(SMX_EUNSUPPORTED, "%s: head dimension %d (64, 128, 256 or 512)", fn, a->D);
  if (a->B > 65535 || a->H > 65535 || (int64_t)a->B * a->H * a->L >= (int64_t)1 << 31)
    return fail(SMX_EUNSUPPORTED, "%s: B %d, H %d, L %d exceed the grid", fn, a->B, a->H, a->L);
  const int es = a->dtype == SMX_BF16 ? 2 : 4;
  const bool need = call != AT_CALL_PLAN;
  int rc;
  if ((rc = at_check_op(fn, "q", a->q, es, need))) return rc;
  if ((rc = at_check_op(fn, "k", a->k, es, need))) return rc;
  if ((rc = at_check_op(fn, "v", a->v, es, need && call != AT_CALL_WEIGHTS))) return rc;
  if (call == AT_CALL_FWD && (rc = at_check_op(fn, "o", a->o, es, true))) return rc;
  if ((rc = at_check_op(fn, "dO", a->dO, es, call == AT_CALL_BWD))) return rc;
  if ((rc = at_check_op(fn, "dq", a->dq, es, call == AT_CALL_BWD))) return rc;
  if ((rc = at_check_op(fn, "dk", a->dk, es, call == AT_CALL_BWD))) return rc;
  if ((rc = at_check_op(fn, "dv", a->dv, es, call == AT_CALL_BWD))) return rc;
  if (need) {
    SMX_REQUIRE(a->lse, "%s: lse is NULL", fn);
    SMX_REQUIRE(call != AT_CALL_BWD || a->delta, "%s: delta (B H L floats of workspace) is NULL", fn);
    SMX_REQUIRE(call != AT_CALL_WEIGHTS || (a->weights && a->ldw >= a->S && a->w_sb >= 0), "%s: weights / ldw", fn);
    SMX_REQUIRE(!a->attn_bias || a->ldbias >= a->S, "%s: ldbias < S", fn);
    SMX_REQUIRE(!a->key_pad || a->ldpad >= a->S, "%s: ldpad < S", fn);
  }
  return SMX_OK;
}

#define AT_DISPATCH(KERNEL, grid)                                                                                   \
  dispatch_dtype(a->dtype, [&](auto tag) {                                                                          \
    using T = decltype(tag);                                                                                        \
    switch (a->D) {                                                                                                 \
      case 64: hipLaunchKernelGGL((KERNEL<T, 64>), grid, dim3(AT_THREADS), 0, STREAM, *a); break;                   \
      case 128: hipLaunchKernelGGL((KERNEL<T, 128>), grid, dim3(AT_THREADS), 0, STREAM, *a); break;                 \
      case 256: hipLaunchKernelGGL((KERNEL<T, 256>), grid, dim3(AT_THREADS), 0, STREAM, *a); break;                 \
      default: hipLaunchKernelGGL((KERNEL<T, 512>), grid, dim3(AT_THREADS), 0, STREAM, *a); break;                  \
    }                                                                                                               \
  })

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_attn_plan_query(const smx_attn_args* a, int pass, smx_attn_plan* plan) {
  SMX_REQUIRE(plan && pass >= SMX_ATTN_PASS_FWD && pass <= SMX_ATTN_PASS_WEIGHTS, "smx_attn_plan_query: plan is NULL or pass %d outside 0..3", pass);
  const int rc = at_check("smx_attn_plan_query", a, AT_CALL_PLAN);
  if (rc) return rc;
  const int es = a->dtype == SMX_BF16 ? 2 : 4;
  memset(plan, 0, sizeof(*plan));
  plan->rows = AT_ROWS;
  plan->key_tile = AT_COLS;
  plan->d_chunk = at_dchunk(a->D);
  plan->threads = AT_THREADS;
  plan->lds_bytes = at_lds_bytes(es, a->D, pass);
  plan->launches = pass == SMX_ATTN_PASS_BWD_DQ || pass == SMX_ATTN_PASS_BWD_DKV ? 2 : 1;
  plan->grid[0] = ((pass == SMX_ATTN_PASS_BWD_DKV ? a->S : a->L) + AT_ROWS - 1) / AT_ROWS;
  plan->grid[1] = pass == SMX_ATTN_PASS_WEIGHTS ? (a->S + AT_COLS - 1) / AT_COLS : a->H;
  plan->grid[2] = a->B;
  return SMX_OK;
}

extern "C" int smx_attn_fwd(const smx_attn_args* a, void* stream) {
  const int rc = at_check("smx_attn_fwd", a, AT_CALL_FWD);
  if (rc) return rc;
  const dim3 grid((a->L + AT_ROWS - 1) / AT_ROWS, a->H, a->B);
  AT_DISPATCH(attn_fwd_kernel, grid);
  return check_launch("smx_attn_fwd");
}

extern "C" int smx_attn_bwd(const smx_attn_args* a, void* stream) {
  const int rc = at_check("smx_attn_bwd", a, AT_CALL_BWD);
  if (rc) return rc;
  const dim3 gq((a->L + AT_ROWS - 1) / AT_ROWS, a->H, a->B), gk((a->S + AT_ROWS - 1) / AT_ROWS, a->H, a->B);
  AT_DISPATCH(attn_bwd_dq_kernel, gq);
  AT_DISPATCH(attn_bwd_dkv_kernel, gk);
  return check_launch("smx_attn_bwd");
}

extern "C" int smx_attn_weights(const smx_attn_args* a, void* stream) {
  const int rc = at_check("smx_attn_weights", a, AT_CALL_WEIGHTS);
  if (rc) return rc;
  const dim3 grid((a->L + AT_ROWS - 1) / AT_ROWS, (a->S + AT_COLS - 1) / AT_COLS, a->B);
  AT_DISPATCH(attn_weights_kernel, grid);
  return check_launch("smx_attn_weights");
}
