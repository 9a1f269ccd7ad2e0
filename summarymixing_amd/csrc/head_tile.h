// head_tile.h — the one fused vocabulary-head tile: z = X W^T on a 128-row x 128-column tile whose epilogue keeps a row's statistics
// and never stores z.  Users: tj_stats_kernel / tj_grad_kernel (transducer.hip) and ctc_head_kernel (ctcdec.hip).
//
// 4 waves (2 x 2) of 64 x 64, 32 x 32 MFMA fragments.  MFMA operand a = W (columns v), b = X (rows n): lane l holds row n = l % 32 of
// each fragment, accumulator register r column v = 8 (r / 4) + 4 (l / 32) + r % 4 (head_col).  A row's reductions over v are
// in-thread, then across the two lane halves and the two waves that share its rows (head_row_meet).  BK: 64 (bf16,
// v_mfma_f32_32x32x16_bf16) / 32 (fp32, v_mfma_f32_32x32x2_f32) reduce elements per LDS stage; the next stage is fetched into
// registers while this one is multiplied.
#pragma once
#include "gemm_common.h"

namespace smx {

static constexpr int HEAD_TILE = 128;                   // rows and columns of a tile
typedef __attribute__((ext_vector_type(4))) uint32_t head_u32x4;

template <typename T>
struct HeadTile {
  static constexpr int BK = sizeof(T) == 2 ? 64 : 32, PAD = sizeof(T) == 2 ? 8 : 4;
  static constexpr int LDK = BK + PAD;                                          // LDS row stride (elements; 16-byte multiple)
  static constexpr int CPR = BK * (int)sizeof(T) / 16;                          // 16-byte chunks per operand row and stage
  static constexpr int NLD = HEAD_TILE * CPR / 256;                             // chunks per thread and operand
  static constexpr int OP_BYTES = HEAD_TILE * LDK * (int)sizeof(T);
};

// the tile-local column of accumulator register r of fragment i, for wave column wv and lane half hi (r = 4 q: the first of the 4
// consecutive columns of group q)
__device__ __forceinline__ int head_col(int wv, int i, int r, int hi) { return wv * 64 + i * 32 + 8 * (r >> 2) + 4 * hi + (r & 3); }

// acc[i][j]: fragment i of the wave's 64 columns, fragment j of its 64 rows, of X[n0 .., :K] (leading dimension ldx) times
// W[v0 .., :K]^T.  K % 64 == 0; X, ldx and W 16-byte aligned.  smem: 2 * OP_BYTES.  The edges are CLAMPED: rows >= N re-read row
// N - 1 and columns >= V re-read column V - 1 (N, V >= 1); the epilogues never let either reach an output.
template <typename T>
__device__ __forceinline__ void head_mainloop(const T* __restrict__ X, long ldx, const T* __restrict__ W, int N, int V, int K, int n0,
                                              int v0, char* smem, f32x16 (&acc)[2][2]) {
  using TT = HeadTile<T>;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wv = wave & 1, wn = wave >> 1, l31 = lane & 31, hi = lane >> 5;
  char* Xs = smem;
  char* Ws = smem + TT::OP_BYTES;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  head_u32x4 rx[TT::NLD], rw[TT::NLD];             // (a first-class vector: the loads below are values, not struct copies)
  auto load = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < TT::NLD; ++p) {
      const int idx = t + 256 * p, r = idx / TT::CPR, c = idx % TT::CPR;
      const int n = min(n0 + r, N - 1), v = min(v0 + r, V - 1);
      rx[p] = *reinterpret_cast<const head_u32x4*>(reinterpret_cast<const char*>(X + (long)n * ldx + k0) + c * 16);
      rw[p] = *reinterpret_cast<const head_u32x4*>(reinterpret_cast<const char*>(W + (long)v * K + k0) + c * 16);
    }
  };
  const int nk = K / TT::BK;
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                                     // the previous stage has been read
#pragma unroll
    for (int p = 0; p < TT::NLD; ++p) {
      const int idx = t + 256 * p, r = idx / TT::CPR, c = idx % TT::CPR;
      *reinterpret_cast<head_u32x4*>(Xs + r * TT::LDK * (int)sizeof(T) + c * 16) = rx[p];
      *reinterpret_cast<head_u32x4*>(Ws + r * TT::LDK * (int)sizeof(T) + c * 16) = rw[p];
    }
    __syncthreads();
    if (kt + 1 < nk) load((kt + 1) * TT::BK);
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int kk = 0; kk < TT::BK / 16; ++kk) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
          fa[i] = *reinterpret_cast<const bf16x8*>(Ws + ((wv * 64 + i * 32 + l31) * TT::LDK + kk * 16 + hi * 8) * 2);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          fb[j] = *reinterpret_cast<const bf16x8*>(Xs + ((wn * 64 + j * 32 + l31) * TT::LDK + kk * 16 + hi * 8) * 2);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    } else {
      const float* Wf = reinterpret_cast<const float*>(Ws);
      const float* Xf = reinterpret_cast<const float*>(Xs);
      // fp32 operands: each stage is summed on its own and then added to the running sum.  One chain over the whole of K rounds
      // K / 2 times in a row (x2 MFMAs); at K = 1088 that put lse / lp / dz 4 - 7 x further from fp64 than a blocked fp32 product
      // (tests/test_transducer_kernels_gpu.py).  Two levels round BK / 2 + K / BK times.
      f32x16 st[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) st[i][j][e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < TT::BK / 2; ++kk) {
        float fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = Wf[(wv * 64 + i * 32 + l31) * TT::LDK + kk * 2 + hi];
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = Xf[(wn * 64 + j * 32 + l31) * TT::LDK + kk * 2 + hi];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) st[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], st[i][j], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] += st[i][j];
    }
  }
}

// ---- what a thread knows of a row after its 32 columns of the tile.  a.meet(b) folds in b, whose columns all lie above a's.
// (max, sum exp(z - max)): the transducer's
struct LseStat {
  float m, s;
  __device__ __forceinline__ LseStat other_half() const { return {__shfl_xor(m, 32, 64), __shfl_xor(s, 32, 64)}; }
  __device__ __forceinline__ void meet(const LseStat& o) {
    const float M = fmaxf(m, o.m);
    s = lse_rescale(s, m, M) + lse_rescale(o.s, o.m, M);
    m = M;
  }
};
// (max, first arg-max, sum exp(z - max)): the CTC head's.  A NaN logit never wins the maximum and makes the sum a NaN.
struct ArgLseStat {
  float m;
  int k;
  float s;
  __device__ __forceinline__ ArgLseStat other_half() const { return {__shfl_xor(m, 32, 64), __shfl_xor(k, 32, 64), __shfl_xor(s, 32, 64)}; }
  __device__ __forceinline__ void meet(const ArgLseStat& o) {
    float M = m;
    int K = k;
    argmax_take(M, K, o.m, o.k);
    s = (__builtin_isnan(s) || __builtin_isnan(o.s)) ? __builtin_nanf("") : lse_rescale(s, m, M) + lse_rescale(o.s, o.m, M);
    m = M;
    k = K;
  }
};

// The fixed-order meet of a row's four partial statistics.  thread_stat(j) gives this thread's, for row fragment j.  Each meets
// the other lane half's at once (same row, the other 4-column groups; lower half first, so both halves end with the same bits),
// which also keeps the two fragments' exponentials apart in the schedule.  Then the two waves of a row pair: wave wv = 1 parks its
// result in red (HEAD_TILE entries of LDS), wave wv = 0 folds it in (column order) and calls write(nl, stat) once per tile-local
// row nl.  Every thread of the workgroup must call it (one barrier).
template <typename S, typename C, typename F>
__device__ __forceinline__ void head_row_meet(S* red, C&& thread_stat, F&& write) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wv = wave & 1, wn = wave >> 1, l31 = lane & 31, hi = lane >> 5;
  S st[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const S mine = thread_stat(j), o = mine.other_half();
    st[j] = hi ? o : mine;
    st[j].meet(hi ? mine : o);
  }
  if (wv == 1 && hi == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) red[wn * 64 + j * 32 + l31] = st[j];
  }
  __syncthreads();
  if (wv == 0 && hi == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = wn * 64 + j * 32 + l31;
      st[j].meet(red[nl]);
      write(nl, st[j]);
    }
  }
}

}  // namespace smx
