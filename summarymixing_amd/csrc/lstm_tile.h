// lstm_tile.h — what the prediction network's kernels (lstm.hip) and the greedy decoder's (greedy.hip) share: the 16 x 16 MFMA tile
// product on operands read straight from memory, the supported hidden sizes and the one-hot column rule.
#pragma once
#include "gemm_common.h"

namespace smx {

typedef __attribute__((ext_vector_type(4))) float lstm_f32x4;

static constexpr int LSTM_H_MAX = 4096;
static inline bool lstm_h_ok(int H) { return H >= 32 && H <= LSTM_H_MAX && H % 32 == 0; }

// acc (16 x 16: row = 4 (lane >> 4) + reg, column = lane & 15) = A (16 x K) . Bm (16 x K)^T, both K-contiguous; a_row / b_row are this
// lane's row (lane & 15) of each.  Each lane fetches 16 bytes per operand and block: bf16 - the 8
// reduce indices of one 16x16x32 MFMA; f32 - 4 reduce indices spent on 4 MFMAs (slot (i, q) holds k = 16 blk + 4 q + i in both
// operands, so the pairing is right whatever the order).  Two (bf16) / four (f32) accumulators hide the dependent-MFMA latency.
// A tile row beyond B reads row B - 1 again (in bounds; its results are never stored).  The 16-byte loads need 16-byte aligned
// rows: the entry points check the base pointers, and every offset added to them (a step u H, a batch row b U H, a gate w H, a
// weight row of H or 4 H elements) is a multiple of H elements = of 64 bytes at least, since H % 32 == 0.
__device__ __forceinline__ lstm_f32x4 tile_dot(const bf16_t* a_row, const bf16_t* b_row, int K, int q) {
  lstm_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  a_row += 8 * q;
  b_row += 8 * q;
  int k0 = 0;
  for (; k0 + 64 <= K; k0 += 64) {
    const uint4 a0 = *reinterpret_cast<const uint4*>(a_row + k0), a1 = *reinterpret_cast<const uint4*>(a_row + k0 + 32);
    const uint4 b0 = *reinterpret_cast<const uint4*>(b_row + k0), b1 = *reinterpret_cast<const uint4*>(b_row + k0 + 32);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a0), __builtin_bit_cast(bf16x8, b0), acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a1), __builtin_bit_cast(bf16x8, b1), acc1, 0, 0, 0);
  }
  if (k0 < K) {                                                               // (K = 32 mod 64)
    const uint4 a0 = *reinterpret_cast<const uint4*>(a_row + k0), b0 = *reinterpret_cast<const uint4*>(b_row + k0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a0), __builtin_bit_cast(bf16x8, b0), acc0, 0, 0, 0);
  }
  return acc0 + acc1;
}
__device__ __forceinline__ lstm_f32x4 tile_dot(const float* a_row, const float* b_row, int K, int q) {
  lstm_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
  a_row += 4 * q;
  b_row += 4 * q;
  for (int k0 = 0; k0 < K; k0 += 16) {
    const float4 a = *reinterpret_cast<const float4*>(a_row + k0);
    const float4 b = *reinterpret_cast<const float4*>(b_row + k0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc1, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc2, 0, 0, 0);
    acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc3, 0, 0, 0);
  }
  return (acc0 + acc1) + (acc2 + acc3);
}

// ---- the one-hot input.  col(k) = k below the blank, k - 1 above it, none for the blank (or a token outside the vocabulary) ---
__device__ __forceinline__ int onehot_col(int tok, int V, int blank) {
  if (tok < 0 || tok >= V || tok == blank) return -1;
  return tok < blank ? tok : tok - 1;
}

}  // namespace smx
