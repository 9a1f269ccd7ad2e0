// lstm_tile.h — the one home of the LSTM cell.  Shared by the prediction network (lstm.hip), the greedy decoder (greedy.hip) and the
// RNNLM decode step (lstm_step.hip): the 16 x 16 MFMA tile product on operands read straight from memory, the supported hidden sizes
// and the cell arithmetic (lstm_cell; lstm_cell_bwd for lstm.hip's BPTT).  lstm.hip and greedy.hip also share the four-waves-one-gate-
// each recurrent product (gate_tiles, gate_tile_to_lds) and the one-hot input (onehot_col, onehot_gate_input).
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
// its contribution to one gate pre-activation: keep W_ih^T[col, n] + bias[n] in ONE fma (wx = 0 without a column).  keep = 1 gives
// fl(wx + bias), the value the dense route's GEMM gives for a one-hot row - its fp32 sum is wx exactly.  The result is ROUNDED here:
// lstm.hip reads it back from memory, and without the empty asm -ffast-math lets greedy.hip, which adds it to the recurrent product in
// registers, regroup the sum as (red + wx) + bias - one ulp away from what the prediction network computes for the same token.
__device__ __forceinline__ float onehot_gate_input(float keep, float wx, float bias) {
  float g = fmaf(keep, wx, bias);
  asm("" : "+v"(g));                                                          // (no instruction: the optimiser cannot look through it)
  return g;
}

// ---- the recurrent product of a 16 (batch rows) x 16 (hidden units) state tile: four waves, one gate each (torch's order i, f, g, o)
// wave w's 16 x 16 accumulator -> red[w][row][column]
__device__ __forceinline__ void gate_tile_to_lds(float (&red)[4][16][17], const lstm_f32x4& acc, int w, int q, int r) {
#pragma unroll
  for (int i = 0; i < 4; ++i) red[w][q * 4 + i][r] = acc[i];
}
// red[w] = h_prev[b0 .. b0 + 15] . W_hh[w H + j0 .. w H + j0 + 15]^T for the workgroup's four waves, then the barrier: every thread may
// read all four tiles.  hp null (uniform): zeros, and W_hh is not read.
template <typename T>
__device__ __forceinline__ void gate_tiles(float (&red)[4][16][17], const T* hp, long ld_hp, const void* Whh, int H, int B, int b0, int j0) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  lstm_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (hp) {
    const T* a_row = hp + (long)min(b0 + r, B - 1) * ld_hp;
    const T* b_row = reinterpret_cast<const T*>(Whh) + ((long)w * H + j0 + r) * H;
    acc = tile_dot(a_row, b_row, H, q);
  }
  gate_tile_to_lds(red, acc, w, q, r);
  __syncthreads();
}

// ---- the cell, in fp32.  z: the four pre-activations (recurrent product + input contribution + biases); g <- the activated gates,
// c <- g_f c_prev + g_i g_g, returns h = g_o tanh(c) (the caller rounds it to its dtype).
__device__ __forceinline__ float lstm_cell(const float (&z)[4], float cprev, float (&g)[4], float& c) {
  g[0] = sigmoidf_(z[0]); g[1] = sigmoidf_(z[1]); g[2] = tanhf(z[2]); g[3] = sigmoidf_(z[3]);
  c = g[1] * cprev + g[0] * g[2];
  return g[3] * tanhf(c);
}
// The same cell undone from its saved gates and c: dz <- the gradients of the four pre-activations, returns the gradient of c_prev.
// dh: the whole gradient of h; dc_in: the gradient of c carried down from the step after.
__device__ __forceinline__ float lstm_cell_bwd(const float (&g)[4], float c, float cprev, float dh, float dc_in, float (&dz)[4]) {
  const float gi = g[0], gf = g[1], gg = g[2], go = g[3];
  const float tc = tanhf(c);
  const float dcv = dc_in + dh * go * (1.f - tc * tc);
  dz[0] = dcv * gg * gi * (1.f - gi);
  dz[1] = dcv * cprev * gf * (1.f - gf);
  dz[2] = dcv * gi * (1.f - gg * gg);
  dz[3] = dh * tc * go * (1.f - go);
  return dcv * gf;
}

}  // namespace smx
