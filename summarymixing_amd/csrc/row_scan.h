// row_scan.h — the one-wave-per-row pass over a row of scores: users seqloss.hip (the forward reads with row_scan; the backward, whose
// row is optional and which writes group by group, walks the same geometry with Grp16 and ROW_DEPTH), ctcdec.hip (best path) and the
// seq2seq selection kernels (attn_step.hip, beam.hip), whose reading of a row (SelRow) is below.
#pragma once
#include "smx_common.h"

#include <limits.h>

namespace smx {

static constexpr int ROW_DEPTH = 4;                     // 16-byte groups a lane has in flight

// 16 bytes of a row <-> floats: 4 fp32 or 8 bf16
template <typename T>
struct Grp16;
template <>
struct Grp16<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float (&f)[4]) { load4<float>(p, f); }
  static __device__ __forceinline__ void store(float* p, const float (&f)[4]) { store4<float>(p, f); }
};
template <>
struct Grp16<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float (&f)[8]) {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    f[0] = bf16_bits_to_f32(r.x & 0xffffu); f[1] = bf16_bits_to_f32(r.x >> 16);
    f[2] = bf16_bits_to_f32(r.y & 0xffffu); f[3] = bf16_bits_to_f32(r.y >> 16);
    f[4] = bf16_bits_to_f32(r.z & 0xffffu); f[5] = bf16_bits_to_f32(r.z >> 16);
    f[6] = bf16_bits_to_f32(r.w & 0xffffu); f[7] = bf16_bits_to_f32(r.w >> 16);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&f)[8]) {
    uint4 r;
    r.x = pack_bf16x2(f[0], f[1]); r.y = pack_bf16x2(f[2], f[3]); r.z = pack_bf16x2(f[4], f[5]); r.w = pack_bf16x2(f[6], f[7]);
    *reinterpret_cast<uint4*>(p) = r;
  }
};

// One wave reads the row x[0, V): the row is cut into 16-byte groups anchored at column 0, group k to lane k % 64, and a tail of
// V % N columns.  f(values, c0) is called with the N = Grp16<T>::N values of a group (first column c0), in increasing c0 per lane,
// then with single tail values (N = 1).  ROW_DEPTH groups of a lane are requested before the first is consumed (one wave per row:
// the loads in flight per lane are what hides the memory latency).  A row whose address is 16-byte aligned loads a group at once,
// any other row loads the same group element by element: the lanes see the same values in the same order, so the two paths give
// the same bits.
template <typename T, typename F>
__device__ __forceinline__ void row_scan(const T* x, int V, int lane, F&& f) {
  constexpr int N = Grp16<T>::N;
  const int Vv = V - V % N;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
  for (int c0 = lane * N; c0 < Vv; c0 += 64 * N * ROW_DEPTH) {
    float g[ROW_DEPTH][N];
#pragma unroll
    for (int d = 0; d < ROW_DEPTH; ++d) {
      const int c = c0 + d * 64 * N;
      if (c < Vv) {
        if (vec) Grp16<T>::load(x + c, g[d]);
        else {
#pragma unroll
          for (int j = 0; j < N; ++j) g[d][j] = to_f32(x[c + j]);
        }
      }
    }
#pragma unroll
    for (int d = 0; d < ROW_DEPTH; ++d) {
      const int c = c0 + d * 64 * N;
      if (c < Vv) f(g[d], c);
    }
  }
  for (int c = Vv + lane; c < V; c += 64) {              // the tail: fewer than N columns
    const float g[1] = {to_f32(x[c])};
    f(g, c);
  }
}

// ---- the selection kernels' reading of a row of logits (attn_step.hip: smx_s2s_select; beam.hip: smx_s2s_beam_select)
// what one lane has seen of its row: the running arg-max over the columns that take part, the online (max, sum exp((z - max) / T))
// over the entries that are numbers, and whether any entry was a NaN
struct SelRow {
  float bv; int bi;
  float m, s;
  int nan;
};

// (the exponent is formed in fp64 from the ONE inverse temperature the whole kernel uses, then rounded once for expf)
template <int N>
__device__ __forceinline__ void sel_row_take(SelRow& r, const float (&x)[N], int c0, int skip, double inv_temp) {
  float gm = NEG_INF;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (c0 + j != skip) argmax_take(r.bv, r.bi, x[j], c0 + j);
    if (x[j] > gm) gm = x[j];
    r.nan |= __builtin_isnan(x[j]) ? 1 : 0;
  }
  if (gm > r.m) {
    r.s = r.m == NEG_INF ? 0.f : r.s * expf((float)((double)(r.m - gm) * inv_temp));
    r.m = gm;
  }
  if (r.m != NEG_INF) {
#pragma clang fp reassociate(off)
#pragma unroll
    for (int j = 0; j < N; ++j) r.s += __builtin_isnan(x[j]) ? 0.f : expf((float)((double)(x[j] - r.m) * inv_temp));
  }
}

}  // namespace smx
