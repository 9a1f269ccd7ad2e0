// tgt_embed.hip - the seq2seq decoder's target embedding (include/smx.h: smx_tgt_embed_fwd / smx_tgt_embed_bwd).
//
// Forward: one launch for NormalizedEmbedding (table[tok] * sqrt(d)) + the abs-sine rows + the key-padding flags; a thread owns 8
// consecutive columns of one row (two 16-byte table loads, two 16-byte PE loads, 16 or 32 bytes stored), consecutive threads walk a
// row and then the next one, so every access is coalesced except the row jump of the gather itself.
// Backward: no atomics.  One workgroup per vocabulary row v; each of its waves scans the token list 64 tokens at a time (one
// coalesced load + a ballot), then adds the rows that hold v in ascending row order - the order of the set bits.  A thread owns 8
// columns again; the gradient row is read and rewritten only when a token matched, so an unused row costs the scan alone
// (B U / 64 loads per wave; 5 000 rows x 5 120 tokens: 400 K wave loads, all L2 hits after the first workgroups).
#include "smx_common.h"

namespace smx {

template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&a)[4], const float (&b)[4]);
template <>
__device__ __forceinline__ void store8<float>(float* p, const float (&a)[4], const float (&b)[4]) {
  store4(p, a);
  store4(p + 4, b);
}
template <>
__device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float (&a)[4], const float (&b)[4]) {
  uint4 r;
  r.x = pack_bf16x2(a[0], a[1]); r.y = pack_bf16x2(a[2], a[3]);
  r.z = pack_bf16x2(b[0], b[1]); r.w = pack_bf16x2(b[2], b[3]);
  *reinterpret_cast<uint4*>(p) = r;
}
template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&a)[4], float (&b)[4]);
template <>
__device__ __forceinline__ void load8<float>(const float* p, float (&a)[4], float (&b)[4]) {
  load4(p, a);
  load4(p + 4, b);
}
template <>
__device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float (&a)[4], float (&b)[4]) {
  const uint4 r = *reinterpret_cast<const uint4*>(p);
  a[0] = bf16_bits_to_f32(r.x & 0xffffu); a[1] = bf16_bits_to_f32(r.x >> 16);
  a[2] = bf16_bits_to_f32(r.y & 0xffffu); a[3] = bf16_bits_to_f32(r.y >> 16);
  b[0] = bf16_bits_to_f32(r.z & 0xffffu); b[1] = bf16_bits_to_f32(r.z >> 16);
  b[2] = bf16_bits_to_f32(r.w & 0xffffu); b[3] = bf16_bits_to_f32(r.w >> 16);
}

template <typename T>
__global__ __launch_bounds__(256) void tgt_embed_fwd_kernel(const int32_t* __restrict__ tok, const float* __restrict__ table, long ldt,
                                                            const float* __restrict__ pe, long ldpe, T* __restrict__ Y, long ldy,
                                                            uint8_t* __restrict__ flags, long rows, int U, int V, int chunks, int pad_idx,
                                                            float scale) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  const long r = id / chunks;
  if (r >= rows) return;
  const int c = (int)(id - r * chunks) * 8;
  const int k = tok[r];
  const bool in = k >= 0 && k < V;                      // compared BEFORE the table is indexed
  float e0[4] = {0.f, 0.f, 0.f, 0.f}, e1[4] = {0.f, 0.f, 0.f, 0.f}, p0[4], p1[4];
  if (in) load8<float>(table + (long)k * ldt + c, e0, e1);
  load8<float>(pe + (r % U) * ldpe + c, p0, p1);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    e0[q] = fmaf(e0[q], scale, p0[q]);
    e1[q] = fmaf(e1[q], scale, p1[q]);
  }
  store8<T>(Y + r * ldy + c, e0, e1);
  if (c == 0) flags[r] = (in && k == pad_idx) ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(256) void tgt_embed_bwd_kernel(const int32_t* __restrict__ tok, const T* __restrict__ dY, long lddy,
                                                            float* __restrict__ gTable, long ldg, int rows, int D, int pad_idx,
                                                            float scale) {
  const int v = blockIdx.x;
  if (v == pad_idx) return;
  const int lane = threadIdx.x & 63;
  const int nthr = blockDim.x;
  // (a wave whose threads all sit beyond the last column chunk has nothing to add)
  if ((int)(threadIdx.x - lane) * 8 >= D) return;
  for (int c0 = 0; c0 < D; c0 += nthr * 8) {            // one trip for D <= 2048
    const int c = c0 + threadIdx.x * 8;
    const bool active = c < D;
    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
    bool any = false;
    for (int base = 0; base < rows; base += 64) {
      const int r = base + lane;
      const bool hit = r < rows && tok[r] == v;
      unsigned long long m = __ballot(hit);
      any = any || m != 0ull;
      while (m) {                                       // ascending row order: the lowest set bit first
        const int b = __ffsll(m) - 1;
        m &= m - 1ull;
        if (active) {
          float d0[4], d1[4];
          load8<T>(dY + (long)(base + b) * lddy + c, d0, d1);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            a0[q] += d0[q];
            a1[q] += d1[q];
          }
        }
      }
    }
    if (any && active) {
      float* g = gTable + (long)v * ldg + c;
      float g0[4], g1[4];
      load8<float>(g, g0, g1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        g0[q] = fmaf(scale, a0[q], g0[q]);
        g1[q] = fmaf(scale, a1[q], g1[q]);
      }
      store8<float>(g, g0, g1);
    }
  }
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_tgt_embed_fwd(int out_dtype, const int32_t* tok, const float* table, int64_t ldt, const float* pe, int64_t ldpe,
                                 void* Y, int64_t ldy, uint8_t* key_pad, int rows, int U, int V, int D, int pad_idx, void* stream) {
  SMX_REQUIRE(out_dtype == SMX_F32 || out_dtype == SMX_BF16, "smx_tgt_embed_fwd: bad output dtype %d", out_dtype);
  SMX_REQUIRE(tok && table && pe && Y && key_pad, "smx_tgt_embed_fwd: null pointer");
  SMX_REQUIRE(rows >= 0 && U >= 1 && V >= 1 && D >= 1 && ldt >= D && ldpe >= D && ldy >= D,
              "smx_tgt_embed_fwd: bad sizes rows=%d U=%d V=%d D=%d ldt=%lld ldpe=%lld ldy=%lld", rows, U, V, D, (long long)ldt,
              (long long)ldpe, (long long)ldy);
  if (D % 8 != 0 || ldt % 8 != 0 || ldpe % 8 != 0 || ldy % 8 != 0 || !aligned16(table) || !aligned16(pe) || !aligned16(Y))
    return fail(SMX_EUNSUPPORTED, "smx_tgt_embed_fwd: d and the leading dimensions must be multiples of 8 elements, the bases 16-byte aligned (d=%d)", D);
  if (rows == 0) return SMX_OK;
  const int chunks = D / 8;
  const long total = (long)rows * chunks;
  const long blocks = (total + 255) / 256;
  SMX_REQUIRE(blocks <= 0x7fffffffL, "smx_tgt_embed_fwd: rows x d too large (%d x %d)", rows, D);
  const float scale = sqrtf((float)D);
  dispatch_dtype(out_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(tgt_embed_fwd_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, STREAM, tok, table, (long)ldt, pe, (long)ldpe, (T*)Y,
                       (long)ldy, key_pad, (long)rows, U, V, chunks, pad_idx, scale);
  });
  return check_launch("smx_tgt_embed_fwd");
}

extern "C" int smx_tgt_embed_bwd(int dy_dtype, const int32_t* tok, const void* dY, int64_t lddy, float* gTable, int64_t ldg, int rows,
                                 int V, int D, int pad_idx, void* stream) {
  SMX_REQUIRE(dy_dtype == SMX_F32 || dy_dtype == SMX_BF16, "smx_tgt_embed_bwd: bad gradient dtype %d", dy_dtype);
  SMX_REQUIRE(tok && dY && gTable, "smx_tgt_embed_bwd: null pointer");
  SMX_REQUIRE(rows >= 0 && V >= 1 && D >= 1 && lddy >= D && ldg >= D, "smx_tgt_embed_bwd: bad sizes rows=%d V=%d D=%d lddy=%lld ldg=%lld", rows,
              V, D, (long long)lddy, (long long)ldg);
  if (D % 8 != 0 || lddy % 8 != 0 || ldg % 8 != 0 || !aligned16(dY) || !aligned16(gTable))
    return fail(SMX_EUNSUPPORTED, "smx_tgt_embed_bwd: d and the leading dimensions must be multiples of 8 elements, the bases 16-byte aligned (d=%d)", D);
  if (rows == 0) return SMX_OK;
  const int need = (D / 8 + 63) / 64 * 64;
  const int threads = need < 256 ? need : 256;
  const float scale = sqrtf((float)D);
  dispatch_dtype(dy_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(tgt_embed_bwd_kernel<T>, dim3((unsigned)V), dim3(threads), 0, STREAM, tok, (const T*)dY, (long)lddy, gTable, (long)ldg,
                       rows, D, pad_idx, scale);
  });
  return check_launch("smx_tgt_embed_bwd");
}
