// resample.hip — the recipes' wav_augment (speechbrain.augment.time_domain.SpeedPerturb -> Resample: torchaudio's polyphase
// windowed-sinc filter, sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) as one launch.  smx_resample_plan builds the tap
// table on the host; smx_resample is one pass over the waveform.  Image layout: include/smx.h.  Arithmetic spec: DESIGN.md §I.16.
#include <cmath>
#include <cstdint>
#include <vector>

#include "smx_common.h"

namespace smx {

#define STREAM reinterpret_cast<hipStream_t>(stream)

constexpr int RS_HDR = 8;                  // header words of the plan image
constexpr int RS_XS = 4096;                // staged input samples per workgroup (LDS floats)
static_assert(RS_XS == 4 * 4 * 256, "a thread stages four 16-byte vectors of the span");
constexpr int RS_XS4 = RS_XS / 4;          // a multiple of 32: the four residue planes of s_x start on the same bank
constexpr int RS_TABLE = 8192;             // most table floats (n * taps)
constexpr int RS_TAB = RS_TABLE + 768;     // + the padding of the swizzled layout (n >= 32: at most 3 phases x 256 taps)
constexpr int RS_MAXN = 1024;              // most phases (first[] lives in LDS as 16-bit)
constexpr int RS_NOMINAL = 3968;           // input samples per workgroup the launch assumes when it sizes the grid

// Sample a of the staged span lives at (a % 4) * RS_XS4 + a / 4.  A thread owns four consecutive outputs, so neighbouring lanes read
// samples about four apart: in this layout they fall on neighbouring banks (plain order would put 32 lanes on 8 banks).
__device__ __forceinline__ int rs_xi(int a) { return (a & 3) * RS_XS4 + (a >> 2); }

// blocks of n outputs per workgroup tile: the span Q * o + K + taps (+ 3 for the 16-byte alignment of its start) fits s_x
__host__ __device__ __forceinline__ int rs_tile_blocks(int o, int K, int taps) { return (RS_XS - K - taps - 3) / o; }

// One workgroup: tiles of Q whole n-sample output blocks of row blockIdx.y (tile = blockIdx.x, + gridDim.x while tiles remain; the
// launch sizes the grid so that the recipes' ratios take one tile per workgroup).  The table is staged once, as [k][p] with the
// phases of one residue mod 4 contiguous (n >= 32; below that every phase has a bank of its own in plain order); the input span
// [q0 * o - width, + (Qt - 1) * o + K + taps), zero outside [0, L), once per tile.  VIN / VOUT: 16-byte global loads / stores.
template <bool VIN, bool VOUT>
__global__ void __launch_bounds__(256) resample_kernel(const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy,
                                                       const int32_t* __restrict__ plan, int64_t L) {
#pragma clang fp reassociate(off)
  __shared__ float s_x[RS_XS];
  __shared__ float s_w[RS_TAB];
  __shared__ uint16_t s_first[RS_MAXN];
  const int tid = threadIdx.x;
  const int o = plan[0], n = plan[1], width = plan[2], K = plan[3], taps = plan[4], Q = plan[5];
  const int np4 = n >= 32 ? (n + 3) >> 2 : 0, np = np4 ? 4 * np4 : n;
  // (a block that is not a plan: nothing is read or written out of bounds, nothing is computed)
  if (o < 1 || n < 1 || n > RS_MAXN || width < 0 || K < 1 || taps < 1 || taps > K || (int64_t)taps * np > RS_TAB || Q < 1 ||
      Q > rs_tile_blocks(o, K, taps))
    return;
  const int32_t* first = plan + RS_HDR;
  const float* w = reinterpret_cast<const float*>(plan + RS_HDR + n);
  // (called once, behind the first tile's input loads, so that the table's memory latency is paid beside theirs)
  auto stage_table = [&]() {
    for (int idx = tid; idx < n * taps; idx += 256) {
      const int p = idx / taps, j = idx - p * taps;
      s_w[j * np + (np4 ? (p & 3) * np4 + (p >> 2) : p)] = w[idx];
    }
    for (int p = tid; p < n; p += 256) s_first[p] = (uint16_t)min(max(first[p], 0), K);
  };
  const int64_t L_out = (n * L + o - 1) / o;
  const int64_t nblk = (L_out + n - 1) / n, ntiles = (nblk + Q - 1) / Q;
  const float* Xb = X + (int64_t)blockIdx.y * ldx;
  float* Yb = Y + (int64_t)blockIdx.y * ldy;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t q0 = tile * Q;
    const int Qt = (int)min((int64_t)Q, nblk - q0);
    const int64_t in0 = q0 * o - width, a0 = in0 & ~(int64_t)3;     // the staged span starts on a multiple of four samples
    const int shift = (int)(in0 - a0), span = shift + (Qt - 1) * o + K + taps;
    if (tile != blockIdx.x) __syncthreads();                        // the previous tile's readers are done with s_x
    if (VIN) {
      // the span is at most RS_XS / 4 = 4 x 256 vectors: a thread's four loads are issued together and waited for once (one after
      // the other, each behind the LDS writes of the one before, the tile paid four memory latencies)
      float4 x4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v = tid + 256 * k;
        const int64_t s = a0 + 4 * v;
        x4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * v < span && s >= 0 && s + 3 < L) x4[k] = *reinterpret_cast<const float4*>(Xb + s);
      }
      if (tile == blockIdx.x) stage_table();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v = tid + 256 * k;
        const int64_t s = a0 + 4 * v;
        if (4 * v < span && !(s >= 0 && s + 3 < L)) {               // a vector across 0 or L: element by element
          x4[k].x = (s >= 0 && s < L) ? Xb[s] : 0.f;
          x4[k].y = (s + 1 >= 0 && s + 1 < L) ? Xb[s + 1] : 0.f;
          x4[k].z = (s + 2 >= 0 && s + 2 < L) ? Xb[s + 2] : 0.f;
          x4[k].w = (s + 3 >= 0 && s + 3 < L) ? Xb[s + 3] : 0.f;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v = tid + 256 * k;
        if (4 * v < span) { s_x[v] = x4[k].x; s_x[RS_XS4 + v] = x4[k].y; s_x[2 * RS_XS4 + v] = x4[k].z; s_x[3 * RS_XS4 + v] = x4[k].w; }
      }
    } else {
      if (tile == blockIdx.x) stage_table();
      for (int a = tid; a < span; a += 256) {
        const int64_t s = a0 + a;
        s_x[rs_xi(a)] = (s >= 0 && s < L) ? Xb[s] : 0.f;
      }
    }
    __syncthreads();
    // outputs [i_beg, i_end) of the row, in groups of four on multiples of four of the row index (so a whole group is one 16-byte store)
    const int64_t i_beg = q0 * n, i_end = min((q0 + Qt) * n, L_out);
    for (int64_t g = (i_beg >> 2) + tid; 4 * g < i_end; g += 256) {
      int xoff[4], woff[4];
      bool ok[4];
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      const int li0 = (int)(4 * g - i_beg), last = Qt * n - 1;      // li0: -3 .. last
      int li = max(li0, 0);                                         // this output's index in the tile, clamped into it
      int qq = li / n, p = li - qq * n;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t i = 4 * g + e;
        ok[e] = i >= i_beg && i < i_end;
        xoff[e] = qq * o + s_first[p] + shift;
        woff[e] = np4 ? (p & 3) * np4 + (p >> 2) : p;
        if (li0 + e + 1 > li && li < last) {                        // the next output, clamped likewise
          ++li;
          if (++p == n) { p = 0; ++qq; }
        }
      }
      // ascending k, one fused multiply-add per tap, float32: the order is fixed, so two runs give the same bits and a unit impulse
      // returns the taps themselves.  Four taps a round: tap j = 4 jb + r of an output reads plane (xoff + r) % 4 at (xoff + r) / 4 + jb, so the sixteen addresses
      // of a round are computed once and step by one word, and the loads of a round are in flight together
      int xb[4][4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int r = 0; r < 4; ++r) xb[e][r] = rs_xi(xoff[e] + r);
      }
      int j = 0;
      for (; j + 4 <= taps; j += 4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(s_w[woff[e] + r * np], s_x[xb[e][r]], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          woff[e] += 4 * np;
#pragma unroll
          for (int r = 0; r < 4; ++r) ++xb[e][r];
        }
      }
      for (int r = 0; j < taps; ++j, ++r) {                         // the last taps % 4 (woff has moved on to tap j - r)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(s_w[woff[e] + r * np], s_x[rs_xi(xoff[e] + j)], acc[e]);
      }
      if (VOUT && ok[0] && ok[3]) {
        *reinterpret_cast<float4*>(Yb + 4 * g) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (ok[e]) Yb[4 * g + e] = acc[e];
      }
    }
  }
}

// h[p][k] in float64 (libm), as torchaudio's _get_sinc_resample_kernel with its defaults evaluates it in float64.  optnone: the
// library is built with -ffast-math, and these are the reference's operations one by one.
__attribute__((optnone)) static double rs_tap(int o, int n, int width, double base, int p, int k) {
  const double pi = 3.14159265358979323846;
  double t = ((double)(k - width) / (double)o - (double)p / (double)n) * base;
  t = t < -6.0 ? -6.0 : (t > 6.0 ? 6.0 : t);
  const double c = std::cos(t * pi / 6.0 / 2.0);
  const double a = t * pi;
  const double s = a == 0.0 ? 1.0 : std::sin(a) / a;
  return s * ((c * c) * (base / (double)o));
}

__attribute__((optnone)) static int rs_width(int o, double base) { return (int)std::ceil(6.0 * (double)o / base); }

}  // namespace smx

using namespace smx;

extern "C" int smx_resample_plan(int orig_freq, int new_freq, int32_t* info, size_t* image_bytes, void* image, size_t image_capacity) {
  SMX_REQUIRE(info, "smx_resample_plan: null info");
  for (int i = 0; i < RS_HDR; ++i) info[i] = 0;
  if (image_bytes) *image_bytes = 0;
  if (orig_freq <= 0 || new_freq <= 0) return fail(SMX_EUNSUPPORTED, "smx_resample_plan: rates must be positive, got %d -> %d", orig_freq, new_freq);
  int a = orig_freq, b = new_freq;
  while (b) { const int r = a % b; a = b; b = r; }
  const int o = orig_freq / a, n = new_freq / a;
  const double base = (double)(o < n ? o : n) * 0.99;
  const int width = rs_width(o, base);
  const int64_t K64 = 2 * (int64_t)width + o;
  info[0] = o; info[1] = n; info[2] = width; info[3] = (int32_t)(K64 < INT32_MAX ? K64 : INT32_MAX);
  // every phase holds at least 8 nonzero taps, so more than 1024 phases cannot fit the table: refused before the taps are evaluated
  if (n > RS_MAXN) return fail(SMX_EUNSUPPORTED, "smx_resample_plan: %d -> %d: n * taps > %d table floats (n = %d)", orig_freq, new_freq, RS_TABLE, n);
  if (K64 + o + 3 > RS_XS) return fail(SMX_EUNSUPPORTED, "smx_resample_plan: %d -> %d: K + o = %lld input samples do not fit one workgroup's span (%d)", orig_freq, new_freq, (long long)(K64 + o), RS_XS);
  const int K = (int)K64;
  std::vector<float> h((size_t)n * K);
  std::vector<int> lo(n), hi(n);
  int taps = 1;
  for (int p = 0; p < n; ++p) {
    lo[p] = K; hi[p] = -1;
    for (int k = 0; k < K; ++k) {
      const float v = (float)rs_tap(o, n, width, base, p, k);
      h[(size_t)p * K + k] = v;
      if (v != 0.0f) { if (k < lo[p]) lo[p] = k; hi[p] = k; }
    }
    if (hi[p] < 0) lo[p] = 0;
    if (hi[p] - lo[p] + 1 > taps) taps = hi[p] - lo[p] + 1;
  }
  info[4] = taps;
  if ((int64_t)n * taps > RS_TABLE) return fail(SMX_EUNSUPPORTED, "smx_resample_plan: %d -> %d: n * taps = %d * %d > %d table floats", orig_freq, new_freq, n, taps, RS_TABLE);
  const int Q = rs_tile_blocks(o, K, taps);
  if (Q < 1) return fail(SMX_EUNSUPPORTED, "smx_resample_plan: %d -> %d: K + taps + o input samples do not fit one workgroup's span (%d)", orig_freq, new_freq, RS_XS);
  info[5] = Q;
  const size_t bytes = sizeof(int32_t) * ((size_t)RS_HDR + n + (size_t)n * taps);
  if (image_bytes) *image_bytes = bytes;
  if (!image) return SMX_OK;
  SMX_REQUIRE(image_capacity >= bytes, "smx_resample_plan: the image needs %zu bytes, the buffer holds %zu", bytes, image_capacity);
  int32_t* img = static_cast<int32_t*>(image);
  for (int i = 0; i < RS_HDR; ++i) img[i] = info[i];
  float* wt = reinterpret_cast<float*>(img + RS_HDR + n);
  for (int p = 0; p < n; ++p) {
    img[RS_HDR + p] = lo[p];
    for (int j = 0; j < taps; ++j) wt[(size_t)p * taps + j] = lo[p] + j <= hi[p] ? h[(size_t)p * K + lo[p] + j] : 0.0f;
  }
  return SMX_OK;
}

extern "C" int smx_resample(const float* X, int64_t ldx, float* Y, int64_t ldy, const int32_t* plan, int B, int64_t L, void* stream) {
  SMX_REQUIRE(X && Y && plan && B > 0, "smx_resample: null pointer or B < 1");
  SMX_REQUIRE(L >= 1 && ldx >= L && ldy >= 1, "smx_resample: L < 1 or a leading dimension below the row length");
  SMX_REQUIRE(L <= ((int64_t)1 << 40), "smx_resample: L above 2^40");
  if (X == Y) return fail(SMX_EUNSUPPORTED, "smx_resample: in place (X == Y) is not supported: samples are gathered");
  if (B > 65535) return fail(SMX_EUNSUPPORTED, "smx_resample: B = %d > 65535", B);
  const bool vin = aligned16(X) && ldx % 4 == 0, vout = aligned16(Y) && ldy % 4 == 0;
  int64_t gx = (L + RS_NOMINAL - 1) / RS_NOMINAL;
  gx = gx > (1 << 20) ? (1 << 20) : gx;
  const dim3 grid((unsigned)gx, (unsigned)B);
  if (vin && vout) hipLaunchKernelGGL((resample_kernel<true, true>), grid, dim3(256), 0, STREAM, X, ldx, Y, ldy, plan, L);
  else if (vin) hipLaunchKernelGGL((resample_kernel<true, false>), grid, dim3(256), 0, STREAM, X, ldx, Y, ldy, plan, L);
  else if (vout) hipLaunchKernelGGL((resample_kernel<false, true>), grid, dim3(256), 0, STREAM, X, ldx, Y, ldy, plan, L);
  else hipLaunchKernelGGL((resample_kernel<false, false>), grid, dim3(256), 0, STREAM, X, ldx, Y, ldy, plan, L);
  return check_launch("smx_resample");
}
