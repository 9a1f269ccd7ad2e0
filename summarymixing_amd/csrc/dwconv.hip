// dwconv.hip — fused GLU + depthwise Conv1d over time (Conformer conv module) and the gated reflect-padded
// variant (Branchformer CSGU), forward and backward, gfx950.
//
// Tile = 64 frames x 64 channels per workgroup (256 threads: lane = channel, 4 waves x 16 frames).  The GLU'd
// input tile with its +-(k-1)/2 halo is built ONCE in LDS ([frame][channel] fp32: consecutive lanes hit
// consecutive banks, conflict free), so P is read from HBM exactly once per tile (+ halo) and u is never
// materialised in HBM.  Dynamic Chunk Convolution only changes a per-tap predicate.
#include "smx_common.h"

namespace smx {

constexpr int DW_TT = 64;      // frames per tile
constexpr int DW_CT = 64;      // channels per tile
constexpr int DW_KMAX = 33;    // max taps
constexpr int DW_ROWS = DW_TT + DW_KMAX - 1;

struct DwParams {
  const void* P; long ldp;
  const float* w; const float* bias;
  const void* gate; long ldg;
  void* Y; long ldy;          // fwd out / bwd: dY in
  void* dP; long lddp;
  void* dgate; long lddg;
  float* dw; float* dbias;
  int B, T, D, k, glu, pad_mode, chunk;
  unsigned dthresh; float dscale; uint64_t dseed; const uint64_t* epoch;   // fused dropout of the output (rolling CSGU forward only)
};

__device__ __forceinline__ int map_frame(int tau, int T, int pad_mode) {
  if (tau >= 0 && tau < T) return tau;
  if (pad_mode == SMX_PAD_REFLECT) {
    int r = tau < 0 ? -tau : 2 * (T - 1) - tau;
    return (r >= 0 && r < T) ? r : -1;
  }
  return -1;
}

// fill the u tile (rows t0-pad .. t0+TT+pad) for channel c of batch b
template <typename T>
__device__ __forceinline__ void fill_u(float (*u)[DW_CT], const DwParams& p, int b, int t0, int pad, int ch, int cl, int wv) {
  const T* P = reinterpret_cast<const T*>(p.P);
  const int rows = DW_TT + 2 * pad;
  for (int i = wv; i < rows; i += 4) {
    int src = map_frame(t0 - pad + i, p.T, p.pad_mode);
    float val = 0.f;
    if (src >= 0 && ch < p.D) {
      const T* row = P + ((long)b * p.T + src) * p.ldp;
      float a = to_f32(row[ch]);
      val = p.glu ? a * sigmoidf_(to_f32(row[p.D + ch])) : a;
    }
    u[i][cl] = val;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(DwParams p) {
  __shared__ float u[DW_ROWS][DW_CT];
  __shared__ float wl[DW_KMAX][DW_CT];
  const int cl = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ch = blockIdx.x * DW_CT + cl, t0 = blockIdx.y * DW_TT, b = blockIdx.z;
  const int pad = (p.k - 1) / 2;
  fill_u<T>(u, p, b, t0, pad, ch, cl, wv);
  for (int j = wv; j < p.k; j += 4) wl[j][cl] = ch < p.D ? p.w[(long)ch * p.k + j] : 0.f;
  __syncthreads();
  if (ch >= p.D) return;
  const float bs = p.bias ? p.bias[ch] : 0.f;
  float acc[16];
#pragma unroll
  for (int o = 0; o < 16; ++o) acc[o] = bs;
  const int f0 = wv * 16;
  if (p.chunk > 0) {
    for (int j = 0; j < p.k; ++j) {
      const float wj = wl[j][cl];
#pragma unroll
      for (int o = 0; o < 16; ++o) {
        int t = t0 + f0 + o, tau = t + j - pad;
        int lim = (t / p.chunk + 1) * p.chunk;
        acc[o] += (tau < lim) ? wj * u[f0 + o + j][cl] : 0.f;
      }
    }
  } else {
    for (int j = 0; j < p.k; ++j) {
      const float wj = wl[j][cl];
#pragma unroll
      for (int o = 0; o < 16; ++o) acc[o] += wj * u[f0 + o + j][cl];
    }
  }
  T* Y = reinterpret_cast<T*>(p.Y);
  const T* G = reinterpret_cast<const T*>(p.gate);
#pragma unroll
  for (int o = 0; o < 16; ++o) {
    int t = t0 + f0 + o;
    if (t < p.T) {
      float y = acc[o];
      if (G) y *= to_f32(G[((long)b * p.T + t) * p.ldg + ch]);
      Y[((long)b * p.T + t) * p.ldy + ch] = from_f32<T>(y);
    }
  }
}

// backward: persistent blocks over (b, t-tile) pairs of one channel tile; dw accumulates in LDS.
// Tap / bias gradients: every wave keeps its own sums in registers over all its tiles, the four waves are folded in a fixed
// order at the end and the workgroup writes ONE partial row [D][k + 1] (partial != NULL: reduced by dw_partials_reduce_kernel,
// bit-reproducible - round 3; LDS and global fp32 atomics before) or, without a workspace, adds it to dw / dbias atomically.
template <typename T>
__global__ __launch_bounds__(256) void dwconv_bwd_kernel(DwParams p, int tiles_t, float* __restrict__ partial) {
  __shared__ float u[DW_ROWS][DW_CT];
  __shared__ float g[DW_ROWS][DW_CT];     // dYg with halo
  __shared__ float wl[DW_KMAX][DW_CT];
  __shared__ float red[3][DW_CT];
  const int cl = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ch = blockIdx.x * DW_CT + cl;
  const int pad = (p.k - 1) / 2;
  const int rows = DW_TT + 2 * pad;
  for (int j = wv; j < p.k; j += 4) wl[j][cl] = ch < p.D ? p.w[(long)ch * p.k + j] : 0.f;
  float dwr[DW_KMAX], dbr = 0.f;
#pragma unroll
  for (int j = 0; j < DW_KMAX; ++j) dwr[j] = 0.f;
  const T* dY = reinterpret_cast<const T*>(p.Y);
  const T* G = reinterpret_cast<const T*>(p.gate);
  const T* P = reinterpret_cast<const T*>(p.P);
  T* dP = reinterpret_cast<T*>(p.dP);
  T* dG = reinterpret_cast<T*>(p.dgate);
  const float bs = (p.bias && ch < p.D) ? p.bias[ch] : 0.f;
  const int f0 = wv * 16;
  const long total = (long)p.B * tiles_t;
  for (long it = blockIdx.y; it < total; it += gridDim.y) {
    const int b = (int)(it / tiles_t), t0 = (int)(it % tiles_t) * DW_TT;
    __syncthreads();
    fill_u<T>(u, p, b, t0, pad, ch, cl, wv);
    for (int i = wv; i < rows; i += 4) {
      int t = t0 - pad + i;
      float val = 0.f;
      if (t >= 0 && t < p.T && ch < p.D) {
        val = to_f32(dY[((long)b * p.T + t) * p.ldy + ch]);
        if (G) val *= to_f32(G[((long)b * p.T + t) * p.ldg + ch]);
      }
      g[i][cl] = val;
    }
    __syncthreads();
    if (ch < p.D) {
      // (1) dgate = dY * conv(t)   (forward recompute), dbias, dw partials
      float dbp = 0.f;
      if (dG) {
        float acc[16];
#pragma unroll
        for (int o = 0; o < 16; ++o) acc[o] = bs;
        for (int j = 0; j < p.k; ++j) {
          const float wj = wl[j][cl];
#pragma unroll
          for (int o = 0; o < 16; ++o) {
            int t = t0 + f0 + o, tau = t + j - pad;
            bool ok = p.chunk > 0 ? (tau < (t / p.chunk + 1) * p.chunk) : true;
            acc[o] += ok ? wj * u[f0 + o + j][cl] : 0.f;
          }
        }
#pragma unroll
        for (int o = 0; o < 16; ++o) {
          int t = t0 + f0 + o;
          if (t < p.T) dG[((long)b * p.T + t) * p.lddg + ch] = from_f32<T>(to_f32(dY[((long)b * p.T + t) * p.ldy + ch]) * acc[o]);
        }
      }
#pragma unroll
      for (int j = 0; j < DW_KMAX; ++j) {
        if (j < p.k) {                                    // (uniform)
          float s = 0.f;
#pragma unroll
          for (int o = 0; o < 16; ++o) {
            int t = t0 + f0 + o, tau = t + j - pad;
            bool ok = p.chunk > 0 ? (tau < (t / p.chunk + 1) * p.chunk) : true;
            s += ok ? g[pad + f0 + o][cl] * u[f0 + o + j][cl] : 0.f;
          }
          dwr[j] += s;
        }
      }
#pragma unroll
      for (int o = 0; o < 16; ++o) dbp += g[pad + f0 + o][cl];
      dbr += dbp;
      // (2) du(tau) = sum_j w_j dYg(tau - j + pad)  [+ reflect folds], then GLU backward
      float du[16];
#pragma unroll
      for (int o = 0; o < 16; ++o) du[o] = 0.f;
      for (int j = 0; j < p.k; ++j) {
        const float wj = wl[j][cl];
#pragma unroll
        for (int o = 0; o < 16; ++o) {
          int tau = t0 + f0 + o, t = tau - j + pad;       // row of g: (t - (t0 - pad)) = f0 + o - j + 2 pad
          bool ok = p.chunk > 0 ? (t >= 0 && tau < (t / p.chunk + 1) * p.chunk) : true;
          du[o] += ok ? wj * g[f0 + o - j + 2 * pad][cl] : 0.f;
        }
      }
      if (p.pad_mode == SMX_PAD_REFLECT) {
#pragma unroll
        for (int o = 0; o < 16; ++o) {
          int tau = t0 + f0 + o;
          if (tau >= 1 && tau <= pad) {              // virtual frame v = -tau reads frame tau
            int v = -tau;
            float s = 0.f;
            for (int j = 0; j < p.k; ++j) {
              int t = v - j + pad, r = t - (t0 - pad);
              if (t >= 0 && t < p.T && r >= 0 && r < rows) s += wl[j][cl] * g[r][cl];
            }
            du[o] += s;
          }
          if (tau <= p.T - 2 && tau >= p.T - 1 - pad) {   // virtual frame v = 2(T-1)-tau
            int v = 2 * (p.T - 1) - tau;
            float s = 0.f;
            for (int j = 0; j < p.k; ++j) {
              int t = v - j + pad, r = t - (t0 - pad);
              if (t >= 0 && t < p.T && r >= 0 && r < rows) s += wl[j][cl] * g[r][cl];
            }
            du[o] += s;
          }
        }
      }
#pragma unroll
      for (int o = 0; o < 16; ++o) {
        int t = t0 + f0 + o;
        if (t < p.T) {
          const T* row = P + ((long)b * p.T + t) * p.ldp;
          T* drow = dP + ((long)b * p.T + t) * p.lddp;
          if (p.glu) {
            float a = to_f32(row[ch]), s = sigmoidf_(to_f32(row[p.D + ch]));
            drow[ch] = from_f32<T>(du[o] * s);
            drow[p.D + ch] = from_f32<T>(du[o] * a * s * (1.f - s));
          } else {
            drow[ch] = from_f32<T>(du[o]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j <= DW_KMAX; ++j) {
    if (j < p.k || j == DW_KMAX) {                        // (uniform; j == DW_KMAX: the bias gradient)
      const float v = j < DW_KMAX ? dwr[j < DW_KMAX ? j : 0] : dbr;
      __syncthreads();
      if (wv > 0) red[wv - 1][cl] = v;
      __syncthreads();
      if (wv == 0 && ch < p.D) {
        const float tot = ((v + red[0][cl]) + red[1][cl]) + red[2][cl];
        const int jj = j < DW_KMAX ? j : p.k;
        if (partial) partial[((long)blockIdx.y * p.D + ch) * (p.k + 1) + jj] = tot;
        else if (j < DW_KMAX) atomicAdd(p.dw + (long)ch * p.k + j, tot);
        else if (p.dbias) atomicAdd(p.dbias + ch, tot);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Register-window specialisations for the production shape (compile-time K taps, zero padding, no chunking,
// no gate, D % 8 == 0): 16-byte global accesses everywhere (a tile row of 64 channels is one 128 B line for bf16),
// each thread pulls its 16+K-1 input frames from LDS ONCE and does all K x 16 FMAs out of registers.
// ---------------------------------------------------------------------------------------------------
template <typename T> struct DwVec { static constexpr int N = 16 / sizeof(T); };

template <typename T>
__device__ __forceinline__ void ld_chunk(const T* p, float (&f)[DwVec<T>::N]) {
  if constexpr (sizeof(T) == 2) {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = bf16_bits_to_f32(w[i] & 0xffffu); f[2 * i + 1] = bf16_bits_to_f32(w[i] >> 16); }
  } else {
    const float4 r = *reinterpret_cast<const float4*>(p);
    f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w;
  }
}
template <typename T>
__device__ __forceinline__ void st_chunk(T* p, const float (&f)[DwVec<T>::N]) {
  if constexpr (sizeof(T) == 2) {
    uint4 r;
    r.x = pack_bf16x2(f[0], f[1]); r.y = pack_bf16x2(f[2], f[3]);
    r.z = pack_bf16x2(f[4], f[5]); r.w = pack_bf16x2(f[6], f[7]);
    *reinterpret_cast<uint4*>(p) = r;
  } else {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
}

// u tile rows [t0-PAD, t0+TT+PAD) x 64 channels, GLU applied, zero padded in time; 16 B per thread per access
template <typename T, int ROWS, int PAD>
__device__ __forceinline__ void fill_u_vec(float (*u)[DW_CT], const DwParams& p, int b, int t0, int c0, int tid) {
  constexpr int VW = DwVec<T>::N, LPR = DW_CT / VW, NITEM = (ROWS * LPR + 255) / 256;
  const T* P = reinterpret_cast<const T*>(p.P);
#pragma unroll
  for (int k = 0; k < NITEM; ++k) {
    const int it = tid + 256 * k;
    if (it < ROWS * LPR) {
      const int i = it / LPR, cc = (it % LPR) * VW;
      const int tau = map_frame(t0 - PAD + i, p.T, p.pad_mode), ch = c0 + cc;   // zero pad -> -1, reflect -> mirrored
      float v[VW];
#pragma unroll
      for (int q = 0; q < VW; ++q) v[q] = 0.f;
      if (tau >= 0 && ch < p.D) {
        const T* row = P + ((long)b * p.T + tau) * p.ldp;
        ld_chunk<T>(row + ch, v);
        if (p.glu) {
          float gte[VW];
          ld_chunk<T>(row + p.D + ch, gte);
#pragma unroll
          for (int q = 0; q < VW; ++q) v[q] *= sigmoidf_(gte[q]);
        }
      }
#pragma unroll
      for (int q4 = 0; q4 < VW / 4; ++q4)
        *reinterpret_cast<float4*>(&u[i][cc + 4 * q4]) = make_float4(v[4 * q4], v[4 * q4 + 1], v[4 * q4 + 2], v[4 * q4 + 3]);
    }
  }
}

template <typename T, int K, bool GATE>
__global__ __launch_bounds__(256) void dwconv_fwd_fast(DwParams p) {
  constexpr int PAD = (K - 1) / 2, WIN = 16 + K - 1, ROWS = DW_TT + K - 1;
  constexpr int VW = DwVec<T>::N, LPR = DW_CT / VW;
  __shared__ __attribute__((aligned(16))) float u[ROWS][DW_CT];
  const int cl = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c0 = blockIdx.x * DW_CT, ch = c0 + cl, t0 = blockIdx.y * DW_TT, b = blockIdx.z;
  fill_u_vec<T, ROWS, PAD>(u, p, b, t0, c0, threadIdx.x);
  float w[K];
#pragma unroll
  for (int j = 0; j < K; ++j) w[j] = ch < p.D ? p.w[(long)ch * K + j] : 0.f;
  const float bs = (p.bias && ch < p.D) ? p.bias[ch] : 0.f;
  __syncthreads();
  const int f0 = wv * 16;
  float win[WIN];
#pragma unroll
  for (int i = 0; i < WIN; ++i) win[i] = u[f0 + i][cl];
  __syncthreads();                                   // every window is in registers: the tile can be reused
#pragma unroll
  for (int o = 0; o < 16; ++o) {
    float acc = bs;
#pragma unroll
    for (int j = 0; j < K; ++j) acc += w[j] * win[o + j];
    u[f0 + o][cl] = acc;
  }
  __syncthreads();
  T* Y = reinterpret_cast<T*>(p.Y);
  for (int it = threadIdx.x; it < DW_TT * LPR; it += 256) {
    const int r = it / LPR, cc = (it % LPR) * VW;
    const int t = t0 + r, chv = c0 + cc;
    if (t < p.T && chv < p.D) {
      float v[VW];
#pragma unroll
      for (int q = 0; q < VW; ++q) v[q] = u[r][cc + q];
      if constexpr (GATE) {                            // CSGU: y = conv(x2) * x1
        float gt[VW];
        ld_chunk<T>(reinterpret_cast<const T*>(p.gate) + ((long)b * p.T + t) * p.ldg + chv, gt);
#pragma unroll
        for (int q = 0; q < VW; ++q) v[q] *= gt[q];
      }
      st_chunk<T>(Y + ((long)b * p.T + t) * p.ldy + chv, v);
    }
  }
}

template <typename T, int K, bool REFLECT, bool GATE>
__global__ __launch_bounds__(256) void dwconv_bwd_fast(DwParams p, int tiles_t, float* __restrict__ partial, int gy) {
  constexpr int PAD = (K - 1) / 2, WIN = 16 + K - 1, ROWS = DW_TT + K - 1;
  constexpr int VW = DwVec<T>::N, LPR = DW_CT / VW, NITEM = (ROWS * LPR + 255) / 256;
  __shared__ __attribute__((aligned(16))) float u[ROWS][DW_CT];
  __shared__ __attribute__((aligned(16))) float g[ROWS][DW_CT];
  // CSGU: the tile's own dY rows, kept for dgate = dY * conv (re-reading them from memory after the conv recompute was
  // one more exposed round trip per tile)
  __shared__ __attribute__((aligned(16))) float dyc[GATE ? DW_TT : 1][DW_CT];
  __shared__ float red[3][DW_CT];
  __shared__ float wl[REFLECT ? K : 1][DW_CT];         // the taps once more, indexable at run time by the edge fold
  const int cl = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // workgroup b runs on XCD b % 8: keep the channel tiles of one frame-tile sequence on ONE XCD and adjacent in
  // dispatch order, so the 128-byte pieces of a feature row are fetched by neighbours at the same time
  const int ctiles = (p.D + DW_CT - 1) / DW_CT;
  const int xcd = blockIdx.x & 7, widx = blockIdx.x >> 3;
  const int by = (widx / ctiles) * 8 + xcd, bx = widx % ctiles;
  if (by >= gy) return;
  const int c0 = bx * DW_CT, ch = c0 + cl;
  const bool cok = ch < p.D;
  float w[K], dw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { w[j] = cok ? p.w[(long)ch * K + j] : 0.f; dw[j] = 0.f; }
  if constexpr (REFLECT) {
    for (int j = wv; j < K; j += 4) wl[j][cl] = cok ? p.w[(long)ch * K + j] : 0.f;   // (first use is behind barriers)
  }
  float dbs = 0.f;
  const T* dY = reinterpret_cast<const T*>(p.Y);
  const T* P = reinterpret_cast<const T*>(p.P);
  T* dP = reinterpret_cast<T*>(p.dP);
  const int f0 = wv * 16;
  const long total = (long)p.B * tiles_t;
  for (long it0 = by; it0 < total; it0 += gy) {
    const int b = (int)(it0 / tiles_t), t0 = (int)(it0 % tiles_t) * DW_TT;
    __syncthreads();
    fill_u_vec<T, ROWS, PAD>(u, p, b, t0, c0, threadIdx.x);
#pragma unroll
    for (int k = 0; k < NITEM; ++k) {                // dY tile with halo, 16 B per thread
      const int it = threadIdx.x + 256 * k;
      if (it < ROWS * LPR) {
        const int i = it / LPR, cc = (it % LPR) * VW;
        const int t = t0 - PAD + i, chv = c0 + cc;
        float v[VW];
#pragma unroll
        for (int q = 0; q < VW; ++q) v[q] = 0.f;
        if (t >= 0 && t < p.T && chv < p.D) {
          ld_chunk<T>(dY + ((long)b * p.T + t) * p.ldy + chv, v);
          if constexpr (GATE) {                        // gradient w.r.t. the conv output: dY * gate
            float gt[VW];
            ld_chunk<T>(reinterpret_cast<const T*>(p.gate) + ((long)b * p.T + t) * p.ldg + chv, gt);
            if (i >= PAD && i < PAD + DW_TT) {
#pragma unroll
              for (int q4 = 0; q4 < VW / 4; ++q4)
                *reinterpret_cast<float4*>(&dyc[i - PAD][cc + 4 * q4]) = make_float4(v[4 * q4], v[4 * q4 + 1], v[4 * q4 + 2], v[4 * q4 + 3]);
            }
#pragma unroll
            for (int q = 0; q < VW; ++q) v[q] *= gt[q];
          }
        }
#pragma unroll
        for (int q4 = 0; q4 < VW / 4; ++q4)
          *reinterpret_cast<float4*>(&g[i][cc + 4 * q4]) = make_float4(v[4 * q4], v[4 * q4 + 1], v[4 * q4 + 2], v[4 * q4 + 3]);
      }
    }
    __syncthreads();
    float uw[WIN], gw[WIN];
#pragma unroll
    for (int i = 0; i < WIN; ++i) { uw[i] = u[f0 + i][cl]; gw[i] = g[f0 + i][cl]; }
    __syncthreads();                                 // windows are in registers: u can take the du tile
    if constexpr (GATE) {                            // dgate = dY * conv(x2)  (forward recompute out of the window)
      const float bsv = (p.bias && cok) ? p.bias[ch] : 0.f;
#pragma unroll
      for (int o = 0; o < 16; ++o) {
        float acc = bsv;
#pragma unroll
        for (int j = 0; j < K; ++j) acc += w[j] * uw[o + j];
        u[f0 + o][cl] = acc;
      }
      __syncthreads();
      T* dG = reinterpret_cast<T*>(p.dgate);
      for (int it = threadIdx.x; it < DW_TT * LPR; it += 256) {
        const int r = it / LPR, cc = (it % LPR) * VW;
        const int t = t0 + r, chv = c0 + cc;
        if (t < p.T && chv < p.D) {
          float o8[VW];
#pragma unroll
          for (int q = 0; q < VW; ++q) o8[q] = dyc[r][cc + q] * u[r][cc + q];
          st_chunk<T>(dG + ((long)b * p.T + t) * p.lddg + chv, o8);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
      float sacc = 0.f;
#pragma unroll
      for (int o = 0; o < 16; ++o) sacc += gw[PAD + o] * uw[o + j];
      dw[j] += sacc;
    }
#pragma unroll
    for (int o = 0; o < 16; ++o) dbs += gw[PAD + o];
#pragma unroll
    for (int o = 0; o < 16; ++o) {
      float du = 0.f;
#pragma unroll
      for (int j = 0; j < K; ++j) du += w[j] * gw[o - j + 2 * PAD];
      u[f0 + o][cl] = du;
    }
    if constexpr (REFLECT) {
      // fold the gradient of the mirrored virtual frames into the edge frames.  Kept OUT of the unrolled FMA block above
      // (a rolled loop over this thread's own 16 rows of the du tile, entered only by tiles that touch an utterance edge)
      // and with the taps read from an LDS copy: branches inside the unrolled block and a run-time index into the
      // register array w[] made every tile of the reflect variant 3.3x slower; taps re-read from global memory cost a
      // dependent L2 round trip per tap (T = 250: half the tiles touch an edge, 451 us vs 322 us for zero padding).
      if (t0 <= PAD || t0 + DW_TT + PAD >= p.T - 1) {
        __syncthreads();                               // every du row of the tile is in LDS
        // the PAD rows next to either edge are shared among the 4 waves.  The wave index is made explicitly uniform: row,
        // tap range and LDS row addresses are then scalar arithmetic, the tap loops are plain counted loops (no per-lane
        // predication) and unroll by 4 so that their LDS reads overlap
        const int wvs = __builtin_amdgcn_readfirstlane(wv);
        for (int idx = wvs; idx < 2 * PAD; idx += 4) {
          const bool top = idx < PAD;
          const int tau = top ? 1 + idx : p.T - 1 - PAD + (idx - PAD);
          const int o = tau - t0;
          // frames 1..PAD are mirrored at the top, frames T-1-PAD..T-2 at the bottom; for T < 32 a frame can sit in both
          // ranges: its top pass then does both folds and the bottom pass skips it
          const bool in_top = tau >= 1 && tau <= PAD && tau <= p.T - 1;
          const bool in_bot = tau >= 0 && tau <= p.T - 2 && tau >= p.T - 1 - PAD;
          if (o < 0 || o >= DW_TT || (top ? !in_top : (!in_bot || in_top))) continue;
          float add = 0.f;
          if (in_top) {                                // virtual frame -tau mirrors frame tau: taps j <= PAD - tau
            const int r0 = 2 * PAD - tau - t0;         // g row of tap 0; tap j reads row r0 - j (frame PAD - tau - j)
            const int jlo = max(max(0, r0 - (ROWS - 1)), PAD - tau - p.T + 1), jhi = min(PAD - tau, r0);
#pragma unroll 4
            for (int j = jlo; j <= jhi; ++j) add += wl[j][cl] * g[r0 - j][cl];
          }
          if (in_bot) {                                // virtual frame 2(T-1)-tau mirrors frame tau: taps j >= T-1-tau+PAD
            const int r0 = 2 * (p.T - 1) - tau + 2 * PAD - t0;   // tap j reads row r0 - j (frame 2(T-1) - tau - j + PAD)
            const int jlo = max(max(0, p.T - 1 - tau + PAD), r0 - (ROWS - 1));
            const int jhi = min(min(K - 1, r0), 2 * (p.T - 1) - tau + PAD);
#pragma unroll 4
            for (int j = jlo; j <= jhi; ++j) add += wl[j][cl] * g[r0 - j][cl];
          }
          u[o][cl] += add;
        }
      }
    }
    __syncthreads();
    for (int it = threadIdx.x; it < DW_TT * LPR; it += 256) {   // GLU backward, 16 B loads / stores
      const int r = it / LPR, cc = (it % LPR) * VW;
      const int t = t0 + r, chv = c0 + cc;
      if (t < p.T && chv < p.D) {
        float du[VW];
#pragma unroll
        for (int q = 0; q < VW; ++q) du[q] = u[r][cc + q];
        T* drow = dP + ((long)b * p.T + t) * p.lddp;
        if (p.glu) {
          const T* row = P + ((long)b * p.T + t) * p.ldp;
          float a[VW], gt[VW], d1[VW], d2[VW];
          ld_chunk<T>(row + chv, a);
          ld_chunk<T>(row + p.D + chv, gt);
#pragma unroll
          for (int q = 0; q < VW; ++q) {
            const float sg = sigmoidf_(gt[q]);
            d1[q] = du[q] * sg;
            d2[q] = du[q] * a[q] * sg * (1.f - sg);
          }
          st_chunk<T>(drow + chv, d1);
          st_chunk<T>(drow + p.D + chv, d2);
        } else {
          st_chunk<T>(drow + chv, du);
        }
      }
    }
  }
  // flush dw / dbias: 4 waves -> LDS -> one partial row per block (reduced in a fixed order by
  // dw_partials_reduce_kernel; same-address fp32 atomics from ~1000 blocks cost ~100 ns each)
#pragma unroll
  for (int j = 0; j <= K; ++j) {
    const float v = j < K ? dw[j < K ? j : 0] : dbs;
    __syncthreads();
    if (wv > 0) red[wv - 1][cl] = v;
    __syncthreads();
    if (wv == 0 && cok) {
      const float tot = ((v + red[0][cl]) + red[1][cl]) + red[2][cl];
      partial[((long)by * p.D + ch) * (K + 1) + j] = tot;
    }
  }
}

// dw[ch][j] += sum_y partial[y][ch][j] (j < K); dbias[ch] += sum_y partial[y][ch][K]
__global__ __launch_bounds__(256) void dw_partials_reduce_kernel(const float* __restrict__ partial, int ny, int D, int K,
                                                                 float* dw, float* dbias) {
  const long W = (long)D * (K + 1);
  const long idx = blockIdx.x * 256L + threadIdx.x;
  if (idx >= W) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int y = 0;
  for (; y + 3 < ny; y += 4) {
    s0 += partial[(long)y * W + idx]; s1 += partial[(long)(y + 1) * W + idx];
    s2 += partial[(long)(y + 2) * W + idx]; s3 += partial[(long)(y + 3) * W + idx];
  }
  for (; y < ny; ++y) s0 += partial[(long)y * W + idx];
  const int ch = (int)(idx / (K + 1)), j = (int)(idx % (K + 1));
  const float tot = (s0 + s1) + (s2 + s3);
  if (j < K) dw[(long)ch * K + j] += tot;
  else if (dbias) dbias[ch] += tot;
}

}  // namespace smx

#include "dwconv_roll.h"

using namespace smx;

// ---- host side.  dw_plan is the only place that looks at k, D, alignment, padding, gate, chunk, dtype and workspace: it
// names the route and the launch geometry or refuses; smx_dwconv_fwd / smx_dwconv_bwd launch what it names and
// smx_dwconv_plan_query hands it out (DESIGN.md "Depthwise conv routes").
static int tiles_of(int n, int tile) { return (n + tile - 1) / tile; }

// partial rows of the tiled and window backward: ~1024 persistent blocks in total, at most one per (batch, time tile)
static long tiled_rows(int B, int T, int D) {
  const long total = (long)B * tiles_of(T, DW_TT), gy = tiles_of(1024, tiles_of(D, DW_CT));
  return gy < total ? gy : total;
}

// every operand of the call has a row stride that is a multiple of v elements and a 16-byte aligned base
static bool dw_aligned(const smx_dwconv_args& a, bool bwd, int v) {
  auto ok = [v](const void* p, int64_t ld) { return ld % v == 0 && aligned16(p); };
  return ok(a.P, a.ldp) && ok(a.Y, a.ldy) && (!a.gate || ok(a.gate, a.ldg)) &&
         (!bwd || (ok(a.dP, a.lddp) && (!a.gate || ok(a.dgate, a.lddg))));
}

static int dw_plan(const smx_dwconv_args& a, bool bwd, smx_dwconv_plan* pl) {
  const char* who = bwd ? "smx_dwconv_bwd" : "smx_dwconv_fwd";
  memset(pl, 0, sizeof(*pl));
  SMX_REQUIRE(a.P && a.w && a.Y && (!bwd || (a.dP && (a.dw || a.workspace))), "%s: null pointer", who);
  SMX_REQUIRE(a.k >= 1 && a.k <= DW_KMAX && (a.k & 1), "%s: k=%d must be odd and <= %d", who, a.k, DW_KMAX);
  if (bwd) SMX_REQUIRE((a.gate == nullptr) == (a.dgate == nullptr), "%s: gate and dgate go together", who);
  else {
    SMX_REQUIRE(a.drop_p >= 0.f && a.drop_p < 1.f, "%s: 0 <= drop_p < 1", who);
    SMX_REQUIRE(a.pad_mode != SMX_PAD_REFLECT || (a.k - 1) / 2 < a.T, "%s: reflect pad needs (k-1)/2 < T", who);
  }
  if (a.B <= 0 || a.T <= 0 || a.D <= 0) return SMX_OK;              // (grid[0] == 0: nothing to launch)
  const bool bf = a.dtype == SMX_BF16, zero = a.pad_mode == SMX_PAD_ZERO, ws = !bwd || a.workspace;
  const int vw = bf ? 8 : 4;
  pl->chunked = a.chunk > 0;
  pl->route = SMX_DW_TILED;
  // the rolling kernels (dwconv_roll.h); the bf16 ones move 16-byte pieces (LDS-DMA in, dwordx4 out)
  if (a.k == 31 && a.D % 64 == 0 && ws && (!bf || dw_aligned(a, bwd, 8))) {
    // (Dynamic Chunk Convolution, chunk > 0, is part of the GLU kernels)
    if (a.glu && !a.gate && zero) pl->route = SMX_DW_ROLL;
    else if (!pl->chunked && !a.glu && a.gate && !zero && bf && a.T > 15) pl->route = SMX_DW_ROLL_CSGU;
  }
  if (pl->route == SMX_DW_TILED && a.k == 31 && !pl->chunked && a.D % vw == 0 && ws && dw_aligned(a, bwd, vw) && (zero || a.T > 15))
    pl->route = SMX_DW_WINDOW;
  const int ctiles = tiles_of(a.D, DW_CT);
  if (pl->route >= SMX_DW_ROLL) {
    auto mx = [](int64_t x, int64_t y) { return x > y ? x : y; };
    const int64_t ldmax = mx(mx(mx(a.ldp, a.ldy), a.ldg), bwd ? mx(a.lddp, a.lddg) : 0);
    SMX_REQUIRE((long)a.T * ldmax * 4 < (1L << 31), "%s: utterance span >= 2 GB", who);
    roll_geometry(a.B, a.T, a.D, &pl->seg, &pl->nseg, &pl->partial_rows);
    pl->grid[0] = 8 * (a.D / 64) * tiles_of(pl->partial_rows, 8);
  } else {
    pl->partial_rows = (int)tiled_rows(a.B, a.T, a.D);
    if (!bwd) pl->grid[0] = ctiles, pl->grid[1] = tiles_of(a.T, DW_TT), pl->grid[2] = a.B;
    else if (pl->route == SMX_DW_WINDOW) pl->grid[0] = 8 * ctiles * tiles_of(pl->partial_rows, 8);
    else pl->grid[0] = ctiles, pl->grid[1] = pl->partial_rows;
  }
  for (int& g : pl->grid) g = g ? g : 1;
  if (!bwd && a.drop_p > 0.f && pl->route != SMX_DW_ROLL_CSGU)
    return fail(SMX_EUNSUPPORTED, "%s: fused output dropout needs the rolling CSGU kernel", who);
  // the tiled kernel keeps no partial rows for a later reduction (without a workspace its tap gradients are atomics)
  pl->deferrable = bwd && pl->route != SMX_DW_TILED;
  if (bwd && !a.dw && !pl->deferrable)
    return fail(SMX_EUNSUPPORTED, "%s: dw == NULL (deferred reduction) needs the window or a rolling route", who);
  return SMX_OK;
}

static DwParams dw_params(const smx_dwconv_args& a, bool bwd, int route) {
  DwParams p;
  memset(&p, 0, sizeof(p));
  p.P = a.P; p.ldp = a.ldp; p.w = a.w; p.bias = a.bias; p.gate = a.gate; p.ldg = a.ldg; p.Y = a.Y; p.ldy = a.ldy;
  p.B = a.B; p.T = a.T; p.D = a.D; p.k = a.k; p.glu = a.glu; p.pad_mode = a.pad_mode; p.chunk = a.chunk;
  if (bwd) {
    p.dP = a.dP; p.lddp = a.lddp; p.dgate = a.dgate; p.lddg = a.lddg; p.dw = a.dw; p.dbias = a.dbias;
  } else if (route == SMX_DW_ROLL_CSGU) {
    p.dthresh = (unsigned)((double)a.drop_p * 4294967296.0); p.dscale = 1.f / (1.f - a.drop_p); p.dseed = a.drop_seed; p.epoch = a.epoch;
  }
  return p;
}

// f(tag) with tag.value = b as a constant: the bool template arguments of the launch sites
template <typename F>
static inline void dw_flag(bool b, F&& f) {
  if (b) f(std::true_type()); else f(std::false_type());
}

extern "C" int smx_dwconv_plan_query(const smx_dwconv_args* a, int backward, smx_dwconv_plan* plan) {
  SMX_REQUIRE(a && plan, "smx_dwconv_plan_query: null pointer");
  return dw_plan(*a, backward != 0, plan);
}

extern "C" size_t smx_dwconv1d_glu_bwd_workspace(int B, int T, int D, int k) {
  if (B <= 0 || T <= 0 || D <= 0) return 0;
  long gy = tiled_rows(B, T, D);
  if (D % 64 == 0 && k == 31) {
    int seg, nseg, gr;
    roll_geometry(B, T, D, &seg, &nseg, &gr);
    if (gr > gy) gy = gr;
  }
  return (size_t)gy * D * (k + 1) * sizeof(float);
}

extern "C" int smx_dwconv_fwd(const smx_dwconv_args* a, void* stream) {
  SMX_REQUIRE(a, "smx_dwconv_fwd: null descriptor");
  smx_dwconv_plan pl;
  if (int rc = dw_plan(*a, false, &pl)) return rc;
  if (!pl.grid[0]) return SMX_OK;
  const DwParams p = dw_params(*a, false, pl.route);
  const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]), blk(256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool bf = a->dtype == SMX_BF16;
  if (pl.route == SMX_DW_ROLL_CSGU) hipLaunchKernelGGL(dwconv_rollc_fwd, grid, blk, 0, s, p, pl.seg, pl.nseg, pl.partial_rows);
  else if (pl.route == SMX_DW_ROLL) dw_flag(pl.chunked, [&](auto ch) {
    constexpr bool CH = decltype(ch)::value;
    if (bf) hipLaunchKernelGGL((dwconv_rolls_fwd<CH>), grid, blk, 0, s, p, pl.seg, pl.nseg, pl.partial_rows);
    else hipLaunchKernelGGL((dwconv_roll_fwd<float, CH>), grid, blk, 0, s, p, pl.seg, pl.nseg, pl.partial_rows);
  });
  else dispatch_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    if (pl.route == SMX_DW_WINDOW) dw_flag(a->gate != nullptr, [&](auto g) {
      hipLaunchKernelGGL((dwconv_fwd_fast<T, 31, decltype(g)::value>), grid, blk, 0, s, p);
    });
    else hipLaunchKernelGGL((dwconv_fwd_kernel<T>), grid, blk, 0, s, p);
  });
  return check_launch("smx_dwconv_fwd");
}

extern "C" int smx_dwconv_bwd(const smx_dwconv_args* a, void* stream) {
  SMX_REQUIRE(a, "smx_dwconv_bwd: null descriptor");
  smx_dwconv_plan pl;
  if (int rc = dw_plan(*a, true, &pl)) return rc;
  if (!pl.grid[0]) return SMX_OK;
  const DwParams p = dw_params(*a, true, pl.route);
  const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]), blk(256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* partial = reinterpret_cast<float*>(a->workspace);
  const int rows = pl.partial_rows, tiles_t = tiles_of(a->T, DW_TT);
  const bool bf = a->dtype == SMX_BF16;
  if (pl.route == SMX_DW_ROLL_CSGU) {
    hipLaunchKernelGGL(dwconv_rollc_bwd, grid, blk, 0, s, p, pl.seg, pl.nseg, rows, partial);
    // the gradient of the mirrored virtual frames goes back to frames 1..15 / T-16..T-2 (30 rows per utterance)
    hipLaunchKernelGGL(dwconv_csgu_fold_kernel, dim3((unsigned)((a->D / 2 + 63) / 64), (unsigned)a->B), dim3(64), 0, s, p);
  }
#ifdef SMX_DIAG
  else if (pl.route == SMX_DW_ROLL && bf && !pl.chunked && cfg().dwroll_ablate == 1)
    hipLaunchKernelGGL((dwconv_rolls_bwd<1>), grid, blk, 0, s, p, pl.seg, pl.nseg, rows, partial);
  else if (pl.route == SMX_DW_ROLL && bf && !pl.chunked && cfg().dwroll_ablate == 2)
    hipLaunchKernelGGL((dwconv_rolls_bwd<2>), grid, blk, 0, s, p, pl.seg, pl.nseg, rows, partial);
#endif
  else if (pl.route == SMX_DW_ROLL) dw_flag(pl.chunked, [&](auto ch) {
    constexpr bool CH = decltype(ch)::value;
    if (bf) hipLaunchKernelGGL((dwconv_rolls_bwd<0, CH>), grid, blk, 0, s, p, pl.seg, pl.nseg, rows, partial);
    else hipLaunchKernelGGL((dwconv_roll_bwd<float, CH>), grid, blk, 0, s, p, pl.seg, pl.nseg, rows, partial);
  });
  else dispatch_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    if (pl.route == SMX_DW_WINDOW) dw_flag(a->pad_mode == SMX_PAD_REFLECT, [&](auto r) {
      dw_flag(a->gate != nullptr, [&](auto g) {
        hipLaunchKernelGGL((dwconv_bwd_fast<T, 31, decltype(r)::value, decltype(g)::value>), grid, blk, 0, s, p, tiles_t, partial, rows);
      });
    });
    // generic shapes (k != 31, D % 8 != 0, ...): with a workspace one partial row per workgroup, else atomics
    else hipLaunchKernelGGL((dwconv_bwd_kernel<T>), grid, blk, 0, s, p, tiles_t, partial);
  });
  // fixed-order reduction of the partial rows [rows][D][k + 1]; dw == NULL: they stay in the workspace for smx_reduce_jobs
  const long W = (long)a->D * (a->k + 1);
  if (a->dw && partial)
    hipLaunchKernelGGL(dw_partials_reduce_kernel, dim3((unsigned)((W + 255) / 256)), blk, 0, s, partial, rows, a->D, a->k, a->dw, a->dbias);
  return check_launch("smx_dwconv_bwd");
}
