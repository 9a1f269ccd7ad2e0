// layernorm.hip — the standalone LayerNorm of the SummaryMixing path (gfx950, wave64): forward (optionally a second LayerNorm
// of the output in the same pass) and backward (optionally a second output, the gradient from split-K slabs, or through the
// activation that produced the input), with one host dispatcher per direction (include/smx.h: smx_ln_fwd / smx_ln_bwd).
#include <type_traits>

#include "smx_common.h"

namespace smx {

// =================================================================================================
// LayerNorm.  One wave per row, 4 rows per block; lane owns 4-element vectors at columns lane*4 + 256*i.
// =================================================================================================
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const T* X, long ldx, const float* gamma, const float* beta,
                                                            T* Y, long ldy, float* stats, int N_, int D, float eps,
                                                            int act) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N_) return;
  const T* x = X + (long)row * ldx;
  T* y = Y + (long)row * ldy;
  float s = 0.f;
  if (VEC) {
    for (int c = lane * 4; c < D; c += 256) { float f[4]; load4<T>(x + c, f); s += (f[0] + f[1]) + (f[2] + f[3]); }
  } else {
    for (int c = lane; c < D; c += 64) s += to_f32(x[c]);
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
  if (VEC) {
    for (int c = lane * 4; c < D; c += 256) {
      float f[4]; load4<T>(x + c, f);
#pragma unroll
      for (int i = 0; i < 4; ++i) { float d = f[i] - mean; q += d * d; }
    }
  } else {
    for (int c = lane; c < D; c += 64) { float d = to_f32(x[c]) - mean; q += d * d; }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
  if (stats && lane == 0) { stats[2 * (long)row] = mean; stats[2 * (long)row + 1] = rstd; }
  if (VEC) {
    for (int c = lane * 4; c < D; c += 256) {
      float f[4]; load4<T>(x + c, f);
      float4 g4 = *reinterpret_cast<const float4*>(gamma + c), b4 = *reinterpret_cast<const float4*>(beta + c);
      float o[4] = {(f[0] - mean) * rstd * g4.x + b4.x, (f[1] - mean) * rstd * g4.y + b4.y,
                    (f[2] - mean) * rstd * g4.z + b4.z, (f[3] - mean) * rstd * g4.w + b4.w};
      if (act == SMX_ACT_SWISH) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = act_fwd_c<SMX_ACT_SWISH>(o[i]);
      } else if (act == SMX_ACT_GELU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = act_fwd_c<SMX_ACT_GELU>(o[i]);
      } else if (act != SMX_ACT_NONE) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = act_fwd(act, o[i]);
      }
      store4<T>(y + c, o);
    }
  } else {
    for (int c = lane; c < D; c += 64) y[c] = from_f32<T>(act_fwd(act, (to_f32(x[c]) - mean) * rstd * gamma[c] + beta[c]));
  }
}

// Single-read forward for D <= 256 * CH (D % 4 == 0, aligned rows): the row lives in registers (one 4-element vector
// per lane and chunk), U rows are in flight per wave (all their loads issued before the first reduction), workgroups
// stride over the rows.  The generic kernel above re-reads the row three times behind three dependent latencies.
// TX: element type of the input (float for the fp32 residual stream: LayerNorm(fp32 x) -> dtype T, smx_ln_fwd.x_f32)
template <typename T, int CH, int U, typename TX = T>
__global__ __launch_bounds__(256) void layernorm_fwd_fast(const TX* __restrict__ X, long ldx, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, T* __restrict__ Y, long ldy,
                                                          float* __restrict__ stats, int N_, int D, float eps, int act) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float gam[CH][4], bet[CH][4];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < D) {
      const float4 g4 = *reinterpret_cast<const float4*>(gamma + c), b4 = *reinterpret_cast<const float4*>(beta + c);
      gam[i][0] = g4.x; gam[i][1] = g4.y; gam[i][2] = g4.z; gam[i][3] = g4.w;
      bet[i][0] = b4.x; bet[i][1] = b4.y; bet[i][2] = b4.z; bet[i][3] = b4.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) gam[i][j] = bet[i][j] = 0.f;
    }
  }
  const float invD = 1.f / (float)D;
  dispatch_act(act, [&](auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;
    for (int row0 = (blockIdx.x * 4 + w) * U; row0 < N_; row0 += gridDim.x * 4 * U) {
      float f[U][CH][4], s[U], q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = min(row0 + u, N_ - 1);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int c = (lane + 64 * i) * 4;
          if (c < D) load4<TX>(X + (long)row * ldx + c, f[u][i]);
          else f[u][i][0] = f[u][i][1] = f[u][i][2] = f[u][i][3] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[u] = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) s[u] += (f[u][i][0] + f[u][i][1]) + (f[u][i][2] + f[u][i][3]);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], off, 64);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[u] *= invD;                                      // mean
        q[u] = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          if ((lane + 64 * i) * 4 < D) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = f[u][i][j] - s[u]; q[u] += d * d; }
          }
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int u = 0; u < U; ++u) q[u] += __shfl_xor(q[u], off, 64);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = row0 + u;
        if (row >= N_) break;
        const float rstd = rsqrtf(q[u] * invD + eps);
        if (stats && lane == 0) *reinterpret_cast<float2*>(stats + 2 * (long)row) = make_float2(s[u], rstd);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int c = (lane + 64 * i) * 4;
          if (c < D) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = act_fwd_c<ACT>((f[u][i][j] - s[u]) * rstd * gam[i][j] + bet[i][j]);
            store4<T>(Y + (long)row * ldy + c, o);
          }
        }
      }
    }
  });
}

// Two LayerNorms in one pass over the float32 residual stream (round 4): y1 = LN1(x) (float32: the layer-final norm2 of
// a Conformer layer, Conformer.py:536 = the next layer's stream input) and y2 = LN2(y1) (dtype T2: the LayerNorm in front of
// the next layer's first feed-forward module, Conformer.py:458-459,507).  y1 never comes back from memory for the second
// statistics.  Same lane / chunk layout and the same reduction trees as layernorm_fwd_fast, so both outputs equal those of
// two separate launches to an ulp.
template <typename T2, int CH, int U>
__global__ __launch_bounds__(256) void layernorm_fwd_pair_fast(const float* __restrict__ X, long ldx, const float* __restrict__ gamma1,
                                                               const float* __restrict__ beta1, float eps1, float* __restrict__ Y1,
                                                               long ldy1, float* __restrict__ stats1,
                                                               const float* __restrict__ gamma2, const float* __restrict__ beta2,
                                                               float eps2, T2* __restrict__ Y2, long ldy2, float* __restrict__ stats2,
                                                               int N_, int D) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float g1[CH][4], b1[CH][4], g2[CH][4], b2[CH][4];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (lane + 64 * i) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) g1[i][j] = b1[i][j] = g2[i][j] = b2[i][j] = 0.f;
    if (c < D) {
      load4<float>(gamma1 + c, g1[i]); load4<float>(beta1 + c, b1[i]);
      load4<float>(gamma2 + c, g2[i]); load4<float>(beta2 + c, b2[i]);
    }
  }
  const float invD = 1.f / (float)D;
  auto row_sum = [&](float (&v)[U]) __attribute__((always_inline)) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] += __shfl_xor(v[u], off, 64);
  };
  for (int row0 = (blockIdx.x * 4 + w) * U; row0 < N_; row0 += gridDim.x * 4 * U) {
    float f[U][CH][4], s[U], q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = min(row0 + u, N_ - 1);
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < D) load4<float>(X + (long)row * ldx + c, f[u][i]);
        else f[u][i][0] = f[u][i][1] = f[u][i][2] = f[u][i][3] = 0.f;
      }
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {               // pass 0: LN1 (f <- y1, stored), pass 1: LN2 of the registers
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[u] = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) s[u] += (f[u][i][0] + f[u][i][1]) + (f[u][i][2] + f[u][i][3]);
      }
      row_sum(s);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[u] *= invD;
        q[u] = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          if ((lane + 64 * i) * 4 < D) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = f[u][i][j] - s[u]; q[u] += d * d; }
          }
        }
      }
      row_sum(q);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = row0 + u;
        const bool live = row < N_;
        const float rstd = rsqrtf(q[u] * invD + (pass == 0 ? eps1 : eps2));
        float* st = pass == 0 ? stats1 : stats2;
        if (live && st && lane == 0) *reinterpret_cast<float2*>(st + 2 * (long)row) = make_float2(s[u], rstd);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int c = (lane + 64 * i) * 4;
          if (c < D) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
              o[j] = (f[u][i][j] - s[u]) * rstd * (pass == 0 ? g1[i][j] : g2[i][j]) + (pass == 0 ? b1[i][j] : b2[i][j]);
            if (pass == 0) {
              if (live) {
                // non-temporal: the stream tensor is next read by a residual epilogue several kernels later, Y2 by the very next
                // GEMM - with an ordinary store the 131 MB of Y1 pushed Y2 out of the 256 MB Infinity Cache at 64000 x 512
                // (that GEMM 220 -> 257 us, the C2a step +0.35 ms; with the hint -0.35 ms against two launches)
                typedef uint32_t u32x4n __attribute__((ext_vector_type(4)));
                u32x4n uu = {__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3])};
                __builtin_nontemporal_store(uu, reinterpret_cast<u32x4n*>(Y1 + (long)row * ldy1 + c));
              }
#pragma unroll
              for (int j = 0; j < 4; ++j) f[u][i][j] = o[j];
            } else if (live) {
              store4<T2>(Y2 + (long)row * ldy2 + c, o);
            }
          }
        }
      }
    }
  }
}

// bwd: dx = R + rstd * (g - mean(g) - xhat * mean(g*xhat)), g = dy*act'(LN(x))*gamma.  Blocks stride over rows;
// gamma/beta of the lane's columns live in registers for the whole kernel, U rows are in flight per wave (all
// their loads issued before any reduction), dgamma/dbeta partial sums stay in registers until one atomic flush.
// Optional second output of the LayerNorm backward: dX2 = alpha * Dropout(dX; seed) * row_mask - the first thing the
// NEXT backward block does to this gradient (FFN: 1/2 * D(dy), conv module: D(dy) * mask).  Written from the registers
// that hold dX anyway, it replaces a separate elementwise pass (one more read and one more launch per module).
struct LnSecond {
  void* dX2; long ld; float alpha; const uint8_t* mask; uint32_t thresh; float scale; uint64_t seed; const uint64_t* epoch;
  // round 6 (split-K dgrads of a small batch, smx_gemm_panel_slabs): the incoming gradient dY = the sum of `nslab` float32 slabs
  // ((N, D) each, `slab_stride` elements apart, added in slab order) instead of a dtype-T tensor; null: dY as given
  const float* slabs; int nslab; long slab_stride;
};

// SLABS (the slab source, a compile-time form): the dense instantiation holds no slab loop at all - as a run-time branch inside the
// unrolled request loop it cost the dense rows 31.5 -> 37.7 us per call at C2b (56.3 -> 73.4 at C2a, 30.6 -> 38.4 at C4).
template <typename T, int VW, int CH, int U, typename TX = T, bool SLABS = false>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const T* __restrict__ dY, long lddy, const TX* __restrict__ X,
                                                            long ldx, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int act,
                                                            const float* __restrict__ stats, const T* __restrict__ R,
                                                            long ldr, T* __restrict__ dX, long lddx,
                                                            float* __restrict__ partial, int N_, int D, LnSecond sec) {
  const uint64_t sseed = sec.dX2 ? epoch_seed(sec.seed, sec.epoch) : 0;
  __shared__ float red[3][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float gam[CH][VW], bet[CH][VW], dg[CH][VW], db[CH][VW];
#pragma unroll
  for (int i = 0; i < CH; ++i)
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const int c = (lane + 64 * i) * VW + j;
      gam[i][j] = c < D ? gamma[c] : 0.f;
      bet[i][j] = (c < D && act != SMX_ACT_NONE) ? beta[c] : 0.f;
      dg[i][j] = db[i][j] = 0.f;
    }
  dispatch_act(act, [&](auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;
    for (int row0 = (blockIdx.x * 4 + w) * U; row0 < N_; row0 += gridDim.x * 4 * U) {
      float fdy[U][CH][VW], fx[U][CH][VW], fr[U][CH][VW == 4 ? 4 : 1], mean[U], rstd[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = min(row0 + u, N_ - 1);           // tail rows re-read the last row (results discarded)
        mean[u] = stats[2 * (long)row];
        rstd[u] = stats[2 * (long)row + 1];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int c = (lane + 64 * i) * VW;
          const int cc = c < D ? c : 0;                  // idle lanes re-read column 0
          if constexpr (VW == 4) {
            if constexpr (SLABS) {
              const float* sp = sec.slabs + (long)row * D + cc;
              fdy[u][i][0] = fdy[u][i][1] = fdy[u][i][2] = fdy[u][i][3] = 0.f;
              for (int s0 = 0; s0 < sec.nslab; s0 += 4) {  // four slabs in flight, summed in slab order
                float4 a4[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) a4[k] = *reinterpret_cast<const float4*>(sp + (long)min(s0 + k, sec.nslab - 1) * sec.slab_stride);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                  if (s0 + k < sec.nslab) { fdy[u][i][0] += a4[k].x; fdy[u][i][1] += a4[k].y; fdy[u][i][2] += a4[k].z; fdy[u][i][3] += a4[k].w; }
              }
            } else {
              load4<T>(dY + (long)row * lddy + cc, fdy[u][i]);
            }
            load4<TX>(X + (long)row * ldx + cc, fx[u][i]);
          }
          else { fdy[u][i][0] = to_f32(dY[(long)row * lddy + cc]); fx[u][i][0] = to_f32(X[(long)row * ldx + cc]); }
          // the residual gradient is requested with the operands: loaded after the reductions it was a second dependent
          // round trip per row group
          if constexpr (VW == 4) {
            if (R) load4<T>(R + (long)row * ldr + cc, fr[u][i]);
            else fr[u][i][0] = fr[u][i][1] = fr[u][i][2] = fr[u][i][3] = 0.f;
          }
        }
      }
      float s1[U], s2[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool rok = row0 + u < N_;
        s1[u] = s2[u] = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const bool cok = (lane + 64 * i) * VW < D;
#pragma unroll
          for (int j = 0; j < VW; ++j) {
            const float xhat = (fx[u][i][j] - mean[u]) * rstd[u];
            float dyn = (cok && rok) ? fdy[u][i][j] : 0.f;
            if constexpr (ACT != SMX_ACT_NONE) dyn *= act_grad_c<ACT>(xhat * gam[i][j] + bet[i][j]);
            const float g = dyn * gam[i][j];
            fx[u][i][j] = xhat;          // reuse registers: fx <- xhat, fdy <- g
            fdy[u][i][j] = g;
            s1[u] += g;
            s2[u] += g * xhat;
            dg[i][j] += dyn * xhat;
            db[i][j] += dyn;
          }
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) { s1[u] += __shfl_xor(s1[u], off, 64); s2[u] += __shfl_xor(s2[u], off, 64); }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = row0 + u;
        if (row >= N_) continue;
        const float m1 = s1[u] / (float)D, m2 = s2[u] / (float)D;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int c = (lane + 64 * i) * VW;
          if (c < D) {
            float o[VW];
#pragma unroll
            for (int j = 0; j < VW; ++j) o[j] = rstd[u] * (fdy[u][i][j] - m1 - fx[u][i][j] * m2);
            if constexpr (VW == 4) {
#pragma unroll
              for (int j = 0; j < 4; ++j) o[j] += fr[u][i][j];
            } else {
              if (R) o[0] += to_f32(R[(long)row * ldr + c]);
            }
            if constexpr (VW == 4) store4<T>(dX + (long)row * lddx + c, o);
            else dX[(long)row * lddx + c] = from_f32<T>(o[0]);
            if (sec.dX2) {                               // (uniform)
              const float mk = (sec.mask ? (sec.mask[row] ? 1.f : 0.f) : 1.f) * sec.alpha;
              if (sec.thresh) dropout_apply_any<VW>(o, sseed, (uint64_t)row * D + c, sec.thresh, sec.scale);
#pragma unroll
              for (int j = 0; j < VW; ++j) o[j] *= mk;
              T* d2 = reinterpret_cast<T*>(sec.dX2);
              if constexpr (VW == 4) store4<T>(d2 + (long)row * sec.ld + c, o);
              else d2[(long)row * sec.ld + c] = from_f32<T>(o[0]);
            }
          }
        }
      }
    }
  });
  // flush dgamma / dbeta: reduce the 4 waves through LDS and write ONE partial row per block (no atomics: with a
  // few thousand blocks adding into the same D addresses the L2 atomic unit serialised, 200 us per call).
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        float v = pass == 0 ? dg[i][j] : db[i][j];
        __syncthreads();
        if (w > 0) red[w - 1][lane] = v;
        __syncthreads();
        if (w == 0) {
          v = ((v + red[0][lane]) + red[1][lane]) + red[2][lane];
          const int c = (lane + 64 * i) * VW + j;
          if (c < D) partial[((long)blockIdx.x * 2 + pass) * D + c] = v;
        }
      }
  }
}

#ifndef SMX_LN_WG8_UF
#define SMX_LN_WG8_UF 2        // rows in flight per workgroup, forward
#endif
#ifndef SMX_LN_WG8_FBLOCKS
#define SMX_LN_WG8_FBLOCKS 2048
#endif
#ifndef SMX_LN_WG8_FROM
#define SMX_LN_WG8_FROM 1024   // rows wider than this (and <= 2048, bf16) take the workgroup-per-row kernels
#endif
// ---- mid-width rows (1024 < D <= 2048, bf16; the CSGU LayerNorm over 1536 channels of the Branchformer's cgMLP) ----------------
// One WORKGROUP per row, thread t owns the 8 consecutive columns 8 t (one 16-byte access per tensor and row), U rows in flight
// per iteration, workgroups stride over the rows; gamma / beta (and the dgamma / dbeta partial sums) of the thread's columns live
// in registers for the whole kernel.  The wave-per-row kernels above need 8 chunks of 4 columns per lane at this width: 128
// parameter registers per lane (backward: 256 VGPRs = ONE wave per SIMD with one 9 KB row in flight: 2.45 TB/s; forward: every
// one of the 8192 waves fetched its own 12 KB of gamma / beta for ~4 rows of 3 KB: 2.2 TB/s; tools/step_records.py c4).
__device__ __forceinline__ void ld8_bf16(const bf16_t* p, float (&f)[8]) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(w[i] << 16); f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}
__device__ __forceinline__ void st8_bf16(bf16_t* p, const float (&f)[8]) {
  *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
}
__device__ __forceinline__ void ld8_f32(const float* p, float (&f)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
// sums of U values per thread over the workgroup (4 waves): wave shuffles, then 4 partials per value through LDS
template <int U>
__device__ __forceinline__ void wg_sum(float (&v)[U], float (*red)[4], int lane, int w) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] += __shfl_xor(v[u], off, 64);
  if (lane == 0) {
#pragma unroll
    for (int u = 0; u < U; ++u) red[u][w] = v[u];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = (red[u][0] + red[u][1]) + (red[u][2] + red[u][3]);
}

template <int U>
__global__ __launch_bounds__(256) void layernorm_fwd_wg8_kernel(const bf16_t* __restrict__ X, long ldx, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, bf16_t* __restrict__ Y, long ldy,
                                                                float* __restrict__ stats, int N_, int D, float eps, int act) {
  __shared__ float red[2][U][4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, c = t * 8;
  const bool in = c < D;
  float gam[8], bet[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { gam[j] = in ? gamma[c + j] : 0.f; bet[j] = in ? beta[c + j] : 0.f; }
  const float invD = 1.f / (float)D;
  dispatch_act(act, [&](auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;
    for (int row0 = blockIdx.x * U; row0 < N_; row0 += gridDim.x * U) {
      float f[U][8], s[U], q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = min(row0 + u, N_ - 1);            // tail rows re-read the last row (results discarded)
        if (in) ld8_bf16(X + (long)row * ldx + c, f[u]);
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) f[u][j] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) s[u] = ((f[u][0] + f[u][1]) + (f[u][2] + f[u][3])) + ((f[u][4] + f[u][5]) + (f[u][6] + f[u][7]));
      wg_sum<U>(s, red[0], lane, w);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[u] *= invD;                                      // mean
        q[u] = 0.f;
        if (in) {
#pragma unroll
          for (int j = 0; j < 8; ++j) { const float d = f[u][j] - s[u]; q[u] += d * d; }
        }
      }
      wg_sum<U>(q, red[1], lane, w);                       // (red[0] is rewritten only after this barrier: no race)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = row0 + u;
        if (row >= N_) break;
        const float rstd = rsqrtf(q[u] * invD + eps);
        if (stats && t == 0) *reinterpret_cast<float2*>(stats + 2 * (long)row) = make_float2(s[u], rstd);
        if (in) {
          float o[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = act_fwd_c<ACT>((f[u][j] - s[u]) * rstd * gam[j] + bet[j]);
          st8_bf16(Y + (long)row * ldy + c, o);
        }
      }
    }
  });
}

// backward (see layernorm_bwd_kernel for the formulas); TX = float: the LayerNorm input is the fp32 residual stream.
// Software-pipelined over the rows of the workgroup: the operands of row i + 1 are requested before row i is reduced, and stay
// PACKED (the 16 bytes as loaded) until they are consumed - 4 registers per bf16 tensor and row instead of 8, unpacked once for
// the row sums and once more for the outputs.  With one row in flight and nothing prefetched the kernel ran at the latency
// bound of 4 workgroups x 9 KB per CU (4.7 TB/s plain, 3.6 TB/s with the extra Z stream of PRE).
// PRE (smx_ln_bwd.Z): the LayerNorm input is X = zact(Z); the kernel then emits the gradient w.r.t. Z,
// dX * zact'(Z), from the registers that hold dX - the consumer's activation-backward pass over this tensor is gone.
template <typename TX>
struct LnRaw {
  uint4 dy, r, z;
  uint4 x0, x1;                                            // (bf16 x: x0 only)
  float mean, rstd;
};
__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(w[i] << 16); f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}
template <bool PRE, typename TX>
__global__ __launch_bounds__(256, 4) void layernorm_bwd_wg8_kernel(const bf16_t* __restrict__ dY, long lddy, const TX* __restrict__ X, long ldx,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta, int act,
                                                                   const float* __restrict__ stats, const bf16_t* __restrict__ R, long ldr,
                                                                   bf16_t* __restrict__ dX, long lddx, float* __restrict__ partial, int N_, int D,
                                                                   const bf16_t* __restrict__ Zp, long ldz, int zact) {
  __shared__ float red[2][2][4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, c = t * 8;
  const bool in = c < D;
  const int cc = in ? c : 0;                               // (idle threads re-read column 0; their results are masked)
  float gam[8], bet[8], dg[8], db[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    gam[j] = in ? gamma[c + j] : 0.f;
    bet[j] = (in && act != SMX_ACT_NONE) ? beta[c + j] : 0.f;
    dg[j] = db[j] = 0.f;
  }
  const float invD = 1.f / (float)D;
  auto fetch = [&](int row, LnRaw<TX>& q) {
    q.mean = stats[2 * (long)row];
    q.rstd = stats[2 * (long)row + 1];
    q.dy = *reinterpret_cast<const uint4*>(dY + (long)row * lddy + cc);
    if constexpr (sizeof(TX) == 4) {
      const float* xp = reinterpret_cast<const float*>(X) + (long)row * ldx + cc;
      q.x0 = *reinterpret_cast<const uint4*>(xp);
      q.x1 = *reinterpret_cast<const uint4*>(xp + 4);
    } else {
      q.x0 = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(X) + (long)row * ldx + cc);
    }
    if constexpr (!PRE) {
      if (R) q.r = *reinterpret_cast<const uint4*>(R + (long)row * ldr + cc);   // (uniform; the PRE variant has no residual gradient)
    }
    if constexpr (PRE) q.z = *reinterpret_cast<const uint4*>(Zp + (long)row * ldz + cc);
  };
  auto xhat8 = [&](const LnRaw<TX>& q, float (&xh)[8]) {
    if constexpr (sizeof(TX) == 4) {
      const uint32_t wv[8] = {q.x0.x, q.x0.y, q.x0.z, q.x0.w, q.x1.x, q.x1.y, q.x1.z, q.x1.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) xh[j] = (__uint_as_float(wv[j]) - q.mean) * q.rstd;
    } else {
      unpack8(q.x0, xh);
#pragma unroll
      for (int j = 0; j < 8; ++j) xh[j] = (xh[j] - q.mean) * q.rstd;
    }
  };
  auto body = [&](auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;
    LnRaw<TX> cur, nxt;
    int row = blockIdx.x, it = 0;
    if (row < N_) fetch(row, cur);
    for (; row < N_; row += gridDim.x, ++it) {
      const int rn = row + gridDim.x;
      if (rn < N_) fetch(rn, nxt);                         // the next row is in flight while this one is reduced
      float g[8], xh[8];
      unpack8(cur.dy, g);
      xhat8(cur, xh);
      float ss[2] = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float dyn = in ? g[j] : 0.f;
        if constexpr (ACT != SMX_ACT_NONE) dyn *= act_grad_c<ACT>(xh[j] * gam[j] + bet[j]);
        const float xq = in ? xh[j] : 0.f;
        const float gg = dyn * gam[j];
        ss[0] += gg;
        ss[1] += gg * xq;
        dg[j] += dyn * xq;
        db[j] += dyn;
      }
      wg_sum<2>(ss, red[it & 1], lane, w);                 // (alternating buffers: ONE barrier per row)
      if (in) {
        const float m1 = ss[0] * invD, m2 = ss[1] * invD;
        float o[8];
        unpack8(cur.dy, g);                                // (unpacked again instead of kept: 16 registers less across the barrier)
        xhat8(cur, xh);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float dyn = g[j];
          if constexpr (ACT != SMX_ACT_NONE) dyn *= act_grad_c<ACT>(xh[j] * gam[j] + bet[j]);
          o[j] = cur.rstd * (dyn * gam[j] - m1 - xh[j] * m2);
        }
        if constexpr (!PRE) {
          if (R) {
            float rr[8];
            unpack8(cur.r, rr);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] += rr[j];
          }
        }
        if constexpr (PRE) {
          float zz[8];
          unpack8(cur.z, zz);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] *= act_grad(zact, zz[j]);
        }
        st8_bf16(dX + (long)row * lddx + c, o);
      }
      cur = nxt;
    }
  };
  if constexpr (PRE) body(ActTag<SMX_ACT_NONE>{});           // (the PRE entry point takes a plain LayerNorm only: one instantiation, no spills)
  else dispatch_act(act, body);
  if (in) {                                                // ONE partial row pair per workgroup (fixed-order reduction downstream)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      partial[((long)blockIdx.x * 2) * D + c + j] = dg[j];
      partial[((long)blockIdx.x * 2 + 1) * D + c + j] = db[j];
    }
  }
}

// wide rows (2048 < D <= 4096, e.g. the (F,C) = 40x64 LayerNorm of the conv front-end): one WORKGROUP per row at a
// time, thread t owns columns t + 256*i; row statistics through an LDS reduction; same partial-row flush as above.
template <typename T, int CH>
__global__ __launch_bounds__(256) void layernorm_bwd_wide_kernel(const T* __restrict__ dY, long lddy, const T* __restrict__ X,
                                                                 long ldx, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, int act,
                                                                 const float* __restrict__ stats, const T* __restrict__ R,
                                                                 long ldr, T* __restrict__ dX, long lddx,
                                                                 float* __restrict__ partial, int N_, int D) {
  __shared__ float red[2][4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  float gam[CH], bet[CH], dg[CH], db[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = t + 256 * i;
    gam[i] = c < D ? gamma[c] : 0.f;
    bet[i] = (c < D && act != SMX_ACT_NONE) ? beta[c] : 0.f;
    dg[i] = db[i] = 0.f;
  }
  for (int row = blockIdx.x; row < N_; row += gridDim.x) {
    const float mean = stats[2 * (long)row], rstd = stats[2 * (long)row + 1];
    float g[CH], xh[CH], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = t + 256 * i;
      g[i] = xh[i] = 0.f;
      if (c < D) {
        const float xhat = (to_f32(X[(long)row * ldx + c]) - mean) * rstd;
        float dyn = to_f32(dY[(long)row * lddy + c]);
        if (act != SMX_ACT_NONE) dyn *= act_grad(act, xhat * gam[i] + bet[i]);
        g[i] = dyn * gam[i]; xh[i] = xhat;
        s1 += g[i]; s2 += g[i] * xhat;
        dg[i] += dyn * xhat; db[i] += dyn;
      }
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    __syncthreads();
    if (lane == 0) { red[0][w] = s1; red[1][w] = s2; }
    __syncthreads();
    const float m1 = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)D;
    const float m2 = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)D;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = t + 256 * i;
      if (c < D) {
        float o = rstd * (g[i] - m1 - xh[i] * m2);
        if (R) o += to_f32(R[(long)row * ldr + c]);
        dX[(long)row * lddx + c] = from_f32<T>(o);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = t + 256 * i;
    if (c < D) { partial[((long)blockIdx.x * 2) * D + c] = dg[i]; partial[((long)blockIdx.x * 2 + 1) * D + c] = db[i]; }
  }
}

// the same with 4 consecutive columns per thread (8-byte accesses in bf16): thread t owns columns (t + 256 i) * 4 .. + 3.
// The 2-byte accesses of the kernel above cap it at the vector-memory issue rate (1.58 ms for the 2 GB of the front-end's
// (128128, 2560) LayerNorm backward = 1.3 TB/s).
template <typename T, int CH>
__global__ __launch_bounds__(256) void layernorm_bwd_wide4_kernel(const T* __restrict__ dY, long lddy, const T* __restrict__ X,
                                                                  long ldx, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, int act,
                                                                  const float* __restrict__ stats, const T* __restrict__ R,
                                                                  long ldr, T* __restrict__ dX, long lddx,
                                                                  float* __restrict__ partial, int N_, int D) {
  __shared__ float red[2][4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  float gam[CH][4], bet[CH][4], dg[CH][4], db[CH][4];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (t + 256 * i) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      gam[i][q] = c < D ? gamma[c + q] : 0.f;
      bet[i][q] = (c < D && act != SMX_ACT_NONE) ? beta[c + q] : 0.f;
      dg[i][q] = db[i][q] = 0.f;
    }
  }
  for (int row = blockIdx.x; row < N_; row += gridDim.x) {
    const float mean = stats[2 * (long)row], rstd = stats[2 * (long)row + 1];
    float g[CH][4], xh[CH][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (t + 256 * i) * 4;
      if (c < D) {
        load4<T>(X + (long)row * ldx + c, xh[i]);
        load4<T>(dY + (long)row * lddy + c, g[i]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) g[i][q] = xh[i][q] = 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float xhat = (xh[i][q] - mean) * rstd;
        float dyn = g[i][q];
        if (act != SMX_ACT_NONE) dyn *= act_grad(act, xhat * gam[i][q] + bet[i][q]);
        const bool in = (t + 256 * i) * 4 < D;
        xh[i][q] = in ? xhat : 0.f;
        dyn = in ? dyn : 0.f;
        g[i][q] = dyn * gam[i][q];
        s1 += g[i][q]; s2 += g[i][q] * xh[i][q];
        dg[i][q] += dyn * xh[i][q]; db[i][q] += dyn;
      }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    __syncthreads();
    if (lane == 0) { red[0][w] = s1; red[1][w] = s2; }
    __syncthreads();
    const float m1 = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)D;
    const float m2 = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)D;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (t + 256 * i) * 4;
      if (c < D) {
        float o[4], rr[4] = {0.f, 0.f, 0.f, 0.f};
        if (R) load4<T>(R + (long)row * ldr + c, rr);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = rstd * (g[i][q] - m1 - xh[i][q] * m2) + rr[q];
        store4<T>(dX + (long)row * lddx + c, o);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (t + 256 * i) * 4;
    if (c < D) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        partial[((long)blockIdx.x * 2) * D + c + q] = dg[i][q];
        partial[((long)blockIdx.x * 2 + 1) * D + c + q] = db[i][q];
      }
    }
  }
}

// dgamma[c] += sum_b partial[b][0][c]; dbeta[c] += sum_b partial[b][1][c]   (fixed order => bit-reproducible)
// block = 32 columns x 8 row groups; every thread sums nblocks/8 partial rows with 4 independent accumulators.
__global__ __launch_bounds__(256) void ln_param_reduce_kernel(const float* __restrict__ partial, int nblocks, int D,
                                                              float* dgamma, float* dbeta) {
  __shared__ float red[16][16];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cx;                 // index into the concatenated [dgamma | dbeta] row of 2*D
  const bool ok = c < 2 * D;
  const int pass = ok ? c / D : 0, col = ok ? c % D : 0;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int b = ry;
  for (; b + 48 < nblocks; b += 64) {
    s0 += partial[((long)b * 2 + pass) * D + col];
    s1 += partial[((long)(b + 16) * 2 + pass) * D + col];
    s2 += partial[((long)(b + 32) * 2 + pass) * D + col];
    s3 += partial[((long)(b + 48) * 2 + pass) * D + col];
  }
  for (; b < nblocks; b += 16) s0 += partial[((long)b * 2 + pass) * D + col];
  red[ry][cx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ry == 0 && ok) {
    float tot = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot += red[r][cx];
    float* dst = pass == 0 ? dgamma : dbeta;
    dst[col] += tot;
  }
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

#ifndef SMX_LNB_BLOCKS
#define SMX_LNB_BLOCKS 1024
#endif
static int ln_bwd_blocks(int N) {
  int blocks = (N + 3) / 4;                              // one row per wave and pass when the rows allow it (D <= 512 keeps ONE row in flight)
  return blocks > SMX_LNB_BLOCKS ? SMX_LNB_BLOCKS : (blocks < 1 ? 1 : blocks);
}

#ifndef SMX_LNB_U1
#define SMX_LNB_U1 2      // rows in flight per wave for D <= 256
#endif
#ifndef SMX_LNB_U2
#define SMX_LNB_U2 1      // ... for 256 < D <= 512 (104 registers = 4 waves per SIMD = the whole 1024-block grid resident; two rows in flight: 75 -> 62 us at 64000 x 512, tools/rowkernels_bench.py)
#endif

extern "C" int smx_layernorm_bwd_blocks(int N) { return ln_bwd_blocks(N); }
extern "C" size_t smx_layernorm_bwd_workspace(int N, int D) { return (size_t)ln_bwd_blocks(N) * 2 * D * sizeof(float); }

// a row operand: NULL, or `align`-byte aligned with a leading dimension that is a multiple of `ldm` elements
static bool rows_ok(const void* p, int64_t ld, size_t align, int ldm) {
  return p == nullptr || ((reinterpret_cast<uintptr_t>(p) % align) == 0 && ld % ldm == 0);
}

// The forward's kernel.  T: Y, TX: X (float next to a bf16 Y: the fp32 residual stream); the pair form has T = TX = float.
template <typename T, typename TX>
static int ln_fwd_launch(const smx_ln_fwd& a, hipStream_t s) {
  const int N = a.N, D = a.D;
  const bool pair = a.Y2 != nullptr, x32 = !std::is_same<T, TX>::value;
  const size_t es2 = a.dtype2 == SMX_BF16 ? 2 : 4;
  const bool vec = D % 4 == 0 && rows_ok(a.X, a.ldx, 4 * sizeof(TX), 4) && rows_ok(a.Y, a.ldy, 4 * sizeof(T), 4) && aligned16(a.gamma) &&
                   aligned16(a.beta) && (!pair || (rows_ok(a.Y2, a.ldy2, 4 * es2, 4) && aligned16(a.gamma2) && aligned16(a.beta2)));
  if ((pair || x32) && !(vec && D <= 2048))
    return fail(SMX_EUNSUPPORTED, "smx_layernorm_fwd: the pair and float32-X forms need D %% 4 == 0, D <= 2048 and aligned rows");
  if (sizeof(T) == 2 && !x32 && vec && D > SMX_LN_WG8_FROM && D <= 2048 && D % 8 == 0 && rows_ok(a.X, a.ldx, 16, 8) && rows_ok(a.Y, a.ldy, 16, 8)) {
    // mid-width rows: one workgroup per row, 16-byte accesses (layernorm_fwd_wg8_kernel)
    int blocks = (N + SMX_LN_WG8_UF - 1) / SMX_LN_WG8_UF;
    if (blocks > SMX_LN_WG8_FBLOCKS) blocks = SMX_LN_WG8_FBLOCKS;
    hipLaunchKernelGGL((layernorm_fwd_wg8_kernel<SMX_LN_WG8_UF>), dim3(blocks), dim3(256), 0, s, (const bf16_t*)a.X, a.ldx, a.gamma, a.beta,
                       (bf16_t*)a.Y, a.ldy, a.stats, N, D, a.eps, a.act);
    return SMX_OK;
  }
  if (vec && D <= 2048) {
    const int ch = (D + 255) / 256;
    const int U = ch <= 1 ? 4 : (ch <= 2 ? 2 : 1);          // (the pair kernel keeps the launch geometry of layernorm_fwd_fast: bit-identical sums)
    int blocks = (N + 4 * U - 1) / (4 * U);
    if (blocks > 2048) blocks = 2048;
    const dim3 grid(blocks);
#define LN_CH(LAUNCH) do { if (ch <= 1) LAUNCH(1, 4); else if (ch <= 2) LAUNCH(2, 2); else if (ch <= 4) LAUNCH(4, 1); else LAUNCH(8, 1); } while (0)
#define LN_FAST(CH, U_) hipLaunchKernelGGL((layernorm_fwd_fast<T, CH, U_, TX>), grid, dim3(256), 0, s, (const TX*)a.X, a.ldx, a.gamma, a.beta, (T*)a.Y, a.ldy, \
                                           a.stats, N, D, a.eps, a.act)
#define LN_PAIR(CH, U_) hipLaunchKernelGGL((layernorm_fwd_pair_fast<T2, CH, U_>), grid, dim3(256), 0, s, (const float*)a.X, a.ldx, a.gamma, a.beta, a.eps, \
                                           (float*)a.Y, a.ldy, a.stats, a.gamma2, a.beta2, a.eps2, (T2*)a.Y2, a.ldy2, a.stats2, N, D)
    if (!pair) LN_CH(LN_FAST);
    else if (a.dtype2 == SMX_BF16) { typedef bf16_t T2; LN_CH(LN_PAIR); }
    else { typedef float T2; LN_CH(LN_PAIR); }
#undef LN_PAIR
#undef LN_FAST
#undef LN_CH
    return SMX_OK;
  }
  if constexpr (std::is_same<T, TX>::value) {
    const dim3 grid((N + 3) / 4);
#define LN_GENERIC(V) hipLaunchKernelGGL((layernorm_fwd_kernel<T, V>), grid, dim3(256), 0, s, (const T*)a.X, a.ldx, a.gamma, a.beta, (T*)a.Y, a.ldy, a.stats, \
                                         N, D, a.eps, a.act)
    if (vec) LN_GENERIC(true); else LN_GENERIC(false);
#undef LN_GENERIC
  }
  return SMX_OK;
}

extern "C" int smx_layernorm_fwd(const smx_ln_fwd* a, void* stream) {
  SMX_REQUIRE(a && a->X && a->Y && a->gamma && a->beta && a->N >= 0 && a->D > 0, "smx_layernorm_fwd: bad arguments");
  const bool x32 = a->x_f32 && a->dtype != SMX_F32;
  SMX_REQUIRE(!x32 || a->dtype == SMX_BF16, "smx_layernorm_fwd: bad dtype");
  SMX_REQUIRE(!a->Y2 || (a->gamma2 && a->beta2 && a->dtype == SMX_F32 && a->act == SMX_ACT_NONE && (a->dtype2 == SMX_BF16 || a->dtype2 == SMX_F32)),
              "smx_layernorm_fwd: the pair form needs gamma2 / beta2, a float32 Y, no activation and dtype2 bf16 or float32");
  if (a->N == 0) return SMX_OK;
  hipStream_t s = STREAM;
  const int rc = a->dtype != SMX_BF16 ? ln_fwd_launch<float, float>(*a, s)
                 : x32 ? ln_fwd_launch<bf16_t, float>(*a, s) : ln_fwd_launch<bf16_t, bf16_t>(*a, s);
  return rc != SMX_OK ? rc : check_launch("smx_layernorm_fwd");
}

// The backward's kernel.  T: dY / R / dX / dX2, TX: X.  partial = the workspace; `blocks` partial rows.
template <typename T, typename TX>
static int ln_bwd_launch(const smx_ln_bwd& a, const LnSecond& sec, int blocks, hipStream_t s) {
  const int N = a.N, D = a.D, act = a.act;
  const bool x32 = !std::is_same<T, TX>::value;
  const dim3 grid(blocks);
  float* partial = reinterpret_cast<float*>(a.workspace);
#define LN_WG8(PRE, TXX, ZP, LDZ, ZACT) hipLaunchKernelGGL((layernorm_bwd_wg8_kernel<PRE, TXX>), grid, dim3(256), 0, s, (const bf16_t*)a.dY, a.lddy, \
                                                           (const TXX*)a.X, a.ldx, a.gamma, a.beta, act, a.stats, (const bf16_t*)a.R, a.ldr, \
                                                           (bf16_t*)a.dX, a.lddx, partial, N, D, (const bf16_t*)ZP, LDZ, ZACT)
  auto ok16 = [](const void* p, int64_t ld) { return rows_ok(p, ld, 16, 8); };
  if (a.Z) {
    if (act != SMX_ACT_NONE)
      return fail(SMX_EUNSUPPORTED, "smx_layernorm_bwd: the pre-activation form is for a LayerNorm without a fused activation of its own");
    if (sizeof(T) != 2 || D > 2048 || D % 8 != 0 || !ok16(a.dY, a.lddy) || !ok16(a.X, a.ldx) || !ok16(a.Z, a.ldz) || !ok16(a.dX, a.lddx))
      return fail(SMX_EUNSUPPORTED, "smx_layernorm_bwd: the pre-activation form needs bf16, D <= 2048, D %% 8 == 0 and 16-byte aligned rows");
    LN_WG8(true, bf16_t, a.Z, a.ldz, a.zact);
    return SMX_OK;
  }
  const size_t vb = 4 * sizeof(T);
  const bool vec = D % 4 == 0 && rows_ok(a.dY, a.lddy, vb, 4) && rows_ok(a.X, a.ldx, 4 * sizeof(TX), 4) && rows_ok(a.R, a.ldr, vb, 4) &&
                   rows_ok(a.dX, a.lddx, vb, 4) && rows_ok(a.dX2, a.lddx2, vb, 4) && (!a.slabs || (aligned16(a.slabs) && a.slab_stride % 4 == 0));
  if (a.dX2 && D > 2048) return fail(SMX_EUNSUPPORTED, "smx_layernorm_bwd: the second output needs D <= 2048");
  if ((x32 || a.slabs) && !(vec && D <= 2048))
    return fail(SMX_EUNSUPPORTED, "smx_layernorm_bwd: float32 X and slabs need D %% 4 == 0, D <= 2048 and aligned rows");
  if (sizeof(T) == 2 && vec && !a.slabs && !a.dX2 && D > SMX_LN_WG8_FROM && D <= 2048 && D % 8 == 0 && ok16(a.dY, a.lddy) && ok16(a.X, a.ldx) &&
      ok16(a.R, a.ldr) && ok16(a.dX, a.lddx)) {
    LN_WG8(false, TX, nullptr, 0, SMX_ACT_NONE);
    return SMX_OK;
  }
#undef LN_WG8
#define LN_ROWS_(VW, CH, U, SLABS) hipLaunchKernelGGL((layernorm_bwd_kernel<T, VW, CH, U, TX, SLABS>), grid, dim3(256), 0, s, (const T*)a.dY, a.lddy, (const TX*)a.X, a.ldx, \
                                                      a.gamma, a.beta, act, a.stats, (const T*)a.R, a.ldr, (T*)a.dX, a.lddx, partial, N, D, sec)
#define LN_ROWS(VW, CH, U) LN_ROWS_(VW, CH, U, false)
#define LN_SLAB(CH) LN_ROWS_(4, CH, 1, true)
#define LN_WIDE(KERNEL, CH) hipLaunchKernelGGL((KERNEL<T, CH>), grid, dim3(256), 0, s, (const T*)a.dY, a.lddy, (const T*)a.X, a.ldx, a.gamma, a.beta, \
                                               act, a.stats, (const T*)a.R, a.ldr, (T*)a.dX, a.lddx, partial, N, D)
  if (vec && D <= 2048) {
    if (!a.slabs) {
      if (D <= 256) LN_ROWS(4, 1, SMX_LNB_U1); else if (D <= 512) LN_ROWS(4, 2, SMX_LNB_U2); else if (D <= 1024) LN_ROWS(4, 4, 1); else LN_ROWS(4, 8, 1);
    } else if constexpr (sizeof(T) == 2) {      // (the slab sums: one row in flight per wave at every width)
      if (D <= 256) LN_SLAB(1); else if (D <= 512) LN_SLAB(2); else if (D <= 1024) LN_SLAB(4); else LN_SLAB(8);
    }
  } else if constexpr (std::is_same<T, TX>::value) {     // (float32 X and slabs stopped above)
    if (vec) {
      if (D <= 3072) LN_WIDE(layernorm_bwd_wide4_kernel, 3);
      else if (D <= 4096) LN_WIDE(layernorm_bwd_wide4_kernel, 4);
      else return fail(SMX_EUNSUPPORTED, "smx_layernorm_bwd: D=%d > 4096", D);
    } else {
      if (D <= 256) LN_ROWS(1, 4, 1); else if (D <= 1024) LN_ROWS(1, 16, 1); else if (D <= 2048) LN_ROWS(1, 32, 1);
      else if (D <= 4096) LN_WIDE(layernorm_bwd_wide_kernel, 16);
      else return fail(SMX_EUNSUPPORTED, "smx_layernorm_bwd: D=%d > 4096", D);
    }
  }
#undef LN_WIDE
#undef LN_SLAB
#undef LN_ROWS
#undef LN_ROWS_
  return SMX_OK;
}

extern "C" int smx_layernorm_bwd(const smx_ln_bwd* a, void* stream) {
  SMX_REQUIRE(a && a->X && a->gamma && a->beta && a->stats && a->dX && a->workspace && a->D > 0 && ((a->dgamma == nullptr) == (a->dbeta == nullptr)),
              "smx_layernorm_bwd: bad arguments");
  SMX_REQUIRE((a->dY == nullptr) != (a->slabs == nullptr), "smx_layernorm_bwd: exactly one of dY and slabs");
  SMX_REQUIRE(!a->slabs || (a->dtype == SMX_BF16 && a->nslab >= 1 && a->nslab <= 16 && !a->dgamma),
              "smx_layernorm_bwd: slabs need bf16, 1 <= nslab <= 16 and dgamma = dbeta = NULL");
  const bool x32 = a->x_f32 && a->dtype != SMX_F32;
  SMX_REQUIRE(!x32 || a->dtype == SMX_BF16, "smx_layernorm_bwd: bad dtype");
  SMX_REQUIRE(!a->Z || (!a->slabs && !a->R && !a->dX2 && !x32), "smx_layernorm_bwd: the pre-activation form takes no slabs, R, dX2 or float32 X");
  SMX_REQUIRE(a->drop_p2 >= 0.f && a->drop_p2 < 1.f, "smx_layernorm_bwd: 0 <= drop_p2 < 1");
  if (a->N == 0) return SMX_OK;
  LnSecond sec;
  sec.slabs = a->slabs; sec.nslab = a->nslab; sec.slab_stride = a->slab_stride;
  sec.dX2 = a->dX2; sec.ld = a->lddx2; sec.alpha = a->alpha2; sec.mask = a->row_mask2;
  sec.thresh = (uint32_t)((double)a->drop_p2 * 4294967296.0); sec.scale = 1.f / (1.f - a->drop_p2); sec.seed = a->drop_seed2; sec.epoch = a->epoch;
  const int blocks = ln_bwd_blocks(a->N);
  hipStream_t s = STREAM;
  const int rc = a->dtype != SMX_BF16 ? ln_bwd_launch<float, float>(*a, sec, blocks, s)
                 : x32 ? ln_bwd_launch<bf16_t, float>(*a, sec, blocks, s) : ln_bwd_launch<bf16_t, bf16_t>(*a, sec, blocks, s);
  if (rc != SMX_OK) return rc;
  if (a->dgamma)   // (NULL dgamma/dbeta: the partial rows stay in the workspace for a deferred smx_reduce_jobs)
    hipLaunchKernelGGL(ln_param_reduce_kernel, dim3((2 * a->D + 15) / 16), dim3(256), 0, s, (const float*)a->workspace, blocks, a->D, a->dgamma, a->dbeta);
  return check_launch("smx_layernorm_bwd");
}
