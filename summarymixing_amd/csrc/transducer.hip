// transducer.hip — the transducer head that the reference recipe trains on (recipe keys `Tjoint`, `transducer_lin`,
// `transducer_cost`: speechbrain.nnet.transducer.transducer_joint.Transducer_joint with joint = "sum", a bias-free Linear to
// the vocabulary and speechbrain.nnet.losses.transducer_loss), gfx950 only.
//
// Lattice rows are ordered (b, t, u), u fastest: row = (b T + t) U1 + u, U1 = U + 1.  H and the logits are the (B, T, U1, .)
// tensors viewed as rows.  Per row the loss needs three fp32 numbers only: lse, lp_blank = z_blank - lse, lp_y = z_y - lse
// (y = targets[b, u] for u < U).  Two ways in share the lattice kernels:
//   drop-in: joint -> logits (the ordinary GEMM) -> row statistics -> DP -> logit gradient (three passes over the logits);
//   fused:   joint -> GEMM whose epilogue keeps only per-(row, column tile) (max, sum exp) partials and z_blank / z_y -> combine
//            -> DP; backward: the same GEMM recomputed, its epilogue turns the tile into dz in registers and stores it once.
// Every reduction has a fixed order (no atomics): losses and gradients are bit-reproducible.
#include "head_tile.h"

namespace smx {

static constexpr double TR_NEG_INF64 = -__builtin_inf();
__device__ __forceinline__ double lae2(double a, double b) {       // log(exp a + exp b), -inf safe
  const double m = fmax(a, b);
  if (m == TR_NEG_INF64) return TR_NEG_INF64;
  return m + log1p(exp(-fabs(a - b)));
}

// the target token of lattice row n (-1 on the u = U column, which emits no label)
__device__ __forceinline__ int row_target(const int32_t* targets, int n, int T, int U1) {
  const int U = U1 - 1;
  const int u = n % U1;
  if (u >= U) return -1;
  const int b = n / (T * U1);
  return targets[(long)b * U + u];
}

// act' as torch differentiates it: LeakyReLU's slope at exactly 0 (torch: x > 0 ? 1 : slope; act_grad_c takes 1 there, and
// bf16 streams hit enc + dec == 0 exactly)
template <int ACT>
__device__ __forceinline__ float joint_grad(float v) {
  if constexpr (ACT == SMX_ACT_LEAKY_RELU) return v > 0.f ? 1.f : 0.01f;
  else return act_grad_c<ACT>(v);
}

// ---- joint: H[b,t,u,:] = act(enc[b,t,:] + dec[b,u,:]).  One workgroup per (b, t): its U1 rows of H are contiguous. -----------
template <typename T, int ACT>
__global__ __launch_bounds__(256) void joint_fwd_kernel(const T* __restrict__ enc, const T* __restrict__ dec, T* __restrict__ H,
                                                        int Tm, int U1, int J) {
  const int bt = blockIdx.x, b = bt / Tm;
  const T* e = enc + (long)bt * J;
  const T* d = dec + (long)b * U1 * J;
  T* h = H + (long)bt * U1 * J;
  const int JQ = J >> 2;
  for (int i = threadIdx.x; i < U1 * JQ; i += 256) {
    const int u = i / JQ, j = (i - u * JQ) * 4;
    float x[4], y[4];
    load4(e + j, x);
    load4(d + (long)u * J + j, y);
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = act_fwd_c<ACT>(x[q] + y[q]);
    store4(h + (long)u * J + j, x);
  }
}

// d_enc[b,t,:] = sum_u dH[b,t,u,:] act'(enc + dec), u in increasing order (the U1 rows of one (b, t) are contiguous)
template <typename T, int ACT>
__global__ __launch_bounds__(256) void joint_bwd_enc_kernel(const T* __restrict__ dH, const T* __restrict__ enc,
                                                            const T* __restrict__ dec, T* __restrict__ d_enc, int Tm, int U1, int J) {
  const int bt = blockIdx.x, b = bt / Tm;
  const T* e = enc + (long)bt * J;
  const T* d = dec + (long)b * U1 * J;
  const T* g = dH + (long)bt * U1 * J;
  for (int j = threadIdx.x * 4; j < J; j += 1024) {
    float x[4], s[4] = {0.f, 0.f, 0.f, 0.f};
    load4(e + j, x);
    for (int u = 0; u < U1; ++u) {
      float y[4], gg[4];
      load4(d + (long)u * J + j, y);
      load4(g + (long)u * J + j, gg);
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += gg[q] * joint_grad<ACT>(x[q] + y[q]);
    }
    store4(d_enc + (long)bt * J + j, s);
  }
}

// d_dec partials: P[b, tb, u, :] = sum_{t in t-block tb} dH[b,t,u,:] act'(enc + dec), t increasing.  One workgroup per (b, tb, u).
static constexpr int JOINT_TB = 32;
template <typename T, int ACT>
__global__ __launch_bounds__(256) void joint_bwd_dec_partial_kernel(const T* __restrict__ dH, const T* __restrict__ enc,
                                                                    const T* __restrict__ dec, float* __restrict__ P, int Tm,
                                                                    int U1, int J, int NTB) {
  const int u = blockIdx.x % U1, btb = blockIdx.x / U1, tb = btb % NTB, b = btb / NTB;
  const int t0 = tb * JOINT_TB, t1 = min(Tm, t0 + JOINT_TB);
  const T* d = dec + ((long)b * U1 + u) * J;
  float* out = P + (((long)b * NTB + tb) * U1 + u) * J;
  for (int j = threadIdx.x * 4; j < J; j += 1024) {
    float y[4], s[4] = {0.f, 0.f, 0.f, 0.f};
    load4(d + j, y);
    for (int t = t0; t < t1; ++t) {
      float x[4], gg[4];
      load4(enc + ((long)b * Tm + t) * J + j, x);
      load4(dH + (((long)b * Tm + t) * U1 + u) * J + j, gg);
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += gg[q] * joint_grad<ACT>(x[q] + y[q]);
    }
    *reinterpret_cast<float4*>(out + j) = make_float4(s[0], s[1], s[2], s[3]);
  }
}

// d_dec[b,u,:] = sum_tb P[b, tb, u, :], tb increasing
template <typename T>
__global__ __launch_bounds__(256) void joint_bwd_dec_sum_kernel(const float* __restrict__ P, T* __restrict__ d_dec, int U1, int J,
                                                                int NTB) {
  const int bu = blockIdx.x, b = bu / U1, u = bu % U1;
  for (int j = threadIdx.x * 4; j < J; j += 1024) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int tb = 0; tb < NTB; ++tb) {
      const float4 v = *reinterpret_cast<const float4*>(P + (((long)b * NTB + tb) * U1 + u) * J + j);
      s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
    }
    store4(d_dec + (long)bu * J + j, s);
  }
}

// ---- drop-in row statistics: one wave per row of the logits --------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void row_stats_kernel(const T* __restrict__ Z, long ldz, const int32_t* __restrict__ targets,
                                                        int rows, int Tm, int U1, int V, int blank, float* __restrict__ lse,
                                                        float* __restrict__ lpb, float* __restrict__ lpy) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= rows) return;
  const T* z = Z + (long)n * ldz;
  float m, s;
  row_max_sumexp(z, V, lane, m, s);
  if (lane == 0) {
    const float l = m + logf(s);
    const int y = row_target(targets, n, Tm, U1);
    lse[n] = l;
    lpb[n] = to_f32(z[blank]) - l;
    lpy[n] = (y >= 0 && y < V) ? to_f32(z[y]) - l : 0.f;
  }
}

// ---- lattice DP: one workgroup per utterance, one anti-diagonal d = t + u per step, u across the threads --------------------
// alpha(0,0) = 0; alpha(t,u) = lae(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpy(t,u-1)); nll = -(alpha(Tb-1,Ub) + lpb(Tb-1,Ub)).
// LDS holds two diagonals indexed by u; the emissions of diagonal d + 1 are requested before diagonal d is combined.
// The recursion runs in fp64: alpha and beta reach |log P| ~ 10^3 at the recipe's lattices, where one fp32 ulp (~1e-4) already
// shows as a relative error of the gradient coefficients exp(alpha + lp + beta - log P).  alpha (B T U1 doubles) is followed by
// -log P in fp64 (B doubles) for the backward; nll (fp32) is the loss.
__device__ __forceinline__ void utt_lengths(const int32_t* in_len, const int32_t* tgt_len, int b, int Tm, int U1, int& Tb, int& Ub) {
  Tb = min(max(in_len[b], 1), Tm);
  Ub = min(max(tgt_len[b], 0), U1 - 1);
}

template <int KS>
__global__ __launch_bounds__(256) void rnnt_alpha_kernel(const float* __restrict__ lpb, const float* __restrict__ lpy,
                                                         const int32_t* __restrict__ in_len, const int32_t* __restrict__ tgt_len,
                                                         int Tm, int U1, double* __restrict__ alpha, float* __restrict__ nll) {
  extern __shared__ double shd[];                        // 2 * U1 doubles
  const int b = blockIdx.x;
  int Tb, Ub;
  utt_lengths(in_len, tgt_len, b, Tm, U1, Tb, Ub);
  const long base = (long)b * Tm * U1;
  double* prev = shd;
  double* cur = shd + U1;
  float eb[KS], ey[KS], nb[KS], ny[KS];
  auto fetch = [&](int d, float (&fb)[KS], float (&fy)[KS]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int u = threadIdx.x + 256 * k, t = d - u;
      fb[k] = (u <= Ub && t >= 1 && t < Tb) ? lpb[base + (long)(t - 1) * U1 + u] : 0.f;
      fy[k] = (u <= Ub && u >= 1 && t >= 0 && t < Tb) ? lpy[base + (long)t * U1 + u - 1] : 0.f;
    }
  };
  fetch(0, eb, ey);
  const int D = Tb + Ub;                                 // diagonals 0 .. D - 1
  for (int d = 0; d < D; ++d) {
    if (d + 1 < D) fetch(d + 1, nb, ny);
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int u = threadIdx.x + 256 * k, t = d - u;
      if (u <= Ub && t >= 0 && t < Tb) {
        double a;
        if (d == 0) {
          a = 0.0;
        } else {
          const double a1 = t > 0 ? prev[u] + (double)eb[k] : TR_NEG_INF64;
          const double a2 = u > 0 ? prev[u - 1] + (double)ey[k] : TR_NEG_INF64;
          a = lae2(a1, a2);
        }
        cur[u] = a;
        alpha[base + (long)t * U1 + u] = a;
      }
    }
    __syncthreads();
    double* tmp = prev; prev = cur; cur = tmp;
#pragma unroll
    for (int k = 0; k < KS; ++k) { eb[k] = nb[k]; ey[k] = ny[k]; }
  }
  if (threadIdx.x == 0) {
    const double l = -(prev[Ub] + (double)lpb[base + (long)(Tb - 1) * U1 + Ub]);
    alpha[(long)gridDim.x * Tm * U1 + b] = l;
    nll[b] = (float)l;
  }
}

// beta(Tb-1,Ub) = lpb(Tb-1,Ub); beta(t,u) = lae(beta(t+1,u) + lpb(t,u), beta(t,u+1) + lpy(t,u)).  Per cell, with logP = -nll:
//   g_blank(t,u) = -gscale exp(alpha(t,u) + lpb(t,u) + beta(t+1,u) - logP)   (beta(Tb,Ub) = 0, nothing after (Tb-1, u < Ub))
//   g_y(t,u)     = -gscale exp(alpha(t,u) + lpy(t,u) + beta(t,u+1) - logP)   (u < Ub)
// and exactly 0 on every row outside t < Tb, u <= Ub.
template <int KS>
__global__ __launch_bounds__(256) void rnnt_beta_kernel(const float* __restrict__ lpb, const float* __restrict__ lpy,
                                                        const double* __restrict__ alpha,
                                                        const float* __restrict__ gscale, const int32_t* __restrict__ in_len,
                                                        const int32_t* __restrict__ tgt_len, int Tm, int U1,
                                                        float* __restrict__ gb, float* __restrict__ gy) {
  extern __shared__ double shd[];
  const int b = blockIdx.x;
  int Tb, Ub;
  utt_lengths(in_len, tgt_len, b, Tm, U1, Tb, Ub);
  const long base = (long)b * Tm * U1;
  for (int i = threadIdx.x; i < Tm * U1; i += 256) {
    const int t = i / U1, u = i - t * U1;
    if (t >= Tb || u > Ub) { gb[base + i] = 0.f; gy[base + i] = 0.f; }
  }
  const double nl = alpha[(long)gridDim.x * Tm * U1 + b];   // -log P in fp64 (rnnt_alpha_kernel)
  const float sc = gscale[b];
  const bool ok = nl < __builtin_inf() && nl == nl;
  double* nxt = shd;
  double* cur = shd + U1;
  float eb[KS], ey[KS], nb[KS], ny[KS];
  double ea[KS], na[KS];
  auto fetch = [&](int d, float (&fb)[KS], float (&fy)[KS], double (&fa)[KS]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int u = threadIdx.x + 256 * k, t = d - u;
      const bool in = u <= Ub && t >= 0 && t < Tb;
      const long r = base + (long)t * U1 + u;
      fb[k] = in ? lpb[r] : 0.f;
      fy[k] = (in && u < Ub) ? lpy[r] : 0.f;
      fa[k] = in ? alpha[r] : 0.0;
    }
  };
  const int D = Tb + Ub;
  fetch(D - 1, eb, ey, ea);
  for (int d = D - 1; d >= 0; --d) {
    if (d > 0) fetch(d - 1, nb, ny, na);
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int u = threadIdx.x + 256 * k, t = d - u;
      if (u <= Ub && t >= 0 && t < Tb) {
        const double bnext_t = t + 1 < Tb ? nxt[u] : (u == Ub ? 0.0 : TR_NEG_INF64);   // beta(t+1, u) (terminal after the last blank)
        const double bnext_u = u < Ub ? nxt[u + 1] : TR_NEG_INF64;                     // beta(t, u+1)
        const double vb = bnext_t == TR_NEG_INF64 ? TR_NEG_INF64 : (double)eb[k] + bnext_t;
        const double vy = bnext_u == TR_NEG_INF64 ? TR_NEG_INF64 : (double)ey[k] + bnext_u;
        cur[u] = lae2(vb, vy);
        const long r = base + (long)t * U1 + u;
        gb[r] = (ok && vb != TR_NEG_INF64) ? -sc * (float)exp(ea[k] + vb + nl) : 0.f;
        gy[r] = (ok && vy != TR_NEG_INF64) ? -sc * (float)exp(ea[k] + vy + nl) : 0.f;
      }
    }
    __syncthreads();
    double* tmp = nxt; nxt = cur; cur = tmp;
#pragma unroll
    for (int k = 0; k < KS; ++k) { eb[k] = nb[k]; ey[k] = ny[k]; ea[k] = na[k]; }
  }
}

// ---- drop-in logit gradient: dz_v = [v = blank] g_b + [v = y] g_y - softmax_v (g_b + g_y); one wave per row ----------------
template <typename T>
__global__ __launch_bounds__(256) void logit_grad_kernel(const T* __restrict__ Z, long ldz, const int32_t* __restrict__ targets,
                                                         const float* __restrict__ lse, const float* __restrict__ gb,
                                                         const float* __restrict__ gy, int rows, int Tm, int U1, int V, int blank,
                                                         T* __restrict__ G, long ldg) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= rows) return;
  const float b_ = gb[n], y_ = gy[n], l = lse[n], gs = b_ + y_;
  const int y = row_target(targets, n, Tm, U1);
  const T* z = Z + (long)n * ldz;
  T* g = G + (long)n * ldg;
  if (gs == 0.f && b_ == 0.f) {
    for (int c = lane; c < V; c += 64) g[c] = from_f32<T>(0.f);
    return;
  }
  for (int c = lane; c < V; c += 64) {
    float v = -expf(to_f32(z[c]) - l) * gs;
    if (c == blank) v += b_;
    if (c == y) v += y_;
    g[c] = from_f32<T>(v);
  }
}

// ---- fused GEMM tiles (head_tile.h): z = H W^T + bias, H's rows being the lattice rows n.  Rows >= N and columns >= V are
// clamped copies in the main loop: every use below is guarded by n < N / v < V, and blank and y are < V. ----
// forward: part[n][ct] = (max, sum exp) of row n over the valid columns of column tile ct; zb[n] / zy[n] from the tile holding
// them.  No logit leaves the registers.
template <typename T>
__global__ __launch_bounds__(256, 2) void tj_stats_kernel(const T* __restrict__ H, const T* __restrict__ W, const float* __restrict__ bias,
                                                          const int32_t* __restrict__ targets, int N, int Tm, int U1, int J, int V,
                                                          int blank, int nct, float2* __restrict__ part, float* __restrict__ zb,
                                                          float* __restrict__ zy) {
  __shared__ __attribute__((aligned(16))) char smem[2 * HeadTile<T>::OP_BYTES];
  __shared__ float sbias[HEAD_TILE];
  __shared__ LseStat red[HEAD_TILE];
  const int ct = blockIdx.x % nct, rt = blockIdx.x / nct;
  const int n0 = rt * HEAD_TILE, v0 = ct * HEAD_TILE;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wv = wave & 1, wn = wave >> 1, l31 = lane & 31, hi = lane >> 5;
  if (t < HEAD_TILE) sbias[t] = (bias && v0 + t < V) ? bias[v0 + t] : 0.f;
  f32x16 acc[2][2];
  head_mainloop<T>(H, J, W, N, V, J, n0, v0, smem, acc);  // (its barriers publish sbias)
  auto thread_stat = [&](int j) __attribute__((always_inline)) -> LseStat {
    const int n = n0 + wn * 64 + j * 32 + l31;
    const int y = n < N ? row_target(targets, n, Tm, U1) : -1;
    float mx = NEG_INF;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int vl = head_col(wv, i, r, hi), v = v0 + vl;
        const float z = acc[i][j][r] + sbias[vl];
        acc[i][j][r] = z;
        if (v < V) mx = fmaxf(mx, z);
        if (n < N && v == blank) zb[n] = z;
        if (n < N && v == y) zy[n] = z;
      }
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (v0 + head_col(wv, i, r, hi) < V) sm += expf(acc[i][j][r] - mx);
    return {mx, sm};
  };
  head_row_meet(red, thread_stat, [&](int nl, const LseStat& r) {
    if (n0 + nl < N) part[(long)(n0 + nl) * nct + ct] = make_float2(r.m, r.s);
  });
}

// lse[n] from the partials in column-tile order; lpb = zb - lse, lpy = zy - lse (0 where the row has no label)
__global__ __launch_bounds__(256) void tj_combine_kernel(const float2* __restrict__ part, int nct, const float* __restrict__ zb,
                                                         const float* __restrict__ zy, const int32_t* __restrict__ targets, int N,
                                                         int Tm, int U1, int V, float* __restrict__ lse, float* __restrict__ lpb,
                                                         float* __restrict__ lpy) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float M = NEG_INF;
  for (int c = 0; c < nct; ++c) M = fmaxf(M, part[(long)n * nct + c].x);
  float S = 0.f;
  for (int c = 0; c < nct; ++c) {
    const float2 p = part[(long)n * nct + c];
    if (p.x != NEG_INF) S += p.y * expf(p.x - M);        // (not lse_rescale: the guarded add contracts to one fma, and that is in the bits)
  }
  const float l = M + logf(S);
  const int y = row_target(targets, n, Tm, U1);
  lse[n] = l;
  lpb[n] = zb[n] - l;
  lpy[n] = (y >= 0 && y < V) ? zy[n] - l : 0.f;
}

// backward: the tile recomputed, dz = [v = blank] g_b + [v = y] g_y - exp(z - lse) (g_b + g_y) stored once in T (4 consecutive
// columns per store; V % 4 == 0).  Rows [row0, row0 + N) of the lattice; dz row n - row0 (leading dimension lddz).  Tiles with no gradient-carrying row
// store zeros and skip the main loop.
template <typename T>
__global__ __launch_bounds__(256, 2) void tj_grad_kernel(const T* __restrict__ H, const T* __restrict__ W, const float* __restrict__ bias,
                                                         const int32_t* __restrict__ targets, const float* __restrict__ lse,
                                                         const float* __restrict__ gb, const float* __restrict__ gy, int row0, int N,
                                                         int Tm, int U1, int J, int V, int blank, int nct, T* __restrict__ dz,
                                                         long lddz) {
  __shared__ __attribute__((aligned(16))) char smem[2 * HeadTile<T>::OP_BYTES];
  __shared__ float sbias[HEAD_TILE];
  const int ct = blockIdx.x % nct, rt = blockIdx.x / nct;
  const int n0 = rt * HEAD_TILE, v0 = ct * HEAD_TILE;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wv = wave & 1, wn = wave >> 1, l31 = lane & 31, hi = lane >> 5;
  int live = 0;
  if (t < HEAD_TILE) {
    sbias[t] = (bias && v0 + t < V) ? bias[v0 + t] : 0.f;
    const int n = n0 + t;
    live = n < N && (gb[row0 + n] != 0.f || gy[row0 + n] != 0.f);
  }
  if (!__syncthreads_or(live)) {
    for (int i = t; i < HEAD_TILE * (HEAD_TILE / 4); i += 256) {
      const int r = i / (HEAD_TILE / 4), v = v0 + (i % (HEAD_TILE / 4)) * 4, n = n0 + r;
      if (n < N && v < V) {
        const float zz[4] = {0.f, 0.f, 0.f, 0.f};
        store4(dz + (long)n * lddz + v, zz);
      }
    }
    return;
  }
  f32x16 acc[2][2];
  head_mainloop<T>(H + (long)row0 * J, J, W, N, V, J, n0, v0, smem, acc);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn * 64 + j * 32 + l31;
    if (n >= N) continue;
    const int y = row_target(targets, row0 + n, Tm, U1);
    const float l = lse[row0 + n], b_ = gb[row0 + n], y_ = gy[row0 + n], gs = b_ + y_;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int vl = head_col(wv, i, 4 * q, hi), v = v0 + vl;
        if (v >= V) continue;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float z = acc[i][j][4 * q + e] + sbias[vl + e];
          float g = -expf(z - l) * gs;
          if (v + e == blank) g += b_;
          if (v + e == y) g += y_;
          o[e] = g;
        }
        store4(dz + (long)n * lddz + v, o);
      }
  }
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

#define TR_ACT_DISPATCH(act, CALL)                               \
  switch (act) {                                                 \
    case SMX_ACT_GELU: CALL(SMX_ACT_GELU); break;                \
    case SMX_ACT_LEAKY_RELU: CALL(SMX_ACT_LEAKY_RELU); break;    \
    case SMX_ACT_RELU: CALL(SMX_ACT_RELU); break;                \
    case SMX_ACT_SWISH: CALL(SMX_ACT_SWISH); break;              \
    default: CALL(SMX_ACT_NONE); break;                          \
  }

static int joint_ntb(int T) { return (T + JOINT_TB - 1) / JOINT_TB; }

extern "C" int smx_transducer_joint_fwd(int dtype, const void* enc, const void* dec, void* H, int B, int T, int U1, int J, int act,
                                        void* stream) {
  SMX_REQUIRE(enc && dec && H, "smx_transducer_joint_fwd: null pointer");
  SMX_REQUIRE(B >= 0 && T > 0 && U1 > 0 && J > 0 && J % 4 == 0, "smx_transducer_joint_fwd: bad sizes (J %% 4 == 0)");
  SMX_REQUIRE(aligned16(enc) && aligned16(dec) && aligned16(H), "smx_transducer_joint_fwd: 16-byte aligned tensors");
  if (B == 0) return SMX_OK;
#define JF(A_) do { if (dtype == SMX_BF16) hipLaunchKernelGGL((joint_fwd_kernel<bf16_t, A_>), dim3(B * T), dim3(256), 0, STREAM, (const bf16_t*)enc, (const bf16_t*)dec, (bf16_t*)H, T, U1, J); \
                    else hipLaunchKernelGGL((joint_fwd_kernel<float, A_>), dim3(B * T), dim3(256), 0, STREAM, (const float*)enc, (const float*)dec, (float*)H, T, U1, J); } while (0)
  TR_ACT_DISPATCH(act, JF)
#undef JF
  return check_launch("smx_transducer_joint_fwd");
}

extern "C" size_t smx_transducer_joint_bwd_workspace(int B, int T, int U1, int J) {
  return (size_t)(B > 0 ? B : 1) * joint_ntb(T > 0 ? T : 1) * (U1 > 0 ? U1 : 1) * (J > 0 ? J : 1) * sizeof(float);
}

extern "C" int smx_transducer_joint_bwd(int dtype, const void* dH, const void* enc, const void* dec, void* d_enc, void* d_dec, int B,
                                        int T, int U1, int J, int act, void* workspace, void* stream) {
  SMX_REQUIRE(dH && enc && dec && d_enc && d_dec && workspace, "smx_transducer_joint_bwd: null pointer");
  SMX_REQUIRE(B >= 0 && T > 0 && U1 > 0 && J > 0 && J % 4 == 0, "smx_transducer_joint_bwd: bad sizes (J %% 4 == 0)");
  SMX_REQUIRE(aligned16(dH) && aligned16(enc) && aligned16(dec) && aligned16(d_enc) && aligned16(d_dec) && aligned16(workspace),
              "smx_transducer_joint_bwd: 16-byte aligned tensors");
  if (B == 0) return SMX_OK;
  const int NTB = joint_ntb(T);
  float* P = reinterpret_cast<float*>(workspace);
#define JB(A_) do { if (dtype == SMX_BF16) { \
      hipLaunchKernelGGL((joint_bwd_enc_kernel<bf16_t, A_>), dim3(B * T), dim3(256), 0, STREAM, (const bf16_t*)dH, (const bf16_t*)enc, (const bf16_t*)dec, (bf16_t*)d_enc, T, U1, J); \
      hipLaunchKernelGGL((joint_bwd_dec_partial_kernel<bf16_t, A_>), dim3(B * NTB * U1), dim3(256), 0, STREAM, (const bf16_t*)dH, (const bf16_t*)enc, (const bf16_t*)dec, P, T, U1, J, NTB); \
    } else { \
      hipLaunchKernelGGL((joint_bwd_enc_kernel<float, A_>), dim3(B * T), dim3(256), 0, STREAM, (const float*)dH, (const float*)enc, (const float*)dec, (float*)d_enc, T, U1, J); \
      hipLaunchKernelGGL((joint_bwd_dec_partial_kernel<float, A_>), dim3(B * NTB * U1), dim3(256), 0, STREAM, (const float*)dH, (const float*)enc, (const float*)dec, P, T, U1, J, NTB); \
    } } while (0)
  TR_ACT_DISPATCH(act, JB)
#undef JB
  if (dtype == SMX_BF16) hipLaunchKernelGGL((joint_bwd_dec_sum_kernel<bf16_t>), dim3(B * U1), dim3(256), 0, STREAM, P, (bf16_t*)d_dec, U1, J, NTB);
  else hipLaunchKernelGGL((joint_bwd_dec_sum_kernel<float>), dim3(B * U1), dim3(256), 0, STREAM, P, (float*)d_dec, U1, J, NTB);
  return check_launch("smx_transducer_joint_bwd");
}

extern "C" int smx_transducer_row_stats(int dtype, const void* logits, int64_t ld, const int32_t* targets, int B, int T, int U1, int V,
                                        int blank, float* lse, float* lpb, float* lpy, void* stream) {
  SMX_REQUIRE(logits && lse && lpb && lpy && (targets || U1 == 1), "smx_transducer_row_stats: null pointer");
  SMX_REQUIRE(B >= 0 && T > 0 && U1 > 0 && V > 0 && ld >= V && blank >= 0 && blank < V, "smx_transducer_row_stats: bad sizes");
  const long rows = (long)B * T * U1;
  SMX_REQUIRE(rows < (1L << 31), "smx_transducer_row_stats: too many lattice rows");
  if (rows == 0) return SMX_OK;
  dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == SMX_BF16) hipLaunchKernelGGL((row_stats_kernel<bf16_t>), grid, dim3(256), 0, STREAM, (const bf16_t*)logits, ld, targets, (int)rows, T, U1, V, blank, lse, lpb, lpy);
  else hipLaunchKernelGGL((row_stats_kernel<float>), grid, dim3(256), 0, STREAM, (const float*)logits, ld, targets, (int)rows, T, U1, V, blank, lse, lpb, lpy);
  return check_launch("smx_transducer_row_stats");
}

static int rnnt_ks(int U1) { return U1 <= 256 ? 1 : U1 <= 512 ? 2 : U1 <= 1024 ? 4 : 8; }

extern "C" int smx_transducer_loss_fwd(const float* lpb, const float* lpy, const int32_t* in_len, const int32_t* tgt_len, int B, int T,
                                       int U1, double* alpha, float* nll, void* stream) {
  SMX_REQUIRE(lpb && lpy && in_len && tgt_len && alpha && nll, "smx_transducer_loss_fwd: null pointer");
  SMX_REQUIRE(B >= 0 && T > 0 && U1 > 0 && U1 <= 2048, "smx_transducer_loss_fwd: bad sizes (U + 1 <= 2048)");
  if (B == 0) return SMX_OK;
  const size_t shm = 2 * (size_t)U1 * sizeof(double);
#define RA(KS_) hipLaunchKernelGGL((rnnt_alpha_kernel<KS_>), dim3(B), dim3(256), shm, STREAM, lpb, lpy, in_len, tgt_len, T, U1, alpha, nll)
  switch (rnnt_ks(U1)) { case 1: RA(1); break; case 2: RA(2); break; case 4: RA(4); break; default: RA(8); break; }
#undef RA
  return check_launch("smx_transducer_loss_fwd");
}

extern "C" int smx_transducer_loss_bwd(const float* lpb, const float* lpy, const double* alpha, const float* gscale,
                                       const int32_t* in_len, const int32_t* tgt_len, int B, int T, int U1, float* gb, float* gy,
                                       void* stream) {
  SMX_REQUIRE(lpb && lpy && alpha && gscale && in_len && tgt_len && gb && gy, "smx_transducer_loss_bwd: null pointer");
  SMX_REQUIRE(B >= 0 && T > 0 && U1 > 0 && U1 <= 2048, "smx_transducer_loss_bwd: bad sizes (U + 1 <= 2048)");
  if (B == 0) return SMX_OK;
  const size_t shm = 2 * (size_t)U1 * sizeof(double);
#define RB(KS_) hipLaunchKernelGGL((rnnt_beta_kernel<KS_>), dim3(B), dim3(256), shm, STREAM, lpb, lpy, alpha, gscale, in_len, tgt_len, T, U1, gb, gy)
  switch (rnnt_ks(U1)) { case 1: RB(1); break; case 2: RB(2); break; case 4: RB(4); break; default: RB(8); break; }
#undef RB
  return check_launch("smx_transducer_loss_bwd");
}

extern "C" int smx_transducer_logit_grad(int dtype, const void* logits, int64_t ld, const int32_t* targets, const float* lse,
                                         const float* gb, const float* gy, int B, int T, int U1, int V, int blank, void* dz,
                                         int64_t lddz, void* stream) {
  SMX_REQUIRE(logits && lse && gb && gy && dz && (targets || U1 == 1), "smx_transducer_logit_grad: null pointer");
  SMX_REQUIRE(B >= 0 && T > 0 && U1 > 0 && V > 0 && ld >= V && lddz >= V && blank >= 0 && blank < V, "smx_transducer_logit_grad: bad sizes");
  const long rows = (long)B * T * U1;
  SMX_REQUIRE(rows < (1L << 31), "smx_transducer_logit_grad: too many lattice rows");
  if (rows == 0) return SMX_OK;
  dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == SMX_BF16) hipLaunchKernelGGL((logit_grad_kernel<bf16_t>), grid, dim3(256), 0, STREAM, (const bf16_t*)logits, ld, targets, lse, gb, gy, (int)rows, T, U1, V, blank, (bf16_t*)dz, lddz);
  else hipLaunchKernelGGL((logit_grad_kernel<float>), grid, dim3(256), 0, STREAM, (const float*)logits, ld, targets, lse, gb, gy, (int)rows, T, U1, V, blank, (float*)dz, lddz);
  return check_launch("smx_transducer_logit_grad");
}

extern "C" int smx_transducer_fused_ok(int dtype, int J, int V) {
  return (dtype == SMX_BF16 || dtype == SMX_F32) && J > 0 && J % 64 == 0 && V > 0 && V % 4 == 0;
}

static int tj_nct(int V) { return (V + HEAD_TILE - 1) / HEAD_TILE; }

extern "C" size_t smx_transducer_stats_workspace(int rows, int V) {
  // [partials (rows, nct) float2][z_blank (rows)][z_y (rows)]
  const size_t r = rows > 0 ? rows : 1;
  return r * tj_nct(V > 0 ? V : 1) * sizeof(float2) + 2 * r * sizeof(float);
}

extern "C" int smx_transducer_gemm_stats(int dtype, const void* H, const void* W, const float* bias, const int32_t* targets, int B, int T,
                                         int U1, int J, int V, int blank, float* lse, float* lpb, float* lpy, void* workspace,
                                         void* stream) {
  SMX_REQUIRE(H && W && lse && lpb && lpy && workspace && (targets || U1 == 1), "smx_transducer_gemm_stats: null pointer");
  SMX_REQUIRE(B >= 0 && T > 0 && U1 > 0 && blank >= 0 && blank < V, "smx_transducer_gemm_stats: bad sizes");
  if (!smx_transducer_fused_ok(dtype, J, V)) return fail(SMX_EUNSUPPORTED, "smx_transducer_gemm_stats: J %% 64 == 0 and V %% 4 == 0 required (J %d, V %d)", J, V);
  SMX_REQUIRE(aligned16(H) && aligned16(W) && aligned16(workspace), "smx_transducer_gemm_stats: 16-byte aligned tensors");
  const long rows = (long)B * T * U1;
  SMX_REQUIRE(rows < (1L << 31) / 2, "smx_transducer_gemm_stats: too many lattice rows");
  if (rows == 0) return SMX_OK;
  const int nct = tj_nct(V), nrt = (int)((rows + HEAD_TILE - 1) / HEAD_TILE);
  float2* part = reinterpret_cast<float2*>(workspace);
  float* zb = reinterpret_cast<float*>(part + rows * nct);
  float* zy = zb + rows;
  const dim3 grid((unsigned)((long)nrt * nct));
  if (dtype == SMX_BF16) hipLaunchKernelGGL((tj_stats_kernel<bf16_t>), grid, dim3(256), 0, STREAM, (const bf16_t*)H, (const bf16_t*)W, bias, targets, (int)rows, T, U1, J, V, blank, nct, part, zb, zy);
  else hipLaunchKernelGGL((tj_stats_kernel<float>), grid, dim3(256), 0, STREAM, (const float*)H, (const float*)W, bias, targets, (int)rows, T, U1, J, V, blank, nct, part, zb, zy);
  hipLaunchKernelGGL(tj_combine_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, STREAM, part, nct, zb, zy, targets, (int)rows, T, U1, V, lse, lpb, lpy);
  return check_launch("smx_transducer_gemm_stats");
}

extern "C" int smx_transducer_gemm_grad(int dtype, const void* H, const void* W, const float* bias, const int32_t* targets,
                                        const float* lse, const float* gb, const float* gy, int B, int T, int U1, int J, int V, int blank,
                                        int row0, int nrows, void* dz, int64_t lddz, void* stream) {
  SMX_REQUIRE(H && W && lse && gb && gy && dz && (targets || U1 == 1), "smx_transducer_gemm_grad: null pointer");
  SMX_REQUIRE(B >= 0 && T > 0 && U1 > 0 && blank >= 0 && blank < V, "smx_transducer_gemm_grad: bad sizes");
  if (!smx_transducer_fused_ok(dtype, J, V)) return fail(SMX_EUNSUPPORTED, "smx_transducer_gemm_grad: J %% 64 == 0 and V %% 4 == 0 required (J %d, V %d)", J, V);
  SMX_REQUIRE(aligned16(H) && aligned16(W) && aligned8(dz) && lddz >= V && lddz % 4 == 0, "smx_transducer_gemm_grad: aligned tensors");
  const long rows = (long)B * T * U1;
  SMX_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + (long)nrows <= rows, "smx_transducer_gemm_grad: row range [%d, %d + %d) outside the lattice", row0, row0, nrows);
  if (nrows == 0) return SMX_OK;
  const int nct = tj_nct(V), nrt = (nrows + HEAD_TILE - 1) / HEAD_TILE;
  const dim3 grid((unsigned)((long)nrt * nct));
  if (dtype == SMX_BF16) hipLaunchKernelGGL((tj_grad_kernel<bf16_t>), grid, dim3(256), 0, STREAM, (const bf16_t*)H, (const bf16_t*)W, bias, targets, lse, gb, gy, row0, nrows, T, U1, J, V, blank, nct, (bf16_t*)dz, lddz);
  else hipLaunchKernelGGL((tj_grad_kernel<float>), grid, dim3(256), 0, STREAM, (const float*)H, (const float*)W, bias, targets, lse, gb, gy, row0, nrows, T, U1, J, V, blank, nct, (float*)dz, lddz);
  return check_launch("smx_transducer_gemm_grad");
}
