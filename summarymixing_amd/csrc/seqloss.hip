// seqloss.hip — the recipes' second loss head, gfx950 only: the label-smoothed sequence losses over (B, U, V) and the accuracy
//   speechbrain.nnet.losses.kldiv_loss  (recipe key `seq_cost`, …/LibriSpeech/ASR/transformer/hparams/branchformer_summarymixing.yaml:278-280)
//   speechbrain.nnet.losses.nll_loss    (recipe key `ce_cost`,  …/LibriSpeech/ASR/transducer/hparams/conformer_summarymixing_transducer.yaml:319-320)
//   speechbrain.utils.Accuracy          (recipe key `acc_computer`)
// One target distribution serves both losses: q[v] = off for v != y, q[y] = conf, and the row loss is
//   cst - conf lp[y] - off (sum_v lp[v] - lp[y]).
// Forward: one wave per row, ONE read of the row.  From raw logits the same read carries an online (max, sum exp) pair, the sum of
// the logits and the argmax: lse = m + log s, lp[v] = z[v] - lse, sum lp = sum z - V lse; no log-probability is stored.  A second,
// tiny launch (one wave per utterance) folds the rows of an utterance in a fixed order: no float atomics, two runs agree bit for
// bit.  Backward: one wave per row, one read (logits form) and one write; dropped rows are written as zeros and never read.
#include "row_scan.h"

namespace smx {

enum { SL_KEEP = 1, SL_HIT = 2 };

// what one lane has seen of its row: the online softmax pair, the plain sum (fp64: at V = 5000 and logits near 80 an fp32 sum
// resolves 0.03, and sum z - V lse cancels to a few units) and the running argmax (first index among equals)
struct RowAcc {
  float m, s;
  double sum;
  float bv;
  int bi;
};

template <bool LOGITS, bool SUM, int N>
__device__ __forceinline__ void row_take(RowAcc& a, const float (&x)[N], int c0) {
  float gm = x[0];
  int gi = 0;
#pragma unroll
  for (int j = 1; j < N; ++j)
    if (x[j] > gm) { gm = x[j]; gi = j; }                // strict: the first of equal entries stays
  argmax_take(a.bv, a.bi, gm, c0 + gi);
  if constexpr (LOGITS) {
    if (gm > a.m) {                                      // one rescale per group; a.s is 0 while a.m is -inf
      a.s = lse_rescale(a.s, a.m, gm);
      a.m = gm;
    }
    if (a.m != NEG_INF) {
#pragma unroll
      for (int j = 0; j < N; ++j) a.s += expf(x[j] - a.m);
    }
  }
  if constexpr (SUM) {
#pragma unroll
    for (int j = 0; j < N; ++j) a.sum += (double)x[j];
  }
}

__device__ __forceinline__ bool sl_keep(const int* __restrict__ len, int b, int u, int y, int pad_idx) {
  return (len == nullptr || u < len[b]) && (pad_idx < 0 || y != pad_idx);
}

// grid = ceil(B U / 4), block = 256: wave w of a block owns row 4 blockIdx.x + w and reads it once (row_scan).
template <typename T, bool LOGITS, bool SUM>
__global__ __launch_bounds__(256) void seqloss_fwd_kernel(const T* __restrict__ X, long ldx, long bsx, const int* __restrict__ tgt,
                                                          long ldt, const int* __restrict__ len, int B, int U, int V, int pad_idx,
                                                          float conf, float off, float cst, float* __restrict__ row_loss,
                                                          float* __restrict__ lse, int* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * U) return;
  const int b = (int)(row / U), u = (int)(row % U);
  const int y = tgt[(long)b * ldt + u];
  if (!sl_keep(len, b, u, y, pad_idx)) {                 // a dropped row is never read
    if (lane == 0) {
      row_loss[row] = 0.f;
      flags[row] = 0;
      if (LOGITS) { lse[2 * row] = 0.f; lse[2 * row + 1] = 0.f; }
    }
    return;
  }
  const T* x = X + (long)b * bsx + (long)u * ldx;
  RowAcc a = {NEG_INF, 0.f, 0.0, NEG_INF, 0x7fffffff};
  row_scan(x, V, lane, [&](const auto& g, int c0) { row_take<LOGITS, SUM>(a, g, c0); });
  // across the wave (butterflies: every lane ends with the same bits)
  float bv = a.bv;
  int bi = a.bi;
  argmax_meet<64>(bv, bi);
  double L = 0.0;                                        // log sum exp of the row (logits form)
  if constexpr (LOGITS) {
    const float m = wave_max(a.m);
    const float s = wave_sum(lse_rescale(a.s, a.m, m));
    L = (double)m + (double)logf(s);
  }
  double sum = 0.0;
  if constexpr (SUM) sum = wave_sum_f64(a.sum);
  if (lane != 0) return;
  // The final combination in fp64, rounded once: the library is built with -ffast-math, which reassociates an fp32
  // (z - m) - log s back into z - (m + log s) (see log_softmax_fwd_kernel in ctc.hip), and with logits near 80 that sum has lost
  // what the loss is made of.
  float loss;
  if (y < 0 || y >= V) {
    loss = __builtin_nanf("");                           // an out-of-range target on a kept row: visible, and never an index
  } else {
    const double zy = (double)to_f32(x[y]);
    const double lpy = LOGITS ? zy - L : zy;
    double r = (double)cst - (double)conf * lpy;
    if constexpr (SUM) r -= (double)off * ((LOGITS ? sum - (double)V * L : sum) - lpy);   // off == 0: the row sum never enters
    loss = (float)r;
  }
  row_loss[row] = loss;
  flags[row] = SL_KEEP | (bi == y ? SL_HIT : 0);
  if constexpr (LOGITS) {
    const float hi = (float)L;
    lse[2 * row] = hi;
    lse[2 * row + 1] = (float)(L - (double)hi);          // the fp32 value and what its rounding dropped: the backward's exp(z - lse)
  }
}

// grid = B, block = 64: utterance sums over the kept rows, lane-strided partials in increasing u, then one butterfly
__global__ __launch_bounds__(64) void seqloss_utt_kernel(const float* __restrict__ row_loss, const int* __restrict__ flags, int U,
                                                         float* __restrict__ utt_loss, int* __restrict__ utt_kept,
                                                         int* __restrict__ utt_hits) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  int k = 0, h = 0;
  for (int u = lane; u < U; u += 64) {
    const int f = flags[(long)b * U + u];
    if (f & SL_KEEP) {
      s += (double)row_loss[(long)b * U + u];
      k += 1;
      h += (f & SL_HIT) ? 1 : 0;
    }
  }
  s = wave_sum_f64(s);
  k = wave_sum_i32(k);
  h = wave_sum_i32(h);
  if (lane == 0) {
    utt_loss[b] = (float)s;
    utt_kept[b] = k;
    if (utt_hits) utt_hits[b] = h;
  }
}

// dX of one row.  log-probability form: -g q (X is not read); logits form: g (exp(z - lse) - q).  Dropped rows: zeros.
template <typename T, bool LOGITS>
__global__ __launch_bounds__(256) void seqloss_bwd_kernel(const T* __restrict__ X, long ldx, long bsx, const int* __restrict__ tgt,
                                                          long ldt, const int* __restrict__ len, int B, int U, int V, int pad_idx,
                                                          float conf, float off, const float* __restrict__ lse,
                                                          const float* __restrict__ g, T* __restrict__ dX, long lddx) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * U) return;
  const int b = (int)(row / U), u = (int)(row % U);
  const int y = tgt[(long)b * ldt + u];
  const bool keep = sl_keep(len, b, u, y, pad_idx);
  const bool bad = keep && (y < 0 || y >= V);
  T* dx = dX + row * lddx;
  const T* x = X + (long)b * bsx + (long)u * ldx;
  constexpr int N = Grp16<T>::N;
  const int Vv = V - V % N;
  const bool read = LOGITS && keep && !bad;
  const bool vec_x = (reinterpret_cast<uintptr_t>(x) & 15u) == 0, vec_d = (reinterpret_cast<uintptr_t>(dx) & 15u) == 0;
  const float gr = keep ? g[row] : 0.f;
  const double L = (LOGITS && keep) ? (double)lse[2 * row] + (double)lse[2 * row + 1] : 0.0;
  const float nan = __builtin_nanf("");
  auto entry = [&](float z, int c) -> float {
    if (!keep) return 0.f;
    if (bad) return nan;
    const float q = c == y ? conf : off;
    if constexpr (LOGITS) return gr * (expf((float)((double)z - L)) - q);    // fp64 difference: see the forward's note
    else return -(gr * q);
  };
  for (int c0 = lane * N; c0 < Vv; c0 += 64 * N * ROW_DEPTH) {
    float f[ROW_DEPTH][N];
#pragma unroll
    for (int d = 0; d < ROW_DEPTH; ++d) {
      const int c = c0 + d * 64 * N;
      if (c < Vv) {
        if (read && vec_x) Grp16<T>::load(x + c, f[d]);
        else {
#pragma unroll
          for (int j = 0; j < N; ++j) f[d][j] = read ? to_f32(x[c + j]) : 0.f;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < ROW_DEPTH; ++d) {
      const int c = c0 + d * 64 * N;
      if (c < Vv) {
#pragma unroll
        for (int j = 0; j < N; ++j) f[d][j] = entry(f[d][j], c + j);
        if (vec_d) Grp16<T>::store(dx + c, f[d]);
        else {
#pragma unroll
          for (int j = 0; j < N; ++j) dx[c + j] = from_f32<T>(f[d][j]);
        }
      }
    }
  }
  for (int c = Vv + lane; c < V; c += 64) {
    const float z = read ? to_f32(x[c]) : 0.f;
    dx[c] = from_f32<T>(entry(z, c));
  }
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_seqloss_fwd(int dtype, int from_logits, const void* X, int64_t ldx, int64_t bsx, const int32_t* targets,
                               int64_t ldt, const int32_t* len, int B, int U, int V, int pad_idx, float conf, float off, float cst,
                               float* row_loss, float* lse, int32_t* row_flags, float* utt_loss, int32_t* utt_kept,
                               int32_t* utt_hits, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_seqloss_fwd: dtype %d", dtype);
  SMX_REQUIRE(X && targets && row_loss && row_flags && utt_loss && utt_kept, "smx_seqloss_fwd: null pointer");
  SMX_REQUIRE(!from_logits || lse, "smx_seqloss_fwd: the logits form needs lse");
  SMX_REQUIRE(B >= 0 && U >= 0 && V > 0 && ldx >= V && ldt >= U && bsx >= 0, "smx_seqloss_fwd: bad sizes");
  SMX_REQUIRE(conf == conf && off == off && cst == cst && off >= 0.f, "smx_seqloss_fwd: conf, off, cst must be numbers and off >= 0");
  if ((int64_t)B * U >= (int64_t)1 << 31 || pad_idx >= V) return fail(SMX_EUNSUPPORTED, "smx_seqloss_fwd: B U = %lld rows, pad_idx %d of %d", (long long)B * U, pad_idx, V);
  if (B == 0 || U == 0) {
    if (B > 0) hipLaunchKernelGGL(seqloss_utt_kernel, dim3(B), dim3(64), 0, STREAM, row_loss, row_flags, 0, utt_loss, utt_kept, utt_hits);
    return check_launch("smx_seqloss_fwd");
  }
  const dim3 grid((unsigned)(((int64_t)B * U + 3) / 4));
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
#define SL_FWD(LG, SM) hipLaunchKernelGGL((seqloss_fwd_kernel<T, LG, SM>), grid, dim3(256), 0, STREAM, (const T*)X, (long)ldx, (long)bsx, targets, (long)ldt, len, B, U, V, pad_idx, conf, off, cst, row_loss, lse, row_flags)
    if (from_logits) { if (off != 0.f) SL_FWD(true, true); else SL_FWD(true, false); }
    else { if (off != 0.f) SL_FWD(false, true); else SL_FWD(false, false); }
#undef SL_FWD
  });
  hipLaunchKernelGGL(seqloss_utt_kernel, dim3(B), dim3(64), 0, STREAM, row_loss, row_flags, U, utt_loss, utt_kept, utt_hits);
  return check_launch("smx_seqloss_fwd");
}

extern "C" int smx_seqloss_bwd(int dtype, int from_logits, const void* X, int64_t ldx, int64_t bsx, const int32_t* targets,
                               int64_t ldt, const int32_t* len, int B, int U, int V, int pad_idx, float conf, float off,
                               const float* lse, const float* g, void* dX, int64_t lddx, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_seqloss_bwd: dtype %d", dtype);
  SMX_REQUIRE(targets && g && dX, "smx_seqloss_bwd: null pointer");
  SMX_REQUIRE(!from_logits || (X && lse), "smx_seqloss_bwd: the logits form needs X and lse");
  SMX_REQUIRE(B >= 0 && U >= 0 && V > 0 && lddx >= V && ldt >= U && (!from_logits || (ldx >= V && bsx >= 0)), "smx_seqloss_bwd: bad sizes");
  SMX_REQUIRE(conf == conf && off == off && off >= 0.f, "smx_seqloss_bwd: conf, off must be numbers and off >= 0");
  if ((int64_t)B * U >= (int64_t)1 << 31 || pad_idx >= V) return fail(SMX_EUNSUPPORTED, "smx_seqloss_bwd: B U = %lld rows, pad_idx %d of %d", (long long)B * U, pad_idx, V);
  if (X == dX) return fail(SMX_EUNSUPPORTED, "smx_seqloss_bwd: in place");
  if (B == 0 || U == 0) return SMX_OK;
  const dim3 grid((unsigned)(((int64_t)B * U + 3) / 4));
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (from_logits) hipLaunchKernelGGL((seqloss_bwd_kernel<T, true>), grid, dim3(256), 0, STREAM, (const T*)X, (long)ldx, (long)bsx, targets, (long)ldt, len, B, U, V, pad_idx, conf, off, lse, g, (T*)dX, (long)lddx);
    else hipLaunchKernelGGL((seqloss_bwd_kernel<T, false>), grid, dim3(256), 0, STREAM, (const T*)nullptr, 0L, 0L, targets, (long)ldt, len, B, U, V, pad_idx, conf, off, lse, g, (T*)dX, (long)lddx);
  });
  return check_launch("smx_seqloss_bwd");
}
