// lm_score.hip - the language model's share of the beam search's scorer hook (include/smx.h: smx_lm_score), gfx950 only.  DESIGN.md
// I.24 holds the definition.  R = B W hypothesis rows; the LM's logits z (R, V) of the step become
//   lmlp[r, v] = (z - max z) inv_temp - log sum exp((z - max z) inv_temp),   extra[r, v] (+)= weight lmlp[r, v]
// in front of smx_s2s_beam_select(extra), behind smx_ctc_prefix_score when there is one (accumulate).  One wave per row, two passes:
// the first is the selection's own reading of a row (row_scan.h: SelRow - fp32 expf of the fp64 exponent, fp32 per-lane sums, the
// lanes and the final expression in fp64), the second walks the same groups again (from L2) and writes extra in 16-byte groups where
// the row of extra is 16-byte aligned, element by element otherwise: a column's value depends on neither path.  No atomics, no LDS,
// nothing allocates or synchronises: capturable, and two runs agree bit for bit.
#include "row_scan.h"

namespace smx {

// N columns of extra at e: lp[j] = weight * lmlp, or -inf for a row that scores nothing.  The product and the sum are single
// roundings (no contraction), so the 16-byte path and the element path give the same bits.
template <int N, bool ACC>
__device__ __forceinline__ void lm_put(float* e, bool evec, const float (&lp)[N]) {
  if constexpr (N % 4 == 0) {
    if (evec) {
#pragma unroll
      for (int q = 0; q < N; q += 4) {
        float o[4] = {lp[q], lp[q + 1], lp[q + 2], lp[q + 3]};
        if (ACC) {
          float old[4];
          load4<float>(e + q, old);
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(old[j], o[j]);
        }
        store4<float>(e + q, o);
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) e[j] = ACC ? __fadd_rn(e[j], lp[j]) : lp[j];
}

// grid = R, block = 64
template <typename T, bool ACC>
__global__ __launch_bounds__(64) void lm_score_kernel(smx_lm_score_args a) {
  const int lane = threadIdx.x;
  const long r = blockIdx.x;
  const int b = (int)(r / a.W);
  const int n = a.n_tok[b];
  const int V = a.V;
  float* out = a.extra + r * a.lde;
  const bool live = !a.done[b] && a.score[r] > NEG_INF && n >= 0 && n < a.cap;      // (the same in every lane)
  if (!live && ACC) return;                                  // the CTC kernel wrote -inf under the same conditions
  const T* z = (const T*)a.logits + r * a.ldz;
  const double inv_temp = a.inv_temp;
  float m = NEG_INF;
  double ls = 0.0;
  bool bad = !live;
  if (live) {                                                // the selection's reading of the row: its max and log-sum-exp
    SelRow s0 = {NEG_INF, INT_MAX, NEG_INF, 0.f, 0};
    row_scan(z, V, lane, [&](const auto& g, int c0) { sel_row_take(s0, g, c0, -1, inv_temp); });
    int nan = s0.nan;
    m = wave_max(s0.m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nan |= __shfl_xor(nan, o, 64);
    const double s = wave_sum_f64(s0.m == NEG_INF ? 0.0 : (double)s0.s * exp((double)(s0.m - m) * inv_temp));
    bad = nan || m == NEG_INF;
    if (!bad) ls = log(s);
  }
  const bool evec = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  if (bad) {                                                 // -inf in every column (a sum with -inf is -inf: plain stores)
    constexpr int N = 4;
    const int Vv = V - V % N;
    const float ninf[N] = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
    for (int c0 = lane * N; c0 < Vv; c0 += 64 * N) lm_put<N, false>(out + c0, evec, ninf);
    for (int c = Vv + lane; c < V; c += 64) out[c] = NEG_INF;
    return;
  }
  const float w = a.weight;
  const double dm = (double)m;
  row_scan(z, V, lane, [&](const auto& g, int c0) {
    constexpr int N = sizeof(g) / sizeof(float);
    float lp[N];
#pragma unroll
    for (int j = 0; j < N; ++j) lp[j] = __fmul_rn(w, (float)(((double)g[j] - dm) * inv_temp - ls));
    lm_put<N, ACC>(out + c0, evec, lp);
  });
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_lm_score(const smx_lm_score_args* a, void* stream) {
  const char* who = "smx_lm_score";
  SMX_REQUIRE(a, "%s: null descriptor", who);
  SMX_REQUIRE(a->B >= 1 && a->W >= 1 && a->V >= 1 && a->cap >= 1, "%s: bad sizes B=%d W=%d V=%d cap=%d", who, a->B, a->W, a->V, a->cap);
  SMX_REQUIRE((int64_t)a->B * a->W <= (1 << 24), "%s: B W = %lld rows exceed %d", who, (long long)a->B * a->W, 1 << 24);
  SMX_REQUIRE(a->dtype == SMX_F32 || a->dtype == SMX_BF16, "%s: dtype %d", who, a->dtype);
  SMX_REQUIRE(a->ldz >= a->V && a->lde >= a->V, "%s: ldz %lld / lde %lld smaller than V %d", who, (long long)a->ldz, (long long)a->lde, a->V);
  SMX_REQUIRE(a->weight > 0.f && a->weight < __builtin_inff(), "%s: the weight must be positive and finite", who);
  SMX_REQUIRE(a->inv_temp > 0.0 && a->inv_temp < __builtin_inf(), "%s: the inverse temperature must be positive and finite", who);
  SMX_REQUIRE(a->accumulate == 0 || a->accumulate == 1, "%s: accumulate %d", who, a->accumulate);
  SMX_REQUIRE(a->logits && a->extra && a->score && a->done && a->n_tok, "%s: null pointer", who);
  const dim3 grid((unsigned)((int64_t)a->B * a->W));
  dispatch_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    if (a->accumulate) hipLaunchKernelGGL((lm_score_kernel<T, true>), grid, dim3(64), 0, STREAM, *a);
    else hipLaunchKernelGGL((lm_score_kernel<T, false>), grid, dim3(64), 0, STREAM, *a);
  });
  return check_launch(who);
}
