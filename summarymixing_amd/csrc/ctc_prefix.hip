// ctc_prefix.hip - CTC prefix scoring for the seq2seq beam search (include/smx.h: smx_ctc_prefix_init / _score / _advance), gfx950
// only.  DESIGN.md I.23 holds the definition (Watanabe et al.); the search itself is beam.hip's.  R = B W hypothesis
// rows; every position (the step n, the row's last token, the encoder length T_b) is read on the device, so the launches are the
// same at every step and sit in the one captured chain: decode_step -> seq_lin -> score -> smx_s2s_beam_select(extra) -> advance.
//
//   a. ctc_prefix_init_kernel     one wave per utterance: slot 0's state at parity 0 - r_n = -inf, r_b = the running sum of the blank
//                                 column, psi = 0.
//   b. ctc_prefix_score_kernel    one workgroup per (row, 256 columns).  Wave 0 reads the row of logits as the selection does
//                                 (row_scan.h: SelRow -> the row's max and log-sum-exp), waves 1 .. 3 stage the parent's r_b[t] and
//                                 logaddexp(r_n[t], r_b[t]) in LDS (for one row phi differs only in the column c == last: that lane
//                                 reads the other array).  Then one lane per column c runs the r_n' chain and psi' serially over
//                                 the frames - x[t, c] coalesced across the lanes - and writes extra = weight (ctc - lp).  r_b' is
//                                 not needed for the score; no (R, V, T) state exists.
//   c. ctc_prefix_advance_kernel  one wave per row, after the selection: the winner's parent and token from anc / tokens at
//                                 n_tok - 1, the parent's state from parity (n_tok - 1) & 1 (several children read one parent: two
//                                 buffers), r_n' / r_b' / psi' into the row's own slot at parity n_tok & 1.
// fp32 log-domain throughout (logaddexp as max + log1p(exp(-|d|)), the form the float32 ATen chain uses, on the hardware exp2 / log2
// with the rounding of 1 + e put back: ctcp_lae); no atomics, every sum in frame order: two runs agree bit for bit.
#include "row_scan.h"

namespace smx {

static constexpr int CTCP_MAX_T = 4096;                    // the LDS staging: 8 T bytes (score), 12 T bytes (advance)

static constexpr int CTCP_PREFETCH = 8;                    // frames of x a lane requests ahead of the serial chain

// logaddexp(a, b) = max + log1p(e), e = exp(-|a - b|) in (0, 1], on the hardware exp2 / log2: log1p(e) = log(u) - ((u - 1) - e) / u
// with u = fl(1 + e) - the second term puts back what rounding 1 + e lost, so the result keeps full precision where e is small and
// the sums are near 0 (blank-dominated frames).  About a third of the instructions of log1pf(expf(.)).  -inf when both are.
__device__ __forceinline__ float ctcp_lae(float a, float b) {
#pragma clang fp reassociate(off)
  const float m = fmaxf(a, b);
  const float e = __expf(-fabsf(a - b));
  const float u = 1.f + e;
  const float l = __logf(u) - ((u - 1.f) - e) * __frcp_rn(u);
  return m == NEG_INF ? NEG_INF : m + l;                   // ((-inf) - (-inf) is no number: decided on the max)
}

__device__ __forceinline__ int ctcp_frames(const smx_ctc_prefix_args& a, int b) {
  const int n = a.enc_len[b];
  return n < 1 ? 1 : (n > a.T ? a.T : n);
}

// grid = B, block = 64, LDS 4 T bytes
__global__ __launch_bounds__(64) void ctc_prefix_init_kernel(smx_ctc_prefix_args a) {
  extern __shared__ float lds[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = ctcp_frames(a, b);
  const float* x = a.x + (long)b * a.T * a.ldx + a.blank;
  for (int t = lane; t < Tb; t += 64) lds[t] = x[(long)t * a.ldx];
  __syncthreads();
  if (lane == 0) {
    float s = 0.f;
    for (int t = 0; t < Tb; ++t) { s += lds[t]; lds[t] = s; }
    a.psi[(long)b * a.W] = 0.f;
  }
  __syncthreads();
  float2* dst = reinterpret_cast<float2*>(a.state + (long)b * a.W * a.T * 2);
  for (int t = lane; t < Tb; t += 64) dst[t] = make_float2(NEG_INF, lds[t]);
}

// grid = (R, ceil(V / 256)), block = 256, LDS 8 T bytes
template <typename T>
__global__ __launch_bounds__(256) void ctc_prefix_score_kernel(smx_ctc_prefix_args a) {
  extern __shared__ float lds[];                           // [0, T): r_b, [T, 2 T): logaddexp(r_n, r_b)
  __shared__ float s_m;
  __shared__ double s_ls;
  __shared__ int s_bad;
  const int t_id = threadIdx.x, lane = t_id & 63, wave = t_id >> 6;
  const long r = blockIdx.x, R = (long)a.B * a.W;
  const int c = blockIdx.y * 256 + t_id;
  const int b = (int)(r / a.W);
  const int n = a.n_tok[b];
  const float sc = a.score[r];
  float* out = a.extra + r * a.lde;
  bool live = !a.done[b] && sc > NEG_INF && n >= 0 && n < a.cap;
  float psi_g = NEG_INF;
  if (live) {
    psi_g = a.psi[(n & 1) * R + r];
    live = psi_g > NEG_INF;
  }
  if (!live) {                                             // (the same in every thread of the workgroup)
    if (c < a.V) out[c] = NEG_INF;
    return;
  }
  const int Tb = ctcp_frames(a, b);
  const double inv_temp = a.inv_temp;
  const T* z = (const T*)a.logits + r * a.ldz;
  if (wave == 0) {                                         // the selection's reading of the row: its max and log-sum-exp
    SelRow s0 = {NEG_INF, INT_MAX, NEG_INF, 0.f, 0};
    row_scan(z, a.V, lane, [&](const auto& g, int c0) { sel_row_take(s0, g, c0, -1, inv_temp); });
    int nan = s0.nan;
    const float m = wave_max(s0.m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nan |= __shfl_xor(nan, o, 64);
    const double s = wave_sum_f64(s0.m == NEG_INF ? 0.0 : (double)s0.s * exp((double)(s0.m - m) * inv_temp));
    if (lane == 0) {
      s_bad = (nan || m == NEG_INF) ? 1 : 0;
      s_m = m;
      s_ls = s_bad ? 0.0 : log(s);
    }
  } else {
    const float2* st = reinterpret_cast<const float2*>(a.state + ((long)(n & 1) * R + r) * a.T * 2);
    for (int t = t_id - 64; t < Tb; t += 192) {
      const float2 v = st[t];
      lds[t] = v.y;
      lds[a.T + t] = ctcp_lae(v.x, v.y);
    }
  }
  __syncthreads();
  if (c >= a.V) return;
  if (s_bad) { out[c] = NEG_INF; return; }
  const float lp = (float)(((double)to_f32(z[c]) - (double)s_m) * inv_temp - s_ls);
  float psi1;
  if (c == a.blank) {
    psi1 = NEG_INF;
  } else if (c == a.eos) {
    psi1 = lds[a.T + Tb - 1];
  } else {
    const int last = n > 0 ? a.tokens[r * a.cap + n - 1] : -1;
    const float* phi = lds + (c == last ? 0 : a.T);
    const float* x = a.x + (long)b * a.T * a.ldx + c;
    float rn = n == 0 ? x[0] : NEG_INF;
    psi1 = rn;
    // the chain is serial in t but its loads are not: two groups of CTCP_PREFETCH frames alternate, the next one requested before
    // this one is consumed.  A frame beyond T_b - 1 loads that frame again, unused: unconditional loads keep the wait counts exact.
    constexpr int PF = CTCP_PREFETCH;
    auto fetch = [&](int t0, float (&buf)[PF]) {
#pragma unroll
      for (int j = 0; j < PF; ++j) buf[j] = x[(long)min(t0 + j, Tb - 1) * a.ldx];
    };
    auto chain = [&](int t0, const float (&buf)[PF]) {
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        if (t0 + j < Tb) {                                 // (T_b is the workgroup's: no lane diverges here)
          const float p = phi[t0 + j - 1];
          psi1 = ctcp_lae(psi1, p + buf[j]);
          rn = ctcp_lae(rn, p) + buf[j];
        }
      }
    };
    float even[PF], odd[PF];
    fetch(1, even);
    for (int t0 = 1; t0 < Tb; t0 += 2 * PF) {
      fetch(t0 + PF, odd);
      chain(t0, even);
      fetch(t0 + 2 * PF, even);
      chain(t0 + PF, odd);
    }
  }
  const float ctc = psi1 > NEG_INF ? psi1 - psi_g : NEG_INF;
  out[c] = (lp > NEG_INF && ctc > NEG_INF) ? a.weight * (ctc - lp) : NEG_INF;
}

// grid = R, block = 64, LDS 12 T bytes
__global__ __launch_bounds__(64) void ctc_prefix_advance_kernel(smx_ctc_prefix_args a) {
  extern __shared__ float lds[];                           // phi | x[., c] -> r_n' | x[., blank] -> r_b'
  const int lane = threadIdx.x;
  const long r = blockIdx.x, R = (long)a.B * a.W;
  const int b = (int)(r / a.W);
  if (a.done[b]) return;                                   // a finished utterance changes nothing
  const int n1 = a.n_tok[b];
  if (n1 < 1 || n1 > a.cap || !(a.score[r] > NEG_INF)) return;
  const int c = a.tokens[r * a.cap + n1 - 1], p = a.anc[r * a.cap + n1 - 1];
  if (p < b * a.W || p >= (b + 1) * a.W || c < 0 || c >= a.V || c == a.blank || c == a.eos) return;
  const int Tb = ctcp_frames(a, b), T = a.T;
  const int last = n1 >= 2 ? a.tokens[r * a.cap + n1 - 2] : -1;          // (the row's own history is its parent's plus c)
  const float2* src = reinterpret_cast<const float2*>(a.state + ((long)((n1 - 1) & 1) * R + p) * T * 2);
  float2* dst = reinterpret_cast<float2*>(a.state + ((long)(n1 & 1) * R + r) * T * 2);
  const float* x = a.x + (long)b * T * a.ldx;
  float *phi = lds, *xc = lds + T, *xb = lds + 2 * T;
  for (int t = lane; t < Tb; t += 64) {
    const float2 v = src[t];
    phi[t] = c == last ? v.y : ctcp_lae(v.x, v.y);
    xc[t] = x[(long)t * a.ldx + c];
    xb[t] = x[(long)t * a.ldx + a.blank];
  }
  __syncthreads();
  if (lane == 0) {
    float rn = n1 == 1 ? xc[0] : NEG_INF, rb = NEG_INF, psi1 = rn;
    xc[0] = rn;
    xb[0] = rb;
    for (int t = 1; t < Tb; ++t) {
      const float xt = xc[t], ph = phi[t - 1];
      psi1 = ctcp_lae(psi1, ph + xt);
      const float nrb = ctcp_lae(rn, rb) + xb[t];
      rn = ctcp_lae(rn, ph) + xt;
      rb = nrb;
      xc[t] = rn;
      xb[t] = rb;
    }
    a.psi[(long)(n1 & 1) * R + r] = psi1;
  }
  __syncthreads();
  for (int t = lane; t < Tb; t += 64) dst[t] = make_float2(xc[t], xb[t]);
}

static int ctcp_check(const smx_ctc_prefix_args* a, const char* who, bool score) {
  SMX_REQUIRE(a, "%s: null descriptor", who);
  SMX_REQUIRE(a->B >= 1 && a->W >= 1 && a->V >= 1 && a->T >= 1 && a->cap >= 1, "%s: bad sizes B=%d W=%d V=%d T=%d cap=%d", who, a->B, a->W,
              a->V, a->T, a->cap);
  SMX_REQUIRE(a->T <= CTCP_MAX_T, "%s: T=%d frames exceed the %d the LDS staging holds", who, a->T, CTCP_MAX_T);
  SMX_REQUIRE((int64_t)a->B * a->W <= (1 << 24), "%s: B W = %lld rows exceed %d", who, (long long)a->B * a->W, 1 << 24);
  SMX_REQUIRE(a->ldx >= a->V, "%s: ldx %lld smaller than V %d", who, (long long)a->ldx, a->V);
  SMX_REQUIRE(a->blank >= 0 && a->blank < a->V && a->eos >= 0 && a->eos != a->blank, "%s: blank=%d eos=%d (V=%d)", who, a->blank, a->eos, a->V);
  SMX_REQUIRE(a->x && a->enc_len && a->state && a->psi, "%s: null pointer", who);
  if (score) {
    SMX_REQUIRE(a->dtype == SMX_F32 || a->dtype == SMX_BF16, "%s: dtype %d", who, a->dtype);
    SMX_REQUIRE(a->ldz >= a->V && a->lde >= a->V, "%s: ldz %lld / lde %lld smaller than V %d", who, (long long)a->ldz, (long long)a->lde, a->V);
    SMX_REQUIRE(a->weight > 0.f && a->weight <= 1.f, "%s: the weight must lie in (0, 1]", who);
    SMX_REQUIRE(a->inv_temp > 0.0 && a->inv_temp < __builtin_inf(), "%s: the inverse temperature must be positive and finite", who);
    SMX_REQUIRE(a->logits && a->extra, "%s: null pointer", who);
  }
  return SMX_OK;
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_ctc_prefix_init(const smx_ctc_prefix_args* a, void* stream) {
  if (int e = ctcp_check(a, "smx_ctc_prefix_init", false)) return e;
  hipLaunchKernelGGL(ctc_prefix_init_kernel, dim3(a->B), dim3(64), (size_t)a->T * 4, STREAM, *a);
  return check_launch("smx_ctc_prefix_init");
}

extern "C" int smx_ctc_prefix_score(const smx_ctc_prefix_args* a, void* stream) {
  if (int e = ctcp_check(a, "smx_ctc_prefix_score", true)) return e;
  SMX_REQUIRE(a->score && a->done && a->n_tok && a->tokens, "smx_ctc_prefix_score: null pointer");
  const dim3 grid((unsigned)((int64_t)a->B * a->W), (unsigned)((a->V + 255) / 256));
  dispatch_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((ctc_prefix_score_kernel<T>), grid, dim3(256), (size_t)a->T * 8, STREAM, *a);
  });
  return check_launch("smx_ctc_prefix_score");
}

extern "C" int smx_ctc_prefix_advance(const smx_ctc_prefix_args* a, void* stream) {
  if (int e = ctcp_check(a, "smx_ctc_prefix_advance", false)) return e;
  SMX_REQUIRE(a->score && a->done && a->n_tok && a->tokens && a->anc, "smx_ctc_prefix_advance: null pointer");
  hipLaunchKernelGGL(ctc_prefix_advance_kernel, dim3((unsigned)((int64_t)a->B * a->W)), dim3(64), (size_t)a->T * 12, STREAM, *a);
  return check_launch("smx_ctc_prefix_advance");
}
