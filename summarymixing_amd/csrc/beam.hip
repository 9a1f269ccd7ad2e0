// beam.hip - the selection step of the seq2seq beam search (include/smx.h: smx_s2s_beam_select), gfx950 only.  R = B W hypothesis
// rows, utterance b owns rows [b W, (b + 1) W); every position is a device counter, so the two launches are the same at every step
// and one captured step serves the whole search (DESIGN.md I.22 holds the definition of the search).
//
//   a. s2s_beam_rows_kernel   one wave per row of logits.  Pass 1 is smx_s2s_select's reading of the row (row_scan.h: SelRow - the
//                             arg-max and the log-sum-exp in the same expressions, so a beam of 1 gives the greedy search's bits);
//                             passes 2 .. min(W, V) each find the best (value, column) strictly after the previous one.  The logits
//                             are read W times and never written.  A dead row (score -inf), a row holding a NaN and a row of a
//                             finished utterance have no candidates.
//   b. s2s_beam_utt_kernel    one workgroup per utterance.  Wave 0 merges the W sorted lists (a lane holds the heads of two parents,
//                             the 64 lanes meet per winner); thread 0 places the winners that end (eos, or the last step) in the pool;
//                             then the gathers: the parents' token / log-probability / ancestor rows go to the scratch tables,
//                             a barrier, and back into the winners' slots - in place, no host-side ping-pong.  When the utterance
//                             ends, the pool is written out in rank order.
// Nothing is atomic; every choice is a comparison with a total order (score, then parent, then column): two runs agree bit for bit.
#include "row_scan.h"

namespace smx {

static constexpr int BEAM_MAX_W = 128;
static constexpr float POS_INF = __builtin_inff();

// the best (key, column) of a group that lies strictly after (pv, pi) in the order (key descending, column ascending)
template <int N, typename KeyF>
__device__ __forceinline__ void beam_next_take(float& bv, int& bi, const float (&x)[N], int c0, int skip, float pv, int pi, KeyF&& key) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int c = c0 + j;
    const float k = key(x[j], c);
    if (c != skip && (k < pv || (k == pv && c > pi))) argmax_take(bv, bi, k, c);
  }
}

// grid = ceil(R / 4), block = 256: wave w of a block owns row 4 blockIdx.x + w
template <typename T, bool EXTRA>
__global__ __launch_bounds__(256) void s2s_beam_rows_kernel(smx_s2s_beam_args a) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int W = a.W;
  if (r >= (long)a.B * W) return;
  const int b = (int)(r / W);
  const int n = a.n_tok[b];
  const float sc = a.score[r];
  int cnt = 0;
  if (!a.done[b] && sc > NEG_INF && n >= 0 && n < a.cap) {     // (a NaN score fails the comparison: a dead row)
    const T* x = (const T*)a.logits + r * a.ldz;
    const float* ex = EXTRA ? a.extra + r * a.ldx : nullptr;
    const double inv_temp = a.inv_temp;
    const int skip = (n < a.min_steps) ? a.eos : -1;
    SelRow s0 = {NEG_INF, INT_MAX, NEG_INF, 0.f, 0};
    row_scan(x, a.V, lane, [&](const auto& g, int c0) { sel_row_take(s0, g, c0, skip, inv_temp); });
    float pv = s0.bv;
    int pi = s0.bi, nan = s0.nan;
    argmax_meet<64>(pv, pi);
    const float m = wave_max(s0.m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nan |= __shfl_xor(nan, o, 64);
    const double s = wave_sum_f64(s0.m == NEG_INF ? 0.0 : (double)s0.s * exp((double)(s0.m - m) * inv_temp));
    if (!nan && m != NEG_INF) {
      const double ls = log(s);
      auto lp_of = [&](float z) { return (float)(((double)z - (double)m) * inv_temp - ls); };
      auto key = [&](float z, int c) { return EXTRA ? lp_of(z) + ex[c] : z; };
      if (EXTRA) { pv = POS_INF; pi = -1; }                    // the first pass ranked the logits, not lp + extra: rank again
      const int want = W < a.V ? W : a.V;
      for (int q = 0; q < want; ++q) {
        if (EXTRA || q > 0) {
          float bv = NEG_INF;
          int bi = INT_MAX;
          row_scan(x, a.V, lane, [&](const auto& g, int c0) { beam_next_take(bv, bi, g, c0, skip, pv, pi, key); });
          argmax_meet<64>(bv, bi);
          pv = bv; pi = bi;
        }
        if (pi == INT_MAX) break;                              // no column is left
        const float lp = lp_of(to_f32(x[pi]));
        const float cs = sc + (EXTRA ? lp + ex[pi] : lp);
        if (!(cs > NEG_INF)) break;                            // -inf or NaN: no candidate, and none after it in this order
        if (lane == 0) {
          a.cand_val[r * W + q] = cs;
          a.cand_lp[r * W + q] = lp;
          a.cand_idx[r * W + q] = pi;
        }
        cnt = q + 1;
      }
    }
  }
  if (lane == 0) a.cand_n[r] = cnt;
}

// grid = B, block = 256
__global__ __launch_bounds__(256) void s2s_beam_utt_kernel(smx_s2s_beam_args a) {
  __shared__ int w_p[BEAM_MAX_W], w_v[BEAM_MAX_W], w_dst[BEAM_MAX_W];       // the winners: parent, token, -1 alive | -2 dead | pool slot
  __shared__ float w_cs[BEAM_MAX_W], w_lp[BEAM_MAX_W];
  __shared__ float p_f[BEAM_MAX_W];                                          // the pool: final score, insertion serial, rank
  __shared__ int p_seq[BEAM_MAX_W], p_rank[BEAM_MAX_W];
  __shared__ int s_nwin, s_cnt, s_end;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int W = a.W, cap = a.cap;
  const long r0 = (long)b * W;
  const int was_done = a.done[b];
  const int n = a.n_tok[b];
  int cnt0 = a.pool_cnt[b];
  cnt0 = cnt0 < 0 ? 0 : (cnt0 > W ? W : cnt0);
  if (was_done) return;                                                      // a finished utterance changes nothing
  if (n < 0 || n >= cap) {                                                   // (no reset leaves such a counter: end, index nothing)
    __syncthreads();                                                         // every thread has read done[b]
    if (t == 0) a.done[b] = 1;
    for (int i = t; i < W; i += 256) a.done_row[r0 + i] = 1;
    return;
  }
  if (t < 64) {
    // lane t holds the heads of parents t and t + 64: (next position, count, value)
    const int c0 = t < W ? min(max(a.cand_n[r0 + t], 0), W) : 0;
    const int c1 = t + 64 < W ? min(max(a.cand_n[r0 + t + 64], 0), W) : 0;
    int h0 = 0, h1 = 0;
    float v0 = c0 > 0 ? a.cand_val[(r0 + t) * W] : NEG_INF, v1 = c1 > 0 ? a.cand_val[(r0 + t + 64) * W] : NEG_INF;
    int nw = 0;
    for (int i = 0; i < W; ++i) {
      float m = v0;
      int k = v0 > NEG_INF ? t : INT_MAX;
      if (v1 > m) { m = v1; k = t + 64; }                                    // (equal: the lower parent)
      argmax_meet<64>(m, k);
      if (k == INT_MAX) break;                                               // every list is used up (the same in all lanes)
      if ((k & 63) == t) {
        const long o = (r0 + k) * W + (k < 64 ? h0 : h1);
        w_p[i] = k; w_v[i] = a.cand_idx[o]; w_cs[i] = m; w_lp[i] = a.cand_lp[o];
        if (k < 64) { ++h0; v0 = h0 < c0 ? a.cand_val[o + 1] : NEG_INF; }
        else { ++h1; v1 = h1 < c1 ? a.cand_val[o + 1] : NEG_INF; }
      }
      nw = i + 1;
    }
    if (t == 0) s_nwin = nw;
  }
  for (int e = t; e < cnt0; e += 256) { p_f[e] = a.pool_final[r0 + e]; p_seq[e] = a.pool_seq[r0 + e]; }
  __syncthreads();
  const int nwin = s_nwin;
  const bool last = n + 1 >= cap;
  if (t == 0) {
    int cnt = cnt0, ins = a.pool_ins[b], alive = 0;
    for (int i = 0; i < nwin; ++i) {
      if (w_v[i] != a.eos && !last) { w_dst[i] = -1; ++alive; continue; }
      const float f = a.length_norm ? __fdiv_rn(w_cs[i], (float)(n + 1)) : w_cs[i];
      int e;
      if (cnt < W) {
        e = cnt++;
      } else {                                                               // the worst entry: the lowest final score, the latest of equals
        e = 0;
        for (int q = 1; q < W; ++q)
          if (p_f[q] < p_f[e] || (p_f[q] == p_f[e] && p_seq[q] > p_seq[e])) e = q;
        if (!(f > p_f[e])) e = -2;                                           // not strictly better: refused
      }
      w_dst[i] = e;
      if (e >= 0) { p_f[e] = f; p_seq[e] = ins++; }
    }
    s_cnt = cnt;
    s_end = (cnt >= W || last || alive == 0) ? 1 : 0;
    a.pool_cnt[b] = cnt;
    a.pool_ins[b] = ins;
    a.n_tok[b] = n + 1;
  }
  __syncthreads();
  // the parents' rows -> the scratch tables (slots that stay alive) or the pool (slots that end); winner i is wave i % 4's
  for (int i = wave; i < nwin; i += 4) {
    const long src = (r0 + w_p[i]) * cap;
    const int dst = w_dst[i];
    if (dst == -1) {
      const long o = (r0 + i) * cap;
      for (int j = lane; j < n; j += 64) {
        a.s_tokens[o + j] = a.tokens[src + j];
        a.s_logp[o + j] = a.logp_tok[src + j];
        a.s_anc[o + j] = a.anc[src + j];
      }
    } else if (dst >= 0) {
      const long o = (r0 + dst) * cap;
      for (int j = lane; j < cap; j += 64) {                                 // (the whole row: the entry it replaces may have been longer)
        a.pool_tokens[o + j] = j < n ? a.tokens[src + j] : (j == n ? w_v[i] : -1);
        a.pool_logp[o + j] = j < n ? a.logp_tok[src + j] : (j == n ? w_lp[i] : 0.f);
      }
      if (lane == 0) {
        a.pool_len[r0 + dst] = n + 1;
        a.pool_sum[r0 + dst] = w_cs[i];
        a.pool_final[r0 + dst] = p_f[dst];
        a.pool_seq[r0 + dst] = p_seq[dst];
      }
    }
  }
  __syncthreads();                                                           // every parent row has been read
  for (int i = wave; i < W; i += 4) {
    const long row = r0 + i, o = row * cap;
    if (i < nwin && w_dst[i] == -1) {
      for (int j = lane; j < n; j += 64) {
        a.tokens[o + j] = a.s_tokens[o + j];
        a.logp_tok[o + j] = a.s_logp[o + j];
        a.anc[o + j] = a.s_anc[o + j];
      }
      if (lane == 0) {
        a.tokens[o + n] = w_v[i];
        a.logp_tok[o + n] = w_lp[i];
        a.anc[o + n] = (int)(r0 + w_p[i]);                                   // this step's key went to the parent's cache row
        a.score[row] = w_cs[i];
        a.tok[row] = w_v[i];
      }
    } else if (lane == 0) {
      a.score[row] = NEG_INF;
      a.tok[row] = a.eos;
    }
  }
  if (!s_end) return;
  // the utterance ends: the pool in rank order (final score descending, the earlier insertion first among equals)
  const int cnt = s_cnt;
  for (int e = t; e < cnt; e += 256) {
    int rk = 0;
    for (int q = 0; q < cnt; ++q) rk += (p_f[q] > p_f[e] || (p_f[q] == p_f[e] && p_seq[q] < p_seq[e])) ? 1 : 0;
    p_rank[e] = rk;
  }
  __syncthreads();                                                           // (and the pool rows written above are visible)
  for (int e = wave; e < cnt; e += 4) {
    const long src = (r0 + e) * cap, o = (r0 + p_rank[e]) * cap;
    for (int j = lane; j < cap; j += 64) {
      a.res_tokens[o + j] = a.pool_tokens[src + j];
      a.res_logp[o + j] = a.pool_logp[src + j];
    }
    if (lane == 0) {
      a.res_len[r0 + p_rank[e]] = a.pool_len[r0 + e];
      a.res_final[r0 + p_rank[e]] = p_f[e];
      a.res_sum[r0 + p_rank[e]] = a.pool_sum[r0 + e];
    }
  }
  if (t == 0) a.done[b] = 1;
  for (int i = t; i < W; i += 256) a.done_row[r0 + i] = 1;
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_s2s_beam_select(const smx_s2s_beam_args* a, void* stream) {
  SMX_REQUIRE(a, "smx_s2s_beam_select: null descriptor");
  SMX_REQUIRE(a->dtype == SMX_F32 || a->dtype == SMX_BF16, "smx_s2s_beam_select: dtype %d", a->dtype);
  SMX_REQUIRE(a->B >= 1 && a->V >= 1 && a->cap >= 1 && a->ldz >= a->V, "smx_s2s_beam_select: bad sizes B=%d V=%d cap=%d ldz=%lld", a->B, a->V,
              a->cap, (long long)a->ldz);
  SMX_REQUIRE(a->W >= 1 && a->W <= BEAM_MAX_W, "smx_s2s_beam_select: beam size W=%d (1 to %d)", a->W, BEAM_MAX_W);
  SMX_REQUIRE((int64_t)a->B * a->W <= (1 << 24), "smx_s2s_beam_select: B W = %lld rows exceed %d", (long long)a->B * a->W, 1 << 24);
  SMX_REQUIRE(a->inv_temp > 0.0 && a->inv_temp < __builtin_inf(), "smx_s2s_beam_select: the inverse temperature must be positive and finite");
  SMX_REQUIRE(!a->extra || a->ldx >= a->V, "smx_s2s_beam_select: ldx %lld smaller than V %d", (long long)a->ldx, a->V);
  SMX_REQUIRE(a->logits && a->tok && a->score && a->done_row && a->done && a->n_tok && a->tokens && a->logp_tok && a->anc && a->s_tokens &&
                  a->s_logp && a->s_anc && a->cand_val && a->cand_lp && a->cand_idx && a->cand_n && a->pool_tokens && a->pool_logp &&
                  a->pool_len && a->pool_final && a->pool_sum && a->pool_seq && a->pool_cnt && a->pool_ins && a->res_tokens && a->res_logp &&
                  a->res_len && a->res_final && a->res_sum,
              "smx_s2s_beam_select: null pointer");
  const dim3 rgrid((unsigned)(((int64_t)a->B * a->W + 3) / 4));
  dispatch_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    if (a->extra) hipLaunchKernelGGL((s2s_beam_rows_kernel<T, true>), rgrid, dim3(256), 0, STREAM, *a);
    else hipLaunchKernelGGL((s2s_beam_rows_kernel<T, false>), rgrid, dim3(256), 0, STREAM, *a);
  });
  hipLaunchKernelGGL(s2s_beam_utt_kernel, dim3(a->B), dim3(256), 0, STREAM, *a);
  return check_launch("smx_s2s_beam_select");
}
