// tbeam.hip — transducer beam search with an optional LM score (recipe key `Beamsearcher`: speechbrain.decoders.transducer.
// TransducerBeamSearcher with beam_size 10, lm_module, lm_weight 0.5, state_beam 2.3, expand_beam 2.3, …transducer.yaml:383-393),
// gfx950 only.  DESIGN.md I.25 holds the definition of the search and of its two caps.
//
// The unit is the EXPANSION: every utterance carries its own frame counter on the device, one step expands the current best open
// hypothesis of every utterance that is not done, and every step is the same launches whatever the data:
//   1. tbeam_pred_kernel     the LSTM tile of greedy_step_kernel without its select half and without a mask: token cur_tok[b] (the
//                            W_ih^T row gather of onehot_col), h_in / c_in -> h_out / c_out, all per-utterance staging rows.
//   2. tbeam_proj_kernel     pdec = h_out W_proj^T (greedy_proj_kernel's tile).
//   3. tbeam_logits_kernel   z[b,:] = act(enc[b, frames[b], :] + pdec[b]) W_lin^T + b_lin - greedy_logits_kernel's arithmetic and
//                            roundings with the frame read on the device - STORED in fp32 (the selection needs a top-k).
//   (the caller's LM step goes here: its logits and its new state land in staging rows of the same shape)
//   4. tbeam_select_kernel   one workgroup per utterance: log-softmax of the z row and of the LM row (row_scan.h: SelRow), the exact
//                            top-W by repeated arg-max, the child inserts, the frame logic, the next pick, and the state moves - the
//                            new state into its slot once per expansion, the survivors' states into the other half of the ping-pong
//                            at a frame end, the picked hypothesis' state into the staging rows of the next step.
// Lists, nodes, prefixes and state slots of an utterance live in one block of `state` (TbLayout below); every index read from it is
// clamped to its capacity before use and every insert is checked against it.  No atomics, every sum in a fixed order, nothing
// depends on B or on the other rows.
// The same search carried across streaming chunks: tbeam_resume_kernel before a chunk's steps (a slot starts, sits out or
// is re-armed) and tbeam_select_kernel<T, true>, which at a chunk's last frame writes the result AND does the frame end (done = paused).
#include "lstm_tile.h"
#include "row_scan.h"

#include <limits.h>

#include <algorithm>

namespace smx {

static constexpr int TBEAM_TILE_V = 128;
static constexpr int TBEAM_J_MAX = 832;           // as greedy.hip: 16 rows of a and the 16 x 129 logit tile stay below 64 KB of LDS
static constexpr int TBEAM_W_MAX = 32;
static constexpr int TBEAM_V_MAX = 8192;          // the selection holds the z row in LDS
static constexpr size_t TBEAM_LDS_MAX = 60 * 1024;
static bool tbeam_shape_ok(int H, int J, int V, int W) {
  return lstm_h_ok(H) && J >= 64 && J <= TBEAM_J_MAX && J % 64 == 0 && V >= 3 && V <= TBEAM_V_MAX && W >= 2 && W <= TBEAM_W_MAX && W < V;
}

template <typename T> struct TbeamPad;
template <> struct TbeamPad<float> { static constexpr int value = 4; };
template <> struct TbeamPad<bf16_t> { static constexpr int value = 8; };

// ---- the per-utterance block of `state`, byte offsets (every section 16-byte aligned)
struct TbLayout {
  long meta;                 // int32[8]: nA, nB, nexp, half, cur_node, cur_len, cur_score (bits), a stream's dead flag (0 after an init)
  long a_node, a_len, a_tok, a_score;      // NA entries each: the open list in insertion order, node -1 = removed
  long b_node, b_len, b_tok, b_score;      // W entries each: the closed list in insertion order
  long nd_parent, nd_tok;    // E W in-frame nodes: node W + e W + j is child j of expansion e
  long prefix;               // (2, W, U) int32: the survivors' tokens, per half
  long plen;                 // (2, W) int32
  long dec_h, dec_c;         // (2, NS, H) dtype / fp32
  long lm_h, lm_c;           // (2, NS, L, Hl) dtype / fp32
  long total;
  int NA, NS;
};

static inline long tb_up16(long x) { return (x + 15) & ~15L; }
static TbLayout tbeam_layout(int es, int H, int W, int E, int U, int Lc, int Hl) {
  TbLayout L;
  L.NA = W + E * W;
  L.NS = W + E;
  long o = 0;
  auto take = [&](long bytes) { const long at = o; o = tb_up16(o + bytes); return at; };
  L.meta = take(32);
  L.a_node = take(4L * L.NA); L.a_len = take(4L * L.NA); L.a_tok = take(4L * L.NA); L.a_score = take(4L * L.NA);
  L.b_node = take(4L * W); L.b_len = take(4L * W); L.b_tok = take(4L * W); L.b_score = take(4L * W);
  L.nd_parent = take(4L * E * W); L.nd_tok = take(4L * E * W);
  L.prefix = take(8L * W * U);
  L.plen = take(8L * W);
  L.dec_h = take(2L * L.NS * H * es); L.dec_c = take(2L * L.NS * H * 4);
  L.lm_h = take(2L * L.NS * Lc * Hl * es); L.lm_c = take(2L * L.NS * Lc * Hl * 4);
  L.total = o;
  return L;
}

// ---- 1. the prediction-network step
template <typename T>
__global__ __launch_bounds__(256) void tbeam_pred_kernel(smx_tbeam_args a) {
  __shared__ float red[4][16][17];
  const int H = a.H, j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int bb = threadIdx.x >> 4, jj = threadIdx.x & 15, b = b0 + bb, j = j0 + jj;
  gate_tiles(red, reinterpret_cast<const T*>(a.h_in), (long)H, a.Whh, H, a.B, b0, j0);
  if (b >= a.B) return;
  const int col = onehot_col(a.cur_tok[b], a.V, a.blank);
  float z[4], g[4], c;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float wx = col >= 0 ? to_f32(reinterpret_cast<const T*>(a.WihT)[(long)col * a.ldw + i * H + j]) : 0.f;
    z[i] = red[i][bb][jj] + onehot_gate_input(1.f, wx, a.bias[i * H + j]);
  }
  reinterpret_cast<T*>(a.h_out)[(long)b * H + j] = from_f32<T>(lstm_cell(z, a.c_in[(long)b * H + j], g, c));
  a.c_out[(long)b * H + j] = c;
}

// ---- 2. pdec (B, J) = h (B, H) . W_proj (J, H)^T: a workgroup owns 16 rows x 64 columns, one 16-column tile per wave
template <typename T>
__global__ __launch_bounds__(256) void tbeam_proj_kernel(const T* __restrict__ h, const T* __restrict__ Wp, T* __restrict__ pdec, int B, int H, int J) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int j0 = blockIdx.x * 64 + 16 * w, b0 = blockIdx.y * 16;
  const lstm_f32x4 acc = tile_dot(h + (long)min(b0 + r, B - 1) * H, Wp + (long)(j0 + r) * H, H, q);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = b0 + q * 4 + i;
    if (b < B) pdec[(long)b * J + j0 + r] = from_f32<T>(acc[i]);
  }
}

// ---- 3. the joint logits of the utterances' current frames, stored
template <typename T>
__global__ __launch_bounds__(256) void tbeam_logits_kernel(smx_tbeam_args s) {
  extern __shared__ __attribute__((aligned(16))) char tbeam_lds[];
  __shared__ float zt[16][TBEAM_TILE_V + 1];
  constexpr int PAD = TbeamPad<T>::value;
  const int J = s.J, lda = J + PAD, v0 = blockIdx.x * TBEAM_TILE_V, b0 = blockIdx.y * 16;
  T* a = reinterpret_cast<T*>(tbeam_lds);
  const T* enc = reinterpret_cast<const T*>(s.enc);
  const T* pdec = reinterpret_cast<const T*>(s.pdec);
  dispatch_act(s.act, [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    for (int idx = threadIdx.x * 4; idx < 16 * J; idx += 1024) {
      const int row = idx / J, col = idx - row * J;
      const int b = min(b0 + row, s.B - 1);
      const int t = min(max(s.frames[b], 0), s.T - 1);                        // (a done utterance re-reads its last frame)
      float e[4], p[4];
      load4(enc + (long)b * s.ld_b + (long)t * s.ld_t + col, e);
      load4(pdec + (long)b * J + col, p);
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = act_fwd_c<ACT>(e[i] + p[i]);
      store4(a + row * lda + col, e);
    }
  });
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int c0 = 32 * w + 16 * half, v = v0 + c0 + r;                      // this lane's vocabulary column
    const T* b_row = reinterpret_cast<const T*>(s.Wlin) + (long)min(v, s.V - 1) * J;
    const lstm_f32x4 acc = tile_dot(a + r * lda, b_row, J, q);
    const float bias = (s.blin && v < s.V) ? s.blin[v] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) zt[q * 4 + i][c0 + r] = acc[i] + bias;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 16 * TBEAM_TILE_V; idx += 256) {
    const int row = idx / TBEAM_TILE_V, col = idx - row * TBEAM_TILE_V, b = b0 + row, v = v0 + col;
    if (b < s.B && v < s.V) s.z[(long)b * s.V + v] = zt[row][col];
  }
}

// ---- 4. the selection
// the best (key, index) of a list, over the whole workgroup: key = score / len, the lowest index among equals; INT_MAX: no entry
__device__ __forceinline__ int tb_pick(const int* node, const int* len, const float* score, int n, float* pv, int* pi) {
  float m = NEG_INF;
  int k = INT_MAX;
  for (int i = threadIdx.x; i < n; i += 256)
    if (node[i] >= 0) argmax_take(m, k, score[i] / (float)len[i], i);
  argmax_meet<64>(m, k);
  if ((threadIdx.x & 63) == 0) { pv[threadIdx.x >> 6] = m; pi[threadIdx.x >> 6] = k; }
  __syncthreads();
  m = pv[0]; k = pi[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) argmax_take(m, k, pv[q], pi[q]);
  __syncthreads();
  return k;
}

// the state slot of a node: a root (a survivor of the frame before) holds its own, child j of expansion e shares slot W + e
__device__ __forceinline__ int tb_slot(int node, int W, int NS) {
  const int s = node < W ? node : W + (node - W) / W;
  return min(max(s, 0), NS - 1);
}

// one thread: the in-frame part of a hypothesis' tokens into dst (U ints), back to front -> its root and the root's share
__device__ __forceinline__ void tb_walk(int node, int len, const int* nd_parent, const int* nd_tok, int W, int E, int U, int32_t* dst,
                                        int& root, int& rootlen) {
  int pos = min(len - 1, U) - 1;
  for (int guard = 0; node >= W && guard <= E; ++guard) {
    const int idx = node - W;
    if (idx >= E * W) { node = 0; break; }
    if (pos >= 0) dst[pos] = nd_tok[idx];
    --pos;
    node = nd_parent[idx];
  }
  root = min(max(node, 0), W - 1);
  rootlen = max(pos + 1, 0);
}

// STREAMED (smx_tbeam_select_stream): a.T / a.lengths / a.frames are those of one CHUNK and sframes counts the frames of
// the whole stream.  The one difference is the frame end at the chunk's last frame: the result is written AND the ordinary turnover is
// done, so that the next chunk goes on from the staged pick; done[b] then means paused.  Everything else is the code below, once.
template <typename T, bool STREAMED>
__global__ __launch_bounds__(256) void tbeam_select_kernel(smx_tbeam_args a, TbLayout L, int32_t* __restrict__ sframes) {
  extern __shared__ __attribute__((aligned(16))) char tbeam_lds[];
  __shared__ int B_node[TBEAM_W_MAX], B_len[TBEAM_W_MAX], B_tok[TBEAM_W_MAX], topk[TBEAM_W_MAX], w_root[TBEAM_W_MAX], w_rootlen[TBEAM_W_MAX],
      src_slot[TBEAM_W_MAX], order[TBEAM_W_MAX];
  __shared__ float B_score[TBEAM_W_MAX], topv[TBEAM_W_MAX], pv[4];
  __shared__ int pi[4], sh[8];
  __shared__ double s_m[2], s_ls[2];
  enum { NA_ = 0, NB_, NEXP_, END_, OVF_ };
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (a.done[b]) return;
  const int V = a.V, W = a.W, E = a.E, U = a.U, NA = L.NA, NS = L.NS, blank = a.blank;
  float* zs = reinterpret_cast<float*>(tbeam_lds);
  int* A_node = reinterpret_cast<int*>(zs + ((V + 3) & ~3));
  int* A_len = A_node + NA;
  int* A_tok = A_len + NA;
  float* A_score = reinterpret_cast<float*>(A_tok + NA);
  char* st = reinterpret_cast<char*>(a.state) + (long)b * L.total;
  int* meta = reinterpret_cast<int*>(st + L.meta);
  int* g_nd_parent = reinterpret_cast<int*>(st + L.nd_parent);
  int* g_nd_tok = reinterpret_cast<int*>(st + L.nd_tok);
  int32_t* g_prefix = reinterpret_cast<int32_t*>(st + L.prefix);
  int* g_plen = reinterpret_cast<int*>(st + L.plen);
  const int nA0 = min(max(meta[0], 0), NA), nB0 = min(max(meta[1], 0), W), e = min(max(meta[2], 0), E - 1), half = meta[3] & 1;
  const int cur_node = min(max(meta[4], 0), W + E * W - 1), cur_len = max(meta[5], 1);
  const float cur_score = __int_as_float(meta[6]);
  const int len_b = a.lengths ? min(max(a.lengths[b], 0), a.T) : a.T;
  // the lists and the z row into LDS
  for (int i = tid; i < nA0; i += 256) {
    A_node[i] = reinterpret_cast<const int*>(st + L.a_node)[i]; A_len[i] = max(reinterpret_cast<const int*>(st + L.a_len)[i], 1);
    A_tok[i] = reinterpret_cast<const int*>(st + L.a_tok)[i]; A_score[i] = reinterpret_cast<const float*>(st + L.a_score)[i];
  }
  if (tid < nB0) {
    B_node[tid] = reinterpret_cast<const int*>(st + L.b_node)[tid]; B_len[tid] = max(reinterpret_cast<const int*>(st + L.b_len)[tid], 1);
    B_tok[tid] = reinterpret_cast<const int*>(st + L.b_tok)[tid]; B_score[tid] = reinterpret_cast<const float*>(st + L.b_score)[tid];
  }
  const float* zrow = a.z + (long)b * V;
  for (int c = tid; c < V; c += 256) zs[c] = zrow[c];
  // the two log-sum-exps: wave 0 the joint row, wave 1 the LM row, each in the expressions of the seq2seq selections
  if (wv == 0 || (wv == 1 && a.lm_L > 0)) {
    SelRow s0 = {NEG_INF, INT_MAX, NEG_INF, 0.f, 0};
    if (wv == 0) row_scan(zrow, V, lane, [&](const auto& g, int c0) { sel_row_take(s0, g, c0, -1, 1.0); });
    else row_scan(reinterpret_cast<const T*>(a.lm_logits) + (long)b * a.ld_lm, V, lane, [&](const auto& g, int c0) { sel_row_take(s0, g, c0, -1, 1.0); });
    const float m = wave_max(s0.m);
    const double s = wave_sum_f64(s0.m == NEG_INF ? 0.0 : (double)s0.s * exp((double)(s0.m - m)));
    if (lane == 0) { s_m[wv] = (double)m; s_ls[wv] = log(s); }
  }
  __syncthreads();
  // the W best of the row, (value descending, index ascending): each pass takes the best strictly after the one before
  {
    float prev_v = __builtin_inff();
    int prev_i = -1;
    for (int j = 0; j < W; ++j) {
      float m = NEG_INF;
      int k = INT_MAX;
      for (int c = tid; c < V; c += 256) {
        const float v = zs[c];
        if (v < prev_v || (v == prev_v && c > prev_i)) argmax_take(m, k, v, c);
      }
      argmax_meet<64>(m, k);
      if (lane == 0) { pv[wv] = m; pi[wv] = k; }
      __syncthreads();
      m = pv[0]; k = pi[0];
#pragma unroll
      for (int q = 1; q < 4; ++q) argmax_take(m, k, pv[q], pi[q]);
      if (tid == 0) { topv[j] = m; topk[j] = k; }
      prev_v = m; prev_i = k;
      __syncthreads();
    }
  }
  // the children (one thread: at most W inserts, in the order of the top-k)
  if (tid == 0) {
    const double m = s_m[0], ls = s_ls[0];
    auto lp_of = [&](float z) { return (float)(((double)z - m) - ls); };
    int nA = nA0, nB = nB0, ovf = a.overflow[b];
    const bool capped = cur_len - 1 >= U;
    if (capped) ovf |= 2;
    const bool ok0 = topk[0] >= 0 && topk[0] < V, ok1 = topk[1] >= 0 && topk[1] < V;
    const float best = (ok0 && topk[0] != blank) ? lp_of(topv[0]) : (ok1 ? lp_of(topv[1]) : NEG_INF);
    bool blank_in = false;
    for (int j = 0; j < W; ++j) {
      const int k = topk[j];
      if (k < 0 || k >= V) break;                                             // (fewer than W numbers in the row)
      const float v = lp_of(topv[j]);
      if (k == blank) {
        blank_in = true;
        if (nB < W) { B_node[nB] = cur_node; B_len[nB] = cur_len; B_tok[nB] = a.cur_tok[b]; B_score[nB] = cur_score + v; ++nB; }
      } else if (!capped && v >= best - a.expand_beam && nA < NA) {
        float s = cur_score + v;
        if (a.lm_L > 0) {
          const float zl = to_f32(reinterpret_cast<const T*>(a.lm_logits)[(long)b * a.ld_lm + k]);
          s = s + a.lm_weight * (float)(((double)zl - s_m[1]) - s_ls[1]);
        }
        const int idx = e * W + j;
        g_nd_parent[idx] = cur_node; g_nd_tok[idx] = k;
        A_node[nA] = W + idx; A_len[nA] = cur_len + 1; A_tok[nA] = k; A_score[nA] = s; ++nA;
      }
    }
    if (capped && !blank_in && nB < W) {                                      // at the symbol cap a hypothesis always closes
      B_node[nB] = cur_node; B_len[nB] = cur_len; B_tok[nB] = a.cur_tok[b]; B_score[nB] = cur_score + lp_of(zs[blank]); ++nB;
    }
    sh[NA_] = nA; sh[NB_] = nB; sh[NEXP_] = e + 1; sh[OVF_] = ovf; sh[END_] = 0;
    a.expansions[b] += 1;
  }
  __syncthreads();
  int nA = sh[NA_], nB = sh[NB_];
  const int nexp = sh[NEXP_];
  int ia = INT_MAX;
  bool end = nB >= W;
  if (!end && nexp >= E) {
    // the expansion cap: the frame ends, the closed list is filled with the best of the open one
    end = true;
    while (nB < W) {
      const int i = tb_pick(A_node, A_len, A_score, nA, pv, pi);
      if (i >= nA) break;
      if (tid == 0) { B_node[nB] = A_node[i]; B_len[nB] = A_len[i]; B_tok[nB] = A_tok[i]; B_score[nB] = A_score[i]; A_node[i] = -1; }
      ++nB;
      __syncthreads();
    }
    if (tid == 0) sh[OVF_] |= 1;
  }
  if (!end) {
    ia = tb_pick(A_node, A_len, A_score, nA, pv, pi);
    if (ia >= nA) end = true;                                                 // nothing left to expand
    else if (nB > 0) {
      const int ib = tb_pick(B_node, B_len, B_score, nB, pv, pi);
      if (ib < nB && B_score[ib] >= a.state_beam + A_score[ia]) end = true;
    }
  }
  const int save_slot = W + e;                                                // where this expansion's new state goes, in `half`
  int new_half = half, ncopy = 0;
  if (end) {
    const int frame = a.frames[b] + 1;
    if (frame >= len_b || nB == 0) {
      // the last frame closed: the closed list sorted by key (stable), the first nbest written out
      const int n_out = min(nB, a.nbest);
      for (int r = 0; r < n_out; ++r) {
        const int i = tb_pick(B_node, B_len, B_score, nB, pv, pi);
        if (tid == 0) {
          order[r] = min(i, nB - 1);
          if (i < nB) {
            a.scores[(long)b * a.nbest + r] = B_score[i] / (float)B_len[i];
            a.sums[(long)b * a.nbest + r] = B_score[i];
            a.out_len[(long)b * a.nbest + r] = min(B_len[i] - 1, U);
          }
        }
        __syncthreads();
        if (tid == 0 && i < nB) B_node[i] = -1 - B_node[i];                   // (taken: out of the next pick, the node kept)
        __syncthreads();
      }
      if (tid < n_out) {
        const int i = order[tid];
        tb_walk(-1 - B_node[i], B_len[i], g_nd_parent, g_nd_tok, W, E, U, a.tokens + ((long)b * a.nbest + tid) * U, w_root[tid], w_rootlen[tid]);
      }
      __syncthreads();
      for (int r = 0; r < n_out; ++r) {
        const int32_t* src = g_prefix + ((long)half * W + w_root[r]) * U;
        const int n = min(w_rootlen[r], min(max(g_plen[half * W + w_root[r]], 0), U));
        for (int p = tid; p < n; p += 256) a.tokens[((long)b * a.nbest + r) * U + p] = src[p];
      }
      if constexpr (!STREAMED) {
        if (tid == 0) {
          a.n_hyps[b] = n_out; a.frames[b] = frame; a.overflow[b] = sh[OVF_] | (nB == 0 ? 4 : 0); a.done[b] = 1;
        }
        return;
      } else {
        // a pause: an earlier pause's result lies in the buffers, so what this one does not write goes back to its cleared value
        // (order[] and B_len[] are as the sort left them; the positions written above and those padded here are disjoint)
        for (long i = tid; i < (long)a.nbest * U; i += 256) {
          const int r = (int)(i / U), p = (int)(i - (long)r * U);
          if (p >= (r < n_out ? min(B_len[order[r]] - 1, U) : 0)) a.tokens[(long)b * a.nbest * U + i] = -1;
        }
        for (int r = n_out + tid; r < a.nbest; r += 256) {
          a.out_len[(long)b * a.nbest + r] = 0; a.scores[(long)b * a.nbest + r] = NEG_INF; a.sums[(long)b * a.nbest + r] = NEG_INF;
        }
        if (tid == 0) { a.n_hyps[b] = n_out; a.done[b] = 1; }
        if (nB == 0) {                                                        // nothing to go on from: the slot is dead until started again
          if (tid == 0) { a.frames[b] = frame; sframes[b] += 1; a.overflow[b] = sh[OVF_] | 4; meta[7] = 1; }
          return;
        }
        if (tid < nB && B_node[tid] < 0) B_node[tid] = -1 - B_node[tid];      // the sort's marks off: the turnover reads the nodes
        __syncthreads();
      }
    }
    // the survivors become the roots of the next frame: prefixes materialised and states copied into the other half
    new_half = half ^ 1;
    ncopy = nB;
    if (tid < nB) {
      tb_walk(B_node[tid], B_len[tid], g_nd_parent, g_nd_tok, W, E, U, g_prefix + ((long)new_half * W + tid) * U, w_root[tid], w_rootlen[tid]);
      src_slot[tid] = tb_slot(B_node[tid], W, NS);
    }
    __syncthreads();
    for (int r = 0; r < nB; ++r) {
      const int32_t* src = g_prefix + ((long)half * W + w_root[r]) * U;
      const int n = min(w_rootlen[r], min(max(g_plen[half * W + w_root[r]], 0), U));
      for (int p = tid; p < n; p += 256) g_prefix[((long)new_half * W + r) * U + p] = src[p];
    }
    if (tid < nB) {
      g_plen[new_half * W + tid] = min(B_len[tid] - 1, U);
      A_node[tid] = tid; A_len[tid] = B_len[tid]; A_tok[tid] = B_tok[tid]; A_score[tid] = B_score[tid];
    }
    __syncthreads();
    nA = nB; nB = 0;
    if (tid == 0) {
      a.frames[b] = frame;
      if constexpr (STREAMED) sframes[b] += 1;
    }
    ia = tb_pick(A_node, A_len, A_score, nA, pv, pi);
    ia = min(ia, nA - 1);                                                     // (nA >= 1 here; a list of NaN keys takes its last)
  }
  // the next hypothesis to expand leaves the open list and is staged
  const int nx_node = A_node[ia], nx_len = A_len[ia], nx_tok = A_tok[ia];
  const float nx_score = A_score[ia];
  __syncthreads();
  if (tid == 0) {
    A_node[ia] = -1;
    meta[0] = nA; meta[1] = nB; meta[2] = end ? 0 : nexp; meta[3] = new_half; meta[4] = nx_node; meta[5] = nx_len;
    meta[6] = __float_as_int(nx_score);
    a.cur_tok[b] = nx_tok;
    a.overflow[b] = sh[OVF_];
  }
  __syncthreads();
  for (int i = tid; i < nA; i += 256) {
    reinterpret_cast<int*>(st + L.a_node)[i] = A_node[i]; reinterpret_cast<int*>(st + L.a_len)[i] = A_len[i];
    reinterpret_cast<int*>(st + L.a_tok)[i] = A_tok[i]; reinterpret_cast<float*>(st + L.a_score)[i] = A_score[i];
  }
  if (tid < nB) {
    reinterpret_cast<int*>(st + L.b_node)[tid] = B_node[tid]; reinterpret_cast<int*>(st + L.b_len)[tid] = B_len[tid];
    reinterpret_cast<int*>(st + L.b_tok)[tid] = B_tok[tid]; reinterpret_cast<float*>(st + L.b_score)[tid] = B_score[tid];
  }
  // the state moves.  A thread owns the same 16 bytes of a row through all three, so they need no barrier between them:
  //   the new state -> slot W + e of `half`;  the survivors' slots -> slots 0 .. of the other half;  the pick's slot -> staging
  const int nx_slot = tb_slot(nx_node, W, NS);
  auto move = [&](const void* out_row, void* in_row, long store, long row_bytes, long slot_stride) {
    const uint4* o = reinterpret_cast<const uint4*>(out_row);
    uint4* in = reinterpret_cast<uint4*>(in_row);
    char* base = st + store;
    const long half_stride = (long)NS * slot_stride;
    for (long x = tid; x < row_bytes / 16; x += 256) {
      *(reinterpret_cast<uint4*>(base + half * half_stride + save_slot * slot_stride) + x) = o[x];
      for (int i = 0; i < ncopy; ++i)
        *(reinterpret_cast<uint4*>(base + new_half * half_stride + i * slot_stride) + x) =
            *(reinterpret_cast<const uint4*>(base + half * half_stride + src_slot[i] * slot_stride) + x);
      in[x] = *(reinterpret_cast<const uint4*>(base + new_half * half_stride + nx_slot * slot_stride) + x);
    }
  };
  const long es = sizeof(T), H = a.H;
  move(reinterpret_cast<const char*>(a.h_out) + b * H * es, reinterpret_cast<char*>(a.h_in) + b * H * es, L.dec_h, H * es, H * es);
  move(a.c_out + b * H, a.c_in + b * H, L.dec_c, H * 4, H * 4);
  if (a.lm_L > 0) {
    const long Hl = a.lm_H, Lc = a.lm_L;
    for (long l = 0; l < Lc; ++l) {
      move(reinterpret_cast<const char*>(a.lm_h_out) + (l * a.B + b) * Hl * es, reinterpret_cast<char*>(a.lm_h_in) + (l * a.B + b) * Hl * es,
           L.lm_h + l * Hl * es, Hl * es, Lc * Hl * es);
      move(a.lm_c_out + (l * a.B + b) * Hl, a.lm_c_in + (l * a.B + b) * Hl, L.lm_c + l * Hl * 4, Hl * 4, Lc * Hl * 4);
    }
  }
}

// ---- the start of a search: every utterance holds the one hypothesis [blank] with zero states, already picked for step 0
template <typename T>
__device__ __forceinline__ void tb_init_row(const smx_tbeam_args& a, const TbLayout& L, int b) {
  const int tid = threadIdx.x;
  char* st = reinterpret_cast<char*>(a.state) + (long)b * L.total;
  const long es = sizeof(T), H = a.H, Hl = a.lm_H, Lc = a.lm_L;
  const uint4 zero = {0u, 0u, 0u, 0u};
  auto clear = [&](void* p, long bytes) {
    for (long x = tid; x < bytes / 16; x += 256) reinterpret_cast<uint4*>(p)[x] = zero;
  };
  clear(reinterpret_cast<char*>(a.h_in) + b * H * es, H * es);
  clear(a.c_in + b * H, H * 4);
  clear(st + L.dec_h, H * es);                                                // (slot 0 of half 0: the first hypothesis' state)
  clear(st + L.dec_c, H * 4);
  for (long l = 0; l < Lc; ++l) {
    clear(reinterpret_cast<char*>(a.lm_h_in) + (l * a.B + b) * Hl * es, Hl * es);
    clear(a.lm_c_in + (l * a.B + b) * Hl, Hl * 4);
  }
  clear(st + L.lm_h, Lc * Hl * es);
  clear(st + L.lm_c, Lc * Hl * 4);
  for (long i = tid; i < (long)a.nbest * a.U; i += 256) a.tokens[(long)b * a.nbest * a.U + i] = -1;
  for (int i = tid; i < a.nbest; i += 256) {
    a.out_len[(long)b * a.nbest + i] = 0; a.scores[(long)b * a.nbest + i] = NEG_INF; a.sums[(long)b * a.nbest + i] = NEG_INF;
  }
  for (int i = tid; i < 2 * a.W; i += 256) reinterpret_cast<int*>(st + L.plen)[i] = 0;
  if (tid == 0) {
    int* meta = reinterpret_cast<int*>(st + L.meta);
    meta[0] = 0; meta[1] = 0; meta[2] = 0; meta[3] = 0; meta[4] = 0; meta[5] = 1; meta[6] = 0; meta[7] = 0;
    a.cur_tok[b] = a.blank;
    a.frames[b] = 0; a.expansions[b] = 0; a.overflow[b] = 0; a.n_hyps[b] = 0;
    const int len_b = a.lengths ? min(max(a.lengths[b], 0), a.T) : a.T;
    if (len_b == 0) {                                                         // no frame: the empty hypothesis, score 0
      a.done[b] = 1; a.n_hyps[b] = 1; a.scores[(long)b * a.nbest] = 0.f; a.sums[(long)b * a.nbest] = 0.f;
    } else {
      a.done[b] = 0;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void tbeam_init_kernel(smx_tbeam_args a, TbLayout L) {
  tb_init_row<T>(a, L, blockIdx.x);
}

// ---- the start of a chunk of a stream: a slot marked `start` is initialised as above, for its own row; a slot that is
// dead (meta[7]) or gets no frame is left as it was; any other is re-armed - the hypothesis staged at the pause is the one to expand
template <typename T>
__global__ __launch_bounds__(256) void tbeam_resume_kernel(smx_tbeam_args a, TbLayout L, const uint8_t* __restrict__ start, int32_t* __restrict__ sframes) {
  const int b = blockIdx.x;
  if (start[b]) {
    tb_init_row<T>(a, L, b);
    if (threadIdx.x == 0) sframes[b] = 0;
    return;
  }
  if (threadIdx.x != 0) return;
  const int len_b = min(max(a.lengths[b], 0), a.T);
  const int dead = reinterpret_cast<const int*>(reinterpret_cast<const char*>(a.state) + (long)b * L.total + L.meta)[7];
  if (dead || len_b == 0) return;
  a.frames[b] = 0;
  a.done[b] = 0;
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_tbeam_ok(int dtype, int H, int J, int V, int W) {
  return (dtype == SMX_F32 || dtype == SMX_BF16) && tbeam_shape_ok(H, J, V, W) ? 1 : 0;
}

static size_t tbeam_select_lds(int V, int W, int E) { return (size_t)((V + 3) & ~3) * 4 + (size_t)(W + E * W) * 16; }

static int tbeam_check(const char* what, const smx_tbeam_args* a, TbLayout* L) {
  SMX_REQUIRE(a, "%s: null argument struct", what);
  SMX_REQUIRE(a->dtype == SMX_F32 || a->dtype == SMX_BF16, "%s: bad dtype %d", what, a->dtype);
  SMX_REQUIRE(a->B >= 1 && a->B <= 65535 && a->T >= 1 && a->H >= 1 && a->J >= 1 && a->V >= 1 && a->W >= 1, "%s: bad sizes B=%d T=%d H=%d J=%d V=%d W=%d",
              what, a->B, a->T, a->H, a->J, a->V, a->W);
  SMX_REQUIRE(a->nbest >= 1 && a->nbest <= a->W && a->E >= 1 && a->E <= 4096 && a->U >= 1 && a->U <= (1 << 20), "%s: bad nbest=%d (W=%d), max_expansions=%d or max_symbols=%d",
              what, a->nbest, a->W, a->E, a->U);
  SMX_REQUIRE(a->blank >= 0 && a->blank < a->V, "%s: bad blank=%d (V=%d)", what, a->blank, a->V);
  SMX_REQUIRE(a->act >= SMX_ACT_NONE && a->act <= SMX_ACT_RELU, "%s: bad activation %d", what, a->act);
  SMX_REQUIRE(a->state_beam == a->state_beam && a->expand_beam == a->expand_beam && a->lm_weight == a->lm_weight, "%s: a NaN beam width or LM weight", what);
  SMX_REQUIRE(a->enc && a->WihT && a->bias && a->Whh && a->Wproj && a->Wlin && a->cur_tok && a->h_in && a->c_in && a->h_out && a->c_out && a->pdec &&
                  a->z && a->state && a->done && a->overflow && a->expansions && a->frames && a->tokens && a->out_len && a->scores && a->sums && a->n_hyps,
              "%s: null pointer", what);
  SMX_REQUIRE(a->h_in != a->h_out && a->c_in != a->c_out, "%s: the staging rows in and out must be distinct", what);
  SMX_REQUIRE(a->ldw >= 4L * a->H && a->ld_t >= a->J && (a->T <= 1 || a->B <= 1 || a->ld_b >= a->J), "%s: bad strides", what);
  SMX_REQUIRE(a->lm_L >= 0 && a->lm_L <= 16, "%s: lm_L=%d outside [0, 16]", what, a->lm_L);
  if (a->lm_L > 0) {
    SMX_REQUIRE(a->lm_h_in && a->lm_c_in && a->lm_h_out && a->lm_c_out && a->lm_H >= 1, "%s: an LM (lm_L > 0) comes with its staged states", what);
    SMX_REQUIRE(a->lm_h_in != a->lm_h_out && a->lm_c_in != a->lm_c_out, "%s: the LM's staging rows in and out must be distinct", what);
  }
  if (!tbeam_shape_ok(a->H, a->J, a->V, a->W) || (a->lm_L > 0 && !lstm_h_ok(a->lm_H)))
    return fail(SMX_EUNSUPPORTED, "%s: H (and the LM's) must be a multiple of 32 in [32, %d], J a multiple of 64 in [64, %d], V in [3, %d], W in [2, %d] and below V; got "
                "H=%d J=%d V=%d W=%d lm_H=%d", what, LSTM_H_MAX, TBEAM_J_MAX, TBEAM_V_MAX, TBEAM_W_MAX, a->H, a->J, a->V, a->W, a->lm_H);
  if (tbeam_select_lds(a->V, a->W, a->E) > TBEAM_LDS_MAX)
    return fail(SMX_EUNSUPPORTED, "%s: the z row and the open list (W + max_expansions W entries) exceed the selection's LDS: V=%d W=%d max_expansions=%d", what, a->V,
                a->W, a->E);
  const size_t es = a->dtype == SMX_BF16 ? 2 : 4;
  if (!aligned16(a->enc) || !aligned16(a->Whh) || !aligned16(a->Wproj) || !aligned16(a->Wlin) || !aligned16(a->h_in) || !aligned16(a->h_out) ||
      !aligned16(a->c_in) || !aligned16(a->c_out) || !aligned16(a->pdec) || !aligned16(a->state) || (a->ld_b * es) % 16 != 0 || (a->ld_t * es) % 16 != 0 ||
      (a->lm_L > 0 && (!aligned16(a->lm_h_in) || !aligned16(a->lm_h_out) || !aligned16(a->lm_c_in) || !aligned16(a->lm_c_out))))
    return fail(SMX_EUNSUPPORTED, "%s: enc (and its strides), the weights, the staging rows and the state must be 16-byte aligned", what);
  *L = tbeam_layout((int)es, a->H, a->W, a->E, a->U, a->lm_L, a->lm_L > 0 ? a->lm_H : 0);
  return SMX_OK;
}

extern "C" size_t smx_tbeam_state_bytes(int dtype, int B, int H, int W, int max_expansions, int max_symbols, int lm_layers, int lm_H) {
  if ((dtype != SMX_F32 && dtype != SMX_BF16) || B < 1 || H < 1 || W < 1 || max_expansions < 1 || max_symbols < 1 || lm_layers < 0 || lm_H < 0) return 0;
  return (size_t)B * (size_t)tbeam_layout(dtype == SMX_BF16 ? 2 : 4, H, W, max_expansions, max_symbols, lm_layers, lm_layers ? lm_H : 0).total;
}

extern "C" int smx_tbeam_init(const smx_tbeam_args* a, void* stream) {
  TbLayout L;
  const int rc = tbeam_check("smx_tbeam_init", a, &L);
  if (rc != SMX_OK) return rc;
  dispatch_dtype(a->dtype, [&](auto tag) {
    using E = decltype(tag);
    hipLaunchKernelGGL(tbeam_init_kernel<E>, dim3(a->B), dim3(256), 0, STREAM, *a, L);
  });
  return check_launch("smx_tbeam_init");
}

extern "C" int smx_tbeam_step(const smx_tbeam_args* a, void* stream) {
  TbLayout L;
  const int rc = tbeam_check("smx_tbeam_step", a, &L);
  if (rc != SMX_OK) return rc;
  const int B = a->B, H = a->H, J = a->J;
  const size_t es = a->dtype == SMX_BF16 ? 2 : 4;
  const size_t lds = 16 * (size_t)(J + (a->dtype == SMX_BF16 ? 8 : 4)) * es;
  const dim3 pgrid(H / 16, (B + 15) / 16), jgrid(J / 64, (B + 15) / 16), lgrid((a->V + TBEAM_TILE_V - 1) / TBEAM_TILE_V, (B + 15) / 16);
  dispatch_dtype(a->dtype, [&](auto tag) {
    using E = decltype(tag);
    hipLaunchKernelGGL(tbeam_pred_kernel<E>, pgrid, dim3(256), 0, STREAM, *a);
    hipLaunchKernelGGL(tbeam_proj_kernel<E>, jgrid, dim3(256), 0, STREAM, (const E*)a->h_out, (const E*)a->Wproj, (E*)a->pdec, B, H, J);
    hipLaunchKernelGGL(tbeam_logits_kernel<E>, lgrid, dim3(256), lds, STREAM, *a);
  });
  return check_launch("smx_tbeam_step");
}

template <bool STREAMED>
static int tbeam_select_launch(const char* what, const smx_tbeam_args* a, int32_t* stream_frames, void* stream) {
  TbLayout L;
  const int rc = tbeam_check(what, a, &L);
  if (rc != SMX_OK) return rc;
  SMX_REQUIRE((a->lm_L > 0) == (a->lm_logits != nullptr) && (!a->lm_logits || a->ld_lm >= a->V), "%s: lm_logits (ld_lm >= V) if and only if lm_L > 0", what);
  if (a->lm_logits && (reinterpret_cast<uintptr_t>(a->lm_logits) & 3u)) return fail(SMX_EUNSUPPORTED, "%s: lm_logits must be 4-byte aligned", what);
  const size_t lds = tbeam_select_lds(a->V, a->W, a->E);
  dispatch_dtype(a->dtype, [&](auto tag) {
    using E = decltype(tag);
    hipLaunchKernelGGL((tbeam_select_kernel<E, STREAMED>), dim3(a->B), dim3(256), lds, STREAM, *a, L, stream_frames);
  });
  return check_launch(what);
}

extern "C" int smx_tbeam_select(const smx_tbeam_args* a, void* stream) {
  return tbeam_select_launch<false>("smx_tbeam_select", a, nullptr, stream);
}

// a stream's entries read `lengths` and `stream_frames` on the device: both must be there (checked before tbeam_check, which allows
// lengths == NULL for the whole search)
static int tbeam_stream_check(const char* what, const smx_tbeam_args* a, const int32_t* stream_frames) {
  SMX_REQUIRE(a, "%s: null argument struct", what);
  SMX_REQUIRE(a->lengths && stream_frames && a->state, "%s: a stream needs lengths (the chunk's frames per slot), stream_frames and state", what);
  return SMX_OK;
}

extern "C" int smx_tbeam_select_stream(const smx_tbeam_args* a, int32_t* stream_frames, void* stream) {
  const int rc = tbeam_stream_check("smx_tbeam_select_stream", a, stream_frames);
  if (rc != SMX_OK) return rc;
  return tbeam_select_launch<true>("smx_tbeam_select_stream", a, stream_frames, stream);
}

extern "C" int smx_tbeam_resume(const smx_tbeam_args* a, const uint8_t* start, int32_t* stream_frames, void* stream) {
  int rc = tbeam_stream_check("smx_tbeam_resume", a, stream_frames);
  if (rc != SMX_OK) return rc;
  SMX_REQUIRE(start, "smx_tbeam_resume: null start vector");
  TbLayout L;
  rc = tbeam_check("smx_tbeam_resume", a, &L);
  if (rc != SMX_OK) return rc;
  dispatch_dtype(a->dtype, [&](auto tag) {
    using E = decltype(tag);
    hipLaunchKernelGGL(tbeam_resume_kernel<E>, dim3(a->B), dim3(256), 0, STREAM, *a, L, start, stream_frames);
  });
  return check_launch("smx_tbeam_resume");
}
