// greedy.hip — greedy transducer decoding (recipe key `Greedysearcher`: speechbrain.decoders.transducer.TransducerBeamSearcher with
// beam_size 1, …transducer.yaml:375-381), gfx950 only.  At most one symbol per frame.
//
// Three launches per frame, always the same three whatever the data, all on the caller's stream; the frame loop is inside
// smx_greedy_decode and nothing in it talks to the host (a captured call is a plain chain of 3 T + 1 kernels):
//   1. greedy_logits_kernel  a = act(enc[b,t,:] + pdec[b,:]) for 16 rows in LDS (fp32 sum and activation, rounded to dtype as the
//                            training joint stores H), times a 128-column slice of W_lin on the MFMA; per (row, tile) the tile's
//                            max, its first argmax and sum exp(z - max).  z is never stored.
//   2. greedy_step_kernel    every workgroup re-reduces the V / 128 partials of its 16 rows (k = argmax, lowest index on a tie; log-prob
//                            = -log sum exp(z - z[k])), then the LSTM step of lstm.hip masked per row, built from the same pieces of
//                            lstm_tile.h (gate_tiles, onehot_gate_input with keep = 1, lstm_cell): rows that emit take a new (h, c)
//                            - bit for bit what lstm.hip gives when the hypothesis is fed back through its one-hot route - and
//                            the others copy h.  h is double-buffered (other workgroups read h_prev in the same launch).  The workgroup of hidden tile 0 appends (token, frame,
//                            log-prob) and counts the frame.
//   3. greedy_proj_kernel    pdec = h W_proj^T for all rows (idempotent for the rows that did not emit: no mask).
// Batch rows beyond B of the last tile re-read row B - 1 and are never stored.  A row's values depend on that row alone: the
// geometry and the K order per row are fixed, every sum has a fixed order and nothing is atomic.
#include "lstm_tile.h"

#include <limits.h>

#include <algorithm>

namespace smx {

static constexpr int GREEDY_TILE_V = 128;
static constexpr int GREEDY_J_MAX = 832;          // 16 rows of a (fp32: J + 4 floats each) and the 16 x 129 logit tile stay below 64 KB of LDS
static bool greedy_shape_ok(int H, int J, int V) { return lstm_h_ok(H) && J >= 64 && J <= GREEDY_J_MAX && J % 64 == 0 && V >= 2; }
static int greedy_tiles(int V) { return (V + GREEDY_TILE_V - 1) / GREEDY_TILE_V; }

template <typename T> struct GreedyPad;           // a's LDS rows are 16 bytes longer than J elements (the rows start in different banks)
template <> struct GreedyPad<float> { static constexpr int value = 4; };
template <> struct GreedyPad<bf16_t> { static constexpr int value = 8; };

struct GreedyLogits {
  const void* enc; long ld_b, ld_t;     // enc[b,t,:] = enc + b ld_b + t ld_t
  const void* pdec;                     // (B, J)
  const void* Wlin;                     // (V, J)
  const float* blin;                    // (V) or null
  float* pmax; int* parg; float* psum;  // (rows, NT) partials
  int t, B, J, V, NT, act;
};

template <typename T>
__global__ __launch_bounds__(256) void greedy_logits_kernel(GreedyLogits s) {
  extern __shared__ __attribute__((aligned(16))) char greedy_lds[];
  __shared__ float zt[16][GREEDY_TILE_V + 1];
  constexpr int PAD = GreedyPad<T>::value;
  const int J = s.J, lda = J + PAD, v0 = blockIdx.x * GREEDY_TILE_V, b0 = blockIdx.y * 16;
  T* a = reinterpret_cast<T*>(greedy_lds);
  const T* enc = reinterpret_cast<const T*>(s.enc);
  const T* pdec = reinterpret_cast<const T*>(s.pdec);
  dispatch_act(s.act, [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    for (int idx = threadIdx.x * 4; idx < 16 * J; idx += 1024) {
      const int row = idx / J, col = idx - row * J;
      const int b = min(b0 + row, s.B - 1);
      float e[4], p[4];
      load4(enc + (long)b * s.ld_b + (long)s.t * s.ld_t + col, e);
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
    for (int i = 0; i < 4; ++i) zt[q * 4 + i][c0 + r] = v < s.V ? acc[i] + bias : NEG_INF;
  }
  __syncthreads();
  // 16 threads per row, 8 consecutive columns each, then the 16 meet
  const int bb = threadIdx.x >> 4, jj = threadIdx.x & 15;
  float m = zt[bb][jj * 8];
  int k = jj * 8;
#pragma unroll
  for (int i = 1; i < 8; ++i) {
    const float z = zt[bb][jj * 8 + i];
    if (z > m) { m = z; k = jj * 8 + i; }
  }
  argmax_meet<16>(m, k);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) sum += __expf(zt[bb][jj * 8 + i] - m);
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 16);
  const int b = b0 + bb;
  if (jj == 0 && b < s.B) {
    const long o = (long)b * s.NT + blockIdx.x;
    s.pmax[o] = m; s.parg[o] = v0 + k; s.psum[o] = sum;
  }
}

struct GreedyStep {
  const float* pmax; const int* parg; const float* psum;    // (rows, NT); unused at the start step
  const int32_t* in_len;                // (B) frames of this call's enc that count per row, or null: all
  const void* WihT; long ldw;           // (V - 1, 4H) = W_ih^T
  const float* bias;                    // (4H) = b_ih + b_hh
  const void* Whh;                      // (4H, H)
  const void* hp;                       // (B, H) h before this frame (null at the start step: zeros)
  void* hn;                             // (B, H) h after it (the other half of the double buffer)
  float* c;                             // (B, H) fp32, updated in place (thread (b, j) is its only reader and writer)
  int32_t* seen;                        // (B) frames decoded so far per row
  int32_t* tokens; int32_t* frames; long ld_tok;            // (B, T) each
  int32_t* n_tok; float* logp;          // (B)
  int t, B, H, V, NT, blank, start;
};

template <typename T>
__global__ __launch_bounds__(256) void greedy_step_kernel(GreedyStep s) {
  __shared__ float red[4][16][17];
  __shared__ int s_k[16], s_emit[16], s_live[16];
  __shared__ float s_lp[16];
  const int H = s.H, j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int bb = threadIdx.x >> 4, jj = threadIdx.x & 15, b = b0 + bb, j = j0 + jj;
  if (s.start) {
    if (jj == 0) { s_k[bb] = s.blank; s_emit[bb] = 1; s_live[bb] = 0; s_lp[bb] = 0.f; }
  } else {
    // select: the NT partials of row b, 16 threads per row in ascending tiles, then the 16 meet
    const long o = (long)min(b, s.B - 1) * s.NT;
    float m = NEG_INF;
    int k = INT_MAX;
    for (int t = jj; t < s.NT; t += 16) {
      const float om = s.pmax[o + t];
      if (t == jj || om > m) { m = om; k = s.parg[o + t]; }                  // (tiles ascend: a tie keeps the lower column)
    }
    argmax_meet<16>(m, k);
    float sum = 0.f;
    for (int t = jj; t < s.NT; t += 16) sum += s.psum[o + t] * __expf(s.pmax[o + t] - m);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 16);
    if (jj == 0) {
      const int live = s.in_len ? (s.t < s.in_len[min(b, s.B - 1)]) : 1;
      s_k[bb] = k;
      s_live[bb] = live;
      s_emit[bb] = live && k >= 0 && k < s.V && k != s.blank;                // (k outside [0, V): only if every logit is a NaN)
      s_lp[bb] = -__logf(sum);                                                // z[k] - logsumexp(z), z[k] being the maximum
    }
  }
  __syncthreads();
  int any = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) any |= s_emit[i];
  const T* hp = reinterpret_cast<const T*>(s.hp);
  gate_tiles(red, any ? hp : nullptr, (long)H, s.Whh, H, s.B, b0, j0);        // (a frame of blanks reads no W_hh)
  if (b >= s.B) return;
  T* hn = reinterpret_cast<T*>(s.hn);
  const int k = s_k[bb];
  if (s_emit[bb]) {
    const int col = onehot_col(k, s.V, s.blank);
    float z[4], g[4], c;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float wx = col >= 0 ? to_f32(reinterpret_cast<const T*>(s.WihT)[(long)col * s.ldw + i * H + j]) : 0.f;
      z[i] = red[i][bb][jj] + onehot_gate_input(1.f, wx, s.bias[i * H + j]);
    }
    hn[(long)b * H + j] = from_f32<T>(lstm_cell(z, s.start ? 0.f : s.c[(long)b * H + j], g, c));
    s.c[(long)b * H + j] = c;
  } else {
    hn[(long)b * H + j] = hp[(long)b * H + j];
  }
  if (blockIdx.x == 0 && jj == 0) {
    if (s.start) {
      s.seen[b] = 0;
    } else if (s_live[bb]) {
      const int f = s.seen[b];
      s.seen[b] = f + 1;
      if (s_emit[bb]) {
        const int n = s.n_tok[b];
        s.tokens[(long)b * s.ld_tok + n] = k;
        s.frames[(long)b * s.ld_tok + n] = f;
        s.logp[b] += s_lp[bb];
        s.n_tok[b] = n + 1;
      }
    }
  }
}

// pdec (B, J) = h (B, H) . W_proj (J, H)^T: a workgroup owns 16 rows x 64 columns, one 16-column tile per wave
template <typename T>
__global__ __launch_bounds__(256) void greedy_proj_kernel(const T* __restrict__ h, const T* __restrict__ Wp, T* __restrict__ pdec, int B, int H, int J) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int j0 = blockIdx.x * 64 + 16 * w, b0 = blockIdx.y * 16;
  const lstm_f32x4 acc = tile_dot(h + (long)min(b0 + r, B - 1) * H, Wp + (long)(j0 + r) * H, H, q);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = b0 + q * 4 + i;
    if (b < B) pdec[(long)b * J + j0 + r] = from_f32<T>(acc[i]);
  }
}

// the call's outputs start empty (tokens / frames -1, n_tok 0) and, for an odd T, h moves to the double buffer's other half so
// that the last frame writes the state's own buffer
template <typename T>
__global__ __launch_bounds__(256) void greedy_begin_kernel(int32_t* tokens, int32_t* frames, int32_t* n_tok, const T* h, T* h_alt,
                                                          long n_out, int B, long n_h) {
  const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  for (long i = i0; i < n_out; i += step) { tokens[i] = -1; frames[i] = -1; }
  for (long i = i0; i < B; i += step) n_tok[i] = 0;
  if (h_alt)
    for (long i = i0; i < n_h; i += step) h_alt[i] = h[i];
}

template <typename T>
static void launch_proj(const void* h, const void* Wp, void* pdec, int B, int H, int J, hipStream_t st) {
  hipLaunchKernelGGL(greedy_proj_kernel<T>, dim3(J / 64, (B + 15) / 16), dim3(256), 0, st, (const T*)h, (const T*)Wp, (T*)pdec, B, H, J);
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_greedy_ok(int dtype, int H, int J, int V) {
  return (dtype == SMX_F32 || dtype == SMX_BF16) && greedy_shape_ok(H, J, V) ? 1 : 0;
}

extern "C" size_t smx_greedy_workspace(int B, int V) {
  if (B <= 0 || V <= 0) return 0;
  return (size_t)B * greedy_tiles(V) * 12;
}

static int greedy_check(const char* what, int dtype, int B, int H, int J, int V) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "%s: bad dtype %d", what, dtype);
  SMX_REQUIRE(B >= 0 && B <= 65535 * 16 && H >= 1 && J >= 1 && V >= 1, "%s: bad sizes B=%d H=%d J=%d V=%d", what, B, H, J, V);
  if (!greedy_shape_ok(H, J, V))
    return fail(SMX_EUNSUPPORTED, "%s: H must be a multiple of 32 in [32, %d], J a multiple of 64 in [64, %d] and V >= 2, got H=%d J=%d V=%d",
                what, LSTM_H_MAX, GREEDY_J_MAX, H, J, V);
  return SMX_OK;
}

extern "C" int smx_greedy_start(int dtype, const float* bias, const void* Wproj, void* h, float* c, void* pdec, int32_t* frames_seen,
                                int B, int H, int J, void* stream) {
  const int rc = greedy_check("smx_greedy_start", dtype, B, H, J, 2);
  if (rc != SMX_OK) return rc;
  SMX_REQUIRE(bias && Wproj && h && c && pdec && frames_seen, "smx_greedy_start: null pointer");
  if (!aligned16(Wproj) || !aligned16(h) || !aligned16(pdec)) return fail(SMX_EUNSUPPORTED, "smx_greedy_start: W_proj, h and pdec must be 16-byte aligned");
  if (B == 0) return SMX_OK;
  GreedyStep s;
  memset(&s, 0, sizeof(s));
  s.bias = bias; s.hn = h; s.c = c; s.seen = frames_seen;
  s.B = B; s.H = H; s.V = 2; s.blank = 0; s.start = 1;
  const dim3 grid(H / 16, (B + 15) / 16);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(greedy_step_kernel<T>, grid, dim3(256), 0, STREAM, s);
    launch_proj<T>(h, Wproj, pdec, B, H, J, STREAM);
  });
  return check_launch("smx_greedy_start");
}

extern "C" int smx_greedy_decode(int dtype, const void* enc, int64_t ld_b, int64_t ld_t, const int32_t* in_len, const void* WihT, int64_t ldw,
                                 const float* bias, const void* Whh, const void* Wproj, const void* Wlin, const float* blin, void* h,
                                 void* h_alt, float* c, void* pdec, int32_t* frames_seen, int32_t* tokens, int32_t* frames, int32_t* n_tok,
                                 float* logp, int B, int T, int H, int J, int V, int act, int blank, void* workspace, void* stream) {
  const int rc = greedy_check("smx_greedy_decode", dtype, B, H, J, V);
  if (rc != SMX_OK) return rc;
  SMX_REQUIRE(T >= 0 && blank >= 0 && blank < V, "smx_greedy_decode: bad T=%d or blank=%d (V=%d)", T, blank, V);
  SMX_REQUIRE(act >= SMX_ACT_NONE && act <= SMX_ACT_RELU, "smx_greedy_decode: bad activation %d", act);
  SMX_REQUIRE(enc && WihT && bias && Whh && Wproj && Wlin && h && h_alt && c && pdec && frames_seen && tokens && frames && n_tok && logp && workspace,
              "smx_greedy_decode: null pointer");
  SMX_REQUIRE(h != h_alt && ldw >= 4L * H && ld_t >= J && (T <= 1 || B <= 1 || ld_b >= J), "smx_greedy_decode: bad strides");
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  if (!aligned16(enc) || !aligned16(Whh) || !aligned16(Wproj) || !aligned16(Wlin) || !aligned16(h) || !aligned16(h_alt) || !aligned16(pdec) ||
      (ld_b * es) % 16 != 0 || (ld_t * es) % 16 != 0 || !aligned16(workspace))
    return fail(SMX_EUNSUPPORTED, "smx_greedy_decode: enc (and its strides), the weights, h and pdec must be 16-byte aligned");
  if (B == 0) return SMX_OK;
  const int NT = greedy_tiles(V);
  float* pmax = reinterpret_cast<float*>(workspace);
  int* parg = reinterpret_cast<int*>(pmax + (size_t)B * NT);
  float* psum = reinterpret_cast<float*>(parg + (size_t)B * NT);
  const long n_out = (long)B * T, n_h = (long)B * H;
  const int nblk = (int)std::min<long>(1024, (std::max(n_out, n_h) + 255) / 256 + 1);
  void* h_first = (T & 1) ? h_alt : nullptr;
  GreedyLogits g;
  g.enc = enc; g.ld_b = ld_b; g.ld_t = ld_t; g.pdec = pdec; g.Wlin = Wlin; g.blin = blin;
  g.pmax = pmax; g.parg = parg; g.psum = psum;
  g.B = B; g.J = J; g.V = V; g.NT = NT; g.act = act;
  GreedyStep s;
  memset(&s, 0, sizeof(s));
  s.pmax = pmax; s.parg = parg; s.psum = psum; s.in_len = in_len;
  s.WihT = WihT; s.ldw = ldw; s.bias = bias; s.Whh = Whh; s.c = c; s.seen = frames_seen;
  s.tokens = tokens; s.frames = frames; s.ld_tok = T; s.n_tok = n_tok; s.logp = logp;
  s.B = B; s.H = H; s.V = V; s.NT = NT; s.blank = blank; s.start = 0;
  const dim3 lgrid(NT, (B + 15) / 16), sgrid(H / 16, (B + 15) / 16);
  const size_t lds = 16 * (size_t)(J + (dtype == SMX_BF16 ? 8 : 4)) * es;
  dispatch_dtype(dtype, [&](auto tag) {
    using E = decltype(tag);                                                   // (T is the frame count here)
    hipLaunchKernelGGL(greedy_begin_kernel<E>, dim3(nblk), dim3(256), 0, STREAM, tokens, frames, n_tok, (const E*)h, (E*)h_first, n_out, B, n_h);
    for (int t = 0; t < T; ++t) {
      // frame t reads the half that frame t - 1 wrote; the parity is chosen so that frame T - 1 writes h
      const bool from_h = ((T - t) & 1) == 0;
      g.t = t; s.t = t;
      s.hp = from_h ? h : h_alt;
      s.hn = from_h ? h_alt : h;
      hipLaunchKernelGGL(greedy_logits_kernel<E>, lgrid, dim3(256), lds, STREAM, g);
      hipLaunchKernelGGL(greedy_step_kernel<E>, sgrid, dim3(256), 0, STREAM, s);
      launch_proj<E>(s.hn, Wproj, pdec, B, H, J, STREAM);
    }
  });
  return check_launch("smx_greedy_decode");
}
