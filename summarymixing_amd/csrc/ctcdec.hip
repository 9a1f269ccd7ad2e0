// ctcdec.hip — CTC greedy (best-path) decoding of the encoder's CTC head (recipe keys `ctc_lin` 512 -> 5000 in the Branchformer
// recipes, `proj_ctc` 640 -> 1000 in the transducer recipes; upstream: speechbrain.decoders.ctc.ctc_greedy_decode /
// filter_ctc_output), gfx950 only: row arg-max, collapse repeats, drop blanks.  Three pieces, all on the caller's stream, none of
// which talks to the host:
//   a. ctc_best_path_kernel   stored scores -> per row (lowest index of the maximum, max - logsumexp).  One wave per row, 16-byte
//                             groups anchored at column 0 plus an element tail (row_scan.h), an online (max, sum exp) pair per
//                             lane.
//   b. ctc_head_kernel        z = X W^T + bias on the 128 x 128 MFMA tile of head_tile.h; the epilogue keeps,
//                             per (row, column tile), the tile's max, its first arg-max and sum exp(z - max) - the partial layout of
//                             greedy.hip.  z is never stored.  ctc_head_reduce_kernel folds a row's tiles in ascending order.
//   c. ctc_collapse_kernel    one wave per utterance: frame t emits iff its token is neither the blank, nor negative, nor the
//                             previous frame's token; a ballot and a prefix popcount per 64 frames place the emissions.  The state
//                             (previous token, frames seen, tokens emitted, score) is carried between calls.
// A NaN never wins a comparison; a token is only ever a value, never an index.  Every sum has a fixed order and nothing is atomic:
// two runs agree bit for bit.
#include "head_tile.h"
#include "row_scan.h"

#include <limits.h>

namespace smx {

static constexpr int CD_NO_TOKEN = INT_MIN;             // `prev` before the first frame: equals no token (not even the -1 of a NaN row)

// what one lane has seen of its row: the running arg-max (bv, bi), the online softmax pair (m, s) over the entries that are
// numbers, and whether any entry was a NaN
struct CdRow {
  float bv; int bi;
  float m, s;
  int nan;
};

template <int N>
__device__ __forceinline__ void cd_row_take(CdRow& a, const float (&x)[N], int c0) {
  float gm = NEG_INF;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    argmax_take(a.bv, a.bi, x[j], c0 + j);
    if (x[j] > gm) gm = x[j];
    a.nan |= __builtin_isnan(x[j]) ? 1 : 0;
  }
  if (gm > a.m) {                                       // one rescale per group; a.s is 0 while a.m is -inf
    a.s = lse_rescale(a.s, a.m, gm);
    a.m = gm;
  }
  if (a.m != NEG_INF) {
    // -ffast-math lets the compiler pick the tree of this sum.  The order below (a.s first, then the columns in turn) is the one the
    // kernel had before it moved onto row_scan; it was pinned against those bits (tests/test_head_bits_gpu.py), and the pragma holds
    // the compiler to it.  seqloss.hip's row_take has no pragma on purpose: its pinned bits are those of the compiler's own tree.
#pragma clang fp reassociate(off)
#pragma unroll
    for (int j = 0; j < N; ++j) a.s += __builtin_isnan(x[j]) ? 0.f : expf(x[j] - a.m);
  }
}

// grid = ceil(N / 4), block = 256: wave w of a block owns row 4 blockIdx.x + w and reads it once (row_scan).
template <typename T>
__global__ __launch_bounds__(256) void ctc_best_path_kernel(const T* __restrict__ X, long ldx, int N, int V, int32_t* __restrict__ tok,
                                                            float* __restrict__ lp) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const T* x = X + row * ldx;
  CdRow a = {NEG_INF, INT_MAX, NEG_INF, 0.f, 0};
  row_scan(x, V, lane, [&](const auto& g, int c0) { cd_row_take(a, g, c0); });
  // across the wave (butterflies: every lane ends with the same bits)
  float bv = a.bv;
  int bi = a.bi, nan = a.nan;
  argmax_meet<64>(bv, bi);
  const float m = wave_max(a.m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nan |= __shfl_xor(nan, o, 64);
  const float s = wave_sum(lse_rescale(a.s, a.m, m));
  if (lane != 0) return;
  tok[row] = bi == INT_MAX ? -1 : bi;                   // (no entry is a number: every comparison failed)
  lp[row] = nan ? __builtin_nanf("") : -logf(s);        // max - logsumexp = -log sum exp(z - max)
}

// ---- fused head (head_tile.h).  Columns beyond V re-read column V - 1 in the main loop; the epilogue sets them to -inf. ----
// part[n][ct] = (max, first arg-max, sum exp(z - max)) of row n over the valid columns of column tile ct.  A thread walks its 32
// columns of a row in ascending order, then the two lane halves and the two waves that share the row meet in a fixed order.
template <typename T>
__global__ __launch_bounds__(256, 2) void ctc_head_kernel(const T* __restrict__ X, long ldx, const T* __restrict__ W,
                                                          const float* __restrict__ bias, int N, int K, int V, int nct,
                                                          float* __restrict__ pmax, int* __restrict__ parg, float* __restrict__ psum) {
  __shared__ __attribute__((aligned(16))) char smem[2 * HeadTile<T>::OP_BYTES];
  __shared__ float sbias[HEAD_TILE];
  __shared__ ArgLseStat red[HEAD_TILE];
  const int ct = blockIdx.x % nct, rt = blockIdx.x / nct;
  const int n0 = rt * HEAD_TILE, v0 = ct * HEAD_TILE;
  const int t = threadIdx.x, wv = (t >> 6) & 1, hi = (t >> 5) & 1;
  if (t < HEAD_TILE) sbias[t] = (bias && v0 + t < V) ? bias[v0 + t] : 0.f;
  f32x16 acc[2][2];
  head_mainloop<T>(X, ldx, W, N, V, K, n0, v0, smem, acc);    // (its barriers publish sbias)
  auto thread_stat = [&](int j) __attribute__((always_inline)) -> ArgLseStat {
    float mx = NEG_INF;
    int kx = INT_MAX;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int vl = head_col(wv, i, r, hi), v = v0 + vl;
        const float z = v < V ? acc[i][j][r] + sbias[vl] : NEG_INF;             // columns beyond V: -inf, not the clamped column's value
        acc[i][j][r] = z;
        if (v < V) argmax_take(mx, kx, z, v);
      }
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float z = acc[i][j][r];
        if (v0 + head_col(wv, i, r, hi) < V) sm += __builtin_isnan(z) ? z : (mx == NEG_INF ? 0.f : expf(z - mx));   // a NaN logit makes the row's lp a NaN
      }
    return {mx, kx, sm};
  };
  head_row_meet(red, thread_stat, [&](int nl, const ArgLseStat& r) {
    const int n = n0 + nl;
    if (n >= N) return;
    const long o = (long)n * nct + ct;
    pmax[o] = r.m;
    parg[o] = r.k;
    psum[o] = r.s;
  });
}

// one thread per row: the tiles in ascending order (a tie keeps the lower column)
__global__ __launch_bounds__(256) void ctc_head_reduce_kernel(const float* __restrict__ pmax, const int* __restrict__ parg,
                                                              const float* __restrict__ psum, int nct, int N, int V,
                                                              int32_t* __restrict__ tok, float* __restrict__ lp) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const long o = (long)n * nct;
  float M = NEG_INF;
  int k = INT_MAX;
  for (int c = 0; c < nct; ++c) argmax_take(M, k, pmax[o + c], parg[o + c]);
  float S = 0.f;
  int nan = 0;
  for (int c = 0; c < nct; ++c) {
    const float ps = psum[o + c];
    nan |= __builtin_isnan(ps) ? 1 : 0;
    S += __builtin_isnan(ps) ? 0.f : lse_rescale(ps, pmax[o + c], M);
  }
  tok[n] = (k >= 0 && k < V) ? k : -1;
  lp[n] = nan ? __builtin_nanf("") : -logf(S);
}

// grid = B, block = 64: one wave per utterance.  64 frames at a time: a ballot of the emitting frames, the popcount of the lanes
// below gives each its place behind the running count.  The score is one fp32 chain strictly in frame order (the left comb: the one
// fixed tree for which a stream cut into chunks, whose carried score is an fp32, sums to the same bits as the whole).
__global__ __launch_bounds__(64) void ctc_collapse_kernel(smx_ctc_collapse_args a) {
  __shared__ float s_lp[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool reset = a.start && a.start[b];
  int prev = reset ? CD_NO_TOKEN : a.prev[b];
  int seen = reset ? 0 : a.seen[b];
  int n = reset ? 0 : a.n_tok[b];
  float score = reset ? 0.f : a.score[b];
  n = max(n, 0);
  const int L = a.in_len ? min(max(a.in_len[b], 0), a.T) : a.T;
  const int32_t* tok = a.tok + (long)b * a.ld;
  const float* lp = a.lp + (long)b * a.ld;
  int32_t* tokens = a.tokens + (long)b * a.cap;
  int32_t* frames = a.frames + (long)b * a.cap;
  for (int c0 = 0; c0 < L; c0 += 64) {
    const int t = c0 + lane;
    const bool live = t < L;
    const int k = live ? tok[t] : a.blank;
    const int pk = !live ? a.blank : (t == 0 ? prev : tok[t - 1]);
    const bool emit = live && k != a.blank && k >= 0 && k != pk;
    const unsigned long long mask = __ballot(emit);
    const long pos = (long)n + __popcll(mask & ((1ull << lane) - 1ull));
    if (emit && pos < a.cap) { tokens[pos] = k; frames[pos] = seen + t; }    // (an emission at or beyond cap is counted, not stored)
    const int add = __popcll(mask);
    n = add > INT_MAX - n ? INT_MAX : n + add;
    __syncthreads();                                     // the previous chunk's chain has been read
    s_lp[lane] = live ? lp[t] : 0.f;
    __syncthreads();
    const int cnt = min(64, L - c0);
    {
#pragma clang fp reassociate(off)
      for (int i = 0; i < cnt; ++i) score = score + s_lp[i];                  // every lane walks the same chain
    }
  }
  if (L > 0) prev = tok[L - 1];
  for (long i = (long)n + lane; i < a.cap; i += 64) { tokens[i] = -1; frames[i] = -1; }
  if (lane == 0) {
    a.prev[b] = prev;
    a.seen[b] = seen + L;
    a.n_tok[b] = n;
    a.score[b] = score;
  }
}

static int cd_tiles(int V) { return (V + HEAD_TILE - 1) / HEAD_TILE; }
static bool cd_head_shape_ok(int K, int V) { return K >= 64 && K % 64 == 0 && V >= 2; }

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_ctc_best_path(int dtype, const void* X, int64_t ldx, int N, int V, int32_t* tok, float* lp, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_ctc_best_path: dtype %d", dtype);
  SMX_REQUIRE(X && tok && lp, "smx_ctc_best_path: null pointer");
  SMX_REQUIRE(N >= 0 && V >= 1 && ldx >= V, "smx_ctc_best_path: bad sizes N=%d V=%d ldx=%lld", N, V, (long long)ldx);
  if (N == 0) return SMX_OK;
  const dim3 grid((unsigned)(((long)N + 3) / 4));
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(ctc_best_path_kernel<T>, grid, dim3(256), 0, STREAM, (const T*)X, (long)ldx, N, V, tok, lp);
  });
  return check_launch("smx_ctc_best_path");
}

extern "C" int smx_ctc_head_ok(int dtype, int K, int V) {
  return (dtype == SMX_F32 || dtype == SMX_BF16) && cd_head_shape_ok(K, V) ? 1 : 0;
}

extern "C" size_t smx_ctc_head_workspace(int N, int V) {
  if (N <= 0 || V <= 0) return 0;
  return (size_t)N * cd_tiles(V) * 12;                   // [max (N, NT) fp32][arg-max (N, NT) int32][sum exp (N, NT) fp32]
}

extern "C" int smx_ctc_head_best_path(int dtype, const void* X, int64_t ldx, const void* W, const float* bias, int N, int K, int V,
                                      int32_t* tok, float* lp, void* workspace, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_ctc_head_best_path: dtype %d", dtype);
  SMX_REQUIRE(N >= 0 && K >= 1 && V >= 1 && ldx >= K, "smx_ctc_head_best_path: bad sizes N=%d K=%d V=%d ldx=%lld", N, K, V, (long long)ldx);
  if (!cd_head_shape_ok(K, V))
    return fail(SMX_EUNSUPPORTED, "smx_ctc_head_best_path: K must be a multiple of 64 and V >= 2, got K=%d V=%d", K, V);
  SMX_REQUIRE(X && W && tok && lp && workspace, "smx_ctc_head_best_path: null pointer");
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  if (!aligned16(X) || !aligned16(W) || !aligned16(workspace) || (ldx * es) % 16 != 0)
    return fail(SMX_EUNSUPPORTED, "smx_ctc_head_best_path: X (and its leading dimension), W and the workspace must be 16-byte aligned");
  const int nct = cd_tiles(V);
  const long nrt = ((long)N + HEAD_TILE - 1) / HEAD_TILE;
  if ((long)N * nct >= (1L << 31) || nrt * nct >= (1L << 31))
    return fail(SMX_EUNSUPPORTED, "smx_ctc_head_best_path: N = %d rows x %d column tiles is too many", N, nct);
  if (N == 0) return SMX_OK;
  float* pmax = reinterpret_cast<float*>(workspace);
  int* parg = reinterpret_cast<int*>(pmax + (size_t)N * nct);
  float* psum = reinterpret_cast<float*>(parg + (size_t)N * nct);
  const dim3 grid((unsigned)(nrt * nct));
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(ctc_head_kernel<T>, grid, dim3(256), 0, STREAM, (const T*)X, (long)ldx, (const T*)W, bias, N, K, V, nct, pmax, parg, psum);
  });
  hipLaunchKernelGGL(ctc_head_reduce_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, STREAM, pmax, parg, psum, nct, N, V, tok, lp);
  return check_launch("smx_ctc_head_best_path");
}

extern "C" int smx_ctc_collapse(const smx_ctc_collapse_args* a, void* stream) {
  SMX_REQUIRE(a, "smx_ctc_collapse: null descriptor");
  SMX_REQUIRE(a->B >= 0 && a->T >= 0 && a->cap >= 0 && a->ld >= a->T, "smx_ctc_collapse: bad sizes B=%d T=%d cap=%d ld=%lld", a->B, a->T,
              a->cap, (long long)a->ld);
  SMX_REQUIRE(a->blank >= 0, "smx_ctc_collapse: blank %d", a->blank);
  SMX_REQUIRE(a->prev && a->seen && a->n_tok && a->score && (a->cap == 0 || (a->tokens && a->frames)) && (a->T == 0 || (a->tok && a->lp)),
              "smx_ctc_collapse: null pointer");
  if (a->B == 0) return SMX_OK;
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3(a->B), dim3(64), 0, STREAM, *a);
  return check_launch("smx_ctc_collapse");
}
