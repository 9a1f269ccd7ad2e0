// ctcdec.hip — CTC greedy (best-path) decoding of the encoder's CTC head (recipe keys `ctc_lin` 512 -> 5000 in the Branchformer
// recipes, `proj_ctc` 640 -> 1000 in the transducer recipes; upstream: speechbrain.decoders.ctc.ctc_greedy_decode /
// filter_ctc_output), gfx950 only: row arg-max, collapse repeats, drop blanks.  Three pieces, all on the caller's stream, none of
// which talks to the host:
//   a. ctc_best_path_kernel   stored scores -> per row (lowest index of the maximum, max - logsumexp).  One wave per row, 16-byte
//                             groups anchored at column 0 plus an element tail, an online (max, sum exp) pair per lane: the row
//                             geometry of seqloss.hip.
//   b. ctc_head_kernel        z = X W^T + bias on the 128 x 128 MFMA tile of transducer.hip's tj_stats_kernel; the epilogue keeps,
//                             per (row, column tile), the tile's max, its first arg-max and sum exp(z - max) - the partial layout of
//                             greedy.hip.  z is never stored.  ctc_head_reduce_kernel folds a row's tiles in ascending order.
//   c. ctc_collapse_kernel    one wave per utterance: frame t emits iff its token is neither the blank, nor negative, nor the
//                             previous frame's token; a ballot and a prefix popcount per 64 frames place the emissions.  The state
//                             (previous token, frames seen, tokens emitted, score) is carried between calls.
// A NaN never wins a comparison; a token is only ever a value, never an index.  Every sum has a fixed order and nothing is atomic:
// two runs agree bit for bit.
#include "gemm_common.h"

#include <limits.h>

namespace smx {

static constexpr float CD_NEG_INF = -__builtin_inff();
static constexpr int CD_TILE = 128;                     // rows and columns of a fused-head tile
static constexpr int CD_NO_TOKEN = INT_MIN;             // `prev` before the first frame: equals no token (not even the -1 of a NaN row)
static constexpr int CD_DEPTH = 4;                      // 16-byte groups a lane has in flight (row pass)

// (value, column) meets (value, column): the higher value, the lower column among equals; a NaN on either side never wins
__device__ __forceinline__ void cd_take(float& m, int& k, float om, int ok) {
  if (om > m || (om == m && ok < k)) { m = om; k = ok; }
}
// sum exp(. - a) and sum exp(. - b) -> sum exp(. - max(a, b)); an empty side (max -inf) contributes nothing
__device__ __forceinline__ float cd_rescale(float s, float m, float M) { return m == CD_NEG_INF ? 0.f : s * expf(m - M); }

template <typename T> struct CdGrp;                     // 16 bytes of a row as floats
template <> struct CdGrp<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float (&f)[4]) { load4<float>(p, f); }
};
template <> struct CdGrp<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float (&f)[8]) {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    f[0] = bf16_bits_to_f32(r.x & 0xffffu); f[1] = bf16_bits_to_f32(r.x >> 16);
    f[2] = bf16_bits_to_f32(r.y & 0xffffu); f[3] = bf16_bits_to_f32(r.y >> 16);
    f[4] = bf16_bits_to_f32(r.z & 0xffffu); f[5] = bf16_bits_to_f32(r.z >> 16);
    f[6] = bf16_bits_to_f32(r.w & 0xffffu); f[7] = bf16_bits_to_f32(r.w >> 16);
  }
};

// what one lane has seen of its row: the running arg-max (bv, bi), the online softmax pair (m, s) over the entries that are
// numbers, and whether any entry was a NaN
struct CdRow {
  float bv; int bi;
  float m, s;
  int nan;
};

template <int N>
__device__ __forceinline__ void cd_row_take(CdRow& a, const float (&x)[N], int c0) {
  float gm = CD_NEG_INF;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    cd_take(a.bv, a.bi, x[j], c0 + j);
    if (x[j] > gm) gm = x[j];
    a.nan |= __builtin_isnan(x[j]) ? 1 : 0;
  }
  if (gm > a.m) {                                       // one rescale per group; a.s is 0 while a.m is -inf
    a.s = cd_rescale(a.s, a.m, gm);
    a.m = gm;
  }
  if (a.m != CD_NEG_INF) {
#pragma unroll
    for (int j = 0; j < N; ++j) a.s += __builtin_isnan(x[j]) ? 0.f : expf(x[j] - a.m);
  }
}

// grid = ceil(N / 4), block = 256: wave w of a block owns row 4 blockIdx.x + w.  A row whose address is 16-byte aligned loads a group
// at once, any other row loads the same group element by element: the lanes see the same values in the same order (same bits).
template <typename T>
__global__ __launch_bounds__(256) void ctc_best_path_kernel(const T* __restrict__ X, long ldx, int N, int V, int32_t* __restrict__ tok,
                                                            float* __restrict__ lp) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const T* x = X + row * ldx;
  constexpr int G = CdGrp<T>::N;
  CdRow a = {CD_NEG_INF, INT_MAX, CD_NEG_INF, 0.f, 0};
  const int Vv = V - V % G;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
  for (int c0 = lane * G; c0 < Vv; c0 += 64 * G * CD_DEPTH) {
    float f[CD_DEPTH][G];
#pragma unroll
    for (int d = 0; d < CD_DEPTH; ++d) {
      const int c = c0 + d * 64 * G;
      if (c < Vv) {
        if (vec) CdGrp<T>::load(x + c, f[d]);
        else {
#pragma unroll
          for (int j = 0; j < G; ++j) f[d][j] = to_f32(x[c + j]);
        }
      }
    }
#pragma unroll
    for (int d = 0; d < CD_DEPTH; ++d) {
      const int c = c0 + d * 64 * G;
      if (c < Vv) cd_row_take<G>(a, f[d], c);
    }
  }
  for (int c = Vv + lane; c < V; c += 64) {             // the tail: fewer than G columns
    const float f[1] = {to_f32(x[c])};
    cd_row_take<1>(a, f, c);
  }
  // across the wave (butterflies: every lane ends with the same bits)
  float bv = a.bv, m = a.m;
  int bi = a.bi, nan = a.nan;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cd_take(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
    m = fmaxf(m, __shfl_xor(m, o, 64));
    nan |= __shfl_xor(nan, o, 64);
  }
  const float s = wave_sum(cd_rescale(a.s, a.m, m));
  if (lane != 0) return;
  tok[row] = bi == INT_MAX ? -1 : bi;                   // (no entry is a number: every comparison failed)
  lp[row] = nan ? __builtin_nanf("") : -logf(s);        // max - logsumexp = -log sum exp(z - max)
}

// ---- fused head: the tile and the K loop of transducer.hip's tj_mainloop (4 waves, 2 x 2 of 64 x 64, 32 x 32 MFMA fragments, MFMA
// operand a = W (columns v), b = X (rows n): lane l holds row n = l % 32 of each fragment, accumulator register r column
// v = 8 (r / 4) + 4 (l / 32) + r % 4) with a leading dimension for X and CLAMPED instead of zero-filled edges: rows >= N re-read row
// N - 1 and columns >= V re-read column V - 1; neither is ever stored (the epilogue sets the columns to -inf).
typedef __attribute__((ext_vector_type(4))) uint32_t cd_u32x4;
template <typename T> struct CdTraits;
template <> struct CdTraits<bf16_t> { static constexpr int BK = 64, PAD = 8; };
template <> struct CdTraits<float> { static constexpr int BK = 32, PAD = 4; };
template <typename T>
struct CdTile {
  static constexpr int BK = CdTraits<T>::BK, LDK = BK + CdTraits<T>::PAD;      // LDS row stride (elements; 16-byte multiple)
  static constexpr int CPR = BK * (int)sizeof(T) / 16;                          // 16-byte chunks per operand row and stage
  static constexpr int NLD = CD_TILE * CPR / 256;                               // chunks per thread and operand
  static constexpr int OP_BYTES = CD_TILE * LDK * (int)sizeof(T);
};

template <typename T>
__device__ __forceinline__ void cd_mainloop(const T* __restrict__ X, long ldx, const T* __restrict__ W, int N, int V, int K, int n0,
                                            int v0, char* smem, f32x16 (&acc)[2][2]) {
  using TT = CdTile<T>;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wv = wave & 1, wn = wave >> 1, l31 = lane & 31, hi = lane >> 5;
  char* Xs = smem;
  char* Ws = smem + TT::OP_BYTES;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  cd_u32x4 rx[TT::NLD], rw[TT::NLD];               // (a first-class vector: the loads below are values, not struct copies)
  auto load = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < TT::NLD; ++p) {
      const int idx = t + 256 * p, r = idx / TT::CPR, c = idx % TT::CPR;
      const int n = min(n0 + r, N - 1), v = min(v0 + r, V - 1);
      rx[p] = *reinterpret_cast<const cd_u32x4*>(reinterpret_cast<const char*>(X + (long)n * ldx + k0) + c * 16);
      rw[p] = *reinterpret_cast<const cd_u32x4*>(reinterpret_cast<const char*>(W + (long)v * K + k0) + c * 16);
    }
  };
  const int nk = K / TT::BK;
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                                     // the previous stage has been read
#pragma unroll
    for (int p = 0; p < TT::NLD; ++p) {
      const int idx = t + 256 * p, r = idx / TT::CPR, c = idx % TT::CPR;
      *reinterpret_cast<cd_u32x4*>(Xs + r * TT::LDK * (int)sizeof(T) + c * 16) = rx[p];
      *reinterpret_cast<cd_u32x4*>(Ws + r * TT::LDK * (int)sizeof(T) + c * 16) = rw[p];
    }
    __syncthreads();
    if (kt + 1 < nk) load((kt + 1) * TT::BK);
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int kk = 0; kk < TT::BK / 16; ++kk) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
          fa[i] = *reinterpret_cast<const bf16x8*>(Ws + ((wv * 64 + i * 32 + l31) * TT::LDK + kk * 16 + hi * 8) * 2);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          fb[j] = *reinterpret_cast<const bf16x8*>(Xs + ((wn * 64 + j * 32 + l31) * TT::LDK + kk * 16 + hi * 8) * 2);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    } else {
      // fp32 operands: each stage is summed on its own and then added to the running sum (two levels of rounding, as tj_mainloop)
      const float* Wf = reinterpret_cast<const float*>(Ws);
      const float* Xf = reinterpret_cast<const float*>(Xs);
      f32x16 st[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) st[i][j][e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < TT::BK / 2; ++kk) {
        float fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = Wf[(wv * 64 + i * 32 + l31) * TT::LDK + kk * 2 + hi];
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = Xf[(wn * 64 + j * 32 + l31) * TT::LDK + kk * 2 + hi];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) st[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], st[i][j], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] += st[i][j];
    }
  }
}

// part[n][ct] = (max, first arg-max, sum exp(z - max)) of row n over the valid columns of column tile ct.  A thread walks its 32
// columns of a row in ascending order, then the two lane halves and the two waves that share the row meet in a fixed order.
template <typename T>
__global__ __launch_bounds__(256, 2) void ctc_head_kernel(const T* __restrict__ X, long ldx, const T* __restrict__ W,
                                                          const float* __restrict__ bias, int N, int K, int V, int nct,
                                                          float* __restrict__ pmax, int* __restrict__ parg, float* __restrict__ psum) {
  __shared__ __attribute__((aligned(16))) char smem[2 * CdTile<T>::OP_BYTES];
  __shared__ float sbias[CD_TILE];
  __shared__ float red_m[CD_TILE], red_s[CD_TILE];
  __shared__ int red_k[CD_TILE];
  const int ct = blockIdx.x % nct, rt = blockIdx.x / nct;
  const int n0 = rt * CD_TILE, v0 = ct * CD_TILE;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wv = wave & 1, wn = wave >> 1, l31 = lane & 31, hi = lane >> 5;
  if (t < CD_TILE) sbias[t] = (bias && v0 + t < V) ? bias[v0 + t] : 0.f;
  f32x16 acc[2][2];
  cd_mainloop<T>(X, ldx, W, N, V, K, n0, v0, smem, acc);      // (its barriers publish sbias)
  float m[2], s[2];
  int k[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float mx = CD_NEG_INF;
    int kx = INT_MAX;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int vl = wv * 64 + i * 32 + 8 * (r >> 2) + 4 * hi + (r & 3), v = v0 + vl;
        const float z = v < V ? acc[i][j][r] + sbias[vl] : CD_NEG_INF;          // columns beyond V: -inf, not the clamped column's value
        acc[i][j][r] = z;
        if (v < V) cd_take(mx, kx, z, v);
      }
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = v0 + wv * 64 + i * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
        const float z = acc[i][j][r];
        if (v < V) sm += __builtin_isnan(z) ? z : (mx == CD_NEG_INF ? 0.f : expf(z - mx));   // a NaN logit makes the row's lp a NaN
      }
    // the other lane half (same row, the other 4-column groups): fixed pairing, both halves end with the same bits
    const float mo = __shfl_xor(mx, 32, 64), so = __shfl_xor(sm, 32, 64);
    const int ko = __shfl_xor(kx, 32, 64);
    float M = mx;
    int Kk = kx;
    cd_take(M, Kk, mo, ko);
    const float a = hi ? mo : mx, sa = hi ? so : sm, bq = hi ? mx : mo, sb = hi ? sm : so;   // (lower half first)
    m[j] = M; k[j] = Kk;
    s[j] = (__builtin_isnan(sa) || __builtin_isnan(sb)) ? __builtin_nanf("") : cd_rescale(sa, a, M) + cd_rescale(sb, bq, M);
  }
  // the two waves of a row pair: wave wv = 1 parks its result, wave wv = 0 folds it in (column order) and writes
  if (wv == 1 && hi == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = wn * 64 + j * 32 + l31;
      red_m[nl] = m[j]; red_k[nl] = k[j]; red_s[nl] = s[j];
    }
  }
  __syncthreads();
  if (wv == 0 && hi == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = wn * 64 + j * 32 + l31, n = n0 + nl;
      if (n < N) {
        const float om = red_m[nl], os = red_s[nl];
        float M = m[j];
        int Kk = k[j];
        cd_take(M, Kk, om, red_k[nl]);
        const long o = (long)n * nct + ct;
        pmax[o] = M;
        parg[o] = Kk;
        psum[o] = (__builtin_isnan(s[j]) || __builtin_isnan(os)) ? __builtin_nanf("") : cd_rescale(s[j], m[j], M) + cd_rescale(os, om, M);
      }
    }
  }
}

// one thread per row: the tiles in ascending order (a tie keeps the lower column)
__global__ __launch_bounds__(256) void ctc_head_reduce_kernel(const float* __restrict__ pmax, const int* __restrict__ parg,
                                                              const float* __restrict__ psum, int nct, int N, int V,
                                                              int32_t* __restrict__ tok, float* __restrict__ lp) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const long o = (long)n * nct;
  float M = CD_NEG_INF;
  int k = INT_MAX;
  for (int c = 0; c < nct; ++c) cd_take(M, k, pmax[o + c], parg[o + c]);
  float S = 0.f;
  int nan = 0;
  for (int c = 0; c < nct; ++c) {
    const float ps = psum[o + c];
    nan |= __builtin_isnan(ps) ? 1 : 0;
    S += __builtin_isnan(ps) ? 0.f : cd_rescale(ps, pmax[o + c], M);
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

static int cd_tiles(int V) { return (V + CD_TILE - 1) / CD_TILE; }
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
  const long nrt = ((long)N + CD_TILE - 1) / CD_TILE;
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
