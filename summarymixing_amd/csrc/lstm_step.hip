// lstm_step.hip — one LSTM-cell step in one launch, for the decode step of the transducer recipe's RNNLM (recipe key `lm_model`:
// an embedding table, a two-layer LSTM of 2048 units, a DNN block and an output Linear), and the table-row gather of its sequence
// form.  gfx950 only.
//
// The step streams its weights once: at the recipe size a layer reads 4 H (I + H) elements (34 - 67 MB in bf16) and a few hundred
// KB of everything else.  A workgroup owns 8 hidden units = the 32 rows {g H + j0 .. g H + j0 + 7, g = i, f, g, o} of W_ih and W_hh,
// two 16-column MFMA tiles (columns 0-15: gates i, f; 16-31: gates g, o), and keeps them for EVERY batch row: the batch tiles
// (16 rows each, up to STEP_TILES accumulator sets at once) are looped inside the workgroup, not spread over the grid, so no weight
// element is fetched by two workgroups whatever B is; H = 2048 gives 256 workgroups.  The reduce dimension K = I + H is cut over the
// 8 waves: wave w takes the w-th eighth (in 32-element blocks) of the input part and of the recurrent part.  A lane reads 32
// contiguous bytes of its weight row per step - the 16 lanes-rows x 4 lanes of a wave cover whole 128-byte lines - straight
// into registers, one step ahead of the MFMAs (weights are used once per workgroup: LDS staging would be a round trip for
// nothing); the same 32 bytes of the activation rows (h, x or a gathered table row; L2 hits) pair with them, so the k order inside
// a step is a permutation the two operands share.  The eight partial tiles of a batch tile meet in LDS, are added in a fixed tree, and
// thread (row, unit) finishes its cell in fp32 (lstm_tile.h's lstm_cell, the cell of lstm.hip and greedy.hip; the K-split reduction before
// it is this file's own).  No atomics, every sum in a fixed order that depends on (I, H) alone: values are
// bit-reproducible and a row's values do not depend on B or on the other rows.  Tile rows beyond B repeat row B - 1 and are never
// stored.
#include "lstm_tile.h"

namespace smx {

static constexpr int STEP_UNITS = 8;       // hidden units per workgroup (x 4 gates = 32 weight rows)
static constexpr int STEP_WAVES = 8;       // the cut of K
static constexpr int STEP_TILES = 6;       // batch tiles per pass over the weights (96 rows: what fits 256 registers); more rows: another pass by the SAME workgroup

struct LstmStepArgs {
  const void* x; long ldx;                 // dense (B, I) rows, or the (V, I) table when tok != null
  const int32_t* tok; int V;
  const void* Wih; const void* Whh;        // (4H, I), (4H, H)
  const float* bias;                       // (4H) = b_ih + b_hh
  const void* h; const float* c;           // (B, H) or null (zeros)
  void* h_out; float* c_out;               // (B, H)
  int B, I, H;
};

struct StepFrag { uint4 lo, hi; };         // 32 bytes of one row: 16 bf16 / 8 f32 reduce indices of this lane

template <typename T>
__device__ __forceinline__ StepFrag step_load(const T* p) {
  StepFrag f;
  f.lo = *reinterpret_cast<const uint4*>(p);
  f.hi = *(reinterpret_cast<const uint4*>(p) + 1);
  return f;
}

__device__ __forceinline__ void step_mma(lstm_f32x4& acc, const StepFrag& a, const StepFrag& b, bf16_t) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a.lo), __builtin_bit_cast(bf16x8, b.lo), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a.hi), __builtin_bit_cast(bf16x8, b.hi), acc, 0, 0, 0);
}
__device__ __forceinline__ void step_mma(lstm_f32x4& acc, const StepFrag& a, const StepFrag& b, float) {
  const float4 a0 = __builtin_bit_cast(float4, a.lo), a1 = __builtin_bit_cast(float4, a.hi);
  const float4 b0 = __builtin_bit_cast(float4, b.lo), b1 = __builtin_bit_cast(float4, b.hi);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, acc, 0, 0, 0);
}

// acc[t][n] += A_t[:, k0:k1] . W_n[:, k0:k1]^T for the NT batch tiles (nt of them live) and the two weight tiles.  b0 / b1: this lane's
// weight rows; A + ai[t] lda: its activation row of tile t (ai[t] < 0: a zero row); k0, k1 multiples of 32.  Steps of 128 bytes per row (64 bf16 /
// 32 f32), the weights of the next step in flight under this step's MFMAs; bf16 ends on a 32-element step when (k1 - k0) / 32 is odd.
template <typename T, int NT>
__device__ __forceinline__ void step_segment(lstm_f32x4 (&acc)[NT][2], const T* b0, const T* b1, const T* A, long lda, const int (&ai)[NT],
                                             int k0, int k1, int nt, int q) {
  constexpr int KS = 128 / (int)sizeof(T), LO = KS / 4;
  const StepFrag zero = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
  int k = k0;
  if (k + KS <= k1) {                                                         // (uniform)
    StepFrag n0 = step_load(b0 + k + LO * q), n1 = step_load(b1 + k + LO * q);
    for (; k + KS <= k1; k += KS) {
      const StepFrag w0 = n0, w1 = n1;
      StepFrag a[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        a[t] = zero;
        if (t < nt && ai[t] >= 0) a[t] = step_load(A + ai[t] * lda + k + LO * q);
      }
      if (k + 2 * KS <= k1) {                                                 // (uniform)
        n0 = step_load(b0 + k + KS + LO * q);
        n1 = step_load(b1 + k + KS + LO * q);
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t < nt) {                                                         // (uniform)
          step_mma(acc[t][0], a[t], w0, T());
          step_mma(acc[t][1], a[t], w1, T());
        }
      }
    }
  }
  if constexpr (sizeof(T) == 2) {
    if (k < k1) {                                                             // (uniform) one 32-element block: 16 bytes per lane
      const uint4 w0 = *reinterpret_cast<const uint4*>(b0 + k + 8 * q), w1 = *reinterpret_cast<const uint4*>(b1 + k + 8 * q);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t < nt) {
          uint4 av = make_uint4(0, 0, 0, 0);
          if (ai[t] >= 0) av = *reinterpret_cast<const uint4*>(A + ai[t] * lda + k + 8 * q);
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, w0), acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, w1), acc[t][1], 0, 0, 0);
        }
      }
    }
  }
}

template <typename T, int NT>
__global__ __launch_bounds__(64 * STEP_WAVES) void lstm_step_kernel(LstmStepArgs s) {
  __shared__ float red[STEP_WAVES][2][16][17];
  const int H = s.H, I = s.I, B = s.B, j0 = blockIdx.x * STEP_UNITS;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  // this lane's weight rows: column r of tile n is gate 2 n + (r >> 3), unit j0 + (r & 7)
  const long wrow0 = (long)(r >> 3) * H + j0 + (r & 7), wrow1 = wrow0 + 2L * H;
  const T* Wih = reinterpret_cast<const T*>(s.Wih);
  const T* Whh = reinterpret_cast<const T*>(s.Whh);
  const T* X = reinterpret_cast<const T*>(s.x);
  const T* Hp = reinterpret_cast<const T*>(s.h);
  const int nx = I / 32, nh = Hp ? H / 32 : 0;
  const int x0 = w * nx / STEP_WAVES * 32, x1 = (w + 1) * nx / STEP_WAVES * 32;
  const int h0 = w * nh / STEP_WAVES * 32, h1 = (w + 1) * nh / STEP_WAVES * 32;
  for (int bg = 0; bg < B; bg += 16 * NT) {
    const int nt = min(NT, (B - bg + 15) / 16);
    lstm_f32x4 acc[NT][2];
    int xi[NT], hi[NT];                                                        // this lane's input and state row per tile
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[t][0] = lstm_f32x4{0.f, 0.f, 0.f, 0.f};
      acc[t][1] = acc[t][0];
      const int row = min(bg + 16 * t + r, B - 1);
      xi[t] = hi[t] = row;
      if (s.tok) {
        const int k = s.tok[row];
        xi[t] = (k >= 0 && k < s.V) ? k : -1;                                  // (a token outside the table: a zero row)
      }
    }
    step_segment<T, NT>(acc, Wih + wrow0 * I, Wih + wrow1 * I, X, s.ldx, xi, x0, x1, nt, q);
    step_segment<T, NT>(acc, Whh + wrow0 * H, Whh + wrow1 * H, Hp, (long)H, hi, h0, h1, nt, q);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < nt) {                                                           // (uniform)
        __syncthreads();                                                      // (the previous tile's cells have read red)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          red[w][0][q * 4 + i][r] = acc[t][0][i];
          red[w][1][q * 4 + i][r] = acc[t][1][i];
        }
        __syncthreads();
        const int bb = tid >> 3, u = tid & 7, b = bg + 16 * t + bb, j = j0 + u;
        if (tid < 16 * STEP_UNITS && b < B) {
          float z[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int n = g >> 1, cc = (g & 1) * 8 + u;
            const float p = ((red[0][n][bb][cc] + red[1][n][bb][cc]) + (red[2][n][bb][cc] + red[3][n][bb][cc])) +
                            ((red[4][n][bb][cc] + red[5][n][bb][cc]) + (red[6][n][bb][cc] + red[7][n][bb][cc]));
            z[g] = p + s.bias[g * H + j];
          }
          float gates[4], c;
          const float h = lstm_cell(z, s.c ? s.c[(long)b * H + j] : 0.f, gates, c);
          s.c_out[(long)b * H + j] = c;
          reinterpret_cast<T*>(s.h_out)[(long)b * H + j] = from_f32<T>(h);
        }
      }
    }
  }
}

// Y[r, :] = table[tok[r], :] (a token outside [0, V): zeros), 16 bytes per thread
__global__ __launch_bounds__(256) void gather_rows_kernel(const int32_t* __restrict__ tok, const char* __restrict__ table, long ldt_bytes,
                                                          char* __restrict__ Y, long ldy_bytes, int V, int chunks) {
  const int r = blockIdx.x, ch = blockIdx.y * 256 + threadIdx.x;
  if (ch >= chunks) return;
  const int k = tok[r];
  uint4 v = make_uint4(0, 0, 0, 0);
  if (k >= 0 && k < V) v = *reinterpret_cast<const uint4*>(table + (long)k * ldt_bytes + (long)ch * 16);
  *reinterpret_cast<uint4*>(Y + (long)r * ldy_bytes + (long)ch * 16) = v;
}

static inline bool step_i_ok(int I) { return I >= 32 && I <= 4096 && I % 32 == 0; }
static inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return a && b && pa < pb + nb && pb < pa + na;
}

template <typename T>
static void launch_step(const LstmStepArgs& s, hipStream_t stream) {
  const dim3 grid(s.H / STEP_UNITS), block(64 * STEP_WAVES);
  const int tiles = (s.B + 15) / 16;
  if (tiles <= 1) hipLaunchKernelGGL((lstm_step_kernel<T, 1>), grid, block, 0, stream, s);
  else if (tiles <= 2) hipLaunchKernelGGL((lstm_step_kernel<T, 2>), grid, block, 0, stream, s);
  else if (tiles <= 4) hipLaunchKernelGGL((lstm_step_kernel<T, 4>), grid, block, 0, stream, s);
  else hipLaunchKernelGGL((lstm_step_kernel<T, STEP_TILES>), grid, block, 0, stream, s);
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_lstm_step_ok(int dtype, int I, int H) {
  return (dtype == SMX_F32 || dtype == SMX_BF16) && lstm_h_ok(H) && step_i_ok(I) ? 1 : 0;
}

extern "C" int smx_lstm_step(int dtype, const void* X, int64_t ldx, const int32_t* tok, int V, const void* Wih, const void* Whh,
                             const float* bias, const void* h, const float* c, void* h_out, float* c_out, int B, int I, int H,
                             void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_lstm_step: bad dtype %d", dtype);
  SMX_REQUIRE(X && Wih && Whh && bias && h_out && c_out, "smx_lstm_step: null pointer");
  SMX_REQUIRE(B >= 0 && I >= 1 && H >= 1 && ldx >= I && (!tok || V >= 1), "smx_lstm_step: bad sizes B=%d I=%d H=%d ldx=%lld V=%d", B, I, H,
              (long long)ldx, V);
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  const size_t nh = (size_t)B * H * es, nc = (size_t)B * H * 4;
  // other workgroups read h, c and the input rows while this one writes its units of h' and c'
  SMX_REQUIRE(!overlap(h_out, nh, h, nh) && !overlap(c_out, nc, c, nc) && !overlap(h_out, nh, c_out, nc) && !overlap(h_out, nh, c, nc) &&
                  !overlap(c_out, nc, h, nh),
              "smx_lstm_step: h' / c' alias the incoming state");
  if (!tok && B > 0)
    SMX_REQUIRE(!overlap(h_out, nh, X, ((size_t)(B - 1) * ldx + I) * es) && !overlap(c_out, nc, X, ((size_t)(B - 1) * ldx + I) * es),
                "smx_lstm_step: h' / c' alias the input rows");
  if (!lstm_h_ok(H)) return fail(SMX_EUNSUPPORTED, "smx_lstm_step: H must be a multiple of 32 in [32, %d], got %d", LSTM_H_MAX, H);
  if (!step_i_ok(I)) return fail(SMX_EUNSUPPORTED, "smx_lstm_step: I must be a multiple of 32 in [32, 4096], got %d", I);
  if (!aligned16(X) || !aligned16(Wih) || !aligned16(Whh) || (h && !aligned16(h)) || ldx % 8 != 0)
    return fail(SMX_EUNSUPPORTED, "smx_lstm_step: X, W_ih, W_hh and h must be 16-byte aligned, ldx a multiple of 8");
  if (B == 0) return SMX_OK;
  LstmStepArgs s;
  s.x = X; s.ldx = (long)ldx; s.tok = tok; s.V = V; s.Wih = Wih; s.Whh = Whh; s.bias = bias; s.h = h; s.c = c;
  s.h_out = h_out; s.c_out = c_out; s.B = B; s.I = I; s.H = H;
  dispatch_dtype(dtype, [&](auto tag) { launch_step<decltype(tag)>(s, STREAM); });
  return check_launch("smx_lstm_step");
}

extern "C" int smx_gather_rows(int dtype, const int32_t* tok, const void* table, int64_t ldt, void* Y, int64_t ldy, int rows, int V, int D,
                               void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_gather_rows: bad dtype %d", dtype);
  SMX_REQUIRE(tok && table && Y, "smx_gather_rows: null pointer");
  SMX_REQUIRE(rows >= 0 && rows <= 65535 * 1024 && V >= 1 && D >= 1 && ldt >= D && ldy >= D, "smx_gather_rows: bad sizes rows=%d V=%d D=%d", rows, V, D);
  if (D % 8 != 0 || ldt % 8 != 0 || ldy % 8 != 0 || !aligned16(table) || !aligned16(Y))
    return fail(SMX_EUNSUPPORTED, "smx_gather_rows: row widths and leading dimensions must be multiples of 8, the bases 16-byte aligned");
  if (rows == 0) return SMX_OK;
  const long es = dtype == SMX_BF16 ? 2 : 4;
  const int chunks = (int)(D * es / 16);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(rows, (chunks + 255) / 256), dim3(256), 0, STREAM, tok, (const char*)table, (long)ldt * es,
                     (char*)Y, (long)ldy * es, V, chunks);
  return check_launch("smx_gather_rows");
}
