// stream.hip — chunk-by-chunk streaming inference of a Dynamic-Chunk-trained Conformer encoder (gfx950).
//
// A chunk step runs the encoder on one chunk of C_cur <= C frames per stream.  Two operators of a layer look at earlier chunks:
// the DynChunk summary (window mean over the chunks [c - left, c]) and the depthwise convolution (the (k-1)/2 previous inputs).
// Their state lives in caller-owned device buffers and is advanced by the kernels below; the chunk index c comes from a
// device-resident counter (smx_step_counter_add convention), so a captured chunk step stays valid on replay.
// Lockstep streaming runs B streams that all sit at the same chunk; slot streaming runs B independent streams, one per batch slot,
// each with its own chunk counter and length.  Both run the SAME kernel bodies below (ChunkRows<SLOTS> says who holds which rows).
#include "smx_common.h"

namespace smx {

constexpr int ST_CMAX = 64;     // max frames per chunk
constexpr int ST_KMAX = 63;     // max depthwise taps
constexpr int ST_HMAX = (ST_KMAX - 1) / 2;
constexpr int ST_COLS = 64;     // columns (channels) per workgroup

// ---- who holds which rows in this step -----------------------------------------------------------------------------------
// Lockstep (SLOTS = false): stream b holds C_cur rows from row b * C_cur; the chunk index is counters[0] (the conv passes none).
// Slots (SLOTS = true): slot b holds min(valid[b], C) rows from row b * C (clamped: a bad host value cannot index past the slot's
// rows; 0 = the slot sits out: nothing of it is read or written); its chunk index is counters[b].  Counter 0 means fresh state
// for a slot: chunk 0 reads no ring slot, no running sum and no convolution state (they are read as zero), so starting a slot is
// counters[b] = 0 and nothing else.  Lockstep reads its state as stored (the contexts zero it).
template <bool SLOTS>
struct ChunkRows {
  const int64_t* counters;      // lockstep: (1,); slots: (B,)
  const int32_t* valid;         // slots: (B,)
  int C_cur, C;
  __device__ int frames(int b) const { return SLOTS ? min(valid[b], C) : C_cur; }
  __device__ long first(int b) const { return (long)b * (SLOTS ? C : C_cur); }
  __device__ long chunk(int b) const { return (long)counters[SLOTS ? b : 0]; }
};

// ---- summary: grid (ceil(D / 64), B), 256 threads = 64 columns x 4 waves -------------------------------------------------
// lane = column, wave w sums the chunk rows w, w + 4, ...; the four partials fold in a fixed order, then the window sum
// (ring slots of the earlier chunks, oldest first) is added and divided by the window's frame count.  Every thread reads the
// ring slots of its own column before it writes the chunk's sum into slot c % left: nothing is shared between threads there.
// One body, one fold order: a step of full, equal-counter slots gives the bits of lockstep.
template <typename T, bool SLOTS>
__global__ __launch_bounds__(256) void chunk_summary_kernel(const T* __restrict__ S, long lds, T* __restrict__ out, long ldo,
                                                            float* __restrict__ ring, ChunkRows<SLOTS> rows, int D, int left) {
  __shared__ float red[4][ST_COLS];
  __shared__ float mean[ST_COLS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
  const int v = rows.frames(b);
  if (SLOTS && v <= 0) return;                            // (uniform over the workgroup: before any barrier)
  const int col = blockIdx.x * ST_COLS + lane;
  const bool ok = col < D;
  const long c = rows.chunk(b), row0 = rows.first(b);
  const int C = rows.C;
  float acc = 0.f;
  if (ok)
    for (int t = w; t < v; t += 4) acc += to_f32(S[(row0 + t) * lds + col]);
  red[w][lane] = acc;
  __syncthreads();
  if (w == 0) {
    const float csum = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    float win = 0.f;
    long frames;
    if (left < 0) {                                       // unlimited: ring = one running (B, D) sum (a slot: not read at chunk 0)
      float* r = ring + (long)b * D + col;
      if (ok) { if (!SLOTS || c > 0) win = *r; *r = win + csum; }
      frames = c * C + v;
    } else {
      const long nprev = c < left ? c : left;
      float* r = ring + (long)b * left * D + col;
      if (ok) {
        for (long j = c - nprev; j < c; ++j) win += r[(j % left) * D];
        if (left > 0) r[(c % left) * D] = csum;           // (slot c % left held chunk c - left: read above when in the window)
      }
      frames = nprev * C + v;
    }
    mean[lane] = (win + csum) / (float)frames;
  }
  __syncthreads();
  if (!ok) return;
  const T m = from_f32<T>(mean[lane]);
  for (int t = w; t < v; t += 4) out[(row0 + t) * ldo + col] = m;
}

// ---- GLU + depthwise conv over one chunk: grid (ceil(D / 64), B), 256 threads = 64 channels x 4 waves ---------------------
// Rows of X = [state (H rows); chunk (v rows)], H = (k-1)/2.  Output frame t of the chunk is X-row H + t; tap j reads X-row
// t + j and reads zero at and beyond H + v (Dynamic Chunk Convolution: nothing past the chunk).  The workgroup reads every
// row of its channels (the GLU'd values into LDS, the last H pre-GLU rows into LDS as well) before one barrier, then writes
// Y and the new state = the last H pre-GLU rows of X: the in-place state update never races a read.  Chunk rows at and beyond
// v are never loaded.
template <typename T, bool SLOTS>
__global__ __launch_bounds__(256) void chunk_dwconv_kernel(const T* __restrict__ P, long ldp, const float* __restrict__ w,
                                                           const float* __restrict__ bias, T* state, T* __restrict__ Y, long ldy,
                                                           ChunkRows<SLOTS> rows, int D, int k) {
  __shared__ float u[ST_HMAX + ST_CMAX][ST_COLS];
  __shared__ float raw[ST_HMAX][2][ST_COLS];
  __shared__ float wl[ST_KMAX][ST_COLS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.y;
  const int v = rows.frames(b);
  if (SLOTS && v <= 0) return;                            // (uniform over the workgroup: before any barrier)
  const bool fresh = SLOTS && rows.chunk(b) == 0;
  const long row0 = rows.first(b);
  const int ch = blockIdx.x * ST_COLS + lane;
  const bool ok = ch < D;
  const int H = (k - 1) / 2, R = H + v;
  T* st = state + (long)b * H * 2 * D;
  for (int i = wv; i < R; i += 4) {
    float a = 0.f, g = 0.f;
    if (ok && !(i < H && fresh)) {
      const T* row = i < H ? st + (long)i * 2 * D : P + (row0 + (i - H)) * ldp;
      a = to_f32(row[ch]);
      g = to_f32(row[D + ch]);
    }
    u[i][lane] = a * sigmoidf_(g);
    if (i >= v) { raw[i - v][0][lane] = a; raw[i - v][1][lane] = g; }
  }
  for (int j = wv; j < k; j += 4) wl[j][lane] = ok ? w[(long)ch * k + j] : 0.f;
  __syncthreads();
  if (!ok) return;
  const float bs = bias ? bias[ch] : 0.f;
  for (int t = wv; t < v; t += 4) {
    float acc = bs;
    const int jmax = min(k, R - t);
    for (int j = 0; j < jmax; ++j) acc += wl[j][lane] * u[t + j][lane];
    Y[(row0 + t) * ldy + ch] = from_f32<T>(acc);
  }
  for (int i = wv; i < H; i += 4) {
    st[(long)i * 2 * D + ch] = from_f32<T>(raw[i][0][lane]);
    st[(long)i * 2 * D + D + ch] = from_f32<T>(raw[i][1][lane]);
  }
}

// ---- end of a chunk step: one workgroup.  c' = counter + 1; pe[r] = table[c' C + r] (zero past the table); counter = c' ----
template <typename T>
__global__ __launch_bounds__(256) void stream_advance_kernel(uint64_t* counter, const T* __restrict__ table, long ldt, int rows,
                                                             T* __restrict__ pe, long ldpe, int C, int D) {
  __shared__ uint64_t next;
  if (threadIdx.x == 0) next = counter[0] + 1;
  __syncthreads();
  const long r0 = (long)next * C;
  for (long i = threadIdx.x; i < (long)C * D; i += 256) {
    const long r = i / D, col = i % D;
    pe[r * ldpe + col] = r0 + r < rows ? table[(r0 + r) * ldt + col] : from_f32<T>(0.f);
  }
  if (threadIdx.x == 0) counter[0] = next;
}

// ---- first launch of a step: grid (C, B) (pe == NULL: (1, B)), 256 threads.  Workgroup (r, b): c = start[b] ? 0 : counters[b],
// pe[b, r] = table[c C + r] (zero past the table).  Only workgroup (0, b) writes counters[b] (to 0, where start[b]); the others
// read it, but a started slot's value is never used, so the read needs no ordering.
template <typename T>
__global__ __launch_bounds__(256) void slot_begin_kernel(int64_t* counters, const uint8_t* __restrict__ start,
                                                         const T* __restrict__ table, long ldt, int rows, T* __restrict__ pe, long ldpe,
                                                         int C, int D) {
  const int r = blockIdx.x, b = blockIdx.y;
  const bool s = start[b] != 0;
  if (pe) {
    const long row = (s ? 0 : (long)counters[b]) * C + r;
    T* dst = pe + ((long)b * C + r) * ldpe;
    if (row < rows) {
      const T* src = table + row * ldt;
      for (int col = threadIdx.x; col < D; col += 256) dst[col] = src[col];
    } else {
      for (int col = threadIdx.x; col < D; col += 256) dst[col] = from_f32<T>(0.f);
    }
  }
  if (s && r == 0 && threadIdx.x == 0) counters[b] = 0;
}

// ---- last launch of a step: counters[b] += (valid[b] == C), one thread per slot --------------------------------------------
__global__ __launch_bounds__(256) void slot_advance_kernel(int64_t* counters, const int32_t* __restrict__ valid, int B, int C) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B && valid[b] == C) counters[b] = counters[b] + 1;
}

}  // namespace smx

using namespace smx;

#define STREAM (reinterpret_cast<hipStream_t>(stream))

// The checks and the dtype dispatch that the lockstep and the slot entry point of an operator share; `what` is the entry point.
template <bool SLOTS>
static int summary_launch(const char* what, int dtype, const void* S, int64_t lds, void* out, int64_t ldo, float* ring,
                          ChunkRows<SLOTS> rows, int B, int D, int left, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "%s: bad dtype", what);
  SMX_REQUIRE(S && out && (ring || left == 0), "%s: null pointer", what);
  SMX_REQUIRE(B > 0 && D > 0 && D % 8 == 0, "%s: B > 0 and D %% 8 == 0 (B=%d D=%d)", what, B, D);
  SMX_REQUIRE(left >= -1 && left <= 32, "%s: left in {-1 (unlimited), 0 .. 32} (left=%d)", what, left);
  SMX_REQUIRE(lds >= D && ldo >= D, "%s: row strides must be >= D", what);
  dim3 grid((unsigned)((D + ST_COLS - 1) / ST_COLS), (unsigned)B);
  if (dtype == SMX_BF16)
    hipLaunchKernelGGL((chunk_summary_kernel<bf16_t, SLOTS>), grid, dim3(256), 0, STREAM, (const bf16_t*)S, (long)lds, (bf16_t*)out,
                       (long)ldo, ring, rows, D, left);
  else
    hipLaunchKernelGGL((chunk_summary_kernel<float, SLOTS>), grid, dim3(256), 0, STREAM, (const float*)S, (long)lds, (float*)out,
                       (long)ldo, ring, rows, D, left);
  return check_launch(what);
}

template <bool SLOTS>
static int dwconv_launch(const char* what, int dtype, const void* P, int64_t ldp, const float* w, const float* bias, void* state,
                         void* Y, int64_t ldy, ChunkRows<SLOTS> rows, int B, int D, int k, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "%s: bad dtype", what);
  SMX_REQUIRE(P && w && Y && (state || k == 1), "%s: null pointer", what);
  SMX_REQUIRE(k >= 1 && k <= ST_KMAX && (k & 1), "%s: k=%d must be odd and <= %d", what, k, ST_KMAX);
  SMX_REQUIRE(B > 0 && D > 0 && D % 8 == 0, "%s: B > 0 and D %% 8 == 0 (B=%d D=%d)", what, B, D);
  SMX_REQUIRE(ldp >= 2 * (int64_t)D && ldy >= D, "%s: ldp >= 2 D and ldy >= D", what);
  dim3 grid((unsigned)((D + ST_COLS - 1) / ST_COLS), (unsigned)B);
  if (dtype == SMX_BF16)
    hipLaunchKernelGGL((chunk_dwconv_kernel<bf16_t, SLOTS>), grid, dim3(256), 0, STREAM, (const bf16_t*)P, (long)ldp, w, bias,
                       (bf16_t*)state, (bf16_t*)Y, (long)ldy, rows, D, k);
  else
    hipLaunchKernelGGL((chunk_dwconv_kernel<float, SLOTS>), grid, dim3(256), 0, STREAM, (const float*)P, (long)ldp, w, bias,
                       (float*)state, (float*)Y, (long)ldy, rows, D, k);
  return check_launch(what);
}

extern "C" int smx_stream_summary(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, float* ring,
                                  const uint64_t* counter, int B, int C_cur, int C, int D, int left, void* stream) {
  SMX_REQUIRE(counter, "smx_stream_summary: null pointer");
  SMX_REQUIRE(C >= 1 && C <= ST_CMAX && C_cur >= 1 && C_cur <= C, "smx_stream_summary: 1 <= C_cur <= C <= %d (C_cur=%d C=%d)",
              ST_CMAX, C_cur, C);
  const ChunkRows<false> rows{reinterpret_cast<const int64_t*>(counter), nullptr, C_cur, C};   // (same bits: the index is >= 0)
  return summary_launch("smx_stream_summary", dtype, S, lds, out, ldo, ring, rows, B, D, left, stream);
}

extern "C" int smx_slot_summary(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, float* ring, const int64_t* counters,
                                const int32_t* valid, int B, int C, int D, int left, void* stream) {
  SMX_REQUIRE(counters && valid, "smx_slot_summary: null pointer");
  SMX_REQUIRE(B <= 65535 && C >= 1 && C <= ST_CMAX, "smx_slot_summary: B <= 65535 and 1 <= C <= %d (B=%d C=%d)", ST_CMAX, B, C);
  return summary_launch("smx_slot_summary", dtype, S, lds, out, ldo, ring, ChunkRows<true>{counters, valid, C, C}, B, D, left, stream);
}

extern "C" int smx_dwconv1d_glu_stream(int dtype, const void* P, int64_t ldp, const float* w, const float* bias, void* state,
                                       void* Y, int64_t ldy, int B, int C_cur, int D, int k, void* stream) {
  SMX_REQUIRE(C_cur >= 1 && C_cur <= ST_CMAX, "smx_dwconv1d_glu_stream: 1 <= C_cur <= %d (C_cur=%d)", ST_CMAX, C_cur);
  const ChunkRows<false> rows{nullptr, nullptr, C_cur, C_cur};   // (the lockstep conv takes no counter: it always reads its state)
  return dwconv_launch("smx_dwconv1d_glu_stream", dtype, P, ldp, w, bias, state, Y, ldy, rows, B, D, k, stream);
}

extern "C" int smx_dwconv1d_glu_slots(int dtype, const void* P, int64_t ldp, const float* w, const float* bias, void* state, void* Y,
                                      int64_t ldy, const int32_t* valid, const int64_t* counters, int B, int C, int D, int k,
                                      void* stream) {
  SMX_REQUIRE(valid && counters, "smx_dwconv1d_glu_slots: null pointer");
  SMX_REQUIRE(B <= 65535 && C >= 1 && C <= ST_CMAX, "smx_dwconv1d_glu_slots: B <= 65535 and 1 <= C <= %d (B=%d C=%d)", ST_CMAX, B, C);
  return dwconv_launch("smx_dwconv1d_glu_slots", dtype, P, ldp, w, bias, state, Y, ldy, ChunkRows<true>{counters, valid, C, C}, B, D,
                       k, stream);
}

extern "C" int smx_stream_advance(int dtype, uint64_t* counter, const void* table, int64_t ldt, int rows, void* pe, int64_t ldpe,
                                  int C, int D, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_stream_advance: bad dtype");
  SMX_REQUIRE(counter && table && pe, "smx_stream_advance: null pointer");
  SMX_REQUIRE(C >= 1 && C <= ST_CMAX && D > 0 && rows >= 0, "smx_stream_advance: 1 <= C <= %d, D > 0", ST_CMAX);
  SMX_REQUIRE(ldt >= D && ldpe >= D, "smx_stream_advance: row strides must be >= D");
  if (dtype == SMX_BF16)
    hipLaunchKernelGGL(stream_advance_kernel<bf16_t>, dim3(1), dim3(256), 0, STREAM, counter, (const bf16_t*)table, (long)ldt, rows,
                       (bf16_t*)pe, (long)ldpe, C, D);
  else
    hipLaunchKernelGGL(stream_advance_kernel<float>, dim3(1), dim3(256), 0, STREAM, counter, (const float*)table, (long)ldt, rows,
                       (float*)pe, (long)ldpe, C, D);
  return check_launch("smx_stream_advance");
}

extern "C" int smx_slot_begin(int dtype, int64_t* counters, const uint8_t* start, const void* table, int64_t ldt, int rows, void* pe,
                              int64_t ldpe, int B, int C, int D, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_slot_begin: bad dtype");
  SMX_REQUIRE(counters && start && (!pe || table), "smx_slot_begin: null pointer");
  SMX_REQUIRE(B > 0 && B <= 65535 && C >= 1 && C <= ST_CMAX && D > 0 && rows >= 0,
              "smx_slot_begin: 0 < B <= 65535, 1 <= C <= %d, D > 0 (B=%d C=%d D=%d)", ST_CMAX, B, C, D);
  SMX_REQUIRE(!pe || (ldt >= D && ldpe >= D), "smx_slot_begin: row strides must be >= D");
  dim3 grid(pe ? (unsigned)C : 1u, (unsigned)B);
  if (dtype == SMX_BF16)
    hipLaunchKernelGGL(slot_begin_kernel<bf16_t>, grid, dim3(256), 0, STREAM, counters, start, (const bf16_t*)table, (long)ldt, rows,
                       (bf16_t*)pe, (long)ldpe, C, D);
  else
    hipLaunchKernelGGL(slot_begin_kernel<float>, grid, dim3(256), 0, STREAM, counters, start, (const float*)table, (long)ldt, rows,
                       (float*)pe, (long)ldpe, C, D);
  return check_launch("smx_slot_begin");
}

extern "C" int smx_slot_advance(int64_t* counters, const int32_t* valid, int B, int C, void* stream) {
  SMX_REQUIRE(counters && valid, "smx_slot_advance: null pointer");
  SMX_REQUIRE(B > 0 && C >= 1 && C <= ST_CMAX, "smx_slot_advance: B > 0 and 1 <= C <= %d (B=%d C=%d)", ST_CMAX, B, C);
  hipLaunchKernelGGL(slot_advance_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, STREAM, counters, valid, B, C);
  return check_launch("smx_slot_advance");
}
