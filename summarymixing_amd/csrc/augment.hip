// augment.hip — the recipes' fea_augment (speechbrain.augment: SpectrogramDrop along time, SpectrogramDrop along frequency, Warping
// bicubic) as two launches: smx_specaug_draw fills an int32 parameter block on the device, smx_specaug_apply is a pure function
// of X and that block (one pass: read once, write once).  Block layout: include/smx.h.  Arithmetic spec: DESIGN.md §I.15.
#include "smx_common.h"

namespace smx {

#define STREAM reinterpret_cast<hipStream_t>(stream)

constexpr int SA_HDR = 8;                // header words of the block
constexpr int SA_CAP = 32;               // most drops per row and stage
constexpr int SA_MAXF = 1024;            // widest feature row
constexpr int SA_ROWS = 128;             // most output rows per workgroup (the launch picks the count: sa_tile_rows)
constexpr uint32_t SA_SALT = 0x5bd1e995u;  // this generator's salt (the dropout masks use none)

// ---- draw ---------------------------------------------------------------------------------------------------------------------
// One 32-bit hash per drawn value: a pure function of (seed, step counter, stream of values, index).  An integer on [0, range)
// is (h * range) >> 32.
__device__ __forceinline__ uint32_t sa_hash(uint64_t seed, uint32_t what, uint32_t idx) {
  return mix32(mix32(idx + what * 0x9E3779B9u) ^ mix32((uint32_t)seed + SA_SALT) ^ (uint32_t)(seed >> 32));
}
__device__ __forceinline__ int sa_int(uint32_t h, int lo, int hi_excl) {
  const uint32_t range = hi_excl > lo ? (uint32_t)(hi_excl - lo) : 1u;
  return lo + (int)(((uint64_t)h * range) >> 32);
}
enum { SA_N_TIME = 0, SA_N_FREQ = 1, SA_C = 2, SA_W = 3, SA_TPOS = 4, SA_TLEN = 5, SA_FPOS = 6, SA_FLEN = 7 };

struct DrawArgs {
  int B, T, F, stages;
  int t_len_lo, t_len_hi, t_cnt_lo, t_cnt_hi;
  int f_len_lo, f_len_hi, f_cnt_lo, f_cnt_hi;
  int window;
  uint64_t seed;
};

__global__ void __launch_bounds__(256) specaug_draw_kernel(int32_t* __restrict__ params, DrawArgs a, const uint64_t* __restrict__ epoch) {
  const uint64_t seed = epoch_seed(a.seed, epoch);
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int tcap = (a.stages & SMX_SPECAUG_TIME) ? a.t_cnt_hi : 0, fcap = (a.stages & SMX_SPECAUG_FREQ) ? a.f_cnt_hi : 0;
  if (tid == 0) {
    int flags = a.stages & (SMX_SPECAUG_TIME | SMX_SPECAUG_FREQ), c = 0, w = 0;
    if ((a.stages & SMX_SPECAUG_WARP) && a.T - a.window > a.window) {
      c = sa_int(sa_hash(seed, SA_C, 0), a.window, a.T - a.window);
      w = sa_int(sa_hash(seed, SA_W, 0), c - a.window + 1, c + a.window + 1);
      flags |= SMX_SPECAUG_WARP;
    }
    params[0] = flags;
    params[1] = c;
    params[2] = w;
    params[3] = tcap ? sa_int(sa_hash(seed, SA_N_TIME, 0), a.t_cnt_lo, a.t_cnt_hi + 1) : 0;
    params[4] = fcap ? sa_int(sa_hash(seed, SA_N_FREQ, 0), a.f_cnt_lo, a.f_cnt_hi + 1) : 0;
    params[5] = params[6] = params[7] = 0;
  }
  const int nt = a.B * tcap, nf = a.B * fcap;
  if (tid < nt) {
    params[SA_HDR + 2 * tid] = sa_int(sa_hash(seed, SA_TPOS, tid), 0, a.T);
    params[SA_HDR + 2 * tid + 1] = sa_int(sa_hash(seed, SA_TLEN, tid), a.t_len_lo, a.t_len_hi);
  }
  if (tid < nf) {
    params[SA_HDR + 2 * nt + 2 * tid] = sa_int(sa_hash(seed, SA_FPOS, tid), 0, a.F);
    params[SA_HDR + 2 * nt + 2 * tid + 1] = sa_int(sa_hash(seed, SA_FLEN, tid), a.f_len_lo, a.f_len_hi);
  }
}

// ---- apply --------------------------------------------------------------------------------------------------------------------
// V consecutive elements <-> V floats; V * sizeof(T) is 16 bytes on the vector path and one element on the scalar path.  The load is
// split from the unpacking so that the four gathers of an output element are issued together and waited for once.
template <typename T, int V>
struct SaVec;
template <>
struct SaVec<float, 4> {
  typedef float4 raw;
  static __device__ __forceinline__ void unpack(const raw& r, float (&f)[4]) { f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w; }
  static __device__ __forceinline__ raw pack(const float (&f)[4]) { return make_float4(f[0], f[1], f[2], f[3]); }
};
template <>
struct SaVec<float, 1> {
  typedef float raw;
  static __device__ __forceinline__ void unpack(const raw& r, float (&f)[1]) { f[0] = r; }
  static __device__ __forceinline__ raw pack(const float (&f)[1]) { return f[0]; }
};
template <>
struct SaVec<bf16_t, 8> {
  typedef uint4 raw;
  static __device__ __forceinline__ void unpack(const raw& r, float (&f)[8]) {
    const uint32_t u[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) { f[2 * q] = bf16_bits_to_f32(u[q] & 0xffffu); f[2 * q + 1] = bf16_bits_to_f32(u[q] >> 16); }
  }
  static __device__ __forceinline__ raw pack(const float (&f)[8]) {
    uint4 r;
    r.x = pack_bf16x2(f[0], f[1]); r.y = pack_bf16x2(f[2], f[3]); r.z = pack_bf16x2(f[4], f[5]); r.w = pack_bf16x2(f[6], f[7]);
    return r;
  }
};
template <>
struct SaVec<bf16_t, 1> {
  typedef uint16_t raw;
  static __device__ __forceinline__ void unpack(const raw& r, float (&f)[1]) { f[0] = bf16_bits_to_f32(r); }
  static __device__ __forceinline__ raw pack(const float (&f)[1]) { return (uint16_t)f32_to_bf16_bits(f[0]); }
};

// torch's cubic convolution coefficients (A = -0.75): c1 on |x| <= 1, c2 on 1 < |x| < 2
__device__ __forceinline__ float sa_c1(float x) { return ((1.25f * x - 2.25f) * x) * x + 1.0f; }
__device__ __forceinline__ float sa_c2(float x) { return ((-0.75f * x + 3.75f) * x - 6.0f) * x + 3.0f; }

// One workgroup: `R` (<= SA_ROWS) output rows of one utterance.  Phase 1 turns the block into this tile's plan in LDS: per output row the
// four source rows (-1: tap not loaded - it is dropped along time, or its weight is exactly zero) and their weights, and per column
// the frequency keep flag.  Phase 2 streams the tile: every (row, 16-byte column group) gathers its taps, accumulates in float32
// and rounds once.  A row whose position falls on a source row (every row when the warp is off) is a copy: its bits pass through.
template <typename T, int V>
__global__ void __launch_bounds__(256) specaug_apply_kernel(const T* __restrict__ X, int64_t ldx, T* __restrict__ Y, int64_t ldy,
                                                            const int32_t* __restrict__ params, int Tn, int F, int tcap, int fcap, int R) {
  __shared__ int4 s_src[SA_ROWS];
  __shared__ float4 s_wt[SA_ROWS];
  __shared__ int s_tdrop[2 * SA_CAP], s_fdrop[2 * SA_CAP];
  __shared__ unsigned char s_fkeep[SA_MAXF];
  const int b = blockIdx.y, t0 = blockIdx.x * R, tid = threadIdx.x;
  const int B = gridDim.y;
  // the whole block in one round of loads: the header through the scalar unit, this utterance's (pos, len) pairs up to the caps
  // (the counts in force are applied below, so no load waits for another)
  if (tid < 2 * tcap) s_tdrop[tid] = params[SA_HDR + 2 * (int64_t)b * tcap + tid];
  else if (tid >= 128 && tid - 128 < 2 * fcap) s_fdrop[tid - 128] = params[SA_HDR + 2 * (int64_t)B * tcap + 2 * (int64_t)b * fcap + (tid - 128)];
  const int flags = params[0], c = params[1], w = params[2];
  const bool warp = (flags & SMX_SPECAUG_WARP) && c >= 1 && c < Tn && w >= 1 && w < Tn;   // (anything else: no warp, never out of bounds)
  const int n_time = (flags & SMX_SPECAUG_TIME) ? min(max(params[3], 0), tcap) : 0;
  const int n_freq = (flags & SMX_SPECAUG_FREQ) ? min(max(params[4], 0), fcap) : 0;
  __syncthreads();
  for (int f = tid; f < F; f += 256) {
    int drop = 0;
    for (int i = 0; i < n_freq; ++i) drop |= (f >= s_fdrop[2 * i]) & (f - s_fdrop[2 * i] < s_fdrop[2 * i + 1]);
    s_fkeep[f] = drop ? 0 : 1;
  }
  if (tid < R && t0 + tid < Tn) {
    const int t = t0 + tid;
    int lo = 0, hi = Tn, i = t, rem = 0, den = 1;            // segment [lo, hi) of the source, tap base i, fraction rem / den
    if (warp) {
      int n_in, n_out, tt;
      if (t < w) { lo = 0; hi = c; n_in = c; n_out = w; tt = t; }
      else { lo = c; hi = Tn; n_in = Tn - c; n_out = Tn - w; tt = t - w; }
      if (n_out > 1) {
        const int64_t num = (int64_t)tt * (n_in - 1);
        den = n_out - 1;
        i = lo + (int)(num / den);
        rem = (int)(num % den);
      } else {
        i = lo;
      }
    }
    float wt[4] = {0.f, 1.f, 0.f, 0.f};
    if (rem != 0) {
      const float fr = (float)((double)rem / (double)den);   // correctly rounded, whatever -ffast-math makes of a float division
      wt[0] = sa_c2(fr + 1.0f); wt[1] = sa_c1(fr); wt[2] = sa_c1(1.0f - fr); wt[3] = sa_c2(2.0f - fr);
    }
    int src[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int s = min(max(i - 1 + k, lo), hi - 1);
      int drop = (rem == 0) & (k != 1);                      // a weight of exactly zero: nothing to load
      for (int d = 0; d < n_time; ++d) drop |= (s >= s_tdrop[2 * d]) & (s - s_tdrop[2 * d] < s_tdrop[2 * d + 1]);
      src[k] = drop ? -1 : s;
    }
    // a copy row (the position falls on source row src.y) is marked by src.x = -2: its bits pass through
    s_src[tid] = make_int4(rem == 0 ? -2 : src[0], src[1], src[2], src[3]);
    s_wt[tid] = make_float4(wt[0], wt[1], wt[2], wt[3]);
  }
  __syncthreads();
  const int nvec = F / V, rows = min(R, Tn - t0);
  const T* Xb = X + (int64_t)b * Tn * ldx;
  T* Yb = Y + ((int64_t)b * Tn + t0) * ldy;
  for (int item = tid; item < rows * nvec; item += 256) {
    const int r = item / nvec, f0 = (item - r * nvec) * V;
    const int4 sv = s_src[r];
    const float4 wv = s_wt[r];
    const int src[4] = {sv.x, sv.y, sv.z, sv.w};
    const float wt[4] = {wv.x, wv.y, wv.z, wv.w};
    typedef typename SaVec<T, V>::raw raw_t;
    raw_t raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                            // the gathers first, all in flight together; a dropped tap is not loaded
      raw[k] = raw_t();
      if (src[k] >= 0) raw[k] = *reinterpret_cast<const raw_t*>(Xb + (int64_t)src[k] * ldx + f0);
    }
    float x[4][V];
#pragma unroll
    for (int k = 0; k < 4; ++k) SaVec<T, V>::unpack(raw[k], x[k]);
    float acc[V];
    if (sv.x == -2) {
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = x[1][j];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) a = fmaf(wt[k], x[k][j], a);     // (an unloaded tap adds a zero: the sum is unchanged)
        acc[j] = (__float_as_uint(a) << 1) == 0u ? __uint_as_float(0u) : a;   // a zero sum is stored as +0 whichever taps were skipped
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = s_fkeep[f0 + j] ? acc[j] : __uint_as_float(0u);
    *reinterpret_cast<raw_t*>(Yb + (int64_t)r * ldy + f0) = SaVec<T, V>::pack(acc);
  }
}

// Rows per workgroup: the largest tile of up to four 256-item sweeps (an item = one row x one 16-byte column group) that leaves
// the fewest idle lanes in its last sweep.  F = 80: 51 rows in float32 (20 groups a row, 1020 items), 51 rows in bfloat16 (10 groups,
// 510 items = two full sweeps; 32 rows were 320 items, a second sweep three quarters idle).
// A workgroup pays a fixed chain of latencies (block, plan, first gather) whatever its tile, so while the grid stays above 2048
// workgroups (8 per CU) the tile doubles: at (128, 2000, 80) 102 rows took the bfloat16 pass from 3.0 to the float32 pass's rate.
static int sa_tile_rows(int nvec, int B, int T) {
  int best = 1;
  double best_eff = 0.0;
  for (int k = 1; k <= 4; ++k) {
    int r = 256 * k / nvec;
    r = r < 1 ? 1 : (r > 64 ? 64 : r);
    const int items = r * nvec;
    const double eff = (double)items / (256.0 * ((items + 255) / 256));
    if (eff >= best_eff) { best_eff = eff; best = r; }
  }
  while (2 * best <= SA_ROWS && (long)B * ((T + 2 * best - 1) / (2 * best)) >= 2048) best *= 2;
  return best;
}

}  // namespace smx

using namespace smx;

extern "C" size_t smx_specaug_params_bytes(int B, int n_time_cap, int n_freq_cap) {
  if (B <= 0 || n_time_cap < 0 || n_freq_cap < 0 || n_time_cap > SA_CAP || n_freq_cap > SA_CAP) return 0;
  return sizeof(int32_t) * ((size_t)SA_HDR + 2 * (size_t)B * ((size_t)n_time_cap + (size_t)n_freq_cap));
}

extern "C" int smx_specaug_draw(int32_t* params, int B, int T, int F, int stages, int t_len_lo, int t_len_hi, int t_cnt_lo,
                                int t_cnt_hi, int f_len_lo, int f_len_hi, int f_cnt_lo, int f_cnt_hi, int warp_window,
                                uint64_t seed, const uint64_t* epoch, void* stream) {
  SMX_REQUIRE(params && B > 0 && T > 0 && F > 0, "smx_specaug_draw: null block or non-positive sizes");
  SMX_REQUIRE(stages >= 0 && stages <= (SMX_SPECAUG_WARP | SMX_SPECAUG_TIME | SMX_SPECAUG_FREQ), "smx_specaug_draw: unknown stage bits");
  if (stages & SMX_SPECAUG_TIME) {
    SMX_REQUIRE(0 <= t_cnt_lo && t_cnt_lo <= t_cnt_hi && 0 <= t_len_lo && t_len_lo < t_len_hi, "smx_specaug_draw: bad time-drop ranges");
    if (t_cnt_hi > SA_CAP) return fail(SMX_EUNSUPPORTED, "smx_specaug_draw: at most %d time drops per row", SA_CAP);
  }
  if (stages & SMX_SPECAUG_FREQ) {
    SMX_REQUIRE(0 <= f_cnt_lo && f_cnt_lo <= f_cnt_hi && 0 <= f_len_lo && f_len_lo < f_len_hi, "smx_specaug_draw: bad frequency-drop ranges");
    if (f_cnt_hi > SA_CAP) return fail(SMX_EUNSUPPORTED, "smx_specaug_draw: at most %d frequency drops per row", SA_CAP);
  }
  if (stages & SMX_SPECAUG_WARP) SMX_REQUIRE(warp_window >= 1, "smx_specaug_draw: warp window < 1");
  const int tcap = (stages & SMX_SPECAUG_TIME) ? t_cnt_hi : 0, fcap = (stages & SMX_SPECAUG_FREQ) ? f_cnt_hi : 0;
  const long n = (long)B * (tcap > fcap ? tcap : fcap);
  DrawArgs a = {B, T, F, stages, t_len_lo, t_len_hi, t_cnt_lo, t_cnt_hi, f_len_lo, f_len_hi, f_cnt_lo, f_cnt_hi, warp_window, seed};
  hipLaunchKernelGGL(specaug_draw_kernel, dim3((unsigned)((n > 0 ? n : 1) + 255) / 256), dim3(256), 0, STREAM, params, a, epoch);
  return check_launch("smx_specaug_draw");
}

extern "C" int smx_specaug_apply(int dtype, const void* X, int64_t ldx, void* Y, int64_t ldy, const int32_t* params, int B, int T,
                                 int F, int n_time_cap, int n_freq_cap, void* stream) {
  SMX_REQUIRE(X && Y && params && B > 0 && T > 0 && F > 0, "smx_specaug_apply: null pointer or non-positive sizes");
  SMX_REQUIRE((dtype == SMX_F32 || dtype == SMX_BF16) && ldx >= F && ldy >= F && n_time_cap >= 0 && n_freq_cap >= 0,
              "smx_specaug_apply: bad dtype, leading dimension or cap");
  if (F > SA_MAXF) return fail(SMX_EUNSUPPORTED, "smx_specaug_apply: F = %d > %d", F, SA_MAXF);
  if (n_time_cap > SA_CAP || n_freq_cap > SA_CAP) return fail(SMX_EUNSUPPORTED, "smx_specaug_apply: caps above %d", SA_CAP);
  if (X == Y) return fail(SMX_EUNSUPPORTED, "smx_specaug_apply: in place (X == Y) is not supported: rows are gathered");
  if (B > 65535) return fail(SMX_EUNSUPPORTED, "smx_specaug_apply: B = %d > 65535", B);
  dispatch_dtype(dtype, [&](auto tag) {
    using Tt = decltype(tag);
    constexpr int V = 16 / sizeof(Tt);
    const bool vec = F % V == 0 && ldx % V == 0 && ldy % V == 0 && aligned16(X) && aligned16(Y);
    const int R = sa_tile_rows(vec ? F / V : F, B, T);
    const dim3 grid((T + R - 1) / R, B);
    if (vec) hipLaunchKernelGGL((specaug_apply_kernel<Tt, V>), grid, dim3(256), 0, STREAM, (const Tt*)X, ldx, (Tt*)Y, ldy, params, T, F, n_time_cap, n_freq_cap, R);
    else hipLaunchKernelGGL((specaug_apply_kernel<Tt, 1>), grid, dim3(256), 0, STREAM, (const Tt*)X, ldx, (Tt*)Y, ldy, params, T, F, n_time_cap, n_freq_cap, R);
  });
  return check_launch("smx_specaug_apply");
}
