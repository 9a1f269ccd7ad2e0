// lstm.hip — the transducer's prediction network (recipe keys `emb`, `dec`: speechbrain.nnet.embedding.Embedding with
// consider_as_one_hot and speechbrain.nnet.RNN.LSTM, one layer, unidirectional, batch first), gfx950 only.
//
// One launch per time step, all on the caller's stream (a captured step is a plain chain).  A workgroup owns a 16 (batch rows) x 16
// (hidden units) tile of the state and has four waves, one per gate (torch's order i, f, g, o): wave w multiplies the 16 rows of
// h_{u-1} with the 16 rows w H + j of W_hh on the MFMA (16x16x32 bf16 / 16x16x4 f32, operands straight from L2: W_hh is 2 MB at
// H = 512 and every workgroup reads 1/32 of it), the four tiles meet in LDS and thread (b, j) finishes its cell in fp32.  The
// backward step has the same shape: wave w reduces over gate w's slice of dgates_{u+1} against W_hh^T.  Batch rows beyond B of
// the last tile are computed from row B - 1 and never stored.  Every sum has a fixed order and nothing is atomic: values are bit-reproducible.
// The cell itself (lstm_cell, lstm_cell_bwd), the forward's four gate tiles (gate_tiles) and the one-hot input (onehot_col,
// onehot_gate_input) live in lstm_tile.h: greedy.hip's masked step and lstm_step.hip's one-launch step compute the same cell from them.
#include "lstm_tile.h"

namespace smx {

struct LstmFwdStep {
  const float* gx; long ld_gx;          // this step's input contribution (+ both biases), (B, 4H) rows ld_gx apart
  const void* hp; long ld_hp;           // h_{u-1} (null: zeros)
  const float* cp; long ld_cp;          // c_{u-1} (null: zeros)
  const void* Whh;                      // (4H, H)
  void* y; long ld_y;                   // h_u
  void* hprev0; void* hnext; long ld_hn;  // the backward's H_prev image: slot u (written from hp at u = 0 only) and slot u + 1
  float* gates; long ld_g;              // the activated gates of this step (null: inference)
  float* csave; long ld_cs;             // c_u kept for the backward (null: inference)
  float* crun;                          // (B, H) running cell state, c_n after the last step
  void* hn;                             // (B, H) h_n, written by the last step only (else null)
  int B, H;
};

template <typename T>
__global__ __launch_bounds__(256) void lstm_step_fwd_kernel(LstmFwdStep s) {
  __shared__ float red[4][16][17];
  const int H = s.H, j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const T* hp = reinterpret_cast<const T*>(s.hp);
  gate_tiles(red, hp, s.ld_hp, s.Whh, H, s.B, b0, j0);
  const int bb = threadIdx.x >> 4, jj = threadIdx.x & 15, b = b0 + bb, j = j0 + jj;
  if (b >= s.B) return;
  const float* gx = s.gx + (long)b * s.ld_gx;
  const float z[4] = {red[0][bb][jj] + gx[j], red[1][bb][jj] + gx[H + j], red[2][bb][jj] + gx[2 * H + j], red[3][bb][jj] + gx[3 * H + j]};
  float g[4], c;
  const T h = from_f32<T>(lstm_cell(z, s.cp ? s.cp[(long)b * s.ld_cp + j] : 0.f, g, c));
  reinterpret_cast<T*>(s.y)[(long)b * s.ld_y + j] = h;
  if (s.hprev0) reinterpret_cast<T*>(s.hprev0)[(long)b * s.ld_hn + j] = hp ? hp[(long)b * s.ld_hp + j] : from_f32<T>(0.f);
  if (s.hnext) reinterpret_cast<T*>(s.hnext)[(long)b * s.ld_hn + j] = h;
  if (s.gates) {
    float* ga = s.gates + (long)b * s.ld_g;
    ga[j] = g[0]; ga[H + j] = g[1]; ga[2 * H + j] = g[2]; ga[3 * H + j] = g[3];
  }
  if (s.csave) s.csave[(long)b * s.ld_cs + j] = c;
  s.crun[(long)b * H + j] = c;
  if (s.hn) reinterpret_cast<T*>(s.hn)[(long)b * H + j] = h;
}

struct LstmBwdStep {
  const void* dgn; long ld_dgn;         // dgates_{u+1} (null at the last step: no recurrent gradient yet)
  const void* WhhT;                     // (H, 4H) = W_hh^T
  const void* dy; long ld_dy;           // the gradient of h_u from above (null: none)
  const float* dhn;                     // (B, H) gradient of h_n (last step only, else null)
  const float* dc_in;                   // (B, H) gradient of c_u carried down (null: zeros)
  float* dc;                            // (B, H) <- gradient of c_{u-1}
  const float* gates; long ld_g;
  const float* c; long ld_c;
  const float* cp; long ld_cp;          // c_{u-1} (null: zeros)
  void* dg; long ld_dg;                 // -> dgates_u, the operand dtype
  float* dh0;                           // != null: the closing launch - only dh0 = dgates_0 . W_hh is written
  int B, H;
};

template <typename T>
__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(LstmBwdStep s) {
  __shared__ float red[4][16][17];
  const int H = s.H, j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const T* dgn = reinterpret_cast<const T*>(s.dgn);
  lstm_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (dgn) {                                                                  // (uniform)
    const T* a_row = dgn + (long)min(b0 + r, s.B - 1) * s.ld_dgn + (long)w * H;
    const T* b_row = reinterpret_cast<const T*>(s.WhhT) + (long)(j0 + r) * 4 * H + (long)w * H;
    acc = tile_dot(a_row, b_row, H, q);
  }
  gate_tile_to_lds(red, acc, w, q, r);
  __syncthreads();
  const int bb = threadIdx.x >> 4, jj = threadIdx.x & 15, b = b0 + bb, j = j0 + jj;
  if (b >= s.B) return;
  float dh = (red[0][bb][jj] + red[1][bb][jj]) + (red[2][bb][jj] + red[3][bb][jj]);
  if (s.dh0) {
    s.dh0[(long)b * H + j] = dh;
    return;
  }
  if (s.dy) dh += to_f32(reinterpret_cast<const T*>(s.dy)[(long)b * s.ld_dy + j]);
  if (s.dhn) dh += s.dhn[(long)b * H + j];
  const float* ga = s.gates + (long)b * s.ld_g;
  const float g[4] = {ga[j], ga[H + j], ga[2 * H + j], ga[3 * H + j]};
  float dz[4];
  s.dc[(long)b * H + j] = lstm_cell_bwd(g, s.c[(long)b * s.ld_c + j], s.cp ? s.cp[(long)b * s.ld_cp + j] : 0.f, dh,
                                        s.dc_in ? s.dc_in[(long)b * H + j] : 0.f, dz);
  T* dg = reinterpret_cast<T*>(s.dg) + (long)b * s.ld_dg;
#pragma unroll
  for (int i = 0; i < 4; ++i) dg[i * H + j] = from_f32<T>(dz[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void onehot_rows_kernel(const int32_t* __restrict__ tokens, T* __restrict__ Y, long ldy, int V, int blank) {
  const int r = blockIdx.x;
  const int col = onehot_col(tokens[r], V, blank);
  T* y = Y + (long)r * ldy;
  for (int c = threadIdx.x; c < V - 1; c += 256) y[c] = from_f32<T>(c == col ? 1.f : 0.f);
}

// Gx[r, n] = keep[r] W_ih^T[col(token[r]), n] + bias[n]; a thread owns four consecutive gate columns
template <typename T>
__global__ __launch_bounds__(256) void onehot_gates_fwd_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ keep,
                                                               const T* __restrict__ WT, long ldw, const float* __restrict__ bias,
                                                               float* __restrict__ Gx, int V, int blank, int G) {
  const int r = blockIdx.x, n = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (n >= G) return;
  const int col = onehot_col(tokens[r], V, blank);
  const float k = keep ? keep[r] : 1.f;
  float w[4] = {0.f, 0.f, 0.f, 0.f};
  if (col >= 0) load4(WT + (long)col * ldw + n, w);
  const float4 bq = *reinterpret_cast<const float4*>(bias + n);
  float4 o;
  o.x = onehot_gate_input(k, w[0], bq.x); o.y = onehot_gate_input(k, w[1], bq.y);
  o.z = onehot_gate_input(k, w[2], bq.z); o.w = onehot_gate_input(k, w[3], bq.w);
  *reinterpret_cast<float4*>(Gx + (long)r * G + n) = o;
}

// dW_ih[n, col] += sum over the rows r' with token[r'] = token[r] of keep[r'] dgates[r', n], in ascending r': the workgroup of the
// FIRST row that carries a token owns that column of dW_ih and walks the later rows in order (no atomics; a fixed order per owned
// gate column).  The other workgroups leave at once.  Every workgroup scans the tokens before its row and an owner those after it,
// so the token reads grow with rows^2 (the gradient reads with rows): sized for the prediction network's B (U + 1) of a few
// thousand tokens (2000 rows: ~2 M token reads per 1024 gate columns, L2 hits), not for an encoder-sized row count.  The final
// adds are lddw floats apart - 4 per thread, once per owned column.
template <typename T>
__global__ __launch_bounds__(256) void onehot_gates_wgrad_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ keep,
                                                                 const T* __restrict__ dG, long lddg, float* __restrict__ dW, long lddw,
                                                                 int rows, int V, int blank, int G) {
  const int r = blockIdx.x;
  const int tok = tokens[r];
  const int col = onehot_col(tok, V, blank);
  if (col < 0) return;                                                       // (uniform)
  int seen = 0;
  for (int p = threadIdx.x; p < r; p += 256) seen |= (tokens[p] == tok);
  if (__syncthreads_or(seen)) return;
  const int n = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (n >= G) return;
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int p = r; p < rows; ++p) {
    if (tokens[p] != tok) continue;                                          // (uniform)
    const float k = keep ? keep[p] : 1.f;
    float g[4];
    load4(dG + (long)p * lddg + n, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] += k * g[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) dW[(long)(n + i) * lddw + col] += sum[i];
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_lstm_ok(int dtype, int H) { return (dtype == SMX_F32 || dtype == SMX_BF16) && lstm_h_ok(H) ? 1 : 0; }

extern "C" int smx_lstm_fwd(int dtype, const float* Gx, const void* Whh, const void* h0, const float* c0, void* Y, void* Hprev,
                            float* gates, float* C, void* hn, float* cn, int B, int U, int H, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_lstm_fwd: bad dtype %d", dtype);
  SMX_REQUIRE(Gx && Whh && Y && hn && cn, "smx_lstm_fwd: null pointer");
  SMX_REQUIRE(B >= 0 && U >= 1 && H >= 1 && B <= 65535 * 16, "smx_lstm_fwd: bad sizes B=%d U=%d H=%d", B, U, H);
  SMX_REQUIRE((gates != nullptr) == (C != nullptr), "smx_lstm_fwd: gates and C are saved together");
  if (!lstm_h_ok(H)) return fail(SMX_EUNSUPPORTED, "smx_lstm_fwd: H must be a multiple of 32 in [32, %d], got %d", LSTM_H_MAX, H);
  if (!aligned16(Whh) || !aligned16(Y) || (h0 && !aligned16(h0)))
    return fail(SMX_EUNSUPPORTED, "smx_lstm_fwd: W_hh, h0 and Y must be 16-byte aligned");
  if (B == 0) return SMX_OK;
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  const long UH = (long)U * H;
  const dim3 grid(H / 16, (B + 15) / 16);
  for (int u = 0; u < U; ++u) {
    LstmFwdStep s;
    s.gx = Gx + (long)u * 4 * H; s.ld_gx = 4 * UH;
    if (u == 0) { s.hp = h0; s.ld_hp = H; s.cp = c0; s.ld_cp = H; }
    else { s.hp = (const char*)Y + (size_t)(u - 1) * H * es; s.ld_hp = UH; s.cp = cn; s.ld_cp = H; }
    s.Whh = Whh;
    s.y = (char*)Y + (size_t)u * H * es; s.ld_y = UH;
    s.hprev0 = (Hprev && u == 0) ? Hprev : nullptr;
    s.hnext = (Hprev && u + 1 < U) ? (char*)Hprev + (size_t)(u + 1) * H * es : nullptr;
    s.ld_hn = UH;
    s.gates = gates ? gates + (long)u * 4 * H : nullptr; s.ld_g = 4 * UH;
    s.csave = C ? C + (long)u * H : nullptr; s.ld_cs = UH;
    s.crun = cn;
    s.hn = u == U - 1 ? hn : nullptr;
    s.B = B; s.H = H;
    dispatch_dtype(dtype, [&](auto tag) { hipLaunchKernelGGL(lstm_step_fwd_kernel<decltype(tag)>, grid, dim3(256), 0, STREAM, s); });
  }
  return check_launch("smx_lstm_fwd");
}

extern "C" int smx_lstm_bwd(int dtype, const void* dY, const float* dhn, const float* dcn, const void* WhhT, const float* gates,
                            const float* C, const float* c0, void* dG, float* dc0, float* dh0, int B, int U, int H, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_lstm_bwd: bad dtype %d", dtype);
  SMX_REQUIRE(WhhT && gates && C && dG && dc0 && dh0, "smx_lstm_bwd: null pointer");
  SMX_REQUIRE(B >= 0 && U >= 1 && H >= 1 && B <= 65535 * 16, "smx_lstm_bwd: bad sizes B=%d U=%d H=%d", B, U, H);
  if (!lstm_h_ok(H)) return fail(SMX_EUNSUPPORTED, "smx_lstm_bwd: H must be a multiple of 32 in [32, %d], got %d", LSTM_H_MAX, H);
  if (!aligned16(WhhT) || !aligned16(dG)) return fail(SMX_EUNSUPPORTED, "smx_lstm_bwd: W_hh^T and dgates must be 16-byte aligned");
  if (B == 0) return SMX_OK;
  const size_t es = dtype == SMX_BF16 ? 2 : 4;
  const long UH = (long)U * H;
  const dim3 grid(H / 16, (B + 15) / 16);
  for (int u = U - 1; u >= -1; --u) {
    LstmBwdStep s;
    memset(&s, 0, sizeof(s));
    s.WhhT = WhhT; s.B = B; s.H = H;
    s.dgn = u + 1 < U ? (const char*)dG + (size_t)(u + 1) * 4 * H * es : nullptr; s.ld_dgn = 4 * UH;
    if (u < 0) {
      s.dh0 = dh0;
    } else {
      s.dy = dY ? (const char*)dY + (size_t)u * H * es : nullptr; s.ld_dy = UH;
      s.dhn = u == U - 1 ? dhn : nullptr;
      s.dc_in = u == U - 1 ? dcn : dc0;
      s.dc = dc0;
      s.gates = gates + (long)u * 4 * H; s.ld_g = 4 * UH;
      s.c = C + (long)u * H; s.ld_c = UH;
      if (u == 0) { s.cp = c0; s.ld_cp = H; }
      else { s.cp = C + (long)(u - 1) * H; s.ld_cp = UH; }
      s.dg = (char*)dG + (size_t)u * 4 * H * es; s.ld_dg = 4 * UH;
    }
    dispatch_dtype(dtype, [&](auto tag) { hipLaunchKernelGGL(lstm_step_bwd_kernel<decltype(tag)>, grid, dim3(256), 0, STREAM, s); });
  }
  return check_launch("smx_lstm_bwd");
}

extern "C" int smx_onehot_rows(int dtype, const int32_t* tokens, void* Y, int64_t ldy, int rows, int V, int blank, void* stream) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "smx_onehot_rows: bad dtype %d", dtype);
  SMX_REQUIRE(tokens && Y, "smx_onehot_rows: null pointer");
  SMX_REQUIRE(rows >= 0 && V >= 2 && blank >= 0 && blank < V && ldy >= V - 1, "smx_onehot_rows: bad sizes rows=%d V=%d blank=%d", rows, V, blank);
  if (rows == 0) return SMX_OK;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(onehot_rows_kernel<T>, dim3(rows), dim3(256), 0, STREAM, tokens, (T*)Y, (long)ldy, V, blank);
  });
  return check_launch("smx_onehot_rows");
}

static int onehot_gates_check(const char* what, int dtype, int rows, int V, int blank, int G, int64_t ld) {
  SMX_REQUIRE(dtype == SMX_F32 || dtype == SMX_BF16, "%s: bad dtype %d", what, dtype);
  SMX_REQUIRE(rows >= 0 && V >= 2 && blank >= 0 && blank < V && G >= 4 && ld >= G, "%s: bad sizes rows=%d V=%d blank=%d G=%d", what, rows, V, blank, G);
  if (G % 4 != 0 || ld % 4 != 0 || G > 65535 * 1024) return fail(SMX_EUNSUPPORTED, "%s: the gate width and its leading dimension must be multiples of 4", what);
  return SMX_OK;
}

extern "C" int smx_onehot_gates_fwd(int dtype, const int32_t* tokens, const float* keep, const void* WihT, int64_t ldw, const float* bias,
                                    float* Gx, int rows, int V, int blank, int G, void* stream) {
  SMX_REQUIRE(tokens && WihT && bias && Gx, "smx_onehot_gates_fwd: null pointer");
  const int rc = onehot_gates_check("smx_onehot_gates_fwd", dtype, rows, V, blank, G, ldw);
  if (rc != SMX_OK) return rc;
  if (!aligned16(WihT) || !aligned16(bias) || !aligned16(Gx)) return fail(SMX_EUNSUPPORTED, "smx_onehot_gates_fwd: operands must be 16-byte aligned");
  if (rows == 0) return SMX_OK;
  const dim3 grid(rows, (G + 1023) / 1024);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(onehot_gates_fwd_kernel<T>, grid, dim3(256), 0, STREAM, tokens, keep, (const T*)WihT, (long)ldw, bias, Gx, V, blank, G);
  });
  return check_launch("smx_onehot_gates_fwd");
}

extern "C" int smx_onehot_gates_wgrad(int dtype, const int32_t* tokens, const float* keep, const void* dG, int64_t lddg, float* dWih,
                                      int64_t lddw, int rows, int V, int blank, int G, void* stream) {
  SMX_REQUIRE(tokens && dG && dWih, "smx_onehot_gates_wgrad: null pointer");
  const int rc = onehot_gates_check("smx_onehot_gates_wgrad", dtype, rows, V, blank, G, lddg);
  if (rc != SMX_OK) return rc;
  SMX_REQUIRE(lddw >= V - 1, "smx_onehot_gates_wgrad: dW_ih rows hold V - 1 columns");
  if (!aligned16(dG)) return fail(SMX_EUNSUPPORTED, "smx_onehot_gates_wgrad: dgates must be 16-byte aligned");
  if (rows == 0) return SMX_OK;
  const dim3 grid(rows, (G + 1023) / 1024);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(onehot_gates_wgrad_kernel<T>, grid, dim3(256), 0, STREAM, tokens, keep, (const T*)dG, (long)lddg, dWih, (long)lddw, rows, V, blank, G);
  });
  return check_launch("smx_onehot_gates_wgrad");
}
