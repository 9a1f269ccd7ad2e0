// optim.hip — the optimizer-side kernels behind summarymixing_amd.trainer that are not AdamW (gfx950, wave64):
//   smx_sgd_step     torch.optim.SGD (momentum, Nesterov, coupled weight decay, dampening 0) over a flat fp32 range, one pass,
//                    with the bf16 shadow refresh; 16 bytes per lane per access of p / g / buf, 8 bytes of shadows;
//   smx_lr_schedule  the recipes' per-update learning rate (Noam, warm-up + exponential decay) written into device memory by
//                    one thread, so that a captured training step follows its schedule on replay.
#include <math.h>

#include "smx_common.h"

namespace smx {

// one element of the update; the vector body and the scalar head / tail go through the same sequence of fused multiply-adds,
// so an element's result does not depend on which path it takes
__device__ __forceinline__ void sgd_one(float& p, float g, float& b, float lr, float mu, float wd, bool nesterov, float gs, bool has_buf) {
  const float gi = fmaf(wd, p, g * gs);
  float d = gi;
  if (has_buf) {
    b = fmaf(mu, b, gi);
    d = nesterov ? fmaf(mu, b, gi) : b;
  }
  p = fmaf(-lr, d, p);
}

// [0, head) and [head + 4 nvec, n) are scalar, the nvec float4 groups between them are 16-byte aligned in p, g and buf and
// 8-byte aligned in the shadows (the host checked that, or set head = n).  Grid-stride over both index spaces.
__global__ __launch_bounds__(256) void sgd_kernel(float* p, const float* g, float* buf, uint16_t* shadow, long n, long head,
                                                  float lr, const float* lr_dev, float mu, float wd, int nesterov, float gscale,
                                                  const float* gscale_dev) {
  // a clip factor of exactly 0 is smx_clip_factor's "non-finite gradient norm" verdict: skip the whole update (adamw_kernel)
  if (gscale_dev && gscale_dev[0] == 0.f) return;
  const float gs = gscale * (gscale_dev ? gscale_dev[0] : 1.f);
  if (lr_dev) lr = lr_dev[0];
  const bool has_buf = buf != nullptr, nest = nesterov != 0;
  const long nvec = (n - head) >> 2, tail0 = head + 4 * nvec, nscalar = head + (n - tail0);
  const long tid = blockIdx.x * 256L + threadIdx.x, stride = (long)gridDim.x * 256;
  for (long v = tid; v < nvec; v += stride) {
    const long i = head + 4 * v;
    float4 pv = *reinterpret_cast<const float4*>(p + i);
    const float4 gv = *reinterpret_cast<const float4*>(g + i);
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_buf) bv = *reinterpret_cast<const float4*>(buf + i);
    sgd_one(pv.x, gv.x, bv.x, lr, mu, wd, nest, gs, has_buf);
    sgd_one(pv.y, gv.y, bv.y, lr, mu, wd, nest, gs, has_buf);
    sgd_one(pv.z, gv.z, bv.z, lr, mu, wd, nest, gs, has_buf);
    sgd_one(pv.w, gv.w, bv.w, lr, mu, wd, nest, gs, has_buf);
    *reinterpret_cast<float4*>(p + i) = pv;
    if (has_buf) *reinterpret_cast<float4*>(buf + i) = bv;
    if (shadow) {
      uint2 s;
      s.x = pack_bf16x2(pv.x, pv.y);
      s.y = pack_bf16x2(pv.z, pv.w);
      *reinterpret_cast<uint2*>(shadow + i) = s;
    }
  }
  for (long s = tid; s < nscalar; s += stride) {
    const long i = s < head ? s : tail0 + (s - head);
    float pi = p[i], bi = has_buf ? buf[i] : 0.f;
    sgd_one(pi, g[i], bi, lr, mu, wd, nest, gs, has_buf);
    p[i] = pi;
    if (has_buf) buf[i] = bi;
    if (shadow) shadow[i] = (uint16_t)f32_to_bf16_bits(pi);
  }
}

// The rate of update t (counted from 1) in float64, stored as float32: what the recipes get by calling their scheduler once
// behind every optimizer step (include/smx.h has the definition).
__global__ void lr_schedule_kernel(int kind, double c0, double c1, double c2, double c3, double lr0, long step,
                                   const uint64_t* step_dev, float* out) {
  const double t = step_dev ? (double)step_dev[0] : (double)step;
  double lr = lr0;
  if (t >= 2.0) {
    if (kind == SMX_LR_NOAM) {
      const double n = t - 1.0, w = c1;
      const double norm = c2 > 0.0 ? 1.0 / sqrt(c2) : sqrt(w);
      const double up = n / (w * sqrt(w)), down = 1.0 / sqrt(n);
      lr = c0 * norm * (down < up ? down : up);
    } else {
      const double c = t - 2.0, w = c1;
      if (c < w) {
        lr = c0 * c / w;
      } else {
        const double d = c0 * pow(c3, (c - w) / c2);
        lr = d < c0 ? d : c0;
      }
    }
  }
  out[0] = (float)lr;
}

}  // namespace smx

using namespace smx;
#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" int smx_sgd_step(float* param, const float* grad, float* momentum_buf, void* shadow_bf16, int64_t n, float lr,
                            const float* lr_dev, float momentum, float weight_decay, int nesterov, float grad_scale,
                            const float* gscale_dev, void* stream) {
  SMX_REQUIRE(param && grad, "smx_sgd_step: bad arguments");
  SMX_REQUIRE(momentum >= 0.f, "smx_sgd_step: momentum < 0");
  SMX_REQUIRE(momentum == 0.f || momentum_buf, "smx_sgd_step: momentum > 0 needs a momentum buffer");
  SMX_REQUIRE(!nesterov || momentum > 0.f, "smx_sgd_step: nesterov needs momentum > 0");
  if (n <= 0) return SMX_OK;
  float* buf = momentum > 0.f ? momentum_buf : nullptr;
  const uintptr_t ap = reinterpret_cast<uintptr_t>(param), ag = reinterpret_cast<uintptr_t>(grad),
                  ab = reinterpret_cast<uintptr_t>(buf), as = reinterpret_cast<uintptr_t>(shadow_bf16);
  // the scalar head: the elements in front of param's first 16-byte boundary.  The vector body needs grad and the buffer at the
  // same offset from a boundary and the shadows 8-byte aligned behind the head (views of parallel flat buffers are); anything
  // else runs scalar as a whole
  long head = (long)(((16 - (ap & 15)) & 15) >> 2);
  const bool congruent = (ap & 3) == 0 && (ag & 15) == (ap & 15) && (!buf || (ab & 15) == (ap & 15)) &&
                         (!shadow_bf16 || ((as + 2 * (uintptr_t)head) & 7) == 0);
  if (!congruent || head > n) head = n;
  const long nvec = (n - head) >> 2, nscalar = n - 4 * nvec;
  const long work = nvec > nscalar ? nvec : nscalar;
  long blocks = (work + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > SMX_SGD_MAX_BLOCKS ? SMX_SGD_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)blocks), dim3(256), 0, STREAM, param, grad, buf, (uint16_t*)shadow_bf16, (long)n,
                     head, lr, lr_dev, momentum, weight_decay, nesterov, grad_scale, gscale_dev);
  return check_launch("smx_sgd_step");
}

extern "C" int smx_lr_schedule(int kind, double c0, double c1, double c2, double c3, double lr0, int64_t step,
                               const uint64_t* step_dev, float* lr_out, void* stream) {
  SMX_REQUIRE(lr_out, "smx_lr_schedule: null pointer");
  SMX_REQUIRE(kind == SMX_LR_NOAM || kind == SMX_LR_WARM_EXP_DECAY, "smx_lr_schedule: unknown kind %d", kind);
  SMX_REQUIRE(step > 0 || step_dev, "smx_lr_schedule: step <= 0 needs the device step counter (step_dev)");
  SMX_REQUIRE(c1 > 0.0, "smx_lr_schedule: the warm-up length must be positive");
  SMX_REQUIRE(kind != SMX_LR_WARM_EXP_DECAY || (c2 > 0.0 && c3 > 0.0), "smx_lr_schedule: total_steps and decay_factor must be positive");
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(1), 0, STREAM, kind, c0, c1, c2, c3, lr0, (long)step,
                     step > 0 ? nullptr : step_dev, lr_out);
  return check_launch("smx_lr_schedule");
}
