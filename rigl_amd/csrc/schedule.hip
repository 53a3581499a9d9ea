// The learning-rate schedule on the device: one single-lane kernel evaluates the segment table at the device step counter,
// writes the rate for this step's update kernels (rigl_masked_sgd_momentum_dlr / rigl_masked_adam_dlr) and advances the
// counter -- all inside whatever is captured, so a replayed graph trains at the schedule's current rate.
//   rigl_lr_schedule_step : *lr_out = f(*step);  *step += 1
#include "common.hpp"

#include <cmath>

// Bit-exact parity with the host twin (rigl_amd/schedules.py): every fp32 operation is rounded separately.
#pragma clang fp contract(off)

namespace rigl {
namespace klr {

// Only the ACTIVE segment is evaluated (the ResNet chain's warm-up divides by its start epoch 0 and is never selected).
__global__ void k_lr_schedule_step(RiglLrSchedule S, int32_t* __restrict__ step, float* __restrict__ lr_out) {
  if (threadIdx.x != 0) return;
  const int32_t s = *step;
  float x = (float)s;                                                // tf.cast(global_step, tf.float32): RNE
  if (S.domain == RIGL_LR_DOMAIN_EPOCH) x = __fdiv_rn(x, S.steps_per_epoch);
  int a = 0;
  for (int i = 1; i < S.n_seg; ++i) {
    const bool below = S.domain == RIGL_LR_DOMAIN_EPOCH ? x < S.seg[i].start : s < S.seg[i].start_step;
    if (!below) a = i;                                               // the LAST segment with !(x < start)
  }
  const RiglLrSegment g = S.seg[a];
  float lr = g.c;
  if (g.kind == RIGL_LR_WARMUP) {
    lr = __fdiv_rn(__fmul_rn(g.c, x), g.d);
  } else if (g.kind == RIGL_LR_COSINE) {
    const float frac = __fdiv_rn(__fsub_rn(__fdiv_rn(x, g.d), g.sum_r), g.len);
    const float t = __fmul_rn(3.14159274101257324f, frac);           // f32(pi) * completed_fraction, rounded
    const float cs = (float)cos((double)t);                          // double cosine, rounded once
    lr = __fmul_rn(g.c, __fmul_rn(__fmul_rn(0.5f, g.m_fac), __fadd_rn(1.0f, cs)));
  }
  *lr_out = lr;
  *step = (int32_t)((uint32_t)s + 1u);                               // int32 wrap-around, as k_dropout_advance
}

}  // namespace klr
}  // namespace rigl

extern "C" {

int rigl_lr_schedule_step(const RiglLrSchedule* sched, int32_t* step, float* lr_out, rigl_stream_t stream) {
  using namespace rigl;
  if (!sched || !step || !lr_out) return fail(RIGL_EINVAL, "rigl_lr_schedule_step: NULL sched / step / lr_out");
  if (((uintptr_t)sched | (uintptr_t)step | (uintptr_t)lr_out) & 3u)
    return fail(RIGL_EINVAL, "rigl_lr_schedule_step: sched / step / lr_out not 4-byte aligned");
  if (sched->n_seg < 1 || sched->n_seg > RIGL_LR_MAX_SEGMENTS)
    return fail(RIGL_EINVAL, "rigl_lr_schedule_step: n_seg %d outside 1..%d", sched->n_seg, RIGL_LR_MAX_SEGMENTS);
  const bool epoch = sched->domain == RIGL_LR_DOMAIN_EPOCH;
  if (!epoch && sched->domain != RIGL_LR_DOMAIN_STEP)
    return fail(RIGL_EINVAL, "rigl_lr_schedule_step: unknown domain %d", sched->domain);
  if (epoch && !(std::isfinite(sched->steps_per_epoch) && sched->steps_per_epoch > 0.0f))
    return fail(RIGL_EINVAL, "rigl_lr_schedule_step: steps_per_epoch must be finite and > 0, got %g",
                (double)sched->steps_per_epoch);
  for (int i = 0; i < sched->n_seg; ++i) {
    const RiglLrSegment& g = sched->seg[i];
    if (g.kind != RIGL_LR_CONST && g.kind != RIGL_LR_WARMUP && g.kind != RIGL_LR_COSINE)
      return fail(RIGL_EINVAL, "rigl_lr_schedule_step: segment %d: unknown kind %d", i, g.kind);
    if (g.kind == RIGL_LR_COSINE && !(g.len > 0.0f))
      return fail(RIGL_EINVAL, "rigl_lr_schedule_step: segment %d: COSINE len must be > 0, got %g", i, (double)g.len);
    if (i > 0) {
      const RiglLrSegment& p = sched->seg[i - 1];
      if (epoch ? !(p.start <= g.start) : !(p.start_step <= g.start_step))
        return fail(RIGL_EINVAL, "rigl_lr_schedule_step: the start of segment %d is below that of segment %d", i, i - 1);
    }
  }
  hipLaunchKernelGGL(klr::k_lr_schedule_step, dim3(1), dim3(64), 0, as_stream(stream), *sched, step, lr_out);
  RIGL_CHECK_LAUNCH("rigl_lr_schedule_step");
  return RIGL_OK;
}

}  // extern "C"
