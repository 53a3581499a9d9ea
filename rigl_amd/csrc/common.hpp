// Shared host-side helpers for the C-ABI translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdarg.h>
#include <atomic>
#include <stdint.h>
#include <stdio.h>

#include "../../include/rigl_hip.h"

namespace rigl {

void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);

// Process-wide development knobs (rigl_tune_set): the run-time twin of the RIGL_* environment variables, for
// A/B runs inside one process.  Unknown keys read as the caller's default.
int tune_get(const char* key, int dflt);
// Per-call-site cache of a knob: valid until the next rigl_tune_set / rigl_tune_unset (a generation counter), so the
// launch paths read their knobs with two atomic loads instead of a mutex and a string scan.  Use through RIGL_TUNE.
struct TuneSite { std::atomic<uint64_t> gen{0}; std::atomic<int> value{0}; };
uint64_t tune_generation();
int tune_cached(TuneSite& site, const char* key, int dflt);
#define RIGL_TUNE(key, dflt) ([]() -> int { static ::rigl::TuneSite site__; return ::rigl::tune_cached(site__, key, dflt); }())

inline hipStream_t as_stream(rigl_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Checks the last launch.  hipGetLastError is cheap and does not synchronise.
#define RIGL_CHECK_LAUNCH(what)                                              \
  do {                                                                       \
    hipError_t e__ = hipGetLastError();                                      \
    if (e__ != hipSuccess)                                                   \
      return ::rigl::fail(RIGL_ELAUNCH, "%s: %s", what, hipGetErrorString(e__)); \
  } while (0)

#define RIGL_HIP(call)                                                       \
  do {                                                                       \
    hipError_t e__ = (call);                                                 \
    if (e__ != hipSuccess)                                                   \
      return ::rigl::fail(RIGL_ELAUNCH, "%s: %s", #call, hipGetErrorString(e__)); \
  } while (0)

// ---- optional per-launch timing (rigl_prof_*) -------------------------------
enum ProfKind { PROF_CONV_FWD = 0, PROF_CONV_DGRAD = 1, PROF_CONV_WGRAD = 2,
                PROF_PRUNE_REGROW = 3, PROF_SGD = 4, PROF_PACK = 5, PROF_CONV_BWD = 6, PROF_DEPTHWISE = 7,
                PROF_ADAM = 8, PROF_MAGPRUNE = 9 };
bool prof_enabled();
void prof_begin(int kind, hipStream_t s);
void prof_end(int kind, hipStream_t s);

// Per-kernel timing without extra queue packets: while profiling is on, K1 kernels are launched with
// hipExtLaunchKernelGGL, whose dispatch packet itself stamps a start / stop event pair (the
// hipEventRecord pairs of ProfScope put two barrier packets around every launch: measured 0.66 ms per
// ResNet-50 step for the 165 K1 launches).  The kernel family is the thread's current ProfFamily.
hipEvent_t prof_get_event();
void prof_add_pair(int kind, hipEvent_t a, hipEvent_t b);
int& prof_current_kind();
void prof_set_tag(const RiglConvDesc* d);      // the conv descriptor the following K1 launches of this thread belong to
struct ProfFamily {
  int prev;
  explicit ProfFamily(int k) : prev(prof_current_kind()) { prof_current_kind() = k; }
  ~ProfFamily() { prof_current_kind() = prev; }
};

struct ProfScope {
  int kind; hipStream_t s; bool on;
  ProfScope(int k, hipStream_t st) : kind(k), s(st), on(prof_enabled()) { if (on) prof_begin(kind, s); }
  ~ProfScope() { if (on) prof_end(kind, s); }
};

template <typename F, typename... Args>
inline void prof_launch(F kernel, dim3 grid, dim3 blk, unsigned lds, hipStream_t st, Args... args) {
  hipEvent_t a = prof_get_event(), b = prof_get_event();
  if (!a || !b) { hipLaunchKernelGGL(kernel, grid, blk, lds, st, args...); return; }
  hipExtLaunchKernelGGL(kernel, grid, blk, lds, st, a, b, 0, args...);
  prof_add_pair(prof_current_kind(), a, b);
}
#define RIGL_K_LAUNCH(kernel, grid, blk, lds, st, ...)                                      \
  do {                                                                                      \
    if (::rigl::prof_enabled()) ::rigl::prof_launch(kernel, grid, blk, lds, st, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel, grid, blk, lds, st, __VA_ARGS__);                       \
  } while (0)

// What every K1 entry point asks of a conv descriptor before it touches a pointer (conv.hip's bodies and the direct kernels
// of conv_ref.hip alike): positive dimensions, an output grid whose windows start inside the padded image, tensors below
// 2^30 elements.
inline int check_desc(const RiglConvDesc* d, const char* who) {
  if (!d) return fail(RIGL_EINVAL, "%s: NULL descriptor", who);
  if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->cin <= 0 || d->ho <= 0 || d->wo <= 0 || d->cout <= 0 || d->kh <= 0 ||
      d->kw <= 0 || d->stride_h <= 0 || d->stride_w <= 0 || d->pad_top < 0 || d->pad_left < 0)
    return fail(RIGL_EINVAL, "%s: non-positive dimension in descriptor", who);
  // every output pixel's window must start inside the padded image
  if ((d->ho - 1) * d->stride_h - d->pad_top >= d->h || (d->wo - 1) * d->stride_w - d->pad_left >= d->w)
    return fail(RIGL_EINVAL, "%s: output size inconsistent with input/stride/pad", who);
  const int64_t lim = (int64_t(1) << 30) - 1;   // bf16 tensors stay below 2^31 bytes (buffer descriptors)
  if ((int64_t)d->n * d->h * d->w * d->cin > lim || (int64_t)d->n * d->ho * d->wo * d->cout > lim ||
      (int64_t)d->kh * d->kw * d->cin * d->cout > lim)
    return fail(RIGL_EUNSUPPORTED, "%s: tensor exceeds 2^30 elements", who);
  return RIGL_OK;
}

inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- ReLU on packed bf16 pairs (the VGG convs: no batch norm between conv and ReLU) ----------------------------
// relu: every value with the sign bit set (negatives and -0) becomes +0; max(bf16(acc), 0) == bf16(max(acc, 0)).
__device__ __forceinline__ uint32_t relu_bf16x2(uint32_t v) {
  return v & ~(((v & 0x80008000u) >> 15) * 0xFFFFu);
}
// gate: v where x > 0 (sign clear and not zero), else +0 -- the ReLU derivative read off the ReLU's own output.
__device__ __forceinline__ uint32_t gate_bf16x2(uint32_t v, uint32_t x) {
  const uint32_t lo = (x & 0xFFFFu) - 1u < 0x7FFFu ? 0x0000FFFFu : 0u;
  const uint32_t hi = (x >> 16) - 1u < 0x7FFFu ? 0xFFFF0000u : 0u;
  return v & (lo | hi);
}
__device__ __forceinline__ uint4 relu_bf16x8(uint4 v) {
  return make_uint4(relu_bf16x2(v.x), relu_bf16x2(v.y), relu_bf16x2(v.z), relu_bf16x2(v.w));
}
__device__ __forceinline__ uint4 gate_bf16x8(uint4 v, uint4 x) {
  return make_uint4(gate_bf16x2(v.x, x.x), gate_bf16x2(v.y, x.y), gate_bf16x2(v.z, x.z), gate_bf16x2(v.w, x.w));
}

// ---- the batch norm's backward apply on one element: dx = a * (dz - b - xhat * c), xhat = (x - mean) * invstd, with
// a = gamma * invstd, b = mean(dz), c = mean(dz * xhat) (k_bwd_finalize's coef[3][C]) and dz the relu-masked output gradient.
// ONE statement of the arithmetic and its rounding points for bn.hip's k_bwd_apply and for the 1x1 backward that applies it
// on its dY load (bwd1x1.hpp): the library is built with -ffp-contract=off, so both kernels evaluate exactly these five
// operations in this order and the products are bit-identical.
__device__ __forceinline__ float bn_bwd_dx(float dz, float x, float mean, float invstd, float a, float b, float c) {
  const float xh = (x - mean) * invstd;
  return a * (dz - b - xh * c);
}

}  // namespace rigl
