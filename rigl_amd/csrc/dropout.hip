// Dropout of the CIFAR WideResNet (rigl/cifar_resnet/resnet_model.py:224-231: bn -> relu -> Dropout(droprate) -> conv2),
// TF's  keep_mask = random_uniform(shape) >= rate;  y = x * 1/(1-rate) * keep_mask  restated on the stateless stream of
// random.hip:  u = tf.random.stateless_uniform([n], seed=[seed0, *step])  (GenerateKey scramble of the int32 pair, element i =
// lane i % 4 of Philox-4x32-10(counter + i/4), 23 mantissa bits), keep[i] = u[i] >= rate.
//   rigl_dropout_fwd     : y[i]  = keep[i] ? round(f32(x[i])  * scale) : +0;  keep_bits byte i/8, bit i%8 (LSB first) = keep[i]
//   rigl_dropout_bwd     : dx[i] = bit[i]  ? round(f32(dy[i]) * scale) : +0   (from the STORED bits, never regenerated)
//   rigl_dropout_advance : *step += 1
// *step is read on the DEVICE: a captured graph freezes kernel arguments, so a step passed by value would replay one mask for
// ever.  The key scramble therefore runs on the device too, once per thread in front of the grid-stride loop: its operands are
// wave-uniform (a kernel argument and one scalar load), so the compiler keeps it on the scalar unit -- ten rounds per WAVE.
// One thread per group of 8 elements = one keep byte, written whole by that thread (no atomics): two Philox calls, one 16-byte
// load and store (bf16; two of each for fp32).  Bases that are not 16-byte aligned, and the last n % 8 elements, take the
// element-wise path of the same kernel; both paths evaluate the same expressions, so their bits agree.
#include "common.hpp"
#include "philox.hpp"

namespace rigl {
namespace kdrop {

constexpr int THREADS = 256;

struct Args {
  const void* x;           // fwd: x, bwd: dy
  void* y;                 // fwd: y, bwd: dx
  uint8_t* bits;           // fwd: written, bwd: read
  int64_t n;
  float rate, scale;
  int32_t seed0;
  const int32_t* step;     // device, fwd only
};

__device__ __forceinline__ float bf2f(uint32_t h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ uint32_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;   // quiet NaN, sign and payload kept
  u += 0x7FFFu + ((u >> 16) & 1u);                                 // RNE (a finite product that overflows rounds to inf)
  return u >> 16;
}
// one element: a select, not a multiply by the mask -- a dropped NaN / inf / -0 gives +0
__device__ __forceinline__ uint32_t drop_bf16(uint32_t h, bool keep, float scale) {
  return keep ? f2bf(__fmul_rn(bf2f(h), scale)) : 0u;
}
__device__ __forceinline__ uint32_t drop_bf16x2(uint32_t w, uint32_t keep2, float scale) {
  return drop_bf16(w & 0xFFFFu, keep2 & 1u, scale) | (drop_bf16(w >> 16, keep2 & 2u, scale) << 16);
}
__device__ __forceinline__ float drop_f32(float v, bool keep, float scale) { return keep ? __fmul_rn(v, scale) : 0.0f; }

struct Key { uint32_t k0, k1, c2, c3; };

// GenerateKey: int32 -> uint64 sign-extends; one Philox call under a fixed key gives (key, high half of the counter)
__device__ __forceinline__ Key scramble(int32_t seed0, int32_t seed1) {
  const uint64_t s0 = (uint64_t)(int64_t)seed0, s1 = (uint64_t)(int64_t)seed1;
  krand::Philox c;
  c.c[0] = (uint32_t)s0; c.c[1] = (uint32_t)(s0 >> 32); c.c[2] = (uint32_t)s1; c.c[3] = (uint32_t)(s1 >> 32);
  const krand::Philox mix = krand::philox4x32_10(c, krand::SCRAMBLE_K0, krand::SCRAMBLE_K1);
  return Key{mix.c[0], mix.c[1], mix.c[2], mix.c[3]};
}

// keep[8g .. 8g+7] as one byte: counters 2g and 2g+1 (the low 64 bits of the base counter are 0 after GenerateKey, so
// base + i/4 never carries into the high half)
__device__ __forceinline__ uint32_t keep_byte(int64_t g, const Key& K, float rate) {
  uint32_t byte = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint64_t lo = (uint64_t)g * 2u + (uint64_t)h;
    krand::Philox c;
    c.c[0] = (uint32_t)lo; c.c[1] = (uint32_t)(lo >> 32); c.c[2] = K.c2; c.c[3] = K.c3;
    const krand::Philox s = krand::philox4x32_10(c, K.k0, K.k1);
#pragma unroll
    for (int i = 0; i < 4; ++i) byte |= (krand::u32_to_float(s.c[i]) >= rate ? 1u : 0u) << (4 * h + i);
  }
  return byte;
}

// BF16: 2-byte elements, else fp32.  VEC: both bases 16-byte aligned.  FWD: draw the keep byte and store it, else read it.
template <bool BF16, bool VEC, bool FWD>
__global__ __launch_bounds__(THREADS) void k_dropout(Args A) {
  const int64_t groups = (A.n + 7) / 8, full = A.n / 8;
  Key K = {};
  if (FWD) K = scramble(A.seed0, *A.step);
  const float scale = A.scale;
  for (int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * THREADS) {
    uint32_t byte = FWD ? keep_byte(g, K, A.rate) : (uint32_t)A.bits[g];
    if (VEC && g < full) {
      if (BF16) {
        const uint4 v = reinterpret_cast<const uint4*>(A.x)[g];
        reinterpret_cast<uint4*>(A.y)[g] = make_uint4(drop_bf16x2(v.x, byte, scale), drop_bf16x2(v.y, byte >> 2, scale),
                                                      drop_bf16x2(v.z, byte >> 4, scale), drop_bf16x2(v.w, byte >> 6, scale));
      } else {
        const float4 a = reinterpret_cast<const float4*>(A.x)[2 * g], b = reinterpret_cast<const float4*>(A.x)[2 * g + 1];
        reinterpret_cast<float4*>(A.y)[2 * g] = make_float4(drop_f32(a.x, byte & 1u, scale), drop_f32(a.y, byte & 2u, scale),
                                                            drop_f32(a.z, byte & 4u, scale), drop_f32(a.w, byte & 8u, scale));
        reinterpret_cast<float4*>(A.y)[2 * g + 1] = make_float4(drop_f32(b.x, byte & 16u, scale), drop_f32(b.y, byte & 32u, scale),
                                                                drop_f32(b.z, byte & 64u, scale), drop_f32(b.w, byte & 128u, scale));
      }
    } else {
      // element-wise: unaligned bases, and the last n % 8 elements of either path
      const int64_t e0 = g * 8;
      const int cnt = A.n - e0 < 8 ? (int)(A.n - e0) : 8;
      byte &= (1u << cnt) - 1u;                                     // the unused high bits of the last byte are written as 0
      for (int i = 0; i < cnt; ++i) {
        const bool keep = (byte >> i) & 1u;
        if (BF16) {
          reinterpret_cast<uint16_t*>(A.y)[e0 + i] = (uint16_t)drop_bf16(reinterpret_cast<const uint16_t*>(A.x)[e0 + i], keep, scale);
        } else {
          reinterpret_cast<float*>(A.y)[e0 + i] = drop_f32(reinterpret_cast<const float*>(A.x)[e0 + i], keep, scale);
        }
      }
    }
    if (FWD) A.bits[g] = (uint8_t)byte;
  }
}

__global__ void k_dropout_advance(int32_t* __restrict__ step) {
  if (threadIdx.x == 0) *step = (int32_t)((uint32_t)*step + 1u);    // wraps like the int32 cast of the reference's seed pair
}

template <bool FWD>
static void launch(const Args& A, int32_t dtype, hipStream_t st) {
  const bool vec = (((uintptr_t)A.x | (uintptr_t)A.y) & 15u) == 0;
  int64_t blocks = ((A.n + 7) / 8 + THREADS - 1) / THREADS;
  if (blocks > 8192) blocks = 8192;
  const dim3 g((unsigned)blocks), b(THREADS);
  if (dtype == 0) {
    if (vec) hipLaunchKernelGGL((k_dropout<true, true, FWD>), g, b, 0, st, A);
    else hipLaunchKernelGGL((k_dropout<true, false, FWD>), g, b, 0, st, A);
  } else {
    if (vec) hipLaunchKernelGGL((k_dropout<false, true, FWD>), g, b, 0, st, A);
    else hipLaunchKernelGGL((k_dropout<false, false, FWD>), g, b, 0, st, A);
  }
}

static int check(const char* who, int64_t n, int32_t dtype, float rate) {
  if (n < 0) return fail(RIGL_EINVAL, "%s: n must be >= 0", who);
  if (dtype != 0 && dtype != 1) return fail(RIGL_EINVAL, "%s: dtype must be 0 (bf16) or 1 (fp32)", who);
  if (!(rate >= 0.0f && rate < 1.0f)) return fail(RIGL_EINVAL, "%s: rate must be in [0, 1), got %g", who, (double)rate);
  return RIGL_OK;
}

}  // namespace kdrop
}  // namespace rigl

extern "C" {

int rigl_dropout_fwd(const void* x, void* y, uint8_t* keep_bits, int64_t n, int32_t dtype, float rate, int32_t seed0,
                     const int32_t* step, rigl_stream_t stream) {
  using namespace rigl;
  using namespace rigl::kdrop;
  if (int rc = check("rigl_dropout_fwd", n, dtype, rate)) return rc;
  if (n == 0) return RIGL_OK;
  if (!x || !y || !keep_bits || !step) return fail(RIGL_EINVAL, "rigl_dropout_fwd: NULL x / y / keep_bits / step");
  if (((uintptr_t)step & 3u) || (dtype == 1 && (((uintptr_t)x | (uintptr_t)y) & 3u)) || (dtype == 0 && (((uintptr_t)x | (uintptr_t)y) & 1u)))
    return fail(RIGL_EINVAL, "rigl_dropout_fwd: x / y / step not aligned to their element size");
  Args A;
  A.x = x; A.y = y; A.bits = keep_bits; A.n = n; A.rate = rate; A.scale = 1.0f / (1.0f - rate); A.seed0 = seed0; A.step = step;
  launch<true>(A, dtype, as_stream(stream));
  RIGL_CHECK_LAUNCH("rigl_dropout_fwd");
  return RIGL_OK;
}

int rigl_dropout_bwd(const void* dy, const uint8_t* keep_bits, void* dx, int64_t n, int32_t dtype, float rate,
                     rigl_stream_t stream) {
  using namespace rigl;
  using namespace rigl::kdrop;
  if (int rc = check("rigl_dropout_bwd", n, dtype, rate)) return rc;
  if (n == 0) return RIGL_OK;
  if (!dy || !dx || !keep_bits) return fail(RIGL_EINVAL, "rigl_dropout_bwd: NULL dy / dx / keep_bits");
  if ((dtype == 1 && (((uintptr_t)dy | (uintptr_t)dx) & 3u)) || (dtype == 0 && (((uintptr_t)dy | (uintptr_t)dx) & 1u)))
    return fail(RIGL_EINVAL, "rigl_dropout_bwd: dy / dx not aligned to their element size");
  Args A;
  A.x = dy; A.y = dx; A.bits = const_cast<uint8_t*>(keep_bits); A.n = n; A.rate = rate; A.scale = 1.0f / (1.0f - rate);
  A.seed0 = 0; A.step = nullptr;
  launch<false>(A, dtype, as_stream(stream));
  RIGL_CHECK_LAUNCH("rigl_dropout_bwd");
  return RIGL_OK;
}

int rigl_dropout_advance(int32_t* step, rigl_stream_t stream) {
  using namespace rigl;
  if (!step || ((uintptr_t)step & 3u)) return fail(RIGL_EINVAL, "rigl_dropout_advance: bad step");
  hipLaunchKernelGGL(kdrop::k_dropout_advance, dim3(1), dim3(64), 0, as_stream(stream), step);
  RIGL_CHECK_LAUNCH("rigl_dropout_advance");
  return RIGL_OK;
}

}  // extern "C"
