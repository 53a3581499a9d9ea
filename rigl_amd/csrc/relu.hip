// Stand-alone ReLU streams of the VGG workload (rigl/imagenet_resnet/vgg.py:124-134: conv2d_fixed_padding, then
// tf.nn.relu, no batch norm).  Where a conv's body has no ReLU epilogue (rigl_conv2d_fwd_takes_relu_epilogue /
// rigl_conv2d_bwd_takes_relu_epilogue say 0) the conv entry points run these behind the plain kernels:
//   rigl_relu_fwd : y  = relu(x)          (+0 for every value with the sign bit set; in place allowed)
//   rigl_relu_bwd : dx = dy * [x > 0]     (x = the ReLU's OUTPUT, or a max pool of it: the same mask at the pool winner)
// Their bits are those of the fused epilogues: both operate on the bf16 values the plain kernels store.
// 16 bytes per lane; every lane issues its loads at a clamped address and only the store is guarded.
#include "common.hpp"

namespace rigl {
namespace krelu {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void k_relu_fwd(const uint4* __restrict__ x, uint4* y, int64_t n8) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i0 = (int64_t)blockIdx.x * THREADS; i0 < n8; i0 += stride) {
    const int64_t i = i0 + threadIdx.x;
    const uint4 v = x[i < n8 ? i : n8 - 1];
    if (i < n8) y[i] = relu_bf16x8(v);
  }
}

__global__ __launch_bounds__(THREADS) void k_relu_bwd(const uint4* __restrict__ dy, const uint4* __restrict__ x, uint4* dx,
                                                      int64_t n8) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i0 = (int64_t)blockIdx.x * THREADS; i0 < n8; i0 += stride) {
    const int64_t i = i0 + threadIdx.x, c = i < n8 ? i : n8 - 1;
    const uint4 g = dy[c], v = x[c];
    if (i < n8) dx[i] = gate_bf16x8(g, v);
  }
}

static unsigned stream_grid(int64_t n8) {
  const int64_t b = (n8 + THREADS - 1) / THREADS;
  return (unsigned)(b < 8192 ? b : 8192);
}

}  // namespace krelu

// (used by conv.hip behind the plain kernels)
int relu_fwd_launch(int64_t n, const rigl_bf16* x, rigl_bf16* y, hipStream_t st) {
  const int64_t n8 = n / 8;
  hipLaunchKernelGGL(krelu::k_relu_fwd, dim3(krelu::stream_grid(n8)), dim3(krelu::THREADS), 0, st,
                     reinterpret_cast<const uint4*>(x), reinterpret_cast<uint4*>(y), n8);
  RIGL_CHECK_LAUNCH("rigl_relu_fwd");
  return RIGL_OK;
}
int relu_bwd_launch(int64_t n, const rigl_bf16* dy, const rigl_bf16* x, rigl_bf16* dx, hipStream_t st) {
  const int64_t n8 = n / 8;
  hipLaunchKernelGGL(krelu::k_relu_bwd, dim3(krelu::stream_grid(n8)), dim3(krelu::THREADS), 0, st,
                     reinterpret_cast<const uint4*>(dy), reinterpret_cast<const uint4*>(x), reinterpret_cast<uint4*>(dx), n8);
  RIGL_CHECK_LAUNCH("rigl_relu_bwd");
  return RIGL_OK;
}

}  // namespace rigl

extern "C" {

int rigl_relu_fwd(int64_t n, const rigl_bf16* x, rigl_bf16* y, rigl_stream_t stream) {
  using namespace rigl;
  if (n <= 0 || (n % 8)) return fail(RIGL_EINVAL, "rigl_relu_fwd: n must be a positive multiple of 8");
  if (!x || !y) return fail(RIGL_EINVAL, "rigl_relu_fwd: NULL tensor");
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return fail(RIGL_EINVAL, "rigl_relu_fwd: tensors must be 16-byte aligned");
  return relu_fwd_launch(n, x, y, as_stream(stream));
}

int rigl_relu_bwd(int64_t n, const rigl_bf16* dy, const rigl_bf16* x, rigl_bf16* dx, rigl_stream_t stream) {
  using namespace rigl;
  if (n <= 0 || (n % 8)) return fail(RIGL_EINVAL, "rigl_relu_bwd: n must be a positive multiple of 8");
  if (!dy || !x || !dx) return fail(RIGL_EINVAL, "rigl_relu_bwd: NULL tensor");
  if (((uintptr_t)dy & 15) || ((uintptr_t)x & 15) || ((uintptr_t)dx & 15))
    return fail(RIGL_EINVAL, "rigl_relu_bwd: tensors must be 16-byte aligned");
  return relu_bwd_launch(n, dy, x, dx, as_stream(stream));
}

}  // extern "C"
