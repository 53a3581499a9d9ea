// The CIFAR input pipeline on the device (rigl/cifar_resnet/data_helper.py:29-109: per_image_standardization, 4-pixel mirror
// pad, random 32x32 crop, random left-right flip, reshuffle each pass), one wave per image:
//   rigl_cifar_batch   : out[i], out_labels[i], out_index[i] for i < batch from the raw uint8 dataset and the DEVICE step counter
//   rigl_cifar_advance : *step += 1
// The semantics (standardization on exact integer sums, the mirror / crop / flip index map, the Philox draws, the Feistel sample
// order, eval mode) are stated once in include/rigl_hip.h and restated in NumPy by tests/input_ref.py; the two agree bit for bit.
// *step is read on the DEVICE (a captured graph freezes kernel arguments), so everything derived from it -- epoch, position,
// round keys, dataset index, crop offsets, flip -- is computed here, per wave, from operands that are wave-uniform (kernel
// arguments, one scalar load, the wave's number): the compiler keeps the five Philox evaluations and the Feistel walk on the
// scalar unit.  No permutation buffer exists, so nothing can go stale under replay.
// Mapping: an image is 3072 bytes = 3 x (64 lanes x 16 bytes).  A wave loads it with three coalesced 16-byte loads per lane,
// sums x and x^2 in integers (exact: S1 <= 783 360, S2 < 2^31) with a butterfly over the wave, stages the bytes in its own 3 KB
// of LDS, and then every lane produces half an output row: 16 pixels x 3 channels read byte-wise from the mirrored, shifted,
// flipped LDS positions, stored as 96 (bf16) or 192 (fp32) contiguous bytes with 16-byte stores.  Four waves per workgroup.
// No fast-math in this file: sqrtf and / are the correctly rounded ones, and the library is built with -ffp-contract=off.
#include "common.hpp"
#include "philox.hpp"

namespace rigl {
namespace kinput {

constexpr int WAVES = 4, THREADS = 64 * WAVES;
constexpr int SIDE = 32, CH = 3, PIXELS = SIDE * SIDE, IMG_BYTES = PIXELS * CH;   // 3072
constexpr int PAD = 4;
constexpr uint32_t FEISTEL_MUL = 0x9E3779B1u, EPOCH_SALT = 0x5eedu;
constexpr int FEISTEL_ROUNDS = 6;

struct Args {
  const uint8_t* images;
  const int32_t* labels;
  uint32_t n_images;       // <= 2^30
  int32_t batch, mode, shard, n_shards, seed0;
  uint32_t spe;            // train: steps per epoch = n_images / (batch * n_shards) >= 1
  uint32_t half_bits;      // h: the Feistel network permutes [0, 2^(2h))
  const int32_t* step;
  void* out;
  int32_t* out_labels;
  int32_t* out_index;      // may be NULL
};

struct Key { uint32_t k0, k1, c2, c3; };

// GenerateKey, as dropout.hip: int32 -> uint64 sign-extends; one Philox call under a fixed key
__device__ __forceinline__ Key scramble(int32_t seed0, int32_t seed1) {
  const uint64_t s0 = (uint64_t)(int64_t)seed0, s1 = (uint64_t)(int64_t)seed1;
  krand::Philox c;
  c.c[0] = (uint32_t)s0; c.c[1] = (uint32_t)(s0 >> 32); c.c[2] = (uint32_t)s1; c.c[3] = (uint32_t)(s1 >> 32);
  const krand::Philox mix = krand::philox4x32_10(c, krand::SCRAMBLE_K0, krand::SCRAMBLE_K1);
  return Key{mix.c[0], mix.c[1], mix.c[2], mix.c[3]};
}
// words 4 * block .. 4 * block + 3 of stateless_u32(., seed pair)
__device__ __forceinline__ krand::Philox block_of(const Key& K, uint32_t block) {
  krand::Philox c;
  c.c[0] = block; c.c[1] = 0u; c.c[2] = K.c2; c.c[3] = K.c3;
  return krand::philox4x32_10(c, K.k0, K.k1);
}

__device__ __forceinline__ uint32_t feistel(uint32_t v, const uint32_t (&k)[FEISTEL_ROUNDS], uint32_t h) {
  const uint32_t m = (1u << h) - 1u;
  uint32_t L = (v >> h) & m, R = v & m;
#pragma unroll
  for (int r = 0; r < FEISTEL_ROUNDS; ++r) {
    const uint32_t f = ((R ^ k[r]) * FEISTEL_MUL) >> (32u - h);
    const uint32_t t = L ^ f;
    L = R; R = t;
  }
  return (L << h) | R;
}

// padded coordinate 0..39 -> source 0..31 (NumPy 'symmetric': 3,2,1,0 | 0..31 | 31,30,29,28)
__device__ __forceinline__ int mirror(int p) { return p < PAD ? PAD - 1 - p : (p < PAD + SIDE ? p - PAD : 2 * SIDE + PAD - 1 - p); }

__device__ __forceinline__ uint32_t f2bf(float f) {                // RNE; the values here are finite
  uint32_t u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

template <bool BF16>
__global__ __launch_bounds__(THREADS) void k_cifar_batch(Args A) {
  __shared__ uint4 stage[WAVES][IMG_BYTES / 16];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x * WAVES + wave;                         // image of the batch, wave-uniform
  const int32_t s = *A.step;
  const uint32_t N = A.n_images;

  bool active = i < A.batch;
  uint32_t idx = 0;
  int oy = PAD, ox = PAD;                                          // eval: the centre crop of the padded image = the image
  bool flip = false;
  if (active) {
    if (A.mode == 0) {
      const uint32_t su = (uint32_t)s, e = su / A.spe;
      uint32_t k[FEISTEL_ROUNDS];
      {
        const Key K = scramble((int32_t)((uint32_t)A.seed0 ^ EPOCH_SALT), (int32_t)e);
        const krand::Philox a = block_of(K, 0u), b = block_of(K, 1u);
        k[0] = a.c[0]; k[1] = a.c[1]; k[2] = a.c[2]; k[3] = a.c[3]; k[4] = b.c[0]; k[5] = b.c[1];
      }
      const uint32_t p = (su % A.spe) * (uint32_t)A.batch * (uint32_t)A.n_shards + (uint32_t)A.shard * (uint32_t)A.batch + (uint32_t)i;
      idx = feistel(p, k, A.half_bits);
      while (idx >= N) idx = feistel(idx, k, A.half_bits);           // cycle-walk: p < N lies on the cycle, so this ends
      const krand::Philox d = block_of(scramble(A.seed0, s), (uint32_t)i);
      oy = (int)(d.c[0] % 9u);
      ox = (int)(d.c[1] % 9u);
      flip = krand::u32_to_float(d.c[2]) < 0.5f;
    } else {
      const uint64_t j = ((uint64_t)(uint32_t)s * (uint32_t)A.n_shards + (uint32_t)A.shard) * (uint32_t)A.batch + (uint32_t)i;
      active = j < (uint64_t)N;                                    // past the end of the dataset: nothing is written
      idx = (uint32_t)j;
    }
  }

  float inv = 0.0f;
  int32_t S1 = 0;
  if (active) {
    const uint4* src = reinterpret_cast<const uint4*>(A.images + (size_t)idx * IMG_BYTES);
    uint32_t s1 = 0, s2 = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const uint4 v = src[q * 64 + lane];
      stage[wave][q * 64 + lane] = v;
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint32_t x = (w[j] >> (8 * b)) & 0xFFu;
          s1 += x; s2 += x * x;
        }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      s1 += __shfl_xor(s1, off, 64);
      s2 += __shfl_xor(s2, off, 64);
    }
    S1 = (int32_t)s1;
    const int64_t D = (int64_t)IMG_BYTES * (int64_t)s2 - (int64_t)s1 * (int64_t)s1;
    const float den = fmaxf(sqrtf((float)D), sqrtf((float)IMG_BYTES));
    inv = 1.0f / den;
  }
  __syncthreads();
  if (!active) return;

  const uint8_t* img = reinterpret_cast<const uint8_t*>(&stage[wave][0]);
  const int r = lane >> 1, c0 = (lane & 1) * 16;
  const int sr = mirror(r + oy);
  uint32_t vals[16 * CH];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = c0 + j;
    const int sc = mirror((flip ? SIDE - 1 - c : c) + ox);
    const uint8_t* px = img + (sr * SIDE + sc) * CH;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
      const float y = (float)(IMG_BYTES * (int32_t)px[ch] - S1) * inv;
      vals[j * CH + ch] = BF16 ? f2bf(y) : __float_as_uint(y);
    }
  }
  const size_t first = ((size_t)i * PIXELS + (size_t)r * SIDE + c0) * CH;      // element offset of this lane's 48 values
  if (BF16) {
    uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(A.out) + first);
#pragma unroll
    for (int q = 0; q < 6; ++q)
      dst[q] = make_uint4(vals[8 * q] | (vals[8 * q + 1] << 16), vals[8 * q + 2] | (vals[8 * q + 3] << 16),
                          vals[8 * q + 4] | (vals[8 * q + 5] << 16), vals[8 * q + 6] | (vals[8 * q + 7] << 16));
  } else {
    uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(A.out) + first);
#pragma unroll
    for (int q = 0; q < 12; ++q) dst[q] = make_uint4(vals[4 * q], vals[4 * q + 1], vals[4 * q + 2], vals[4 * q + 3]);
  }
  if (lane == 0) {
    A.out_labels[i] = A.labels[idx];
    if (A.out_index) A.out_index[i] = (int32_t)idx;
  }
}

__global__ void k_cifar_advance(int32_t* __restrict__ step) {
  if (threadIdx.x == 0) *step = (int32_t)((uint32_t)*step + 1u);    // int32 wrap-around, as k_dropout_advance
}

}  // namespace kinput
}  // namespace rigl

extern "C" {

int rigl_cifar_batch(const uint8_t* images, const int32_t* labels, int64_t n_images, int32_t batch, int32_t mode,
                     int32_t shard, int32_t n_shards, int32_t seed0, const int32_t* step, void* out, int32_t dtype,
                     int32_t* out_labels, int32_t* out_index, rigl_stream_t stream) {
  using namespace rigl;
  using namespace rigl::kinput;
  if (batch <= 0) return fail(RIGL_EINVAL, "rigl_cifar_batch: batch must be > 0, got %d", batch);
  if (!images || !labels || !step || !out || !out_labels)
    return fail(RIGL_EINVAL, "rigl_cifar_batch: NULL images / labels / step / out / out_labels");
  if (n_images <= 0 || n_images > ((int64_t)1 << 30))
    return fail(RIGL_EINVAL, "rigl_cifar_batch: n_images must be in 1 .. 2^30, got %lld", (long long)n_images);
  if (mode != 0 && mode != 1) return fail(RIGL_EINVAL, "rigl_cifar_batch: mode must be 0 (train) or 1 (eval), got %d", mode);
  if (dtype != 0 && dtype != 1) return fail(RIGL_EINVAL, "rigl_cifar_batch: dtype must be 0 (bf16) or 1 (fp32), got %d", dtype);
  if (n_shards <= 0 || shard < 0 || shard >= n_shards)
    return fail(RIGL_EINVAL, "rigl_cifar_batch: shard %d outside [0, n_shards = %d)", shard, n_shards);
  const int64_t per_step = (int64_t)batch * (int64_t)n_shards;
  if (mode == 0 && n_images < per_step)
    return fail(RIGL_EINVAL, "rigl_cifar_batch: train mode needs n_images >= batch * n_shards, got %lld < %lld",
                (long long)n_images, (long long)per_step);
  if ((((uintptr_t)images | (uintptr_t)out) & 15u) || (((uintptr_t)labels | (uintptr_t)step | (uintptr_t)out_labels | (uintptr_t)out_index) & 3u))
    return fail(RIGL_EINVAL, "rigl_cifar_batch: images / out must be 16-byte aligned, labels / step / out_labels / out_index 4-byte");
  Args A;
  A.images = images; A.labels = labels; A.n_images = (uint32_t)n_images; A.batch = batch; A.mode = mode; A.shard = shard;
  A.n_shards = n_shards; A.seed0 = seed0; A.step = step; A.out = out; A.out_labels = out_labels; A.out_index = out_index;
  A.spe = mode == 0 ? (uint32_t)(n_images / per_step) : 1u;
  uint32_t bits = 0;
  for (uint64_t v = (uint64_t)n_images - 1u; v; v >>= 1) ++bits;     // bit_length(N - 1)
  A.half_bits = bits < 2 ? 1u : (bits + 1u) / 2u;                     // h = max(1, ceil(bits / 2))
  const dim3 g((unsigned)((batch + WAVES - 1) / WAVES)), b(THREADS);
  if (dtype == 0) hipLaunchKernelGGL((k_cifar_batch<true>), g, b, 0, as_stream(stream), A);
  else hipLaunchKernelGGL((k_cifar_batch<false>), g, b, 0, as_stream(stream), A);
  RIGL_CHECK_LAUNCH("rigl_cifar_batch");
  return RIGL_OK;
}

int rigl_cifar_advance(int32_t* step, rigl_stream_t stream) {
  using namespace rigl;
  if (!step || ((uintptr_t)step & 3u)) return fail(RIGL_EINVAL, "rigl_cifar_advance: bad step");
  hipLaunchKernelGGL(kinput::k_cifar_advance, dim3(1), dim3(64), 0, as_stream(stream), step);
  RIGL_CHECK_LAUNCH("rigl_cifar_advance");
  return RIGL_OK;
}

}  // extern "C"
