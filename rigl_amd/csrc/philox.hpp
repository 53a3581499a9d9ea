// Philox-4x32-10 (Salmon et al., SC'11) and TensorFlow's Uint32ToFloat, shared by the stateless random fills
// (random.hip) and the dropout keep mask (dropout.hip): one statement of the generator both are pinned against
// (oracle/tf_random.py).
#pragma once
#include "common.hpp"

namespace rigl {
namespace krand {

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
// stateless_random_ops.cc GenerateKey: the fixed key the int32 seed pair is scrambled under
constexpr uint32_t SCRAMBLE_K0 = 0x3ec8f720u, SCRAMBLE_K1 = 0x02461e29u;

struct Philox { uint32_t c[4]; };

__host__ __device__ inline Philox philox4x32_10(Philox ctr, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += W0; k1 += W1; }
    const uint64_t p0 = (uint64_t)M0 * ctr.c[0], p1 = (uint64_t)M1 * ctr.c[2];
    Philox n;
    n.c[0] = (uint32_t)(p1 >> 32) ^ ctr.c[1] ^ k0;
    n.c[1] = (uint32_t)p1;
    n.c[2] = (uint32_t)(p0 >> 32) ^ ctr.c[3] ^ k1;
    n.c[3] = (uint32_t)p0;
    ctr = n;
  }
  return ctr;
}

__device__ __forceinline__ float u32_to_float(uint32_t x) {
  return __uint_as_float((127u << 23) | (x & 0x7FFFFFu)) - 1.0f;
}

}  // namespace krand
}  // namespace rigl
