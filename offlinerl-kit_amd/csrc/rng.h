// rng.h — the device random numbers of the engine (kernels.h) and of the dynamics ensemble (dynamics.hip): Philox4x32-10 keyed by a
// 64-bit seed (low / high word = k0 / k1), the uniform in (0, 1) of a 32-bit word and Box-Muller on a pair of words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orl {

struct Philox {
  uint32_t k0, k1;
  __device__ Philox(uint64_t seed) : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)) {}
  __device__ void operator()(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t (&out)[4]) const {
    uint32_t a = k0, b = k1;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
      const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ a, n1 = (uint32_t)p1;
      const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ b, n3 = (uint32_t)p0;
      c0 = n0; c1 = n1; c2 = n2; c3 = n3;
      a += 0x9E3779B9u; b += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
  }
};
__device__ inline float u01(uint32_t x) { return ((x >> 8) + 0.5f) * (1.0f / 16777216.0f); }  // (0,1)
__device__ inline void box_muller(uint32_t x, uint32_t y, float& n0, float& n1) {
  const float r = sqrtf(-2.0f * logf(u01(x)));
  const float t = 6.28318530717958647692f * u01(y);
  n0 = r * cosf(t); n1 = r * sinf(t);
}
// ONE of box_muller's two values: element j of a Philox word o takes the pair (o[j & ~1], o[j | 1]), cos for an even j, sin for an odd
// one (for a consumer that may stop in the middle of a word and should not pay for the value it drops)
__device__ inline float box_muller_one(const uint32_t (&o)[4], int j) {
  const float r = sqrtf(-2.0f * logf(u01(o[j & ~1])));
  const float t = 6.28318530717958647692f * u01(o[j | 1]);
  return (j & 1) ? r * sinf(t) : r * cosf(t);
}

}  // namespace orl
