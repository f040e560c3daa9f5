// reduce.h — device helpers shared by the stand-alone device objects (dynamics.hip, diffusion.hip).
//
// block_sum256_pairwise is NOT kernels.h's block_sum256 and must not be merged with it: that one reduces with __shfl_down and adds the
// wave sums as ((s0 + s1) + s2) + s3, this one with __shfl_xor and (s0 + s1) + (s2 + s3).  Either change moves the engine's or these
// objects' bits.
#pragma once
#include <hip/hip_runtime.h>

namespace orl {

// sum over the 64 lanes of a wave, in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}
// sum over a 256-thread block, for thread 0: the four wave sums as (s0 + s1) + (s2 + s3)
__device__ __forceinline__ float block_sum256_pairwise(float s) {
  __shared__ float s_red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}
// torch.nn.functional.softplus (beta 1, threshold 20)
__device__ __forceinline__ float softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }

}  // namespace orl
