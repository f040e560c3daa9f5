// train_ops.h — the device pieces of a training step that the stand-alone models share (diffusion.hip, rnn_dynamics.hip): the
// statistics and the backward core of a GroupNorm / LayerNorm whose group one wave holds, the MSE loss, and torch.optim.Adam's
// element update.  Every helper is the text its users had, so the compiler contracts the same products into the same fmas.
#pragma once
#include "reduce.h"

namespace orl {

// statistics of n <= 64 NJ values x[0 .. n) in one wave: the values in registers (lane + 64 j), mean, then the centred second
// moment; eps 1e-5
template <int NJ>
__device__ __forceinline__ void norm_stats(const float* x, int n, int lane, float (&v)[NJ], float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < n ? x[c] : 0.f;
    s += v[j];
  }
  mean = wave_sum(s) / (float)n;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float dlt = (lane + 64 * j) < n ? v[j] - mean : 0.f;
    q += dlt * dlt;
  }
  rstd = 1.f / sqrtf(wave_sum(q) / (float)n + 1e-5f);
}

// The core of the norm's backward over the n values of a wave's group.  s1 / s2: this lane's sums of dxh = dy gamma and of dxh xh (xh:
// the normalised values).  They stay in the caller's element loop, next to the products they are formed from: summed in a loop of
// their own here, the compiler contracts other products into fmas and the bits move.  The constructor forms the group's means (two
// wave sums); dx is then one element's input gradient rstd (dxh - mean(dxh) - xh mean(dxh xh))
struct NormBwd {
  float s1, s2, rstd;
  __device__ __forceinline__ NormBwd(float lane_s1, float lane_s2, float rstd_, int n)
      : s1(wave_sum(lane_s1) / (float)n), s2(wave_sum(lane_s2) / (float)n), rstd(rstd_) {}
  __device__ __forceinline__ float dx(float dxh, float xh) const { return rstd * (dxh - s1 - xh * s2); }
};

// loss = mean over (rows x od) of (pred - tgt)^2 [times msk[row]], dPRED = 2 (pred - tgt) [msk] / (rows od); one block per run (pred
// and dpred at stride p_rs, tgt / msk at tm_rs * od / tm_rs, the loss cells [run]; the two may be one array), fixed order.  MASKED is
// a compile-time switch and not a mask of ones: s += df df is one fma, s += df df m rounds the product first
template <bool MASKED>
__global__ __launch_bounds__(256) void k_mse_loss(const float* __restrict__ pred, int pp, long p_rs, const float* __restrict__ tgt,
                                                  const float* __restrict__ msk, long tm_rs, long rows, int od, float* __restrict__ dpred,
                                                  float* loss_out, float* loss_last) {
  const long run = blockIdx.x;
  pred += run * p_rs; dpred += run * p_rs; tgt += run * tm_rs * od;
  if constexpr (MASKED) msk += run * tm_rs;
  const long n = rows * od;
  const float inv = 1.f / (float)n;
  float s = 0.f;
  for (long e = threadIdx.x; e < n; e += 256) {
    const long r = e / od; const int d = (int)(e - r * od);
    if constexpr (MASKED) {
      const float df = pred[r * pp + d] - tgt[e], m = msk[r];
      s += df * df * m;
      dpred[r * pp + d] = 2.f * df * m * inv;
    } else {
      const float df = pred[r * pp + d] - tgt[e];
      s += df * df;
      dpred[r * pp + d] = 2.f * df * inv;
    }
  }
  s = block_sum256_pairwise(s);
  if (threadIdx.x == 0) {
    const float l = s * inv;
    loss_out[run] = l;
    loss_last[run] = l;
  }
}

// torch.optim.Adam's element update (exp_avg lerp, exp_avg_sq, the bias corrections folded into step and bc2s); updates the moments,
// returns the new weight.  How step and 1 - beta are formed is the caller's
__device__ __forceinline__ float adam_update(float p, float& m, float& v, float g, float step, float bc2s, float omb1, float b2, float omb2, float eps) {
  m = m + (g - m) * omb1;
  v = v * b2 + omb2 * g * g;
  return p - step * (m / (sqrtf(v) / bc2s + eps));
}

}  // namespace orl
