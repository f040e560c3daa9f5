// dynamics.hip — the probabilistic dynamics ensemble of MOPO / COMBO on the device (reference: dynamics/ensemble_dynamics.py,
// modules/dynamics_module.py): orl_dyn_* of include/orl_engine.h.
//
// One minibatch of learn() is a plain run of launches on one stream, enqueued for the whole epoch before the host waits once:
//   k_dyn_gather       bootstrap rows of the HBM dataset, (x - mu) / std fused in (StandardScaler.transform's fp32 operations)
//   L x E_BIAS_SWISH   hidden layers on the tiled GEMM (gemm_inst_swish.hip): h = z sigmoid(z), z kept for the backward
//   1 x E_BIAS         output layer -> [mean | raw logvar]
//   k_dyn_nll          soft_clamp, the Gaussian NLL terms, d mean / d raw logvar, per-element max / min_logvar gradient terms
//   k_dyn_nll_reduce   per run: the minibatch loss (mean over rows and dims, summed over members, + coef (sum max - sum min)) and the
//                      max / min_logvar gradients, reduced in a fixed order
//   (L+1) x E_WGRAD, L x E_SWISH_GRAD   weight / bias gradients and the Swish-scaled input gradients, top down
//   k_dyn_adam         torch.optim.Adam with the weight-decay term wd_l W_l folded into the weights' gradients; the decay loss of the
//                      weights it reads is reduced on the way; inactive runs are skipped (their state stays bit for bit)
//   k_dyn_loss         adds the decay loss and accumulates the minibatch loss of the active runs
// Members and runs are batched through blockIdx.z = run * K + member of every GEMM; a 2-D input shared by the members (validate, step)
// is a member stride of 0.  RAMBO's adversarial update of the same ensemble (orl_dynadv_*) is described where its kernels start.
//
// Every formula that more than one kernel needs exists ONCE, as a device function below: dyn_soft_clamp(_grad) and dyn_std (every
// logvar and std of this file), dyn_nll_elem (the NLL element of k_dyn_nll and of k_dyn_adv_head's dataset rows), dyn_col_sum and
// dyn_reduce_tail (the two reduce kernels), dyn_draw_elite, dyn_scale_row, reduce.h's wave_sum / block_sum256_pairwise / softplus and
// rng.h's Philox / box_muller_one.  A sampler that must agree with another bit for bit agrees because both call the same function.
// On the host, DynWs is the one workspace type (learn, adversarial update, and step as a forward-only view) and dyn_forward /
// dyn_backward are the only layer loops.  Allocation, the tensor table, transfers, staging and the GemmP of a layer's products come
// from devobj.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "devobj.h"
#include "reduce.h"
#include "rng.h"

namespace orl {

// the derivative of reduce.h's softplus
__device__ inline float dyn_dsoftplus(float y) { return y > 20.f ? 1.f : 1.f / (1.f + expf(-y)); }

// soft_clamp of a raw logvar x (modules/dynamics_module.py): l1 = mx - softplus(mx - x), lv = mn + softplus(l1 - mn), with
// s1 = d l1 / d x and s2 = d lv / d l1.  Every logvar of this file comes from here: the training heads, step() and both samplers.
struct DynClamp { float lv, s1, s2; };
__device__ __forceinline__ DynClamp dyn_soft_clamp_grad(float x, float mx, float mn) {
  const float y1 = mx - x;
  const float l1 = mx - softplus(y1);
  const float y2 = l1 - mn;
  return {mn + softplus(y2), dyn_dsoftplus(y1), dyn_dsoftplus(y2)};
}
__device__ __forceinline__ float dyn_soft_clamp(float x, float mx, float mn) { return dyn_soft_clamp_grad(x, mx, mn).lv; }
// std = sqrt(exp(logvar)) as the reference writes it
__device__ __forceinline__ float dyn_std(float x, float mx, float mn) { return sqrtf(expf(dyn_soft_clamp(x, mx, mn))); }

// One element of the Gaussian NLL ((mean - target)^2 exp(-lv) + lv, times `scale` in the gradients): d / d mean, d / d raw logvar,
// the loss term and the element's share of the max / min_logvar gradients.
struct DynNll { float dmean, draw, lterm, gmax, gmin; };
__device__ __forceinline__ DynNll dyn_nll_elem(float mean, float x, float target, float mx, float mn, float scale) {
  const DynClamp c = dyn_soft_clamp_grad(x, mx, mn);
  const float inv = expf(-c.lv);
  const float diff = mean - target;
  const float sq = diff * diff * inv;
  const float dlv = (1.f - sq) * scale;
  const float dl1 = dlv * c.s2;
  return {2.f * diff * inv * scale, dl1 * c.s1, sq + c.lv, dl1 * (1.f - c.s1), dlv * (1.f - c.s2)};
}
// ... stored: dOUT [row][op] (mean: cols 0..D, raw logvar: D..2D), lterm / gmax / gmin [row][D]
__device__ __forceinline__ void dyn_store_elem(const DynNll& g, long row, int d, int op, int D, float* dOUT, float* lterm, float* gmax,
                                               float* gmin) {
  dOUT[row * op + d] = g.dmean;
  dOUT[row * op + D + d] = g.draw;
  lterm[row * D + d] = g.lterm;
  gmax[row * D + d] = g.gmax;
  gmin[row * D + d] = g.gmin;
}

// c - a b with two roundings in fp32, as numpy evaluates the reference's reward - penalty_coef * penalty.  Contraction is switched off
// for the two operations: to this compiler __fmul_rn is a plain product, and it fuses a plain product into the subtraction.
__device__ __forceinline__ float dyn_sub_mul(float c, float a, float b) {
#pragma clang fp contract(off)
  const float prod = a * b;
  return c - prod;
}

// the member of a row drawn from the run's elites with the first word of a Philox draw
__device__ __forceinline__ int dyn_draw_elite(const int* elites, int r, int K, int n_elites, uint32_t rnd0) {
  return elites[r * K + (int)(((uint64_t)rnd0 * (uint64_t)n_elites) >> 32)];
}

// x[0..xp) = (concat(o[0..od), a[0..ad)) - mu) / std with zero pads: StandardScaler.transform's fp32 operations
__device__ __forceinline__ void dyn_scale_row(const float* o, int od, const float* a, int ad, const float* m, const float* s, float* x,
                                              int xp) {
  for (int c = 0; c < od; ++c) x[c] = (o[c] - m[c]) / s[c];
  for (int c = 0; c < ad; ++c) x[od + c] = (a[c] - m[od + c]) / s[od + c];
  for (int c = od + ad; c < xp; ++c) x[c] = 0.f;
}

// rows [row0, row0 + rows) of idx[r][k][*] -> X[r][k][i][0..xp) = (in - mu) / std (zero pads), T[r][k][i][0..D)
__global__ void k_dyn_gather(const int* __restrict__ idx, long idx_s0, long idx_s1, long row0, int rows, const float* __restrict__ din,
                             const float* __restrict__ dtg, int in, int D, const float* __restrict__ mu, const float* __restrict__ sd,
                             float* __restrict__ X, long x_s0, long x_s1, int xp, float* __restrict__ T, long t_s0, long t_s1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y, r = blockIdx.z;
  if (i >= rows) return;
  const long g = idx[r * idx_s0 + k * idx_s1 + row0 + i];
  dyn_scale_row(din + g * in, in, nullptr, 0, mu + (long)r * in, sd + (long)r * in, X + r * x_s0 + k * x_s1 + (long)i * xp, xp);
  if (T) {
    const float* tg = dtg + g * D;
    float* t = T + r * t_s0 + k * t_s1 + (long)i * D;
    for (int d = 0; d < D; ++d) t[d] = tg[d];
  }
}

// step(): X[r][i] = scaler(concat(obs, act))
__global__ void k_dyn_step_input(const float* __restrict__ obs, const float* __restrict__ act, long n, int od, int ad,
                                 const float* __restrict__ mu, const float* __restrict__ sd, float* __restrict__ X, int xp) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (i >= n) return;
  const long ri = (long)r * n + i;
  dyn_scale_row(obs + ri * od, od, act + ri * ad, ad, mu + (long)r * (od + ad), sd + (long)r * (od + ad), X + ri * xp, xp);
}

// k_dyn_step_input on pitched source rows (the policy engine's batch slots): obs[r][i] at obs + r obs_rs + i obs_pitch, act likewise;
// dyn_scale_row's arithmetic, so the forward sees the bits it sees from packed rows
__global__ void k_dyn_step_input_rows(const float* __restrict__ obs, long obs_rs, int obs_pitch, const float* __restrict__ act, long act_rs,
                                      int act_pitch, long n, int od, int ad, const float* __restrict__ mu, const float* __restrict__ sd,
                                      float* __restrict__ X, int xp) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (i >= n) return;
  dyn_scale_row(obs + r * obs_rs + i * obs_pitch, od, act + r * act_rs + i * act_pitch, ad, mu + (long)r * (od + ad),
                sd + (long)r * (od + ad), X + ((long)r * n + i) * xp, xp);
}

// Gaussian NLL head, one thread per (run, member, row, dim).  OUT / dOUT [r][k][i][op] (mean: cols 0..D, raw logvar: D..2D),
// T / lterm / gmax / gmin [r][k][i][D] with row stride `bs` rows per (r, k).
__global__ void k_dyn_nll(const float* __restrict__ OUT, float* __restrict__ dOUT, int op, const float* __restrict__ T,
                          float* __restrict__ lterm, float* __restrict__ gmax, float* __restrict__ gmin, const float* __restrict__ params,
                          long P, long off_max, long off_min, int K, int bs, int rows, int D) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (e >= (long)K * rows * D) return;
  const int d = (int)(e % D);
  const long ki = e / D;
  const int i = (int)(ki % rows), k = (int)(ki / rows);
  const long row = ((long)r * K + k) * bs + i;
  const DynNll g = dyn_nll_elem(OUT[row * op + d], OUT[row * op + D + d], T[row * D + d], params[r * P + off_max + d],
                                params[r * P + off_min + d], 1.0f / ((float)rows * (float)D));
  dyn_store_elem(g, row, d, op, D, dOUT, lterm, gmax, gmin);
}

// The two reduce kernels, one workgroup of 1024 threads per run.  Column c of [lterm | gmax | gmin] summed by one wave over
// (member k, row i0 + i) of a[r][k][bs rows][D] in a fixed order: lane stride 64 over e -> (k, i), then the shuffle tree.
__device__ __forceinline__ float dyn_col_sum(const float* lterm, const float* gmax, const float* gmin, int c, int D, int r, int K, int bs,
                                             int i0, int rows, int lane) {
  const float* a = c < D ? lterm : (c < 2 * D ? gmax : gmin);
  const int d = c % D;
  const int KR = K * rows;
  float s = 0.f;
  for (int e = lane; e < KR; e += 64) {
    const int k = e / rows, i = i0 + (e - k * rows);
    s += a[(((long)r * K + k) * bs + i) * D + d];
  }
  return wave_sum(s);
}
// ... and their tail on the 3 D column sums: the max / min_logvar gradients (+coef / -coef of the logvar-bound term) into the gradient
// block and the loss without the decay term, the NLL a mean over `rows` rows and D dims
__device__ __forceinline__ void dyn_reduce_tail(const float* red, int r, int rows, int D, const float* params, float* G, long P, long off_max,
                                                long off_min, float coef, float* nll_out) {
  const int t = threadIdx.x;
  if (t < D) {
    G[r * P + off_max + t] = red[D + t] + coef;
    G[r * P + off_min + t] = red[2 * D + t] - coef;
  }
  if (t == 0) {
    float ls = 0.f, smax = 0.f, smin = 0.f;
    for (int d = 0; d < D; ++d) {
      ls += red[d];
      smax += params[r * P + off_max + d];
      smin += params[r * P + off_min + d];
    }
    nll_out[r] = ls / ((float)rows * (float)D) + (coef * smax - coef * smin);
  }
}

// per run (blockIdx.x): the three column sums over (member, row), the minibatch loss without the decay term and the max / min_logvar
// gradients
__global__ __launch_bounds__(1024) void k_dyn_nll_reduce(const float* __restrict__ lterm, const float* __restrict__ gmax,
                                                         const float* __restrict__ gmin, int K, int bs, int rows, int D,
                                                         const float* __restrict__ params, float* __restrict__ G, long P, long off_max,
                                                         long off_min, float coef, float* __restrict__ nll_out) {
  __shared__ float red[3 * 64];
  const int r = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nw = blockDim.x >> 6;
  for (int c = w; c < 3 * D; c += nw) {
    const float s = dyn_col_sum(lterm, gmax, gmin, c, D, r, K, bs, 0, rows, lane);
    if (lane == 0) red[c] = s;
  }
  __syncthreads();
  dyn_reduce_tail(red, r, rows, D, params, G, P, off_max, off_min, coef, nll_out);
}

struct DynAdamP {
  float* params; float* m; float* v; const float* G;
  long P;
  int nseg;
  long seg_b[12], seg_e[12];
  float seg_wd[12];
  const int* active;
  const long long* t0;
  int batch;
  float lr, b1, b2, eps;
  float* decay_part;
  int nblk;
};

// torch.optim.Adam (exp_avg lerp, exp_avg_sq, bias corrections of the run's own step count) on the trainable tensors of one run; the
// gradient of the decay loss 0.5 wd_l sum W_l^2 (wd_l W_l) is added to the weights' gradients here and the decay loss of the weights
// read (those of the minibatch's forward pass) is reduced into decay_part[r][block].  Four floats per thread (tensors are 16-B aligned).
__global__ __launch_bounds__(256) void k_dyn_adam(DynAdamP p) {
  __shared__ float s_step, s_bc2s;
  const int r = blockIdx.y;
  if (!p.active[r]) return;                                   // uniform per block
  if (threadIdx.x == 0) {
    const double t = (double)(p.t0[r] + p.batch + 1);
    const double bc1 = 1.0 - pow((double)p.b1, t), bc2 = 1.0 - pow((double)p.b2, t);
    s_step = (float)((double)p.lr / bc1);
    s_bc2s = (float)sqrt(bc2);
  }
  __syncthreads();
  const long i0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  float dec = 0.f;
  int sg = -1;
  for (int s = 0; s < p.nseg; ++s)
    if (i0 >= p.seg_b[s] && i0 < p.seg_e[s]) sg = s;
  if (sg >= 0) {
    const long o = r * p.P + i0;
    const float wd = p.seg_wd[sg];
    const int cnt = (int)min(4L, p.seg_e[sg] - i0);
    for (int j = 0; j < cnt; ++j) {
      const float w = p.params[o + j];
      const float g = p.G[o + j] + wd * w;
      dec += w * w;
      const float m = p.m[o + j] + (g - p.m[o + j]) * (1.0f - p.b1);
      const float v = p.v[o + j] * p.b2 + (1.0f - p.b2) * g * g;
      p.m[o + j] = m; p.v[o + j] = v;
      p.params[o + j] = w - s_step * (m / (sqrtf(v) / s_bc2s + p.eps));
    }
    dec *= 0.5f * wd;
  }
  dec = block_sum256_pairwise(dec);
  if (threadIdx.x == 0) p.decay_part[(long)r * p.nblk + blockIdx.x] = dec;
}

// loss_sum[r] += nll[r] + sum_b decay_part[r][b] for the active runs (fixed order)
__global__ __launch_bounds__(256) void k_dyn_loss(const float* __restrict__ nll, const float* __restrict__ decay_part, int nblk,
                                                  const int* __restrict__ active, float* __restrict__ loss_sum) {
  const int r = blockIdx.x;
  if (!active[r]) return;
  float s = 0.f;
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) s += decay_part[(long)r * nblk + b];
  s = block_sum256_pairwise(s);
  if (threadIdx.x == 0) loss_sum[r] += nll[r] + s;
}

// validate(): mse[r][k] = mean over (row, dim) of (mean - target)^2; OUT [r][k][H][op], T [r][H][D]
__global__ __launch_bounds__(256) void k_dyn_val_mse(const float* __restrict__ OUT, int op, const float* __restrict__ T, int H, int D,
                                                     int K, float* __restrict__ mse) {
  const int k = blockIdx.x, r = blockIdx.y;
  float s = 0.f;
  const long n = (long)H * D;
  for (long e = threadIdx.x; e < n; e += blockDim.x) {
    const long i = e / D; const int d = (int)(e - i * D);
    const float diff = OUT[(((long)r * K + k) * H + i) * op + d] - T[((long)r * H + i) * D + d];
    s += diff * diff;
  }
  s = block_sum256_pairwise(s);
  if (threadIdx.x == 0) mse[r * K + k] = s / (float)n;
}

enum { DYN_MAXD = 64 };

struct DynHeadP {
  const float* OUT; int op;
  const float* obs; long n; int od, D, K;
  const float* params; long P, off_max, off_min;
  const float* noise; const int* midx;
  const int* elites; int n_elites;
  uint64_t seed; uint64_t call;
  int mode; float coef;
  float* next_obs; float* reward; float* raw_reward; float* penalty; int* midx_out;
};

// step()'s head, one thread per (run, row): soft_clamp, mean[:-1] += obs, std = sqrt(exp(logvar)), the sample of the chosen member
// (mean + eps std: double like the reference's float64 noise, then fp32) and the penalty over ALL members
__global__ __launch_bounds__(256) void k_dyn_head(DynHeadP p) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (i >= p.n) return;
  const int D = p.D, od = p.od, K = p.K;
  const float* mx = p.params + r * p.P + p.off_max;
  const float* mn = p.params + r * p.P + p.off_min;
  const float* obs = p.obs + ((long)r * p.n + i) * od;
  auto mean_at = [&](int k, int d) {
    float m = p.OUT[(((long)r * K + k) * p.n + i) * p.op + d];
    if (d < od) m += obs[d];
    return m;
  };
  auto std_at = [&](int k, int d) {
    return dyn_std(p.OUT[(((long)r * K + k) * p.n + i) * p.op + D + d], mx[d], mn[d]);
  };
  int mi;
  uint32_t rnd[4];
  const Philox ph(p.seed);
  if (p.midx) mi = p.midx[(long)r * p.n + i];
  else {
    ph((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)r, (uint32_t)(0x80000000u | (uint32_t)p.call), rnd);
    mi = dyn_draw_elite(p.elites, r, K, p.n_elites, rnd[0]);
  }
  for (int d0 = 0; d0 < D; d0 += 4) {
    if (!p.noise) ph((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)r, ((uint32_t)p.call << 8) | (uint32_t)(d0 >> 2), rnd);
    for (int j = 0; j < 4 && d0 + j < D; ++j) {
      const int d = d0 + j;
      const double eps = p.noise ? (double)p.noise[(((long)r * K + mi) * p.n + i) * D + d] : (double)box_muller_one(rnd, j);
      const float s = (float)((double)mean_at(mi, d) + eps * (double)std_at(mi, d));
      if (d < od) p.next_obs[((long)r * p.n + i) * od + d] = s;
      else p.raw_reward[(long)r * p.n + i] = s;
    }
  }
  double pen = 0.0;
  if (p.mode == ORL_DYN_PENALTY_ALEATORIC) {
    for (int k = 0; k < K; ++k) {
      double ss = 0.0;
      for (int d = 0; d < D; ++d) { const double s = std_at(k, d); ss += s * s; }
      pen = fmax(pen, sqrt(ss));
    }
  } else {
    float mbar[DYN_MAXD];
    for (int d = 0; d < od; ++d) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += mean_at(k, d);
      mbar[d] = (float)(s / K);
    }
    if (p.mode == ORL_DYN_PENALTY_PAIRWISE_DIFF) {
      for (int k = 0; k < K; ++k) {
        double ss = 0.0;
        for (int d = 0; d < od; ++d) { const double df = (double)(mean_at(k, d) - mbar[d]); ss += df * df; }
        pen = fmax(pen, sqrt(ss));
      }
    } else {
      double vs = 0.0;
      for (int d = 0; d < od; ++d) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) { const double df = (double)mean_at(k, d) - (double)mbar[d]; s += df * df; }
        vs += s / K;
      }
      pen = sqrt(vs / od);
    }
  }
  const float penf = (float)pen;
  const float raw = p.raw_reward[(long)r * p.n + i];
  p.penalty[(long)r * p.n + i] = penf;
  p.reward[(long)r * p.n + i] = dyn_sub_mul(raw, p.coef, penf);
  if (p.midx_out) p.midx_out[(long)r * p.n + i] = mi;
}

// ---- MOBILE's next-state samples (reference: dynamics/ensemble_dynamics.py:82-99): orl_dynsample_next ----
struct DynSampleNextP {
  const float* OUT; int op;
  const float* obs; long n; int od, D, K, S, E;
  const float* params; long P, off_max, off_min;
  const float* noise;                 // [R][S][E][n][D] or null
  const int* elites;                  // [R][K], the first E entries in set_elites order
  uint64_t seed; uint64_t call;
  float* next_obs;                    // [R][S * E * n][od], row (s * E + e) * n + b
};

// one thread per (run, sample s, elite position e, row b, four output dims): mean_m + eps std_m of elite m = elites[e], std_m from
// dyn_std like k_dyn_head's; the reward column is drawn like the others and dropped
__global__ __launch_bounds__(256) void k_dyn_sample_next(DynSampleNextP p) {
  const int nq = (p.D + 3) >> 2;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  const long rows = (long)p.S * p.E * p.n;
  if (t >= rows * nq) return;
  const long row = t / nq;
  const int q = (int)(t - row * nq);
  const long se = row / p.n, b = row - se * p.n;
  const int e = (int)(se % p.E);
  const int D = p.D, od = p.od, K = p.K;
  const int mi = p.elites[r * K + e];
  const float* mx = p.params + r * p.P + p.off_max;
  const float* mn = p.params + r * p.P + p.off_min;
  uint32_t rnd[4];
  if (!p.noise) Philox(p.seed)((uint32_t)b, (uint32_t)se, (uint32_t)r, ((uint32_t)p.call << 8) | (uint32_t)q, rnd);
  const float* out = p.OUT + (((long)r * K + mi) * p.n + b) * p.op;
  const float* obs = p.obs + ((long)r * p.n + b) * od;
  float* dst = p.next_obs + ((long)r * rows + row) * od;
  for (int j = 0; j < 4 && 4 * q + j < od; ++j) {
    const int d = 4 * q + j;
    const float eps = p.noise ? p.noise[((long)r * rows + row) * D + d] : box_muller_one(rnd, j);
    const float mean = out[d] + obs[d];
    // two roundings in fp32: the reference's mean + torch.randn_like(std) * std
    dst[d] = __fadd_rn(mean, __fmul_rn(eps, dyn_std(out[D + d], mx[d], mn[d])));
  }
}

// k_dyn_sample_next's samples written straight into the operands of MOBILE's penalty pass (orl::dynsample_enqueue, the device loop of
// orl_mobile_learn_n): the actor's input rows xs (pitch OP) and the observation columns of the target critics' input rows xl (pitch XP)
struct DynSampleRowsP {
  const float* OUT; int op;
  const float* obs; long obs_rs; int obs_pitch;   // the engine's pitched batch slot: row b of run r at obs + r obs_rs + b obs_pitch
  long n; int od, D, K, S, E;
  const float* params; long P, off_max, off_min;
  const int* elites;                  // [R][K], the first E entries in set_elites order
  uint64_t seed; uint64_t call;
  float* xs; long xs_rs; int OP;      // [R][S * E * n][OP], row (s * E + e) * n + b
  float* xl; long xl_rs; int XP;      // [R][S * E * n][XP]
  int ad;
  int vec;                            // both operands 16-byte aligned with pitches and run strides of whole quads: a full quad is one store
};

// one thread per (run, sample s, elite position e, row b, four output dims), the values of k_dyn_sample_next (same Philox counter, same
// two roundings; the reward column is drawn and dropped).  The row's last quad also zeroes the pad columns [od, OP) of xs and
// [od + ad, XP) of xl; the action columns [od, od + ad) of xl are the sampling job's
__global__ __launch_bounds__(256) void k_dyn_sample_rows(DynSampleRowsP p) {
  const int nq = (p.D + 3) >> 2;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  const long rows = (long)p.S * p.E * p.n;
  if (t >= rows * nq) return;
  const long row = t / nq;
  const int q = (int)(t - row * nq);
  const long se = row / p.n, b = row - se * p.n;
  const int e = (int)(se % p.E);
  const int D = p.D, od = p.od, K = p.K;
  const int mi = p.elites[r * K + e];
  const float* mx = p.params + r * p.P + p.off_max;
  const float* mn = p.params + r * p.P + p.off_min;
  uint32_t rnd[4];
  Philox(p.seed)((uint32_t)b, (uint32_t)se, (uint32_t)r, ((uint32_t)p.call << 8) | (uint32_t)q, rnd);
  const float* out = p.OUT + (((long)r * K + mi) * p.n + b) * p.op;
  const float* obs = p.obs + r * p.obs_rs + b * p.obs_pitch;
  float* a = p.xs + r * p.xs_rs + row * p.OP;
  float* x = p.xl + r * p.xl_rs + row * p.XP;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < 4 && 4 * q + j < od; ++j) {
    const int d = 4 * q + j;
    const float eps = box_muller_one(rnd, j);
    const float mean = out[d] + obs[d];
    // two roundings in fp32: the reference's mean + torch.randn_like(std) * std
    v[j] = __fadd_rn(mean, __fmul_rn(eps, dyn_std(out[D + d], mx[d], mn[d])));
  }
  if (p.vec && 4 * q + 3 < od) {
    const float4 v4 = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(a + 4 * q) = v4;
    *reinterpret_cast<float4*>(x + 4 * q) = v4;
  } else {
    for (int j = 0; j < 4 && 4 * q + j < od; ++j) { a[4 * q + j] = v[j]; x[4 * q + j] = v[j]; }
  }
  if (q == nq - 1) {
    for (int c = od; c < p.OP; ++c) a[c] = 0.f;
    for (int c = od + p.ad; c < p.XP; ++c) x[c] = 0.f;
  }
}

// ---- RAMBO's adversarial model update (reference: policy/model_based/rambo.py:129-207): orl_dynadv_* ----
// One update is two calls with the caller's advantage between them:
//   forward   k_dyn_adv_input (scale + concatenate the Ba rollout rows and the Bs dataset rows into ONE input shared by the members,
//             the supervised target), L x E_BIAS_SWISH + E_BIAS with the pre-activations kept, k_dyn_adv_sample
//   update    k_dyn_adv_head (mixture log-prob + policy-gradient term on the rollout rows, the Gaussian NLL on the dataset rows),
//             k_dyn_adv_reduce, ONE backward over the Ba + Bs rows, k_dyn_adam on the adversarial optimizer's state, k_dyn_adv_metrics
// The launches of either call are one host function each (dynadv_forward_launches / dynadv_update_launches): the public entries add
// staging, the synchronise and the metric read-back, the RAMBO device loop of the engine (orl::dynadv_*_enqueue, devobj.h) adds nothing

// rows [0, Ba): scaler(concat(obs, act)), obs kept for the head; rows [Ba, Ba + Bs): scaler(concat(sl_obs, sl_act)) and the target
// T[r][j] = [sl_next_obs - sl_obs, sl_rew]
__global__ void k_dyn_adv_input(const float* __restrict__ obs, const float* __restrict__ act, const float* __restrict__ sl_obs,
                                const float* __restrict__ sl_act, const float* __restrict__ sl_next, const float* __restrict__ sl_rew,
                                int Ba, int Bs, int od, int ad, const float* __restrict__ mu, const float* __restrict__ sd,
                                float* __restrict__ X, int xp, float* __restrict__ T, int D, float* __restrict__ obs_keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  const int N = Ba + Bs;
  if (i >= N) return;
  const bool sl = i >= Ba;
  const long j = sl ? (long)r * Bs + (i - Ba) : (long)r * Ba + i;
  const float* o = (sl ? sl_obs : obs) + j * od;
  const float* a = (sl ? sl_act : act) + j * ad;
  dyn_scale_row(o, od, a, ad, mu + (long)r * (od + ad), sd + (long)r * (od + ad), X + ((long)r * N + i) * xp, xp);
  if (sl) {
    float* t = T + j * D;
    const float* nx = sl_next + j * od;
    for (int c = 0; c < od; ++c) t[c] = nx[c] - o[c];
    t[od] = sl_rew[j];
  } else {
    for (int c = 0; c < od; ++c) obs_keep[j * od + c] = o[c];
  }
}

struct DynAdvSampleP {
  const float* OUT; int op;
  const float* obs; int Ba, N, od, D, K;
  const float* params; long P, off_max, off_min;
  const float* noise; const int* midx;
  const int* elites; int n_elites;
  uint64_t seed; uint64_t call;
  float* next_obs; float* reward; float* S; int* midx_out;
};

// the sampling head, one thread per (run, rollout row, four output dims): s = mean_m + std_m eps_m of the row's member m in fp32
// (torch.normal: eps std rounded, then + mean), kept in S[r][i][D] for the update
__global__ __launch_bounds__(256) void k_dyn_adv_sample(DynAdvSampleP p) {
  const int nq = (p.D + 3) >> 2;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (e >= p.Ba * nq) return;
  const int i = e / nq, q = e - i * nq;
  const int D = p.D, od = p.od, K = p.K;
  const float* mx = p.params + r * p.P + p.off_max;
  const float* mn = p.params + r * p.P + p.off_min;
  int mi;
  uint32_t rnd[4];
  const Philox ph(p.seed);
  if (p.midx) mi = p.midx[(long)r * p.Ba + i];
  else {
    ph((uint32_t)i, 0u, (uint32_t)r, (uint32_t)(0x80000000u | (uint32_t)p.call), rnd);
    mi = dyn_draw_elite(p.elites, r, K, p.n_elites, rnd[0]);
  }
  if (!p.noise) ph((uint32_t)i, 0u, (uint32_t)r, ((uint32_t)p.call << 8) | (uint32_t)q, rnd);
  const float* out = p.OUT + (((long)r * K + mi) * p.N + i) * p.op;
  const long ri = (long)r * p.Ba + i;
  for (int j = 0; j < 4 && 4 * q + j < D; ++j) {
    const int d = 4 * q + j;
    const float eps = p.noise ? p.noise[(((long)r * K + mi) * p.Ba + i) * D + d] : box_muller_one(rnd, j);
    float mean = out[d];
    if (d < od) mean += p.obs[ri * od + d];
    // two roundings in fp32: the reference's torch.distributions.Normal(mean, std).sample() = torch.normal: std * eps, then + mean
    const float s = __fadd_rn(mean, __fmul_rn(dyn_std(out[D + d], mx[d], mn[d]), eps));
    p.S[ri * D + d] = s;
    if (d < od) p.next_obs[ri * od + d] = s;
    else p.reward[ri] = s;
  }
  if (q == 0 && p.midx_out) p.midx_out[ri] = mi;
}

struct DynAdvHeadP {
  const float* OUT; float* dOUT; int op;
  const float* obs; const float* S; const float* T; const float* adv;
  float* lterm; float* gmax; float* gmin; double* rowlp;
  const float* params; long P, off_max, off_min;
  const int* elites; int n_elites;
  int K, D, od, Ba, Bs, wpb;
  float adv_weight;
};

// the head of the update, one WAVE per (run, row), lanes over (member, dim); blockDim = 64 wpb, dynamic LDS wpb (K D + 64) doubles.
// Rollout rows (i < Ba): lp_k = sum_d Normal(mean_k, std_k).log_prob(s) summed in double in dim order, the elite mixture as a
// log-sum-exp (finite where exp(lp_k) underflows), w_k = softmax over the elites (exactly 0 elsewhere) and the gradient
// adv_weight A_i / Ba w_k through mean, soft_clamp and max / min_logvar.  Dataset rows: dyn_nll_elem, as in k_dyn_nll, with Bs rows.
__global__ void k_dyn_adv_head(DynAdvHeadP p) {
  extern __shared__ double adv_sm[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.y;
  const int K = p.K, D = p.D, KD = K * D, N = p.Ba + p.Bs;
  const int i = blockIdx.x * p.wpb + w;
  const bool valid = i < N, roll = valid && i < p.Ba;
  double* lp = adv_sm + (long)w * (KD + 64);
  double* wk = lp + KD;
  const float* mxp = p.params + r * p.P + p.off_max;
  const float* mnp = p.params + r * p.P + p.off_min;
  const long ri = (long)r * p.Ba + i;
  if (roll) {
    for (int e = lane; e < KD; e += 64) {
      const int k = e / D, d = e - k * D;
      const float* out = p.OUT + (((long)r * K + k) * N + i) * p.op;
      float mean = out[d];
      if (d < p.od) mean += p.obs[ri * p.od + d];
      const float sdv = dyn_std(out[D + d], mxp[d], mnp[d]);
      const float z = p.S[ri * D + d] - mean;
      lp[e] = (double)(-(z * z) / (2.f * (sdv * sdv)) - logf(sdv) - 0.91893853320467274178f);
    }
  }
  __syncthreads();
  if (roll) {
    double s = 0.0;
    bool el = false;
    if (lane < K) {
      for (int d = 0; d < D; ++d) s += lp[lane * D + d];
      for (int j = 0; j < p.n_elites; ++j) el = el || (p.elites[r * K + j] == lane);
    }
    double m = el ? s : -INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    const double ex = el ? exp(s - m) : 0.0;
    const double sum = wave_sum(ex);
    wk[lane] = ex / sum;
    if (lane == 0) p.rowlp[ri] = m + log(sum) - log((double)p.n_elites);
  }
  __syncthreads();
  if (!valid) return;
  if (roll) {
    const float c0 = p.adv_weight * p.adv[ri] / (float)p.Ba;
    for (int e = lane; e < KD; e += 64) {
      const int k = e / D, d = e - k * D;
      const long row = ((long)r * K + k) * N + i;
      const float* out = p.OUT + row * p.op;
      float mean = out[d];
      if (d < p.od) mean += p.obs[ri * p.od + d];
      const DynClamp cl = dyn_soft_clamp_grad(out[D + d], mxp[d], mnp[d]);
      const float inv = expf(-cl.lv);
      const float z = p.S[ri * D + d] - mean;
      const float c = c0 * (float)wk[k];
      const float dlv = c * 0.5f * (z * z * inv - 1.f);
      const float dl1 = dlv * cl.s2;
      dyn_store_elem({c * z * inv, dl1 * cl.s1, 0.f, dl1 * (1.f - cl.s1), dlv * (1.f - cl.s2)}, row, d, p.op, D, p.dOUT, p.lterm, p.gmax,
                     p.gmin);
    }
  } else {
    const long tj = (long)r * p.Bs + (i - p.Ba);
    const float scale = 1.0f / ((float)p.Bs * (float)D);
    for (int e = lane; e < KD; e += 64) {
      const int k = e / D, d = e - k * D;
      const long row = ((long)r * K + k) * N + i;
      const DynNll g = dyn_nll_elem(p.OUT[row * p.op + d], p.OUT[row * p.op + D + d], p.T[tj * D + d], mxp[d], mnp[d], scale);
      dyn_store_elem(g, row, d, p.op, D, p.dOUT, p.lterm, p.gmax, p.gmin);
    }
  }
}

// per run (blockIdx.x), 1024 threads, fixed order: the NLL terms' column sums over the dataset rows, the max / min_logvar gradient
// columns over all rows (+coef / -coef), sum_i log_prob_i A_i and sum_i log_prob_i over the rollout rows (double)
__global__ __launch_bounds__(1024) void k_dyn_adv_reduce(const float* __restrict__ lterm, const float* __restrict__ gmax,
                                                         const float* __restrict__ gmin, const double* __restrict__ rowlp,
                                                         const float* __restrict__ adv, int K, int Ba, int Bs, int D,
                                                         const float* __restrict__ params, float* __restrict__ G, long P, long off_max,
                                                         long off_min, float coef, float* __restrict__ nll_out, float* __restrict__ advm) {
  __shared__ float red[3 * 64];
  __shared__ double red2[2];
  const int r = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nw = blockDim.x >> 6;
  const int N = Ba + Bs;
  for (int c = w; c < 3 * D + 2; c += nw) {
    if (c < 3 * D) {
      const int i0 = c < D ? Ba : 0;
      const float s = dyn_col_sum(lterm, gmax, gmin, c, D, r, K, N, i0, N - i0, lane);
      if (lane == 0) red[c] = s;
    } else {
      const bool wa = c == 3 * D;
      double s = 0.0;
      for (int i = lane; i < Ba; i += 64) s += wa ? rowlp[(long)r * Ba + i] * (double)adv[(long)r * Ba + i] : rowlp[(long)r * Ba + i];
      s = wave_sum(s);
      if (lane == 0) red2[c - 3 * D] = s;
    }
  }
  __syncthreads();
  dyn_reduce_tail(red, r, Bs, D, params, G, P, off_max, off_min, coef, nll_out);
  if (threadIdx.x == 0) {
    advm[2 * r] = (float)(red2[0] / (double)Ba);
    advm[2 * r + 1] = (float)(red2[1] / (double)Ba);
  }
}

// metrics[r] = {all_loss, sl_loss (NLL + decay + logvar terms), adv_loss (unweighted), mean log_prob}; zeros for an inactive run
__global__ __launch_bounds__(256) void k_dyn_adv_metrics(const float* __restrict__ nll, const float* __restrict__ decay_part, int nblk,
                                                         const int* __restrict__ active, const float* __restrict__ advm, float adv_weight,
                                                         float* __restrict__ metrics) {
  const int r = blockIdx.x;
  float s = 0.f;
  if (active[r])
    for (int b = threadIdx.x; b < nblk; b += blockDim.x) s += decay_part[(long)r * nblk + b];
  s = block_sum256_pairwise(s);
  if (threadIdx.x == 0) {
    float* m = metrics + 4 * r;
    if (!active[r]) { m[0] = m[1] = m[2] = m[3] = 0.f; return; }
    const float sl = nll[r] + s;
    m[0] = adv_weight * advm[2 * r] + sl;
    m[1] = sl;
    m[2] = advm[2 * r];
    m[3] = advm[2 * r + 1];
  }
}

}  // namespace orl

using namespace orl;

// A training workspace: the matrices of one forward + backward over `rows` rows per (run, member), [R][K][rows][pitch] each.
// `shared`: layer 0's input X is ONE [R][rows][pitch] matrix for the members (member stride 0).  The forward-only step workspace is a
// view of the same type: X, OUT and H[l] alternating between two buffers, `rows` set by each call.
struct DynWs {
  long rows = 0;
  bool shared = false;
  float *X = nullptr, *OUT = nullptr, *dOUT = nullptr, *dA = nullptr, *dB = nullptr;
  float *H[ORL_MAX_HIDDEN] = {}, *Z[ORL_MAX_HIDDEN] = {};
  float *lterm = nullptr, *gmax = nullptr, *gmin = nullptr;
};

struct orl_dynamics {
  orl_dyn_config c;
  int R, K, L, od, ad, in, D, O, B;
  int width[ORL_MAX_HIDDEN + 2], pitch[ORL_MAX_HIDDEN + 2];
  long P = 0, off_max = 0, off_min = 0;
  long w_off[ORL_MAX_HIDDEN + 1], b_off[ORL_MAX_HIDDEN + 1], sw_off[ORL_MAX_HIDDEN + 1], sb_off[ORL_MAX_HIDDEN + 1];
  TensorTable tensors;
  hipStream_t stream = nullptr;
  float *params = nullptr, *adam_m = nullptr, *adam_v = nullptr, *grads = nullptr;
  int* elites_d = nullptr;
  std::vector<std::vector<int64_t>> elites_h;
  std::vector<long long> tstep;
  float *data_in = nullptr, *data_tg = nullptr; long n_data = 0;
  float *mu = nullptr, *sd = nullptr;
  DynWs lw;                                  // learn(): B rows, an input per member
  float *T = nullptr, *decay_part = nullptr, *nll = nullptr, *loss_sum = nullptr;
  int nblk = 0;
  int* active_d = nullptr; long long* t0_d = nullptr;
  int* idx_d = nullptr; long idx_cap = 0;
  // validate / step workspaces, grown on demand: rows capacity
  long s_cap = 0;
  DynWs sw;
  float *sT = nullptr, *sH0 = nullptr, *sH1 = nullptr, *sObs = nullptr, *sAct = nullptr, *sNoise = nullptr;
  float *sNext = nullptr, *sRew = nullptr, *sRaw = nullptr, *sPen = nullptr;
  int *sIdx = nullptr, *sMidx = nullptr, *sMidxOut = nullptr;
  uint64_t step_calls = 0;
  // MOBILE's samples (orl_dynsample_next): its own call counter, host-noise staging and host-output staging, grown on demand
  uint64_t sample_calls = 0;
  long m_cap = 0;
  float *mNoise = nullptr, *mNext = nullptr;
  // RAMBO's adversarial update (orl_dynadv_*): its own optimizer state, workspaces over Ba + Bs rows and the kept sample
  bool adv_on = false, adv_pending = false;
  int aBa = 0, aBs = 0;
  float adv_lr = 0.f, adv_b1 = 0.9f, adv_b2 = 0.999f, adv_eps = 1e-8f, adv_weight = 0.f;
  float *adv_m = nullptr, *adv_v = nullptr;
  std::vector<long long> adv_tstep;
  uint64_t adv_calls = 0;
  DynWs aw;                                  // Ba + Bs rows, one input shared by the members
  float *aT = nullptr, *aS = nullptr, *aObs = nullptr, *aAdv = nullptr, *aAdvm = nullptr, *aMetrics = nullptr;
  double* aRowlp = nullptr;
  float *aInObs = nullptr, *aInAct = nullptr, *aSlObs = nullptr, *aSlAct = nullptr, *aSlNext = nullptr, *aSlRew = nullptr,
        *aNoise = nullptr, *aNext = nullptr, *aRew = nullptr;
  int *aMidx = nullptr, *aMidxOut = nullptr;
  // what orl_dyn_debug_read returns rows of: the row count of the last learn minibatch and of the last validate / step / sample_next
  // (0: no such call, or its workspace has been replaced since), whether that call left targets, and how far the adversarial pair got
  long tap_learn_rows = 0, tap_step_rows = 0;
  bool tap_step_t = false, tap_nll = false, tap_adv_fwd = false, tap_adv_upd = false;
  DevAllocs mem{"orl_dyn"};
};

static int dyn_hmax(const orl_dynamics* d, int last) {      // widest pitch of layers 1 .. last
  int hmax = 4;
  for (int l = 1; l <= last; ++l) hmax = std::max(hmax, d->pitch[l]);
  return hmax;
}

static void dyn_ws_release(orl_dynamics* d, DynWs& w) {
  d->mem.release(&w.X, &w.OUT, &w.dOUT, &w.dA, &w.dB, &w.lterm, &w.gmax, &w.gmin);
  for (int l = 0; l < d->L; ++l) d->mem.release(&w.H[l], &w.Z[l]);
  w.rows = 0;
}
static int dyn_ws_alloc(orl_dynamics* d, DynWs& w, long rows, bool shared) {
  dyn_ws_release(d, w);
  const long RK = (long)d->R * d->K * rows, po = d->pitch[d->L + 1], hmax = dyn_hmax(d, d->L + 1);
  bool bad = d->mem.alloc(&w.X, (shared ? d->R * rows : RK) * d->pitch[0]) || d->mem.alloc(&w.OUT, RK * po) ||
             d->mem.alloc(&w.dOUT, RK * po) || d->mem.alloc(&w.dA, RK * hmax) || d->mem.alloc(&w.dB, RK * hmax) ||
             d->mem.alloc(&w.lterm, RK * d->D) || d->mem.alloc(&w.gmax, RK * d->D) || d->mem.alloc(&w.gmin, RK * d->D);
  for (int l = 0; l < d->L && !bad; ++l) bad = d->mem.alloc(&w.H[l], RK * d->pitch[l + 1]) || d->mem.alloc(&w.Z[l], RK * d->pitch[l + 1]);
  if (bad) return -1;
  w.rows = rows; w.shared = shared;
  return 0;
}

// ---- the matrix products (devobj.h's builders on csrc/gemm.h), batched over (run, member) ----
// layer l's EnsembleLinear weight and bias inside `block` (the parameters or the gradients)
static LinearP dyn_linear(const orl_dynamics* d, float* block, int l) {
  const int in = d->width[l], out = d->width[l + 1];
  return {{block + d->w_off[l], d->P, (long)in * out}, {block + d->b_off[l], d->P, (long)out}, in, out, true, d->K};
}

// Y = act(X W_l + b_l) for every (run, member); epi E_BIAS_SWISH (z to Zo when non-null) or E_BIAS
static int dyn_fwd(orl_dynamics* d, const DevMat& X, int M, int l, const DevMat& Y, float* Zo, bool swish) {
  GemmP p = linear_fwd_p(X, M, dyn_linear(d, d->params, l), Y);
  p.z_out = Zo;
  const int nz = d->R * d->K, cfg = pick_cfg(p.M, p.N, p.K, nz);
  const bool kpad = X.pitch >= rup4(p.K);
  return gemm_done(swish ? launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_SWISH>(cfg, p, nz, d->stream, kpad, false, P_F32)
                         : launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS>(cfg, p, nz, d->stream, kpad, false, P_F32), "orl_dyn forward");
}

// dX = (dY W_l^T) * Swish'(Zin) where Zin is the pre-activation of layer l's input
static int dyn_dgrad(orl_dynamics* d, const DevMat& dY, int M, int l, const DevMat& dX, const DevMat& Zin) {
  GemmP p = linear_dgrad_p(dY, M, dyn_linear(d, d->params, l), dX);
  p.aux = Zin.z(); p.aux_sr = Zin.pitch;
  const int nz = d->R * d->K;
  return gemm_done(launch_gemm<PA_PLAIN, PB_PLAIN, E_SWISH_GRAD>(pick_cfg(p.M, p.N, p.K, nz), p, nz, d->stream, dY.pitch >= rup4(p.K),
                                                                 false, P_F32), "orl_dyn dgrad");
}

// dW_l = X^T dY (stored (in, out)-major like the weight), db_l = column sums of dY, into the gradient block
static int dyn_wgrad(orl_dynamics* d, const DevMat& dY, const DevMat& X, int M, int l) {
  const GemmP p = linear_wgrad_p(dY, X, M, dyn_linear(d, d->grads, l));
  const int nz = d->R * d->K;
  return gemm_done(launch_gemm<PA_PLAIN, PB_PLAIN, E_WGRAD>(pick_cfg(p.M, p.N, p.K, nz), p, nz, d->stream, false, false, P_F32),
                   "orl_dyn wgrad");
}

// k_dyn_adam's arguments less the optimizer (m, v, lr, betas, eps, batch): the trainable segments with their decays
static DynAdamP dyn_adam_params(orl_dynamics* d) {
  DynAdamP a;
  memset(&a, 0, sizeof(a));
  a.params = d->params; a.G = d->grads; a.P = d->P;
  for (int l = 0; l <= d->L; ++l) {
    const long nw = (long)d->K * d->width[l] * d->width[l + 1], nbias = (long)d->K * d->width[l + 1];
    a.seg_b[a.nseg] = d->w_off[l]; a.seg_e[a.nseg] = d->w_off[l] + nw; a.seg_wd[a.nseg++] = d->c.weight_decay[l];
    a.seg_b[a.nseg] = d->b_off[l]; a.seg_e[a.nseg] = d->b_off[l] + nbias; a.seg_wd[a.nseg++] = 0.f;
  }
  a.seg_b[a.nseg] = d->off_max; a.seg_e[a.nseg] = d->off_max + d->D; a.seg_wd[a.nseg++] = 0.f;
  a.seg_b[a.nseg] = d->off_min; a.seg_e[a.nseg] = d->off_min + d->D; a.seg_wd[a.nseg++] = 0.f;
  a.active = d->active_d; a.t0 = d->t0_d;
  a.decay_part = d->decay_part; a.nblk = d->nblk;
  return a;
}

// matrix p of a workspace at layer l's width, and the workspace's layer-0 input
static DevMat dyn_mat(const orl_dynamics* d, const DynWs& w, float* p, int l) {
  const long pt = d->pitch[l];
  return {p, d->K * w.rows * pt, w.rows * pt, (int)pt, (int)pt};
}
static DevMat dyn_input(const orl_dynamics* d, const DynWs& w) {
  DevMat X = dyn_mat(d, w, w.X, 0);
  if (w.shared) { X.s0 = X.s1; X.s1 = 0; }
  return X;
}

// forward of the whole ensemble over the first `rows` rows of a workspace: L x E_BIAS_SWISH (pre-activations to Z when kept), E_BIAS
static int dyn_forward(orl_dynamics* d, const DynWs& w, int rows, bool keep_z) {
  DevMat X = dyn_input(d, w);
  for (int l = 0; l < d->L; ++l) {
    const DevMat Y = dyn_mat(d, w, w.H[l], l + 1);
    if (dyn_fwd(d, X, rows, l, Y, keep_z ? w.Z[l] : nullptr, true)) return -1;
    X = Y;
  }
  return dyn_fwd(d, X, rows, d->L, dyn_mat(d, w, w.OUT, d->L + 1), nullptr, false);
}

// backward from dOUT, top down: weight / bias gradients into the gradient block, input gradients alternating between dA and dB
static int dyn_backward(orl_dynamics* d, const DynWs& w, int rows) {
  DevMat dY = dyn_mat(d, w, w.dOUT, d->L + 1);
  for (int l = d->L; l >= 0; --l) {
    if (dyn_wgrad(d, dY, l ? dyn_mat(d, w, w.H[l - 1], l) : dyn_input(d, w), rows, l)) return -1;
    if (l > 0) {
      const DevMat dX = dyn_mat(d, w, (l & 1) ? w.dB : w.dA, l);
      if (dyn_dgrad(d, dY, rows, l, dX, dyn_mat(d, w, w.Z[l - 1], l))) return -1;
      dY = dX;
    }
  }
  return 0;
}

static int dyn_grow_step(orl_dynamics* d, long rows) {
  if (rows <= d->s_cap) return 0;
  ORL_HIP(hipStreamSynchronize(d->stream));
  DynWs& w = d->sw;
  d->mem.release(&w.X, &d->sT, &d->sH0, &d->sH1, &w.OUT, &d->sObs, &d->sAct, &d->sNoise, &d->sNext, &d->sRew, &d->sRaw, &d->sPen, &d->sIdx,
              &d->sMidx, &d->sMidxOut);
  const long R = d->R, K = d->K;
  const int hmax = dyn_hmax(d, d->L);
  if (d->mem.alloc(&w.X, R * rows * d->pitch[0]) || d->mem.alloc(&d->sT, R * rows * d->D) ||
      d->mem.alloc(&d->sH0, R * K * rows * hmax) || d->mem.alloc(&d->sH1, R * K * rows * hmax) ||
      d->mem.alloc(&w.OUT, R * K * rows * d->pitch[d->L + 1]) || d->mem.alloc(&d->sObs, R * rows * d->od) ||
      d->mem.alloc(&d->sAct, R * rows * d->ad) || d->mem.alloc(&d->sNoise, R * K * rows * d->D) ||
      d->mem.alloc(&d->sNext, R * rows * d->od) || d->mem.alloc(&d->sRew, R * rows) || d->mem.alloc(&d->sRaw, R * rows) ||
      d->mem.alloc(&d->sPen, R * rows) || d->mem.alloc(&d->sIdx, R * rows) || d->mem.alloc(&d->sMidx, R * rows) ||
      d->mem.alloc(&d->sMidxOut, R * rows))
    return -1;
  for (int l = 0; l < d->L; ++l) w.H[l] = (l & 1) ? d->sH1 : d->sH0;
  w.shared = true;
  d->s_cap = rows;
  d->tap_step_rows = 0; d->tap_step_t = false;
  return 0;
}

// parameter block: state_dict order, every tensor 16-B aligned; returns its floats
static long dyn_layout(orl_dynamics* d) {
  TensorTable& t = d->tensors;
  auto add = [&](const std::string& name, std::initializer_list<long> shape) { return t.add(name, shape, false, true); };
  const long K = d->K;
  d->off_max = add("max_logvar", {d->D});
  d->off_min = add("min_logvar", {d->D});
  for (int l = 0; l <= d->L; ++l) {
    const std::string pre = l < d->L ? "backbones." + std::to_string(l) + "." : std::string("output_layer.");
    const long in = d->width[l], o = d->width[l + 1];
    d->w_off[l] = add(pre + "weight", {K, in, o});
    d->b_off[l] = add(pre + "bias", {K, 1, o});
    d->sw_off[l] = add(pre + "saved_weight", {K, in, o});
    d->sb_off[l] = add(pre + "saved_bias", {K, 1, o});
  }
  return t.off;
}

// the elite count that every run shares, or -1 with the refusal of the call named
static int dyn_n_elites(orl_dynamics* d, const char* what) {
  const int E = (int)d->elites_h[0].size();
  for (int r = 1; r < d->R; ++r)
    if ((int)d->elites_h[r].size() != E) return fail(std::string(what) + ": every run needs the same number of elites");
  return E;
}

// teacher-forced member indices: int64 -> int with the range check into h, uploaded to dst on the stream (h lives until the call's
// final synchronise)
static int dyn_upload_midx(orl_dynamics* d, const int64_t* idx, long count, std::vector<int>& h, int* dst, const char* what) {
  h.resize((size_t)count);
  for (long i = 0; i < count; ++i) {
    if (idx[i] < 0 || idx[i] >= d->K) return fail(std::string(what) + ": model index out of range");
    h[i] = (int)idx[i];
  }
  ORL_HIP(hipMemcpyAsync(dst, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, d->stream));
  return 0;
}

// k_dyn_adam's run state: the active flags (into act as well; all runs when null) and the optimizer's step counts; either a blocking
// copy or one on the stream, whose sources then live until the call's final synchronise
static int dyn_upload_run_state(orl_dynamics* d, const int32_t* active, const std::vector<long long>& tstep, std::vector<int>& act,
                                bool on_stream) {
  act.assign(d->R, 1);
  if (active) for (int r = 0; r < d->R; ++r) act[r] = active[r] ? 1 : 0;
  auto upload = [&](void* dst, const void* src, size_t bytes) {
    return on_stream ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream) : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  };
  ORL_HIP(upload(d->active_d, act.data(), sizeof(int) * d->R));
  ORL_HIP(upload(d->t0_d, tstep.data(), sizeof(long long) * d->R));
  return 0;
}

extern "C" {

void orl_dyn_config_default(orl_dyn_config* c) {
  memset(c, 0, sizeof(*c));
  c->obs_dim = 17; c->act_dim = 6;
  c->n_hidden = 4;
  for (int i = 0; i < 4; ++i) c->hidden[i] = 200;
  c->num_ensemble = 7; c->num_elites = 5; c->with_reward = 1;
  const float wd[5] = {2.5e-5f, 5e-5f, 7.5e-5f, 7.5e-5f, 1e-4f};
  for (int i = 0; i < 5; ++i) c->weight_decay[i] = wd[i];
  c->lr = 1e-3f; c->adam_beta1 = 0.9f; c->adam_beta2 = 0.999f; c->adam_eps = 1e-8f;
  c->batch_size = 256; c->logvar_loss_coef = 0.01f;
  c->n_runs = 1; c->device = 0; c->precision = 0; c->seed = 0;
}

int orl_dyn_create(const orl_dyn_config* cfg, orl_dynamics** out) {
  if (!cfg || !out) return fail("orl_dyn_create: null argument");
  *out = nullptr;
  const orl_dyn_config& c = *cfg;
  if (c.n_hidden < 1 || c.n_hidden > ORL_MAX_HIDDEN) return fail("orl_dyn_create: n_hidden must be in [1, 4]");
  if (c.obs_dim < 1 || c.act_dim < 1 || c.batch_size < 1 || c.n_runs < 1) return fail("orl_dyn_create: bad dims");
  if (c.num_ensemble < 1 || c.num_ensemble > 64 || c.num_elites < 1 || c.num_elites > c.num_ensemble)
    return fail("orl_dyn_create: need 1 <= num_elites <= num_ensemble <= 64");
  if (c.obs_dim + (c.with_reward ? 1 : 0) > DYN_MAXD) return fail("orl_dyn_create: obs_dim + with_reward must be <= 64");
  for (int i = 0; i < c.n_hidden; ++i) if (c.hidden[i] < 1) return fail("orl_dyn_create: bad hidden width");
  if (c.precision != 0)
    return fail("orl_dyn_create: the dynamics ensemble implements precision 0 (fp32 MFMA) only; precision 1 / 2 are not supported");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("orl_dyn_create: no HIP device (MI355X) visible");
  if (c.device < 0 || c.device >= ndev) return fail("orl_dyn_create: device ordinal out of range");
  if (hipSetDevice(c.device) != hipSuccess) return fail("orl_dyn_create: hipSetDevice failed");
  orl_dynamics* d = new orl_dynamics();
  d->c = c;
  d->R = c.n_runs; d->K = c.num_ensemble; d->L = c.n_hidden; d->od = c.obs_dim; d->ad = c.act_dim;
  d->in = c.obs_dim + c.act_dim; d->D = c.obs_dim + (c.with_reward ? 1 : 0); d->O = 2 * d->D; d->B = c.batch_size;
  d->width[0] = d->in;
  for (int l = 0; l < d->L; ++l) d->width[l + 1] = c.hidden[l];
  d->width[d->L + 1] = d->O;
  for (int l = 0; l <= d->L + 1; ++l) d->pitch[l] = rup4(d->width[l]);
  d->P = dyn_layout(d);
  const long R = d->R, B = d->B, K = d->K;
  d->nblk = (int)((d->P + 1023) / 1024);
  bool bad = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess;
  if (c.external_arena) d->params = c.external_arena;
  else bad = bad || d->mem.alloc(&d->params, R * d->P);
  bad = bad || d->mem.alloc(&d->adam_m, R * d->P) || d->mem.alloc(&d->adam_v, R * d->P) ||
        d->mem.alloc(&d->grads, R * d->P) || d->mem.alloc(&d->elites_d, R * K) || d->mem.alloc(&d->mu, R * d->in) ||
        d->mem.alloc(&d->sd, R * d->in) || dyn_ws_alloc(d, d->lw, B, false) || d->mem.alloc(&d->T, R * K * B * d->D) ||
        d->mem.alloc(&d->decay_part, R * d->nblk) || d->mem.alloc(&d->nll, R) || d->mem.alloc(&d->loss_sum, R) ||
        d->mem.alloc(&d->active_d, R) || d->mem.alloc(&d->t0_d, R);
  if (bad) {
    const std::string msg = orl_last_error();
    orl_dyn_destroy(d);
    return fail(msg.empty() ? "orl_dyn_create: allocation failed" : msg);
  }
  d->tstep.assign(R, 0);
  d->elites_h.assign(R, std::vector<int64_t>());
  std::vector<int> el(R * K, 0);
  for (int r = 0; r < R; ++r) {
    for (int k = 0; k < c.num_elites; ++k) { d->elites_h[r].push_back(k); el[r * K + k] = k; }
  }
  if (hipMemcpy(d->elites_d, el.data(), sizeof(int) * el.size(), hipMemcpyHostToDevice) != hipSuccess) {
    orl_dyn_destroy(d);
    return fail("orl_dyn_create: elites upload failed");
  }
  // scaler defaults to the identity until orl_dyn_set_scaler
  std::vector<float> one(R * d->in, 1.0f);
  if (hipMemcpy(d->sd, one.data(), sizeof(float) * one.size(), hipMemcpyHostToDevice) != hipSuccess) {
    orl_dyn_destroy(d);
    return fail("orl_dyn_create: scaler upload failed");
  }
  *out = d;
  return 0;
}

void orl_dyn_destroy(orl_dynamics* d) {
  if (!d) return;
  if (d->stream) hipStreamSynchronize(d->stream);
  d->mem.free_all();
  if (d->stream) hipStreamDestroy(d->stream);
  delete d;
}

int orl_dyn_sync(orl_dynamics* d) {
  ORL_HIP(hipStreamSynchronize(d->stream));
  return 0;
}

int64_t orl_dyn_floats(orl_dynamics* d) { return d ? d->P : -1; }

int64_t orl_dyn_config_floats(const orl_dyn_config* c) {
  if (!c || c->n_hidden < 1 || c->n_hidden > ORL_MAX_HIDDEN) return -1;
  orl_dynamics d;
  d.K = c->num_ensemble; d.L = c->n_hidden; d.in = c->obs_dim + c->act_dim; d.D = c->obs_dim + (c->with_reward ? 1 : 0); d.O = 2 * d.D;
  d.width[0] = d.in;
  for (int l = 0; l < d.L; ++l) d.width[l + 1] = c->hidden[l];
  d.width[d.L + 1] = d.O;
  return dyn_layout(&d);
}
int orl_dyn_num_tensors(orl_dynamics* d) { return d ? (int)d->tensors.size() : -1; }

int orl_dyn_tensor(orl_dynamics* d, int idx, char* name, int name_cap, int64_t* offset, int32_t* ndim, int64_t shape[4]) {
  if (!d || d->tensors.query(idx, name, name_cap, offset, ndim, shape)) return fail("orl_dyn_tensor: index out of range");
  return 0;
}

float* orl_dyn_ptr(orl_dynamics* d, int run) { return (d && run >= 0 && run < d->R) ? d->params + (long)run * d->P : nullptr; }

static int dyn_check_run(orl_dynamics* d, int run, int64_t n, const char* what) {
  if (!d) return fail(std::string(what) + ": null handle");
  if (run < 0 || run >= d->R) return fail(std::string(what) + ": run out of range");
  if (n >= 0 && n != d->P) return fail(std::string(what) + ": expected " + std::to_string(d->P) + " floats");
  return 0;
}

int orl_dyn_set(orl_dynamics* d, int run, const float* host, int64_t n) {
  return dyn_check_run(d, run, n, "orl_dyn_set") || block_from_host(d->stream, d->params + (long)run * d->P, host, d->P) ? -1 : 0;
}

int orl_dyn_get(orl_dynamics* d, int run, float* host, int64_t n) {
  return dyn_check_run(d, run, n, "orl_dyn_get") || block_to_host(d->stream, host, d->params + (long)run * d->P, d->P) ? -1 : 0;
}

// one run's Adam moments to (get) or from (set) host arrays, either of which may be null
static int dyn_adam_xfer(orl_dynamics* d, int run, float* dev_m, float* dev_v, const float* m, const float* v, bool get) {
  const float* host[2] = {m, v};
  float* dev[2] = {dev_m + (long)run * d->P, dev_v + (long)run * d->P};
  for (int i = 0; i < 2; ++i) {
    if (!host[i]) continue;
    if (get ? block_to_host(d->stream, const_cast<float*>(host[i]), dev[i], d->P) : block_from_host(d->stream, dev[i], host[i], d->P)) return -1;
  }
  return 0;
}

int orl_dyn_adam_get(orl_dynamics* d, int run, float* m, float* v, int64_t n, int64_t* step) {
  if (dyn_check_run(d, run, n, "orl_dyn_adam_get") || dyn_adam_xfer(d, run, d->adam_m, d->adam_v, m, v, true)) return -1;
  if (step) *step = d->tstep[run];
  return 0;
}

int orl_dyn_adam_set(orl_dynamics* d, int run, const float* m, const float* v, int64_t n, int64_t step) {
  if (dyn_check_run(d, run, n, "orl_dyn_adam_set") || dyn_adam_xfer(d, run, d->adam_m, d->adam_v, m, v, false)) return -1;
  d->tstep[run] = step;
  return 0;
}

int orl_dyn_set_elites(orl_dynamics* d, int run, const int64_t* idx, int n) {
  if (dyn_check_run(d, run, -1, "orl_dyn_set_elites")) return -1;
  if (n < 1 || n > d->K) return fail("orl_dyn_set_elites: need 1 <= n <= num_ensemble");
  std::vector<int> el(d->K, 0);
  for (int i = 0; i < n; ++i) {
    if (idx[i] < 0 || idx[i] >= d->K) return fail("orl_dyn_set_elites: member index out of range");
    el[i] = (int)idx[i];
  }
  ORL_HIP(hipStreamSynchronize(d->stream));
  ORL_HIP(hipMemcpy(d->elites_d + (long)run * d->K, el.data(), sizeof(int) * d->K, hipMemcpyHostToDevice));
  d->elites_h[run].assign(idx, idx + n);
  return 0;
}

int orl_dyn_get_elites(orl_dynamics* d, int run, int64_t* idx, int cap) {
  if (dyn_check_run(d, run, -1, "orl_dyn_get_elites")) return -1;
  const auto& e = d->elites_h[run];
  for (int i = 0; i < (int)e.size() && i < cap; ++i) idx[i] = e[i];
  return (int)e.size();
}

int orl_dyn_load_data(orl_dynamics* d, const float* inputs, const float* targets, int64_t n) {
  if (!d || n < 1) return fail("orl_dyn_load_data: empty dataset");
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->mem.release(&d->data_in, &d->data_tg);
  d->n_data = 0;
  if (d->mem.alloc(&d->data_in, n * d->in) || d->mem.alloc(&d->data_tg, n * d->D)) return -1;
  ORL_HIP(hipMemcpy(d->data_in, inputs, sizeof(float) * n * d->in, hipMemcpyHostToDevice));
  ORL_HIP(hipMemcpy(d->data_tg, targets, sizeof(float) * n * d->D, hipMemcpyHostToDevice));
  d->n_data = n;
  return 0;
}

int orl_dyn_set_scaler(orl_dynamics* d, int run, const float* mu, const float* std) {
  if (dyn_check_run(d, run, -1, "orl_dyn_set_scaler")) return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  ORL_HIP(hipMemcpy(d->mu + (long)run * d->in, mu, sizeof(float) * d->in, hipMemcpyHostToDevice));
  ORL_HIP(hipMemcpy(d->sd + (long)run * d->in, std, sizeof(float) * d->in, hipMemcpyHostToDevice));
  return 0;
}

static int dyn_upload_idx(orl_dynamics* d, const int64_t* idx, long count) {
  std::vector<int> h(count);
  for (long i = 0; i < count; ++i) {
    if (idx[i] < 0 || idx[i] >= d->n_data) return fail("orl_dyn: row index " + std::to_string(idx[i]) + " outside the loaded data");
    h[i] = (int)idx[i];
  }
  if (d->mem.grow(&d->idx_d, &d->idx_cap, count, d->stream)) return -1;
  ORL_HIP(hipMemcpyAsync(d->idx_d, h.data(), sizeof(int) * count, hipMemcpyHostToDevice, d->stream));
  ORL_HIP(hipStreamSynchronize(d->stream));      // h is released on return
  return 0;
}

int orl_dyn_learn_epoch(orl_dynamics* d, const int64_t* idx, int64_t train_size, const int32_t* active, float* loss_out) {
  if (!d || !idx || train_size < 1) return fail("orl_dyn_learn_epoch: bad arguments");
  if (!d->n_data) return fail("orl_dyn_learn_epoch: no data loaded (orl_dyn_load_data)");
  const int R = d->R, K = d->K, B = d->B, D = d->D;
  const DynWs& w = d->lw;
  if (dyn_upload_idx(d, idx, (long)R * K * train_size)) return -1;
  std::vector<int> act;
  if (dyn_upload_run_state(d, active, d->tstep, act, false)) return -1;
  ORL_HIP(hipMemsetAsync(d->loss_sum, 0, sizeof(float) * R, d->stream));
  const long nb = (train_size + B - 1) / B;
  const int p0 = d->pitch[0], po = d->pitch[d->L + 1];
  DynAdamP a = dyn_adam_params(d);
  a.m = d->adam_m; a.v = d->adam_v;
  a.lr = d->c.lr; a.b1 = d->c.adam_beta1; a.b2 = d->c.adam_beta2; a.eps = d->c.adam_eps;
  const long xs1 = (long)B * p0, xs0 = (long)K * xs1;
  for (long b = 0; b < nb; ++b) {
    const int rows = (int)std::min<long>(B, train_size - b * B);
    DEV_LAUNCH(d->stream, k_dyn_gather, dim3((rows + 255) / 256, K, R), dim3(256), 0, (const int*)d->idx_d, (long)K * train_size,
                (long)train_size, b * B, rows, (const float*)d->data_in, (const float*)d->data_tg, d->in, D, (const float*)d->mu,
                (const float*)d->sd, w.X, xs0, xs1, p0, d->T, (long)K * B * D, (long)B * D);
    if (dyn_forward(d, w, rows, true)) return -1;
    // Gaussian NLL head
    const long ne = (long)K * rows * D;
    DEV_LAUNCH(d->stream, k_dyn_nll, dim3((unsigned)((ne + 255) / 256), R), dim3(256), 0, (const float*)w.OUT, w.dOUT, po,
                (const float*)d->T, w.lterm, w.gmax, w.gmin, (const float*)d->params, d->P, d->off_max, d->off_min, K, B, rows, D);
    DEV_LAUNCH(d->stream, k_dyn_nll_reduce, dim3(R), dim3(1024), 0, (const float*)w.lterm, (const float*)w.gmax,
                (const float*)w.gmin, K, B, rows, D, (const float*)d->params, d->grads, d->P, d->off_max, d->off_min,
                d->c.logvar_loss_coef, d->nll);
    if (dyn_backward(d, w, rows)) return -1;
    a.batch = (int)b;
    DEV_LAUNCH(d->stream, k_dyn_adam, dim3(d->nblk, R), dim3(256), 0, a);
    DEV_LAUNCH(d->stream, k_dyn_loss, dim3(R), dim3(256), 0, (const float*)d->nll, (const float*)d->decay_part, d->nblk,
                (const int*)d->active_d, d->loss_sum);
  }
  std::vector<float> ls(R);
  ORL_HIP(hipMemcpyAsync(ls.data(), d->loss_sum, sizeof(float) * R, hipMemcpyDeviceToHost, d->stream));
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->tap_learn_rows = train_size - (nb - 1) * B;
  d->tap_nll = true;
  for (int r = 0; r < R; ++r) {
    if (act[r]) d->tstep[r] += nb;
    if (loss_out) loss_out[r] = act[r] ? (float)((double)ls[r] / (double)nb) : 0.f;
  }
  return 0;
}

int orl_dyn_validate(orl_dynamics* d, const int64_t* idx, int64_t H, float* mse_out) {
  if (!d || !idx || H < 1 || !mse_out) return fail("orl_dyn_validate: bad arguments");
  if (!d->n_data) return fail("orl_dyn_validate: no data loaded (orl_dyn_load_data)");
  const int R = d->R, K = d->K, D = d->D;
  if (dyn_grow_step(d, H)) return -1;
  if (dyn_upload_idx(d, idx, (long)R * H)) return -1;
  DEV_LAUNCH(d->stream, k_dyn_gather, dim3((unsigned)((H + 255) / 256), 1, R), dim3(256), 0, (const int*)d->idx_d, (long)H, 0L, 0L,
              (int)H, (const float*)d->data_in, (const float*)d->data_tg, d->in, D, (const float*)d->mu, (const float*)d->sd, d->sw.X,
              (long)H * d->pitch[0], 0L, d->pitch[0], d->sT, (long)H * D, 0L);
  d->sw.rows = H;
  if (dyn_forward(d, d->sw, (int)H, false)) return -1;
  float* mse = d->sNoise;      // R * K floats of the noise staging (R * K * H * D)
  DEV_LAUNCH(d->stream, k_dyn_val_mse, dim3(K, R), dim3(256), 0, (const float*)d->sw.OUT, d->pitch[d->L + 1], (const float*)d->sT,
              (int)H, D, K, mse);
  ORL_HIP(hipMemcpyAsync(mse_out, mse, sizeof(float) * R * K, hipMemcpyDeviceToHost, d->stream));
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->tap_step_rows = H; d->tap_step_t = true;
  return 0;
}

int orl_dyn_update_save(orl_dynamics* d, int run, const int32_t* mask) {
  if (dyn_check_run(d, run, -1, "orl_dyn_update_save")) return -1;
  float* base = d->params + (long)run * d->P;
  for (int l = 0; l <= d->L; ++l) {
    const long nw = (long)d->width[l] * d->width[l + 1], nbias = d->width[l + 1];
    for (int k = 0; k < d->K; ++k) {
      if (!mask[k]) continue;
      ORL_HIP(hipMemcpyAsync(base + d->sw_off[l] + k * nw, base + d->w_off[l] + k * nw, sizeof(float) * nw, hipMemcpyDeviceToDevice, d->stream));
      ORL_HIP(hipMemcpyAsync(base + d->sb_off[l] + k * nbias, base + d->b_off[l] + k * nbias, sizeof(float) * nbias, hipMemcpyDeviceToDevice, d->stream));
    }
  }
  return 0;
}

int orl_dyn_load_save(orl_dynamics* d, int run) {
  if (dyn_check_run(d, run, -1, "orl_dyn_load_save")) return -1;
  float* base = d->params + (long)run * d->P;
  for (int l = 0; l <= d->L; ++l) {
    const long nw = (long)d->K * d->width[l] * d->width[l + 1], nbias = (long)d->K * d->width[l + 1];
    ORL_HIP(hipMemcpyAsync(base + d->w_off[l], base + d->sw_off[l], sizeof(float) * nw, hipMemcpyDeviceToDevice, d->stream));
    ORL_HIP(hipMemcpyAsync(base + d->b_off[l], base + d->sb_off[l], sizeof(float) * nbias, hipMemcpyDeviceToDevice, d->stream));
  }
  return 0;
}

// step() / sample_next(): scaler(concat(obs, act)) into the step workspace and the ensemble's forward over its n rows
static int dyn_step_forward(orl_dynamics* d, const float* obs, const float* act, long n) {
  DEV_LAUNCH(d->stream, k_dyn_step_input, dim3((unsigned)((n + 255) / 256), d->R), dim3(256), 0, obs, act, n, d->od, d->ad,
              (const float*)d->mu, (const float*)d->sd, d->sw.X, d->pitch[0]);
  d->sw.rows = n;
  return dyn_forward(d, d->sw, (int)n, false);
}

// the launches of a step on device rows: k_dyn_step_input, the ensemble's forward, k_dyn_head; the call counter advances.  orl_dyn_step
// stages around them, dynstep_enqueue (the MBRCSL rollout loop) is nothing else
static int dyn_step_launches(orl_dynamics* d, const float* obs, const float* act, long n, const float* noise, const int* midx, int mode,
                             float coef, float* next_obs, float* reward, float* raw_reward, float* penalty, int* midx_out, const char* who) {
  if (dyn_step_forward(d, obs, act, n)) return -1;
  DynHeadP h;
  memset(&h, 0, sizeof(h));
  h.OUT = d->sw.OUT; h.op = d->pitch[d->L + 1];
  h.obs = obs; h.n = n; h.od = d->od; h.D = d->D; h.K = d->K;
  h.params = d->params; h.P = d->P; h.off_max = d->off_max; h.off_min = d->off_min;
  h.noise = noise; h.midx = midx;
  h.elites = d->elites_d;
  if ((h.n_elites = dyn_n_elites(d, who)) < 0) return -1;
  h.seed = d->c.seed; h.call = d->step_calls++;
  h.mode = mode; h.coef = coef;
  h.next_obs = next_obs; h.reward = reward; h.raw_reward = raw_reward; h.penalty = penalty; h.midx_out = midx_out;
  DEV_LAUNCH(d->stream, k_dyn_head, dim3((unsigned)((n + 255) / 256), d->R), dim3(256), 0, h);
  return 0;
}

int orl_dyn_step(orl_dynamics* d, const float* obs, const float* act, int64_t n, int on_device, const float* noise, const int64_t* model_idx,
                 int mode, float coef, float* next_obs, float* reward, float* raw_reward, float* penalty, int32_t* midx_out) {
  if (!d || !obs || !act || n < 1 || !next_obs || !reward || !raw_reward || !penalty) return fail("orl_dyn_step: bad arguments");
  if (!d->c.with_reward) return fail("orl_dyn_step: needs with_reward (step() splits the reward off the last output)");
  if (mode < 0 || mode > 2) return fail("orl_dyn_step: unknown penalty mode");
  const int R = d->R, K = d->K, D = d->D, od = d->od, ad = d->ad;
  if (dyn_grow_step(d, n)) return -1;
  if (stage_in(d->stream, obs, d->sObs, (size_t)R * n * od, on_device) || stage_in(d->stream, act, d->sAct, (size_t)R * n * ad, on_device) ||
      stage_in(d->stream, noise, d->sNoise, (size_t)R * K * n * D, on_device))
    return -1;
  std::vector<int> mi;
  if (model_idx) {
    if (on_device) return fail("orl_dyn_step: teacher-forced model indices are host arrays");
    if (dyn_upload_midx(d, model_idx, (long)R * n, mi, d->sMidx, "orl_dyn_step")) return -1;
  }
  if (dyn_step_launches(d, obs, act, n, noise, model_idx ? d->sMidx : nullptr, mode, coef, stage_dst(next_obs, d->sNext, on_device),
                        stage_dst(reward, d->sRew, on_device), stage_dst(raw_reward, d->sRaw, on_device),
                        stage_dst(penalty, d->sPen, on_device), stage_dst((int*)midx_out, d->sMidxOut, on_device), "orl_dyn_step"))
    return -1;
  if (stage_out(d->stream, next_obs, d->sNext, (size_t)R * n * od, on_device) || stage_out(d->stream, reward, d->sRew, (size_t)R * n, on_device) ||
      stage_out(d->stream, raw_reward, d->sRaw, (size_t)R * n, on_device) || stage_out(d->stream, penalty, d->sPen, (size_t)R * n, on_device) ||
      stage_out(d->stream, (int*)midx_out, d->sMidxOut, (size_t)R * n, on_device))
    return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->tap_step_rows = n; d->tap_step_t = false;
  return 0;
}

// ---- MOBILE's next-state samples ----
// what orl_dynsample_next and orl::dynsample_enqueue refuse; returns the elite count
static int dyn_sample_elites(orl_dynamics* d, long n, long num_samples, const char* who) {
  const std::string w(who);
  if (num_samples < 1) return fail(w + ": num_samples must be >= 1");
  const int E = dyn_n_elites(d, who);
  if (E < 0) return -1;
  if (E < 2) return fail(w + ": needs at least 2 elites (the standard deviation over one elite is NaN)");
  if (num_samples * E * n * ((d->D + 3) / 4) > (1L << 38) || n > 0x7fffffffL) return fail(w + ": too many rows");
  return E;
}

int orl_dynsample_next(orl_dynamics* d, const float* obs, const float* act, int64_t n, int32_t num_samples, int on_device,
                       const float* noise, float* next_obs) {
  if (!d || !obs || !act || n < 1 || !next_obs) return fail("orl_dynsample_next: bad arguments");
  const int R = d->R, K = d->K, D = d->D, od = d->od, ad = d->ad;
  const int E = dyn_sample_elites(d, (long)n, num_samples, "orl_dynsample_next");
  if (E < 0) return -1;
  const long S = num_samples, rows = S * E * n;
  if (dyn_grow_step(d, n)) return -1;
  if (!on_device && rows > d->m_cap) {
    ORL_HIP(hipStreamSynchronize(d->stream));
    d->mem.release(&d->mNoise, &d->mNext);
    d->m_cap = 0;
    if (d->mem.alloc(&d->mNoise, (size_t)R * rows * D) || d->mem.alloc(&d->mNext, (size_t)R * rows * od)) return -1;
    d->m_cap = rows;
  }
  if (stage_in(d->stream, obs, d->sObs, (size_t)R * n * od, on_device) || stage_in(d->stream, act, d->sAct, (size_t)R * n * ad, on_device) ||
      stage_in(d->stream, noise, d->mNoise, (size_t)R * rows * D, on_device))
    return -1;
  if (dyn_step_forward(d, obs, act, n)) return -1;
  DynSampleNextP p;
  memset(&p, 0, sizeof(p));
  p.OUT = d->sw.OUT; p.op = d->pitch[d->L + 1];
  p.obs = obs; p.n = n; p.od = od; p.D = D; p.K = K; p.S = (int)S; p.E = E;
  p.params = d->params; p.P = d->P; p.off_max = d->off_max; p.off_min = d->off_min;
  p.noise = noise; p.elites = d->elites_d;
  p.seed = d->c.seed ^ 0xD1B54A32D192ED03ull; p.call = d->sample_calls++;
  p.next_obs = stage_dst(next_obs, d->mNext, on_device);
  const long nt = rows * ((D + 3) / 4);
  DEV_LAUNCH(d->stream, k_dyn_sample_next, dim3((unsigned)((nt + 255) / 256), R), dim3(256), 0, p);
  if (stage_out(d->stream, next_obs, d->mNext, (size_t)R * rows * od, on_device)) return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->tap_step_rows = n; d->tap_step_t = false;
  return 0;
}

int64_t orl_dynsample_calls(orl_dynamics* d) {
  if (!d) return fail("orl_dynsample_calls: null handle");
  return (int64_t)d->sample_calls;
}

int orl_dyn_debug_grads(orl_dynamics* d, int run, float* host, int64_t n) {
  return dyn_check_run(d, run, n, "orl_dyn_debug_grads") || block_to_host(d->stream, host, d->grads + (long)run * d->P, d->P) ? -1 : 0;
}

// test tap: the workspaces as the last call left them, nothing on any call's path.  A member block [rows][cols] of src
// [R][members][stride rows][pitch] per member; `members` 1 for the matrices the members share.
int64_t orl_dyn_debug_read(orl_dynamics* d, int run, const char* name, float* host, int64_t cap) {
  if (!d || !name || !host) return fail("orl_dyn_debug_read: bad arguments");
  const std::string nm(name), who = "orl_dyn_debug_read: " + nm;
  if (run < 0 || run >= d->R) return fail(who + ": run out of range");
  const int K = d->K, D = d->D, p0 = d->pitch[0], po = d->pitch[d->L + 1];
  const long N = (long)d->aBa + d->aBs;
  const float* src = nullptr;
  long members = 1, stride = 0, rows = 0;
  int cols = 0, pitch = 0;
  auto view = [&](const float* p, long mem, long st, long n, int c, int pt) {
    src = p; members = mem; stride = st; rows = n; cols = c; pitch = pt;
  };
  const bool learn = nm.compare(0, 6, "learn.") == 0, step = nm.compare(0, 5, "step.") == 0, adv = nm.compare(0, 4, "adv.") == 0;
  const std::string leaf = nm.substr(learn ? 6 : (step ? 5 : (adv ? 4 : 0)));
  if (learn) {
    const DynWs& w = d->lw;
    const long n = d->tap_learn_rows, B = d->B;
    if (leaf == "x") view(w.X, K, B, n, p0, p0);
    else if (leaf == "t") view(d->T, K, B, n, D, D);
    else if (leaf == "out") view(w.OUT, K, B, n, 2 * D, po);
    else if (leaf == "dout") view(w.dOUT, K, B, n, 2 * D, po);
    else if (leaf == "lterm") view(w.lterm, K, B, n, D, D);
    else if (leaf == "gmax") view(w.gmax, K, B, n, D, D);
    else if (leaf == "gmin") view(w.gmin, K, B, n, D, D);
    else if (leaf == "nll") view(d->nll, 1, 1, d->tap_nll ? 1 : 0, 1, 1);                    // shared with orl_dynadv_update
    else if (leaf == "decay") view(d->decay_part, 1, 1, d->tap_nll ? 1 : 0, d->nblk, d->nblk);
    else return fail(who + ": unknown tap");
    if (rows < 1) return fail(who + ": nothing recorded (no orl_dyn_learn_epoch yet)");
  } else if (step) {
    const long n = d->tap_step_rows;
    if (leaf == "x") view(d->sw.X, 1, n, n, p0, p0);
    else if (leaf == "out") view(d->sw.OUT, K, n, n, 2 * D, po);
    else if (leaf == "t") view(d->sT, 1, n, d->tap_step_t ? n : 0, D, D);
    else return fail(who + ": unknown tap");
    if (rows < 1)
      return fail(who + (leaf == "t" ? ": nothing recorded (the last call on the step workspace was not orl_dyn_validate)"
                                     : ": nothing recorded (no orl_dyn_step / orl_dynsample_next / orl_dyn_validate yet)"));
  } else if (adv) {
    const DynWs& w = d->aw;
    const long Ba = d->aBa, Bs = d->aBs;
    bool upd = true;
    if (leaf == "x") { view(w.X, 1, N, N, p0, p0); upd = false; }
    else if (leaf == "t") { view(d->aT, 1, Bs, Bs, D, D); upd = false; }
    else if (leaf == "obs") { view(d->aObs, 1, Ba, Ba, d->od, d->od); upd = false; }
    else if (leaf == "s") { view(d->aS, 1, Ba, Ba, D, D); upd = false; }
    else if (leaf == "out") { view(w.OUT, K, N, N, 2 * D, po); upd = false; }
    else if (leaf == "dout") view(w.dOUT, K, N, N, 2 * D, po);
    else if (leaf == "lterm") view(w.lterm, K, N, N, D, D);
    else if (leaf == "gmax") view(w.gmax, K, N, N, D, D);
    else if (leaf == "gmin") view(w.gmin, K, N, N, D, D);
    else if (leaf == "rowlp") view(nullptr, 1, Ba, Ba, 2, 2);
    else if (leaf == "advm") view(d->aAdvm, 1, 1, 1, 2, 2);
    else return fail(who + ": unknown tap");
    if (!d->adv_on) return fail(who + ": orl_dynadv_configure first");
    if (!d->tap_adv_fwd) return fail(who + ": nothing recorded (no orl_dynadv_forward yet)");
    if (upd && !d->tap_adv_upd) return fail(who + ": nothing recorded (no orl_dynadv_update since the last orl_dynadv_forward)");
  } else {
    return fail(who + ": unknown tap");
  }
  const int64_t total = (int64_t)members * rows * cols;
  if (total > cap) return fail(who + " needs " + std::to_string(total) + " floats");
  ORL_HIP(hipStreamSynchronize(d->stream));
  if (adv && leaf == "rowlp") {      // doubles as (hi, lo) float pairs
    std::vector<double> lp((size_t)rows);
    ORL_HIP(hipMemcpy(lp.data(), d->aRowlp + (long)run * rows, sizeof(double) * rows, hipMemcpyDeviceToHost));
    for (long i = 0; i < rows; ++i) {
      host[2 * i] = (float)lp[i];
      host[2 * i + 1] = (float)(lp[i] - (double)host[2 * i]);
    }
    return total;
  }
  for (long k = 0; k < members; ++k)
    ORL_HIP(hipMemcpy2D(host + k * rows * cols, sizeof(float) * cols, src + ((long)run * members + k) * stride * pitch,
                        sizeof(float) * pitch, sizeof(float) * cols, rows, hipMemcpyDeviceToHost));
  return total;
}

// ---- RAMBO's adversarial update ----
int orl_dynadv_configure(orl_dynamics* d, float lr, float beta1, float beta2, float eps, float adv_weight, int32_t rollout_rows,
                         int32_t sl_rows) {
  if (!d) return fail("orl_dynadv_configure: null handle");
  if (rollout_rows < 1 || sl_rows < 1) return fail("orl_dynadv_configure: need rollout_rows >= 1 and sl_rows >= 1");
  if (!d->c.with_reward) return fail("orl_dynadv_configure: needs with_reward (the sample's last dim is the reward)");
  ORL_HIP(hipStreamSynchronize(d->stream));
  const long R = d->R, K = d->K, D = d->D;
  d->adv_lr = lr; d->adv_b1 = beta1; d->adv_b2 = beta2; d->adv_eps = eps; d->adv_weight = adv_weight;
  if (!d->adv_m) {
    if (d->mem.alloc(&d->adv_m, R * d->P) || d->mem.alloc(&d->adv_v, R * d->P)) return -1;
    d->adv_tstep.assign(R, 0);
  }
  if (d->adv_on && d->aBa == rollout_rows && d->aBs == sl_rows) return 0;
  d->adv_pending = false;
  d->tap_adv_fwd = d->tap_adv_upd = false;
  dyn_ws_release(d, d->aw);
  d->mem.release(&d->aT, &d->aS, &d->aObs, &d->aAdv, &d->aAdvm, &d->aMetrics, &d->aRowlp, &d->aInObs, &d->aInAct, &d->aSlObs, &d->aSlAct,
              &d->aSlNext, &d->aSlRew, &d->aNoise, &d->aNext, &d->aRew, &d->aMidx, &d->aMidxOut);
  d->adv_on = false;
  const long Ba = rollout_rows, Bs = sl_rows;
  if (dyn_ws_alloc(d, d->aw, Ba + Bs, true) || d->mem.alloc(&d->aT, R * Bs * D) || d->mem.alloc(&d->aS, R * Ba * D) ||
      d->mem.alloc(&d->aObs, R * Ba * d->od) || d->mem.alloc(&d->aAdv, R * Ba) || d->mem.alloc(&d->aAdvm, R * 2) ||
      d->mem.alloc(&d->aMetrics, R * 4) || d->mem.alloc(&d->aRowlp, R * Ba) || d->mem.alloc(&d->aInObs, R * Ba * d->od) ||
      d->mem.alloc(&d->aInAct, R * Ba * d->ad) || d->mem.alloc(&d->aSlObs, R * Bs * d->od) ||
      d->mem.alloc(&d->aSlAct, R * Bs * d->ad) || d->mem.alloc(&d->aSlNext, R * Bs * d->od) ||
      d->mem.alloc(&d->aSlRew, R * Bs) || d->mem.alloc(&d->aNoise, R * K * Ba * D) || d->mem.alloc(&d->aNext, R * Ba * d->od) ||
      d->mem.alloc(&d->aRew, R * Ba) || d->mem.alloc(&d->aMidx, R * Ba) || d->mem.alloc(&d->aMidxOut, R * Ba))
    return -1;
  d->aBa = rollout_rows; d->aBs = sl_rows;
  d->adv_on = true;
  return 0;
}

// the launches of a forward on device arrays: input, ensemble forward, sample.  Draws at the call counter, which it advances.  No
// host synchronisation: orl_dynadv_forward and the RAMBO device loop (orl::dynadv_forward_enqueue) share it
static int dynadv_forward_launches(orl_dynamics* d, const float* obs, const float* act, const float* sl_obs, const float* sl_act,
                                   const float* sl_next_obs, const float* sl_rew, const float* noise, const int* midx, float* next_obs,
                                   float* reward, int* midx_out, const char* who) {
  const int R = d->R, K = d->K, D = d->D, od = d->od, ad = d->ad;
  const size_t Ba = d->aBa, Bs = d->aBs, N = Ba + Bs;
  const DynWs& w = d->aw;
  const int p0 = d->pitch[0], po = d->pitch[d->L + 1];
  DEV_LAUNCH(d->stream, k_dyn_adv_input, dim3((unsigned)((N + 255) / 256), R), dim3(256), 0, obs, act, sl_obs, sl_act, sl_next_obs,
              sl_rew, (int)Ba, (int)Bs, od, ad, (const float*)d->mu, (const float*)d->sd, w.X, p0, d->aT, D, d->aObs);
  if (dyn_forward(d, w, (int)N, true)) return -1;
  DynAdvSampleP s;
  memset(&s, 0, sizeof(s));
  s.OUT = w.OUT; s.op = po;
  s.obs = d->aObs; s.Ba = (int)Ba; s.N = (int)N; s.od = od; s.D = D; s.K = K;
  s.params = d->params; s.P = d->P; s.off_max = d->off_max; s.off_min = d->off_min;
  s.noise = noise; s.midx = midx;
  s.elites = d->elites_d;
  if ((s.n_elites = dyn_n_elites(d, who)) < 0) return -1;
  s.seed = d->c.seed ^ 0x9E3779B97F4A7C15ull; s.call = d->adv_calls++;
  s.next_obs = next_obs;
  s.reward = reward;
  s.S = d->aS;
  s.midx_out = midx_out;
  const long ns = Ba * ((D + 3) / 4);
  DEV_LAUNCH(d->stream, k_dyn_adv_sample, dim3((unsigned)((ns + 255) / 256), R), dim3(256), 0, s);
  return 0;
}

int orl_dynadv_forward(orl_dynamics* d, const float* obs, const float* act, const float* sl_obs, const float* sl_act,
                       const float* sl_next_obs, const float* sl_rew, int on_device, const float* noise, const int64_t* model_idx,
                       float* next_obs, float* reward, int32_t* midx_out) {
  if (!d || !obs || !act || !sl_obs || !sl_act || !sl_next_obs || !sl_rew || !next_obs || !reward)
    return fail("orl_dynadv_forward: bad arguments");
  if (!d->adv_on) return fail("orl_dynadv_forward: orl_dynadv_configure first");
  const int R = d->R, K = d->K, D = d->D, od = d->od, ad = d->ad;
  const size_t Ba = d->aBa, Bs = d->aBs;
  d->adv_pending = false;
  if (stage_in(d->stream, obs, d->aInObs, R * Ba * od, on_device) || stage_in(d->stream, act, d->aInAct, R * Ba * ad, on_device) ||
      stage_in(d->stream, sl_obs, d->aSlObs, R * Bs * od, on_device) || stage_in(d->stream, sl_act, d->aSlAct, R * Bs * ad, on_device) ||
      stage_in(d->stream, sl_next_obs, d->aSlNext, R * Bs * od, on_device) || stage_in(d->stream, sl_rew, d->aSlRew, R * Bs, on_device) ||
      stage_in(d->stream, noise, d->aNoise, R * K * Ba * D, on_device))
    return -1;
  std::vector<int> mi;
  if (model_idx && dyn_upload_midx(d, model_idx, (long)(R * Ba), mi, d->aMidx, "orl_dynadv_forward")) return -1;
  if (dynadv_forward_launches(d, obs, act, sl_obs, sl_act, sl_next_obs, sl_rew, noise, model_idx ? d->aMidx : nullptr,
                              stage_dst(next_obs, d->aNext, on_device), stage_dst(reward, d->aRew, on_device),
                              stage_dst((int*)midx_out, d->aMidxOut, on_device), "orl_dynadv_forward"))
    return -1;
  if (stage_out(d->stream, next_obs, d->aNext, R * Ba * od, on_device) || stage_out(d->stream, reward, d->aRew, R * Ba, on_device) ||
      stage_out(d->stream, (int*)midx_out, d->aMidxOut, R * Ba, on_device))
    return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->adv_pending = true;
  d->tap_adv_fwd = true; d->tap_adv_upd = false;
  return 0;
}

// the launches of an update on a device advantage: head, reduce, ONE backward over the Ba + Bs rows, Adam step t0 + batch + 1 of the
// adversarial optimizer, metrics into aMetrics.  The run state (active flags, t0) has been uploaded.  No host synchronisation
static int dynadv_update_launches(orl_dynamics* d, const float* advantage, int batch, const char* who) {
  const int R = d->R, K = d->K, D = d->D;
  const long Ba = d->aBa, Bs = d->aBs, N = Ba + Bs;
  const DynWs& w = d->aw;
  DynAdvHeadP h;
  memset(&h, 0, sizeof(h));
  h.OUT = w.OUT; h.dOUT = w.dOUT; h.op = d->pitch[d->L + 1];
  h.obs = d->aObs; h.S = d->aS; h.T = d->aT; h.adv = advantage;
  h.lterm = w.lterm; h.gmax = w.gmax; h.gmin = w.gmin; h.rowlp = d->aRowlp;
  h.params = d->params; h.P = d->P; h.off_max = d->off_max; h.off_min = d->off_min;
  h.elites = d->elites_d;
  if ((h.n_elites = dyn_n_elites(d, who)) < 0) return -1;
  h.K = K; h.D = D; h.od = d->od; h.Ba = (int)Ba; h.Bs = (int)Bs;
  h.adv_weight = d->adv_weight;
  const size_t per_wave = sizeof(double) * ((size_t)K * D + 64);
  h.wpb = (int)std::max<size_t>(1, std::min<size_t>(4, (32 * 1024) / per_wave));
  if (per_wave > 48 * 1024) return fail(std::string(who) + ": num_ensemble * (obs_dim + 1) is too large for the head's LDS");
  DEV_LAUNCH(d->stream, k_dyn_adv_head, dim3((unsigned)((N + h.wpb - 1) / h.wpb), R), dim3(64 * h.wpb), per_wave * h.wpb, h);
  DEV_LAUNCH(d->stream, k_dyn_adv_reduce, dim3(R), dim3(1024), 0, (const float*)w.lterm, (const float*)w.gmax,
              (const float*)w.gmin, (const double*)d->aRowlp, advantage, K, (int)Ba, (int)Bs, D, (const float*)d->params, d->grads,
              d->P, d->off_max, d->off_min, 0.001f, d->nll, d->aAdvm);
  if (dyn_backward(d, w, (int)N)) return -1;      // ONE backward over the Ba + Bs rows
  DynAdamP a = dyn_adam_params(d);
  a.m = d->adv_m; a.v = d->adv_v;
  a.lr = d->adv_lr; a.b1 = d->adv_b1; a.b2 = d->adv_b2; a.eps = d->adv_eps;
  a.batch = batch;
  DEV_LAUNCH(d->stream, k_dyn_adam, dim3(d->nblk, R), dim3(256), 0, a);
  DEV_LAUNCH(d->stream, k_dyn_adv_metrics, dim3(R), dim3(256), 0, (const float*)d->nll, (const float*)d->decay_part, d->nblk,
              (const int*)d->active_d, (const float*)d->aAdvm, d->adv_weight, d->aMetrics);
  return 0;
}

int orl_dynadv_update(orl_dynamics* d, const float* advantage, int on_device, const int32_t* active, float* metrics_out) {
  if (!d || !advantage) return fail("orl_dynadv_update: bad arguments");
  if (!d->adv_on || !d->adv_pending) return fail("orl_dynadv_update: no pending forward (orl_dynadv_forward first; one update per forward)");
  const int R = d->R;
  const long Ba = d->aBa;
  d->adv_pending = false;
  std::vector<int> act;
  if (dyn_upload_run_state(d, active, d->adv_tstep, act, true)) return -1;
  if (stage_in(d->stream, advantage, d->aAdv, (size_t)R * Ba, on_device)) return -1;
  if (dynadv_update_launches(d, advantage, 0, "orl_dynadv_update")) return -1;
  std::vector<float> ms((size_t)R * 4);
  ORL_HIP(hipMemcpyAsync(ms.data(), d->aMetrics, sizeof(float) * ms.size(), hipMemcpyDeviceToHost, d->stream));
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->tap_adv_upd = true; d->tap_nll = true;
  for (int r = 0; r < R; ++r)
    if (act[r]) d->adv_tstep[r] += 1;
  if (metrics_out) memcpy(metrics_out, ms.data(), sizeof(float) * ms.size());
  return 0;
}

int orl_dynadv_adam_get(orl_dynamics* d, int run, float* m, float* v, int64_t n, int64_t* step) {
  if (dyn_check_run(d, run, n, "orl_dynadv_adam_get")) return -1;
  if (!d->adv_m) return fail("orl_dynadv_adam_get: orl_dynadv_configure first");
  if (dyn_adam_xfer(d, run, d->adv_m, d->adv_v, m, v, true)) return -1;
  if (step) *step = d->adv_tstep[run];
  return 0;
}

int orl_dynadv_adam_set(orl_dynamics* d, int run, const float* m, const float* v, int64_t n, int64_t step) {
  if (dyn_check_run(d, run, n, "orl_dynadv_adam_set")) return -1;
  if (!d->adv_m) return fail("orl_dynadv_adam_set: orl_dynadv_configure first");
  if (dyn_adam_xfer(d, run, d->adv_m, d->adv_v, m, v, false)) return -1;
  d->adv_tstep[run] = step;
  return 0;
}

}  // extern "C"

// ---- the adversarial pair as the RAMBO device loop drives it (algo_rambo.inc: Engine::rambo_loop; declared in devobj.h) ----
namespace orl {

DynStreamLease::DynStreamLease(orl_dynamics* d, hipStream_t loop_stream) : d(d), own(d->stream) { d->stream = loop_stream; }
DynStreamLease::~DynStreamLease() { d->stream = own; }

int dynadv_info(orl_dynamics* d, DynAdvInfo* o) {
  if (!d || !o) return fail("dynadv_info: null handle");
  o->dev = d->c.device; o->R = d->R; o->od = d->od; o->ad = d->ad; o->Ba = d->aBa; o->Bs = d->aBs; o->on = d->adv_on;
  o->stream = d->stream; o->metrics = d->aMetrics;
  return 0;
}

int dynadv_loop_begin(orl_dynamics* d) {
  d->adv_pending = false;
  std::vector<int> act;
  // (blocking copies: the sources are locals; nothing of the loop has been enqueued yet)
  return dyn_upload_run_state(d, nullptr, d->adv_tstep, act, false);
}

int dynadv_forward_enqueue(orl_dynamics* d, const float* obs, const float* act, const float* sl_obs, const float* sl_act,
                           const float* sl_next_obs, const float* sl_rew, float* next_obs, float* reward) {
  return dynadv_forward_launches(d, obs, act, sl_obs, sl_act, sl_next_obs, sl_rew, nullptr, nullptr, next_obs, reward, nullptr,
                                 "orl_rambo_update_dynamics");
}

int dynadv_update_enqueue(orl_dynamics* d, const float* advantage, int step) {
  return dynadv_update_launches(d, advantage, step, "orl_rambo_update_dynamics");
}

void dynadv_loop_end(orl_dynamics* d, long steps_done) {
  for (int r = 0; r < d->R; ++r) d->adv_tstep[r] += steps_done;
  if (steps_done > 0) { d->tap_adv_fwd = d->tap_adv_upd = d->tap_nll = true; }
}

// ---- the model step as the MBRCSL rollout loop drives it (algo_autoreg.inc: Engine::mbrcsl_loop; declared in devobj.h) ----
int dynstep_info(orl_dynamics* d, DynStepInfo* o) {
  if (!d || !o) return fail("dynstep_info: null handle");
  o->dev = d->c.device; o->R = d->R; o->od = d->od; o->ad = d->ad; o->with_reward = d->c.with_reward != 0; o->stream = d->stream;
  return 0;
}

// (before the lease: growing waits for the object's own stream)
int dynstep_loop_begin(orl_dynamics* d, long n_max) { return dyn_grow_step(d, n_max); }

// (the raw reward and the penalty land in the step workspace, as they do for a host caller of orl_dyn_step)
int dynstep_enqueue(orl_dynamics* d, const float* obs, const float* act, long n, int mode, float coef, float* next_obs, float* reward) {
  if (dyn_step_launches(d, obs, act, n, nullptr, nullptr, mode, coef, next_obs, reward, d->sRaw, d->sPen, nullptr, "orl_mbrcsl_rollout")) return -1;
  d->tap_step_rows = n; d->tap_step_t = false;
  return 0;
}

// ---- MOBILE's samples as the device loop of orl_mobile_learn_n drives them (algo_mobile.inc: Engine::mobile_loop; declared in devobj.h) ----
int dynsample_info(orl_dynamics* d, DynSampleInfo* o) {
  if (!d || !o) return fail("dynsample_info: null handle");
  o->dev = d->c.device; o->R = d->R; o->od = d->od; o->ad = d->ad; o->with_reward = d->c.with_reward != 0; o->stream = d->stream;
  o->n_elites = (int)d->elites_h[0].size();
  return 0;
}

// the launches of orl_dynsample_next on the engine's pitched batch rows with the samples written in place: k_dyn_step_input_rows, the
// ensemble's forward, k_dyn_sample_rows; the call counter advances.  No staging, no synchronisation, nothing grown (dynstep_loop_begin
// before the loop)
int dynsample_enqueue(orl_dynamics* d, const DynSampleRows& a, const char* who) {
  if (!d || !a.obs || !a.act || a.n < 1 || !a.xs || !a.xl) return fail(std::string(who) + ": bad arguments");
  const int E = dyn_sample_elites(d, a.n, a.num_samples, who);
  if (E < 0) return -1;
  const long n = a.n;
  if (n > d->s_cap) return fail(std::string(who) + ": the step workspaces hold fewer rows (dynstep_loop_begin before the loop)");
  DEV_LAUNCH(d->stream, k_dyn_step_input_rows, dim3((unsigned)((n + 255) / 256), d->R), dim3(256), 0, a.obs, a.obs_rs, a.obs_pitch, a.act,
             a.act_rs, a.act_pitch, n, d->od, d->ad, (const float*)d->mu, (const float*)d->sd, d->sw.X, d->pitch[0]);
  d->sw.rows = n;
  if (dyn_forward(d, d->sw, (int)n, false)) return -1;
  DynSampleRowsP p;
  memset(&p, 0, sizeof(p));
  p.OUT = d->sw.OUT; p.op = d->pitch[d->L + 1];
  p.obs = a.obs; p.obs_rs = a.obs_rs; p.obs_pitch = a.obs_pitch;
  p.n = n; p.od = d->od; p.D = d->D; p.K = d->K; p.S = a.num_samples; p.E = E;
  p.params = d->params; p.P = d->P; p.off_max = d->off_max; p.off_min = d->off_min;
  p.elites = d->elites_d;
  p.seed = d->c.seed ^ 0xD1B54A32D192ED03ull; p.call = d->sample_calls++;
  p.xs = a.xs; p.xs_rs = a.xs_rs; p.OP = a.OP;
  p.xl = a.xl; p.xl_rs = a.xl_rs; p.XP = a.XP;
  p.ad = d->ad;
  p.vec = ((((uintptr_t)a.xs | (uintptr_t)a.xl) & 15) == 0 && ((a.OP | a.XP) & 3) == 0 && ((a.xs_rs | a.xl_rs) & 3) == 0) ? 1 : 0;
  const long nt = (long)a.num_samples * E * n * ((d->D + 3) / 4);
  DEV_LAUNCH(d->stream, k_dyn_sample_rows, dim3((unsigned)((nt + 255) / 256), d->R), dim3(256), 0, p);
  d->tap_step_rows = n; d->tap_step_t = false;
  return 0;
}

}  // namespace orl
