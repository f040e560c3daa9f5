// diffusion.hip — DiffusionBC on the device (reference: policy/others/diffusion.py, nets/unet.py): orl_diffusion_* of
// include/orl_engine.h.
//
// DiffusionBC calls ConditionalUnet1D with a sequence of length 1.  At that length every Conv1d(k, padding = k / 2) reads its centre
// tap only and the down / up sampling is absent, so the U-Net is a FiLM-conditioned residual MLP:
//   cond    gf = [Linear(Mish(Linear(sinusoidal(t)))) | obs],  mc = Mish(gf), once per pass for every block
//   block   h1 = x W0^T + b0;  y1 = scale * Mish(GN(h1)) + bias;  h2 = y1 W1^T + b1;  out = Mish(GN(h2)) + (x Wr^T + br  or  x)
//           with [scale | bias] = mc Wc^T + bc
//   net     2 blocks per down level (the level's output kept as a skip), 2 mid blocks, 2 blocks per up level on [x | skip],
//           then Linear, GN + Mish, Linear
// One training step is a plain run of launches on one stream:
//   k_diff_input      rows of the attached buffer, t and eps (Philox or teacher-forced), x_t, the sinusoidal embedding, obs into gf
//   tiled GEMMs       every Linear (gemm.h: E_BIAS forward, E_PLAIN dgrad, E_WGRAD weight + bias gradient).  The 2 x n_blocks FiLM
//                     encoders are ONE GEMM over their concatenated output columns; a block with a residual_conv runs [W0; Wr] as one
//                     GEMM in the forward, the dgrad (K = 2 out) and the wgrad (M = 2 out)
//   k_diff_norm_fwd   everything a block does between two GEMMs: GroupNorm statistics of one (row, group) per wave, affine, Mish and
//                     the FiLM or the residual tail
//   k_diff_norm_bwd   its backward: sums the gradient terms of the block's consumers, dX, the FiLM dscale / dbias, and the row's
//                     terms of dgamma / dbeta into a [rows][norm floats] slab that k_diff_colsum adds in row order (no atomics)
//   k_mse_loss<false> the MSE, its seed 2 (pred - eps) / (rows act_dim) (train_ops.h)
//   k_diff_adam_ema   torch.optim.Adam with lr[k] read from the device table, then ema <- ema decay + p (1 - decay)
// Sampling is N forward-only passes on the EMA block with k_diff_ddpm between them and one host synchronisation at the end.
// Allocation, the tensor table, transfers, staging, the workspace matrices, the GemmP and tile choice of a Linear's products and the
// learn-epoch driver come from devobj.h; the wave / block sums and softplus from reduce.h; the norm statistics and backward core, the
// loss and Adam's element update from train_ops.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "devobj.h"
#include "reduce.h"
#include "rng.h"
#include "train_ops.h"

namespace orl {

enum { DIFF_NJ = 8, DIFF_MAX_TERMS = 4 };
enum { DIFF_FINAL_GROUPS = 8 };      // final_conv's Conv1dBlock is built without n_groups: always GroupNorm(8)
enum { DIFF_TAG_T = 1u, DIFF_TAG_EPS = 2u, DIFF_TAG_Z = 3u };     // Philox streams: c3 = tag << 28 | high bits of the counter

// nn.Mish: x tanh(softplus(x)), and what its backward needs
struct DiffMish { float y, dy; };
__device__ __forceinline__ float diff_mish(float x) { return x * tanhf(softplus(x)); }
__device__ __forceinline__ DiffMish diff_mish_grad(float x) {
  const float ts = tanhf(softplus(x));
  const float sg = 1.f / (1.f + expf(-x));
  return {x * ts, ts + x * sg * (1.f - ts * ts)};
}

__device__ __forceinline__ void diff_philox(uint64_t seed, uint32_t row, uint32_t q, uint64_t counter, uint32_t tag, uint32_t (&out)[4]) {
  const Philox ph(seed);
  ph(row, q, (uint32_t)counter, (tag << 28) | (uint32_t)((counter >> 32) & 0x0fffffffu), out);
}

struct DiffInputP {
  int rows, od, ad, OP, AP, dsed, N;
  const long long* idx;            // dataset row per batch row, or null (sampling: obs / x given)
  const float* d_obs; const float* d_act; long n_data;    // dataset, pitches OP / AP
  const float* s_obs;              // sampling: packed [rows][od]
  const long long* t_in; const float* eps_in; // teacher-forced draws or null
  int t_const;                     // sampling: the step of every row (>= 0), training: -1
  const float* acp;
  uint64_t seed, counter;
  float* XT; int xp;               // [rows][xp]: x_t (training only)
  float* EPS; float* TF;           // [rows][ad], [rows] (training only)
  float* E0; int ep;               // sinusoidal embedding [rows][ep]
  float* GF; int gp;               // condition vector [rows][gp]: obs into columns dsed ..
};

// one wave per row
__global__ __launch_bounds__(64) void k_diff_input(DiffInputP p) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= p.rows) return;
  int t = p.t_const;
  const float* obs;
  if (t < 0) {
    const long g = min(max((long)p.idx[i], 0L), p.n_data - 1);          // (host orders are range-checked; a device order is clamped)
    obs = p.d_obs + g * p.OP;
    uint32_t rnd[4];
    if (p.t_in) t = (int)p.t_in[i];
    else {
      diff_philox(p.seed, (uint32_t)i, 0u, p.counter, DIFF_TAG_T, rnd);
      t = (int)(((uint64_t)rnd[0] * (uint64_t)p.N) >> 32);
    }
    const float sa = sqrtf(p.acp[t]), sb = sqrtf(1.f - p.acp[t]);
    for (int d = lane; d < p.ad; d += 64) {
      float e;
      if (p.eps_in) e = p.eps_in[(long)i * p.ad + d];
      else {
        diff_philox(p.seed, (uint32_t)i, (uint32_t)(d >> 2), p.counter, DIFF_TAG_EPS, rnd);
        e = box_muller_one(rnd, d & 3);
      }
      p.EPS[(long)i * p.ad + d] = e;
      p.XT[(long)i * p.xp + d] = __fadd_rn(__fmul_rn(sa, p.d_act[g * p.AP + d]), __fmul_rn(sb, e));
    }
    if (lane == 0) p.TF[i] = (float)t;
  } else {
    obs = p.s_obs + (long)i * p.od;
  }
  const int half = p.dsed >> 1;
  const float step = 9.210340371976184f / (float)(half - 1);          // ln(10000) / (half - 1)
  for (int j = lane; j < half; j += 64) {
    const float a = (float)t * expf((float)j * -step);
    p.E0[(long)i * p.ep + j] = sinf(a);
    p.E0[(long)i * p.ep + half + j] = cosf(a);
  }
  for (int c = lane; c < p.od; c += 64) p.GF[(long)i * p.gp + p.dsed + c] = obs[c];
}

// out = Mish(in) over [rows][cols]
__global__ void k_diff_mish(const float* __restrict__ in, int ip, float* __restrict__ out, int op, int rows, int cols) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)rows * cols) return;
  const int r = (int)(e / cols), c = (int)(e - (long)r * cols);
  out[(long)r * op + c] = diff_mish(in[(long)r * ip + c]);
}
// dz = dy Mish'(z)
__global__ void k_diff_mish_bwd(const float* __restrict__ dy, int dp, const float* __restrict__ z, int zp, float* __restrict__ dz, int op,
                                int rows, int cols) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)rows * cols) return;
  const int r = (int)(e / cols), c = (int)(e - (long)r * cols);
  dz[(long)r * op + c] = dy[(long)r * dp + c] * diff_mish_grad(z[(long)r * zp + c]).dy;
}
// dst[r][c] = src[idx ? idx[r] : r][c]; a gathered row index is clamped to [0, src_rows)
// (not merged with k_rnn_copy: that one addresses by run and time step, this one through a row index)
__global__ void k_diff_copy(const float* __restrict__ src, int sp, const long long* __restrict__ idx, long src_rows,
                            float* __restrict__ dst, int dp, long rows, int cols) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * cols) return;
  const long r = e / cols; const int c = (int)(e - r * cols);
  dst[r * dp + c] = src[(idx ? min(max((long)idx[r], 0L), src_rows - 1) : r) * sp + c];
}

struct DiffNormP {
  int rows, C, cg;                 // channels, channels per group; blockDim = 64 * groups
  const float* h; int hp;          // the Linear's output
  const float* gamma; const float* beta;
  const float* film; int fp;       // FiLM tail: scale = film[row][c], bias = film[row][C + c]; null = none
  const float* res; int rp;        // residual tail or null
  float* out; int op;
  // backward
  int nterm; const float* g[DIFF_MAX_TERMS]; int gpitch[DIFF_MAX_TERMS];    // dOut = the sum of the terms
  float* dsum; int sp;             // dOut itself (the residual path's gradient) or null
  float* dh; int dhp;
  float* dfilm; int dfp;           // dscale at [row][c], dbias at [row][C + c]
  float* part; long pn;            // [row][pn]: dgamma at [c], dbeta at [C + c]
};

// GroupNorm (eps 1e-5, affine) + Mish + the optional FiLM or residual tail; one block per row, one wave per group
__global__ void k_diff_norm_fwd(DiffNormP p) {
  const int row = blockIdx.x, g = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (row >= p.rows) return;
  const int c0 = g * p.cg;
  float v[DIFF_NJ], mean, rstd;
  norm_stats(p.h + (long)row * p.hp + c0, p.cg, lane, v, mean, rstd);
#pragma unroll
  for (int j = 0; j < DIFF_NJ; ++j) {
    const int c = c0 + lane + 64 * j;
    if (lane + 64 * j >= p.cg) break;
    float m = diff_mish((v[j] - mean) * rstd * p.gamma[c] + p.beta[c]);
    if (p.film) m = p.film[(long)row * p.fp + c] * m + p.film[(long)row * p.fp + p.C + c];
    if (p.res) m += p.res[(long)row * p.rp + c];
    p.out[(long)row * p.op + c] = m;
  }
}

__global__ void k_diff_norm_bwd(DiffNormP p) {
  const int row = blockIdx.x, g = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (row >= p.rows) return;
  const int c0 = g * p.cg;
  float v[DIFF_NJ], mean, rstd;
  norm_stats(p.h + (long)row * p.hp + c0, p.cg, lane, v, mean, rstd);
  float dxh[DIFF_NJ], xh[DIFF_NJ];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < DIFF_NJ; ++j) {
    const int c = c0 + lane + 64 * j;
    dxh[j] = 0.f; xh[j] = 0.f;
    if (lane + 64 * j < p.cg) {
      float dy = 0.f;
      for (int k = 0; k < p.nterm; ++k) dy += p.g[k][(long)row * p.gpitch[k] + c];
      if (p.dsum) p.dsum[(long)row * p.sp + c] = dy;
      const float gm = p.gamma[c];
      xh[j] = (v[j] - mean) * rstd;
      const DiffMish m = diff_mish_grad(xh[j] * gm + p.beta[c]);
      float dm = dy;
      if (p.film) {
        p.dfilm[(long)row * p.dfp + c] = dy * m.y;
        p.dfilm[(long)row * p.dfp + p.C + c] = dy;
        dm = dy * p.film[(long)row * p.fp + c];
      }
      const float du = dm * m.dy;
      p.part[(long)row * p.pn + c] = du * xh[j];
      p.part[(long)row * p.pn + p.C + c] = du;
      dxh[j] = du * gm;
      s1 += dxh[j];
      s2 += dxh[j] * xh[j];
    }
  }
  const NormBwd nb(s1, s2, rstd, p.cg);
#pragma unroll
  for (int j = 0; j < DIFF_NJ; ++j) {
    if (lane + 64 * j >= p.cg) break;
    p.dh[(long)row * p.dhp + c0 + lane + 64 * j] = nb.dx(dxh[j], xh[j]);
  }
}

// G[j] = sum over rows (in row order) of part[row][j]: the dgamma / dbeta of every norm in one launch
// (not merged with rnn_dynamics.hip's two-level column sums: the orders of summation differ and the tests pin both)
__global__ void k_diff_colsum(const float* __restrict__ part, long pn, int rows, float* __restrict__ G) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= pn) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += part[(long)r * pn + j];
  G[j] = s;
}

// torch.optim.Adam (exp_avg lerp, exp_avg_sq, the bias corrections of step k + 1) with lr[k] from the device table, then the EMA
__global__ __launch_bounds__(256) void k_diff_adam_ema(float* __restrict__ params, float* __restrict__ m_, float* __restrict__ v_,
                                                       const float* __restrict__ G, float* __restrict__ ema, long P,
                                                       const double* __restrict__ lr_tab, long k, double bc1, float bc2s, float b1, float b2,
                                                       float eps, float decay, float omd) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const float step = (float)(lr_tab[k] / bc1);
  float m = m_[i], v = v_[i];
  const float w = adam_update(params[i], m, v, G[i], step, bc2s, 1.0f - b1, b2, 1.0f - b2, eps);
  m_[i] = m; v_[i] = v;
  params[i] = w;
  ema[i] = __fadd_rn(__fmul_rn(ema[i], decay), __fmul_rn(w, omd));
}

// the DDPM update: x0 = clip((x - s1 e) / s0, -1, 1); x <- c0 x0 + c1 x (+ sigma z for t > 0); coef = {s0, s1, c0, c1, sigma}
__global__ void k_diff_ddpm(float* __restrict__ x, int xp, const float* __restrict__ e, int ep, const float* __restrict__ coef, int t,
                            const float* __restrict__ z_in, float* __restrict__ z_keep, long n, int ad, uint64_t seed, uint64_t counter) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n * ad) return;
  const long i = id / ad; const int d = (int)(id - i * ad);
  const float* c = coef + 5 * t;
  const float xv = x[i * xp + d];
  const float x0 = fminf(fmaxf((xv - c[1] * e[i * ep + d]) / c[0], -1.f), 1.f);
  float nx = __fadd_rn(__fmul_rn(c[2], x0), __fmul_rn(c[3], xv));
  if (t > 0) {
    float z;
    if (z_in) z = z_in[id];
    else {
      uint32_t rnd[4];
      diff_philox(seed, (uint32_t)i, (uint32_t)(d >> 2) | ((uint32_t)(i >> 32) << 8), counter, DIFF_TAG_Z, rnd);
      z = box_muller_one(rnd, d & 3);
    }
    z_keep[id] = z;
    nx = __fadd_rn(nx, __fmul_rn(c[4], z));
  }
  x[i * xp + d] = nx;
}

}  // namespace orl

using namespace orl;

struct DiffBlock {
  int in, out; bool res;
  long w0, b0, w1, b1;             // [W0; Wr] stacked when res (2 out rows), likewise [b0; br]
  long n0, n1;                     // [gamma | beta] of the two norms inside the norm region (offsets from its start)
  int film_col;                    // first column of the block's [scale | bias] in the FiLM matrix
  int src;                         // input: -1 the net's input, else the output of block src ...
  int skip;                        // ... concatenated with the output of block skip (>= 0)
};
// activations of one pass over `cap` rows; the backward's buffers when train
struct DiffWs {
  long cap = 0; bool train = false;
  DevMat XT, E0, Z1, M1, GF, MC, FILM, HF, YF, PRED;
  std::vector<DevMat> CAT, HR, Y1, H2, OUT;
  // backward
  DevMat dPRED, dYF, dHF, dLAST, dFILM, dMC, dE, dM1, dZ1, dH2, dY1;
  std::vector<DevMat> D2, DR, DX;
  float* part = nullptr;
};

struct orl_diffusion {
  orl_diffusion_config c;
  int od, ad, dsed, cond, N, B, G, nlev;
  std::vector<DiffBlock> blocks;
  int last_block = 0;
  long P = 0, s1w = 0, s1b = 0, s2w = 0, s2b = 0, f0w = 0, f0b = 0, f1w = 0, f1b = 0, fn = 0, cw = 0, cb = 0, norm_off = 0, norm_n = 0;
  int film_cols = 0, start_dim = 0;
  TensorTable tensors;
  hipStream_t stream = nullptr;
  float *params = nullptr, *ema = nullptr, *adam_m = nullptr, *adam_v = nullptr, *grads = nullptr;
  float *acp = nullptr, *coef = nullptr; bool have_sched = false;
  double* lr_tab = nullptr; long n_lr = 0;
  long long kstep = 0;
  uint64_t sample_calls = 0;
  // dataset
  const float *d_obs = nullptr, *d_act = nullptr; int OP = 0, AP = 0; long n_data = 0;
  DiffWs tw, sw;
  long long *idx_d = nullptr, *t_d = nullptr; long idx_cap = 0;
  float *eps_in = nullptr, *EPS = nullptr, *TF = nullptr, *loss_cell = nullptr, *loss_steps = nullptr; long loss_cap = 0;
  // sampling staging
  long s_cap = 0, s_noise_cap = 0;
  float *sObs = nullptr, *sX = nullptr, *sNoise = nullptr, *sZ = nullptr, *sZkeep = nullptr, *sOut = nullptr;
  long long* sIdx = nullptr;
  long last_sample_n = 0; int last_rows = 0;
  DevAllocs mem{"orl_diffusion"};
};

static int diff_ws_alloc(orl_diffusion* d, DiffWs& w, long rows, bool train) {
  const size_t nb = d->blocks.size();
  w.CAT.resize(nb); w.HR.resize(nb); w.Y1.resize(nb); w.H2.resize(nb); w.OUT.resize(nb);
  w.D2.resize(nb); w.DR.resize(nb); w.DX.resize(nb);
  bool bad = dev_mat(d->mem, w.XT, rows, d->ad) || dev_mat(d->mem, w.E0, rows, d->dsed) || dev_mat(d->mem, w.Z1, rows, 4 * d->dsed) ||
             dev_mat(d->mem, w.M1, rows, 4 * d->dsed) || dev_mat(d->mem, w.GF, rows, d->cond) || dev_mat(d->mem, w.MC, rows, d->cond) ||
             dev_mat(d->mem, w.FILM, rows, d->film_cols) || dev_mat(d->mem, w.HF, rows, d->start_dim) || dev_mat(d->mem, w.YF, rows, d->start_dim) ||
             dev_mat(d->mem, w.PRED, rows, d->ad);
  int wmax = 4;
  for (size_t b = 0; b < nb && !bad; ++b) {
    const DiffBlock& k = d->blocks[b];
    wmax = std::max(wmax, k.out);
    bad = (k.skip >= 0 && dev_mat(d->mem, w.CAT[b], rows, k.in)) || dev_mat(d->mem, w.HR[b], rows, k.res ? 2 * k.out : k.out) ||
          dev_mat(d->mem, w.Y1[b], rows, k.out) || dev_mat(d->mem, w.H2[b], rows, k.out) || dev_mat(d->mem, w.OUT[b], rows, k.out);
    if (train && !bad)
      bad = dev_mat(d->mem, w.D2[b], rows, k.res ? 2 * k.out : k.out) || (!k.res && dev_mat(d->mem, w.DR[b], rows, k.out)) ||
            (k.src >= 0 && dev_mat(d->mem, w.DX[b], rows, k.in));
  }
  if (train && !bad)
    bad = dev_mat(d->mem, w.dPRED, rows, d->ad) || dev_mat(d->mem, w.dYF, rows, d->start_dim) || dev_mat(d->mem, w.dHF, rows, d->start_dim) ||
          dev_mat(d->mem, w.dLAST, rows, d->start_dim) || dev_mat(d->mem, w.dFILM, rows, d->film_cols) || dev_mat(d->mem, w.dMC, rows, d->cond) ||
          dev_mat(d->mem, w.dE, rows, d->dsed) || dev_mat(d->mem, w.dM1, rows, 4 * d->dsed) || dev_mat(d->mem, w.dZ1, rows, 4 * d->dsed) ||
          dev_mat(d->mem, w.dH2, rows, wmax) || dev_mat(d->mem, w.dY1, rows, wmax) ||
          (d->mem.free(w.part), d->mem.alloc(&w.part, (size_t)rows * d->norm_n));
  if (bad) return -1;
  w.cap = rows; w.train = train;
  return 0;
}

// ---- the matrix products (csrc/gemm.h), one problem per launch ----
// the nn.Linear at offsets w / b of `block` (the parameters, the EMA or the gradients): W [out][in]
static LinearP diff_linear(float* block, long w, long b, int in, int out) { return {{block + w, 0, 0}, {block + b, 0, 0}, in, out, false, 1}; }
// Y = X W^T + b
static int diff_fwd(orl_diffusion* d, float* base, const DevMat& X, int M, long w, long b, int in, int out, const DevMat& Y) {
  const GemmP p = linear_fwd_p(X, M, diff_linear(base, w, b, in, out), Y);
  return gemm_done(launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS>(linear_cfg(p.M, p.N), p, 1, d->stream, false, false, P_F32), "orl_diffusion forward");
}
// dX = dY W
static int diff_dgrad(orl_diffusion* d, const DevMat& dY, int M, long w, int in, int out, const DevMat& dX) {
  const GemmP p = linear_dgrad_p(dY, M, diff_linear(d->params, w, 0, in, out), dX);
  return gemm_done(launch_gemm<PA_PLAIN, PB_PLAIN, E_PLAIN>(linear_cfg(p.M, p.N), p, 1, d->stream, false, false, P_F32), "orl_diffusion dgrad");
}
// dW = dY^T X ([out][in]) and db = the column sums of dY into the gradient block
static int diff_wgrad(orl_diffusion* d, const DevMat& dY, const DevMat& X, int M, long w, long b, int in, int out) {
  const GemmP p = linear_wgrad_p(dY, X, M, diff_linear(d->grads, w, b, in, out));
  return gemm_done(launch_gemm<PA_PLAIN, PB_PLAIN, E_WGRAD>(pick_cfg(p.M, p.N, p.K, 1), p, 1, d->stream, false, false, P_F32), "orl_diffusion wgrad");
}

static DiffNormP diff_norm_params(orl_diffusion* d, const float* base, int rows, int C, const DevMat& h, long noff, int groups) {
  DiffNormP p;
  memset(&p, 0, sizeof(p));
  p.rows = rows; p.C = C; p.cg = C / groups;
  p.h = h.p; p.hp = h.pitch;
  p.gamma = base + d->norm_off + noff; p.beta = p.gamma + C;
  return p;
}

// the forward pass over `rows` rows of workspace w on the parameter block `base` (the trained one or the EMA); E0, GF[:, dsed:] and
// x (the net's input) are already in place
static int diff_forward(orl_diffusion* d, DiffWs& w, float* base, int rows, const DevMat& x) {
  const int ds = d->dsed;
  if (diff_fwd(d, base, w.E0, rows, d->s1w, d->s1b, ds, 4 * ds, w.Z1)) return -1;
  DEV_LAUNCH(d->stream, k_diff_mish, dim3(ew_grid((long)rows * 4 * ds)), dim3(256), 0, w.Z1.p, w.Z1.pitch, w.M1.p, w.M1.pitch, rows, 4 * ds);
  if (diff_fwd(d, base, w.M1, rows, d->s2w, d->s2b, 4 * ds, ds, w.GF)) return -1;
  DEV_LAUNCH(d->stream, k_diff_mish, dim3(ew_grid((long)rows * d->cond)), dim3(256), 0, w.GF.p, w.GF.pitch, w.MC.p, w.MC.pitch, rows, d->cond);
  if (diff_fwd(d, base, w.MC, rows, d->cw, d->cb, d->cond, d->film_cols, w.FILM)) return -1;
  for (size_t b = 0; b < d->blocks.size(); ++b) {
    const DiffBlock& k = d->blocks[b];
    DevMat X = k.src < 0 ? x : w.OUT[k.src];
    if (k.skip >= 0) {
      const int c1 = d->blocks[k.src].out, c2 = d->blocks[k.skip].out;
      DEV_LAUNCH(d->stream, k_diff_copy, dim3(ew_grid((long)rows * c1)), dim3(256), 0, X.p, X.pitch, (const long long*)nullptr, 0L, w.CAT[b].p,
                  w.CAT[b].pitch, (long)rows, c1);
      DEV_LAUNCH(d->stream, k_diff_copy, dim3(ew_grid((long)rows * c2)), dim3(256), 0, w.OUT[k.skip].p, w.OUT[k.skip].pitch, (const long long*)nullptr, 0L,
                  w.CAT[b].p + c1, w.CAT[b].pitch, (long)rows, c2);
      X = w.CAT[b];
    }
    if (diff_fwd(d, base, X, rows, k.w0, k.b0, k.in, k.res ? 2 * k.out : k.out, w.HR[b])) return -1;
    DiffNormP n0 = diff_norm_params(d, base, rows, k.out, w.HR[b], k.n0, d->G);
    n0.film = w.FILM.p + k.film_col; n0.fp = w.FILM.pitch;
    n0.out = w.Y1[b].p; n0.op = w.Y1[b].pitch;
    DEV_LAUNCH(d->stream, k_diff_norm_fwd, dim3(rows), dim3(64 * d->G), 0, n0);
    if (diff_fwd(d, base, w.Y1[b], rows, k.w1, k.b1, k.out, k.out, w.H2[b])) return -1;
    DiffNormP n1 = diff_norm_params(d, base, rows, k.out, w.H2[b], k.n1, d->G);
    if (k.res) { n1.res = w.HR[b].p + k.out; n1.rp = w.HR[b].pitch; }
    else { n1.res = X.p; n1.rp = X.pitch; }
    n1.out = w.OUT[b].p; n1.op = w.OUT[b].pitch;
    DEV_LAUNCH(d->stream, k_diff_norm_fwd, dim3(rows), dim3(64 * d->G), 0, n1);
  }
  const DevMat& last = w.OUT[d->last_block];
  if (diff_fwd(d, base, last, rows, d->f0w, d->f0b, d->start_dim, d->start_dim, w.HF)) return -1;
  DiffNormP nf = diff_norm_params(d, base, rows, d->start_dim, w.HF, d->fn, DIFF_FINAL_GROUPS);
  nf.out = w.YF.p; nf.op = w.YF.pitch;
  DEV_LAUNCH(d->stream, k_diff_norm_fwd, dim3(rows), dim3(64 * DIFF_FINAL_GROUPS), 0, nf);
  return diff_fwd(d, base, w.YF, rows, d->f1w, d->f1b, d->start_dim, d->ad, w.PRED);
}

// the gradient terms of a block's output: one per consumer (a column slice where the consumer read a concatenation)
struct DiffTerms { int n = 0; const float* g[DIFF_MAX_TERMS]; int pitch[DIFF_MAX_TERMS]; };
static int diff_add_term(DiffTerms& t, const DevMat& v) {
  if (t.n >= DIFF_MAX_TERMS) return fail("orl_diffusion: more gradient terms than a block's backward sums");
  t.g[t.n] = v.p; t.pitch[t.n] = v.pitch; ++t.n;
  return 0;
}

// backward from dPRED over the first `rows` rows of the training workspace
static int diff_backward(orl_diffusion* d, DiffWs& w, int rows, const DevMat& x) {
  const float* base = d->params;
  const int sd = d->start_dim, ds = d->dsed;
  const size_t nb = d->blocks.size();
  std::vector<DiffTerms> terms(nb);
  // final_conv
  if (diff_wgrad(d, w.dPRED, w.YF, rows, d->f1w, d->f1b, sd, d->ad) || diff_dgrad(d, w.dPRED, rows, d->f1w, sd, d->ad, w.dYF)) return -1;
  {
    DiffNormP nf = diff_norm_params(d, base, rows, sd, w.HF, d->fn, DIFF_FINAL_GROUPS);
    nf.nterm = 1; nf.g[0] = w.dYF.p; nf.gpitch[0] = w.dYF.pitch;
    nf.dh = w.dHF.p; nf.dhp = w.dHF.pitch;
    nf.part = w.part + d->fn; nf.pn = d->norm_n;
    DEV_LAUNCH(d->stream, k_diff_norm_bwd, dim3(rows), dim3(64 * DIFF_FINAL_GROUPS), 0, nf);
  }
  if (diff_wgrad(d, w.dHF, w.OUT[d->last_block], rows, d->f0w, d->f0b, sd, sd) || diff_dgrad(d, w.dHF, rows, d->f0w, sd, sd, w.dLAST)) return -1;
  if (diff_add_term(terms[d->last_block], w.dLAST)) return -1;
  for (int b = (int)nb - 1; b >= 0; --b) {
    const DiffBlock& k = d->blocks[b];
    const DiffTerms& tm = terms[b];
    if (tm.n == 0) return fail("orl_diffusion: a block without a consumer");
    const DevMat X = k.skip >= 0 ? w.CAT[b] : (k.src < 0 ? x : w.OUT[k.src]);
    const DevMat dRv = k.res ? w.D2[b].cols(k.out) : w.DR[b];
    DiffNormP n1 = diff_norm_params(d, base, rows, k.out, w.H2[b], k.n1, d->G);
    n1.nterm = tm.n;
    for (int i = 0; i < tm.n; ++i) { n1.g[i] = tm.g[i]; n1.gpitch[i] = tm.pitch[i]; }
    n1.dsum = dRv.p; n1.sp = dRv.pitch;
    n1.dh = w.dH2.p; n1.dhp = w.dH2.pitch;
    n1.part = w.part + k.n1; n1.pn = d->norm_n;
    DEV_LAUNCH(d->stream, k_diff_norm_bwd, dim3(rows), dim3(64 * d->G), 0, n1);
    DevMat dH2 = w.dH2; dH2.lim = dH2.pitch;
    if (diff_wgrad(d, dH2, w.Y1[b], rows, k.w1, k.b1, k.out, k.out) || diff_dgrad(d, dH2, rows, k.w1, k.out, k.out, w.dY1)) return -1;
    DiffNormP n0 = diff_norm_params(d, base, rows, k.out, w.HR[b], k.n0, d->G);
    n0.film = w.FILM.p + k.film_col; n0.fp = w.FILM.pitch;
    n0.nterm = 1; n0.g[0] = w.dY1.p; n0.gpitch[0] = w.dY1.pitch;
    n0.dh = w.D2[b].p; n0.dhp = w.D2[b].pitch;
    n0.dfilm = w.dFILM.p + k.film_col; n0.dfp = w.dFILM.pitch;
    n0.part = w.part + k.n0; n0.pn = d->norm_n;
    DEV_LAUNCH(d->stream, k_diff_norm_bwd, dim3(rows), dim3(64 * d->G), 0, n0);
    const int so = k.res ? 2 * k.out : k.out;                 // [dH1 | dR] against [W0; Wr]
    if (diff_wgrad(d, w.D2[b], X, rows, k.w0, k.b0, k.in, so)) return -1;
    if (k.src < 0) continue;                                   // the net's input needs no gradient
    if (diff_dgrad(d, w.D2[b], rows, k.w0, k.in, so, w.DX[b])) return -1;
    const int c1 = d->blocks[k.src].out;
    if (diff_add_term(terms[k.src], w.DX[b])) return -1;
    if (!k.res && diff_add_term(terms[k.src], w.DR[b])) return -1;
    if (k.skip >= 0) {
      if (diff_add_term(terms[k.skip], w.DX[b].cols(c1))) return -1;
      if (!k.res && diff_add_term(terms[k.skip], w.DR[b].cols(c1))) return -1;
    }
  }
  // the FiLM encoders (one GEMM each way), Mish of the condition vector, the step encoder
  if (diff_wgrad(d, w.dFILM, w.MC, rows, d->cw, d->cb, d->cond, d->film_cols) ||
      diff_dgrad(d, w.dFILM, rows, d->cw, d->cond, d->film_cols, w.dMC))
    return -1;
  DEV_LAUNCH(d->stream, k_diff_mish_bwd, dim3(ew_grid((long)rows * ds)), dim3(256), 0, w.dMC.p, w.dMC.pitch, w.GF.p, w.GF.pitch, w.dE.p, w.dE.pitch,
              rows, ds);
  if (diff_wgrad(d, w.dE, w.M1, rows, d->s2w, d->s2b, 4 * ds, ds) || diff_dgrad(d, w.dE, rows, d->s2w, 4 * ds, ds, w.dM1)) return -1;
  DEV_LAUNCH(d->stream, k_diff_mish_bwd, dim3(ew_grid((long)rows * 4 * ds)), dim3(256), 0, w.dM1.p, w.dM1.pitch, w.Z1.p, w.Z1.pitch, w.dZ1.p,
              w.dZ1.pitch, rows, 4 * ds);
  if (diff_wgrad(d, w.dZ1, w.E0, rows, d->s1w, d->s1b, ds, 4 * ds)) return -1;
  DEV_LAUNCH(d->stream, k_diff_colsum, dim3(ew_grid(d->norm_n)), dim3(256), 0, w.part, d->norm_n, rows, d->grads + d->norm_off);
  return 0;
}

// EMAModel(power = 0.75).step after optimizer step k (0-based): decay 0 for the first two steps, then min(1 - (1 + s)^-0.75, 0.9999)
static double diff_ema_decay(long long k) {
  const long long s = std::max(0LL, k - 1);
  if (s <= 0) return 0.0;
  return std::min(1.0 - std::pow(1.0 + (double)s, -0.75), 0.9999);
}

// one optimizer step on the rows idx_d[pos .. pos + rows) (device); t / eps teacher-forced from device arrays or null
static int diff_enqueue_step(orl_diffusion* d, const long long* idx, int rows, const long long* t_in, const float* eps_in, float* loss_dst) {
  if (d->kstep >= d->n_lr) return fail("orl_diffusion: optimizer step " + std::to_string(d->kstep) + " is past the learning-rate table (" +
                                      std::to_string(d->n_lr) + " steps)");
  DiffWs& w = d->tw;
  DiffInputP ip;
  memset(&ip, 0, sizeof(ip));
  ip.rows = rows; ip.od = d->od; ip.ad = d->ad; ip.OP = d->OP; ip.AP = d->AP; ip.dsed = d->dsed; ip.N = d->N;
  ip.idx = idx; ip.d_obs = d->d_obs; ip.d_act = d->d_act; ip.n_data = d->n_data;
  ip.t_in = t_in; ip.eps_in = eps_in; ip.t_const = -1;
  ip.acp = d->acp; ip.seed = d->c.seed; ip.counter = (uint64_t)d->kstep;
  ip.XT = w.XT.p; ip.xp = w.XT.pitch; ip.EPS = d->EPS; ip.TF = d->TF;
  ip.E0 = w.E0.p; ip.ep = w.E0.pitch; ip.GF = w.GF.p; ip.gp = w.GF.pitch;
  DEV_LAUNCH(d->stream, k_diff_input, dim3(rows), dim3(64), 0, ip);
  if (diff_forward(d, w, d->params, rows, w.XT)) return -1;
  DEV_LAUNCH(d->stream, k_mse_loss<false>, dim3(1), dim3(256), 0, (const float*)w.PRED.p, w.PRED.pitch, 0L, (const float*)d->EPS, (const float*)nullptr, 0L,
              (long)rows, d->ad, w.dPRED.p, loss_dst, d->loss_cell);
  if (diff_backward(d, w, rows, w.XT)) return -1;
  const double tt = (double)(d->kstep + 1);
  const double bc1 = 1.0 - std::pow((double)d->c.adam_beta1, tt), bc2 = 1.0 - std::pow((double)d->c.adam_beta2, tt);
  const double decay = diff_ema_decay(d->kstep);
  DEV_LAUNCH(d->stream, k_diff_adam_ema, dim3(ew_grid(d->P)), dim3(256), 0, d->params, d->adam_m, d->adam_v, d->grads, d->ema, d->P, d->lr_tab,
              (long)d->kstep, bc1, (float)std::sqrt(bc2), d->c.adam_beta1, d->c.adam_beta2, d->c.adam_eps, (float)decay, (float)(1.0 - decay));
  d->kstep += 1;
  d->last_rows = rows;
  return 0;
}

static int diff_ready(orl_diffusion* d, const char* what, bool data) {
  if (!d) return fail(std::string(what) + ": null handle");
  if (!d->have_sched) return fail(std::string(what) + ": no schedule (orl_diffusion_set_schedule)");
  if (data && !d->d_obs) return fail(std::string(what) + ": no buffer attached (orl_diffusion_attach_buffer)");
  if (data && !d->lr_tab) return fail(std::string(what) + ": no learning-rate table (orl_diffusion_set_lr)");
  if (hipSetDevice(d->c.device) != hipSuccess) return fail(std::string(what) + ": hipSetDevice failed");
  return 0;
}

// the layout of the parameter block; tensors in state_dict order of the modules that own them
static long diff_layout(orl_diffusion* d) {
  TensorTable& t = d->tensors;
  auto add = [&](const std::string& name, std::initializer_list<long> shape, bool align) { return t.add(name, shape, align, false); };
  const long ds = d->dsed;
  d->s1w = add("diffusion_step_encoder.1.weight", {4 * ds, ds}, true);
  d->s1b = add("diffusion_step_encoder.1.bias", {4 * ds}, true);
  d->s2w = add("diffusion_step_encoder.3.weight", {ds, 4 * ds}, true);
  d->s2b = add("diffusion_step_encoder.3.bias", {ds}, true);
  // the blocks in execution order with their module names
  std::vector<std::string> names;
  std::vector<int> dims(d->c.down_dims, d->c.down_dims + d->nlev);
  d->blocks.clear();
  auto push = [&](const std::string& nm, int in, int out, int src, int skip) {
    DiffBlock k;
    memset(&k, 0, sizeof(k));
    k.in = in; k.out = out; k.res = in != out; k.src = src; k.skip = skip;
    d->blocks.push_back(k);
    names.push_back(nm);
    return (int)d->blocks.size() - 1;
  };
  std::vector<int> level_out;
  int prev = -1, cin = d->ad;
  for (int l = 0; l < d->nlev; ++l) {
    prev = push("down_modules." + std::to_string(l) + ".0", cin, dims[l], prev, -1);
    prev = push("down_modules." + std::to_string(l) + ".1", dims[l], dims[l], prev, -1);
    level_out.push_back(prev);
    cin = dims[l];
  }
  const int mid = dims[d->nlev - 1];
  prev = push("mid_modules.0", mid, mid, prev, -1);
  prev = push("mid_modules.1", mid, mid, prev, -1);
  for (int u = 0; u < d->nlev - 1; ++u) {             // reversed(in_out[1:]): (dim_in, dim_out) = (dims[l - 1], dims[l]), l = nlev-1 .. 1
    const int l = d->nlev - 1 - u;
    const int skip = level_out[l];
    prev = push("up_modules." + std::to_string(u) + ".0", d->blocks[prev].out + dims[l], dims[l - 1], prev, skip);
    prev = push("up_modules." + std::to_string(u) + ".1", dims[l - 1], dims[l - 1], prev, -1);
  }
  d->last_block = prev;
  d->start_dim = dims[0];
  for (size_t b = 0; b < d->blocks.size(); ++b) {
    DiffBlock& k = d->blocks[b];
    const std::string& nm = names[b];
    k.w0 = add(nm + ".blocks.0.block.0.weight", {k.out, k.in}, true);
    if (k.res) add(nm + ".residual_conv.weight", {k.out, k.in}, false);
    k.b0 = add(nm + ".blocks.0.block.0.bias", {k.out}, true);
    if (k.res) add(nm + ".residual_conv.bias", {k.out}, false);
    k.w1 = add(nm + ".blocks.1.block.0.weight", {k.out, k.out}, true);
    k.b1 = add(nm + ".blocks.1.block.0.bias", {k.out}, true);
  }
  d->f0w = add("final_conv.0.block.0.weight", {d->start_dim, d->start_dim}, true);
  d->f0b = add("final_conv.0.block.0.bias", {d->start_dim}, true);
  d->f1w = add("final_conv.1.weight", {d->ad, d->start_dim}, true);
  d->f1b = add("final_conv.1.bias", {d->ad}, true);
  // the FiLM encoders: one [film_cols][cond] matrix and one bias vector
  int col = 0;
  for (size_t b = 0; b < d->blocks.size(); ++b) {
    const long o = add(names[b] + ".cond_encoder.1.weight", {2 * d->blocks[b].out, d->cond}, b == 0);
    if (b == 0) d->cw = o;
    d->blocks[b].film_col = col;
    col += 2 * d->blocks[b].out;
  }
  d->film_cols = col;
  for (size_t b = 0; b < d->blocks.size(); ++b) {
    const long o = add(names[b] + ".cond_encoder.1.bias", {2 * d->blocks[b].out}, b == 0);
    if (b == 0) d->cb = o;
  }
  // the norm region: [gamma | beta] per GroupNorm
  d->norm_off = t.align4();
  for (size_t b = 0; b < d->blocks.size(); ++b) {
    DiffBlock& k = d->blocks[b];
    k.n0 = add(names[b] + ".blocks.0.block.1.weight", {k.out}, false) - d->norm_off;
    add(names[b] + ".blocks.0.block.1.bias", {k.out}, false);
    k.n1 = add(names[b] + ".blocks.1.block.1.weight", {k.out}, false) - d->norm_off;
    add(names[b] + ".blocks.1.block.1.bias", {k.out}, false);
  }
  d->fn = add("final_conv.0.block.1.weight", {d->start_dim}, false) - d->norm_off;
  add("final_conv.0.block.1.bias", {d->start_dim}, false);
  d->norm_n = t.off - d->norm_off;
  return t.align4();
}

extern "C" {

void orl_diffusion_config_default(orl_diffusion_config* c) {
  memset(c, 0, sizeof(*c));
  c->obs_dim = 11; c->act_dim = 3; c->step_embed_dim = 256;
  c->n_levels = 3; c->down_dims[0] = 256; c->down_dims[1] = 512; c->down_dims[2] = 1024;
  c->kernel_size = 5; c->n_groups = 8; c->num_diffusion_iters = 10; c->batch_size = 256;
  c->adam_beta1 = 0.9f; c->adam_beta2 = 0.999f; c->adam_eps = 1e-8f;
  c->n_runs = 1; c->device = 0; c->precision = 0; c->seed = 0;
}

int orl_diffusion_create(const orl_diffusion_config* cfg, orl_diffusion** out) {
  if (!cfg || !out) return fail("orl_diffusion_create: null argument");
  *out = nullptr;
  const orl_diffusion_config& c = *cfg;
  if (c.n_runs != 1) return fail("orl_diffusion_create: one run per object (n_runs > 1 is not supported)");
  if (c.precision != 0) return fail("orl_diffusion_create: precision 0 (fp32 MFMA) only; the split precisions are not supported");
  if (c.kernel_size < 1 || !(c.kernel_size & 1)) return fail("orl_diffusion_create: kernel_size must be odd (the centre tap is the layer)");
  if (c.obs_dim < 1 || c.act_dim < 1 || c.batch_size < 1 || c.num_diffusion_iters < 1) return fail("orl_diffusion_create: bad dims");
  if (c.step_embed_dim < 4 || (c.step_embed_dim & 1)) return fail("orl_diffusion_create: step_embed_dim must be even and >= 4");
  if (c.n_levels < 1 || c.n_levels > ORL_DIFF_MAX_LEVELS) return fail("orl_diffusion_create: n_levels must be in [1, 4]");
  if (c.n_groups < 1 || c.n_groups > 16) return fail("orl_diffusion_create: n_groups must be in [1, 16]");
  for (int l = 0; l < c.n_levels; ++l) {
    if (c.down_dims[l] < 1 || c.down_dims[l] % c.n_groups) return fail("orl_diffusion_create: every channel count must be a multiple of n_groups");
    if (c.down_dims[l] / c.n_groups > 64 * DIFF_NJ) return fail("orl_diffusion_create: a group is wider than 512 channels");
  }
  if (c.down_dims[0] % DIFF_FINAL_GROUPS || c.down_dims[0] / DIFF_FINAL_GROUPS > 64 * DIFF_NJ)
    return fail("orl_diffusion_create: down_dims[0] must be a multiple of 8 (final_conv's norm is GroupNorm(8) whatever n_groups is)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("orl_diffusion_create: no HIP device (MI355X) visible");
  if (c.device < 0 || c.device >= ndev) return fail("orl_diffusion_create: device ordinal out of range");
  if (hipSetDevice(c.device) != hipSuccess) return fail("orl_diffusion_create: hipSetDevice failed");
  orl_diffusion* d = new orl_diffusion();
  d->c = c;
  d->od = c.obs_dim; d->ad = c.act_dim; d->dsed = c.step_embed_dim; d->cond = d->dsed + d->od; d->N = c.num_diffusion_iters;
  d->B = c.batch_size; d->G = c.n_groups; d->nlev = c.n_levels;
  d->P = diff_layout(d);
  bool bad = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess;
  bad = bad || d->mem.alloc(&d->params, d->P) || d->mem.alloc(&d->ema, d->P) || d->mem.alloc(&d->adam_m, d->P) ||
        d->mem.alloc(&d->adam_v, d->P) || d->mem.alloc(&d->grads, d->P) || d->mem.alloc(&d->acp, d->N) ||
        d->mem.alloc(&d->coef, 5 * (size_t)d->N) || diff_ws_alloc(d, d->tw, d->B, true) || d->mem.alloc(&d->t_d, d->B) ||
        d->mem.alloc(&d->eps_in, (size_t)d->B * d->ad) || d->mem.alloc(&d->EPS, (size_t)d->B * d->ad) || d->mem.alloc(&d->TF, d->B) ||
        d->mem.alloc(&d->loss_cell, 1);
  if (bad) {
    const std::string msg = orl_last_error();
    orl_diffusion_destroy(d);
    return fail(msg.empty() ? "orl_diffusion_create: allocation failed" : msg);
  }
  *out = d;
  return 0;
}

void orl_diffusion_destroy(orl_diffusion* d) {
  if (!d) return;
  if (d->stream) hipStreamSynchronize(d->stream);
  d->mem.free_all();
  if (d->stream) hipStreamDestroy(d->stream);
  delete d;
}

int64_t orl_diffusion_floats(orl_diffusion* d) { return d ? d->P : -1; }
int orl_diffusion_num_tensors(orl_diffusion* d) { return d ? (int)d->tensors.size() : -1; }
int orl_diffusion_tensor(orl_diffusion* d, int idx, char* name, int name_cap, int64_t* offset, int32_t* ndim, int64_t shape[4]) {
  if (!d || d->tensors.query(idx, name, name_cap, offset, ndim, shape)) return fail("orl_diffusion_tensor: index out of range");
  return 0;
}

static float* diff_block_of(orl_diffusion* d, int which) {
  return which == 0 ? d->params : which == 1 ? d->ema : which == 2 ? d->adam_m : which == 3 ? d->adam_v : nullptr;
}
int orl_diffusion_set(orl_diffusion* d, int which, const float* host, int64_t n) {
  if (!d || !host || !diff_block_of(d, which)) return fail("orl_diffusion_set: bad arguments");
  if (n != d->P) return fail("orl_diffusion_set: expected " + std::to_string(d->P) + " floats");
  return block_from_host(d->stream, diff_block_of(d, which), host, d->P);
}
int orl_diffusion_get(orl_diffusion* d, int which, float* host, int64_t n) {
  if (!d || !host || !diff_block_of(d, which)) return fail("orl_diffusion_get: bad arguments");
  if (n != d->P) return fail("orl_diffusion_get: expected " + std::to_string(d->P) + " floats");
  return block_to_host(d->stream, host, diff_block_of(d, which), d->P);
}
int orl_diffusion_set_step_count(orl_diffusion* d, int64_t k) {
  if (!d || k < 0) return fail("orl_diffusion_set_step_count: bad arguments");
  d->kstep = k;
  return 0;
}
int64_t orl_diffusion_step_count(orl_diffusion* d) { return d ? d->kstep : -1; }

int orl_diffusion_set_schedule(orl_diffusion* d, const float* acp, const float* coef) {
  if (!d || !acp || !coef) return fail("orl_diffusion_set_schedule: bad arguments");
  for (int i = 0; i < d->N; ++i)
    if (!(acp[i] > 0.f && acp[i] < 1.f) || !(coef[5 * i] > 0.f)) return fail("orl_diffusion_set_schedule: alphas_cumprod must lie in (0, 1)");
  ORL_HIP(hipStreamSynchronize(d->stream));
  ORL_HIP(hipMemcpy(d->acp, acp, sizeof(float) * d->N, hipMemcpyHostToDevice));
  ORL_HIP(hipMemcpy(d->coef, coef, sizeof(float) * 5 * d->N, hipMemcpyHostToDevice));
  d->have_sched = true;
  return 0;
}
int orl_diffusion_set_lr(orl_diffusion* d, const double* table, int64_t n) {
  if (!d || !table || n < 1) return fail("orl_diffusion_set_lr: bad arguments");
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->mem.release(&d->lr_tab); d->n_lr = 0;
  if (d->mem.alloc(&d->lr_tab, (size_t)n)) return -1;
  ORL_HIP(hipMemcpy(d->lr_tab, table, sizeof(double) * n, hipMemcpyHostToDevice));
  d->n_lr = n;
  return 0;
}
int orl_diffusion_attach_buffer(orl_diffusion* d, orl_buffer* b) {
  if (!d || !b) return fail("orl_diffusion_attach_buffer: bad arguments");
  int dev, od, ad, OP, AP; long n; const float *obs, *act;
  buffer_view(b, &dev, &od, &ad, &OP, &AP, &n, &obs, &act);
  if (dev != d->c.device || od != d->od || ad != d->ad) return fail("orl_diffusion_attach_buffer: the buffer's device or dims differ");
  if (n < 1 || !obs || !act) return fail("orl_diffusion_attach_buffer: the buffer is empty");
  ORL_HIP(hipDeviceSynchronize());
  d->d_obs = obs; d->d_act = act; d->OP = OP; d->AP = AP; d->n_data = n;
  return 0;
}

int orl_diffusion_step(orl_diffusion* d, const int64_t* idx, int32_t rows, const int64_t* t, const float* eps, float* loss_out) {
  if (diff_ready(d, "orl_diffusion_step", true)) return -1;
  if (!idx || rows < 1 || rows > d->B) return fail("orl_diffusion_step: need 1 <= rows <= batch_size row indices");
  for (int i = 0; i < rows; ++i) {
    if (idx[i] < 0 || idx[i] >= d->n_data) return fail("orl_diffusion_step: row index out of range");
    if (t && (t[i] < 0 || t[i] >= d->N)) return fail("orl_diffusion_step: t out of range");
  }
  if (d->mem.grow(&d->idx_d, &d->idx_cap, d->B, d->stream)) return -1;
  ORL_HIP(hipMemcpyAsync(d->idx_d, idx, sizeof(int64_t) * rows, hipMemcpyHostToDevice, d->stream));
  if (t) ORL_HIP(hipMemcpyAsync(d->t_d, t, sizeof(int64_t) * rows, hipMemcpyHostToDevice, d->stream));
  if (eps) ORL_HIP(hipMemcpyAsync(d->eps_in, eps, sizeof(float) * rows * d->ad, hipMemcpyHostToDevice, d->stream));
  if (diff_enqueue_step(d, d->idx_d, rows, t ? d->t_d : nullptr, eps ? d->eps_in : nullptr, d->loss_cell)) return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  if (loss_out) ORL_HIP(hipMemcpy(loss_out, d->loss_cell, sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int orl_diffusion_learn_epoch(orl_diffusion* d, const int64_t* order, int64_t n_rows, int on_device, float* losses_out) {
  if (diff_ready(d, "orl_diffusion_learn_epoch", true)) return -1;
  // (the epoch must stay inside the learning-rate table: refused before anything is queued)
  if (order && n_rows >= 1 && d->kstep + (n_rows + d->B - 1) / d->B > d->n_lr)
    return fail("orl_diffusion_learn_epoch: the epoch runs past the learning-rate table");
  return learn_epoch_steps(d->stream, d->mem, &d->idx_d, &d->idx_cap, &d->loss_steps, &d->loss_cap, d->B, d->n_data, 1, "orl_diffusion_learn_epoch",
                           order, n_rows, on_device, losses_out, [d](const long long* idx, int rows, float* loss_dst) {
                             return diff_enqueue_step(d, idx, rows, nullptr, nullptr, loss_dst);
                           });
}

int orl_diffusion_sample(orl_diffusion* d, const float* obs, int64_t n, const float* init_noise, const int64_t* noise_idx, int64_t noise_rows,
                         const float* z, int on_device, float* act_out) {
  if (diff_ready(d, "orl_diffusion_sample", false)) return -1;
  if (!obs || !init_noise || !act_out || n < 1 || n > 0x7fffffffLL / (4 * d->film_cols + 16)) return fail("orl_diffusion_sample: bad arguments");
  if (!noise_idx) noise_rows = n;
  if (noise_rows < 1) return fail("orl_diffusion_sample: noise_rows must be positive");
  if (noise_idx && !on_device)
    for (int64_t i = 0; i < n; ++i)
      if (noise_idx[i] < 0 || noise_idx[i] >= noise_rows) return fail("orl_diffusion_sample: noise index out of range");
  const int ad = d->ad, od = d->od, N = d->N;
  if (n > d->s_cap || (!on_device && noise_rows > d->s_noise_cap)) {
    ORL_HIP(hipStreamSynchronize(d->stream));
    const long cap = std::max<long>(n, d->s_cap), ncap = std::max<long>(noise_rows, d->s_noise_cap);
    d->mem.release(&d->sObs, &d->sX, &d->sNoise, &d->sZ, &d->sZkeep, &d->sOut, &d->sIdx);
    if (d->mem.alloc(&d->sObs, (size_t)cap * od) || d->mem.alloc(&d->sX, (size_t)cap * rup4(ad)) ||
        d->mem.alloc(&d->sNoise, (size_t)ncap * ad) || d->mem.alloc(&d->sZ, (size_t)N * cap * ad) ||
        d->mem.alloc(&d->sZkeep, (size_t)cap * ad) || d->mem.alloc(&d->sOut, (size_t)cap * ad) || d->mem.alloc(&d->sIdx, (size_t)cap))
      return -1;
    if (cap > d->sw.cap && diff_ws_alloc(d, d->sw, cap, false)) return -1;
    d->s_cap = cap; d->s_noise_cap = ncap;
  }
  const float* obs_d = obs; const float* noise_d = init_noise; const float* z_d = z; const long long* nidx_d = (const long long*)noise_idx;
  if (stage_in(d->stream, obs_d, d->sObs, (size_t)n * od, on_device) || stage_in(d->stream, noise_d, d->sNoise, (size_t)noise_rows * ad, on_device) ||
      stage_in(d->stream, z_d, d->sZ, (size_t)N * n * ad, on_device) || stage_in(d->stream, nidx_d, d->sIdx, (size_t)n, on_device))
    return -1;
  DiffWs& w = d->sw;
  DevMat X; X.p = d->sX; X.pitch = X.lim = rup4(ad);
  DEV_LAUNCH(d->stream, k_diff_copy, dim3(ew_grid(n * ad)), dim3(256), 0, noise_d, ad, nidx_d, (long)noise_rows, X.p, X.pitch, (long)n, ad);
  for (int t = N - 1; t >= 0; --t) {
    DiffInputP ip;
    memset(&ip, 0, sizeof(ip));
    ip.rows = (int)n; ip.od = od; ip.ad = ad; ip.dsed = d->dsed; ip.N = N;
    ip.s_obs = obs_d; ip.t_const = t;
    ip.E0 = w.E0.p; ip.ep = w.E0.pitch; ip.GF = w.GF.p; ip.gp = w.GF.pitch;
    DEV_LAUNCH(d->stream, k_diff_input, dim3((unsigned)n), dim3(64), 0, ip);
    if (diff_forward(d, w, d->ema, (int)n, X)) return -1;
    DEV_LAUNCH(d->stream, k_diff_ddpm, dim3(ew_grid(n * ad)), dim3(256), 0, X.p, X.pitch, w.PRED.p, w.PRED.pitch, d->coef, t,
                z_d ? z_d + (long)t * n * ad : (const float*)nullptr, d->sZkeep, (long)n, ad, d->c.seed, d->sample_calls * (uint64_t)N + (uint64_t)t);
  }
  float* dst = stage_dst(act_out, d->sOut, on_device);
  DEV_LAUNCH(d->stream, k_diff_copy, dim3(ew_grid(n * ad)), dim3(256), 0, X.p, X.pitch, (const long long*)nullptr, 0L, dst, ad, (long)n, ad);
  if (stage_out(d->stream, act_out, d->sOut, (size_t)n * ad, on_device)) return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->sample_calls += 1;
  d->last_sample_n = n;
  return 0;
}

int64_t orl_diffusion_debug_read(orl_diffusion* d, const char* name, float* host, int64_t cap) {
  if (!d || !name || !host) return fail("orl_diffusion_debug_read: bad arguments");
  const std::string nm(name);
  const float* src = nullptr; long rows = d->last_rows; int cols = 0, pitch = 0;
  const DiffWs& w = d->tw;
  if (nm == "pred") { src = w.PRED.p; cols = d->ad; pitch = w.PRED.pitch; }
  else if (nm == "x_t") { src = w.XT.p; cols = d->ad; pitch = w.XT.pitch; }
  else if (nm == "eps") { src = d->EPS; cols = d->ad; pitch = d->ad; }
  else if (nm == "t") { src = d->TF; cols = 1; pitch = 1; }
  else if (nm == "gf") { src = w.GF.p; cols = d->cond; pitch = w.GF.pitch; }
  else if (nm == "film") { src = w.FILM.p; cols = d->film_cols; pitch = w.FILM.pitch; }
  else if (nm == "e0") { src = w.E0.p; cols = d->dsed; pitch = w.E0.pitch; }
  else if (nm == "mc") { src = w.MC.p; cols = d->cond; pitch = w.MC.pitch; }
  else if (nm == "yf") { src = w.YF.p; cols = d->start_dim; pitch = w.YF.pitch; }
  else if (nm.compare(0, 3, "y1.") == 0 || nm.compare(0, 4, "out.") == 0) {      // "y1.<b>" / "out.<b>": block b of the layer table
    const bool y1 = nm[0] == 'y';
    const std::string num = nm.substr(y1 ? 3 : 4);
    if (num.empty() || num.size() > 4 || num.find_first_not_of("0123456789") != std::string::npos || (num.size() > 1 && num[0] == '0'))
      return fail("orl_diffusion_debug_read: unknown tap " + nm);
    const size_t b = (size_t)std::stoi(num);
    if (b >= d->blocks.size()) return fail("orl_diffusion_debug_read: unknown tap " + nm + " (the net has " + std::to_string(d->blocks.size()) + " blocks)");
    const DevMat& m = y1 ? w.Y1[b] : w.OUT[b];
    src = m.p; cols = d->blocks[b].out; pitch = m.pitch;
  }
  else if (nm == "loss") { src = d->loss_cell; rows = 1; cols = 1; pitch = 1; }
  else if (nm == "z") { src = d->sZkeep; rows = d->last_sample_n; cols = d->ad; pitch = d->ad; }
  else if (nm == "x") { src = d->sX; rows = d->last_sample_n; cols = d->ad; pitch = rup4(d->ad); }
  else return fail("orl_diffusion_debug_read: unknown tap " + nm);
  if (!src || rows < 1) return fail("orl_diffusion_debug_read: nothing recorded for " + nm);
  if ((int64_t)rows * cols > cap) return fail("orl_diffusion_debug_read: " + nm + " needs " + std::to_string(rows * cols) + " floats");
  ORL_HIP(hipStreamSynchronize(d->stream));
  ORL_HIP(hipMemcpy2D(host, sizeof(float) * cols, src, sizeof(float) * pitch, sizeof(float) * cols, rows, hipMemcpyDeviceToHost));
  return (int64_t)rows * cols;
}
int orl_diffusion_debug_grads(orl_diffusion* d, float* host, int64_t n) {
  if (!d || !host || n != d->P) return fail("orl_diffusion_debug_grads: bad arguments");
  return block_to_host(d->stream, host, d->grads, d->P);
}

}  // extern "C"
