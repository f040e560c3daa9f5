// rnn_dynamics.hip — RNNDynamics on the device (reference: dynamics/rnn_dynamics.py, nets/rnn.py:RNNModel): orl_rnn_* of
// include/orl_engine.h.
//
// Every sequence array is a [rows * T][cols] matrix, row b * T + t (batch_first).  One training step is a run of launches on one stream:
//   k_rnn_gather       the step's sequences, targets and loss masks out of the HBM data set
//   per GRU layer      ONE tiled GEMM for the input projections of all T steps (E_BIAS), then ONE launch of k_rnn_scan_fwd: a
//                      workgroup owns 16 batch rows and all H hidden units of them for all T steps, keeps h_{t-1} in LDS, multiplies it
//                      by W_hh on the fp32 MFMA and applies the gates in the same step's epilogue.  Batch rows are independent, so no
//                      workgroup ever waits for another one: __syncthreads() only, and the bounded loop over t.
//   the tail           tiled GEMMs (E_BIAS_SWISH keeps the pre-activation) with k_rnn_ln_fwd between them: dropout, residual, LayerNorm
//   k_mse_loss<true>   the masked MSE and its gradient, one block per run, fixed order (train_ops.h)
//   the backward       the tail top down (k_rnn_ln_bwd folds the dropout mask and Swish' in), then per GRU layer ONE launch of
//                      k_rnn_scan_bwd (t = T-1 .. 0, same ownership; carries dh_{t-1} = dh_t z + dGH_t W_hh in LDS) and three tiled
//                      GEMMs over all rows: dW_hh / db_hh from dGH and the shifted h, dW_ih / db_ih, and the dX of the layer below
//   k_rnn_colsum_*     dgamma / dbeta: per-row terms summed in row order in two levels (64-row chunks, then the chunks)
//   k_rnn_slab_sum     the weight gradients are split-K products into up to 8 slabs (k ranges of >= 256 rows): the slabs added in order
//   k_rnn_adam         torch.optim.Adam over the flat block
// Nothing accumulates with atomics: two identical calls give identical bits.
//
// Runs (orl_rnn_config::n_runs = R): every launch above gets a run dimension and nothing else.  Parameters, moments, gradients and
// slabs are [R][P] per block, every workspace matrix is [R][cap rows][pitch], the data set is one and each run gathers its own rows.
// The scans and the row kernels add blockIdx.y * stride to their base pointers, the matrix products take the runs as launch_gemm's
// batch.  Tile configurations and slab counts are functions of the per-run shape, so run r's bits do not depend on R.
//
// Rollouts (orl_rnn_state_*): the h of every GRU layer of n_traj trajectories stays in HBM, and one model step of n rows is
//   k_rnn_roll_in      x = ([obs | act] - mu) / std
//   per GRU layer      ONE launch of k_rnn_cell: gathers h_prev of each row's trajectory, W_ih x and W_hh h on the fp32 MFMA, the gates,
//                      the new h to the trajectory's slot and to the layer's output rows; a workgroup owns 16 rows x 16 units
//   the tail           the window forward's own (rnn_tail), on n rows
//   k_rnn_roll_head    next_obs = pred[:, :-1] + obs, reward = pred[:, -1]
// O(1) per model step at any horizon; no atomics here either.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "devobj.h"
#include "reduce.h"
#include "rng.h"
#include "train_ops.h"

namespace orl {

enum { RNN_RB = 16 };                 // batch rows of a scan workgroup: one MFMA tile
enum { RNN_FWD_WAVES = 8, RNN_BWD_WAVES = 4 };
// 16-deep k blocks whose weight loads a scan wave issues together.  Measured at the default shape (3 layers, 256 x 20): the backward scans
// 1.85 -> 1.49 ms with 4; the forward scans, two waves per SIMD already, 1.15 -> 1.37 ms with 4, so they keep 1
enum { RNN_KU_FWD = 1, RNN_KU_BWD = 4 };
enum { RNN_MAX_H = 512, RNN_MAX_LAYERS = 4, RNN_MAX_NORMS = ORL_MAX_HIDDEN + 1 };
enum { RNN_NJ = RNN_MAX_H / 64 };     // LayerNorm: values of a row per lane
enum { RNN_CHUNK = 64 };              // rows of a first-level column sum

__device__ __forceinline__ float rnn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
// Swish'(z) = sigmoid(z) (1 + z (1 - sigmoid(z))) on the library exp and a true division
__device__ __forceinline__ float rnn_dswish(float z) { const float s = rnn_sigmoid(z); return s * (1.f + z * (1.f - s)); }

// ---- the GRU recurrence of one layer over all T steps ----
struct RnnScanP {
  int rows, T, H;
  const float* gi; int gip;          // [rows * T][3H]: W_ih x + b_ih, gates r | z | n
  const float* whh;                  // [3H][H]
  const float* bhh;                  // [3H]
  float* ho; int hop;                // [rows * T][H]: h_t
  float *r, *z, *n, *hn, *hp; int sp;   // training: the gates, W_hn h + b_hn and h_{t-1} ([rows * T][H] each); eval: null
  long gi_rs, par_rs, ho_rs, s_rs;   // run strides (floats) of gi, of whh / bhh, of ho and of the saved matrices: run = blockIdx.y
};

// LDS: h_{t-1} of the block's 16 rows as [16][HP], HP = 16 ceil(H / 16) + 4, columns past H zero.  Wave w owns the unit tiles
// w, w + 8, ...: 16 hidden units each, the r, z and n accumulators of a unit side by side in the same lane.  Lane (i = l & 15, q = l >> 4)
// reads four consecutive k of h row i (one ds_read_b128) and of the W_hh rows of its unit (three global dwordx4 along k): MFMA s of a
// 16-deep k block carries logical k = 16 kb + 4 q + s in hardware slot q on both operands.
__global__ __launch_bounds__(64 * RNN_FWD_WAVES) void k_rnn_scan_fwd(RnnScanP p) {
  extern __shared__ __attribute__((aligned(16))) float rnn_lds[];
  const int H = p.H, KB = (H + 15) >> 4, HP = KB * 16 + 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const int b0 = blockIdx.x * RNN_RB;
  const int nrow = min((int)RNN_RB, p.rows - b0);
  {                                                     // this workgroup's run: its operands, weights and outputs
    const long run = blockIdx.y;
    p.gi += run * p.gi_rs; p.whh += run * p.par_rs; p.bhh += run * p.par_rs; p.ho += run * p.ho_rs;
    if (p.r) { p.r += run * p.s_rs; p.z += run * p.s_rs; p.n += run * p.s_rs; p.hn += run * p.s_rs; p.hp += run * p.s_rs; }
  }
  for (int e = tid; e < RNN_RB * HP; e += 64 * RNN_FWD_WAVES) rnn_lds[e] = 0.f;
  __syncthreads();
  for (int t = 0; t < p.T; ++t) {
    float hnew[4][4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
#pragma unroll
      for (int r = 0; r < 4; ++r) hnew[it][r] = 0.f;
      const int tile = wave + RNN_FWD_WAVES * it;
      if (tile < KB) {                                  // (unit tiles = ceil(H / 16) = KB; wave-uniform)
        const int j = tile * 16 + li;
        const int jc = min(j, H - 1);                   // a clamped row is read and its result dropped
        const float* wr = p.whh + (long)jc * H;
        const float* wz = p.whh + (long)(H + jc) * H;
        const float* wn = p.whh + (long)(2 * H + jc) * H;
        f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, an = ar;
        // the step's input projections of this lane's four (row, unit) pairs, asked for before the k loop so that they arrive under it
        float gr[4], gz[4], gn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int b = min(4 * lq + r, nrow - 1);
          const float* g = p.gi + ((long)(b0 + b) * p.T + t) * p.gip;
          gr[r] = g[jc]; gz[r] = g[H + jc]; gn[r] = g[2 * H + jc];
        }
        // RNN_KU_FWD k blocks at a time (the enum says why it is 1 here): with more, their weight loads are in flight together before the
        // first MFMA waits for one; a k block past the end multiplies zeros
        for (int kb0 = 0; kb0 < KB; kb0 += RNN_KU_FWD) {
          f32x4 a[RNN_KU_FWD], vr[RNN_KU_FWD], vz[RNN_KU_FWD], vn[RNN_KU_FWD];
#pragma unroll
          for (int u = 0; u < RNN_KU_FWD; ++u) {
            const int k4 = (kb0 + u) * 16 + 4 * lq;
            a[u] = vr[u] = vz[u] = vn[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k4 < H) {                               // (H is a multiple of 4: a quad is inside or outside)
              vr[u] = *(const f32x4*)(wr + k4);
              vz[u] = *(const f32x4*)(wz + k4);
              vn[u] = *(const f32x4*)(wn + k4);
            }
            if (kb0 + u < KB) a[u] = *(const f32x4*)&rnn_lds[li * HP + k4];
          }
#pragma unroll
          for (int u = 0; u < RNN_KU_FWD; ++u) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][s], vr[u][s], ar, 0, 0, 0);      // D[batch row 4 q + r][unit i]
              az = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][s], vz[u][s], az, 0, 0, 0);
              an = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][s], vn[u][s], an, 0, 0, 0);
            }
          }
        }
        if (j < H) {
          const float br = p.bhh[j], bz = p.bhh[H + j], bn = p.bhh[2 * H + j];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int b = 4 * lq + r;
            if (b < nrow) {
              const long row = (long)(b0 + b) * p.T + t;
              const float hn = an[r] + bn;
              const float rg = rnn_sigmoid(gr[r] + (ar[r] + br));
              const float zg = rnn_sigmoid(gz[r] + (az[r] + bz));
              const float ng = tanhf(gn[r] + rg * hn);
              const float hprev = rnn_lds[b * HP + j];
              const float hv = (1.f - zg) * ng + zg * hprev;
              p.ho[row * p.hop + j] = hv;
              if (p.r) {
                const long o = row * p.sp + j;
                p.r[o] = rg; p.z[o] = zg; p.n[o] = ng; p.hn[o] = hn; p.hp[o] = hprev;
              }
              hnew[it][r] = hv;
            }
          }
        }
      }
    }
    __syncthreads();                                    // every wave has read h_{t-1}
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int j = (wave + RNN_FWD_WAVES * it) * 16 + li;
      if (j < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) rnn_lds[(4 * lq + r) * HP + j] = hnew[it][r];
      }
    }
    __syncthreads();
  }
}

struct RnnScanBP {
  int rows, T, H;
  const float* dout; int dop;        // [rows * T][H]: the gradient of h_t from the layer above
  const float* whh;
  const float *r, *z, *n, *hn, *hp; int sp;
  float* dgi; float* dgh; int gp;    // [rows * T][3H]: gradients of the input-side and hidden-side pre-activations
  long do_rs, par_rs, s_rs, g_rs;    // run strides (floats) of dout, of whh, of the saved matrices and of dgi / dgh: run = blockIdx.y
};

// LDS: dGH_t of the block's 16 rows as [16][GP], GP = 16 ceil(3H / 16) + 4 (columns past 3H zero), and the carried dh as [16][H + 4].
// Per step every thread first does the gate backward of its elements (dh_t = dout_t + carry; carry <- dh_t z), then the waves add
// dGH_t W_hh to the carry.  W_hh's rows run along the OUTPUT units here, so a wave owns 64 units: lane i loads units 4 i .. 4 i + 3 of
// row k with one dwordx4 and element e feeds accumulator e, whose column i is unit 64 g + 4 i + e.
__global__ __launch_bounds__(64 * RNN_BWD_WAVES) void k_rnn_scan_bwd(RnnScanBP p) {
  extern __shared__ __attribute__((aligned(16))) float rnn_lds[];
  const int H = p.H, K3 = 3 * H, KB = (K3 + 15) >> 4, GP = KB * 16 + 4, CP = H + 4;
  float* dg = rnn_lds;
  float* carry = rnn_lds + RNN_RB * GP;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const int b0 = blockIdx.x * RNN_RB;
  const int nrow = min((int)RNN_RB, p.rows - b0);
  {
    const long run = blockIdx.y;
    p.dout += run * p.do_rs; p.whh += run * p.par_rs;
    p.r += run * p.s_rs; p.z += run * p.s_rs; p.n += run * p.s_rs; p.hn += run * p.s_rs; p.hp += run * p.s_rs;
    p.dgi += run * p.g_rs; p.dgh += run * p.g_rs;
  }
  for (int e = tid; e < RNN_RB * (GP + CP); e += 64 * RNN_BWD_WAVES) rnn_lds[e] = 0.f;
  __syncthreads();
  for (int t = p.T - 1; t >= 0; --t) {
    // (read-only views: the loads of several elements may be issued before the first store)
    const float* __restrict__ s_r = p.r; const float* __restrict__ s_z = p.z; const float* __restrict__ s_n = p.n;
    const float* __restrict__ s_hn = p.hn; const float* __restrict__ s_hp = p.hp; const float* __restrict__ s_do = p.dout;
#pragma unroll 4
    for (int e = tid; e < RNN_RB * H; e += 64 * RNN_BWD_WAVES) {
      const int b = e / H, j = e - b * H;
      float gr = 0.f, gz = 0.f, gn = 0.f, gnr = 0.f, cz = 0.f;
      if (b < nrow) {
        const long row = (long)(b0 + b) * p.T + t;
        const long o = row * p.sp + j;
        const float dh = s_do[row * p.dop + j] + carry[b * CP + j];
        const float rg = s_r[o], zg = s_z[o], ng = s_n[o], hn = s_hn[o], hprev = s_hp[o];
        gn = dh * (1.f - zg) * (1.f - ng * ng);
        gz = dh * (hprev - ng) * zg * (1.f - zg);
        gr = gn * hn * rg * (1.f - rg);
        gnr = gn * rg;
        cz = dh * zg;
        float* gi = p.dgi + row * p.gp;
        float* gh = p.dgh + row * p.gp;
        gi[j] = gr; gi[H + j] = gz; gi[2 * H + j] = gn;
        gh[j] = gr; gh[H + j] = gz; gh[2 * H + j] = gnr;
      }
      dg[b * GP + j] = gr; dg[b * GP + H + j] = gz; dg[b * GP + 2 * H + j] = gnr;
      carry[b * CP + j] = cz;
    }
    __syncthreads();
    if (t > 0) {                                        // (dh_{-1} has no consumer)
      for (int grp = wave; grp * 64 < H; grp += RNN_BWD_WAVES) {
        const int jl = grp * 64 + 4 * li;
        f32x4 acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kb0 = 0; kb0 < KB; kb0 += RNN_KU_BWD) {      // (RNN_KU_BWD k blocks of loads in flight together, as in the forward)
          f32x4 a[RNN_KU_BWD], w[RNN_KU_BWD][4];
#pragma unroll
          for (int u = 0; u < RNN_KU_BWD; ++u) {
            const int k4 = (kb0 + u) * 16 + 4 * lq;
            a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              w[u][s] = f32x4{0.f, 0.f, 0.f, 0.f};
              if (k4 < K3 && jl < H) w[u][s] = *(const f32x4*)(p.whh + (long)(k4 + s) * H + jl);   // (3H and H are multiples of 4)
            }
            if (kb0 + u < KB) a[u] = *(const f32x4*)&dg[li * GP + k4];
          }
#pragma unroll
          for (int u = 0; u < RNN_KU_BWD; ++u) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][s], w[u][s][e], acc[e], 0, 0, 0);
            }
          }
        }
        if (jl < H) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int r = 0; r < 4; ++r) carry[(4 * lq + r) * CP + jl + e] += acc[e][r];
          }
        }
      }
    }
    __syncthreads();
  }
}

// ---- the small kernels of the tail ----
// the step's sequences out of the data set: X0 [rows * T][xp], TGT [rows * T][od], MSK [rows * T]; a row index is clamped.  Run
// blockIdx.y reads its own index list (stride idx_rs) and writes its own X0 / TGT / MSK (strides x_rs, tm_rs * od, tm_rs)
__global__ void k_rnn_gather(const float* __restrict__ inputs, const float* __restrict__ targets, const float* __restrict__ masks,
                             const long long* __restrict__ idx, long idx_rs, long n_data, int T, int in, int od, int rows, float* __restrict__ X0,
                             int xp, long x_rs, float* __restrict__ TGT, float* __restrict__ MSK, long tm_rs) {
  const int per = in + od + 1;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)rows * T * per) return;
  const long run = blockIdx.y;
  idx += run * idx_rs; X0 += run * x_rs; TGT += run * tm_rs * od; MSK += run * tm_rs;
  const long row = e / per; const int c = (int)(e - row * per);
  const long b = row / T; const int t = (int)(row - b * T);
  const long g = min(max((long)idx[b], 0L), n_data - 1) * T + t;
  if (c < in) X0[row * xp + c] = inputs[g * in + c];
  else if (c < in + od) TGT[row * od + (c - in)] = targets[g * od + (c - in)];
  else MSK[row] = masks[g];
}
// dst [rows][cols] (pitch dp) = src (pitch sp); step > 1: source row = r * step + (step - 1), the last time step of sequence r.
// Run blockIdx.y: src + run * s_rs, dst + run * d_rs  (not merged with k_diff_copy: that one gathers through a row index)
__global__ void k_rnn_copy(const float* __restrict__ src, int sp, long s_rs, float* __restrict__ dst, int dp, long d_rs, long rows, int cols,
                           int step) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * cols) return;
  src += (long)blockIdx.y * s_rs; dst += (long)blockIdx.y * d_rs;
  const long r = e / cols; const int c = (int)(e - r * cols);
  dst[r * dp + c] = src[(r * step + (step - 1)) * sp + c];
}
// keep masks 1[u < 1 - p] of dropout `slot`: Philox keyed by the seed, counter = (step count, slot), (row, column quad).  Run
// blockIdx.y (masks at mk + run * mk_rs) draws the stream of a one-run object with seed + run
__global__ void k_rnn_mask(float* __restrict__ mk, long mk_rs, long rows, int H, float keep, uint64_t seed, uint64_t kstep, uint32_t slot) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int q4 = H >> 2;
  if (e >= rows * q4) return;
  const long row = e / q4; const int q = (int)(e - row * q4);
  mk += (long)blockIdx.y * mk_rs;
  uint32_t rnd[4];
  const Philox ph(seed + (uint64_t)blockIdx.y);
  ph((uint32_t)row, (uint32_t)q, (uint32_t)kstep, (slot << 28) | (uint32_t)((kstep >> 32) & 0x0fffffffu), rnd);
#pragma unroll
  for (int k = 0; k < 4; ++k) mk[row * H + 4 * q + k] = u01(rnd[k]) < keep ? 1.f : 0.f;
}

struct RnnNormP {
  int rows, H;
  const float* s; int sp;            // swish(Linear(x))
  const float* mask; float scale;    // keep mask [rows][H] and 1 / (1 - p), or null
  const float* res; int rp;          // the residual input or null
  const float* gamma; const float* beta;
  float* u; int up;                  // what the LayerNorm reads: res + dropout(s)
  float* out; int op;
  // backward
  int nterm; const float* g[2]; int gpitch[2];    // dOut = the sum of the terms
  const float* zpre; int zp;         // the Linear's output (Swish' argument)
  float* du; int dup;                // the residual path's gradient or null
  float* dz; int dzp;                // the Linear's output gradient
  float* part; long pn;              // [row][pn]: dgamma at [c], dbeta at [H + c]
  // run strides (floats): run = blockIdx.y
  long s_rs, mask_rs, res_rs, par_rs, u_rs, out_rs, g_rs[2], z_rs, du_rs, dz_rs, part_rs;
};
// the views of run `run`
__device__ __forceinline__ void rnn_norm_run(RnnNormP& p, long run) {
  p.s += run * p.s_rs; p.gamma += run * p.par_rs; p.beta += run * p.par_rs; p.u += run * p.u_rs;
  if (p.mask) p.mask += run * p.mask_rs;
  if (p.res) p.res += run * p.res_rs;
  if (p.out) p.out += run * p.out_rs;
  if (p.g[0]) p.g[0] += run * p.g_rs[0];
  if (p.g[1]) p.g[1] += run * p.g_rs[1];
  if (p.zpre) p.zpre += run * p.z_rs;
  if (p.du) p.du += run * p.du_rs;
  if (p.dz) p.dz += run * p.dz_rs;
  if (p.part) p.part += run * p.part_rs;
}

// u = res + mask s / (1 - p); out = LayerNorm(u) (eps 1e-5, affine); one wave per row
__global__ __launch_bounds__(64) void k_rnn_ln_fwd(RnnNormP p) {
  const int row = blockIdx.x, lane = threadIdx.x;
  if (row >= p.rows) return;
  rnn_norm_run(p, blockIdx.y);
#pragma unroll
  for (int j = 0; j < RNN_NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < p.H) {
      float y = p.s[(long)row * p.sp + c];
      if (p.mask) y = y * p.mask[(long)row * p.H + c] * p.scale;
      if (p.res) y = p.res[(long)row * p.rp + c] + y;
      p.u[(long)row * p.up + c] = y;
    }
  }
  float v[RNN_NJ], mean, rstd;
  norm_stats(p.u + (long)row * p.up, p.H, lane, v, mean, rstd);     // (a lane reads back what it wrote itself)
#pragma unroll
  for (int j = 0; j < RNN_NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < p.H) p.out[(long)row * p.op + c] = (v[j] - mean) * rstd * p.gamma[c] + p.beta[c];
  }
}

// the backward of k_rnn_ln_fwd: du (to the residual input), dz = du mask / (1 - p) Swish'(z), and the row's dgamma / dbeta terms
__global__ __launch_bounds__(64) void k_rnn_ln_bwd(RnnNormP p) {
  const int row = blockIdx.x, lane = threadIdx.x;
  if (row >= p.rows) return;
  rnn_norm_run(p, blockIdx.y);
  float v[RNN_NJ], mean, rstd;
  norm_stats(p.u + (long)row * p.up, p.H, lane, v, mean, rstd);
  float dxh[RNN_NJ], xh[RNN_NJ];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < RNN_NJ; ++j) {
    const int c = lane + 64 * j;
    dxh[j] = 0.f; xh[j] = 0.f;
    if (c < p.H) {
      float dy = p.g[0][(long)row * p.gpitch[0] + c];
      if (p.nterm > 1) dy += p.g[1][(long)row * p.gpitch[1] + c];
      xh[j] = (v[j] - mean) * rstd;
      p.part[(long)row * p.pn + c] = dy * xh[j];
      p.part[(long)row * p.pn + p.H + c] = dy;
      dxh[j] = dy * p.gamma[c];
      s1 += dxh[j];
      s2 += dxh[j] * xh[j];
    }
  }
  const NormBwd nb(s1, s2, rstd, p.H);
#pragma unroll
  for (int j = 0; j < RNN_NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < p.H) {
      const float du = nb.dx(dxh[j], xh[j]);
      if (p.du) p.du[(long)row * p.dup + c] = du;
      float ds = du;
      if (p.mask) ds = du * p.mask[(long)row * p.H + c] * p.scale;
      p.dz[(long)row * p.dzp + c] = ds * rnn_dswish(p.zpre[(long)row * p.zp + c]);
    }
  }
}

// dz = (a + b) Swish'(z): the merge layer under the first residual block; run blockIdx.y at each matrix's run stride
__global__ void k_rnn_swish_bwd(const float* __restrict__ a, int ap, long a_rs, const float* __restrict__ b, int bp, long b_rs,
                                const float* __restrict__ z, int zp, long z_rs, float* __restrict__ dz, int dp, long d_rs, long rows, int cols) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * cols) return;
  const long run = blockIdx.y;
  a += run * a_rs; b += run * b_rs; z += run * z_rs; dz += run * d_rs;
  const long r = e / cols; const int c = (int)(e - r * cols);
  dz[r * dp + c] = (a[r * ap + c] + b[r * bp + c]) * rnn_dswish(z[r * zp + c]);
}

// first level: chunk sums of 64 rows each in row order, [chunks][pn]; run blockIdx.z
// (not merged with diffusion.hip's k_diff_colsum, which adds all rows in one pass: the orders of summation differ and the tests pin both)
__global__ void k_rnn_colsum_part(const float* __restrict__ part, long part_rs, long pn, long rows, float* __restrict__ chunk, long chunk_rs) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= pn) return;
  part += (long)blockIdx.z * part_rs; chunk += (long)blockIdx.z * chunk_rs;
  const long r0 = (long)blockIdx.y * RNN_CHUNK, r1 = min(r0 + (long)RNN_CHUNK, rows);
  float s = 0.f;
  for (long r = r0; r < r1; ++r) s += part[r * pn + j];
  chunk[(long)blockIdx.y * pn + j] = s;
}
struct RnnNormDst { long gamma[RNN_MAX_NORMS], beta[RNN_MAX_NORMS]; };
// second level: the chunks in order, into the gradient block at each norm's gamma / beta; run blockIdx.y (G at stride g_rs)
__global__ void k_rnn_colsum_fin(const float* __restrict__ chunk, long chunk_rs, long pn, int chunks, int H, RnnNormDst dst, float* __restrict__ G,
                                 long g_rs) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= pn) return;
  chunk += (long)blockIdx.y * chunk_rs; G += (long)blockIdx.y * g_rs;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += chunk[(long)c * pn + j];
  const int slot = (int)(j / (2 * H)), c2 = (int)(j - (long)slot * 2 * H);
  G[c2 < H ? dst.gamma[slot] + c2 : dst.beta[slot] + (c2 - H)] = s;
}

// G[i] = the slabs' sum in slab order: the k ranges of the split weight gradients (and slab 0's dgamma / dbeta)
__global__ __launch_bounds__(256) void k_rnn_slab_sum(const float* __restrict__ slabs, long P, int n_slabs, float* __restrict__ G) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  float s = slabs[i];
  for (int k = 1; k < n_slabs; ++k) s += slabs[(long)k * P + i];
  G[i] = s;
}

// torch.optim.Adam (exp_avg lerp, exp_avg_sq, the bias corrections of step k + 1).  omb1 / omb2: 1 - beta formed in double on the host and
// rounded once, as torch forms the scalars it passes to lerp_ and addcmul_ (1 - 0.999f is 1.3e-5 away from 0.001f)
__global__ __launch_bounds__(256) void k_rnn_adam(float* __restrict__ params, float* __restrict__ m_, float* __restrict__ v_, const float* __restrict__ G,
                                                  long P, float step, float bc2s, float omb1, float b2, float omb2, float eps) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  float m = m_[i], v = v_[i];
  params[i] = adam_update(params[i], m, v, G[i], step, bc2s, omb1, b2, omb2, eps);
  m_[i] = m; v_[i] = v;
}

// ---- the carried state: one model step of n rows (orl_rnn_state_step) ----
// Every trajectory has a slot in the state [R][L][n_traj][H], kept twice (st[0], st[1]) with a side bit per (run, slot): a step reads a
// slot's h from the buffer its bit names and writes the new h to the other one, and the step's last launch flips the bits of the slots
// it stepped.  The unit tiles of a row are spread over workgroups, each of which reads the WHOLE previous row as its k operand, so the
// new row must not land where a neighbour still reads; a slot no step names keeps its buffer, its bit and its bits.
// The trajectory of row i: idx[i] clamped into the state, or i
__device__ __forceinline__ long rnn_traj_of(const long long* idx, long i, long n_traj) {
  return idx ? min(max((long)idx[i], 0L), n_traj - 1) : i;
}

// x [n][in] = ([obs | act] - mu) / std: StandardScaler.transform's two fp32 operations (a subtraction and a division, nothing to fuse).
// Run blockIdx.y: its own obs / act ([n][od], [n][ad]; strides o_rs, a_rs, 0: shared) and its own x; the scaler is shared
__global__ void k_rnn_roll_in(const float* __restrict__ obs, long o_rs, const float* __restrict__ act, long a_rs, int od, int ad,
                              const float* __restrict__ mu, const float* __restrict__ sd, long n, float* __restrict__ X, int xp, long x_rs) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int in = od + ad;
  if (e >= n * in) return;
  const long run = blockIdx.y;
  const long i = e / in; const int c = (int)(e - i * in);
  const float v = c < od ? obs[run * o_rs + i * od + c] : act[run * a_rs + i * ad + (c - od)];
  X[run * x_rs + i * xp + c] = (v - mu[c]) / sd[c];
}

struct RnnCellP {
  int n, H, K;                       // rows of the step, hidden units, the layer's input width
  const float* x; int xp; long x_rs; // [n][K], pitch xp >= 4 ceil(K / 4) with zero pads: the step's scaled inputs or the h of the layer below
  const float *wih, *whh, *bih, *bhh; long par_rs;     // [3H][K], [3H][H], [3H], [3H]
  const long long* idx;              // [n]: the trajectory of row i, or null (= i); shared by the runs
  float* st[2]; long st_rs;          // this layer's [n_traj][H] in both buffers
  const int* side; long n_traj;      // [R][n_traj]: the buffer that holds each slot's h
  float* ho; int hop; long ho_rs;    // [n][H]: the new h in row order
};

// torch.nn.GRU's cell on one workgroup of one wave: 16 rows x 16 hidden units, grid (row tiles, unit tiles, runs).  Lane
// (i = l & 15, q = l >> 4) carries k = 16 kb + 4 q + s of input row i (x, then the gathered h) and of the three weight rows of unit i,
// as the scan does.  The x and h products of r and of z share an accumulator (first every k of x, then every k of h: one fixed order
// per element); n keeps W_in x and W_hn h apart.  A row past n repeats row n - 1 and its results are dropped, so an element's value
// does not depend on its tile's other rows.  Layer 0's W_ih rows are K floats long, no multiple of 4: those are loaded one by one
__global__ __launch_bounds__(64) void k_rnn_cell(RnnCellP p) {
  const int H = p.H, K = p.K;
  const int lane = threadIdx.x, li = lane & 15, lq = lane >> 4;
  const int b0 = blockIdx.x * RNN_RB;
  const int nrow = min((int)RNN_RB, p.n - b0);
  {
    const long run = blockIdx.z;
    p.x += run * p.x_rs; p.wih += run * p.par_rs; p.whh += run * p.par_rs; p.bih += run * p.par_rs; p.bhh += run * p.par_rs;
    p.st[0] += run * p.st_rs; p.st[1] += run * p.st_rs; p.side += run * p.n_traj; p.ho += run * p.ho_rs;
  }
  const int j = blockIdx.y * 16 + li;
  const int jc = min(j, H - 1);                         // a clamped unit is computed and dropped
  const long ra = b0 + min(li, nrow - 1);
  const long ta = rnn_traj_of(p.idx, ra, p.n_traj);
  const float* xrow = p.x + ra * p.xp;
  const float* hrow = p.st[p.side[ta] & 1] + ta * H;
  f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, anx = ar, anh = ar;
  {
    const float* wr = p.wih + (long)jc * K;
    const float* wz = p.wih + (long)(H + jc) * K;
    const float* wn = p.wih + (long)(2 * H + jc) * K;
    const bool quads = (K & 3) == 0;
    for (int k4 = 4 * lq; k4 < ((K + 15) & ~15); k4 += 16) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, vr = a, vz = a, vn = a;
      if (k4 < K) {
        a = *(const f32x4*)(xrow + k4);                 // (inside the pitch; the pads are zero)
        if (quads) {
          vr = *(const f32x4*)(wr + k4); vz = *(const f32x4*)(wz + k4); vn = *(const f32x4*)(wn + k4);
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if (k4 + s < K) { vr[s] = wr[k4 + s]; vz[s] = wz[k4 + s]; vn[s] = wn[k4 + s]; }
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], vr[s], ar, 0, 0, 0);      // D[row 4 q + r][unit i]
        az = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], vz[s], az, 0, 0, 0);
        anx = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], vn[s], anx, 0, 0, 0);
      }
    }
  }
  {
    const float* wr = p.whh + (long)jc * H;
    const float* wz = p.whh + (long)(H + jc) * H;
    const float* wn = p.whh + (long)(2 * H + jc) * H;
    for (int k4 = 4 * lq; k4 < ((H + 15) & ~15); k4 += 16) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, vr = a, vz = a, vn = a;
      if (k4 < H) {                                     // (H is a multiple of 4: a quad is inside or outside)
        a = *(const f32x4*)(hrow + k4);
        vr = *(const f32x4*)(wr + k4); vz = *(const f32x4*)(wz + k4); vn = *(const f32x4*)(wn + k4);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], vr[s], ar, 0, 0, 0);
        az = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], vz[s], az, 0, 0, 0);
        anh = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], vn[s], anh, 0, 0, 0);
      }
    }
  }
  if (j >= H) return;
  const float bir = p.bih[j], biz = p.bih[H + j], bin = p.bih[2 * H + j];
  const float bhr = p.bhh[j], bhz = p.bhh[H + j], bhn = p.bhh[2 * H + j];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = 4 * lq + r;
    if (b < nrow) {
      const long t = rnn_traj_of(p.idx, b0 + b, p.n_traj);
      const int sd = p.side[t] & 1;
      const float hprev = p.st[sd][t * H + j];
      const float rg = rnn_sigmoid((ar[r] + bir) + bhr);
      const float zg = rnn_sigmoid((az[r] + biz) + bhz);
      const float ng = tanhf((anx[r] + bin) + rg * (anh[r] + bhn));
      const float hv = (1.f - zg) * ng + zg * hprev;
      p.st[sd ^ 1][t * H + j] = hv;
      p.ho[(long)(b0 + b) * p.hop + j] = hv;
    }
  }
}

// next_obs [n][od - 1] = pred[:, :-1] + obs, reward [n] = pred[:, -1] (plain fp32), and the side bits of the stepped slots flipped: the
// step's last launch, after every layer has read them.  Run blockIdx.y
__global__ void k_rnn_roll_head(const float* __restrict__ pred, int pp, long p_rs, const float* __restrict__ obs, long o_rs, int od, long n,
                                float* __restrict__ next_obs, float* __restrict__ reward, const long long* __restrict__ idx, int* __restrict__ side,
                                long n_traj) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * od) return;
  const long run = blockIdx.y;
  const long i = e / od; const int c = (int)(e - i * od);
  const float v = pred[run * p_rs + i * pp + c];
  if (c < od - 1) next_obs[(run * n + i) * (od - 1) + c] = v + obs[run * o_rs + i * (od - 1) + c];
  else {
    reward[run * n + i] = v;
    side[run * n_traj + rnn_traj_of(idx, i, n_traj)] ^= 1;
  }
}

}  // namespace orl

using namespace orl;

struct RnnLin { long w, b; };
struct RnnNorm { long g, b; };
// activations of one pass over `cap` rows (sequences x time steps) of `runs` runs, every matrix [runs][cap][pitch] (DevMat::s0 is the
// run stride); the backward's buffers when train
struct RnnWs {
  long cap = 0; int runs = 0; bool train = false;
  DevMat X0, SI, ZI, UI, CAT, M0, ZM, PRED;
  std::vector<DevMat> GI, HO, R, Z, NN, HN, HP;       // per GRU layer
  std::vector<DevMat> SB, ZB, UB, XO;                 // per residual block
  float* MK = nullptr;                                // [runs][norms][cap][H] keep masks
  // backward
  DevMat dPRED, dX, DU, DZ, DT, dZM, dCAT, dGI, dGH, dXL[2];
  float *part = nullptr, *chunk = nullptr;            // [runs][cap][pn], [runs][chunks of cap][pn]
  long mk_rs = 0, part_rs = 0, chunk_rs = 0;          // their run strides
  // What each stage of the backward writes: GRU layer l's dGI / dGH and the dXL of its input, block i's DU and DT, norm slot s's DZ.
  // By default they are views of the shared buffers above (every layer's dGI is dGI, layer l's dXL is dXL[l & 1], ...), which a later
  // stage overwrites; with keep (orl_rnn_debug_keep, tests only) every stage owns a matrix of the same pitch and run stride
  std::vector<DevMat> dGIl, dGHl, dXLl, DUb, DTb, DZs;
  bool keep = false;
};

struct orl_rnn {
  orl_rnn_config c;
  int in, od, H, L, nb, B, Tmax, norms;
  int R = 1;                                      // runs: the blocks below are [R][P], run r's at r * P
  long P = 0;
  RnnLin wih[RNN_MAX_LAYERS], whh[RNN_MAX_LAYERS], lin_in, lin_merge, lin_out, lin_b[ORL_MAX_HIDDEN];
  RnnNorm norm_in, norm_b[ORL_MAX_HIDDEN];
  TensorTable tensors;
  hipStream_t stream = nullptr;
  float *params = nullptr, *adam_m = nullptr, *adam_v = nullptr, *grads = nullptr;
  float* slabs = nullptr; int max_slabs = 1;      // [max_slabs][R][P]: the k ranges of the split weight gradients, summed into grads
  long long kstep = 0;                            // shared by the runs
  size_t lds_fwd = 0, lds_bwd = 0;
  // dataset (one, read by every run)
  float *d_in = nullptr, *d_tgt = nullptr, *d_msk = nullptr; long n_data = 0; int T = 0;
  RnnWs tw, ew;
  // TGT [R][cap][od], MSK [R][cap], loss_cell [R], loss_steps [steps][R]
  float *TGT = nullptr, *MSK = nullptr, *loss_cell = nullptr, *loss_steps = nullptr; long loss_cap = 0;
  long long* idx_d = nullptr; long idx_cap = 0;
  // forward staging
  float *fIn = nullptr, *fLast = nullptr, *fAll = nullptr; long f_cap = 0; int f_runs = 0;
  // what the taps read: the workspace of the last pass, its rows, and the runs it held (run last_r0 + i at workspace slot i); last_roll:
  // that pass was a state step (no input projections kept, the roll.* names readable)
  const RnnWs* last_ws = nullptr; long last_rows = 0; int last_r0 = 0, last_nr = 0; bool last_roll = false;
  // the carried state (orl_rnn_state_*): st[0], st[1] [R][L][n_traj][H], side [R][n_traj] (k_rnn_cell says how they take turns); the
  // input scaler [in] each; a step's host arrays staged as obs | act | next_obs | reward, and its trajectory indices
  float* st[2] = {nullptr, nullptr}; int* side = nullptr; long n_traj = 0;
  float *sc_mu = nullptr, *sc_std = nullptr; bool has_scaler = false;
  float* r_stage = nullptr; long r_stage_cap = 0;
  long long* r_idx = nullptr; long r_idx_cap = 0;
  // orl_rnn_profile: events of the last step -- 0 start, 1 after the forward, 2 after the backward, 3 after Adam, then per layer
  // [before, after] of the forward scan and of the backward scan
  bool prof = false, prof_valid = false;
  hipEvent_t ev[4 + 4 * RNN_MAX_LAYERS] = {};
  DevAllocs mem{"orl_rnn"};
};

static int rnn_ws_stages(orl_rnn* d, RnnWs& w, bool keep);

static int rnn_ws_alloc(orl_rnn* d, RnnWs& w, long rows, bool train, int runs) {
  const int H = d->H, L = d->L, nb = d->nb;
  auto rnn_mat = [runs](orl_rnn* o, DevMat& v, long n, int cols) { return dev_mat(o->mem, v, n, cols, runs); };
  w.GI.resize(L); w.HO.resize(L); w.R.resize(L); w.Z.resize(L); w.NN.resize(L); w.HN.resize(L); w.HP.resize(L);
  w.SB.resize(nb); w.ZB.resize(nb); w.UB.resize(nb); w.XO.resize(nb);
  bool bad = rnn_mat(d, w.X0, rows, d->in) || rnn_mat(d, w.SI, rows, H) || rnn_mat(d, w.ZI, rows, H) || rnn_mat(d, w.UI, rows, H) ||
             rnn_mat(d, w.CAT, rows, 2 * H) || rnn_mat(d, w.M0, rows, H) || rnn_mat(d, w.ZM, rows, H) || rnn_mat(d, w.PRED, rows, d->od);
  for (int l = 0; l < L && !bad; ++l) {
    bad = rnn_mat(d, w.GI[l], rows, 3 * H) || (l < L - 1 && rnn_mat(d, w.HO[l], rows, H));
    if (l == L - 1) w.HO[l] = w.CAT.cols(H);          // the last layer writes the right half of the merge layer's input
    if (train && !bad)
      bad = rnn_mat(d, w.R[l], rows, H) || rnn_mat(d, w.Z[l], rows, H) || rnn_mat(d, w.NN[l], rows, H) || rnn_mat(d, w.HN[l], rows, H) ||
            rnn_mat(d, w.HP[l], rows, H);
  }
  for (int i = 0; i < nb && !bad; ++i)
    bad = rnn_mat(d, w.SB[i], rows, H) || rnn_mat(d, w.ZB[i], rows, H) || rnn_mat(d, w.UB[i], rows, H) || rnn_mat(d, w.XO[i], rows, H);
  if (train && !bad) {
    const long pn = (long)d->norms * 2 * H, chunks = (rows + RNN_CHUNK - 1) / RNN_CHUNK;
    bad = rnn_mat(d, w.dPRED, rows, d->od) || rnn_mat(d, w.dX, rows, H) || rnn_mat(d, w.DU, rows, H) || rnn_mat(d, w.DZ, rows, H) ||
          rnn_mat(d, w.DT, rows, H) || rnn_mat(d, w.dZM, rows, H) || rnn_mat(d, w.dCAT, rows, 2 * H) || rnn_mat(d, w.dGI, rows, 3 * H) ||
          rnn_mat(d, w.dGH, rows, 3 * H) || rnn_mat(d, w.dXL[0], rows, H) || rnn_mat(d, w.dXL[1], rows, H) ||
          (d->mem.free(w.MK), d->mem.alloc(&w.MK, (size_t)runs * d->norms * rows * H)) ||
          (d->mem.free(w.part), d->mem.alloc(&w.part, (size_t)runs * rows * pn)) ||
          (d->mem.free(w.chunk), d->mem.alloc(&w.chunk, (size_t)runs * chunks * pn));
    w.mk_rs = (long)d->norms * rows * H; w.part_rs = rows * pn; w.chunk_rs = chunks * pn;
  }
  if (bad) return -1;
  w.cap = rows; w.runs = runs; w.train = train;
  return train ? rnn_ws_stages(d, w, false) : 0;
}

// the per-stage views of the backward: onto the shared buffers, or (keep) onto matrices of their own.  The stream is idle
static int rnn_ws_stages(orl_rnn* d, RnnWs& w, bool keep) {
  const int H = d->H, L = d->L, nb = d->nb;
  std::vector<DevMat>* all[] = {&w.dGIl, &w.dGHl, &w.dXLl, &w.DUb, &w.DTb, &w.DZs};
  if (w.keep)
    for (auto* v : all)
      for (DevMat& m : *v) d->mem.free(m.p);
  w.keep = false;
  w.dGIl.assign(L, w.dGI); w.dGHl.assign(L, w.dGH); w.dXLl.resize(L);
  for (int l = 0; l < L; ++l) w.dXLl[l] = w.dXL[l & 1];
  w.DUb.assign(nb, w.DU); w.DTb.assign(nb, w.DT); w.DZs.assign(nb + 1, w.DZ);
  if (!keep) return 0;
  for (auto* v : all)
    for (DevMat& m : *v) m = DevMat();
  w.keep = true;
  bool bad = false;
  for (int l = 0; l < L && !bad; ++l)
    bad = dev_mat(d->mem, w.dGIl[l], w.cap, 3 * H, w.runs) || dev_mat(d->mem, w.dGHl[l], w.cap, 3 * H, w.runs) ||
          dev_mat(d->mem, w.dXLl[l], w.cap, H, w.runs);
  for (int i = 0; i < nb && !bad; ++i) bad = dev_mat(d->mem, w.DUb[i], w.cap, H, w.runs) || dev_mat(d->mem, w.DTb[i], w.cap, H, w.runs);
  for (int s = 0; s <= nb && !bad; ++s) bad = dev_mat(d->mem, w.DZs[s], w.cap, H, w.runs);
  if (bad) {
    rnn_ws_stages(d, w, false);
    return -1;
  }
  return 0;
}

// ---- the matrix products (csrc/gemm.h): one launch per product, the runs as its batch (z0) ----
// The runs r0 .. r0 + n of the object that a pass computes, at slots 0 .. n of its workspace.  The tile configuration and the slab count
// of every product are functions of the per-run shape only, so an output element's reduction order -- and run r's bits -- do not depend
// on how many runs share the launch.
struct RnnRuns { int r0, n; };
// the weight gradients reduce over every row of the step and have few output tiles: the smallest tile that still gives the CUs work
static int rnn_wgrad_cfg(int M, int N) {
  if (N <= 16) return CFG_TALL;
  const long small_tiles = (long)((M + 15) / 16) * ((N + 63) / 64);
  return small_tiles <= 1024 ? CFG_SMALL : CFG_MID;
}
// layer l of the runs' blocks [.][P] starting at `block`
static LinearP rnn_linear(const orl_rnn* d, float* block, const RnnLin& l, int in, int out) {
  return {{block + l.w, d->P, 0}, {block + l.b, d->P, 0}, in, out, false, 1};
}
static float* rnn_params_of(orl_rnn* d, const RnnRuns& rs) { return d->params + (long)rs.r0 * d->P; }
// Y = X W^T + b, or swish of it with the pre-activation kept in Z (same pitch as Y) when Z is given
static int rnn_fwd(orl_rnn* d, const RnnRuns& rs, const DevMat& X, int M, const RnnLin& l, int in, int out, const DevMat& Y, bool swish, float* Z) {
  GemmP p = linear_fwd_p(X, M, rnn_linear(d, rnn_params_of(d, rs), l, in, out), Y);
  p.z_out = Z;
  const bool kpad = X.pitch >= rup4(p.K);
  const int cfg = linear_cfg(p.M, p.N);
  return gemm_done(swish ? launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_SWISH>(cfg, p, rs.n, d->stream, kpad, false, P_F32)
                         : launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS>(cfg, p, rs.n, d->stream, kpad, false, P_F32), "orl_rnn forward");
}
// dX = dY W
static int rnn_dgrad(orl_rnn* d, const RnnRuns& rs, const DevMat& dY, int M, const RnnLin& l, int in, int out, const DevMat& dX) {
  const GemmP p = linear_dgrad_p(dY, M, rnn_linear(d, rnn_params_of(d, rs), l, in, out), dX);
  return gemm_done(launch_gemm<PA_PLAIN, PB_PLAIN, E_PLAIN>(linear_cfg(p.M, p.N), p, rs.n, d->stream, dY.pitch >= rup4(p.K), false, P_F32), "orl_rnn dgrad");
}
// The weight gradients reduce over all rows * T rows of a step and have few output tiles (600 x 200 at the default shape), so the
// reduction is cut into k ranges of at least 256 rows, each into a slab of its own; k_rnn_slab_sum adds the slabs in order.
static int rnn_slabs(const orl_rnn* d, long N) { return (int)std::max(1L, std::min((long)d->max_slabs, N / 256)); }
// dW = dY^T X ([out][in]) and db = the column sums of dY into the slabs ([slab][R][P]; the backward runs every run of the object)
static int rnn_wgrad(orl_rnn* d, const DevMat& dY, const DevMat& X, int M, const RnnLin& l, int in, int out) {
  GemmP p = linear_wgrad_p(dY, X, M, rnn_linear(d, d->slabs, l, in, out));
  p.ksplit = rnn_slabs(d, M); p.c_ks = (long)d->R * d->P; p.bo_ks = p.c_ks;
  return gemm_done(launch_gemm<PA_PLAIN, PB_PLAIN, E_WGRAD>(rnn_wgrad_cfg(p.M, p.N), p, d->R, d->stream, false, false, P_F32), "orl_rnn wgrad");
}

// the profile's event `i` on the stream when the step is being timed
static void rnn_mark(orl_rnn* d, bool on, int i) {
  if (on && d->prof) hipEventRecord(d->ev[i], d->stream);
}

static RnnNormP rnn_norm_params(orl_rnn* d, const RnnRuns& rs, const RnnWs& w, int slot, long N, const DevMat& S, const DevMat& U, const RnnNorm& nm,
                                bool drop) {
  RnnNormP p;
  memset(&p, 0, sizeof(p));
  p.rows = (int)N; p.H = d->H;
  p.s = S.p; p.sp = S.pitch; p.s_rs = S.s0;
  if (drop) { p.mask = w.MK + (size_t)slot * w.cap * d->H; p.mask_rs = w.mk_rs; p.scale = 1.f / (1.f - d->c.dropout_rate); }
  p.gamma = rnn_params_of(d, rs) + nm.g; p.beta = rnn_params_of(d, rs) + nm.b; p.par_rs = d->P;
  p.u = U.p; p.up = U.pitch; p.u_rs = U.s0;
  return p;
}

// the GRU layers of the runs rs over `rows` sequences of T steps from h = 0: per layer the input projections of every step in one
// product, then the scan.  X0: the input rows; layer l's h_t goes to w.HO[l]
static int rnn_gru_windows(orl_rnn* d, const RnnRuns& rs, RnnWs& w, const DevMat& X0, int rows, int T, bool train) {
  const int H = d->H;
  const long N = (long)rows * T;
  float* params = rnn_params_of(d, rs);
  DevMat X = X0;
  for (int l = 0; l < d->L; ++l) {
    if (rnn_fwd(d, rs, X, (int)N, d->wih[l], l ? H : d->in, 3 * H, w.GI[l], false, nullptr)) return -1;
    RnnScanP sp;
    memset(&sp, 0, sizeof(sp));
    sp.rows = rows; sp.T = T; sp.H = H;
    sp.gi = w.GI[l].p; sp.gip = w.GI[l].pitch; sp.gi_rs = w.GI[l].s0;
    sp.whh = params + d->whh[l].w; sp.bhh = params + d->whh[l].b; sp.par_rs = d->P;
    sp.ho = w.HO[l].p; sp.hop = w.HO[l].pitch; sp.ho_rs = w.HO[l].s0;
    if (train) {
      sp.r = w.R[l].p; sp.z = w.Z[l].p; sp.n = w.NN[l].p; sp.hn = w.HN[l].p; sp.hp = w.HP[l].p; sp.sp = w.R[l].pitch; sp.s_rs = w.R[l].s0;
    }
    rnn_mark(d, train, 4 + 4 * l);
    DEV_LAUNCH(d->stream, k_rnn_scan_fwd, dim3((rows + RNN_RB - 1) / RNN_RB, rs.n), dim3(64 * RNN_FWD_WAVES), d->lds_fwd, sp);
    rnn_mark(d, train, 5 + 4 * l);
    X = w.HO[l];
  }
  return 0;
}

// the tail over N rows: the input block on X0, the merge layer on [its output | the top GRU layer's h] (w.CAT), the residual blocks and the
// head into w.PRED.  The window forward and the one-step path (orl_rnn_state_step) both end here
static int rnn_tail(orl_rnn* d, const RnnRuns& rs, RnnWs& w, const DevMat& X0, long N, bool train) {
  const int H = d->H;
  const bool drop = train && d->c.dropout_rate > 0.f;
  if (rnn_fwd(d, rs, X0, (int)N, d->lin_in, d->in, H, w.SI, true, train ? w.ZI.p : nullptr)) return -1;
  RnnNormP n0 = rnn_norm_params(d, rs, w, 0, N, w.SI, w.UI, d->norm_in, drop);
  n0.out = w.CAT.p; n0.op = w.CAT.pitch; n0.out_rs = w.CAT.s0;
  DEV_LAUNCH(d->stream, k_rnn_ln_fwd, dim3((unsigned)N, rs.n), dim3(64), 0, n0);
  if (rnn_fwd(d, rs, w.CAT, (int)N, d->lin_merge, 2 * H, H, w.M0, true, train ? w.ZM.p : nullptr)) return -1;
  DevMat X = w.M0;
  for (int i = 0; i < d->nb; ++i) {
    if (rnn_fwd(d, rs, X, (int)N, d->lin_b[i], H, H, w.SB[i], true, train ? w.ZB[i].p : nullptr)) return -1;
    RnnNormP nb = rnn_norm_params(d, rs, w, 1 + i, N, w.SB[i], w.UB[i], d->norm_b[i], drop);
    nb.res = X.p; nb.rp = X.pitch; nb.res_rs = X.s0;
    nb.out = w.XO[i].p; nb.op = w.XO[i].pitch; nb.out_rs = w.XO[i].s0;
    DEV_LAUNCH(d->stream, k_rnn_ln_fwd, dim3((unsigned)N, rs.n), dim3(64), 0, nb);
    X = w.XO[i];
  }
  return rnn_fwd(d, rs, X, (int)N, d->lin_out, H, d->od, w.PRED, false, nullptr);
}

// the forward of the runs rs over `rows` sequences of T steps of workspace w (X0 in place; shared_x: every run reads slot 0's X0); train:
// the scans save what the backward reads, the pre-activations are kept and the dropouts read the keep masks of w.MK
static int rnn_forward(orl_rnn* d, const RnnRuns& rs, RnnWs& w, int rows, int T, bool train, bool shared_x) {
  DevMat X0 = w.X0;
  if (shared_x) X0.s0 = 0;
  return rnn_gru_windows(d, rs, w, X0, rows, T, train) || rnn_tail(d, rs, w, X0, (long)rows * T, train) ? -1 : 0;
}

// backward of every run from dPRED over the first rows * T rows of the training workspace
static int rnn_backward(orl_rnn* d, RnnWs& w, int rows, int T) {
  const int H = d->H, R = d->R;
  const RnnRuns rs{0, R};
  const long N = (long)rows * T;
  const long pn = (long)d->norms * 2 * H;
  const bool drop = d->c.dropout_rate > 0.f;
  const DevMat& last = w.XO[d->nb - 1];
  if (rnn_wgrad(d, w.dPRED, last, (int)N, d->lin_out, H, d->od) || rnn_dgrad(d, rs, w.dPRED, (int)N, d->lin_out, H, d->od, w.dX)) return -1;
  // residual block i: dOut = dX (block nb - 1: the head's dgrad) or DU + DT of the block above
  for (int i = d->nb - 1; i >= 0; --i) {
    const DevMat& Xin = i ? w.XO[i - 1] : w.M0;
    RnnNormP nb = rnn_norm_params(d, rs, w, 1 + i, N, w.SB[i], w.UB[i], d->norm_b[i], drop);
    if (i == d->nb - 1) { nb.nterm = 1; nb.g[0] = w.dX.p; nb.gpitch[0] = w.dX.pitch; nb.g_rs[0] = w.dX.s0; }
    else {
      const DevMat &gu = w.DUb[i + 1], &gt = w.DTb[i + 1];
      nb.nterm = 2; nb.g[0] = gu.p; nb.gpitch[0] = gu.pitch; nb.g_rs[0] = gu.s0;
      nb.g[1] = gt.p; nb.gpitch[1] = gt.pitch; nb.g_rs[1] = gt.s0;
    }
    const DevMat &DU = w.DUb[i], &DZ = w.DZs[1 + i];
    nb.zpre = w.ZB[i].p; nb.zp = w.ZB[i].pitch; nb.z_rs = w.ZB[i].s0;
    nb.du = DU.p; nb.dup = DU.pitch; nb.du_rs = DU.s0;             // (shared: a lane overwrites only the elements it has read itself)
    nb.dz = DZ.p; nb.dzp = DZ.pitch; nb.dz_rs = DZ.s0;
    nb.part = w.part + (long)(1 + i) * 2 * H; nb.pn = pn; nb.part_rs = w.part_rs;
    DEV_LAUNCH(d->stream, k_rnn_ln_bwd, dim3((unsigned)N, R), dim3(64), 0, nb);
    if (rnn_wgrad(d, DZ, Xin, (int)N, d->lin_b[i], H, H) || rnn_dgrad(d, rs, DZ, (int)N, d->lin_b[i], H, H, w.DTb[i])) return -1;
  }
  const DevMat &DU0 = w.DUb[0], &DT0 = w.DTb[0];
  DEV_LAUNCH(d->stream, k_rnn_swish_bwd, dim3(ew_grid(N * H), R), dim3(256), 0, DU0.p, DU0.pitch, DU0.s0, DT0.p, DT0.pitch, DT0.s0,
              w.ZM.p, w.ZM.pitch, w.ZM.s0, w.dZM.p, w.dZM.pitch, w.dZM.s0, N, H);
  if (rnn_wgrad(d, w.dZM, w.CAT, (int)N, d->lin_merge, 2 * H, H) || rnn_dgrad(d, rs, w.dZM, (int)N, d->lin_merge, 2 * H, H, w.dCAT)) return -1;
  // the input block (no residual, no gradient to the net's input)
  {
    RnnNormP n0 = rnn_norm_params(d, rs, w, 0, N, w.SI, w.UI, d->norm_in, drop);
    n0.nterm = 1; n0.g[0] = w.dCAT.p; n0.gpitch[0] = w.dCAT.pitch; n0.g_rs[0] = w.dCAT.s0;
    n0.zpre = w.ZI.p; n0.zp = w.ZI.pitch; n0.z_rs = w.ZI.s0;
    const DevMat& DZ = w.DZs[0];
    n0.dz = DZ.p; n0.dzp = DZ.pitch; n0.dz_rs = DZ.s0;
    n0.part = w.part; n0.pn = pn; n0.part_rs = w.part_rs;
    DEV_LAUNCH(d->stream, k_rnn_ln_bwd, dim3((unsigned)N, R), dim3(64), 0, n0);
    if (rnn_wgrad(d, DZ, w.X0, (int)N, d->lin_in, d->in, H)) return -1;
  }
  {
    const int chunks = (int)((N + RNN_CHUNK - 1) / RNN_CHUNK);
    RnnNormDst dst;
    memset(&dst, 0, sizeof(dst));
    dst.gamma[0] = d->norm_in.g; dst.beta[0] = d->norm_in.b;
    for (int i = 0; i < d->nb; ++i) { dst.gamma[1 + i] = d->norm_b[i].g; dst.beta[1 + i] = d->norm_b[i].b; }
    DEV_LAUNCH(d->stream, k_rnn_colsum_part, dim3(ew_grid(pn), chunks, R), dim3(256), 0, w.part, w.part_rs, pn, N, w.chunk, w.chunk_rs);
    DEV_LAUNCH(d->stream, k_rnn_colsum_fin, dim3(ew_grid(pn), R), dim3(256), 0, w.chunk, w.chunk_rs, pn, chunks, H, dst, d->slabs, d->P);
  }
  // the GRU layers top down: the top layer's dh is the right half of the merge layer's input gradient
  DevMat dOut = w.dCAT.cols(H);
  for (int l = d->L - 1; l >= 0; --l) {
    RnnScanBP bp;
    memset(&bp, 0, sizeof(bp));
    bp.rows = rows; bp.T = T; bp.H = H;
    bp.dout = dOut.p; bp.dop = dOut.pitch; bp.do_rs = dOut.s0;
    bp.whh = d->params + d->whh[l].w; bp.par_rs = d->P;
    bp.r = w.R[l].p; bp.z = w.Z[l].p; bp.n = w.NN[l].p; bp.hn = w.HN[l].p; bp.hp = w.HP[l].p; bp.sp = w.R[l].pitch; bp.s_rs = w.R[l].s0;
    const DevMat &dGI = w.dGIl[l], &dGH = w.dGHl[l];
    bp.dgi = dGI.p; bp.dgh = dGH.p; bp.gp = dGI.pitch; bp.g_rs = dGI.s0;
    rnn_mark(d, true, 6 + 4 * l);
    DEV_LAUNCH(d->stream, k_rnn_scan_bwd, dim3((rows + RNN_RB - 1) / RNN_RB, R), dim3(64 * RNN_BWD_WAVES), d->lds_bwd, bp);
    rnn_mark(d, true, 7 + 4 * l);
    const DevMat& Xl = l ? w.HO[l - 1] : w.X0;
    if (rnn_wgrad(d, dGH, w.HP[l], (int)N, d->whh[l], H, 3 * H) || rnn_wgrad(d, dGI, Xl, (int)N, d->wih[l], l ? H : d->in, 3 * H)) return -1;
    if (l == 0) break;
    if (rnn_dgrad(d, rs, dGI, (int)N, d->wih[l], H, 3 * H, w.dXLl[l])) return -1;
    dOut = w.dXLl[l];
  }
  const long RP = (long)R * d->P;
  DEV_LAUNCH(d->stream, k_rnn_slab_sum, dim3(ew_grid(RP)), dim3(256), 0, (const float*)d->slabs, RP, rnn_slabs(d, N), d->grads);
  return 0;
}

// one optimizer step of every run, run r on the sequences idx[r * idx_rs + (0 .. rows)) (device); the dropouts' keep masks are in tw.MK
// already when forced.  loss_dst: [R]
static int rnn_enqueue_step(orl_rnn* d, const long long* idx, long idx_rs, int rows, bool forced_masks, float* loss_dst) {
  RnnWs& w = d->tw;
  const int T = d->T, H = d->H, R = d->R;
  const long N = (long)rows * T, RP = (long)R * d->P;
  rnn_mark(d, true, 0);
  DEV_LAUNCH(d->stream, k_rnn_gather, dim3(ew_grid(N * (d->in + d->od + 1)), R), dim3(256), 0, d->d_in, d->d_tgt, d->d_msk, idx, idx_rs,
              d->n_data, T, d->in, d->od, rows, w.X0.p, w.X0.pitch, w.X0.s0, d->TGT, d->MSK, w.cap);
  if (d->c.dropout_rate > 0.f && !forced_masks)
    for (int s = 0; s < d->norms; ++s)
      DEV_LAUNCH(d->stream, k_rnn_mask, dim3(ew_grid(N * (H / 4)), R), dim3(256), 0, w.MK + (size_t)s * w.cap * H, w.mk_rs, N, H,
                  1.f - d->c.dropout_rate, d->c.seed, (uint64_t)d->kstep, (uint32_t)s);
  if (rnn_forward(d, RnnRuns{0, R}, w, rows, T, true, false)) return -1;
  rnn_mark(d, true, 1);
  DEV_LAUNCH(d->stream, k_mse_loss<true>, dim3(R), dim3(256), 0, (const float*)w.PRED.p, w.PRED.pitch, w.PRED.s0, (const float*)d->TGT,
              (const float*)d->MSK, w.cap, N, d->od, w.dPRED.p, loss_dst, d->loss_cell);
  if (rnn_backward(d, w, rows, T)) return -1;
  rnn_mark(d, true, 2);
  const double tt = (double)(d->kstep + 1);
  const double bc1 = 1.0 - std::pow(d->c.adam_beta1, tt), bc2 = 1.0 - std::pow(d->c.adam_beta2, tt);
  DEV_LAUNCH(d->stream, k_rnn_adam, dim3(ew_grid(RP)), dim3(256), 0, d->params, d->adam_m, d->adam_v, d->grads, RP, (float)(d->c.lr / bc1),
              (float)std::sqrt(bc2), (float)(1.0 - d->c.adam_beta1), (float)d->c.adam_beta2, (float)(1.0 - d->c.adam_beta2), (float)d->c.adam_eps);
  rnn_mark(d, true, 3);
  d->prof_valid = d->prof;
  d->kstep += 1;
  d->last_ws = &w; d->last_rows = N; d->last_r0 = 0; d->last_nr = R; d->last_roll = false;
  return 0;
}

static int rnn_ready(orl_rnn* d, const char* what, bool data) {
  if (!d) return fail(std::string(what) + ": null handle");
  if (data && !d->d_in) return fail(std::string(what) + ": no data loaded (orl_rnn_load_data)");
  if (hipSetDevice(d->c.device) != hipSuccess) return fail(std::string(what) + ": hipSetDevice failed");
  return 0;
}

// the refusals of a config; empty = supported
static std::string rnn_refusal(const orl_rnn_config& c) {
  if (c.n_runs < 1 || c.n_runs > 64) return "n_runs must be in [1, 64]";
  if (c.precision != 0) return "precision 0 (fp32 MFMA) only; the split precisions are not supported";
  if (c.input_dim < 1 || c.output_dim < 1) return "input_dim and output_dim must be positive";
  if (c.n_hidden < 2 || c.n_hidden > ORL_MAX_HIDDEN + 1)
    return "len(hidden_dims) must be in [2, " + std::to_string(ORL_MAX_HIDDEN + 1) + "]";
  for (int i = 1; i < c.n_hidden; ++i)
    if (c.hidden[i] != c.hidden[0]) return "all hidden_dims must be equal (the residual blocks add their input)";
  if (c.hidden[0] < 8 || c.hidden[0] > RNN_MAX_H || (c.hidden[0] & 3)) return "the hidden width must be a multiple of 4 in [8, 512]";
  if (c.rnn_num_layers < 1 || c.rnn_num_layers > RNN_MAX_LAYERS) return "rnn_num_layers must be in [1, 4]";
  if (!(c.dropout_rate >= 0.f && c.dropout_rate < 1.f)) return "dropout_rate must be in [0, 1)";
  if (c.batch_size < 1 || c.max_seq_len < 1) return "batch_size and max_seq_len must be positive";
  if ((long)c.batch_size * c.max_seq_len > 0x7fffffffL / (8 * c.hidden[0] * (ORL_MAX_HIDDEN + 1)))
    return "batch_size * max_seq_len rows are more than one step's matrices index";
  if (!(c.lr > 0.0)) return "lr must be positive";
  if (!(c.adam_beta1 >= 0.0 && c.adam_beta1 < 1.0 && c.adam_beta2 >= 0.0 && c.adam_beta2 < 1.0 && c.adam_eps >= 0.0)) return "Adam's betas must be in [0, 1) and eps non-negative";
  return "";
}

// the layout of the parameter block: RNNModel.state_dict() order, every tensor on 4 floats
static long rnn_layout(orl_rnn* d) {
  TensorTable& t = d->tensors;
  auto add = [&](const std::string& name, std::initializer_list<long> shape) { return t.add(name, shape, true, false); };
  const long H = d->H;
  for (int l = 0; l < d->L; ++l) {
    const std::string k = std::to_string(l);
    d->wih[l].w = add("rnn_layer.weight_ih_l" + k, {3 * H, l ? H : (long)d->in});
    d->whh[l].w = add("rnn_layer.weight_hh_l" + k, {3 * H, H});
    d->wih[l].b = add("rnn_layer.bias_ih_l" + k, {3 * H});
    d->whh[l].b = add("rnn_layer.bias_hh_l" + k, {3 * H});
  }
  d->lin_in.w = add("input_layer.linear.weight", {H, (long)d->in});
  d->lin_in.b = add("input_layer.linear.bias", {H});
  d->norm_in.g = add("input_layer.layer_norm.weight", {H});
  d->norm_in.b = add("input_layer.layer_norm.bias", {H});
  for (int i = 0; i < d->nb; ++i) {
    const std::string k = "backbones." + std::to_string(i);
    d->lin_b[i].w = add(k + ".linear.weight", {H, H});
    d->lin_b[i].b = add(k + ".linear.bias", {H});
    d->norm_b[i].g = add(k + ".layer_norm.weight", {H});
    d->norm_b[i].b = add(k + ".layer_norm.bias", {H});
  }
  d->lin_merge.w = add("merge_layer.weight", {H, 2 * H});
  d->lin_merge.b = add("merge_layer.bias", {H});
  d->lin_out.w = add("output_layer.weight", {(long)d->od, H});
  d->lin_out.b = add("output_layer.bias", {(long)d->od});
  return t.align4();
}

static void rnn_dims(orl_rnn* d, const orl_rnn_config& c) {
  d->c = c;
  d->in = c.input_dim; d->od = c.output_dim; d->H = c.hidden[0]; d->L = c.rnn_num_layers; d->nb = c.n_hidden - 1;
  d->norms = d->nb + 1; d->B = c.batch_size; d->Tmax = c.max_seq_len; d->R = c.n_runs;
  d->P = rnn_layout(d);
}

extern "C" {

void orl_rnn_config_default(orl_rnn_config* c) {
  memset(c, 0, sizeof(*c));
  c->input_dim = 14; c->output_dim = 12; c->n_hidden = 4;
  for (int i = 0; i < 4; ++i) c->hidden[i] = 200;
  c->rnn_num_layers = 3; c->dropout_rate = 0.1f; c->batch_size = 256; c->max_seq_len = 20; c->lr = 1e-3;
  c->adam_beta1 = 0.9; c->adam_beta2 = 0.999; c->adam_eps = 1e-8;
  c->n_runs = 1; c->device = 0; c->precision = 0; c->seed = 0; c->external_arena = nullptr;
}

int64_t orl_rnn_config_floats(const orl_rnn_config* cfg) {
  if (!cfg) return fail("orl_rnn_config_floats: null argument");
  const std::string why = rnn_refusal(*cfg);
  if (!why.empty()) return fail("orl_rnn_config_floats: " + why);
  orl_rnn tmp;
  rnn_dims(&tmp, *cfg);
  return tmp.P;
}

int orl_rnn_create(const orl_rnn_config* cfg, orl_rnn** out) {
  if (!cfg || !out) return fail("orl_rnn_create: null argument");
  *out = nullptr;
  const orl_rnn_config& c = *cfg;
  const std::string why = rnn_refusal(c);
  if (!why.empty()) return fail("orl_rnn_create: " + why);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("orl_rnn_create: no HIP device (MI355X) visible");
  if (c.device < 0 || c.device >= ndev) return fail("orl_rnn_create: device ordinal out of range");
  if (hipSetDevice(c.device) != hipSuccess) return fail("orl_rnn_create: hipSetDevice failed");
  if (c.external_arena && (((uintptr_t)c.external_arena) & 15)) return fail("orl_rnn_create: external_arena must be 16-byte aligned");
  orl_rnn* d = new orl_rnn();
  rnn_dims(d, c);
  const int H = d->H;
  d->lds_fwd = sizeof(float) * RNN_RB * (size_t)(((H + 15) / 16) * 16 + 4);
  d->lds_bwd = sizeof(float) * RNN_RB * (size_t)(((3 * H + 15) / 16) * 16 + 4 + H + 4);
  bool bad = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess;
  if (!bad && d->lds_bwd > 64 * 1024)
    bad = hipFuncSetAttribute((const void*)k_rnn_scan_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)d->lds_bwd) != hipSuccess;
  const size_t RP = (size_t)d->R * d->P;
  if (c.external_arena) d->params = (float*)c.external_arena;
  else bad = bad || d->mem.alloc(&d->params, RP);
  const long cap = (long)d->B * d->Tmax;
  d->max_slabs = (int)std::max(1L, std::min({8L, cap / 256, (64L << 20) / d->P}));      // (per run: the slab count never depends on R)
  bad = bad || d->mem.alloc(&d->slabs, (size_t)d->max_slabs * RP) || d->mem.alloc(&d->adam_m, RP) || d->mem.alloc(&d->adam_v, RP) ||
        d->mem.alloc(&d->grads, RP) || rnn_ws_alloc(d, d->tw, cap, true, d->R) || d->mem.alloc(&d->TGT, (size_t)d->R * cap * d->od) ||
        d->mem.alloc(&d->MSK, (size_t)d->R * cap) || d->mem.alloc(&d->loss_cell, d->R);
  if (bad) {
    const std::string msg = orl_last_error();
    orl_rnn_destroy(d);
    return fail(msg.empty() ? "orl_rnn_create: allocation failed" : msg);
  }
  *out = d;
  return 0;
}

void orl_rnn_destroy(orl_rnn* d) {
  if (!d) return;
  if (d->stream) hipStreamSynchronize(d->stream);
  for (hipEvent_t e : d->ev)
    if (e) hipEventDestroy(e);
  d->mem.free_all();
  if (d->stream) hipStreamDestroy(d->stream);
  delete d;
}

int64_t orl_rnn_floats(orl_rnn* d) { return d ? d->P : -1; }
int orl_rnn_num_tensors(orl_rnn* d) { return d ? (int)d->tensors.size() : -1; }
int orl_rnn_tensor(orl_rnn* d, int idx, char* name, int name_cap, int64_t* offset, int32_t* ndim, int64_t shape[4]) {
  if (!d || d->tensors.query(idx, name, name_cap, offset, ndim, shape)) return fail("orl_rnn_tensor: index out of range");
  return 0;
}

static float* rnn_block_of(orl_rnn* d, int which) { return which == 0 ? d->params : which == 1 ? d->adam_m : which == 2 ? d->adam_v : nullptr; }
// the one-run entry points on an object of several runs
static int rnn_one_run_only(const orl_rnn* d, const char* what, const char* form) {
  if (d->R == 1) return 0;
  return fail(std::string(what) + ": the object has " + std::to_string(d->R) + " runs, use " + form);
}
static int rnn_run_ok(const orl_rnn* d, int run, const char* what) {
  if (run < 0 || run >= d->R) return fail(std::string(what) + ": run out of range (" + std::to_string(d->R) + " runs)");
  return 0;
}
int orl_rnn_set_run(orl_rnn* d, int run, int which, const float* host, int64_t n) {
  if (!d || !host || !rnn_block_of(d, which)) return fail("orl_rnn_set_run: bad arguments");
  if (rnn_run_ok(d, run, "orl_rnn_set_run")) return -1;
  if (n != d->P) return fail("orl_rnn_set_run: expected " + std::to_string(d->P) + " floats");
  return block_from_host(d->stream, rnn_block_of(d, which) + (long)run * d->P, host, d->P);
}
int orl_rnn_get_run(orl_rnn* d, int run, int which, float* host, int64_t n) {
  if (!d || !host || !rnn_block_of(d, which)) return fail("orl_rnn_get_run: bad arguments");
  if (rnn_run_ok(d, run, "orl_rnn_get_run")) return -1;
  if (n != d->P) return fail("orl_rnn_get_run: expected " + std::to_string(d->P) + " floats");
  return block_to_host(d->stream, host, rnn_block_of(d, which) + (long)run * d->P, d->P);
}
int orl_rnn_set(orl_rnn* d, int which, const float* host, int64_t n) {
  if (!d || !host || !rnn_block_of(d, which)) return fail("orl_rnn_set: bad arguments");
  if (rnn_one_run_only(d, "orl_rnn_set", "orl_rnn_set_run")) return -1;
  if (n != d->P) return fail("orl_rnn_set: expected " + std::to_string(d->P) + " floats");
  return orl_rnn_set_run(d, 0, which, host, n);
}
int orl_rnn_get(orl_rnn* d, int which, float* host, int64_t n) {
  if (!d || !host || !rnn_block_of(d, which)) return fail("orl_rnn_get: bad arguments");
  if (rnn_one_run_only(d, "orl_rnn_get", "orl_rnn_get_run")) return -1;
  if (n != d->P) return fail("orl_rnn_get: expected " + std::to_string(d->P) + " floats");
  return orl_rnn_get_run(d, 0, which, host, n);
}
int orl_rnn_set_step_count(orl_rnn* d, int64_t k) {
  if (!d || k < 0) return fail("orl_rnn_set_step_count: bad arguments");
  d->kstep = k;
  return 0;
}
int64_t orl_rnn_step_count(orl_rnn* d) { return d ? d->kstep : -1; }

int orl_rnn_load_data(orl_rnn* d, const float* inputs, const float* targets, const float* masks, int64_t n, int32_t T) {
  if (rnn_ready(d, "orl_rnn_load_data", false)) return -1;
  if (!inputs || !targets || !masks || n < 1) return fail("orl_rnn_load_data: bad arguments");
  if (T < 1 || T > d->Tmax) return fail("orl_rnn_load_data: need 1 <= T <= max_seq_len (" + std::to_string(d->Tmax) + ")");
  if (n > 0x7fffffffffffLL / ((int64_t)T * (d->in + d->od))) return fail("orl_rnn_load_data: too many sequences");
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->mem.release(&d->d_in, &d->d_tgt, &d->d_msk);
  d->n_data = 0;
  const size_t rows = (size_t)n * T;
  if (d->mem.alloc(&d->d_in, rows * d->in) || d->mem.alloc(&d->d_tgt, rows * d->od) || d->mem.alloc(&d->d_msk, rows)) return -1;
  ORL_HIP(hipMemcpy(d->d_in, inputs, sizeof(float) * rows * d->in, hipMemcpyHostToDevice));
  ORL_HIP(hipMemcpy(d->d_tgt, targets, sizeof(float) * rows * d->od, hipMemcpyHostToDevice));
  ORL_HIP(hipMemcpy(d->d_msk, masks, sizeof(float) * rows, hipMemcpyHostToDevice));
  d->n_data = n; d->T = T;
  return 0;
}

// orl_rnn_step / orl_rnn_step_runs (`what` names the caller in the errors): idx [R][rows], drop_masks [R][norms][rows * T][H], loss_out [R]
static int rnn_step_runs(orl_rnn* d, const char* what, const int64_t* idx, int32_t rows, const float* drop_masks, float* loss_out) {
  const std::string w(what);
  if (!idx || rows < 1 || rows > d->B) return fail(w + ": need 1 <= rows <= batch_size row indices");
  const int R = d->R;
  for (long i = 0; i < (long)R * rows; ++i)
    if (idx[i] < 0 || idx[i] >= d->n_data) return fail(w + ": row index out of range" + (R > 1 ? " in run " + std::to_string(i / rows) : ""));
  if (d->mem.grow(&d->idx_d, &d->idx_cap, (long)R * d->B, d->stream)) return -1;
  ORL_HIP(hipMemcpyAsync(d->idx_d, idx, sizeof(int64_t) * R * rows, hipMemcpyHostToDevice, d->stream));
  const bool forced = drop_masks && d->c.dropout_rate > 0.f;
  if (forced) {
    const size_t per = (size_t)rows * d->T * d->H;
    for (int r = 0; r < R; ++r)
      for (int s = 0; s < d->norms; ++s)
        ORL_HIP(hipMemcpyAsync(d->tw.MK + (size_t)r * d->tw.mk_rs + (size_t)s * d->tw.cap * d->H, drop_masks + ((size_t)r * d->norms + s) * per,
                               sizeof(float) * per, hipMemcpyHostToDevice, d->stream));
  }
  if (rnn_enqueue_step(d, d->idx_d, rows, rows, forced, d->loss_cell)) return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  if (loss_out) ORL_HIP(hipMemcpy(loss_out, d->loss_cell, sizeof(float) * R, hipMemcpyDeviceToHost));
  return 0;
}
int orl_rnn_step(orl_rnn* d, const int64_t* idx, int32_t rows, const float* drop_masks, float* loss_out) {
  if (rnn_ready(d, "orl_rnn_step", true) || rnn_one_run_only(d, "orl_rnn_step", "orl_rnn_step_runs")) return -1;
  return rnn_step_runs(d, "orl_rnn_step", idx, rows, drop_masks, loss_out);
}
int orl_rnn_step_runs(orl_rnn* d, const int64_t* idx, int32_t rows, const float* drop_masks, float* losses_out) {
  if (rnn_ready(d, "orl_rnn_step_runs", true)) return -1;
  return rnn_step_runs(d, "orl_rnn_step_runs", idx, rows, drop_masks, losses_out);
}

// orl_rnn_learn_epoch / orl_rnn_learn_epoch_runs: orders [R][n_rows], losses_out [steps][R]
static int rnn_learn_epoch_runs(orl_rnn* d, const char* what, const int64_t* orders, int64_t n_rows, int on_device, float* losses_out) {
  return learn_epoch_steps(d->stream, d->mem, &d->idx_d, &d->idx_cap, &d->loss_steps, &d->loss_cap, d->B, d->n_data, d->R, what, orders, n_rows,
                           on_device, losses_out, [d, n_rows](const long long* idx, int rows, float* loss_dst) {
                             return rnn_enqueue_step(d, idx, (long)n_rows, rows, false, loss_dst);
                           });
}
int orl_rnn_learn_epoch(orl_rnn* d, const int64_t* order, int64_t n_rows, int on_device, float* losses_out) {
  if (rnn_ready(d, "orl_rnn_learn_epoch", true) || rnn_one_run_only(d, "orl_rnn_learn_epoch", "orl_rnn_learn_epoch_runs")) return -1;
  return rnn_learn_epoch_runs(d, "orl_rnn_learn_epoch", order, n_rows, on_device, losses_out);
}
int orl_rnn_learn_epoch_runs(orl_rnn* d, const int64_t* orders, int64_t n_rows, int on_device, float* losses_out) {
  if (rnn_ready(d, "orl_rnn_learn_epoch_runs", true)) return -1;
  return rnn_learn_epoch_runs(d, "orl_rnn_learn_epoch_runs", orders, n_rows, on_device, losses_out);
}

// the eval workspace and the forward staging for N rows of `runs` runs, grown on demand
static int rnn_eval_ws(orl_rnn* d, long N, int runs) {
  if (N <= d->f_cap && runs <= d->f_runs) return 0;
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->mem.release(&d->fIn, &d->fLast, &d->fAll);
  const long cap = std::max(N, d->f_cap);
  runs = std::max(runs, d->f_runs);
  d->f_cap = 0; d->f_runs = 0;
  if (d->last_ws == &d->ew) d->last_ws = nullptr;
  if (d->mem.alloc(&d->fIn, (size_t)runs * cap * d->in) || d->mem.alloc(&d->fLast, (size_t)runs * cap * d->od) ||
      d->mem.alloc(&d->fAll, (size_t)runs * cap * d->od) || rnn_ws_alloc(d, d->ew, cap, false, runs))
    return -1;
  d->f_cap = cap; d->f_runs = runs;
  return 0;
}
// the eval forward of the runs rs over the windows inputs [n][T][in] (one array when shared or one run, else one per run), enqueued
static int rnn_eval_windows(orl_rnn* d, const RnnRuns& rs, const float* inputs, int64_t n, int32_t T, int on_device, int shared) {
  const int n_in = (shared || rs.n == 1) ? 1 : rs.n;     // input arrays
  const long N = (long)n * T;
  if (rnn_eval_ws(d, N, rs.n)) return -1;
  RnnWs& w = d->ew;
  const float* in_d = inputs;
  if (stage_in(d->stream, in_d, d->fIn, (size_t)n_in * N * d->in, on_device)) return -1;
  DEV_LAUNCH(d->stream, k_rnn_copy, dim3(ew_grid(N * d->in), n_in), dim3(256), 0, in_d, d->in, N * d->in, w.X0.p, w.X0.pitch, w.X0.s0, N, d->in, 1);
  return rnn_forward(d, rs, w, (int)n, T, false, n_in < rs.n);
}

// orl_rnn_forward / orl_rnn_forward_runs: run >= 0 that run alone, -1 every run (inputs shared or [R][n][T][in])
static int rnn_forward_runs(orl_rnn* d, const char* what, const float* inputs, int64_t n, int32_t T, int on_device, int shared, int run, float* out_last,
                            float* out_all) {
  const std::string wh(what);
  if (!inputs || !out_last || n < 1) return fail(wh + ": bad arguments");
  if (run < -1 || run >= d->R) return fail(wh + ": run out of range (" + std::to_string(d->R) + " runs, or -1 for all)");
  if (T < 1 || T > d->Tmax) return fail(wh + ": need 1 <= T <= max_seq_len (" + std::to_string(d->Tmax) + ")");
  if (n > 0x7fffffffL / ((int64_t)T * 8 * d->H)) return fail(wh + ": too many sequences for one call");
  const RnnRuns rs{run < 0 ? 0 : run, run < 0 ? d->R : 1};
  const long N = (long)n * T;
  if (rnn_eval_windows(d, rs, inputs, n, T, on_device, shared)) return -1;
  RnnWs& w = d->ew;
  float* last = stage_dst(out_last, d->fLast, on_device);
  DEV_LAUNCH(d->stream, k_rnn_copy, dim3(ew_grid((long)n * d->od), rs.n), dim3(256), 0, (const float*)w.PRED.p, w.PRED.pitch, w.PRED.s0, last, d->od,
              (long)n * d->od, (long)n, d->od, (int)T);
  if (stage_out(d->stream, out_last, d->fLast, (size_t)rs.n * n * d->od, on_device)) return -1;
  if (out_all) {
    float* all = stage_dst(out_all, d->fAll, on_device);
    DEV_LAUNCH(d->stream, k_rnn_copy, dim3(ew_grid(N * d->od), rs.n), dim3(256), 0, (const float*)w.PRED.p, w.PRED.pitch, w.PRED.s0, all, d->od,
                N * d->od, N, d->od, 1);
    if (stage_out(d->stream, out_all, d->fAll, (size_t)rs.n * N * d->od, on_device)) return -1;
  }
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->last_ws = &w; d->last_rows = N; d->last_r0 = rs.r0; d->last_nr = rs.n; d->last_roll = false;
  return 0;
}
int orl_rnn_forward(orl_rnn* d, const float* inputs, int64_t n, int32_t T, int on_device, float* out_last, float* out_all) {
  if (rnn_ready(d, "orl_rnn_forward", false) || rnn_one_run_only(d, "orl_rnn_forward", "orl_rnn_forward_runs")) return -1;
  return rnn_forward_runs(d, "orl_rnn_forward", inputs, n, T, on_device, 1, 0, out_last, out_all);
}
int orl_rnn_forward_runs(orl_rnn* d, const float* inputs, int64_t n, int32_t T, int on_device, int shared_inputs, int run, float* out_last,
                         float* out_all) {
  if (rnn_ready(d, "orl_rnn_forward_runs", false)) return -1;
  return rnn_forward_runs(d, "orl_rnn_forward_runs", inputs, n, T, on_device, shared_inputs, run, out_last, out_all);
}

// ---- the carried state ----
// layer l of run r in state buffer s
static float* rnn_state_at(orl_rnn* d, int s, int run, int l) { return d->st[s] + (((long)run * d->L + l) * d->n_traj) * d->H; }
static int rnn_has_state(const orl_rnn* d, const char* what) {
  return d->st[0] ? 0 : fail(std::string(what) + ": no state yet (orl_rnn_state_reset)");
}

int orl_rnn_set_scaler(orl_rnn* d, const float* mu, const float* std_, int64_t n) {
  if (rnn_ready(d, "orl_rnn_set_scaler", false)) return -1;
  if (!mu || !std_) return fail("orl_rnn_set_scaler: bad arguments");
  if (n != d->in) return fail("orl_rnn_set_scaler: expected input_dim = " + std::to_string(d->in) + " floats each");
  for (int c = 0; c < d->in; ++c)
    if (!(std_[c] != 0.f) || !std::isfinite(std_[c]) || !std::isfinite(mu[c])) return fail("orl_rnn_set_scaler: mu must be finite, std finite and not 0");
  if (!d->sc_mu && (d->mem.alloc(&d->sc_mu, d->in) || d->mem.alloc(&d->sc_std, d->in))) return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  ORL_HIP(hipMemcpy(d->sc_mu, mu, sizeof(float) * d->in, hipMemcpyHostToDevice));
  ORL_HIP(hipMemcpy(d->sc_std, std_, sizeof(float) * d->in, hipMemcpyHostToDevice));
  d->has_scaler = true;
  return 0;
}

int orl_rnn_state_reset(orl_rnn* d, int64_t n_traj) {
  if (rnn_ready(d, "orl_rnn_state_reset", false)) return -1;
  if (n_traj < 1 || n_traj > 0x7fffffffL / ((int64_t)8 * d->H)) return fail("orl_rnn_state_reset: n_traj must be positive and index one step's matrices");
  ORL_HIP(hipStreamSynchronize(d->stream));
  const size_t per = (size_t)d->R * d->L * n_traj * d->H;
  if (n_traj != d->n_traj) {
    d->mem.release(&d->st[0], &d->st[1], &d->side);
    d->n_traj = 0;
    if (d->mem.alloc(&d->st[0], per) || d->mem.alloc(&d->st[1], per) || d->mem.alloc(&d->side, (size_t)d->R * n_traj)) return -1;   // (zero-filled)
    d->n_traj = n_traj;
    return 0;
  }
  ORL_HIP(hipMemsetAsync(d->st[0], 0, sizeof(float) * per, d->stream));
  ORL_HIP(hipMemsetAsync(d->st[1], 0, sizeof(float) * per, d->stream));
  ORL_HIP(hipMemsetAsync(d->side, 0, sizeof(int) * d->R * n_traj, d->stream));
  ORL_HIP(hipStreamSynchronize(d->stream));
  return 0;
}

int orl_rnn_state_set(orl_rnn* d, int run, int layer, const float* host, int64_t n_traj) {
  if (rnn_ready(d, "orl_rnn_state_set", false) || rnn_has_state(d, "orl_rnn_state_set") || rnn_run_ok(d, run, "orl_rnn_state_set")) return -1;
  if (!host) return fail("orl_rnn_state_set: bad arguments");
  if (layer < 0 || layer >= d->L) return fail("orl_rnn_state_set: layer out of range (" + std::to_string(d->L) + " GRU layers)");
  if (n_traj != d->n_traj) return fail("orl_rnn_state_set: the state has " + std::to_string(d->n_traj) + " trajectories");
  ORL_HIP(hipStreamSynchronize(d->stream));
  for (int s = 0; s < 2; ++s)                             // both buffers: whichever a slot's side bit names holds the planted row
    ORL_HIP(hipMemcpy(rnn_state_at(d, s, run, layer), host, sizeof(float) * n_traj * d->H, hipMemcpyHostToDevice));
  return 0;
}

int orl_rnn_state_prime(orl_rnn* d, const float* inputs, int64_t n, int32_t T, int on_device, int shared_inputs) {
  if (rnn_ready(d, "orl_rnn_state_prime", false) || rnn_has_state(d, "orl_rnn_state_prime")) return -1;
  if (!inputs || n < 1) return fail("orl_rnn_state_prime: bad arguments");
  if (n > d->n_traj) return fail("orl_rnn_state_prime: " + std::to_string(n) + " windows for a state of " + std::to_string(d->n_traj) + " trajectories");
  if (T < 1 || T > d->Tmax) return fail("orl_rnn_state_prime: need 1 <= T <= max_seq_len (" + std::to_string(d->Tmax) + ")");
  if (n > 0x7fffffffL / ((int64_t)T * 8 * d->H)) return fail("orl_rnn_state_prime: too many sequences for one call");
  const RnnRuns rs{0, d->R};
  if (rnn_eval_windows(d, rs, inputs, n, T, on_device, shared_inputs)) return -1;
  const RnnWs& w = d->ew;
  const long st_rs = (long)d->L * d->n_traj * d->H;
  for (int l = 0; l < d->L; ++l)
    for (int s = 0; s < 2; ++s)                           // slots 0 .. n - 1 of both buffers <- row b T + T - 1 of the layer's h
      DEV_LAUNCH(d->stream, k_rnn_copy, dim3(ew_grid((long)n * d->H), rs.n), dim3(256), 0, (const float*)w.HO[l].p, w.HO[l].pitch, w.HO[l].s0,
                 rnn_state_at(d, s, 0, l), d->H, st_rs, (long)n, d->H, (int)T);
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->last_ws = &w; d->last_rows = (long)n * T; d->last_r0 = 0; d->last_nr = rs.n; d->last_roll = false;
  return 0;
}

int orl_rnn_state_step(orl_rnn* d, const float* obs, const float* act, const int64_t* index, int64_t n, int on_device, int run, float* next_obs,
                       float* reward) {
  if (rnn_ready(d, "orl_rnn_state_step", false) || rnn_has_state(d, "orl_rnn_state_step")) return -1;
  const int odim = d->od - 1, adim = d->in - odim;        // the model predicts [delta obs | reward] from [obs | act]
  if (adim < 1)
    return fail("orl_rnn_state_step: output_dim " + std::to_string(d->od) + " means obs_dim " + std::to_string(odim) + ", which leaves act_dim = input_dim - obs_dim = " +
                std::to_string(adim) + " < 1");
  if (odim < 1) return fail("orl_rnn_state_step: output_dim must be obs_dim + 1 with obs_dim >= 1");
  if (!d->has_scaler) return fail("orl_rnn_state_step: no input scaler (orl_rnn_set_scaler)");
  if (!obs || !act || !next_obs || !reward || n < 1) return fail("orl_rnn_state_step: bad arguments");
  if (run < -1 || run >= d->R) return fail("orl_rnn_state_step: run out of range (" + std::to_string(d->R) + " runs, or -1 for all)");
  if (n > d->n_traj) return fail("orl_rnn_state_step: " + std::to_string(n) + " rows for a state of " + std::to_string(d->n_traj) + " trajectories");
  const RnnRuns rs{run < 0 ? 0 : run, run < 0 ? d->R : 1};
  const int H = d->H;
  if (rnn_eval_ws(d, n, rs.n)) return -1;
  const long long* idx_d = nullptr;
  if (index && on_device) idx_d = (const long long*)index;      // (the kernels clamp what they read)
  else if (index) {
    std::vector<char> seen((size_t)d->n_traj, 0);
    for (int64_t i = 0; i < n; ++i) {
      if (index[i] < 0 || index[i] >= d->n_traj)
        return fail("orl_rnn_state_step: trajectory index out of range (" + std::to_string(d->n_traj) + " trajectories)");
      if (seen[index[i]]) return fail("orl_rnn_state_step: trajectory index " + std::to_string(index[i]) + " twice in one step");
      seen[index[i]] = 1;
    }
    if (d->mem.grow(&d->r_idx, &d->r_idx_cap, d->n_traj, d->stream)) return -1;
    ORL_HIP(hipMemcpyAsync(d->r_idx, index, sizeof(int64_t) * n, hipMemcpyHostToDevice, d->stream));
    idx_d = d->r_idx;
  }
  // host arrays: obs | act | next_obs | reward of the step's runs, staged
  const size_t no = (size_t)rs.n * n * odim, na = (size_t)rs.n * n * adim, nr = (size_t)rs.n * n;
  if (!on_device && d->mem.grow(&d->r_stage, &d->r_stage_cap, (long)(2 * no + na + nr), d->stream)) return -1;
  const float *obs_d = obs, *act_d = act;
  if (stage_in(d->stream, obs_d, d->r_stage, no, on_device) || stage_in(d->stream, act_d, d->r_stage + no, na, on_device)) return -1;
  float* next_d = stage_dst(next_obs, d->r_stage + no + na, on_device);
  float* rew_d = stage_dst(reward, d->r_stage + 2 * no + na, on_device);
  RnnWs& w = d->ew;
  DEV_LAUNCH(d->stream, k_rnn_roll_in, dim3(ew_grid(n * d->in), rs.n), dim3(256), 0, obs_d, (long)n * odim, act_d, (long)n * adim, odim, adim,
             (const float*)d->sc_mu, (const float*)d->sc_std, (long)n, w.X0.p, w.X0.pitch, w.X0.s0);
  float* params = rnn_params_of(d, rs);
  DevMat X = w.X0;
  for (int l = 0; l < d->L; ++l) {
    RnnCellP cp;
    memset(&cp, 0, sizeof(cp));
    cp.n = (int)n; cp.H = H; cp.K = l ? H : d->in;
    cp.x = X.p; cp.xp = X.pitch; cp.x_rs = X.s0;
    cp.wih = params + d->wih[l].w; cp.whh = params + d->whh[l].w; cp.bih = params + d->wih[l].b; cp.bhh = params + d->whh[l].b; cp.par_rs = d->P;
    cp.idx = idx_d;
    cp.st[0] = rnn_state_at(d, 0, rs.r0, l); cp.st[1] = rnn_state_at(d, 1, rs.r0, l); cp.st_rs = (long)d->L * d->n_traj * H;
    cp.side = d->side + (long)rs.r0 * d->n_traj; cp.n_traj = d->n_traj;
    cp.ho = w.HO[l].p; cp.hop = w.HO[l].pitch; cp.ho_rs = w.HO[l].s0;
    DEV_LAUNCH(d->stream, k_rnn_cell, dim3((unsigned)((n + RNN_RB - 1) / RNN_RB), (H + 15) / 16, rs.n), dim3(64), 0, cp);
    X = w.HO[l];
  }
  if (rnn_tail(d, rs, w, w.X0, (long)n, false)) return -1;
  DEV_LAUNCH(d->stream, k_rnn_roll_head, dim3(ew_grid(n * d->od), rs.n), dim3(256), 0, (const float*)w.PRED.p, w.PRED.pitch, w.PRED.s0, obs_d,
             (long)n * odim, d->od, (long)n, next_d, rew_d, idx_d, d->side + (long)rs.r0 * d->n_traj, d->n_traj);
  if (stage_out(d->stream, next_obs, d->r_stage + no + na, no, on_device) || stage_out(d->stream, reward, d->r_stage + 2 * no + na, nr, on_device))
    return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  d->last_ws = &w; d->last_rows = (long)n; d->last_r0 = rs.r0; d->last_nr = rs.n; d->last_roll = true;
  return 0;
}

// "<prefix><k>" with 0 <= k < count; -1 otherwise
static int rnn_tap_index(const std::string& nm, const char* prefix, int count) {
  const size_t n = strlen(prefix);
  if (nm.compare(0, n, prefix) != 0) return -1;
  const std::string num = nm.substr(n);
  if (num.size() != 1 || num[0] < '0' || num[0] > '9') return -1;
  const int k = num[0] - '0';
  return k < count ? k : -1;
}

int64_t orl_rnn_debug_read_run(orl_rnn* d, int run, const char* name, float* host, int64_t cap) {
  if (!d || !name || !host) return fail("orl_rnn_debug_read: bad arguments");
  if (rnn_run_ok(d, run, "orl_rnn_debug_read")) return -1;
  const std::string nm(name);
  int k;
  if ((k = rnn_tap_index(nm, "state.", d->L)) >= 0) {         // the carried h of every slot: each from the buffer its side bit names
    if (rnn_has_state(d, "orl_rnn_debug_read")) return -1;
    const long n = d->n_traj * d->H;
    if (n > cap) return fail("orl_rnn_debug_read: " + nm + " needs " + std::to_string(n) + " floats");
    ORL_HIP(hipStreamSynchronize(d->stream));
    std::vector<float> other((size_t)n);
    std::vector<int> side((size_t)d->n_traj);
    ORL_HIP(hipMemcpy(host, rnn_state_at(d, 0, run, k), sizeof(float) * n, hipMemcpyDeviceToHost));
    ORL_HIP(hipMemcpy(other.data(), rnn_state_at(d, 1, run, k), sizeof(float) * n, hipMemcpyDeviceToHost));
    ORL_HIP(hipMemcpy(side.data(), d->side + (long)run * d->n_traj, sizeof(int) * d->n_traj, hipMemcpyDeviceToHost));
    for (long t = 0; t < d->n_traj; ++t)
      if (side[t] & 1) memcpy(host + t * d->H, other.data() + t * d->H, sizeof(float) * d->H);
    return n;
  }
  const RnnWs* w = d->last_ws ? d->last_ws : &d->tw;          // (names are resolved before "nothing recorded": an unknown one is always refused)
  const float* src = nullptr; long rows = d->last_rows, rs = 0; int cols = d->H, pitch = d->H;
  bool roll = false;                                          // a name of the one-step path
  const bool rolled = d->last_ws && d->last_roll;             // ... which the last pass was
  auto mat = [&](const DevMat& m) { src = m.p; pitch = m.pitch; rs = m.s0; };
  if (nm == "loss") { src = d->loss_cell + run; rows = 1; cols = 1; pitch = 1; }
  else if (nm == "pred") { mat(w->PRED); cols = d->od; }
  else if (nm == "in") mat(w->CAT);
  else if (nm == "merge") mat(w->M0);
  else if ((k = rnn_tap_index(nm, "gru.", d->L)) >= 0) mat(w->HO[k]);
  else if ((k = rnn_tap_index(nm, "block.", d->nb)) >= 0) mat(w->XO[k]);
  else if ((k = rnn_tap_index(nm, "act.", d->norms)) >= 0) mat(k ? w->SB[k - 1] : w->SI);
  else if ((k = rnn_tap_index(nm, "drop.", d->norms)) >= 0) mat(k ? w->UB[k - 1] : w->UI);
  else if ((k = rnn_tap_index(nm, "mask.", d->norms)) >= 0) {
    if (!w->train || !(d->c.dropout_rate > 0.f)) return fail("orl_rnn_debug_read: no dropout mask was applied");
    src = w->MK + (size_t)k * w->cap * d->H; rs = w->mk_rs;
  }
  else if ((k = rnn_tap_index(nm, "gi.", d->L)) >= 0) {
    if (rolled) return fail("orl_rnn_debug_read: a state step keeps no input projections (" + nm + "): k_rnn_cell forms them in registers");
    mat(w->GI[k]); cols = 3 * d->H;
  }
  else if (nm == "x0") { mat(w->X0); cols = d->in; }
  else if (nm == "roll.x") { roll = true; cols = d->in; if (rolled) mat(w->X0); }
  else if (nm == "roll.pred") { roll = true; cols = d->od; if (rolled) mat(w->PRED); }
  else if ((k = rnn_tap_index(nm, "roll.h.", d->L)) >= 0) { roll = true; if (rolled) mat(w->HO[k]); }
  else {
    // what only a training step computes.  st: the stage's index when the matrix is one of a shared buffer's stages, last: the stage
    // that writes the shared buffer last (the one still readable without orl_rnn_debug_keep)
    int st = -1, last = 0;
    const int H = d->H, L = d->L, nb = d->nb;
    const long pn = (long)d->norms * 2 * H;
    bool tr = true;
    if (nm == "tgt") { src = d->TGT; rs = w->cap * d->od; cols = pitch = d->od; }
    else if (nm == "msk") { src = d->MSK; rs = w->cap; cols = pitch = 1; }
    else if ((k = rnn_tap_index(nm, "r.", L)) >= 0) { if (w->train) mat(w->R[k]); }
    else if ((k = rnn_tap_index(nm, "z.", L)) >= 0) { if (w->train) mat(w->Z[k]); }
    else if ((k = rnn_tap_index(nm, "n.", L)) >= 0) { if (w->train) mat(w->NN[k]); }
    else if ((k = rnn_tap_index(nm, "hn.", L)) >= 0) { if (w->train) mat(w->HN[k]); }
    else if ((k = rnn_tap_index(nm, "hp.", L)) >= 0) { if (w->train) mat(w->HP[k]); }
    else if ((k = rnn_tap_index(nm, "zpre.", d->norms)) >= 0) mat(k ? w->ZB[k - 1] : w->ZI);
    else if (nm == "zmerge") mat(w->ZM);
    else if (nm == "dpred") { mat(w->dPRED); cols = d->od; }
    else if (nm == "dx") mat(w->dX);
    else if (nm == "dzm") mat(w->dZM);
    else if (nm == "dcat") { mat(w->dCAT); cols = 2 * H; }
    else if ((k = rnn_tap_index(nm, "du.", nb)) >= 0) { if (w->train) mat(w->DUb[k]); st = k; }
    else if ((k = rnn_tap_index(nm, "dt.", nb)) >= 0) { if (w->train) mat(w->DTb[k]); st = k; }
    else if ((k = rnn_tap_index(nm, "dz.", d->norms)) >= 0) { if (w->train) mat(w->DZs[k]); st = k; }
    else if ((k = rnn_tap_index(nm, "dgi.", L)) >= 0) { if (w->train) mat(w->dGIl[k]); cols = 3 * H; st = k; }
    else if ((k = rnn_tap_index(nm, "dgh.", L)) >= 0) { if (w->train) mat(w->dGHl[k]); cols = 3 * H; st = k; }
    else if ((k = rnn_tap_index(nm, "dxl.", L)) >= 1) { if (w->train) mat(w->dXLl[k]); st = k; last = k < 3 ? k : k - 2; }   // (layer 1 reuses layer 3's)
    else if (nm == "part") { src = w->part; rs = w->part_rs; cols = pitch = (int)pn; }
    else if (nm == "chunk") { src = w->chunk; rs = w->chunk_rs; cols = pitch = (int)pn; rows = (rows + RNN_CHUNK - 1) / RNN_CHUNK; }
    else if ((k = rnn_tap_index(nm, "slab.", 8)) >= 0) {
      if (d->last_ws && w->train && k >= rnn_slabs(d, d->last_rows))
        return fail("orl_rnn_debug_read: the last step wrote " + std::to_string(rnn_slabs(d, d->last_rows)) + " slabs, " + nm + " is none of them");
      src = d->slabs + (long)k * d->R * d->P; rs = d->P; rows = d->last_ws ? 1 : 0; cols = pitch = (int)d->P;
    }
    else tr = false;
    if (!tr) return fail("orl_rnn_debug_read: unknown tap " + nm);
    if (d->last_ws && !w->train) return fail("orl_rnn_debug_read: only a training step computes " + nm + " (the last pass was a forward)");
    if (d->last_ws && !w->keep && st >= 0 && st != last)
      return fail("orl_rnn_debug_read: a later stage of the step has overwritten " + nm + " (orl_rnn_debug_keep keeps every stage's)");
  }
  if (roll && !rolled) return fail("orl_rnn_debug_read: nothing recorded for " + nm + " (the last pass was no state step)");
  if (!src || rows < 1 || (!d->last_ws && nm != "loss")) return fail("orl_rnn_debug_read: nothing recorded for " + nm);
  if (nm != "loss") {                                         // the run's slot in the workspace of the last pass
    if (run < d->last_r0 || run >= d->last_r0 + d->last_nr) return fail("orl_rnn_debug_read: the last pass did not compute run " + std::to_string(run));
    src += (long)(run - d->last_r0) * rs;
  }
  if ((int64_t)rows * cols > cap) return fail("orl_rnn_debug_read: " + nm + " needs " + std::to_string(rows * cols) + " floats");
  ORL_HIP(hipStreamSynchronize(d->stream));
  ORL_HIP(hipMemcpy2D(host, sizeof(float) * cols, src, sizeof(float) * pitch, sizeof(float) * cols, rows, hipMemcpyDeviceToHost));
  return (int64_t)rows * cols;
}
int64_t orl_rnn_debug_read(orl_rnn* d, const char* name, float* host, int64_t cap) {
  if (!d || !name || !host) return fail("orl_rnn_debug_read: bad arguments");
  if (rnn_one_run_only(d, "orl_rnn_debug_read", "orl_rnn_debug_read_run")) return -1;
  return orl_rnn_debug_read_run(d, 0, name, host, cap);
}
int orl_rnn_debug_keep(orl_rnn* d, int on) {
  if (rnn_ready(d, "orl_rnn_debug_keep", false)) return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  if ((on != 0) == d->tw.keep) return 0;
  if (d->last_ws == &d->tw) d->last_ws = nullptr;          // the stages of the last step are not where the views point any more
  return rnn_ws_stages(d, d->tw, on != 0);
}
int orl_rnn_profile(orl_rnn* d, int enable) {
  if (rnn_ready(d, "orl_rnn_profile", false)) return -1;
  ORL_HIP(hipStreamSynchronize(d->stream));
  if (enable)
    for (hipEvent_t& e : d->ev)
      if (!e) ORL_HIP(hipEventCreate(&e));
  d->prof = enable != 0;
  d->prof_valid = false;
  return 0;
}
int orl_rnn_profile_read(orl_rnn* d, float ms[6]) {
  if (!d || !ms) return fail("orl_rnn_profile_read: bad arguments");
  if (!d->prof_valid) return fail("orl_rnn_profile_read: no timed step (orl_rnn_profile, then a step)");
  ORL_HIP(hipStreamSynchronize(d->stream));
  ORL_HIP(hipEventElapsedTime(&ms[0], d->ev[0], d->ev[3]));
  ORL_HIP(hipEventElapsedTime(&ms[1], d->ev[0], d->ev[1]));
  ORL_HIP(hipEventElapsedTime(&ms[3], d->ev[1], d->ev[2]));
  ORL_HIP(hipEventElapsedTime(&ms[5], d->ev[2], d->ev[3]));
  ms[2] = ms[4] = 0.f;
  for (int l = 0; l < d->L; ++l) {
    float f = 0.f, b = 0.f;
    ORL_HIP(hipEventElapsedTime(&f, d->ev[4 + 4 * l], d->ev[5 + 4 * l]));
    ORL_HIP(hipEventElapsedTime(&b, d->ev[6 + 4 * l], d->ev[7 + 4 * l]));
    ms[2] += f; ms[4] += b;
  }
  return 0;
}
int orl_rnn_debug_grads_run(orl_rnn* d, int run, float* host, int64_t n) {
  if (!d || !host || n != d->P) return fail("orl_rnn_debug_grads: bad arguments");
  if (rnn_run_ok(d, run, "orl_rnn_debug_grads")) return -1;
  return block_to_host(d->stream, host, d->grads + (long)run * d->P, d->P);
}
int orl_rnn_debug_grads(orl_rnn* d, float* host, int64_t n) {
  if (!d || !host || n != d->P) return fail("orl_rnn_debug_grads: bad arguments");
  if (rnn_one_run_only(d, "orl_rnn_debug_grads", "orl_rnn_debug_grads_run")) return -1;
  return orl_rnn_debug_grads_run(d, 0, host, n);
}

}  // extern "C"
