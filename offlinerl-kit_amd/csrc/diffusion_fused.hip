// diffusion_fused.hip — DiffusionBC's sampler at sample precision 1: Linear + GroupNorm + Mish + tail in one launch on
// v_mfma_f32_16x16x32_f16 with split operands (x = hi + lo fp16 planes, products hi*hi + hi*lo + lo*hi, fp32 accumulators).
//
// Work split.  A workgroup (4 waves) owns 16 MA rows and one column slab of at most 64 NFW columns.  A norm slab is `gps` WHOLE
// GroupNorm groups (gps cg <= 64 NFW), so a (row, group) never leaves its workgroup: no second pass, no atomics.  The slabs after
// the norm ones are plain 64 NFW-column slabs with a bias(-and-Mish) epilogue: the Wr half of a stacked [W0; Wr], or a Linear without a
// norm.  Wave w multiplies the slab's columns [16 NFW w, 16 NFW (w + 1)).
// Operands.  The weights arrive pre-split (dfu_split_weights: [N][Kp] planes of w ORL_WSCALE, k-contiguous, the K tail zero), so a
// lane's B fragment -- 8 consecutive k of one output column -- is one 16-byte global load per plane; no wave shares a B fragment with
// another, so B does not pass through LDS.  The loads of chunk k + 1 (B fragments and raw A pieces) are issued into registers before
// the MFMAs of chunk k.  The activations are fp32 in HBM, read as one or
// two column ranges ([x | skip] without a copy), optionally through Mish, split once per 64-deep K chunk into LDS planes that the
// four waves share; rows past `rows` and the K tail are zero-filled there and nothing past a row's K floats is read.
// Epilogue.  The MFMAs are issued with the operands swapped (gemm_kernel.h), so lane (li, lq) holds four consecutive columns
// 4 lq .. 4 lq + 3 of row li.  accumulators / ORL_WSCALE + bias go to an LDS tile; 16 lanes per row then take the groups of the slab
// one after the other: mean, the centred second moment (two passes over LDS, sums across the 16 lanes by __shfl_xor), affine, Mish,
// FiLM or residual tail, fp32 store.  The pre-norm matrix never reaches HBM.
#include "diffusion_fused.h"

namespace orl {

enum { DFU_KC = 64, DFU_AP = DFU_KC + 8 };       // K chunk; pitch of an LDS A-plane row in halves (144 B: 16-byte aligned fragments)

__device__ __forceinline__ float dfu_at(const DfuCols& m, long row, int k) {
  return k < m.k0 ? m.p0[row * m.s0 + k] : m.p1[row * m.s1 + (k - m.k0)];
}
// elements k .. k + 3 of a row (k + 4 <= K): one 16-byte load where they lie in one range at an aligned address
__device__ __forceinline__ f32x4 dfu_load4(const DfuCols& m, long row, int k) {
  const float* q = nullptr;
  if (k + 4 <= m.k0) q = m.p0 + row * m.s0 + k;
  else if (k >= m.k0) q = m.p1 + row * m.s1 + (k - m.k0);
  if (q && (((uintptr_t)q) & 15) == 0) return *(const f32x4*)q;
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = dfu_at(m, row, k + j);
  return v;
}

template <int MA, int NFW>
__global__ __launch_bounds__(256) void k_diff_fused(DfuP p) {
  constexpr int RT = 16 * MA, SW = 64 * NFW, CP = SW + 16;
  __shared__ __attribute__((aligned(16))) hx_t sA[2][RT][DFU_AP];
  __shared__ __attribute__((aligned(16))) float sC[RT][CP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const long row0 = (long)blockIdx.x * RT;
  const int slab = blockIdx.y;
  const bool norm = slab < p.norm_slabs;
  int c0, ncols;
  if (norm) { c0 = slab * p.gps * p.cg; ncols = min(p.gps * p.cg, p.Cn - c0); }
  else { c0 = p.Cn + (slab - p.norm_slabs) * SW; ncols = min(SW, p.N - c0); }
  const int wcol = wave * 16 * NFW;
  const bool wave_on = wcol < ncols;                       // (uniform per wave) this wave's columns exist

  f32x4 acc[MA][NFW];
#pragma unroll
  for (int a = 0; a < MA; ++a)
#pragma unroll
    for (int b = 0; b < NFW; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // this lane's B rows (output columns), clamped into the matrix: a clamped column's products are discarded by the epilogue
  long boff[NFW];
#pragma unroll
  for (int b = 0; b < NFW; ++b) boff[b] = (long)min(c0 + wcol + b * 16 + li, p.N - 1) * p.Kp + 8 * lq;
  unsigned int bad = 0;

  // the next chunk's operands travel in registers while the current one is multiplied: B fragments (this wave's own), A pieces (raw
  // fp32: Mish, the range check and the split wait until the piece is stored to LDS)
  hx8 nbh[2][NFW], nbl[2][NFW];
  f32x4 nv[MA];
  auto fetch = [&](int kc) {
    if (wave_on) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int b = 0; b < NFW; ++b)
          if (s == 0 || kc + 32 < p.Kp) {                  // Kp is a multiple of 32: a chunk holds one or two k-steps
            nbh[s][b] = *(const hx8*)(p.Bh + boff[b] + kc + 32 * s);
            nbl[s][b] = *(const hx8*)(p.Bl + boff[b] + kc + 32 * s);
          }
    }
#pragma unroll
    for (int i = 0; i < MA; ++i) {                         // RT rows x 64 k as 4-k pieces, MA pieces per thread
      const int e = tid + 256 * i, r = e >> 4, k = kc + (e & 15) * 4;
      const long row = row0 + r;
      nv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (row < p.rows) {
        if (k + 4 <= p.K) nv[i] = dfu_load4(p.A, row, k);
        else
#pragma unroll
          for (int j = 0; j < 4; ++j) if (k + j < p.K) nv[i][j] = dfu_at(p.A, row, k + j);
      }
    }
  };
  fetch(0);
  for (int kc = 0; kc < p.Kp; kc += DFU_KC) {
    const bool two = kc + 32 < p.Kp;
    hx8 fbh[2][NFW], fbl[2][NFW];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int b = 0; b < NFW; ++b) { fbh[s][b] = nbh[s][b]; fbl[s][b] = nbl[s][b]; }
#pragma unroll
    for (int i = 0; i < MA; ++i) {
      const int e = tid + 256 * i, r = e >> 4, kq = (e & 15) * 4;
      f32x4 v = nv[i];
      if (p.a_mish)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = diff_mish(v[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) bad |= !(fabsf(v[j]) < 32768.f);         // (a NaN fails the comparison too; the zero fill passes)
      hx4 h, l;
      orl_split4(v, h, l);
      *(hx4*)&sA[0][r][kq] = h;
      *(hx4*)&sA[1][r][kq] = l;
    }
    __syncthreads();
    if (kc + DFU_KC < p.Kp) fetch(kc + DFU_KC);
    if (wave_on) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s == 1 && !two) break;
        hx8 fah[MA], fal[MA];
#pragma unroll
        for (int a = 0; a < MA; ++a) {
          fah[a] = *(const hx8*)&sA[0][a * 16 + li][32 * s + 8 * lq];
          fal[a] = *(const hx8*)&sA[1][a * 16 + li][32 * s + 8 * lq];
        }
#pragma unroll
        for (int a = 0; a < MA; ++a)
#pragma unroll
          for (int b = 0; b < NFW; ++b) {
            acc[a][b] = ORL_MFMA_16x16x32(fbl[s][b], fah[a], acc[a][b]);
            acc[a][b] = ORL_MFMA_16x16x32(fbh[s][b], fal[a], acc[a][b]);
            acc[a][b] = ORL_MFMA_16x16x32(fbh[s][b], fah[a], acc[a][b]);
          }
      }
    }
    __syncthreads();
  }
  if (bad) p.flags[DFU_FLAG_ACT] = 1u;

  // accumulators / ORL_WSCALE (exact) + bias into the LDS tile; columns past the slab hold 0
  constexpr float inv = 1.0f / ORL_WSCALE;
#pragma unroll
  for (int a = 0; a < MA; ++a)
#pragma unroll
    for (int b = 0; b < NFW; ++b) {
      const int c = wcol + b * 16 + 4 * lq;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (c + j < ncols) ? acc[a][b][j] * inv + p.bias[c0 + c + j] : 0.f;
      *(f32x4*)&sC[a * 16 + li][c] = v;
    }
  __syncthreads();

  const int j16 = tid & 15;
  if (!norm) {
#pragma unroll
    for (int a = 0; a < MA; ++a) {
      const int r = a * 16 + (tid >> 4);
      const long row = row0 + r;
      if (row >= p.rows) continue;
      for (int c = j16; c < ncols; c += 16) {
        const float v = sC[r][c];
        p.out2[row * p.o2p + (c0 - p.Cn) + c] = p.plain_mish ? diff_mish(v) : v;
      }
    }
    return;
  }
  const int ng = ncols / p.cg;
  const float rn = 1.f / (float)p.cg;
#pragma unroll
  for (int a = 0; a < MA; ++a) {
    const int r = a * 16 + (tid >> 4);
    const long row = row0 + r;
    for (int g = 0; g < ng; ++g) {                         // (uniform trip counts: every lane takes part in the shuffles)
      const float* x = &sC[r][g * p.cg];
      float s = 0.f;
      for (int c = j16; c < p.cg; c += 16) s += x[c];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
      const float mean = s * rn;
      float q = 0.f;
      for (int c = j16; c < p.cg; c += 16) { const float dlt = x[c] - mean; q += dlt * dlt; }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) q += __shfl_xor(q, o, 16);
      const float rstd = 1.f / sqrtf(q * rn + 1e-5f);
      if (row >= p.rows) continue;
      for (int c = j16; c < p.cg; c += 16) {
        const int ch = c0 + g * p.cg + c;
        float m = diff_mish((x[c] - mean) * rstd * p.gamma[ch] + p.beta[ch]);
        if (p.film) m = p.film[row * p.fp + ch] * m + p.film[row * p.fp + p.Cn + ch];
        if (p.res.p0) m += dfu_at(p.res, row, ch);
        p.out[row * p.op + ch] = m;
      }
    }
  }
}

// one thread per 4 k of a plane row
__global__ __launch_bounds__(256) void k_diff_split_weights(const float* __restrict__ W, int N, int K, int Kp, hx_t* __restrict__ Bh,
                                                            hx_t* __restrict__ Bl, unsigned int* flags) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = Kp >> 2;
  if (e >= (long)N * q) return;
  const long n = e / q;
  const int k = (int)(e - n * q) * 4;
  f32x4 v;
  unsigned int bad = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = k + j < K ? W[n * K + k + j] * ORL_WSCALE : 0.f;
    bad |= !(fabsf(v[j]) < 65504.f);
  }
  hx4 h, l;
  orl_split4(v, h, l);
  *(hx4*)(Bh + n * Kp + k) = h;
  *(hx4*)(Bl + n * Kp + k) = l;
  if (bad) flags[DFU_FLAG_W] = 1u;
}

__global__ void k_diff_clear_flag(unsigned int* flags, int which) { flags[which] = 0u; }

static int dfu_slabs(int nfw, int N, int Cn, int cg) {
  const int sw = 64 * nfw;
  const int groups = Cn ? Cn / cg : 0, gps = Cn ? sw / cg : 1;
  return (groups + gps - 1) / gps + (N - Cn + sw - 1) / sw;
}

// The largest tile that still gives every CU of the MI355X a workgroup; else the smallest one.  A group wider than 64 channels needs
// the 128-column slab.
DfuTile dfu_pick_tile(int rows, int N, int Cn, int cg) {
  const int nfw_min = (Cn && cg > 64) ? 2 : 1;
  const DfuTile order[4] = {{2, 2}, {2, 1}, {1, 2}, {1, 1}};
  for (const DfuTile& t : order) {
    if (t.nfw < nfw_min || (t.ma == 2 && rows <= 16)) continue;
    if ((long)((rows + 16 * t.ma - 1) / (16 * t.ma)) * dfu_slabs(t.nfw, N, Cn, cg) >= 256) return t;
  }
  return {1, nfw_min};
}

hipError_t dfu_launch(DfuP p, hipStream_t st) {
  if (p.rows < 1 || p.N < 1 || p.K < 1 || (p.Kp & 31) || p.Kp < p.K || (p.Cn && (p.cg < 1 || p.cg > ORL_DIFF_FUSED_MAX_GROUP || p.Cn % p.cg)))
    return hipErrorInvalidValue;
  if (!p.A.p1) p.A.k0 = p.K;
  if (p.res.p0 && !p.res.p1) p.res.k0 = p.Cn;
  const DfuTile t = dfu_pick_tile(p.rows, p.N, p.Cn, p.cg);
  const int sw = 64 * t.nfw;
  p.gps = p.Cn ? sw / p.cg : 1;
  p.norm_slabs = p.Cn ? (p.Cn / p.cg + p.gps - 1) / p.gps : 0;
  const dim3 grid((unsigned)((p.rows + 16 * t.ma - 1) / (16 * t.ma)), (unsigned)dfu_slabs(t.nfw, p.N, p.Cn, p.cg));
  if (t.ma == 2 && t.nfw == 2) hipLaunchKernelGGL((k_diff_fused<2, 2>), grid, dim3(256), 0, st, p);
  else if (t.ma == 2) hipLaunchKernelGGL((k_diff_fused<2, 1>), grid, dim3(256), 0, st, p);
  else if (t.nfw == 2) hipLaunchKernelGGL((k_diff_fused<1, 2>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((k_diff_fused<1, 1>), grid, dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t dfu_split_weights(const float* W, int N, int K, int Kp, hx_t* Bh, hx_t* Bl, unsigned int* flags, hipStream_t st) {
  const long n = (long)N * (Kp >> 2);
  hipLaunchKernelGGL(k_diff_split_weights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, N, K, Kp, Bh, Bl, flags);
  return hipGetLastError();
}

hipError_t dfu_clear_flag(unsigned int* flags, int which, hipStream_t st) {
  hipLaunchKernelGGL(k_diff_clear_flag, dim3(1), dim3(1), 0, st, flags, which);
  return hipGetLastError();
}

}  // namespace orl
