// autoreg_fused.hip — the autoregressive behaviour policy's sampling at sample precision 1: all act_dim passes and all layers of every
// pass of one row tile in one launch on v_mfma_f32_16x16x32_f16 with split operands (x = hi + lo fp16 planes, products lo*hi + hi*lo +
// hi*hi, fp32 accumulators).
//
// Work split.  Grid (row tiles, R runs).  A workgroup (4 waves) owns RT = 16 / 32 / 64 rows of one run through the A passes; rows are
// independent, so __syncthreads() is the only synchronisation.  Per layer the 16-column fragments of the output are dealt to the waves
// as in k_dyn_fused_fwd (dyf_wave_frags); a wave holds RT / 16 x NF accumulators (NF = 4 up to 256 columns; 8 up to 512, on 16-row
// tiles only) over the layer's whole K.  The activations live in LDS as two fp16 planes [2][RT][Wp + 8], the weights arrive pre-split
// (k_autoreg_pack_planes: [R][layer][out][Kp] planes of w ORL_WSCALE, nn.Linear's [out][in] rows are k-contiguous already), a lane's B
// fragment is one 16-byte global load per plane, fetched into registers one k-step ahead -- across layers and passes too.
// Layer 0.  The input of pass j is [obs | a_<j, 0 | onehot_j], so z0_j = W0[:, :od] obs + b0 + sum_{i<j} a_i W0[:, od + i] + W0[:, od + A + j].
// base = W0[:, :od] obs + b0 is computed ONCE per tile with split MFMAs (only the observation columns of W0 are packed; obs is split into
// the planes as it is loaded) and stays in registers in the accumulator layout, in fp32, for the whole kernel.  Before pass j > 0 every
// lane adds a_{j-1} W0[:, od + j - 1] to its elements (fp32 FMAs; the column straight from the parameter block, a_{j-1} from a small fp32
// LDS array [RT][A]); z0 = base + W0[:, od + A + j], LeakyReLU, split into the planes.  Passes after the first issue no MFMA for layer 0.
// Tail and draw.  The tail's 2 columns are one fragment on wave 0; the MFMAs are issued with the operands swapped (gemm_kernel.h), so its
// lanes lq = 0 hold (mean, logstd) of row li: they apply the output LeakyReLU, read eps[run][row][j], form a_j = mean + e^logstd eps
// (k_autoreg_draw's formula) and store it to the LDS array and to act[run][row][j].  One barrier, then the next pass.  Rows past n are
// zero throughout and store nothing.
#include "autoreg_fused.h"

namespace orl {

__device__ __forceinline__ float arf_leaky(float v) { return v > 0.f ? v : ORL_LEAKY_SLOPE * v; }

template <int RT, int NF>
__global__ __launch_bounds__(256) void k_autoreg_fused_sample(ArfP q) {
  constexpr int MA = RT / 16;
  const DyfP& p = q.g;
  extern __shared__ __attribute__((aligned(16))) hx_t arf_lds[];
  const int AP = p.Wp + 8, A = q.A, od = p.width[0], H0 = p.width[1];
  hx_t* const sH = arf_lds;
  hx_t* const sL = arf_lds + RT * AP;
  float* const sA = (float*)(arf_lds + 2 * RT * AP);         // [RT][A] the tile's actions so far
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const long row0 = (long)blockIdx.x * RT;
  const int r = blockIdx.y;
  const hx_t* const Bh = p.Bh + (long)r * p.pmember;
  const hx_t* const Bl = p.Bl + (long)r * p.pmember;
  const float* const par = p.params + (long)r * p.P;
  const float* const W0 = par + p.w_off[0];
  unsigned int bad = 0;

  // the next k-step's B fragments (this wave's own) travel in registers while the current one is multiplied; a column past the layer
  // is clamped into it: its products are discarded by the epilogue
  hx8 nbh[NF], nbl[NF];
  auto fetch = [&](int l, int ks) {
    const int N = p.width[l + 1];
    int f0, cnt;
    dyf_wave_frags(N, wave, f0, cnt);
#pragma unroll
    for (int b = 0; b < NF; ++b)
      if (b < cnt) {
        const long off = p.poff[l] + (long)min((f0 + b) * 16 + li, N - 1) * p.Kp[l] + ks * 32 + 8 * lq;
        nbh[b] = *(const hx8*)(Bh + off);
        nbl[b] = *(const hx8*)(Bl + off);
      }
  };
  fetch(0, 0);

  // layer l's products over its whole K out of the planes; `next`: the layer whose first B fragments follow this layer's last (-1: none)
  auto kloop = [&](int l, int next, f32x4 (&acc)[MA][NF]) {
    const int nks = p.Kp[l] >> 5;
    int f0, cnt;
    dyf_wave_frags(p.width[l + 1], wave, f0, cnt);
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
      for (int b = 0; b < NF; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < nks; ++ks) {
      hx8 fbh[NF], fbl[NF];
#pragma unroll
      for (int b = 0; b < NF; ++b) { fbh[b] = nbh[b]; fbl[b] = nbl[b]; }
      if (ks + 1 < nks) fetch(l, ks + 1);
      else if (next >= 0) fetch(next, 0);
      if (cnt > 0) {
        hx8 fah[MA], fal[MA];
#pragma unroll
        for (int a = 0; a < MA; ++a) {
          fah[a] = *(const hx8*)&sH[(a * 16 + li) * AP + ks * 32 + 8 * lq];
          fal[a] = *(const hx8*)&sL[(a * 16 + li) * AP + ks * 32 + 8 * lq];
        }
#pragma unroll
        for (int b = 0; b < NF; ++b)
          if (b < cnt) {
#pragma unroll
            for (int a = 0; a < MA; ++a) {
              acc[a][b] = ORL_MFMA_16x16x32(fbl[b], fah[a], acc[a][b]);
              acc[a][b] = ORL_MFMA_16x16x32(fbh[b], fal[a], acc[a][b]);
              acc[a][b] = ORL_MFMA_16x16x32(fbh[b], fah[a], acc[a][b]);
            }
          }
      }
    }
  };
  // the next layer's K tail past the last fragment of an N-column activation: none, or 16 columns (Kp is a multiple of 32)
  auto zero_tail = [&](int N, int Kp_next) {
    const int t0 = ((N + 15) >> 4) * 16;
    if (t0 < Kp_next)
      for (int e = tid; e < RT * 4; e += 256) {
        hx_t* const s = (e & 1) ? sL : sH;
        hx8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (hx_t)0.f;
        *(hx8*)&s[(e >> 2) * AP + t0 + 8 * ((e >> 1) & 1)] = z;
      }
  };
  // this lane's four columns c .. c + 3 of the rows a * 16 + li: the activation v (zero past the layer and past n) checked and split
  // into the planes
  auto put = [&](int a, int c, const f32x4& v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) bad |= !(fabsf(v[j]) < 32768.f);      // (a NaN fails the comparison too; the zero fill passes)
    hx4 h, lo;
    orl_split4(v, h, lo);
    *(hx4*)&sH[(a * 16 + li) * AP + c] = h;
    *(hx4*)&sL[(a * 16 + li) * AP + c] = lo;
  };

  // the observations: RT rows x Kp[0], split into the planes; the rows past n and the K tail are zero
  {
    const int K0 = p.Kp[0];
    const float* const O = q.obs + (long)r * p.n * od;
    for (int e = tid; e < RT * K0; e += 256) {
      const int rr = e / K0, c = e - rr * K0;
      float v = 0.f;
      if (row0 + rr < p.n && c < od) v = O[(row0 + rr) * od + c];
      bad |= !(fabsf(v) < 32768.f);
      hx_t h, lo;
      orl_split1(v, h, lo);
      sH[rr * AP + c] = h;
      sL[rr * AP + c] = lo;
    }
  }
  __syncthreads();

  constexpr float inv = 1.0f / ORL_WSCALE;
  int f00, cnt0;
  dyf_wave_frags(H0, wave, f00, cnt0);
  // base = W0[:, :od] obs + b0 of this lane's elements, resident for every pass
  f32x4 base[MA][NF];
  kloop(0, 1, base);
  {
    const float* const b0 = par + p.b_off[0];
#pragma unroll
    for (int b = 0; b < NF; ++b)
      if (b < cnt0) {
        const int c = (f00 + b) * 16 + 4 * lq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float bj = b0[min(c + j, H0 - 1)];
#pragma unroll
          for (int a = 0; a < MA; ++a) base[a][b][j] = base[a][b][j] * inv + bj;
        }
      }
  }
  __syncthreads();                                           // every wave has read the observations out of the planes

  for (int j = 0; j < A; ++j) {
    // layer 0 of pass j without an MFMA: the rank-1 update by a_{j-1}, then the one-hot's column, LeakyReLU, the split
#pragma unroll
    for (int b = 0; b < NF; ++b)
      if (b < cnt0) {
        const int c = (f00 + b) * 16 + 4 * lq;
        f32x4 wa = f32x4{0.f, 0.f, 0.f, 0.f}, wo;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float* const wrow = W0 + (long)min(c + jj, H0 - 1) * q.in0 + od;
          if (j > 0) wa[jj] = wrow[j - 1];
          wo[jj] = wrow[A + j];
        }
#pragma unroll
        for (int a = 0; a < MA; ++a) {
          const int rr = a * 16 + li;
          const bool live = row0 + rr < p.n;
          const float prev = j > 0 ? sA[rr * A + j - 1] : 0.f;
          f32x4 v;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            base[a][b][jj] = fmaf(prev, wa[jj], base[a][b][jj]);
            v[jj] = (live && c + jj < H0) ? arf_leaky(base[a][b][jj] + wo[jj]) : 0.f;
          }
          put(a, c, v);
        }
      }
    zero_tail(H0, p.Kp[1]);
    __syncthreads();

    for (int l = 1; l < p.nl; ++l) {
      const int N = p.width[l + 1];
      const bool last = l + 1 == p.nl;
      int f0, cnt;
      dyf_wave_frags(N, wave, f0, cnt);
      f32x4 acc[MA][NF];
      kloop(l, last ? (j + 1 < A ? 1 : -1) : l + 1, acc);
      const float* const bias = par + p.b_off[l];
      if (last) {
        // the tail: (mean, logstd) of row li in elements 0, 1 of the lanes lq = 0 of wave 0; the draw
        if (wave == 0 && lq == 0) {
          const float bm = bias[0], bs = bias[1];
#pragma unroll
          for (int a = 0; a < MA; ++a) {
            const int rr = a * 16 + li;
            const long row = row0 + rr;
            float aj = 0.f;
            if (row < p.n) {
              const float mean = arf_leaky(acc[a][0][0] * inv + bm), lsd = arf_leaky(acc[a][0][1] * inv + bs);
              aj = mean + expf(lsd) * q.eps[(long)r * q.e_rs + row * A + j];
              q.act[((long)r * p.n + row) * A + j] = aj;
            }
            sA[rr * A + j] = aj;
          }
        }
        __syncthreads();                                     // the planes are read, the actions of pass j are in LDS
        break;
      }
      __syncthreads();                                       // every wave has read this layer's input out of the planes
#pragma unroll
      for (int b = 0; b < NF; ++b)
        if (b < cnt) {
          const int c = (f0 + b) * 16 + 4 * lq;
#pragma unroll
          for (int a = 0; a < MA; ++a) {
            const bool live = row0 + a * 16 + li < p.n;
            f32x4 v;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
              v[jj] = (live && c + jj < N) ? arf_leaky(acc[a][b][jj] * inv + bias[min(c + jj, N - 1)]) : 0.f;
            put(a, c, v);
          }
        }
      zero_tail(N, p.Kp[l + 1]);
      __syncthreads();
    }
  }
  if (bad) p.flags[DYF_FLAG_ACT] = 1u;
}

// one thread per 4 k of a plane row of one run; adjacent threads read adjacent k of a row of the [out][in] weight
__global__ __launch_bounds__(256) void k_autoreg_pack_planes(ArfP q) {
  dyf_pack_one<true>(q.g, (long)blockIdx.x * blockDim.x + threadIdx.x, 0, blockIdx.y, q.in0);
}

long arf_layout(ArfP& p) { return dyf_layout(p.g); }

// accumulator fragments per wave: 4 while every layer has at most 256 outputs, else 8
static int arf_nf(const ArfP& p) {
  int w = 0;
  for (int l = 1; l <= p.g.nl; ++l) w = p.g.width[l] > w ? p.g.width[l] : w;
  return w <= 256 ? 4 : 8;
}
// two planes [rt][Wp + 8] and the fp32 actions [rt][A]
static size_t arf_lds_bytes(const ArfP& p, int rt) { return sizeof(hx_t) * 2 * (size_t)rt * (p.g.Wp + 8) + sizeof(float) * (size_t)rt * p.A; }

int arf_pick_tile(const ArfP& p) {
  const int nf = arf_nf(p);
  for (int rt : {64, 32}) {
    if (nf == 8 || arf_lds_bytes(p, rt) > 65536) continue;       // (8 fragments per wave: 16 rows keep base + accumulators at 64 registers)
    if ((p.g.n + rt - 1) / rt * p.g.R >= 256) return rt;
  }
  return 16;
}

hipError_t arf_pack(const ArfP& p, hipStream_t st) {
  const long n = p.g.pmember >> 2;
  hipLaunchKernelGGL(k_autoreg_pack_planes, dim3((unsigned)((n + 255) / 256), p.g.R), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t arf_sample(const ArfP& p, hipStream_t st) {
  const DyfP& g = p.g;
  if (g.n < 1 || g.R < 1 || g.K != 1 || g.nl < 2 || g.nl > DYF_MAX_LAYERS || g.Wp > ORL_AUTOREG_FUSED_MAX_WIDTH || p.A < 1 || p.A > 32 ||
      g.width[g.nl] != 2 || p.in0 != g.width[0] + 2 * p.A)
    return hipErrorInvalidValue;
  for (int l = 0; l < g.nl; ++l)
    if (g.width[l] < 1 || g.width[l] > ORL_AUTOREG_FUSED_MAX_WIDTH) return hipErrorInvalidValue;
  const int rt = arf_pick_tile(p), nf = arf_nf(p);
  const dim3 grid((unsigned)((g.n + rt - 1) / rt), g.R);
  const size_t lds = arf_lds_bytes(p, rt);
  if (nf == 4 && rt == 64) hipLaunchKernelGGL((k_autoreg_fused_sample<64, 4>), grid, dim3(256), lds, st, p);
  else if (nf == 4 && rt == 32) hipLaunchKernelGGL((k_autoreg_fused_sample<32, 4>), grid, dim3(256), lds, st, p);
  else if (nf == 4) hipLaunchKernelGGL((k_autoreg_fused_sample<16, 4>), grid, dim3(256), lds, st, p);
  else hipLaunchKernelGGL((k_autoreg_fused_sample<16, 8>), grid, dim3(256), lds, st, p);
  return hipGetLastError();
}

}  // namespace orl
