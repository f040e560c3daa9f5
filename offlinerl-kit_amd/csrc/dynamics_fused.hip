// dynamics_fused.hip — the dynamics ensemble's forward-only pass at precision 1: every layer of one (run, member) row tile in one launch
// on v_mfma_f32_16x16x32_f16 with split operands (x = hi + lo fp16 planes, products hi*hi + hi*lo + lo*hi, fp32 accumulators).
//
// Work split.  Grid (row tiles, K members, R runs).  A workgroup (4 waves) owns RT = 16 / 32 / 64 rows of one (run, member) through all
// layers.  Per layer the 16-column fragments of the output are dealt out in contiguous runs of ceil(fragments / 4): 200 columns are 13
// fragments, 4 + 4 + 4 + 1.  A wave holds RT / 16 x NF accumulators (NF = 4 up to 256 columns; 8 up to 512, on 16-row tiles only) over the layer's whole K.
// Operands.  The activations live in LDS as two fp16 planes [2][RT][Wp + 8] (Wp: the widest layer input rounded up to 32; the 8 halves
// keep every fragment 16-byte aligned and the rows off each other's banks).  Layer 0's input is the fp32 step.x matrix, shared by the
// members and split as it is loaded; rows past n and the K tail are zero there and nothing past a row's floats is read.  The weights
// arrive pre-split (k_dyn_pack_planes: [R][K][layer][out][Kp] planes of w ORL_WSCALE, k-contiguous, the K tail zero), so a lane's B
// fragment -- 8 consecutive k of one output column -- is one 16-byte global load per plane; no wave shares a B fragment with another, so
// B does not pass through LDS, and one member's planes (0.6 MB at [200] x 4) stay in L2 under the row tiles that walk them.  The loads
// of k-step s + 1 -- or of the next layer's first one -- are issued into registers before the MFMAs of step s.
// Epilogue.  The MFMAs are issued with the operands swapped (gemm_kernel.h), so lane (li, lq) holds four consecutive columns 4 lq ..
// 4 lq + 3 of row li.  After a layer's k loop one barrier (every wave has read the planes), then accumulators / ORL_WSCALE + bias,
// orl_swish, the range check and the split back into the SAME planes, zeros in the columns up to the next layer's Kp and in the rows past
// n, and a second barrier.  The last layer stores fp32 rows of OUT instead.  A hidden activation never reaches HBM.
#include "dynamics_fused.h"

namespace orl {

template <int RT, int NF>
__global__ __launch_bounds__(256) void k_dyn_fused_fwd(DyfP p) {
  constexpr int MA = RT / 16;
  extern __shared__ __attribute__((aligned(16))) hx_t dyf_lds[];
  const int AP = p.Wp + 8;
  hx_t* const sH = dyf_lds;
  hx_t* const sL = dyf_lds + RT * AP;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const long row0 = (long)blockIdx.x * RT;
  const int k = blockIdx.y, r = blockIdx.z;
  const long rk = (long)r * p.K + k;
  const hx_t* const Bh = p.Bh + rk * p.pmember;
  const hx_t* const Bl = p.Bl + rk * p.pmember;
  const float* const par = p.params + (long)r * p.P;
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

  // layer 0's input: RT rows x Kp[0] as 4-k pieces, split into the planes
  {
    const int in = p.width[0], q0 = p.Kp[0] >> 2;
    const float* const X = p.X + (long)r * p.n * p.xp;
    for (int e = tid; e < RT * q0; e += 256) {
      const int rr = e / q0, kk = (e - rr * q0) * 4;
      const long row = row0 + rr;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (row < p.n && kk < p.xp) {                          // (xp is a multiple of 4: the piece lies inside the row's floats)
        v = *(const f32x4*)(X + row * p.xp + kk);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (kk + j >= in) v[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) bad |= !(fabsf(v[j]) < 32768.f);          // (a NaN fails the comparison too; the zero fill passes)
      hx4 h, lo;
      orl_split4(v, h, lo);
      *(hx4*)&sH[rr * AP + kk] = h;
      *(hx4*)&sL[rr * AP + kk] = lo;
    }
  }
  __syncthreads();

  constexpr float inv = 1.0f / ORL_WSCALE;
  for (int l = 0; l < p.nl; ++l) {
    const int N = p.width[l + 1], nks = p.Kp[l] >> 5;
    const bool last = l + 1 == p.nl;
    int f0, cnt;
    dyf_wave_frags(N, wave, f0, cnt);
    f32x4 acc[MA][NF];
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
      for (int b = 0; b < NF; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ks = 0; ks < nks; ++ks) {
      hx8 fbh[NF], fbl[NF];
#pragma unroll
      for (int b = 0; b < NF; ++b) { fbh[b] = nbh[b]; fbl[b] = nbl[b]; }
      if (ks + 1 < nks) fetch(l, ks + 1);
      else if (!last) fetch(l + 1, 0);
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

    const float* const bias = par + p.b_off[l] + (long)k * N;
    if (last) {
      float* const O = p.OUT + rk * p.n * p.op;
#pragma unroll
      for (int b = 0; b < NF; ++b)
        if (b < cnt) {
          const int c = (f0 + b) * 16 + 4 * lq;
#pragma unroll
          for (int a = 0; a < MA; ++a) {
            const long row = row0 + a * 16 + li;
            if (row >= p.n || c >= N) continue;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[a][b][j] * inv + bias[min(c + j, N - 1)];
            float* const o = O + row * p.op + c;
            if (c + 4 <= N) *(f32x4*)o = v;
            else
#pragma unroll
              for (int j = 0; j < 4; ++j) if (c + j < N) o[j] = v[j];
          }
        }
      break;
    }

    __syncthreads();                                         // every wave has read this layer's input out of the planes
#pragma unroll
    for (int b = 0; b < NF; ++b)
      if (b < cnt) {
        const int c = (f0 + b) * 16 + 4 * lq;
#pragma unroll
        for (int a = 0; a < MA; ++a) {
          const int rr = a * 16 + li;
          const bool live = row0 + rr < p.n;
          f32x4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = (live && c + j < N) ? orl_swish(acc[a][b][j] * inv + bias[min(c + j, N - 1)]) : 0.f;
            bad |= !(fabsf(v[j]) < 32768.f);
          }
          hx4 h, lo;
          orl_split4(v, h, lo);
          *(hx4*)&sH[rr * AP + c] = h;
          *(hx4*)&sL[rr * AP + c] = lo;
        }
      }
    // the next layer's K tail past the last fragment: none, or 16 columns (Kp is a multiple of 32)
    const int t0 = ((N + 15) >> 4) * 16;
    if (t0 < p.Kp[l + 1])
      for (int e = tid; e < RT * 4; e += 256) {
        hx_t* const s = (e & 1) ? sL : sH;
        hx8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (hx_t)0.f;
        *(hx8*)&s[(e >> 2) * AP + t0 + 8 * ((e >> 1) & 1)] = z;
      }
    __syncthreads();
  }
  if (bad) p.flags[DYF_FLAG_ACT] = 1u;
}

// one thread per 4 k of a plane row of one (run, member); adjacent threads read adjacent output columns of the (in, out)-major weight
__global__ __launch_bounds__(256) void k_dyn_pack_planes(DyfP p) {
  dyf_pack_one<false>(p, (long)blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y, blockIdx.z, 0);
}

long dyf_layout(DyfP& p) {
  long off = 0;
  p.Wp = 0;
  for (int l = 0; l < p.nl; ++l) {
    p.Kp[l] = (p.width[l] + 31) & ~31;
    p.Wp = p.Kp[l] > p.Wp ? p.Kp[l] : p.Wp;
    p.poff[l] = off;
    off += (long)p.width[l + 1] * p.Kp[l];
  }
  p.pmember = off;
  return (long)p.R * p.K * off;
}

// accumulator fragments per wave: 4 while every layer has at most 256 outputs, else 8
static int dyf_nf(const DyfP& p) {
  int w = 0;
  for (int l = 1; l <= p.nl; ++l) w = p.width[l] > w ? p.width[l] : w;
  return w <= 256 ? 4 : 8;
}
static size_t dyf_lds_bytes(const DyfP& p, int rt) { return sizeof(hx_t) * 2 * (size_t)rt * (p.Wp + 8); }

int dyf_pick_tile(const DyfP& p) {
  const int nf = dyf_nf(p);
  for (int rt : {64, 32}) {
    if (nf == 8 || dyf_lds_bytes(p, rt) > 65536) continue;       // (8 fragments per wave: 16 rows keep the accumulators at 32 registers)
    if ((p.n + rt - 1) / rt * p.K * p.R >= 256) return rt;
  }
  return 16;
}

hipError_t dyf_pack(const DyfP& p, hipStream_t st) {
  const long n = p.pmember >> 2;
  hipLaunchKernelGGL(k_dyn_pack_planes, dim3((unsigned)((n + 255) / 256), p.K, p.R), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t dyf_forward(const DyfP& p, hipStream_t st) {
  if (p.n < 1 || p.nl < 2 || p.nl > DYF_MAX_LAYERS || p.Wp > ORL_DYN_FUSED_MAX_WIDTH || (p.xp & 3)) return hipErrorInvalidValue;
  for (int l = 0; l <= p.nl; ++l)
    if (p.width[l] < 1 || p.width[l] > ORL_DYN_FUSED_MAX_WIDTH) return hipErrorInvalidValue;
  const int rt = dyf_pick_tile(p), nf = dyf_nf(p);
  const dim3 grid((unsigned)((p.n + rt - 1) / rt), p.K, p.R);
  const size_t lds = dyf_lds_bytes(p, rt);
  if (nf == 4 && rt == 64) hipLaunchKernelGGL((k_dyn_fused_fwd<64, 4>), grid, dim3(256), lds, st, p);
  else if (nf == 4 && rt == 32) hipLaunchKernelGGL((k_dyn_fused_fwd<32, 4>), grid, dim3(256), lds, st, p);
  else if (nf == 4) hipLaunchKernelGGL((k_dyn_fused_fwd<16, 4>), grid, dim3(256), lds, st, p);
  else hipLaunchKernelGGL((k_dyn_fused_fwd<16, 8>), grid, dim3(256), lds, st, p);
  return hipGetLastError();
}

}  // namespace orl
