// actor_fused.hip — the tanh-Gaussian actor's rollout sampling: backbone, head and draw of one row tile in one launch on
// v_mfma_f32_16x16x32_f16 with split operands (x = hi + lo fp16 planes, products lo*hi + hi*lo + hi*hi, fp32 accumulators).
//
// Work split.  Grid (row tiles, R runs).  A workgroup (4 waves) owns RT = 16 / 32 / 64 rows of one run through all layers; rows are
// independent, so __syncthreads() is the only synchronisation.  Per layer the 16-column fragments of the output are dealt to the waves
// as in k_dyn_fused_fwd (dyf_wave_frags); a wave holds RT / 16 x NF accumulators (NF = 4 up to 256 columns; 8 up to 512, on 16-row
// tiles only) over the layer's whole K.  The activations live in LDS as two fp16 planes [2][RT][Wp + 8], the weights arrive pre-split
// (k_actor_pack_planes: [R][layer][out][Kp] planes of w ORL_WSCALE; nn.Linear's [out][in] rows are k-contiguous already), a lane's B
// fragment is one 16-byte global load per plane, fetched into registers one k-step ahead -- across layers too.
// Backbone.  After a layer's k loop one barrier (every wave has read the planes), then accumulators / ORL_WSCALE + bias, ReLU, the range
// check and the split back into the SAME planes, zeros up to the next layer's Kp and in the rows that do not count, a second barrier.
// Head.  The arena keeps [mu ; sigma] as one [2A][H] matrix, so the head is one plane layer of 2A <= 64 columns.  mu_j and ls_j of a row
// land in different fragments (columns j and A + j), for A > 8 in different waves: accumulators / ORL_WSCALE + bias go to an fp32
// staging block [RT][2A] behind the planes, and after ONE barrier thread e of RT x A takes (row e / A, j = e % A) through
// orl_tanh_sample (sample.h: the clamp, expf, tanhf of the training step's sampling epilogues) and stores act[run][row][j] -- plain
// 4-byte stores, consecutive threads to consecutive floats, because a row of A floats is not 16-byte friendly.
// Ragged runs.  live[r] rows of run r count.  A workgroup whose tile starts at or past live[r] stores zeros to its rows and returns
// before the first fetch and the first barrier (the test is uniform over the block); a partly live tile carries zero rows through the
// layers and stores zeros for them.
#include "actor_fused.h"
#include "sample.h"

namespace orl {

template <int RT, int NF>
__global__ __launch_bounds__(256) void k_actor_fused_sample(AcfP q) {
  constexpr int MA = RT / 16;
  const DyfP& p = q.g;
  extern __shared__ __attribute__((aligned(16))) hx_t acf_lds[];
  const int AP = p.Wp + 8, A = q.A, A2 = 2 * q.A;
  hx_t* const sH = acf_lds;
  hx_t* const sL = acf_lds + RT * AP;
  float* const sS = (float*)(acf_lds + 2 * RT * AP);         // [RT][2A] the head: mu | raw log-sigma
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const long row0 = (long)blockIdx.x * RT;
  const int r = blockIdx.y;
  const long nlive = q.live ? min((long)max(q.live[r], 0), p.n) : p.n;
  float* const ACT = q.act + (long)r * p.n * A;
  if (row0 >= nlive) {
    for (int e = tid; e < RT * A; e += 256)
      if (row0 + e / A < p.n) ACT[row0 * A + e] = 0.f;
    return;
  }
  const hx_t* const Bh = p.Bh + (long)r * p.pmember;
  const hx_t* const Bl = p.Bl + (long)r * p.pmember;
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

  // the observations: RT rows x Kp[0], split into the planes; the rows that do not count and the K tail are zero
  {
    const int K0 = p.Kp[0], od = p.width[0];
    const float* const O = q.obs + (long)r * p.n * od;
    for (int e = tid; e < RT * K0; e += 256) {
      const int rr = e / K0, c = e - rr * K0;
      float v = 0.f;
      if (row0 + rr < nlive && c < od) v = O[(row0 + rr) * od + c];
      bad |= !(fabsf(v) < 32768.f);                          // (a NaN fails the comparison too)
      hx_t h, lo;
      orl_split1(v, h, lo);
      sH[rr * AP + c] = h;
      sL[rr * AP + c] = lo;
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
    const float* const bias = par + p.b_off[l];
    if (last) {
      // the head: lane (li, lq) holds columns c .. c + 3 of the rows a * 16 + li; staged in fp32, nothing is split
#pragma unroll
      for (int b = 0; b < NF; ++b)
        if (b < cnt) {
          const int c = (f0 + b) * 16 + 4 * lq;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c + j < A2) {
              const float bj = bias[c + j];
#pragma unroll
              for (int a = 0; a < MA; ++a) sS[(a * 16 + li) * A2 + c + j] = acc[a][b][j] * inv + bj;
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
          const bool on = row0 + a * 16 + li < nlive;
          f32x4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = (on && c + j < N) ? fmaxf(acc[a][b][j] * inv + bias[min(c + j, N - 1)], 0.f) : 0.f;
            bad |= !(fabsf(v[j]) < 32768.f);
          }
          hx4 h, lo;
          orl_split4(v, h, lo);
          *(hx4*)&sH[(a * 16 + li) * AP + c] = h;
          *(hx4*)&sL[(a * 16 + li) * AP + c] = lo;
        }
      }
    // the next layer's K tail past the last fragment of this N-column activation: none, or 16 columns (Kp is a multiple of 32)
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
  __syncthreads();                                           // the head of every row is staged

  const float* const E = q.deterministic ? nullptr : q.eps + (long)r * q.e_rs;
  for (int e = tid; e < RT * A; e += 256) {
    const int rr = e / A, j = e - rr * A;
    const long row = row0 + rr;
    if (row >= p.n) break;                                   // (rows grow with e)
    float a = 0.f;
    if (row < nlive) {
      const float mu = sS[rr * A2 + j];
      if (E) orl_tanh_sample(mu, sS[rr * A2 + A + j], E[row * A + j], a);
      else a = tanhf(mu);
    }
    ACT[row * A + j] = a;
  }
  if (bad) p.flags[DYF_FLAG_ACT] = 1u;
}

// one thread per 4 k of a plane row of one run; adjacent threads read adjacent k of a row of the [out][in] weight
__global__ __launch_bounds__(256) void k_actor_pack_planes(AcfP q) {
  dyf_pack_one<true>(q.g, (long)blockIdx.x * blockDim.x + threadIdx.x, 0, blockIdx.y, q.g.width[0]);
}

long acf_layout(AcfP& p) { return dyf_layout(p.g); }

// accumulator fragments per wave: 4 while every layer has at most 256 outputs, else 8
static int acf_nf(const AcfP& p) {
  int w = 0;
  for (int l = 1; l <= p.g.nl; ++l) w = p.g.width[l] > w ? p.g.width[l] : w;
  return w <= 256 ? 4 : 8;
}
// two planes [rt][Wp + 8] and the fp32 head staging [rt][2A]
static size_t acf_lds_bytes(const AcfP& p, int rt) { return sizeof(hx_t) * 2 * (size_t)rt * (p.g.Wp + 8) + sizeof(float) * (size_t)rt * 2 * p.A; }

int acf_pick_tile(const AcfP& p) {
  const int nf = acf_nf(p);
  for (int rt : {64, 32}) {
    if (nf == 8 || acf_lds_bytes(p, rt) > 65536) continue;       // (8 fragments per wave: 16 rows keep the accumulators at 32 registers)
    if ((p.g.n + rt - 1) / rt * p.g.R >= 256) return rt;
  }
  return 16;
}

hipError_t acf_pack(const AcfP& p, hipStream_t st) {
  const long n = p.g.pmember >> 2;
  hipLaunchKernelGGL(k_actor_pack_planes, dim3((unsigned)((n + 255) / 256), p.g.R), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t acf_sample(const AcfP& p, hipStream_t st) {
  const DyfP& g = p.g;
  if (g.n < 1 || g.R < 1 || g.K != 1 || g.nl < 2 || g.nl > DYF_MAX_LAYERS || g.Wp > ORL_ACTOR_FUSED_MAX_WIDTH || p.A < 1 ||
      p.A > ORL_ACTOR_FUSED_MAX_ACT || g.width[g.nl] != 2 * p.A || (!p.deterministic && !p.eps))
    return hipErrorInvalidValue;
  for (int l = 0; l < g.nl; ++l)
    if (g.width[l] < 1 || g.width[l] > ORL_ACTOR_FUSED_MAX_WIDTH) return hipErrorInvalidValue;
  const int rt = acf_pick_tile(p), nf = acf_nf(p);
  const dim3 grid((unsigned)((g.n + rt - 1) / rt), g.R);
  const size_t lds = acf_lds_bytes(p, rt);
  if (nf == 4 && rt == 64) hipLaunchKernelGGL((k_actor_fused_sample<64, 4>), grid, dim3(256), lds, st, p);
  else if (nf == 4 && rt == 32) hipLaunchKernelGGL((k_actor_fused_sample<32, 4>), grid, dim3(256), lds, st, p);
  else if (nf == 4) hipLaunchKernelGGL((k_actor_fused_sample<16, 4>), grid, dim3(256), lds, st, p);
  else hipLaunchKernelGGL((k_actor_fused_sample<16, 8>), grid, dim3(256), lds, st, p);
  return hipGetLastError();
}

}  // namespace orl
