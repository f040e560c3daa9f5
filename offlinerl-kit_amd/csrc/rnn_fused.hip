// rnn_fused.hip — RNNDynamics' GRU stack at eval precision 1: all L layers of a row tile of sequences over all T steps in one launch on
// v_mfma_f32_16x16x32_f16 with split operands (x = hi + lo fp16 planes, products lo*hi + hi*lo + hi*hi, fp32 accumulators).
//
// Work split.  Grid (row tiles, runs).  A workgroup of 8 waves owns RT = 16 / 32 / 64 sequences through every layer and step; sequences
// are independent, so __syncthreads() is the only synchronisation.  Wave w owns the unit tiles w, w + 8, ... of 16 hidden units each: NT
// = 2 tiles per wave up to H = 256, 4 up to 512 (on 16-row tiles only: 4 accumulators per (row fragment, tile) are 16 registers).  A
// layer-step multiplies the concatenated operand [x_t | h_{t-1}] (Kxp + Hp deep) by the packed rows [W_ih | W_hh] of the gates r, z, n of
// the wave's units: r and z accumulate the x and the h products in one accumulator each, in one fixed order (every k of x, then every k
// of h, as k_rnn_cell does); n keeps W_in x and W_hn h apart.  The wave's tiles are taken two at a time, one on 64-row tiles (a pass: 6 B fragments of
// two planes, 48 registers), each pass running the whole k loop; a B fragment is loaded once and multiplies every row fragment of the tile.
// Operands.  LDS holds h of every layer as two fp16 planes [L][2][RT][Hp + 8] (zero at t = 0; the 8 halves keep a fragment 16-byte
// aligned and the rows off each other's banks) and the step's layer-0 input [2][RT][Kxp0 + 8], read from the fp32 X0 rows and split as it
// is staged.  Layer l reads layer l - 1's NEW planes as x and its own OLD planes as h.  The weights arrive pre-split (k_rnn_pack_planes,
// k-contiguous, tails zero): a lane's B fragment -- 8 consecutive k of one gate row -- is one 16-byte global load per plane, and the
// fragments of the next k-step (or of the next pass, layer or time step) are asked for before the MFMAs of the current one.
// A layer-step.  The k loops; the gate arithmetic on the accumulators (/ ORL_WSCALE, biases, rnn_sigmoid, tanhf, h = (1 - z) n + z h_prev
// with h_prev = hi + lo of the lane's own elements), which like k_rnn_scan_fwd runs BEFORE the barrier so that it overlaps the other
// waves' MFMAs and only the new h stays in registers; a barrier (every wave has read the old planes); the split of the new h into the
// same planes -- and, after layer 0, the staging of x_{t+1} --; a second barrier.  2 L T barriers in all.  The MFMAs are issued with the
// operands swapped (gemm_kernel.h), so lane (li, lq) holds the units 4 lq .. 4 lq + 3 of sequence li: one 8-byte store per plane.  The top
// layer stores fp32 h_t to HO at every t; when priming every layer stores h_{T-1} to the state slots.  Nothing else reaches HBM.
#include "rnn_fused.h"

namespace orl {

template <int RT, int NT>
__global__ __launch_bounds__(64 * RNF_WAVES) void k_rnn_fused_fwd(RnfP p) {
  constexpr int MA = RT / 16, TP = RT == 64 ? 1 : 2, NP = NT / TP;       // TP: tiles of a pass
  extern __shared__ __attribute__((aligned(16))) hx_t rnf_lds[];
  const int H = p.H, Hp = p.Hp, HP = Hp + 8, L = p.L, T = p.T, XP = p.Kxp[0] + 8;
  hx_t* const sX = rnf_lds + (long)L * 2 * RT * HP;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const long row0 = (long)blockIdx.x * RT;
  const long run = blockIdx.y;
  const hx_t* const Bh = p.Bh + run * p.prun;
  const hx_t* const Bl = p.Bl + run * p.prun;
  const float* const par = p.params + run * p.P;
  const float* const X = p.X0 + run * p.x_rs;
  float* const HO = p.HO + run * p.ho_rs;
  unsigned int bad = 0;

  // this wave's B fragments of the next k-step: [tile of the pass][gate]; a unit past H is clamped into the layer and its results dropped
  hx8 nbh[TP][3], nbl[TP][3];
  auto fetch = [&](int l, int ps, int ks) {
    const int KW = p.Kxp[l] + Hp;
#pragma unroll
    for (int u = 0; u < TP; ++u) {
      const int j0 = (wave + RNF_WAVES * (TP * ps + u)) * 16;
      if (j0 < H) {                                            // (wave-uniform)
        const long off = p.poff[l] + (long)min(j0 + li, H - 1) * KW + ks * 32 + 8 * lq;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          nbh[u][g] = *(const hx8*)(Bh + off + (long)g * H * KW);
          nbl[u][g] = *(const hx8*)(Bl + off + (long)g * H * KW);
        }
      }
    }
  };
  fetch(0, 0, 0);

  // layer 0's input of step t: RT rows x Kxp0, rows past the tile's sequences and the k tail zero
  auto stage = [&](int t) {
    const int K0 = p.Kxp[0];
    for (int e = tid; e < RT * K0; e += 64 * RNF_WAVES) {
      const int rr = e / K0, c = e - rr * K0;
      float v = 0.f;
      if (row0 + rr < p.rows && c < p.in) v = X[((row0 + rr) * T + t) * p.xp + c];
      bad |= !(fabsf(v) < 32768.f);                            // (a NaN fails the comparison too; the zero fill passes)
      hx_t h, lo;
      orl_split1(v, h, lo);
      sX[rr * XP + c] = h;
      sX[(RT + rr) * XP + c] = lo;
    }
  };
  {
    const int n8 = (L * 2 * RT * HP + 2 * RT * XP) >> 3;       // (HP and XP are multiples of 8)
    hx8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (hx_t)0.f;
    for (int e = tid; e < n8; e += 64 * RNF_WAVES) ((hx8*)rnf_lds)[e] = z;
  }
  __syncthreads();
  stage(0);
  __syncthreads();

  constexpr float inv = 1.0f / ORL_WSCALE;
  for (int t = 0; t < T; ++t)
    for (int l = 0; l < L; ++l) {
      const int nkx = p.Kxp[l] >> 5, nks = nkx + (Hp >> 5);
      hx_t* const hown = rnf_lds + (long)l * 2 * RT * HP;      // this layer's planes: hi, then lo at + RT * HP
      const hx_t* const xin = l ? hown - 2 * RT * HP : sX;
      const int xpitch = l ? HP : XP;
      f32x4 acc[NT][MA][4];                                    // r, z, W_in x, W_hn h
#pragma unroll
      for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int a = 0; a < MA; ++a)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[it][a][g] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
      for (int ps = 0; ps < NP; ++ps) {
        const bool live[2] = {(wave + RNF_WAVES * (TP * ps)) * 16 < H, (wave + RNF_WAVES * (TP * ps + 1)) * 16 < H};
        for (int ks = 0; ks < nks; ++ks) {
          hx8 fbh[TP][3], fbl[TP][3];
#pragma unroll
          for (int u = 0; u < TP; ++u)
#pragma unroll
            for (int g = 0; g < 3; ++g) { fbh[u][g] = nbh[u][g]; fbl[u][g] = nbl[u][g]; }
          if (ks + 1 < nks) fetch(l, ps, ks + 1);
          else if (ps + 1 < NP) fetch(l, ps + 1, 0);
          else if (l + 1 < L) fetch(l + 1, 0, 0);
          else if (t + 1 < T) fetch(0, 0, 0);
          const bool isx = ks < nkx;
          const hx_t* const ab = isx ? xin + ks * 32 : hown + (ks - nkx) * 32;
          const int ap = isx ? xpitch : HP;
#pragma unroll
          for (int a = 0; a < MA; ++a) {
            const int o = (a * 16 + li) * ap + 8 * lq;
            const hx8 fah = *(const hx8*)(ab + o), fal = *(const hx8*)(ab + RT * ap + o);
#pragma unroll
            for (int u = 0; u < TP; ++u) {
              if (!live[u]) continue;
              f32x4* const A = acc[TP * ps + u][a];
              auto mul3 = [&](int g, f32x4& d) {
                d = ORL_MFMA_16x16x32(fbl[u][g], fah, d);
                d = ORL_MFMA_16x16x32(fbh[u][g], fal, d);
                d = ORL_MFMA_16x16x32(fbh[u][g], fah, d);
              };
              mul3(0, A[0]);
              mul3(1, A[1]);
              if (isx) mul3(2, A[2]);                          // (wave-uniform)
              else mul3(2, A[3]);
            }
          }
        }
      }

      // the gates of this lane's elements: sequence a * 16 + li, units c .. c + 3 (H is a multiple of 4: a quad is inside or outside)
      f32x4 hnew[NT][MA];
      const bool top = l + 1 == L, prime = p.st[0] && t + 1 == T;
#pragma unroll
      for (int it = 0; it < NT; ++it) {
        const int c = (wave + RNF_WAVES * it) * 16 + 4 * lq;
        if (c >= H) continue;
        const f32x4 bir = *(const f32x4*)(par + p.bih[l] + c), biz = *(const f32x4*)(par + p.bih[l] + H + c),
                    bin = *(const f32x4*)(par + p.bih[l] + 2 * H + c);
        const f32x4 bhr = *(const f32x4*)(par + p.bhh[l] + c), bhz = *(const f32x4*)(par + p.bhh[l] + H + c),
                    bhn = *(const f32x4*)(par + p.bhh[l] + 2 * H + c);
#pragma unroll
        for (int a = 0; a < MA; ++a) {
          const int rr = a * 16 + li;
          const hx4 ph = *(const hx4*)&hown[rr * HP + c], pl = *(const hx4*)&hown[(RT + rr) * HP + c];
          const f32x4* const A = acc[it][a];
          f32x4 hv;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float hprev = (float)ph[j] + (float)pl[j];
            const float rg = rnn_sigmoid((A[0][j] * inv + bir[j]) + bhr[j]);
            const float zg = rnn_sigmoid((A[1][j] * inv + biz[j]) + bhz[j]);
            const float ng = tanhf((A[2][j] * inv + bin[j]) + rg * (A[3][j] * inv + bhn[j]));
            hv[j] = (1.f - zg) * ng + zg * hprev;
          }
          hnew[it][a] = hv;
          const long b = row0 + rr;
          if (b < p.rows) {
            if (top) *(f32x4*)(HO + (b * T + t) * p.hop + c) = hv;
            if (prime) {
              const long o = run * p.st_rs + ((long)l * p.n_traj + b) * H + c;
              *(f32x4*)(p.st[0] + o) = hv;
              *(f32x4*)(p.st[1] + o) = hv;
            }
          }
        }
      }
      __syncthreads();                                         // every wave has read this layer's old planes (and layer 0's input)
#pragma unroll
      for (int it = 0; it < NT; ++it) {
        const int c = (wave + RNF_WAVES * it) * 16 + 4 * lq;
        if (c >= H) continue;
#pragma unroll
        for (int a = 0; a < MA; ++a) {
          const int rr = a * 16 + li;
          hx4 h, lo;
          orl_split4(hnew[it][a], h, lo);
          *(hx4*)&hown[rr * HP + c] = h;
          *(hx4*)&hown[(RT + rr) * HP + c] = lo;
        }
      }
      if (l == 0 && t + 1 < T) stage(t + 1);
      __syncthreads();
    }
  if (bad) p.flags[RNF_FLAG_ACT] = 1u;
}

// one thread per 4 k of a plane row of one run: the rows of W_ih, then the rows of W_hh along k.  Layer 0's W_ih rows are `in` floats
// long, no multiple of 4, so the weights are read one by one here (adjacent threads read adjacent k) and the hot kernel never does
__global__ __launch_bounds__(256) void k_rnn_pack_planes(RnfP p) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (p.prun >> 2)) return;
  const long run = blockIdx.y;
  int l = 0;
  while (l + 1 < p.L && e >= (p.poff[l + 1] >> 2)) ++l;
  const long le = e - (p.poff[l] >> 2);
  const int K = l ? p.H : p.in, Kxp = p.Kxp[l], q = (Kxp + p.Hp) >> 2;
  const int row = (int)(le / q), kk = (int)(le - (long)row * q) * 4;
  const float* const par = p.params + run * p.P;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  unsigned int bad = 0;
  if (row < 3 * p.H) {
    const bool xpart = kk < Kxp;                               // (Kxp is a multiple of 4: a quad lies in one part)
    const int k0 = xpart ? kk : kk - Kxp, width = xpart ? K : p.H;
    const float* const W = par + (xpart ? p.wih[l] : p.whh[l]) + (long)row * width;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k0 + j < width) v[j] = W[k0 + j] * ORL_WSCALE;
      bad |= !(fabsf(v[j]) < 65504.f);
    }
  }
  hx4 h, lo;
  orl_split4(v, h, lo);
  const long at = run * p.prun + p.poff[l] + (long)row * (Kxp + p.Hp) + kk;
  *(hx4*)(p.Bh + at) = h;
  *(hx4*)(p.Bl + at) = lo;
  if (bad) p.flags[RNF_FLAG_W] = 1u;
}

long rnf_layout(RnfP& p) {
  p.Hp = (p.H + 31) & ~31;
  p.G16 = (3 * p.H + 15) & ~15;
  long off = 0;
  for (int l = 0; l < p.L; ++l) {
    p.Kxp[l] = ((l ? p.H : p.in) + 31) & ~31;
    p.poff[l] = off;
    off += (long)p.G16 * (p.Kxp[l] + p.Hp);
  }
  p.prun = off;
  return off;
}

size_t rnf_lds_bytes(const RnfP& p, int rt) {
  return sizeof(hx_t) * 2 * (size_t)rt * ((size_t)p.L * (p.Hp + 8) + p.Kxp[0] + 8);
}

int rnf_pick_tile(const RnfP& p, int runs) {
  for (int rt : {64, 32}) {
    if (p.H > 256 || rnf_lds_bytes(p, rt) > RNF_LDS_BYTES) continue;       // (4 tiles per wave: 16 rows keep the accumulators at 64 registers)
    if ((long)((p.rows + rt - 1) / rt) * runs >= p.cus) return rt;
  }
  return rnf_lds_bytes(p, 16) <= RNF_LDS_BYTES ? 16 : 0;
}

hipError_t rnf_pack(const RnfP& p, int runs, hipStream_t st) {
  const long n = p.prun >> 2;
  hipLaunchKernelGGL(k_rnn_pack_planes, dim3((unsigned)((n + 255) / 256), runs), dim3(256), 0, st, p);
  return hipGetLastError();
}

template <int RT, int NT>
static hipError_t rnf_launch(const RnfP& p, int runs, hipStream_t st) {
  const size_t lds = rnf_lds_bytes(p, RT);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)k_rnn_fused_fwd<RT, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_rnn_fused_fwd<RT, NT>), dim3((unsigned)((p.rows + RT - 1) / RT), runs), dim3(64 * RNF_WAVES), lds, st, p);
  return hipGetLastError();
}

hipError_t rnf_forward(const RnfP& p, int runs, hipStream_t st) {
  if (p.rows < 1 || p.T < 1 || runs < 1 || p.L < 1 || p.L > RNF_MAX_LAYERS || p.H < 4 || p.H > RNF_MAX_H || (p.H & 3) || p.in < 1 ||
      (p.hop & 3) || (p.P & 3))
    return hipErrorInvalidValue;
  const int rt = rnf_pick_tile(p, runs);
  if (rt == 64) return rnf_launch<64, 2>(p, runs, st);
  if (rt == 32) return rnf_launch<32, 2>(p, runs, st);
  if (rt == 16) return p.H <= 256 ? rnf_launch<16, 2>(p, runs, st) : rnf_launch<16, 4>(p, runs, st);
  return hipErrorInvalidValue;
}

}  // namespace orl
