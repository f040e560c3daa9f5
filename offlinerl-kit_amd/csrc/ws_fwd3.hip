// ws_fwd3.hip — precision 2 (three fp16 planes, fp32-class arithmetic) flavour of ws_fwd_kernel<TQ, L0, ., SY = false>: the fused
// first + second layer forward of a single-output net with the tail folded in (interface and design notes: ws_gemm.h; the two-plane
// kernel this follows: ws_fwd.hip).
//
// x = hi + mid + lo in fp16 planes represents an fp32 operand exactly; the six products hi*hi, hi*mid, mid*hi, hi*lo, mid*mid, lo*hi with
// fp32 accumulation drop only terms below 2^-33 of a product.  Three resident planes of W1 for 32 columns would be 192 VGPRs per lane, so a
// workgroup owns HALF of the net's 256 output columns (blockIdx.y = the half; wave w: columns 128 half + 16 w .. + 15 = 96 VGPRs) and two
// workgroups stream the same row groups.  Layer 1 needs all 256 columns of h0, so BOTH halves run the fused first layer for all columns
// (wave w: h0 columns 32 w .. + 31, 24 of a wave's 120 MFMAs per group); a wave stores its h0 block to HBM only in the workgroup whose half
// contains those columns -- the other copy goes to a scratch line through the same store instruction (a wave-uniform branch inside the row
// loop costs the product kernel ~20 %: DESIGN.md section 8).  Each half reduces the tail over its 128 columns: half 0 writes q (with the
// tail bias), half 1 a partial that k_tail_add folds in.  Mask words: a half writes its four words per row of h1; half 0 writes h0's.
// Reference: nets/mlp.py:9-33 (Linear + ReLU stack), modules/critic_module.py:17-28 (the single-output tail), modules/actor_module.py:22-27.
#include "ws_device.h"

namespace orl {

// TQ: the single-output tail folded in (two partial sums); SY: the top activation is stored (each half its 128 columns); XS: h0 is stored
// (false: forward-only passes, WsFwdP::x0_discard).  L0 = false: no fused first layer -- the layer's input rows come from HBM (a hidden layer
// above the second one of a deeper net: run_cql.py:31's [256, 256, 256]) and are split into the three planes while both halves stage them.
// DG (with L0 = false, SY): plain dgrad mode -- Y = (X B^T) (.) mask with X a materialised gradient (times the run's dynamic scale while it is
// staged), B the weights viewed transposed, no bias / ReLU / mask emission; the mask of the receiving activation comes from its packed bits.
// All compile-time flavours, as in ws_fwd_kernel.
template <bool TQ, bool SY, bool XS, bool L0 = true, bool DG = false>
__global__ __launch_bounds__(WS_NT) void ws_fwd3_kernel(const WsFwdP p) {
  static_assert(!DG || (!TQ && SY && !L0), "gradient mode: rows from HBM, result stored, no tail");
  static_assert(WS_NW == 8 && WS_ROWS == 32 && WS_SUB == 2, "eight waves, 32-row groups");
  extern __shared__ __attribute__((aligned(16))) float ws_smem[];
  hx_t* Ah = (hx_t*)ws_smem;                                           // [buf][hi, mid, lo][row][WS_PITCH]
  float* qs = ws_smem + (2 * 3 * WS_ROWS * WS_PITCH * 2) / 4;             // [parity][wave][row]
  unsigned char* nbs = (unsigned char*)(qs + 2 * WS_NW * WS_ROWS);         // [parity][row][WS_NBP]: 4 mask bits per (row, 4 columns of this half)
  float* Xl = (float*)(nbs + 2 * WS_ROWS * WS_NBP);                        // [buf][row][WF3_XLP]: narrow input rows, planes in 16-bit slots 0.. / 32.. / 64..
  unsigned char* nbs0 = (unsigned char*)(Xl + 2 * WS_ROWS * WF3_XLP);      // mask nibbles of the produced h0 (all 256 columns)
  float* cst = (float*)(nbs0 + 2 * WS_ROWS * WS_NBP);                      // [bias | tail weights]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const int half = blockIdx.y;
  const int z = blockIdx.z, z0 = z / p.nz1, z1 = z - z0 * p.nz1;
  const float* __restrict__ Wg = p.W.p + z0 * p.W.s0 + z1 * p.W.s1;
  const float* __restrict__ bg = DG ? nullptr : p.bias.p + z0 * p.bias.s0 + z1 * p.bias.s1;
  const unsigned int* __restrict__ dmg = DG ? p.dmask.p + z0 * p.dmask.s0 + z1 * p.dmask.s1 : nullptr;
  const float a_sc = (DG && p.gscale) ? p.gscale[z0] : 1.f;          // gradient mode: the staged rows carry the run's dynamic gradient scale
  float* __restrict__ Y0g = const_cast<float*>(p.X.p) + z0 * p.X.s0 + z1 * p.X.s1;      // h0 is written where the plain kernel reads it
  float* __restrict__ Yg = SY ? p.Y.p + z0 * p.Y.s0 + z1 * p.Y.s1 : nullptr;
  const float* __restrict__ X0g = L0 ? p.X0.p + z0 * p.X0.s0 + z1 * p.X0.s1 : nullptr;
  const float* __restrict__ Xg = p.X.p + z0 * p.X.s0 + z1 * p.X.s1;           // L0 = false: the layer's input rows
  const int ncol1 = 128 * half + 16 * wave;                              // layer-1 columns of this wave
  const int ncol0 = 32 * wave;                                           // h0 columns this wave produces
  // the h0 store of a wave whose columns belong to the other half lands in a per-workgroup scratch line (row pitch 0)
  const bool mine = (wave >> 2) == half;
  float* __restrict__ y0b = !XS ? nullptr : (mine ? Y0g : p.dump + (long)(((blockIdx.z * gridDim.x + blockIdx.x) * 2 + half) & (WS_DUMP_SLOTS - 1)) * WS_N);
  const long y0p = mine ? p.x_pitch : 0;

  // ---- resident layer-1 fragments: lane (li, lq) supplies W1[n = ncol1 + li][k = 32 ks + 8 lq .. + 7], times ORL_WSCALE ----
  hx8 bh[8], bm[8], bl[8];
  {
    f32x4 raw[1][8][2];
    ws_w_frag_load(Wg, p.w_sn, p.w_sk, ncol1, li, lq, raw);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) ws_split8x3(raw[0][ks][0] * ORL_WSCALE, raw[0][ks][1] * ORL_WSCALE, bh[ks], bm[ks], bl[ks]);
  }
  // first-layer fragments of columns ncol0 + 16 cb + li, K = 32: W0'[n][k] = W0[n][k] (k < in0), b0[n] (k == in0), 0 beyond (unscaled, as in ws_fwd)
  hx8 b0[2][3];                                                          // [cb][hi, mid, lo]
  if constexpr (L0) {
    const float* __restrict__ W0g = p.W0.p + z0 * p.W0.s0 + z1 * p.W0.s1;
    const float* __restrict__ b0g = p.b0.p + z0 * p.b0.s0 + z1 * p.b0.s1;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) ws_w0_frag(p, W0g, ncol0 + 16 * cb + li, lq, b0g[ncol0 + 16 * cb + li], b0[cb]);
  }
  const float* __restrict__ twg = TQ ? p.tw.p + z0 * p.tw.s0 + z1 * p.tw.s1 : bg;
  if (!DG && tid < WS_N) { cst[tid] = bg[tid]; cst[WS_N + tid] = twg[tid]; }     // visible after the prologue's barriers
  const float tbias = (TQ && half == 0) ? (p.tb.p + z0 * p.tb.s0 + z1 * p.tb.s1)[0] : 0.f;
  float* __restrict__ tqo = !TQ ? nullptr : (half == 0 ? p.tq.p + z0 * p.tq.s0 + z1 * p.tq.s1 : p.tq2.p + z0 * p.tq2.s0 + z1 * p.tq2.s1);
  const long tqsm = half == 0 ? p.tq_sm : 1;
  const float inv_sc = 1.0f / (ORL_WSCALE * a_sc);

  // ---- narrow-input staging (two elements per thread), split ONCE into three planes ----
  const int xe = L0 ? WS_ROWS * p.x0_pitch : 0;
  int xr[2], xc[2];
  float sx[2];
  ws_x_index(L0, tid, p.x0_pitch, xe, xr, xc);
  // ---- L0 = false: staging of one [32][256] row group from HBM (thread t moves float4 #(t + 512 i), i = 0..3), split into three planes ----
  f32x4 st0[WS_LD];
  auto load_piece = [&](int g, int i) __attribute__((always_inline)) {
    const int idx = tid + WS_NT * i, r = idx >> 6, kq = idx & 63;
    st0[i] = *(const f32x4*)&Xg[((long)g * WS_ROWS + r) * p.x_pitch + 4 * kq];
  };
  auto store_piece = [&](int buf, int i) __attribute__((always_inline)) {
    hx_t* dh = Ah + (long)buf * 3 * WS_ROWS * WS_PITCH;
    const int idx = tid + WS_NT * i, r = idx >> 6, kq = idx & 63;
    hx4 h, mm, l;
    if (DG) orl_split4x3(st0[i] * a_sc, h, mm, l); else orl_split4x3(st0[i], h, mm, l);
    const int o = ws_a_off(r, kq);
    *(hx4*)(dh + o) = h;
    *(hx4*)(dh + WS_ROWS * WS_PITCH + o) = mm;
    *(hx4*)(dh + 2 * WS_ROWS * WS_PITCH + o) = l;
  };
  auto loadX = [&](int g) __attribute__((always_inline)) { ws_x_load(X0g, g, xe, tid, sx); };
  auto storeX = [&](int buf) __attribute__((always_inline)) { ws_x_store<3, WF3_XLP>(Xl, buf, p.in0, xr, xc, sx); };
  auto prod_x = [&](int xbuf, int s, hx8 (&xa)[3]) __attribute__((always_inline)) { ws_x_frag<WF3_XLP>(Xl, xbuf, s, li, lq, xa); };
  // one 16 x 16 block of h0 (row block s, column block cb of this wave) -> global (fp32), the three planes of LDS image `buf`, mask nibbles
  auto prod_block = [&](int g, int buf, int par, int s, int cb, const hx8 (&xa)[3]) __attribute__((always_inline)) {
    hx_t* dh = Ah + (long)buf * 3 * WS_ROWS * WS_PITCH;
    const int r = 16 * s + li;
    const long m = (long)g * WS_ROWS + r;
    f32x4 v;
    const unsigned int nib0 = ws_h0_block(b0[cb], xa, v);
    const int k = ncol0 + 16 * cb + 4 * lq;                              // h0 columns k .. k + 3 of row r
    if constexpr (XS) *(f32x4*)&y0b[m * y0p + k] = v;
    hx4 h, mm, l;
    orl_split4x3(v, h, mm, l);
    const int o = ws_a_off(r, k >> 2);
    *(hx4*)(dh + o) = h;
    *(hx4*)(dh + WS_ROWS * WS_PITCH + o) = mm;
    *(hx4*)(dh + 2 * WS_ROWS * WS_PITCH + o) = l;
    nbs0[(par * WS_ROWS + r) * WS_NBP + (k >> 2)] = (unsigned char)nib0;
  };
  auto produce = [&](int g, int buf, int xbuf, int par) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < WS_SUB; ++s) {
      hx8 xa[3];
      prod_x(xbuf, s, xa);
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) prod_block(g, buf, par, s, cb, xa);
    }
  };
  auto finish0 = [&](int g, int par) __attribute__((always_inline)) {    // after the barrier that follows produce(g): pack the h0 mask (half 0 only)
    if (tid < WS_ROWS * 8 && half == 0) {
      const int row = tid >> 3, wd = tid & 7;
      const unsigned int word = ws_pack_nibbles(nbs0 + (par * WS_ROWS + row) * WS_NBP + 8 * wd);
      p.mb0.p[z0 * p.mb0.s0 + z1 * p.mb0.s1 + ((long)g * WS_ROWS + row) * p.mb0_g + wd] = word;
    }
  };
  // the epilogue of one 16 x 16 block of h1 (row block s): bias, ReLU, tail partial sum, 4 mask bits -> LDS
  auto epi_block = [&](const f32x4& a, int g, int par, int s) __attribute__((always_inline)) {
    if constexpr (DG) {                                                  // gradient epilogue: ReLU mask of the receiving activation from its packed bits
      const long m = (long)g * WS_ROWS + 16 * s + li;
      const unsigned int nib = dmg[m * p.dm_g + (ncol1 >> 5)] >> ((ncol1 & 31) + 4 * lq);
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = ((nib >> r) & 1u) ? a[r] * inv_sc : 0.f;
      *(f32x4*)&Yg[m * p.y_pitch + ncol1 + 4 * lq] = v;
      return;
    }
    const f32x4 bq = *(const f32x4*)&cst[ncol1 + 4 * lq], twq = *(const f32x4*)&cst[WS_N + ncol1 + 4 * lq];
    f32x4 v = a * inv_sc + bq;
    const unsigned int nib = orl_relu_mask4(v);
    if constexpr (SY) *(f32x4*)&Yg[((long)g * WS_ROWS + 16 * s + li) * p.y_pitch + ncol1 + 4 * lq] = v;
    nbs[(par * WS_ROWS + 16 * s + li) * WS_NBP + 4 * wave + lq] = (unsigned char)nib;
    if constexpr (TQ) {
      float part = (v[0] * twq[0] + v[1] * twq[1]) + (v[2] * twq[2] + v[3] * twq[3]);
      part += __shfl_xor(part, 16);
      part += __shfl_xor(part, 32);
      (qs + (par * WS_NW + wave) * WS_ROWS)[16 * s + li] = part;         // all four lq lanes hold the same sum
    }
  };
  auto finish = [&](int g, int par) __attribute__((always_inline)) {     // after the barrier that follows the epilogue of group g
    if (!DG && tid < WS_ROWS * 4) {                                      // thread (row, word of this half): eight nibbles -> one 32-column mask word
      const int row = tid >> 2, wd = tid & 3, m = g * WS_ROWS + row;
      const unsigned int word = ws_pack_nibbles(nbs + (par * WS_ROWS + row) * WS_NBP + 8 * wd);
      p.mb.p[z0 * p.mb.s0 + z1 * p.mb.s1 + (long)m * p.mb_g + 4 * half + wd] = word;
    }
    if (TQ && tid >= WS_NT - WS_ROWS) {                                  // eight column-slice partial sums per row, fixed order
      const int row = tid - (WS_NT - WS_ROWS), m = g * WS_ROWS + row;
      const float q = ws_tail_sum(qs + par * WS_NW * WS_ROWS + row, tbias);
      tqo[(long)m * tqsm] = q;
    }
  };

  const int g0 = blockIdx.x, gs = gridDim.x;
  if (g0 >= p.groups) return;
  if constexpr (L0) {
    for (int e = tid; e < 2 * WS_ROWS * WF3_XLP; e += WS_NT) Xl[e] = 0.f;  // columns >= x0_pitch stay zero
    loadX(g0);
    __syncthreads();
    storeX(0);
    if (g0 + gs < p.groups) loadX(g0 + gs);
    __syncthreads();
    produce(g0, 0, 0, 0);
    if (g0 + gs < p.groups) storeX(1);
    if (g0 + 2 * gs < p.groups) loadX(g0 + 2 * gs);
    __syncthreads();
    finish0(g0, 0);
  } else {
#pragma unroll
    for (int i = 0; i < WS_LD; ++i) load_piece(g0, i);
#pragma unroll
    for (int i = 0; i < WS_LD; ++i) store_piece(0, i);
    if (g0 + gs < p.groups) {
#pragma unroll
      for (int i = 0; i < WS_LD; ++i) load_piece(g0 + gs, i);
    }
    __syncthreads();
  }

  // Software pipeline as in ws_fwd_kernel: iteration `it` multiplies group g out of LDS buffer it & 1 while the epilogue of the PREVIOUS group and
  // the first layer of the NEXT one run, cut into pieces, in the shadow of its MFMAs.
  f32x4 pacc[WS_SUB];
  auto iteration = [&](int g, int it, bool first, bool steady) __attribute__((always_inline)) {
    const int buf = it & 1;
    const hx_t* ah = Ah + (long)buf * 3 * WS_ROWS * WS_PITCH;
    const hx_t* am = ah + WS_ROWS * WS_PITCH;
    const hx_t* al = am + WS_ROWS * WS_PITCH;
    f32x4 acc[WS_SUB];
#pragma unroll
    for (int s = 0; s < WS_SUB; ++s) acc[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
    hx8 fxa[3];
    // steady state, one piece per k step (fenced with that step's 12 MFMAs): 0, 1 the two epilogue blocks of the previous group; 2 .. 5 the four
    // first-layer blocks of the next group; 6 the narrow rows of the group after next
    auto piece = [&](int ks) __attribute__((always_inline)) {
      const int par = (it - 1) & 1;
      if (ks < 2) epi_block(pacc[ks], g - gs, par, ks);
      else if (ks < 6) {
        if constexpr (L0) {
          const int s = (ks - 2) >> 1, cb = (ks - 2) & 1;
          if (cb == 0) prod_x((it + 1) & 1, s, fxa);
          prod_block(g + gs, buf ^ 1, (it + 1) & 1, s, cb, fxa);
        } else {                                                         // the staging register is refilled right after it was written to LDS
          store_piece(buf ^ 1, ks - 2);
          load_piece(g + 2 * gs, ks - 2);
        }
      } else if (L0 && ks == 6) { storeX(it & 1); loadX(g + 3 * gs); }
    };
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      hx8 fah[WS_SUB], fam[WS_SUB], fal[WS_SUB];
#pragma unroll
      for (int s = 0; s < WS_SUB; ++s) {
        const int o = ws_a_frag(s, li, 4 * ks + lq);
        fah[s] = *(const hx8*)&ah[o]; fam[s] = *(const hx8*)&am[o]; fal[s] = *(const hx8*)&al[o];
      }
      // smallest terms first; operands swapped: D[n][m], lane holds C[m = li][n = 4 lq + r]
#pragma unroll
      for (int s = 0; s < WS_SUB; ++s) acc[s] = ORL_MFMA_16x16x32(bl[ks], fah[s], acc[s]);
#pragma unroll
      for (int s = 0; s < WS_SUB; ++s) acc[s] = ORL_MFMA_16x16x32(bh[ks], fal[s], acc[s]);
#pragma unroll
      for (int s = 0; s < WS_SUB; ++s) acc[s] = ORL_MFMA_16x16x32(bm[ks], fam[s], acc[s]);
#pragma unroll
      for (int s = 0; s < WS_SUB; ++s) acc[s] = ORL_MFMA_16x16x32(bm[ks], fah[s], acc[s]);
#pragma unroll
      for (int s = 0; s < WS_SUB; ++s) acc[s] = ORL_MFMA_16x16x32(bh[ks], fam[s], acc[s]);
#pragma unroll
      for (int s = 0; s < WS_SUB; ++s) acc[s] = ORL_MFMA_16x16x32(bh[ks], fah[s], acc[s]);
      if (steady) {
        piece(ks);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (!steady) {
      if (!first) {
#pragma unroll
        for (int s = 0; s < WS_SUB; ++s) epi_block(pacc[s], g - gs, (it - 1) & 1, s);
      }
      if constexpr (L0) {
        // X rows of group g + gs sit in Xl[(it + 1) & 1] (written one iteration ago); rows of g + 2 gs are in registers
        if (g + gs < p.groups) produce(g + gs, buf ^ 1, (it + 1) & 1, (it + 1) & 1);
        if (g + 2 * gs < p.groups) storeX(it & 1);
        if (g + 3 * gs < p.groups) loadX(g + 3 * gs);
      } else {
        if (g + gs < p.groups) {
#pragma unroll
          for (int i = 0; i < WS_LD; ++i) store_piece(buf ^ 1, i);
        }
        if (g + 2 * gs < p.groups) {
#pragma unroll
          for (int i = 0; i < WS_LD; ++i) load_piece(g + 2 * gs, i);
        }
      }
    }
    __syncthreads();
    if (!first) finish(g - gs, (it - 1) & 1);
    if (L0 && (steady || g + gs < p.groups)) finish0(g + gs, (it + 1) & 1);
#pragma unroll
    for (int s = 0; s < WS_SUB; ++s) pacc[s] = acc[s];
  };
  int g = g0, it = 0;
  iteration(g, it, true, false);
  g += gs; ++it;
  while (g + 3 * gs < p.groups) {
    iteration(g, it, false, true);
    g += gs; ++it;
  }
  while (g < p.groups) {
    iteration(g, it, false, false);
    g += gs; ++it;
  }
  // drain: the last group's epilogue
#pragma unroll
  for (int s = 0; s < WS_SUB; ++s) epi_block(pacc[s], g - gs, (it - 1) & 1, s);
  __syncthreads();
  finish(g - gs, (it - 1) & 1);
}

#define WS_FWD3_ROW(TQ, SY, XS, L0, DG) {"ws_fwd3<" #TQ "," #SY "," #XS "," #L0 "," #DG ">", (const void*)ws_fwd3_kernel<TQ, SY, XS, L0, DG>, ws_fwd3_lds_bytes()}
const WsTable& ws_fwd3_table() {
  static const WsFlavour rows[] = {WS_FWD3_ROW(1, 0, 1, 1, 0), WS_FWD3_ROW(1, 1, 1, 1, 0), WS_FWD3_ROW(0, 1, 1, 1, 0), WS_FWD3_ROW(1, 0, 0, 1, 0), WS_FWD3_ROW(0, 1, 0, 1, 0),
                                               WS_FWD3_ROW(1, 0, 0, 0, 0), WS_FWD3_ROW(1, 1, 0, 0, 0), WS_FWD3_ROW(0, 1, 0, 0, 0), WS_FWD3_ROW(0, 1, 0, 0, 1)};
  static const WsTable t = {rows, 9};
  return t;
}

int ws_fwd3_flavour(const WsFwdP& p) {
  const bool tq = p.tq.p != nullptr, sy = p.Y.p != nullptr, xs = !p.x0_discard;
  if (p.dmask.p) return sy ? 8 : -1;                  // plain dgrad mode
  if (!tq && !sy) return -1;
  if (!p.X0.p) return tq ? (sy ? 6 : 5) : 7;          // no fused first layer: the input rows are staged from HBM
  if (xs) return tq ? (sy ? 1 : 0) : 2;
  return tq ? (sy ? -1 : 3) : 4;                      // h0 discarded: forward-only passes (tail alone, or the activation alone)
}

hipError_t launch_ws_fwd3(WsFwdP p, int nz, int per_z, hipStream_t st) {
  p.groups = p.M / WS_ROWS;
  static const hipError_t attr_err = ws_table_attrs(ws_fwd3_table());
  if (attr_err != hipSuccess) return attr_err;
  return ws_table_launch(ws_fwd3_table(), ws_fwd3_flavour(p), dim3(per_z, 2, nz), p, st);
}

}  // namespace orl
