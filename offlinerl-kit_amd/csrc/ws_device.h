// ws_device.h — the device blocks that several weight-stationary kernels (ws_fwd.hip, ws_fwd3.hip, ws_dgrad.hip, ws_dgrad3.hip, ws_wgrad.hip) share:
// each exists once, here, so that kernels which must agree bit for bit (the forward's h0 and the wgrad's recomputed h0; the two- and three-plane
// forward's mask words and tail sums) agree because they call the same function.  Every function is forced inline and takes its operands by
// value or reference -- the kernels' lambdas bind their locals to them in one line; nothing here changes a pipeline, an LDS layout or the order
// of floating-point operations.  Templates on NPL: the number of 16-bit planes (2: hi + lo, 3: hi + mid + lo; plane 0 = hi, NPL - 1 = lo);
// the exact-fp32 kernels have overloads on f32x4 operands.
#pragma once
#include "ws_gemm.h"

namespace orl {

__device__ inline void ws_split8(const f32x4& a, const f32x4& b, hx8& h, hx8& l) {
  hx4 ha, la, hb, lb;
  orl_split4(a, ha, la);
  orl_split4(b, hb, lb);
  h = __builtin_shufflevector(ha, hb, 0, 1, 2, 3, 4, 5, 6, 7);
  l = __builtin_shufflevector(la, lb, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ inline void ws_split8x3(const f32x4& a, const f32x4& b, hx8& h, hx8& m, hx8& l) {
  hx4 ha, ma, la, hb, mb, lb;
  orl_split4x3(a, ha, ma, la);
  orl_split4x3(b, hb, mb, lb);
  h = __builtin_shufflevector(ha, hb, 0, 1, 2, 3, 4, 5, 6, 7);
  m = __builtin_shufflevector(ma, mb, 0, 1, 2, 3, 4, 5, 6, 7);
  l = __builtin_shufflevector(la, lb, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ void ws_split8(const f32x4& a, const f32x4& b, hx8 (&pl)[2]) { ws_split8(a, b, pl[0], pl[1]); }
__device__ __forceinline__ void ws_split8(const f32x4& a, const f32x4& b, hx8 (&pl)[3]) { ws_split8x3(a, b, pl[0], pl[1], pl[2]); }

// ---- the swizzled A image [row][WS_PITCH] of 16-bit elements (ws_fwd, ws_fwd3, ws_dgrad, ws_dgrad3) ----
// The 16-byte chunk c = k / 8 of row r lives at chunk c ^ (r & 15): ds_read_b128 of a fragment column is then conflict-free for the hardware's
// 16-lane groups (which mix lanes of two neighbouring chunks), and the 8-byte staging stores stay so too.
// Offset of the four elements k = 4 kq .. 4 kq + 3 of row r (an 8-byte store):
__device__ __forceinline__ int ws_a_off(int r, int kq) { return r * WS_PITCH + ((((kq >> 1) ^ (r & 15)) << 3) | ((kq & 1) << 2)); }
// Offset of the fragment (row 16 s + li, chunk c) a lane reads with ds_read_b128:
__device__ __forceinline__ int ws_a_frag(int s, int li, int c) { return (16 * s + li) * WS_PITCH + ((c ^ li) << 3); }

// ---- resident weight fragments of the forward kernels: the raw fp32 values W[n = ncol0 + 16 cb + li][k = 32 ks + 8 lq .. + 7] ----
// The layout test (w_sk == 1) sits OUTSIDE the fragment loops and all loads of a layout are issued before the first conversion: with the test
// inside, every fragment was its own load -> wait -> split round trip (16 - 32 serialized L2 latencies = the ~20 us floor of a launch).
template <int CB>
__device__ __forceinline__ void ws_w_frag_load(const float* __restrict__ Wg, long w_sn, long w_sk, int ncol0, int li, int lq, f32x4 (&raw)[CB][8][2]) {
  if (w_sk == 1) {                                                       // nn.Linear (out, in): k-contiguous rows
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const float* src = Wg + (long)(ncol0 + 16 * cb + li) * w_sn + (32 * ks + 8 * lq);
        raw[cb][ks][0] = *(const f32x4*)src; raw[cb][ks][1] = *(const f32x4*)(src + 4);
      }
  } else {                                                               // EnsembleLinear (in, out): eight strided loads per fragment, once per workgroup
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const float* src = Wg + (long)(ncol0 + 16 * cb + li) * w_sn + (long)(32 * ks + 8 * lq) * w_sk;
#pragma unroll
        for (int j = 0; j < 4; ++j) { raw[cb][ks][0][j] = src[(long)j * w_sk]; raw[cb][ks][1][j] = src[(long)(4 + j) * w_sk]; }
      }
  }
}

// ---- the fused / recomputed first layer (ws_fwd<., L0>, ws_fwd3<., L0>, ws_wgrad<4>, ws_wgrad32<4>) ----
// One value of W0'[n][k], K = 32: W0[n][k] for k < in0, b0[n] (= bn) at k == in0, 0 beyond.  Clamped addresses and 0 / 1 factors, not guarded
// loads (each guard is a branch with its own wait: twelve serialized round trips per workgroup and problem).  0 * w is exact for finite
// weights; a diverged run's Inf / NaN would spread into the zero columns.  P: WsFwdP or WsWgradP.
template <class P>
__device__ __forceinline__ float ws_w0_value(const P& p, const float* __restrict__ W0g, int n, int k, float bn) {
  const float w = W0g[(long)n * p.w0_sn + (long)(k < p.in0 ? k : p.in0 - 1) * p.w0_sk];
  return (k < p.in0 ? 1.f : 0.f) * w + (k == p.in0 ? 1.f : 0.f) * bn;
}
// split planes: lane (li, lq) supplies W0'[n][k = 8 lq .. 8 lq + 7] (unscaled)
template <int NPL, class P>
__device__ __forceinline__ void ws_w0_frag(const P& p, const float* __restrict__ W0g, int n, int lq, float bn, hx8 (&pl)[NPL]) {
  f32x4 a, b;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = ws_w0_value(p, W0g, n, 8 * lq + j, bn);
    b[j] = ws_w0_value(p, W0g, n, 8 * lq + 4 + j, bn);
  }
  ws_split8(a, b, pl);
}
// exact fp32: k = 16 t + 4 lq + e (element e of the float4 = MFMA k step e of block t)
template <class P>
__device__ __forceinline__ void ws_w0_frag(const P& p, const float* __restrict__ W0g, int n, int lq, float bn, f32x4 (&w)[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) w[t][j] = ws_w0_value(p, W0g, n, 16 * t + 4 * lq + j, bn);
}

// Narrow-input staging: element e = tid + WS_NT i of the [WS_ROWS][x0_pitch] rows of a group -> (row xr, column xc) of the LDS rows; surplus
// threads get column 32, a pad slot that is never read (rows are consumed as 32 columns).  `on` = the kernel has a first layer at all.
template <int XI>
__device__ __forceinline__ void ws_x_index(bool on, int tid, int x0_pitch, int xe, int (&xr)[XI], int (&xc)[XI]) {
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    const int e = tid + WS_NT * i;
    xr[i] = on ? e / (on ? x0_pitch : 1) : 0; xc[i] = on ? e - xr[i] * x0_pitch : 0;
    if (on && e >= xe) { xr[i] = 0; xc[i] = 32; }
  }
}
template <int XI>
__device__ __forceinline__ void ws_x_load(const float* __restrict__ X0g, int g, int xe, int tid, float (&sx)[XI]) {
#pragma unroll
  for (int i = 0; i < XI; ++i) { const int e = tid + WS_NT * i; sx[i] = X0g[(long)g * xe + (e < xe ? e : xe - 1)]; }   // clamped, not predicated
}
// The narrow rows are split ONCE here, by the staging thread of an element, into NPL planes (16-bit slots 0..31, 32..63 (, 64..95) of the row of
// XLP floats) -- not by every wave in ws_x_frag (eight times the same vector instructions per group, and vector instructions do not overlap
// with a SIMD's MFMAs).  Surplus threads write the pad slots 32 NPL ...  NPL = 0: the fp32 rows themselves (pad column 32).  The ones column
// (bias) sits at in0.
template <int NPL, int XLP, int XI>
__device__ __forceinline__ void ws_x_store(float* Xl, int buf, int in0, const int (&xr)[XI], const int (&xc)[XI], const float (&sx)[XI]) {
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    const float x = (xc[i] == in0) ? 1.0f : sx[i];
    if constexpr (NPL == 0) Xl[(buf * WS_ROWS + xr[i]) * XLP + xc[i]] = x;
    else {
      hx_t* row = (hx_t*)(Xl + (buf * WS_ROWS + xr[i]) * XLP);
      const bool pad = xc[i] >= 32;
      if constexpr (NPL == 2) {
        hx_t hh, ll;
        orl_split1(x, hh, ll);
        row[pad ? 64 : xc[i]] = hh;
        row[pad ? 65 : 32 + xc[i]] = ll;
      } else {
        hx_t hh, mm, ll;
        orl_split1x3(x, hh, mm, ll);
        row[pad ? 96 : xc[i]] = hh;
        row[pad ? 97 : 32 + xc[i]] = mm;
        row[pad ? 98 : 64 + xc[i]] = ll;
      }
    }
  }
}
// the A fragments of row block s of the rows staged in Xl[xbuf]: lane (li, lq) reads k = 8 lq .. + 7 of row 16 s + li from every plane
template <int XLP, int NPL>
__device__ __forceinline__ void ws_x_frag(const float* Xl, int xbuf, int s, int li, int lq, hx8 (&x)[NPL]) {
  const hx_t* xrow = (const hx_t*)(Xl + (xbuf * WS_ROWS + 16 * s + li) * XLP) + 8 * lq;
#pragma unroll
  for (int pl = 0; pl < NPL; ++pl) x[pl] = *(const hx8*)(xrow + 32 * pl);
}
template <int XLP>
__device__ __forceinline__ void ws_x_frag(const float* Xl, int xbuf, int s, int li, int lq, f32x4 (&x)[2]) {      // exact fp32: k = 16 t + 4 lq + e
  const float* xrow = Xl + (xbuf * WS_ROWS + 16 * s + li) * XLP + 4 * lq;
  x[0] = *(const f32x4*)xrow; x[1] = *(const f32x4*)(xrow + 16);
}
// One 16 x 16 block of h0 = relu(X0 W0'^T): the products smallest terms first (operands swapped: D[n][m], the lane holds C[m = li][n = 4 lq + r]),
// then the ReLU; returns the block's four mask bits.  The forward kernels and the recomputing wgrads call THIS, so their h0 agree bit for bit.
__device__ __forceinline__ unsigned int ws_h0_block(const hx8 (&b0)[2], const hx8 (&x)[2], f32x4& v) {
  v = (f32x4){0.f, 0.f, 0.f, 0.f};
  v = ORL_MFMA_16x16x32(b0[1], x[0], v);
  v = ORL_MFMA_16x16x32(b0[0], x[1], v);
  v = ORL_MFMA_16x16x32(b0[0], x[0], v);
  return orl_relu_mask4(v);
}
__device__ __forceinline__ unsigned int ws_h0_block(const hx8 (&b0)[3], const hx8 (&x)[3], f32x4& v) {
  v = (f32x4){0.f, 0.f, 0.f, 0.f};
  v = ORL_MFMA_16x16x32(b0[2], x[0], v);
  v = ORL_MFMA_16x16x32(b0[0], x[2], v);
  v = ORL_MFMA_16x16x32(b0[1], x[1], v);
  v = ORL_MFMA_16x16x32(b0[1], x[0], v);
  v = ORL_MFMA_16x16x32(b0[0], x[1], v);
  v = ORL_MFMA_16x16x32(b0[0], x[0], v);
  return orl_relu_mask4(v);
}
__device__ __forceinline__ unsigned int ws_h0_block(const f32x4 (&b0)[2], const f32x4 (&x)[2], f32x4& v) {
  v = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) v = __builtin_amdgcn_mfma_f32_16x16x4f32(b0[t][e], x[t][e], v, 0, 0, 0);
  return orl_relu_mask4(v);
}

// ---- epilogue pieces of the forward kernels ----
// eight mask nibbles (one per byte, 4 bits per (row, 4 columns)) -> one 32-column mask word
__device__ __forceinline__ unsigned int ws_pack_nibbles(const unsigned char* nb8) {
  const unsigned int* nb = (const unsigned int*)nb8;
  const unsigned int d0 = nb[0], d1 = nb[1];
  const unsigned int lo16 = (d0 & 0xFu) | ((d0 >> 4) & 0xF0u) | ((d0 >> 8) & 0xF00u) | ((d0 >> 12) & 0xF000u);
  const unsigned int hi16 = (d1 & 0xFu) | ((d1 >> 4) & 0xF0u) | ((d1 >> 8) & 0xF00u) | ((d1 >> 12) & 0xF000u);
  return lo16 | (hi16 << 16);
}
// the tail of one row: the eight waves' column-slice partial sums q8[w * WS_ROWS], added to the bias in a fixed order
__device__ __forceinline__ float ws_tail_sum(const float* q8, float tbias) {
  float a = tbias;
#pragma unroll
  for (int w = 0; w < WS_NW; ++w) a += q8[w * WS_ROWS];
  return a;
}

// ---- the dW0 / db0 slab of the dgrad kernels, after the row loop ----
// one 16 x 16 block of dW0^T: the lane holds rows c = c0 + 4 lq + r of column n; row in0 is the bias gradient, rows beyond it do not exist
__device__ __forceinline__ void ws_w0_slab_block(const WsDgradP& p, float* wo, float* bo, const f32x4& d, int c0, int lq, int n, float scale) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = c0 + 4 * lq + r;
    if (c < p.in0) wo[(long)n * p.o_sr + (long)c * p.o_sc] = d[r] * scale;
    else if (c == p.in0) bo[n] = d[r] * scale;
  }
}

}  // namespace orl
