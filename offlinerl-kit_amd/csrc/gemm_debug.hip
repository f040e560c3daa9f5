// gemm_debug.hip — the unit-test taps of the tiled GEMM (orl_debug_gemm, orl_debug_gemm_ex, orl_debug_gemm_time; include/orl_engine.h):
// launches of the kernels instantiated in gemm_inst_*.hip on host arrays.  Host code only.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "debug_tap.h"
#include "devobj.h"
#include "gemm.h"

// what orl_debug_gemm_ex reports about the tile it will run
namespace orl {
namespace {

struct ExTile { int TM, TN, TK, NT; bool epi_fits; };
template <class CFG>
static ExTile ex_tile_of(int prec) {
  return {CFG::TM, CFG::TN, CFG::kTK, CFG::NT,
          CFG::epi_lds_bytes() <= CFG::epi_lds_limit(prec) && (CFG::NT % (CFG::TN / 4)) == 0};      // the kernel's LDS_EPI_FITS
}
// tile shape that runs (launch_cfg_prec: a tile whose three-plane buffers exceed the LDS goes to the 128 x 128 one)
static int ex_run_cfg(int cfg, int prec) {
  if (prec == P_SPLIT3 && cfg == CFG_WG && CfgWg::lds_bytes(P_SPLIT3) > (size_t)160 * 1024) return CFG_SQ;
  return cfg;
}
static ExTile ex_tile(int cfg, int prec) {
  switch (cfg) {
    case CFG_BIG: return ex_tile_of<CfgBig>(prec);
    case CFG_MID: return ex_tile_of<CfgMid>(prec);
    case CFG_SMALL: return ex_tile_of<CfgSmall>(prec);
    case CFG_SQ: return ex_tile_of<CfgSq>(prec);
    case CFG_SQ8: return ex_tile_of<CfgSq8>(prec);
    case CFG_WG: return ex_tile_of<CfgWg>(prec);
    default: return ex_tile_of<CfgTall>(prec);
  }
}

}  // namespace
}  // namespace orl

using namespace orl;

extern "C" {

// kernel unit test: C = op(A) op(B) through one tile configuration.
//  mode 0: forward   C[M,N] = relu(A[M,K] B[N,K]^T + v0[N])
//  mode 1: dgrad     C[M,N] = A[M,K] Bm[K,N], masked by v0 viewed [M,N] (>0)
//  mode 2: wgrad     A is [K,M], B is [K,N]: C = [A^T B (M*N) | column sums of A (M)]; split-K slabs summed on host
//  mode 3: rank-1 dgrad  A_eff[m,k] = A[m,k]>0 ? v0[m]*v1[k] : 0 ; C = A_eff Bm[K,N]
//  mode 4: rank-1 wgrad  A_eff[k,m] = A[k,m]>0 ? v0[k]*v1[m] : 0 ; output like mode 2
int orl_debug_gemm(int cfg, int mode, int M, int N, int K, const float* A, const float* Bh, const float* v0, const float* v1,
                   float* C, int ksplit, int precision) {
  if (precision < 0 || precision > 2) return fail("precision must be 0, 1 or 2");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device");
  hipStream_t st = nullptr;
  const bool wg = (mode == 2 || mode == 4);
  const long nA = (long)M * K, nB = (long)N * K;
  const long nC = wg ? (long)M * (N + 1) : (long)M * N;
  const long n0 = (mode == 0) ? N : (mode == 1 ? (long)M * N : (mode == 3 ? M : (mode == 4 ? K : 0)));
  const long n1 = (mode == 3) ? K : (mode == 4 ? M : 0);
  if (ksplit < 1) ksplit = 1;
  TapDev dev;      // (an error return frees what was allocated)
  char* in[4];
  float* dC = nullptr;
  if (tap_upload(dev, {{A, nullptr, nA}, {Bh, nullptr, nB}, {n0 ? v0 : nullptr, nullptr, n0}, {n1 ? v1 : nullptr, nullptr, n1}}, in, "orl_debug_gemm") ||
      dev.alloc(&dC, nC * ksplit, "orl_debug_gemm")) return -1;
  float *dA = (float*)in[0], *dB = (float*)in[1], *d0 = (float*)in[2], *d1 = (float*)in[3];
  ORL_HIP(hipMemset(dC, 0, sizeof(float) * nC * ksplit));
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.nz1 = 1; p.ksplit = ksplit; p.C = dC; p.c_ks = nC; p.c_sn = 1;
  const bool fs = (cfg & 16) != 0;      // bit 4 of cfg forces the scalar loaders (unit tests cover both paths)
  cfg &= 15;
  p.a_rlim = M & ~3; p.b_rlim = N & ~3;
  hipError_t err = hipSuccess;
  if (mode == 0) {
    p.A = {dA, 0, 0}; p.a_sr = K; p.a_sk = 1; p.B = {dB, 0, 0}; p.b_sr = K; p.b_sk = 1;
    p.M = M; p.N = N; p.K = K; p.c_sr = N; p.bias = {d0, 0, 0};
    err = launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_RELU>(cfg, p, 1, st, false, fs, precision);
  } else if (mode == 1 || mode == 3) {
    p.A = {dA, 0, 0}; p.a_sr = K; p.a_sk = 1; p.B = {dB, 0, 0}; p.b_sr = 1; p.b_sk = N;
    p.M = M; p.N = N; p.K = K; p.c_sr = N;
    if (mode == 1) { p.aux = {d0, 0, 0}; p.aux_sr = N; err = launch_gemm<PA_PLAIN, PB_PLAIN, E_MASK>(cfg, p, 1, st, false, fs, precision); }
    else { p.rowv = {d0, 0, 0}; p.colv = {d1, 0, 0}; p.a_trans = 0; err = launch_gemm<PA_RANK1, PB_PLAIN, E_PLAIN>(cfg, p, 1, st, false, fs, precision); }
  } else {
    p.A = {dA, 0, 0}; p.a_sr = 1; p.a_sk = M; p.B = {dB, 0, 0}; p.b_sr = 1; p.b_sk = N;
    p.M = M; p.N = N; p.K = K; p.c_sr = N; p.ones_row = 1 << 30;
    p.bias_out = dC + (long)M * N; p.bo_ks = nC;
    if (mode == 2) err = launch_gemm<PA_PLAIN, PB_PLAIN, E_WGRAD>(cfg, p, 1, st, false, fs, precision);
    else { p.rowv = {d0, 0, 0}; p.colv = {d1, 0, 0}; p.a_trans = 1; err = launch_gemm<PA_RANK1, PB_PLAIN, E_WGRAD>(cfg, p, 1, st, false, fs, precision); }
  }
  if (err != hipSuccess) return fail(std::string("debug gemm launch: ") + hipGetErrorString(err));
  ORL_HIP(hipDeviceSynchronize());
  std::vector<float> tmp(nC * ksplit);
  ORL_HIP(hipMemcpy(tmp.data(), dC, sizeof(float) * nC * ksplit, hipMemcpyDeviceToHost));
  for (long i = 0; i < nC; ++i) {
    float s = 0.f;
    for (int k = 0; k < ksplit; ++k) s += tmp[k * nC + i];
    C[i] = s;
  }
  return 0;
}

// ---- the wider unit-test tap: every epilogue / tile shape / batch mapping / pitch / side output of the template ----
int orl_debug_gemm_ex(orl_gemm_ex* a) {
  if (!a) return fail("orl_debug_gemm_ex: null arguments");
  const bool fs = (a->cfg & 16) != 0;
  const int cfg = a->cfg & 15;
  const int epi = a->epi, M = a->M, N = a->N, K = a->K, nz0 = a->nz0, nz1 = a->nz1, prec = a->precision;
  // ---- argument checks: all of them before the first HIP call ----
  if ((a->cfg & ~31) || cfg > CFG_WG) return fail("orl_debug_gemm_ex: cfg must be 0..6, plus 16 for the scalar loaders");
  if (prec < 0 || prec > 2) return fail("orl_debug_gemm_ex: precision must be 0, 1 or 2");
  if (epi < E_PLAIN || epi > E_LEAKY_MASK) return fail("orl_debug_gemm_ex: epi must be 0..8");
  if (a->layout < 0 || a->layout > 2) return fail("orl_debug_gemm_ex: layout must be 0, 1 or 2");
  if ((epi == E_WGRAD) != (a->layout == 2)) return fail("orl_debug_gemm_ex: layout 2 goes with the weight-gradient epilogue and with no other");
  if (a->pa < 0 || a->pa > 2) return fail("orl_debug_gemm_ex: pa must be 0, 1 or 2");
  if (a->pa == 1 && epi != E_PLAIN && epi != E_MASK && epi != E_WGRAD) return fail("orl_debug_gemm_ex: the rank-1 operand is instantiated for epi 0, 3 and 4 only");
  if (a->pa == 2 && epi != E_MASK) return fail("orl_debug_gemm_ex: the rank-1 operand from mask words is instantiated for epi 3 only");
  if (M < 1 || N < 1 || K < 1 || M > 65536 || N > 65536 || K > 65536) return fail("orl_debug_gemm_ex: M, N, K must be 1..65536");
  if (nz0 < 1 || nz1 < 1 || (long)nz0 * nz1 > 4096) return fail("orl_debug_gemm_ex: nz0 x nz1 must be 1..4096");
  if (a->ksplit < 1 || a->ksplit > 64) return fail("orl_debug_gemm_ex: ksplit must be 1..64");
  if (a->ksplit > 1 && epi != E_WGRAD) return fail("orl_debug_gemm_ex: split-K slabs exist for the weight-gradient epilogue only");
  const int ksplit = a->ksplit, nz = nz0 * nz1;
  const bool wg = epi == E_WGRAD;
  const bool bias_epi = epi == E_BIAS || epi == E_BIAS_RELU || epi == E_BIAS_SWISH || epi == E_BIAS_LEAKY;
  const bool aux_epi = epi == E_MASK || epi == E_SWISH_GRAD || epi == E_LEAKY_MASK;
  if (a->a_kpad && (a->layout == 2 || a->pa != 0)) return fail("orl_debug_gemm_ex: a_kpad is for a k-contiguous plain A operand");
  if (a->c_trans && !wg) return fail("orl_debug_gemm_ex: the transposed store belongs to the weight-gradient epilogue");
  if (a->bias_out.host && !wg) return fail("orl_debug_gemm_ex: bias_out belongs to the weight-gradient epilogue");
  if (a->z_out.host && epi != E_BIAS_SWISH) return fail("orl_debug_gemm_ex: z_out belongs to the Swish forward epilogue");
  if (a->mb_out.host && epi != E_BIAS_RELU) return fail("orl_debug_gemm_ex: mask words are emitted by the ReLU forward epilogue only");
  if ((a->tq_out.host || a->tq_part.host || a->tq_w.host || a->tq_b.host) && epi != E_BIAS_RELU) return fail("orl_debug_gemm_ex: the fused tail belongs to the ReLU forward epilogue");
  if (a->aux_bits.host && (epi != E_MASK)) return fail("orl_debug_gemm_ex: aux_bits belongs to the mask epilogue");
  if ((a->w0_out.host || a->w0_bias.host || a->w0_x.host) && (epi != E_MASK)) return fail("orl_debug_gemm_ex: the fused layer-0 gradient belongs to the mask epilogue");
  if (a->c_null && !a->w0_out.host) return fail("orl_debug_gemm_ex: C may be left out only with the fused layer-0 gradient");
  if ((a->pa == 2) != (a->a_bits.host != nullptr)) return fail("orl_debug_gemm_ex: a_bits goes with pa 2 and with nothing else");
  if (a->pa == 2 && (fs || (cfg != CFG_BIG && cfg != CFG_SQ))) return fail("orl_debug_gemm_ex: the rank-1 operand from mask words runs on CFG_BIG and CFG_SQ with the vector loaders only");

  std::string why;
  const long k4 = (K + 3) & ~3;
  // operands
  if (a->pa != 2) {
    if (a->layout == 2) {
      if (a->A.pitch < M) return fail("orl_debug_gemm_ex: A's pitch is below its width (M)");
      // (the 4 x 4 block loader may read every row of four that starts inside the pitch: GemmP::a_rlim)
      if (!tap_fits(a->A, "A", (long)(K - 1) * a->A.pitch + std::max((long)M, (long)(a->A.pitch & ~3L)), nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
    } else {
      if (a->A.pitch < (a->a_kpad ? k4 : K)) return fail("orl_debug_gemm_ex: A's pitch is below its width (K, rounded up to 4 with a_kpad)");
      if (!tap_fits(a->A, "A", (long)(M - 1) * a->A.pitch + (a->a_kpad ? k4 : K), nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
    }
  }
  if (a->layout == 0) {
    if (a->B.pitch < K) return fail("orl_debug_gemm_ex: B's pitch is below its width (K)");
    if (!tap_fits(a->B, "B", (long)(N - 1) * a->B.pitch + K, nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
  } else {
    if (a->B.pitch < N) return fail("orl_debug_gemm_ex: B's pitch is below its width (N)");
    if (!tap_fits(a->B, "B", (long)(K - 1) * a->B.pitch + std::max((long)N, (long)(a->B.pitch & ~3L)), nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
  }
  if (bias_epi && !tap_fits(a->bias, "bias", N, nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
  if (aux_epi) {
    if (a->aux.pitch < N) return fail("orl_debug_gemm_ex: aux's pitch is below its width (N)");
    if (!tap_fits(a->aux, "aux", (long)(M - 1) * a->aux.pitch + N, nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
  }
  if (a->pa != 0) {
    const int nrow = a->layout == 2 ? K : M, ncol = a->layout == 2 ? std::max(M, (int)(a->A.pitch & ~3L)) : K;      // (the block loader reads colv like A's rows)
    if (!tap_fits(a->rowv, "rowv", nrow, nz0, nz1, 1, false, why) || !tap_fits(a->colv, "colv", ncol, nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
  }
  if (a->pa == 2) {
    if (K & 31) return fail("orl_debug_gemm_ex: the rank-1 operand from mask words needs K % 32 == 0");
    if (a->a_bits.pitch < K / 32) return fail("orl_debug_gemm_ex: a_bits' pitch is below its width (K / 32 words)");
    if (!tap_fits(a->a_bits, "a_bits", (long)(M - 1) * a->a_bits.pitch + K / 32, nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
  }
  // results
  const bool has_c = !a->c_null;
  const long c_rows = a->c_trans ? N : M, c_cols = a->c_trans ? M : N;
  if (has_c) {
    if (a->C.pitch < c_cols) return fail("orl_debug_gemm_ex: C's pitch is below its width");
    if (!tap_fits(a->C, "C", (c_rows - 1) * a->C.pitch + c_cols, nz0, nz1, ksplit, true, why)) return fail("orl_debug_gemm_ex: " + why);
  }
  if (a->z_out.host && a->z_out.n != a->C.n) return fail("orl_debug_gemm_ex: z_out has C's geometry, so it needs C's element count");
  if (a->bias_out.host && !tap_fits(a->bias_out, "bias_out", M, nz0, nz1, ksplit, true, why)) return fail("orl_debug_gemm_ex: " + why);

  // ---- the launch parameters, on any 16-byte aligned bases (alignment decides the paths; the device bases are 256-byte aligned) ----
  const ExTile t = ex_tile(ex_run_cfg(cfg, prec), prec);
  const int tiles_n = (N + t.TN - 1) / t.TN, tiles_m = (M + t.TM - 1) / t.TM;
  enum { B_A, B_B, B_BIAS, B_AUX, B_ROWV, B_COLV, B_XBITS, B_ABITS, B_TQW, B_TQB, B_W0X, B_C, B_ZOUT, B_BO, B_MB, B_TQO, B_TQP, B_W0O, B_W0B, B_COUNT };
  const orl_gemm_buf* bufs[B_COUNT] = {&a->A, &a->B, &a->bias, &a->aux, &a->rowv, &a->colv, &a->aux_bits, &a->a_bits, &a->tq_w, &a->tq_b, &a->w0_x,
                                       &a->C, &a->z_out, &a->bias_out, &a->mb_out, &a->tq_out, &a->tq_part, &a->w0_out, &a->w0_bias};
  auto params = [&](char* const* base) {
    auto fp = [&](int i) -> float* { return bufs[i]->host ? (float*)base[i] + (i == B_ZOUT ? a->C.off : bufs[i]->off) : nullptr; };
    auto zp = [&](int i) -> ZPtr { return ZPtr{fp(i), bufs[i]->s0, bufs[i]->s1}; };
    GemmP p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.N = N; p.K = K; p.nz1 = nz1; p.ksplit = ksplit;
    if (a->pa != 2) p.A = zp(B_A);
    if (a->layout == 2) { p.a_sr = 1; p.a_sk = a->A.pitch; p.a_rlim = (int)(a->A.pitch & ~3L); }      // rows that may be read: the engine passes the pitch too
    else { p.a_sr = a->pa == 2 ? K : a->A.pitch; p.a_sk = 1; }
    p.B = zp(B_B);
    if (a->layout == 0) { p.b_sr = a->B.pitch; p.b_sk = 1; }
    else { p.b_sr = 1; p.b_sk = a->B.pitch; p.b_rlim = (int)(a->B.pitch & ~3L); }
    p.C = has_c ? fp(B_C) : nullptr;
    p.c_s0 = a->C.s0; p.c_s1 = a->C.s1; p.c_ks = a->C.ks;
    if (a->c_trans) { p.c_sr = 1; p.c_sn = a->C.pitch; } else { p.c_sr = a->C.pitch; p.c_sn = 1; }
    if (bias_epi) p.bias = zp(B_BIAS);
    if (aux_epi) { p.aux = zp(B_AUX); p.aux_sr = a->aux.pitch; }
    if (a->pa != 0) { p.rowv = zp(B_ROWV); p.colv = zp(B_COLV); p.a_trans = a->layout == 2; }
    if (wg) {
      p.ones_row = 1 << 30;
      if (a->bias_out.host) { p.bias_out = fp(B_BO); p.bo_s0 = a->bias_out.s0; p.bo_s1 = a->bias_out.s1; p.bo_ks = a->bias_out.ks; }
    }
    if (a->z_out.host) p.z_out = fp(B_ZOUT);
    if (a->pa == 2) { p.a_bits = (const unsigned int*)fp(B_ABITS); p.ab_s0 = a->a_bits.s0; p.ab_s1 = a->a_bits.s1; p.ab_g = (int)a->a_bits.pitch; }
    return p;
  };
  char* fake[B_COUNT];
  for (int i = 0; i < B_COUNT; ++i) fake[i] = (char*)(uintptr_t)4096;
  GemmP p = params(fake);

  // what the launch will do: loaders (launch_gemm + launch_cfg), workgroup mapping (launch_inst), store path (the kernel's epilogue)
  int la = L_SCALAR, lb = L_SCALAR;
  a->r_la_pick = a->pa == 2 ? L_VECK : pick_loader(p.A, p.a_sr, p.a_sk, K, a->a_kpad != 0, p.a_rlim);
  a->r_lb_pick = pick_loader(p.B, p.b_sr, p.b_sk, K, false, p.b_rlim);
  if (a->pa == 2) {
    if (!rank1_bits_supported(cfg, p, fs)) return fail("orl_debug_gemm_ex: this rank-1 operand from mask words is refused by rank1_bits_supported (colv alignment, B's loader)");
    la = L_VECK; lb = a->r_lb_pick;
  } else if (!fs) {
    la = a->r_la_pick; lb = a->r_lb_pick;
    if (a->pa == 1) {
      if (la == L_VECK && (p.a_trans != 0 || !p.colv.vec4())) la = L_SCALAR;
      if (la == L_BLK4 && (p.a_trans != 1 || !p.colv.vec4())) la = L_SCALAR;
    }
    if (!((la == L_VECK && (lb == L_VECK || lb == L_BLK4 || lb == L_VECKU)) || (la == L_BLK4 && lb == L_BLK4))) {
      if (la == L_VECK) lb = L_SCALAR;
      else la = lb = L_SCALAR;
    }
  }
  a->r_cfg = ex_run_cfg(cfg, prec); a->r_la = la; a->r_lb = lb;
  {
    const char* f = getenv("ORL_GEMM_ZMAJOR_MAX");
    const int zm_max = f ? atoi(f) : 16, items = tiles_m * tiles_n * ksplit;
    a->r_zmajor = (nz >= 8 && items > 1 && items <= zm_max) ? 1 : 0;
  }

  // side outputs: each is granted only where the launch honours it
  a->r_mb = a->r_tq_parts = a->r_w0_slabs = a->r_aux_bits = a->r_a_bits = 0;
  const bool c_vec = has_c && p.c_sn == 1 && aligned16(p.C) && !(p.c_sr & 3) && !(p.c_s0 & 3) && !(p.c_s1 & 3);
  const bool lds_all = t.epi_fits && c_vec && !(N & 3) && (!bias_epi || p.bias.vec4());      // the LDS-staged store for every problem (float-aux terms below)
  if (a->mb_out.host) {
    const bool cap = ((t.TN / 4) % 8) == 0;      // the kernel's MB_CAP
    if (fs || !cap || !lds_all || !mb_supported(cfg, p)) return fail("orl_debug_gemm_ex: mask words need a tile with 8 lanes per 32 columns, N % 32 == 0, the vector loaders and 16-byte aligned C / bias (mb_supported)");
    if (a->mb_out.pitch < N / 32) return fail("orl_debug_gemm_ex: mb_out's pitch is below its width (N / 32 words)");
    if (!tap_fits(a->mb_out, "mb_out", (long)(M - 1) * a->mb_out.pitch + N / 32, nz0, nz1, 1, true, why)) return fail("orl_debug_gemm_ex: " + why);
    a->r_mb = 1;
  }
  if (a->tq_out.host || a->tq_part.host || a->tq_w.host || a->tq_b.host) {
    if (!a->tq_out.host || !a->tq_w.host || !a->tq_b.host) return fail("orl_debug_gemm_ex: the fused tail needs tq_w, tq_b and tq_out");
    if (!tap_fits(a->tq_w, "tq_w", N, nz0, nz1, 1, false, why) || !tap_fits(a->tq_b, "tq_b", 1, nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
    const int parts = (fs || !lds_all) ? 0 : tq_fused_parts(cfg, p, (const float*)fake[B_TQW] + a->tq_w.off, a->tq_w.s0, a->tq_w.s1);
    if (parts < 1) return fail("orl_debug_gemm_ex: the fused tail runs on CFG_BIG and CFG_SQ8 with N % 4 == 0, the vector loaders and 16-byte aligned C / bias / tail weights (tq_fused_parts)");
    if (a->tq_sm < 1) return fail("orl_debug_gemm_ex: tq_sm must be >= 1");
    if (!tap_fits(a->tq_out, "tq_out", (long)(M - 1) * a->tq_sm + 1, nz0, nz1, 1, true, why)) return fail("orl_debug_gemm_ex: " + why);
    if (parts > 1) {
      if (a->tq_part.pitch < M) return fail("orl_debug_gemm_ex: tq_part's pitch is below its width (M)");
      if (!tap_fits(a->tq_part, "tq_part", (long)(parts - 2) * a->tq_part.pitch + M, nz0, nz1, 1, true, why)) return fail("orl_debug_gemm_ex: " + why);
    }
    a->r_tq_parts = parts;
  }
  if (a->aux_bits.host) {
    if (a->aux_bits.pitch < (N + 31) / 32) return fail("orl_debug_gemm_ex: aux_bits' pitch is below its width ((N + 31) / 32 words)");
    if (!tap_fits(a->aux_bits, "aux_bits", (long)(M - 1) * a->aux_bits.pitch + (N + 31) / 32, nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
    if (!lds_all && !a->c_null) return fail("orl_debug_gemm_ex: the mask epilogue reads packed words only on the LDS-staged store (N % 4 == 0, 16-byte aligned C)");
  }
  if (a->w0_out.host || a->w0_bias.host || a->w0_x.host) {
    if (!a->w0_out.host || !a->w0_bias.host || !a->w0_x.host) return fail("orl_debug_gemm_ex: the fused layer-0 gradient needs w0_x, w0_out and w0_bias");
    if (a->w0_in < 1 || a->w0_x.pitch < 1 || a->w0_x.pitch > W0_XP) return fail("orl_debug_gemm_ex: w0_in and w0_x's pitch must be 1..28");
    if (!tap_fits(a->w0_x, "w0_x", (long)M * a->w0_x.pitch, nz0, nz1, 1, false, why)) return fail("orl_debug_gemm_ex: " + why);
    if (a->w0_bias.s0 != a->w0_out.s0 || a->w0_bias.ks != a->w0_out.ks) return fail("orl_debug_gemm_ex: w0_bias shares w0_out's s0 and slab stride");
    if (a->w0_out.pitch < a->w0_in) return fail("orl_debug_gemm_ex: w0_out's pitch is below its width (w0_in)");
    const bool cap = t.TN / (t.NT / 64) == 32 && t.TM % 16 == 0;      // the kernel's W0_CAP
    GemmP q = p;
    if (a->aux_bits.host) q.aux_bits = (const unsigned int*)fake[B_XBITS];
    const int slabs = (fs || !cap || !t.epi_fits || cfg != pick_cfg(M, N, K, nz) || (has_c && !lds_all)) ? 0 :
        w0_fused_slabs(q, nz, a->w0_in, a->w0_x.pitch, (const float*)fake[B_W0X] + a->w0_x.off, a->w0_x.s0, a->w0_x.s1, 64);
    if (slabs < 1) return fail("orl_debug_gemm_ex: the fused layer-0 gradient runs where pick_cfg chooses CFG_BIG or CFG_SQ, with N % 4 == 0, at most 64 row tiles and 16-byte aligned aux / C / w0_x (w0_fused_slabs)");
    if (!tap_fits(a->w0_out, "w0_out", (long)(N - 1) * a->w0_out.pitch + a->w0_in, nz0, nz1, slabs, true, why) ||
        !tap_fits(a->w0_bias, "w0_bias", N, nz0, nz1, slabs, true, why)) return fail("orl_debug_gemm_ex: " + why);
    a->r_w0_slabs = slabs;
  }
  // store path per problem and slab (the kernel's vec_ok / tr_ok / LDS conditions)
  {
    const bool tr_cap = wg && t.TM == t.TN && t.epi_fits && (t.NT % (t.TM / 4)) == 0;
    const bool tr_ok = tr_cap && p.c_sr == 1 && p.c_sn != 1 && !(p.c_sn & 3) && !(p.c_s0 & 3) && !(p.c_s1 & 3) && !(p.c_ks & 3) && aligned16(p.C) && !(M & 3);
    int first = -1; bool mixed = false;
    for (int z0 = 0; z0 < nz0; ++z0)
      for (int z1 = 0; z1 < nz1; ++z1)
        for (int ks = 0; ks < ksplit; ++ks) {
          const float* Cg = p.C + z0 * p.c_s0 + z1 * p.c_s1 + (long)ks * p.c_ks;
          const float* aux = p.aux.at(z0, z1);
          const bool aux_al = !(p.aux_sr & 3) && aligned16(aux);
          const bool vec_ok = has_c && p.c_sn == 1 && !(p.c_sr & 3) && aligned16(Cg) && (epi != E_MASK || a->aux_bits.host || aux_al) &&
                              ((epi != E_SWISH_GRAD && epi != E_LEAKY_MASK) || aux_al) && (!bias_epi || aligned16(p.bias.at(z0, z1)));
          int path = tr_ok ? 3 : ((t.epi_fits && (vec_ok || (a->r_w0_slabs && !has_c)) && !(N & 3)) ? 0 : (vec_ok ? 1 : 2));
          if (first < 0) first = path;
          else if (path != first) mixed = true;
          if (path != 0 && (a->r_mb || a->r_tq_parts || a->r_w0_slabs || a->aux_bits.host))
            return fail("orl_debug_gemm_ex: a side output was requested but some problem does not take the LDS-staged store");
        }
    a->r_store = first; a->r_store_mixed = mixed ? 1 : 0;
  }
  if (a->aux_bits.host) a->r_aux_bits = 1;
  if (a->pa == 2) a->r_a_bits = 1;

  if (a->dry_run) return 0;
  // ---- device ----
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device");
  // every array given gets a device copy (z_out has C's element count); the results, B_C onwards, come back
  TapDev dev;
  std::vector<TapArray> arrays;
  for (int i = 0; i < B_COUNT; ++i) {
    const orl_gemm_buf& b = *bufs[i];
    const bool skip = !b.host || (i == B_A && a->pa == 2) || (i == B_C && !has_c);
    arrays.push_back({skip ? nullptr : b.host, i >= B_C ? b.host : nullptr, i == B_ZOUT ? a->C.n : b.n});
  }
  std::vector<float> a_pad;
  if (arrays[B_A].src && a->a_kpad && k4 > K) {      // zero the k pad of every row of every problem
    const orl_gemm_buf& b = a->A;
    a_pad.assign((const float*)b.host, (const float*)b.host + b.n);
    for (int z0 = 0; z0 < nz0; ++z0)
      for (int z1 = 0; z1 < nz1; ++z1)
        for (int m = 0; m < M; ++m)
          for (long k = K; k < k4; ++k) a_pad[b.off + z0 * b.s0 + z1 * b.s1 + (long)m * b.pitch + k] = 0.f;
    arrays[B_A].src = a_pad.data();
  }
  char* base[B_COUNT];
  if (tap_upload(dev, arrays, base, "orl_debug_gemm_ex")) return -1;
  p = params(base);
  if (a->r_mb) { p.mb_out = (unsigned int*)base[B_MB] + a->mb_out.off; p.mb_s0 = a->mb_out.s0; p.mb_s1 = a->mb_out.s1; p.mb_g = (int)a->mb_out.pitch; }
  if (a->r_tq_parts) {
    p.tq_w = ZPtr{(const float*)base[B_TQW] + a->tq_w.off, a->tq_w.s0, a->tq_w.s1};
    p.tq_b = ZPtr{(const float*)base[B_TQB] + a->tq_b.off, a->tq_b.s0, a->tq_b.s1};
    p.tq_out = (float*)base[B_TQO] + a->tq_out.off; p.tq_s0 = a->tq_out.s0; p.tq_s1 = a->tq_out.s1; p.tq_sm = a->tq_sm;
    if (a->r_tq_parts > 1) { p.tq_part = (float*)base[B_TQP] + a->tq_part.off; p.tq_ps0 = a->tq_part.s0; p.tq_ps1 = a->tq_part.s1; p.tq_ts = a->tq_part.pitch; }
  }
  if (a->r_aux_bits) { p.aux_bits = (const unsigned int*)base[B_XBITS] + a->aux_bits.off; p.xb_s0 = a->aux_bits.s0; p.xb_s1 = a->aux_bits.s1; p.xb_g = (int)a->aux_bits.pitch; }
  if (a->r_w0_slabs) {
    p.w0_x = ZPtr{(const float*)base[B_W0X] + a->w0_x.off, a->w0_x.s0, a->w0_x.s1}; p.w0_xsr = a->w0_x.pitch; p.w0_in = a->w0_in;
    p.w0_out = (float*)base[B_W0O] + a->w0_out.off; p.w0_bias = (float*)base[B_W0B] + a->w0_bias.off;
    p.w0_s0 = a->w0_out.s0; p.w0_s1 = a->w0_out.s1; p.w0_bs1 = a->w0_bias.s1; p.w0_ks = a->w0_out.ks; p.w0_sr = a->w0_out.pitch;
  }
  hipStream_t st = nullptr;
  hipError_t err = hipErrorInvalidValue;
  const bool kpad = a->a_kpad != 0;
  if (a->pa == 2) err = launch_gemm_rank1_bits<E_MASK>(cfg, p, nz, st, prec);
  else if (a->pa == 1) {
    if (epi == E_PLAIN) err = launch_gemm<PA_RANK1, PB_PLAIN, E_PLAIN>(cfg, p, nz, st, false, fs, prec);
    else if (epi == E_MASK) err = launch_gemm<PA_RANK1, PB_PLAIN, E_MASK>(cfg, p, nz, st, false, fs, prec);
    else err = launch_gemm<PA_RANK1, PB_PLAIN, E_WGRAD>(cfg, p, nz, st, false, fs, prec);
  } else {
    switch (epi) {
      case E_PLAIN: err = launch_gemm<PA_PLAIN, PB_PLAIN, E_PLAIN>(cfg, p, nz, st, kpad, fs, prec); break;
      case E_BIAS: err = launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS>(cfg, p, nz, st, kpad, fs, prec); break;
      case E_BIAS_RELU: err = launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_RELU>(cfg, p, nz, st, kpad, fs, prec); break;
      case E_MASK: err = launch_gemm<PA_PLAIN, PB_PLAIN, E_MASK>(cfg, p, nz, st, kpad, fs, prec); break;
      case E_WGRAD: err = launch_gemm<PA_PLAIN, PB_PLAIN, E_WGRAD>(cfg, p, nz, st, kpad, fs, prec); break;
      case E_BIAS_SWISH: err = launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_SWISH>(cfg, p, nz, st, kpad, fs, prec); break;
      case E_SWISH_GRAD: err = launch_gemm<PA_PLAIN, PB_PLAIN, E_SWISH_GRAD>(cfg, p, nz, st, kpad, fs, prec); break;
      case E_BIAS_LEAKY: err = launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_LEAKY>(cfg, p, nz, st, kpad, fs, prec); break;
      default: err = launch_gemm<PA_PLAIN, PB_PLAIN, E_LEAKY_MASK>(cfg, p, nz, st, kpad, fs, prec); break;
    }
  }
  if (err != hipSuccess) return fail(std::string("orl_debug_gemm_ex launch: ") + hipGetErrorString(err));
  ORL_HIP(hipDeviceSynchronize());
  return tap_download(arrays, base, "orl_debug_gemm_ex");
}

// GEMM tuning tap: times `reps` launches of one tile configuration on random data of the hot-path shapes.
//  kind 0: forward  (VECK,VECK, bias+relu)   C[M,N]   = relu(A[M,K] W[N,K]^T + b)
//  kind 1: dgrad    (VECK,BLK4, rank-1, mask) C[M,N]   = ((H>0) dq w) W[K,N]  masked
//  kind 2: wgrad    (BLK4,BLK4, rank-1, ones) C[M,N+1] = ((H>0) dq w)^T X     (M = out, K = rows), split-K
int orl_debug_gemm_time(int cfg, int kind, int M, int N, int K, int nz, int ksplit, int reps, float* ms_out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device");
  const long nA = (kind == 2) ? (long)K * M : (long)M * K;
  const long nB = (kind == 0) ? (long)N * K : (kind == 1 ? (long)K * N : (long)K * N);
  const long nC = (kind == 2) ? (long)M * (N + 1) * ksplit : (long)M * N;
  float *dA, *dB, *dC, *dv0, *dv1, *dH;
  TapDev dev;      // (an error return frees what was allocated)
  const char* F = "orl_debug_gemm_time";
  if (dev.alloc(&dA, nA * nz, F) || dev.alloc(&dB, nB * nz, F) || dev.alloc(&dC, nC * nz, F) || dev.alloc(&dH, (long)M * N * nz, F) ||
      dev.alloc(&dv0, (long)(M + K + N) * nz, F) || dev.alloc(&dv1, (long)(M + K + N) * nz, F)) return -1;
  std::vector<float> h(std::max(std::max(nA, nB), std::max((long)M * N, (long)(M + K + N))) * nz);
  unsigned s = 12345u;
  auto fill = [&](float* d, long n) { for (long i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; h[i] = ((s >> 8) / 8388608.0f) - 1.0f; } return hipMemcpy(d, h.data(), sizeof(float) * n, hipMemcpyHostToDevice); };
  ORL_HIP(fill(dA, nA * nz)); ORL_HIP(fill(dB, nB * nz)); ORL_HIP(fill(dH, (long)M * N * nz)); ORL_HIP(fill(dv0, (long)(M + K + N) * nz)); ORL_HIP(fill(dv1, (long)(M + K + N) * nz));
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.nz1 = nz; p.ksplit = ksplit; p.C = dC; p.c_sn = 1; p.c_s1 = nC;
  p.A = {dA, 0, nA}; p.B = {dB, 0, nB};
  p.rowv = {dv0, 0, (long)(M + K + N)}; p.colv = {dv1, 0, (long)(M + K + N)};
  p.bias = {dv0, 0, (long)(M + K + N)}; p.aux = {dH, 0, (long)M * N}; p.aux_sr = N;
  hipStream_t st = nullptr;
  LoopScope timed;
  hipError_t err = hipSuccess;
  for (int it = 0; it < reps + 3; ++it) {
    if (it == 3 && timed.begin(st, {})) return -1;
    if (kind == 0) {
      p.a_sr = K; p.a_sk = 1; p.b_sr = K; p.b_sk = 1; p.M = M; p.N = N; p.K = K; p.c_sr = N;
      err = launch_tune(cfg, 0, p, nz, st);
    } else if (kind == 1) {
      p.a_sr = K; p.a_sk = 1; p.b_sr = 1; p.b_sk = N; p.b_rlim = N & ~3; p.M = M; p.N = N; p.K = K; p.c_sr = N; p.a_trans = 0;
      err = launch_tune(cfg, 1, p, nz, st);
    } else {
      p.a_sr = 1; p.a_sk = M; p.b_sr = 1; p.b_sk = N; p.a_rlim = M & ~3; p.b_rlim = N & ~3; p.M = M; p.N = N; p.K = K; p.c_sr = N;
      p.ones_row = 1 << 30; p.a_trans = 1; p.c_ks = (long)M * (N + 1); p.c_s1 = nC; p.bias_out = dC + (long)M * N; p.bo_s1 = nC; p.bo_ks = (long)M * (N + 1);
      err = launch_tune(cfg, 2, p, nz, st);
    }
    if (err != hipSuccess) return fail(std::string("gemm_time launch: ") + hipGetErrorString(err));
  }
  float ms = 0.f;
  if (timed.end(0, F, &ms)) return -1;
  *ms_out = ms / reps;
  return 0;
}

}  // extern "C"
