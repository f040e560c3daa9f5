// ws_debug.hip — the unit-test tap of the weight-stationary kernels (orl_debug_ws, include/orl_engine.h): one launch of one launch_ws_*
// function on host arrays, every check before the first HIP call.  Host code only.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/orl_engine.h"
#include "debug_tap.h"
#include "ws_gemm.h"

namespace orl {
namespace {

// Every instantiation of the ws_* kernels = the launchers' own tables (ws_gemm.h: WsTable), in the order of the tap's kinds; a launch reports the
// row its launcher's selector picked, counted through all six.
//   ws_fwd<TQ,L0,DG,SY,F32,XS>  ws_fwd3<TQ,SY,XS,L0,DG>  ws_dgrad<W0,STORE,PLAIN> (ws_dgrad32: the exact-fp32 kernel)  ws_dgrad3<W0,PLAIN>
//   ws_wgrad<MODE> / ws_wgrad32<MODE>  ws_wgrad3p
typedef const WsTable& (*WsTableFn)();
static const WsTableFn WS_TABLES[] = {ws_fwd_table, ws_fwd3_table, ws_dgrad_table, ws_dgrad3_table, ws_wgrad_table, ws_wgrad3p_table};

enum { B_X, B_W, B_BIAS, B_TW, B_TB, B_X0, B_W0, B_B0, B_DMASK, B_ABITS, B_XBITS, B_DQ, B_WT, B_Z, B_H0, B_H1, B_W1, B_B1, B_DZ, B_GSCALE,
       B_Y, B_MB, B_MB0, B_TQ, B_TQ2, B_C, B_W0O, B_B0O, B_DW, B_DB, B_DWT, B_DBT, B_COUNT };
static const char* const WS_BUF_NAMES[B_COUNT] = {"X", "W", "bias", "tw", "tb", "X0", "W0", "b0", "dmask", "abits", "xbits", "dq", "wt", "Z", "H0", "H1",
                                                   "W1", "b1", "dZ", "gscale", "Y", "mb", "mb0", "tq", "tq2", "C", "w0_out", "b0_out", "dW", "db", "dwt", "dbt"};

// which arrays a launcher may be given
static bool ws_buf_allowed(int kind, int i) {
  const bool fwd = kind == ORL_WS_FWD || kind == ORL_WS_FWD3, dg = kind == ORL_WS_DGRAD || kind == ORL_WS_DGRAD3;
  switch (i) {
    case B_X: case B_W: return fwd || dg;
    case B_BIAS: case B_TW: case B_TB: case B_DMASK: case B_Y: case B_MB: case B_MB0: case B_TQ: return fwd;
    case B_TQ2: return kind == ORL_WS_FWD3;
    case B_X0: case B_W0: case B_B0: return fwd || kind == ORL_WS_WGRAD;
    case B_XBITS: case B_Z: case B_C: case B_W0O: case B_B0O: return dg;
    case B_ABITS: case B_DQ: case B_WT: return dg || kind == ORL_WS_WGRAD;
    case B_H0: case B_DZ: case B_DW: case B_DB: return kind == ORL_WS_WGRAD || kind == ORL_WS_WGRAD3P;
    case B_H1: case B_W1: case B_B1: case B_DWT: case B_DBT: return kind == ORL_WS_WGRAD;
    default: return true;      // gscale
  }
}

}  // namespace
}  // namespace orl

using namespace orl;

extern "C" {

const char* orl_debug_ws_flavour(int idx) {
  for (WsTableFn table : WS_TABLES) {
    const WsTable& t = table();
    if (idx >= 0 && idx < t.n) return t.rows[idx].name;
    idx -= t.n;
  }
  return nullptr;
}

int orl_debug_ws(orl_ws_ex* a) {
  if (!a) return fail("orl_debug_ws: null arguments");
  const int kind = a->kind, M = a->M, nz0 = a->nz0, nz1 = a->nz1, per_z = a->per_z;
  auto bad = [](const std::string& m) { return fail("orl_debug_ws: " + m); };
  // ---- argument checks: all of them before the first HIP call ----
  if (kind < ORL_WS_FWD || kind > ORL_WS_WGRAD3P) return bad("kind must be 0..5");
  if (M < 1 || M > 4096) return bad("M must be 1..4096");
  if (M % WS_ROWS) return bad("M must be a multiple of 32 (whole row groups)");
  if (nz0 < 1 || nz1 < 1 || (long)nz0 * nz1 > 64) return bad("nz0 x nz1 must be 1..64");
  if (per_z < 1) return bad("per_z must be >= 1");
  if (per_z > M / WS_ROWS) return bad("per_z exceeds the row groups (M / 32): a workgroup would own no group");
  const int nz = nz0 * nz1, groups = M / WS_ROWS;
  const bool fwd = kind == ORL_WS_FWD || kind == ORL_WS_FWD3, dg = kind == ORL_WS_DGRAD || kind == ORL_WS_DGRAD3;
  const bool wg = kind == ORL_WS_WGRAD || kind == ORL_WS_WGRAD3P;
  if (a->f32 && (kind == ORL_WS_FWD3 || kind == ORL_WS_DGRAD3 || kind == ORL_WS_WGRAD3P)) return bad("f32 does not go with a three-plane launcher");
  if (a->np3 && kind != ORL_WS_WGRAD) return bad("np3 selects ws_wgrad_kernel<5> of launch_ws_wgrad and nothing else");
  if (a->np3 && a->f32) return bad("np3 and f32 exclude each other");

  orl_gemm_buf* bufs[B_COUNT] = {&a->X, &a->W, &a->bias, &a->tw, &a->tb, &a->X0, &a->W0, &a->b0, &a->dmask, &a->abits, &a->xbits, &a->dq, &a->wt, &a->Z,
                                 &a->H0, &a->H1, &a->W1, &a->b1, &a->dZ, &a->gscale, &a->Y, &a->mb, &a->mb0, &a->tq, &a->tq2, &a->C, &a->w0_out, &a->b0_out,
                                 &a->dW, &a->db, &a->dwt, &a->dbt};
  auto has = [&](int i) { return bufs[i]->host != nullptr; };
  for (int i = 0; i < B_COUNT; ++i)
    if (has(i) && !ws_buf_allowed(kind, i)) return bad(std::string(WS_BUF_NAMES[i]) + " does not belong to this launcher");

  std::string why;
  auto fits = [&](int i, long ext, int nslab, bool result) { return tap_fits(*bufs[i], WS_BUF_NAMES[i], ext, nz0, nz1, nslab, result, why); };
  // a row-major [M][cols] matrix with a pitch
  auto rows_fit = [&](int i, long cols, bool result) {
    if (has(i) && bufs[i]->pitch < cols) { why = std::string(WS_BUF_NAMES[i]) + ": the pitch is below the width"; return false; }
    return fits(i, (long)(M - 1) * bufs[i]->pitch + cols, 1, result);
  };
  // a narrow input matrix: the kernels read whole row groups, 32 * pitch consecutive elements each
  auto narrow_fit = [&](int i) {
    if (has(i) && (bufs[i]->pitch < 1 || bufs[i]->pitch > 32)) { why = std::string(WS_BUF_NAMES[i]) + ": the pitch must be 1..32"; return false; }
    return fits(i, (long)M * bufs[i]->pitch, 1, false);
  };
  auto strided_fit = [&](int i, long sn, long sk, int nn, int nk, int nslab, bool result) {      // element (n, k) at n sn + k sk
    if (sn < 1 || sk < 1) { why = std::string(WS_BUF_NAMES[i]) + ": strides must be >= 1"; return false; }
    return fits(i, (long)(nn - 1) * sn + (long)(nk - 1) * sk + 1, nslab, result);
  };
  const bool l0 = fwd && has(B_X0), recomp = wg && has(B_X0);
  if ((l0 || recomp || (dg && has(B_W0O))) && (a->in0 < 1 || a->in0 + 1 > 32)) return bad("in0 must be 1..31 (in0 + 1 <= 32: the ones column takes a slot)");
  if (has(B_GSCALE)) {
    const orl_gemm_buf& b = a->gscale;
    if (b.n <= 0 || b.off < 0 || b.off + nz0 > b.n) return bad("gscale: one float per run (nz0) from its offset");
  }

  if (fwd) {
    const bool dgm = has(B_DMASK), tq = has(B_TQ), sy = has(B_Y);
    if (a->tq_sm < 1) return bad("tq_sm must be >= 1");
    if (has(B_TW) != tq || has(B_TB) != tq) return bad("the fused tail needs tw, tb and tq together");
    if (kind == ORL_WS_FWD3 && tq && !has(B_TQ2)) return bad("the three-plane forward writes its tail as two partial sums: tq needs tq2");
    if (has(B_TQ2) && !tq) return bad("tq2 goes with tq");
    if (dgm && (tq || l0 || has(B_BIAS) || has(B_MB) || has(B_MB0))) return bad("plain dgrad mode (dmask) has no bias, tail, fused first layer or mask output");
    if (dgm && bufs[B_DMASK]->pitch != 8) return bad("dm_g (dmask's pitch) must be 8 words");
    if (l0 != has(B_W0) || l0 != has(B_B0) || l0 != has(B_MB0)) return bad("the fused first layer needs X0, W0, b0 and mb0 together");
    if (a->x0_discard && !l0) return bad("x0_discard belongs to the fused first layer");
    if (!rows_fit(B_X, WS_K, l0) || !strided_fit(B_W, a->w_sn, a->w_sk, WS_N, WS_K, 1, false)) return bad(why);
    if (!dgm && !has(B_MB)) return bad("mb is required (the forward always emits mask words)");
    if (!dgm && (!fits(B_BIAS, WS_N, 1, false) || !rows_fit(B_MB, 8, true))) return bad(why);
    if (sy && !rows_fit(B_Y, WS_N, true)) return bad(why);
    if (tq && (!fits(B_TW, WS_N, 1, false) || !fits(B_TB, 1, 1, false) || !fits(B_TQ, (long)(M - 1) * a->tq_sm + 1, 1, true))) return bad(why);
    if (has(B_TQ2) && !fits(B_TQ2, M, 1, true)) return bad(why);
    if (dgm && !rows_fit(B_DMASK, 8, false)) return bad(why);
    if (l0) {
      if (a->in0 >= bufs[B_X0]->pitch) return bad("in0 must be below x0_pitch (the ones column needs a slot of the staged row)");
      if (bufs[B_MB0]->pitch != 8) return bad("mb0_g (mb0's pitch) must be 8 words");
      if (!narrow_fit(B_X0) || !strided_fit(B_W0, a->w0_sn, a->w0_sk, WS_N, a->in0, 1, false) || !fits(B_B0, WS_N, 1, false) || !rows_fit(B_MB0, 8, true)) return bad(why);
    }
  } else if (dg) {
    const bool plain = has(B_Z), w0 = has(B_W0O), store = has(B_C);
    if (a->dq_sm < 1) return bad("dq_sm must be >= 1");
    if (w0 == store) return bad("give either the dW0 / db0 slabs (w0_out, b0_out) or C (the stored dz0), not both and not neither");
    if (w0 != has(B_B0O)) return bad("w0_out and b0_out go together");
    if (plain && (has(B_ABITS) || has(B_DQ) || has(B_WT))) return bad("the plain flavour (Z) takes no abits, dq or wt");
    if (!has(B_XBITS) || bufs[B_XBITS]->pitch != 8) return bad("xb_g (xbits' pitch) must be 8 words");
    if (!plain && (!has(B_ABITS) || bufs[B_ABITS]->pitch != 8)) return bad("ab_g (abits' pitch) must be 8 words");
    if (!rows_fit(B_XBITS, 8, false) || !strided_fit(B_W, a->w_sn, a->w_sk, WS_N, WS_K, 1, false)) return bad(why);
    if (plain) { if (!rows_fit(B_Z, WS_K, false)) return bad(why); }
    else if (!rows_fit(B_ABITS, 8, false) || !fits(B_DQ, (long)(M - 1) * a->dq_sm + 1, 1, false) || !fits(B_WT, WS_K, 1, false)) return bad(why);
    if (w0) {
      if (!has(B_X)) return bad("X is required");
      if (a->in0 >= bufs[B_X]->pitch) return bad("in0 must be below x_pitch (the ones column needs a slot of the staged row)");
      if (a->b0_out.s0 != a->w0_out.s0 || a->b0_out.ks != a->w0_out.ks) return bad("b0_out shares w0_out's s0 and slab stride");
      if (!narrow_fit(B_X) || !strided_fit(B_W0O, a->o_sr, a->o_sc, WS_N, a->in0, per_z, true) || !fits(B_B0O, WS_N, per_z, true)) return bad(why);
    } else {
      if (has(B_X)) return bad("X belongs to the dW0 / db0 flavour");
      if (!rows_fit(B_C, WS_N, true)) return bad(why);
    }
  } else {
    const bool plain = has(B_DZ), tails = has(B_H1), derived = !tails && has(B_W1);
    if (a->dq_sm < 1) return bad("dq_sm must be >= 1");
    if (kind == ORL_WS_WGRAD3P && !plain) return bad("launch_ws_wgrad3p is the plain (materialised dZ) flavour: dZ is required");
    if (a->np3 && tails) return bad("np3 is the derived-tail flavour: it takes W1 / b1, not H1");
    if (plain && (has(B_ABITS) || has(B_DQ) || has(B_WT) || tails || has(B_W1) || has(B_B1) || has(B_DWT) || has(B_DBT))) return bad("the plain flavour (dZ) takes no abits, dq, wt, H1, W1, b1 and writes no tail gradients");
    if (recomp && !plain) return bad("X0 (recompute) belongs to the plain flavour");
    if (recomp == has(B_H0)) return bad("give either H0 or X0 / W0 / b0 (recompute)");
    if (recomp != has(B_W0) || recomp != has(B_B0)) return bad("recompute needs X0, W0 and b0 together");
    if (tails && has(B_W1)) return bad("H1 (streamed tails) and W1 (derived tails) exclude each other");
    if (has(B_W1) != has(B_B1)) return bad("W1 and b1 go together");
    if ((tails || derived) != has(B_DWT) || has(B_DWT) != has(B_DBT)) return bad("dwt and dbt go with the tail gradients (H1, or W1 / b1) and with nothing else");
    if (!plain && (!has(B_ABITS) || bufs[B_ABITS]->pitch != 8)) return bad("ab_g (abits' pitch) must be 8 words");
    if (plain) { if (!rows_fit(B_DZ, WS_K, false)) return bad(why); }
    else if (!rows_fit(B_ABITS, 8, false) || !fits(B_DQ, (long)(M - 1) * a->dq_sm + 1, 1, false) || !fits(B_WT, WS_K, 1, false)) return bad(why);
    if (recomp) {
      if (a->in0 >= bufs[B_X0]->pitch) return bad("in0 must be below x0_pitch (the ones column needs a slot of the staged row)");
      if (!narrow_fit(B_X0) || !strided_fit(B_W0, a->w0_sn, a->w0_sk, WS_N, a->in0, 1, false) || !fits(B_B0, WS_N, 1, false)) return bad(why);
    } else if (!rows_fit(B_H0, WS_N, false)) return bad(why);
    if (tails && !rows_fit(B_H1, WS_K, false)) return bad(why);
    if (derived && (!fits(B_W1, (long)WS_K * WS_N, 1, false) || !fits(B_B1, WS_K, 1, false))) return bad(why);
    if (!fits(B_DW, (long)WS_K * WS_N, per_z, true) || !fits(B_DB, WS_K, per_z, true)) return bad(why);
    if (a->db.s0 != a->dW.s0 || a->db.ks != a->dW.ks) return bad("db shares dW's s0 and slab stride");
    if (has(B_DWT)) {
      if (!fits(B_DWT, WS_K, per_z, true) || !fits(B_DBT, 1, per_z, true)) return bad(why);
      if (a->dwt.s0 != a->dW.s0 || a->dwt.ks != a->dW.ks || a->dbt.s0 != a->dW.s0 || a->dbt.ks != a->dW.ks) return bad("dwt and dbt share dW's s0 and slab stride");
    }
  }

  // ---- the launch parameters, on any 16-byte aligned bases (alignment decides the predicates; the device bases are 256-byte aligned) ----
  WsFwdP pf;
  WsDgradP pd;
  WsWgradP pw;
  auto params = [&](char* const* base, float* dump) {
    auto fp = [&](int i) -> float* { return bufs[i]->host ? (float*)base[i] + bufs[i]->off : nullptr; };
    auto zp = [&](int i) { return ZPtr{fp(i), bufs[i]->s0, bufs[i]->s1}; };
    auto zo = [&](int i) { return ZOut{fp(i), bufs[i]->s0, bufs[i]->s1}; };
    auto zb = [&](int i) { return ZBits{(unsigned int*)fp(i), bufs[i]->s0, bufs[i]->s1}; };
    memset(&pf, 0, sizeof(pf)); memset(&pd, 0, sizeof(pd)); memset(&pw, 0, sizeof(pw));
    if (fwd) {
      pf.X = zp(B_X); pf.x_pitch = (int)a->X.pitch;
      pf.W = zp(B_W); pf.w_sn = a->w_sn; pf.w_sk = a->w_sk;
      pf.bias = zp(B_BIAS);
      pf.Y = zo(B_Y); pf.y_pitch = (int)a->Y.pitch;
      pf.mb = zb(B_MB); pf.mb_g = (int)a->mb.pitch;
      pf.tw = zp(B_TW); pf.tb = zp(B_TB); pf.tq = zo(B_TQ); pf.tq_sm = a->tq_sm; pf.tq2 = zo(B_TQ2);
      pf.M = M; pf.nz1 = nz1; pf.groups = groups;
      pf.X0 = zp(B_X0); pf.x0_pitch = (int)a->X0.pitch; pf.in0 = a->in0; pf.x0_discard = a->x0_discard;
      pf.W0 = zp(B_W0); pf.w0_sn = a->w0_sn; pf.w0_sk = a->w0_sk; pf.b0 = zp(B_B0);
      pf.mb0 = zb(B_MB0); pf.mb0_g = (int)a->mb0.pitch;
      pf.dmask = zb(B_DMASK); pf.dm_g = (int)a->dmask.pitch;
      pf.f32 = a->f32; pf.gscale = fp(B_GSCALE); pf.np3 = kind == ORL_WS_FWD3; pf.dump = dump;
    } else if (dg) {
      pd.abits = zb(B_ABITS); pd.ab_g = (int)a->abits.pitch;
      pd.xbits = zb(B_XBITS); pd.xb_g = (int)a->xbits.pitch;
      pd.dq = zp(B_DQ); pd.dq_sm = a->dq_sm; pd.wt = zp(B_WT);
      pd.W = zp(B_W); pd.w_sn = a->w_sn; pd.w_sk = a->w_sk;
      pd.X = zp(B_X); pd.x_pitch = (int)a->X.pitch; pd.in0 = a->in0;
      pd.w0_out = fp(B_W0O); pd.b0_out = fp(B_B0O);
      pd.o_rs = a->w0_out.s0; pd.o_ms = a->w0_out.s1; pd.ob_ms = a->b0_out.s1; pd.o_ks = a->w0_out.ks; pd.o_sr = a->o_sr; pd.o_sc = a->o_sc;
      pd.C = zo(B_C); pd.c_pitch = (int)a->C.pitch;
      pd.Z = zp(B_Z); pd.z_pitch = (int)a->Z.pitch;
      pd.M = M; pd.nz1 = nz1; pd.groups = groups; pd.f32 = a->f32; pd.gscale = fp(B_GSCALE);
    } else {
      pw.abits = zb(B_ABITS); pw.ab_g = (int)a->abits.pitch;
      pw.dq = zp(B_DQ); pw.dq_sm = a->dq_sm;
      pw.H0 = zp(B_H0); pw.h0_pitch = (int)a->H0.pitch; pw.wt = zp(B_WT);
      pw.dW = fp(B_DW); pw.db = fp(B_DB);
      pw.o_rs = a->dW.s0; pw.o_msw = a->dW.s1; pw.o_msb = a->db.s1; pw.o_ks = a->dW.ks;
      pw.H1 = zp(B_H1); pw.h1_pitch = (int)a->H1.pitch;
      pw.dwt = fp(B_DWT); pw.dbt = fp(B_DBT); pw.o_mswt = a->dwt.s1; pw.o_msbt = a->dbt.s1;
      pw.W1 = zp(B_W1); pw.b1 = zp(B_B1);
      pw.dZ = zp(B_DZ); pw.dz_pitch = (int)a->dZ.pitch;
      pw.X0 = zp(B_X0); pw.x0_pitch = (int)a->X0.pitch; pw.in0 = a->in0;
      pw.W0 = zp(B_W0); pw.w0_sn = a->w0_sn; pw.w0_sk = a->w0_sk; pw.b0 = zp(B_B0);
      pw.M = M; pw.nz1 = nz1; pw.groups = groups; pw.f32 = a->f32; pw.np3 = a->np3; pw.gscale = fp(B_GSCALE);
    }
  };
  char* fake[B_COUNT];
  for (int i = 0; i < B_COUNT; ++i) fake[i] = (char*)(uintptr_t)4096;
  params(fake, (float*)(uintptr_t)4096);
  bool ok = false;
  int row = -1;      // the instantiation the launcher will take: its own selector's row of its own table
  const char* pred = "";
  switch (kind) {
    case ORL_WS_FWD: ok = ws_fwd_supported(pf, WS_K, WS_N) && (!l0 || ws_fwd01_supported(pf)); row = ws_fwd_flavour(pf); pred = "ws_fwd_supported / ws_fwd01_supported"; break;
    case ORL_WS_FWD3: ok = ws_fwd3_supported(pf, WS_K, WS_N); row = ws_fwd3_flavour(pf); pred = "ws_fwd3_supported"; break;
    case ORL_WS_DGRAD: ok = ws_dgrad_supported(pd, WS_K, WS_N); row = ws_dgrad_flavour(pd); pred = "ws_dgrad_supported"; break;
    case ORL_WS_DGRAD3: ok = ws_dgrad3_supported(pd, WS_K, WS_N); row = ws_dgrad3_flavour(pd); pred = "ws_dgrad3_supported"; break;
    case ORL_WS_WGRAD: ok = ws_wgrad_supported(pw, WS_K, WS_N); row = ws_wgrad_flavour(pw); pred = "ws_wgrad_supported"; break;
    default: ok = ws_wgrad3p_supported(pw, WS_K, WS_N); row = ws_wgrad3p_flavour(pw); pred = "ws_wgrad3p_supported"; break;
  }
  if (!ok) return bad(std::string("refused by ") + pred + " (M >= 256 in whole row groups, 16-byte aligned vector operands, pitches and strides that are multiples of 4, a flavour the launcher has)");
  int id = 0;
  if (row < 0) return bad("the launcher has no instantiation for these parameters");
  for (int k = 0; k < kind; ++k) id += WS_TABLES[k]().n;
  a->r_launcher = kind; a->r_flavour = id + row; a->r_lds = (int)WS_TABLES[kind]().rows[row].lds; a->r_groups = groups;
  if (a->dry_run) return 0;

  // ---- device ----
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device");
  // everything comes back, operands included: the caller checks that they are bit-identical (X under the fused first layer is a result)
  TapDev dev;
  std::vector<TapArray> arrays;
  for (int i = 0; i < B_COUNT; ++i) arrays.push_back({bufs[i]->host, bufs[i]->host, bufs[i]->n});
  char* base[B_COUNT];
  if (tap_upload(dev, arrays, base, "orl_debug_ws")) return -1;
  float* dump = nullptr;
  if (kind == ORL_WS_FWD3 && dev.alloc(&dump, (size_t)WS_DUMP_SLOTS * WS_N, "orl_debug_ws")) return -1;
  params(base, dump);
  hipStream_t st = nullptr;
  hipError_t err = hipErrorInvalidValue;
  switch (kind) {
    case ORL_WS_FWD: { WsGeom geo; geo.cus = per_z * nz; geo.one_round = true; err = launch_ws_fwd(pf, nz, st, geo); break; }
    case ORL_WS_FWD3: err = launch_ws_fwd3(pf, nz, per_z, st); break;
    case ORL_WS_DGRAD: err = launch_ws_dgrad_w0(pd, nz, per_z, st); break;
    case ORL_WS_DGRAD3: err = launch_ws_dgrad3_w0(pd, nz, per_z, st); break;
    case ORL_WS_WGRAD: err = launch_ws_wgrad(pw, nz, per_z, st); break;
    default: err = launch_ws_wgrad3p(pw, nz, per_z, st); break;
  }
  if (err != hipSuccess) return fail(std::string("orl_debug_ws device: launch: ") + hipGetErrorString(err));
  err = hipDeviceSynchronize();
  if (err != hipSuccess) return fail(std::string("orl_debug_ws device: ") + hipGetErrorString(err));
  return tap_download(arrays, base, "orl_debug_ws");
}

}  // extern "C"
