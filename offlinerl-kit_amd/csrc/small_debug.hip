// small_debug.hip — the unit-test tap of the few-rows kernels (orl_debug_small, include/orl_engine.h): one launch of launch_small_fwd or
// launch_small_abwd on host arrays, every check before the first HIP call.  Host code only.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/orl_engine.h"
#include "debug_tap.h"
#include "scalars.h"
#include "small_bwd.h"
#include "small_fwd.h"

namespace orl {
namespace {

struct SmallBuf { const char* name; orl_gemm_buf* b; };

static_assert(sizeof(RunScalars) == 16 * sizeof(float) && sizeof(Hyper) == 8 * sizeof(float), "the tap exposes RunScalars as 16 floats and Hyper as 8");

}  // namespace
}  // namespace orl

using namespace orl;

extern "C" {

const char* orl_debug_small_flavour(int idx) {
  int nf = 0, nb = 0;
  const SmallFlavour* f = small_fwd_flavours(&nf);
  const SmallFlavour* b = small_abwd_flavours(&nb);
  if (idx >= 0 && idx < nf) return f[idx].name;
  if (idx >= nf && idx < nf + nb) return b[idx - nf].name;
  return nullptr;
}

int orl_debug_small(orl_small_ex* a) {
  if (!a) return fail("orl_debug_small: null arguments");
  auto bad = [](const std::string& m) { return fail("orl_debug_small: " + m); };
  const int kind = a->kind, M = a->M, nz0 = a->nz0, nz1 = a->nz1, A = a->A;
  // ---- argument checks: all of them before the first HIP call ----
  if (kind != ORL_SMALL_FWD && kind != ORL_SMALL_ABWD) return bad("kind must be 0 (small_fwd) or 1 (small_abwd)");
  if (M < 1 || M > 2048) return bad("M must be 1..2048");
  if (nz0 < 1 || nz1 < 1 || (long)nz0 * nz1 > 16) return bad("nz0 x nz1 must be 1..16");
  const bool fwd = kind == ORL_SMALL_FWD;
  if (!fwd && nz1 != 1) return bad("small_abwd has runs (nz0) only: nz1 must be 1");
  const int nz = nz0 * nz1;

  // every array of the struct, in one list: the device copies and the copies back walk it
  std::vector<SmallBuf> bufs = {{"X", &a->X}, {"W0", &a->W0}, {"b0", &a->b0}, {"W1", &a->W1}, {"b1", &a->b1}, {"Wt", &a->Wt}, {"bt", &a->bt}, {"H0", &a->H0},
                                {"H1", &a->H1}, {"OUT", &a->OUT}, {"G", &a->G}};
  static const char* const JOB_NAMES[3][3] = {{"job[0].eps", "job[0].dst", "job[0].logp"}, {"job[1].eps", "job[1].dst", "job[1].logp"}, {"job[2].eps", "job[2].dst", "job[2].logp"}};
  for (int i = 0; i < 3; ++i) {
    bufs.push_back({JOB_NAMES[i][0], &a->job[i].eps});
    bufs.push_back({JOB_NAMES[i][1], &a->job[i].dst});
    bufs.push_back({JOB_NAMES[i][2], &a->job[i].logp});
  }
  const size_t first_abwd = bufs.size();
  const std::vector<SmallBuf> ab = {{"head", &a->head}, {"eps", &a->eps}, {"xa", &a->xa}, {"logp", &a->logp}, {"qa", &a->qa}, {"ga", &a->ga}, {"Wh", &a->Wh}, {"out", &a->out},
                                    {"sc", &a->sc}, {"hy", &a->hy}, {"gstep", &a->gstep}, {"metrics_last", &a->metrics_last}, {"metrics_sum", &a->metrics_sum},
                                    {"part", &a->part}, {"ticket", &a->ticket}};
  bufs.insert(bufs.end(), ab.begin(), ab.end());
  auto idx_of = [&](const orl_gemm_buf* b) { for (size_t i = 0; i < bufs.size(); ++i) if (bufs[i].b == b) return (int)i; return -1; };
  for (size_t i = 0; i < bufs.size(); ++i) {
    if (!bufs[i].b->host) continue;
    const bool shared = i == 0 || i == 3 || i == 7 || i == 8;      // X, W1, H0, H1 belong to both launchers
    if (fwd ? i >= first_abwd : (i < first_abwd && !shared)) return bad(std::string(bufs[i].name) + " does not belong to this launcher");
  }

  // (no slabs here; use_z1 = false: an array that s1 does not walk)
  std::string why;
  auto fits = [&](orl_gemm_buf* bp, long ext, bool result, bool use_z1 = true) {
    return tap_fits(*bp, bufs[idx_of(bp)].name, ext, nz0, use_z1 ? nz1 : 1, 0, result, why);
  };
  auto rows_fit = [&](orl_gemm_buf* bp, long rows, long cols, bool result, long col0 = 0) {      // row-major [rows][pitch], columns col0 .. col0 + cols
    if (bp->host && bp->pitch < col0 + cols) { why = std::string(bufs[idx_of(bp)].name) + ": the pitch is below the width"; return false; }
    return fits(bp, (rows - 1) * bp->pitch + col0 + cols, result);
  };
  auto has = [](const orl_gemm_buf& b) { return b.host != nullptr; };
  const int in0 = a->in0, groups = M / 32;

  if (fwd) {
    const int od = a->out_dim, nj = a->njobs;
    if (!has(a->OUT)) return bad("OUT is required");
    if (a->OUT.pitch < od) return bad("o_pitch (OUT's pitch) is below out_dim");
    if (nj < 0 || nj > 3) return bad("njobs must be 0..3");
    for (int i = 0; i < 3; ++i)
      if (i >= nj && (has(a->job[i].eps) || has(a->job[i].dst) || has(a->job[i].logp))) return bad("an array of a job >= njobs was given");
    if (in0 >= 1 && in0 <= 31 && od >= 1 && od <= SF_MAXOUT) {      // (outside: the predicate below refuses; the extents would be meaningless)
      if (a->X.pitch < in0) return bad("X: the pitch is below in0");
      if (!fits(&a->X, (long)(M - 1) * a->X.pitch + in0, false) || !fits(&a->W0, (long)SF_N * in0, false) || !fits(&a->b0, SF_N, false) ||
          !fits(&a->W1, (long)SF_N * SF_N, false) || !fits(&a->b1, SF_N, false) || !fits(&a->Wt, (long)od * SF_N, false) || !fits(&a->bt, od, false) ||
          !rows_fit(&a->OUT, M, od, true)) return bad(why);
      if (has(a->H0) && !fits(&a->H0, (long)M * SF_N, true)) return bad(why);
      if (has(a->H1) && !fits(&a->H1, (long)M * SF_N, true)) return bad(why);
      if (has(a->G) && a->gn >= 1 && a->gn <= 8 && !rows_fit(&a->G, M, a->gn, true)) return bad(why);
      for (int i = 0; i < nj && A >= 1 && A <= 8; ++i) {
        orl_small_job& j = a->job[i];
        if (j.rep < 1 || j.rep > 16) continue;      // refused by the predicate
        if (j.rows < 1 || j.head_row0 < 0 || j.dst_row0 < 0 || j.dst_col < 0) return bad("a job needs rows >= 1 and head_row0, dst_row0, dst_col >= 0");
        if (j.head_row0 + (j.rows + j.rep - 1) / j.rep > M) return bad("a job draws from head rows past M");
        if (has(j.eps) && !fits(&j.eps, (long)j.rows * A, false, false)) return bad(why);
        if (!has(j.dst)) return bad("job.dst is required");
        if (j.dst.pitch < j.dst_col + A) return bad("job.dst: the pitch is below dst_col + A");
        if (!fits(&j.dst, (long)(j.dst_row0 + j.rows - 1) * j.dst.pitch + j.dst_col + A, true, false)) return bad(why);
        if (has(j.logp) && !fits(&j.logp, j.rows, true, false)) return bad(why);
      }
    }
  } else {
    if (in0 >= 1 && in0 <= 31 && A >= 1 && A <= 8 && a->K == 2 && groups >= 1 && groups <= SB_MAXGROUPS) {
      if (a->X.pitch < in0) return bad("X: the pitch is below in0");
      if (a->xa_col < 0) return bad("xa_col must be >= 0");
      if (a->nm < 1 || a->m_actor < 0 || a->m_actor >= a->nm || a->m_alpha_loss < 0 || a->m_alpha_loss >= a->nm || a->m_alpha < 0 || a->m_alpha >= a->nm)
        return bad("the metric slots must lie in [0, nm)");
      if (!fits(&a->X, (long)(M - 1) * a->X.pitch + in0, false) || !fits(&a->H0, (long)M * SB_N, false) || !fits(&a->H1, (long)M * SB_N, false) ||
          !fits(&a->head, (long)M * 2 * A, false) || !fits(&a->eps, (long)M * A, false) || !rows_fit(&a->xa, M, A, false, a->xa_col) || !fits(&a->logp, M, false) ||
          !fits(&a->W1, (long)SB_N * SB_N, false) || !fits(&a->Wh, (long)2 * A * SB_N, false)) return bad(why);
      // qa [K][M], ga [K][M][ga_pitch]: s1 is the critic stride, walked once (K = 2)
      if (!has(a->qa) || !has(a->ga)) return bad("qa and ga are required");
      if (a->qa.s1 < 0 || a->ga.s1 < 0) return bad("qa / ga: negative critic stride");
      if (!fits(&a->qa, a->qa.s1 + M, false, false)) return bad(why);
      if (a->ga.pitch < A) { /* refused by the predicate */ }
      else if (!fits(&a->ga, a->ga.s1 + (long)(M - 1) * a->ga.pitch + A, false, false)) return bad(why);
      // the slabs: six tensors inside [0, o_ks), disjoint; one slab per row group
      const long o_ks = a->out.ks;
      const long offs[6] = {a->off_w0, a->off_b0, a->off_w1, a->off_b1, a->off_wh, a->off_bh};
      const long lens[6] = {(long)SB_N * in0, SB_N, (long)SB_N * SB_N, SB_N, (long)2 * A * SB_N, 2 * A};
      static const char* const on[6] = {"off_w0", "off_b0", "off_w1", "off_b1", "off_wh", "off_bh"};
      for (int i = 0; i < 6; ++i) {
        if (offs[i] < 0 || offs[i] + lens[i] > o_ks) return bad(std::string(on[i]) + ": the tensor does not fit the slab stride o_ks (out's ks)");
        for (int k = 0; k < i; ++k)
          if (offs[i] < offs[k] + lens[k] && offs[k] < offs[i] + lens[i]) return bad(std::string(on[i]) + " overlaps " + on[k]);
      }
      if (!fits(&a->out, (long)groups * o_ks, true)) return bad(why);
      if (!fits(&a->sc, 16, true) || !fits(&a->metrics_last, a->nm, true) || !fits(&a->metrics_sum, a->nm, true) || !fits(&a->part, (long)SB_MAXGROUPS * 2, true) ||
          !fits(&a->ticket, 1, true)) return bad(why);
      if (a->sc.s0 != 16 || a->metrics_last.s0 != a->nm || a->metrics_sum.s0 != a->nm || a->part.s0 != SB_MAXGROUPS * 2 || a->ticket.s0 != 1)
        return bad("sc, metrics_last, metrics_sum, part and ticket are dense per run: s0 = 16, nm, nm, 128, 1");
      if (!has(a->hy) || a->hy.off < 0 || a->hy.off + 8 > a->hy.n) return bad("hy: 8 floats from its offset");
      if (!has(a->gstep) || a->gstep.off < 0 || (a->gstep.off & 1) || a->gstep.off + 2 > a->gstep.n) return bad("gstep: one 64-bit value (two words) from an even offset");
      for (int r = 0; r < nz0; ++r)
        if (((const unsigned int*)a->ticket.host)[a->ticket.off + r] != 0u) return bad("ticket must be zero before a launch");
    }
  }

  // ---- the launch parameters, on any 16-byte aligned bases (alignment decides the predicates; the device bases are 256-byte aligned) ----
  SmallFwdP pf;
  SmallABwdP pb;
  auto params = [&](const std::vector<char*>& base) {
    auto fp = [&](orl_gemm_buf* b) -> float* { return b->host ? (float*)base[idx_of(b)] + b->off : nullptr; };
    memset(&pf, 0, sizeof(pf)); memset(&pb, 0, sizeof(pb));
    if (fwd) {
      auto zp = [&](orl_gemm_buf* b) { return ZPtr{fp(b), b->s0, b->s1}; };
      auto zo = [&](orl_gemm_buf* b) { return ZOut{fp(b), b->s0, b->s1}; };
      pf.X = zp(&a->X); pf.x_pitch = (int)a->X.pitch; pf.in0 = in0;
      pf.W0 = zp(&a->W0); pf.b0 = zp(&a->b0); pf.W1 = zp(&a->W1); pf.b1 = zp(&a->b1); pf.Wt = zp(&a->Wt); pf.bt = zp(&a->bt);
      pf.H0 = zo(&a->H0); pf.H1 = zo(&a->H1);
      pf.OUT = zo(&a->OUT); pf.o_pitch = (int)a->OUT.pitch; pf.out_dim = a->out_dim;
      pf.M = M; pf.nz1 = nz1; pf.f32 = a->f32;
      pf.G = zo(&a->G); pf.g_pitch = (int)a->G.pitch; pf.gc0 = a->gc0; pf.gn = a->gn;
      pf.njobs = a->njobs; pf.A = A;
      for (int i = 0; i < 3 && i < a->njobs; ++i) {
        orl_small_job& j = a->job[i];
        SampleJob& s = pf.job[i];
        s.head_row0 = j.head_row0; s.rows = j.rows; s.rep = j.rep;
        s.eps = fp(&j.eps); s.eps_rs = j.eps.s0;
        s.dst = fp(&j.dst); s.dst_rs = j.dst.s0; s.dst_pitch = (int)j.dst.pitch; s.dst_col = j.dst_col; s.dst_row0 = j.dst_row0;
        s.logp = fp(&j.logp); s.logp_rs = j.logp.s0;
      }
    } else {
      pb.X = fp(&a->X); pb.x_s0 = a->X.s0; pb.x_pitch = (int)a->X.pitch; pb.in0 = in0;
      pb.H0 = fp(&a->H0); pb.h0_s0 = a->H0.s0; pb.H1 = fp(&a->H1); pb.h1_s0 = a->H1.s0;
      pb.head = fp(&a->head); pb.head_s0 = a->head.s0;
      pb.eps = fp(&a->eps); pb.eps_s0 = a->eps.s0;
      pb.xa = fp(&a->xa); pb.xa_s0 = a->xa.s0; pb.xa_pitch = (int)a->xa.pitch; pb.xa_col = a->xa_col;
      pb.logp = fp(&a->logp); pb.logp_s0 = a->logp.s0;
      pb.qa = ZPtr{fp(&a->qa), a->qa.s0, a->qa.s1};
      pb.ga = ZPtr{fp(&a->ga), a->ga.s0, a->ga.s1}; pb.ga_pitch = (int)a->ga.pitch;
      pb.K = a->K;
      pb.W1 = fp(&a->W1); pb.w1_s0 = a->W1.s0; pb.Wh = fp(&a->Wh); pb.wh_s0 = a->Wh.s0;
      pb.out = fp(&a->out); pb.o_s0 = a->out.s0; pb.o_ks = a->out.ks;
      pb.off_w0 = a->off_w0; pb.off_b0 = a->off_b0; pb.off_w1 = a->off_w1; pb.off_b1 = a->off_b1; pb.off_wh = a->off_wh; pb.off_bh = a->off_bh;
      pb.sc = (RunScalars*)fp(&a->sc); pb.hy = (const Hyper*)fp(&a->hy);
      pb.auto_alpha = a->auto_alpha; pb.fixed_alpha = a->fixed_alpha; pb.target_entropy = a->target_entropy; pb.clamp_alpha01 = a->clamp_alpha01;
      pb.b1 = a->adam_b1; pb.b2 = a->adam_b2; pb.adam_eps = a->adam_eps;
      pb.gstep = (const unsigned long long*)fp(&a->gstep);
      pb.metrics_last = fp(&a->metrics_last); pb.metrics_sum = fp(&a->metrics_sum); pb.nm = a->nm;
      pb.m_actor = a->m_actor; pb.m_alpha_loss = a->m_alpha_loss; pb.m_alpha = a->m_alpha;
      pb.part = fp(&a->part); pb.ticket = (unsigned int*)fp(&a->ticket);
      pb.M = M; pb.A = A; pb.f32 = a->f32;
    }
  };
  params(std::vector<char*>(bufs.size(), (char*)(uintptr_t)4096));
  int nrows = 0, row, id0 = 0;
  const SmallFlavour* table;
  if (fwd) {
    if (!small_fwd_supported(pf))
      return bad("refused by small_fwd_supported (M in whole 32-row groups, in0 1..31 <= x_pitch <= 32, out_dim 1..16, 16-byte aligned W1 / H0 / H1, jobs: at most 3, nz1 = 1, "
                 "out_dim = 2 A, A <= 8, rep 1..16, no G; G: out_dim = 1, gn 1..8, 0 <= gc0, gc0 + gn <= in0, g_pitch >= gn)");
    table = small_fwd_flavours(&nrows);
    row = small_fwd_flavour(pf);
  } else {
    if (!small_abwd_supported(pb))
      return bad("refused by small_abwd_supported (M in 1..64 whole 32-row groups, in0 1..31 <= x_pitch <= 32, A 1..8, K = 2, ga_pitch >= A, 16-byte aligned W1 / H0 / H1 / Wh "
                 "with run strides that are multiples of 4)");
    small_fwd_flavours(&id0);
    table = small_abwd_flavours(&nrows);
    row = small_abwd_flavour(pb);
  }
  if (row < 0 || row >= nrows) return bad("the launcher has no instantiation for these parameters");
  a->r_kind = kind; a->r_flavour = id0 + row; a->r_lds = (int)table[row].lds; a->r_groups = groups;
  if (a->dry_run) return 0;

  // ---- device ----
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device");
  // everything comes back, operands included: the caller checks that they are bit-identical
  TapDev dev;
  std::vector<TapArray> arrays;
  for (const SmallBuf& sb : bufs) {
    const orl_gemm_buf& b = *sb.b;
    if (b.host && (b.n <= 0 || b.n > (1L << 28))) return bad(std::string(sb.name) + ": bad element count");
    arrays.push_back({b.host, b.host, b.n});
  }
  std::vector<char*> base(bufs.size(), nullptr);
  if (tap_upload(dev, arrays, base.data(), "orl_debug_small")) return -1;
  params(base);
  hipStream_t st = nullptr;
  hipError_t err = fwd ? launch_small_fwd(pf, nz, st) : launch_small_abwd(pb, nz0, st);
  if (err != hipSuccess) return fail(std::string("orl_debug_small device: launch: ") + hipGetErrorString(err));
  err = hipDeviceSynchronize();
  if (err != hipSuccess) return fail(std::string("orl_debug_small device: ") + hipGetErrorString(err));
  return tap_download(arrays, base.data(), "orl_debug_small");
}

}  // extern "C"
