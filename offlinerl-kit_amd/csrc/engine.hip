// engine.hip — MI355X-native update engine: host side (arenas, launch helpers, ABI).
// Algorithm schedules live in algo_*.inc (same translation unit).
// Build: hipcc -O3 --offload-arch=gfx950 -fPIC -shared engine.hip -o liborlengine.so
#include "engine.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <tuple>

namespace orl {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(const std::string& msg) {
  set_error(msg);
  return -1;
}

static inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// ---------------------------------------------------------------------------------------------
// layouts (reference state_dict key names: SURVEY Appendix B)
// ---------------------------------------------------------------------------------------------
static void add_tensor(NetLayout& l, const std::string& name, long off, std::initializer_list<long> shape) { l.tensors.put(name, off, shape); }

enum TailKind { TAIL_CRITIC, TAIL_TANH_GAUSS, TAIL_GAUSS, TAIL_DET, TAIL_LINEAR, TAIL_LINEAR_GAUSS };

// the two return-conditioned algorithms share inputs, buffers, the ordered epoch and every refusal
static inline bool is_rcsl(int algo) { return algo == ORL_ALGO_RCSL || algo == ORL_ALGO_RCSL_GAUSS; }
// ... and the autoregressive behaviour policy shares all of that but the return-to-go, which it does not read
static inline bool is_epoch_algo(int algo) { return is_rcsl(algo) || algo == ORL_ALGO_AUTOREG; }

// seq_step: distance of consecutive Linear layers in the backbone's nn.Sequential -- 2 for [Linear, ReLU], 3 when every ReLU is followed by
// nn.Dropout (nets/mlp.py:20-23): the state_dict keys are backbone.model.{0, 3, 6, ...} then
static NetLayout make_mlp_layout(int in_dim, const int* hidden, int L, TailKind tail, int act_dim, int seq_step = 2, const std::string& prefix = "backbone.model.") {
  NetLayout l;
  l.present = true;
  l.in_dim = in_dim;
  l.L = L;
  long off = 0;
  int d = in_dim;
  for (int i = 0; i < L; ++i) {
    l.H[i] = hidden[i];
    l.w_off[i] = off;
    add_tensor(l, prefix + std::to_string(seq_step * i) + ".weight", off, {hidden[i], d});
    off += (long)hidden[i] * d;
    l.b_off[i] = off;
    add_tensor(l, prefix + std::to_string(seq_step * i) + ".bias", off, {hidden[i]});
    off += hidden[i];
    d = hidden[i];
  }
  if (tail == TAIL_CRITIC) {
    l.out_dim = 1;
    l.w_off[L] = off; add_tensor(l, "last.weight", off, {1, d}); off += d;
    l.b_off[L] = off; add_tensor(l, "last.bias", off, {1}); off += 1;
  } else if (tail == TAIL_TANH_GAUSS) {
    // head = [mu ; sigma] stored as one (2A x H) matrix so a single GEMM yields both
    l.out_dim = 2 * act_dim;
    l.w_off[L] = off;
    add_tensor(l, "dist_net.mu.weight", off, {act_dim, d});
    add_tensor(l, "dist_net.sigma.weight", off + (long)act_dim * d, {act_dim, d});
    off += 2L * act_dim * d;
    l.b_off[L] = off;
    add_tensor(l, "dist_net.mu.bias", off, {act_dim});
    add_tensor(l, "dist_net.sigma.bias", off + act_dim, {act_dim});
    off += 2 * act_dim;
  } else if (tail == TAIL_GAUSS) {
    l.out_dim = act_dim;
    l.w_off[L] = off; add_tensor(l, "dist_net.mu.weight", off, {act_dim, d}); off += (long)act_dim * d;
    l.b_off[L] = off; add_tensor(l, "dist_net.mu.bias", off, {act_dim}); off += act_dim;
    l.extra_off = off; add_tensor(l, "dist_net.sigma_param", off, {act_dim, 1}); off += act_dim;
  } else if (tail == TAIL_LINEAR || tail == TAIL_LINEAR_GAUSS) {
    // the output layer is the backbone's own last nn.Linear (nets/mlp.py with output_dim: RcslModule): no tanh, no distribution head
    const std::string n = prefix + std::to_string(seq_step * L);
    l.out_dim = act_dim;
    l.w_off[L] = off; add_tensor(l, n + ".weight", off, {act_dim, d}); off += (long)act_dim * d;
    l.b_off[L] = off; add_tensor(l, n + ".bias", off, {act_dim}); off += act_dim;
    if (tail == TAIL_LINEAR_GAUSS) {
      // RcslGaussianModule: that output is the latent z (act_dim wide) of DiagGaussian(act_dim, act_dim, conditioned_sigma): two A x A heads
      // behind the body, unstacked and in the reference's state_dict order; k_rcslg_head reads them and writes their gradients (slab 0)
      l.extra_off = off;
      add_tensor(l, "dist_net.mu.weight", off, {act_dim, act_dim}); off += (long)act_dim * act_dim;
      add_tensor(l, "dist_net.mu.bias", off, {act_dim}); off += act_dim;
      add_tensor(l, "dist_net.sigma.weight", off, {act_dim, act_dim}); off += (long)act_dim * act_dim;
      add_tensor(l, "dist_net.sigma.bias", off, {act_dim}); off += act_dim;
    }
  } else {
    l.out_dim = act_dim;
    l.w_off[L] = off; add_tensor(l, "last.weight", off, {act_dim, d}); off += (long)act_dim * d;
    l.b_off[L] = off; add_tensor(l, "last.bias", off, {act_dim}); off += act_dim;
  }
  l.size = off;
  for (int i = 0; i <= L; ++i) l.w_ms[i] = l.b_ms[i] = l.stride();
  return l;
}

// MCQ's behaviour policy (nets/vae.py:8-66) as two MLP families whose tensors carry the reference's parameter names:
//   encoder e1, e2 (ReLU) + tail [mean ; log_std] stored as one (2Z x VH) matrix;  decoder d1, d2 (ReLU) + tail d3
static NetLayout make_vae_layout(bool encoder, int in_dim, int vh, int out_dim) {
  NetLayout l;
  l.present = true;
  l.in_dim = in_dim; l.L = 2; l.out_dim = encoder ? 2 * out_dim : out_dim;
  const char* n0 = encoder ? "e1" : "d1";
  const char* n1 = encoder ? "e2" : "d2";
  long off = 0;
  int d = in_dim;
  const char* names[2] = {n0, n1};
  for (int i = 0; i < 2; ++i) {
    l.H[i] = vh;
    l.w_off[i] = off; add_tensor(l, std::string(names[i]) + ".weight", off, {vh, d}); off += (long)vh * d;
    l.b_off[i] = off; add_tensor(l, std::string(names[i]) + ".bias", off, {vh}); off += vh;
    d = vh;
  }
  l.w_off[2] = off;
  if (encoder) {
    add_tensor(l, "mean.weight", off, {out_dim, d});
    add_tensor(l, "log_std.weight", off + (long)out_dim * d, {out_dim, d});
    off += 2L * out_dim * d;
    l.b_off[2] = off;
    add_tensor(l, "mean.bias", off, {out_dim});
    add_tensor(l, "log_std.bias", off + out_dim, {out_dim});
    off += 2 * out_dim;
  } else {
    add_tensor(l, "d3.weight", off, {out_dim, d}); off += (long)out_dim * d;
    l.b_off[2] = off; add_tensor(l, "d3.bias", off, {out_dim}); off += out_dim;
  }
  l.size = off;
  for (int i = 0; i <= 2; ++i) l.w_ms[i] = l.b_ms[i] = l.stride();
  return l;
}

// EnsembleCritic (modules/ensemble_critic_module.py:11-31): model.{0,2,..}.weight (K,in,out), .bias (K,1,out)
static NetLayout make_ensemble_layout(int in_dim, const int* hidden, int L, int K) {
  NetLayout l;
  l.present = true; l.ens = true; l.members = K;
  l.in_dim = in_dim; l.L = L; l.out_dim = 1;
  long off = 0;
  int d = in_dim;
  for (int i = 0; i <= L; ++i) {
    const int o = (i == L) ? 1 : hidden[i];
    if (i < L) l.H[i] = hidden[i];
    l.w_off[i] = off; l.w_ms[i] = (long)d * o;
    add_tensor(l, "model." + std::to_string(2 * i) + ".weight", off, {K, d, o});
    off += (long)K * d * o;
    l.b_off[i] = off; l.b_ms[i] = o;
    add_tensor(l, "model." + std::to_string(2 * i) + ".bias", off, {K, 1, o});
    off += (long)K * o;
    d = o;
  }
  l.size = off;
  return l;
}

static int build_layouts(const orl_config& c, NetLayout* lay, long* net_off, bool* is_tgt, long* P_train, long* P_tgt) {
  for (int i = 0; i < ORL_NUM_NETS; ++i) { lay[i] = NetLayout(); net_off[i] = 0; is_tgt[i] = false; }
  if (c.n_hidden < 1 || c.n_hidden > ORL_MAX_HIDDEN) return fail("n_hidden must be in [1,4]");
  if (c.obs_dim < 1 || c.act_dim < 1 || c.batch_size < 1 || c.n_runs < 1) return fail("bad dims");
  if (c.act_dim > 32) return fail("act_dim > 32 not supported");
  const int od = c.obs_dim, ad = c.act_dim, L = c.n_hidden;
  const NetLayout crit = make_mlp_layout(od + ad, c.hidden, L, TAIL_CRITIC, ad);
  long o = 0, t = 0;
  auto train = [&](int id, const NetLayout& l) { lay[id] = l; net_off[id] = o; o += l.stride(); };
  auto target = [&](int id, const NetLayout& l) { lay[id] = l; net_off[id] = t; is_tgt[id] = true; t += l.stride(); };
  if (c.algo == ORL_ALGO_CQL || c.algo == ORL_ALGO_SAC || c.algo == ORL_ALGO_MCQ || c.algo == ORL_ALGO_MOBILE) {
    train(ORL_NET_ACTOR, make_mlp_layout(od, c.hidden, L, TAIL_TANH_GAUSS, ad));
    train(ORL_NET_CRITIC1, crit); train(ORL_NET_CRITIC2, crit);
    target(ORL_NET_CRITIC1_OLD, crit); target(ORL_NET_CRITIC2_OLD, crit);
    if (c.algo == ORL_ALGO_MCQ) {
      if (c.vae_hidden < 1 || c.vae_latent < 1 || c.vae_latent > 64) return fail("MCQ: vae_hidden / vae_latent out of range");
      train(ORL_NET_VAE_ENC, make_vae_layout(true, od + ad, c.vae_hidden, c.vae_latent));
      train(ORL_NET_VAE_DEC, make_vae_layout(false, od + c.vae_latent, c.vae_hidden, ad));
    }
  } else if (c.algo == ORL_ALGO_IQL) {
    train(ORL_NET_ACTOR, make_mlp_layout(od, c.hidden, L, TAIL_GAUSS, ad, c.actor_dropout > 0.f ? 3 : 2));
    train(ORL_NET_CRITIC1, crit); train(ORL_NET_CRITIC2, crit);
    train(ORL_NET_CRITIC_V, make_mlp_layout(od, c.hidden, L, TAIL_CRITIC, ad));
    target(ORL_NET_CRITIC1_OLD, crit); target(ORL_NET_CRITIC2_OLD, crit);
  } else if (c.algo == ORL_ALGO_TD3BC) {
    const NetLayout act = make_mlp_layout(od, c.hidden, L, TAIL_DET, ad);
    train(ORL_NET_ACTOR, act);
    train(ORL_NET_CRITIC1, crit); train(ORL_NET_CRITIC2, crit);
    target(ORL_NET_CRITIC1_OLD, crit); target(ORL_NET_CRITIC2_OLD, crit);
    target(ORL_NET_ACTOR_OLD, act);
  } else if (c.algo == ORL_ALGO_EDAC) {
    if (c.num_critics < 2 || c.num_critics > 64) return fail("num_critics must be in [2,64]");
    train(ORL_NET_ACTOR, make_mlp_layout(od, c.hidden, L, TAIL_TANH_GAUSS, ad));
    const NetLayout ens = make_ensemble_layout(od + ad, c.hidden, L, c.num_critics);
    train(ORL_NET_CRITIC1, ens);
    target(ORL_NET_CRITIC1_OLD, ens);
  } else if (c.algo == ORL_ALGO_RCSL) {
    train(ORL_NET_ACTOR, make_mlp_layout(od + 1, c.hidden, L, TAIL_LINEAR, ad));      // MLP(obs_dim + 1, hidden, act_dim) of RcslModule
  } else if (c.algo == ORL_ALGO_RCSL_GAUSS) {
    train(ORL_NET_ACTOR, make_mlp_layout(od + 1, c.hidden, L, TAIL_LINEAR_GAUSS, ad));      // RcslGaussianModule: backbone + DiagGaussian heads
  } else if (c.algo == ORL_ALGO_AUTOREG) {
    // AutoregressivePolicy.model: [Linear, LeakyReLU] x (L + 1), keys model.{0, 2, ...}; the last Linear has the two outputs (mean, logstd)
    if (ad > AR_AMAX) return fail("AUTOREG: act_dim beyond 32");
    train(ORL_NET_ACTOR, make_mlp_layout(od + 2 * ad, c.hidden, L, TAIL_LINEAR, 2, 2, "model."));
  } else {
    return fail("unknown algorithm id");
  }
  *P_train = o; *P_tgt = t;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Engine basics
// ---------------------------------------------------------------------------------------------
Engine::~Engine() {
  for (int i = 0; i < 2; ++i) {
    if (graph_exec[i]) hipGraphExecDestroy(graph_exec[i]);
    if (graph[i]) hipGraphDestroy(graph[i]);
  }
  for (auto& e : ev_pool) hipEventDestroy(e);
  for (auto& e : ml_events) hipEventDestroy(e);
  if (ml_counts) hipHostFree(ml_counts);
  mem.free_all();
  if (stream) hipStreamDestroy(stream);
}

void Engine::drop_graphs() {
  for (int i = 0; i < 2; ++i) {
    if (graph_exec[i]) { hipGraphExecDestroy(graph_exec[i]); graph_exec[i] = nullptr; }
    if (graph[i]) { hipGraphDestroy(graph[i]); graph[i] = nullptr; }
  }
}

float* Engine::raw_alloc(size_t bytes) {
  char* p = nullptr;
  return mem.alloc(&p, bytes) ? nullptr : (float*)p;
}

void Engine::drop(Mat& m) {
  if (m.p) { range_watch.erase(m.p); vals_dead.erase(m.p); mem.free(m.p); }
  if (m.bits) { bits_live.erase(m.bits); mem.free(m.bits); }
  m = Mat();
}

int Engine::room(RowScratch& s, long rows) {
  if (rows <= s.cap) return 0;
  ORL_HIP(hipStreamSynchronize(stream));
  for (auto& x : s.mats) drop(*x.m);
  for (const char* t : s.taps) taps.erase(t);
  s.cap = 0;
  for (auto& x : s.mats) {
    x.m->p = raw_alloc(sizeof(float) * (size_t)rows * x.factor * x.pitch * x.nets * R);
    x.m->pitch = x.pitch;
    if (!x.m->p) return fail(s.what);
  }
  s.cap = rows;
  return 0;
}

Mat Engine::alloc(const std::string& name, long rows, int pitch, int nets) {
  Mat m;
  const long per_net = rows * pitch;
  const long per_run = per_net * nets;
  m.p = raw_alloc(sizeof(float) * per_run * R);
  m.rs = per_run;
  m.cs = per_net;
  m.pitch = pitch;
  if (pitch >= 128 && (pitch & 127) == 0) {          // hidden-activation shaped: room for the packed ReLU masks
    m.bg = pitch / 32;                                 // one 32-bit word per 32 columns
    m.bcs = rows * m.bg; m.brs = m.bcs * nets;
    m.bits = (unsigned int*)raw_alloc(sizeof(unsigned int) * m.brs * R);
  }
  ws[name] = m;
  ws_len[name] = per_run;
  return m;
}

std::vector<std::string> Engine::alloc_layers(const std::string& stem, long rows, int nets, int upto, int width) {
  const int n = upto < 0 ? L : upto;
  std::vector<Mat>& fam = families[stem];
  fam.assign(width > 0 ? n : L, Mat());
  std::vector<std::string> names;
  for (int i = 0; i < n; ++i) {
    names.push_back(stem + std::to_string(i));
    fam[i] = alloc(names.back(), rows, width > 0 ? width : cfg.hidden[i], nets);
  }
  return names;
}

float* Engine::net_ptr(int run, int net) const {
  if (net < 0 || net >= ORL_NUM_NETS || !lay[net].present) return nullptr;
  if (net_is_target[net]) return arena + (long)R * P_train + (long)run * P_tgt + net_off[net];
  return arena + (long)run * P_train + net_off[net];
}

NetRef Engine::net_ref(int net, int members) const {
  NetRef r;
  r.base = net_ptr(0, net);
  r.rs = net_is_target[net] ? P_tgt : P_train;
  r.g_off = net_off[net];
  r.lay = &lay[net];
  r.nz1 = members;
  return r;
}

void Engine::prof_begin(const char* name, double flops, double bytes) {
  if (!prof_on) return;
  while (ev_pool.size() < ev_used + 2) {
    hipEvent_t e;
    hipEventCreate(&e);
    ev_pool.push_back(e);
  }
  ProfEntry pe;
  pe.name = name;
  pe.flops = flops;
  pe.bytes = bytes;
  pe.a = ev_pool[ev_used++];
  pe.b = ev_pool[ev_used++];
  hipEventRecord(pe.a, stream);
  prof.push_back(pe);
}
void Engine::prof_end() {
  if (!prof_on) return;
  hipEventRecord(prof.back().b, stream);
}

float* Engine::gscale_slot() {
  if (!split_scales()) return nullptr;
  if (gscale_next >= GSCALE_SLOTS) { fail("grad_scale: out of slots"); return nullptr; }
  return gscale_buf + (long)(gscale_next++) * R;
}

// split precision: choose the dynamic scale of a backward pass from its seed (kernels.h: k_grad_scale); null at precision 0
const float* Engine::grad_scale(const Mat& seed, int rows, int cols, int nets, const char* tag) {
  if (!split_scales()) return nullptr;
  if (gscale_next >= GSCALE_SLOTS) { fail("grad_scale: out of slots"); return nullptr; }
  float* out = gscale_buf + (long)(gscale_next++) * R;
  GradScaleP g;
  g.seed = seed.p; g.rs = seed.rs; g.cs = seed.cs; g.rows = rows; g.cols = cols; g.pitch = seed.pitch; g.nets = nets; g.out = out;
  prof_begin((std::string(tag) + ".gscale").c_str(), 0);
  hipLaunchKernelGGL(k_grad_scale, dim3(R), dim3(256), 0, stream, g);
  prof_end();
  return out;
}

void Engine::watch_range(const Mat& m, int rows, int cols, int nets, const char* what) {
  if (!split_scales() || !m.p) return;
  RangeWatch w{m, rows, cols, nets, what ? what : ""};
  range_watch[m.p] = w;
}

// every matrix the last enqueued step feeds to the split-precision MFMAs at operand scale 1 (dead ones -- never stored by the forward pass --
// skipped), then the parameters of every net (operand scale ORL_WSCALE)
int Engine::range_scan() {
  if (!split_scales()) return 0;
  const float lim = 65504.0f;
  for (auto& kv : range_watch) {
    const RangeWatch& w = kv.second;
    if (vals_dead.count(w.m.p)) continue;
    hipLaunchKernelGGL(k_range_scan, dim3(R), dim3(256), 0, stream, (const float*)w.m.p, w.m.rs, w.m.cs, w.nets, w.rows, w.cols, w.m.pitch, lim, health);
  }
  hipLaunchKernelGGL(k_range_scan, dim3(R), dim3(256), 0, stream, (const float*)arena, P_train, 0L, 1, 1, (int)P_train, (int)P_train, lim / ORL_WSCALE, health);
  if (P_tgt > 0)
    hipLaunchKernelGGL(k_range_scan, dim3(R), dim3(256), 0, stream, (const float*)(arena + (long)R * P_train), P_tgt, 0L, 1, 1, (int)P_tgt, (int)P_tgt, lim / ORL_WSCALE, health);
  return hipGetLastError() == hipSuccess ? 0 : fail("range scan launch");
}

// Called after the stream has been synchronised: folds what the host just read (non-finite metrics) and what the kernels raised into the
// sticky per-run flags.  A split-precision engine gets the operands of its last step scanned for the fp16-plane range when a run turned
// non-finite (so the report can name the cause) and every RANGE_SCAN_EVERY steps: an activation beyond 65504 does NOT surface by itself --
// its hi / lo planes are +inf / -inf, the MFMA adds them to the NaN 0xffc00000 (tools/probes/nan_sign_probe.hip, measured on gfx950), and
// a ReLU (integer view or v_max_f32 alike) turns a sign-bit NaN into +0: the row's next layer is silently all zero.  The scan is a pass
// over the workspaces (~0.1 % of 256 steps); steps_done < 0: scan now (orl_health_check).
// *any = OR over the runs.  Sets the error string (not the return code) when a flag is up.
int Engine::health_update(const float* metrics, long steps_done, unsigned int* any) {
  std::vector<unsigned int> dv(R);
  ORL_HIP(hipMemcpy(dv.data(), health, sizeof(unsigned int) * R, hipMemcpyDeviceToHost));
  bool fresh = false;
  for (int r = 0; r < R; ++r) {
    unsigned int f = dv[r];
    if (metrics)
      for (int k = 0; k < nm; ++k) if (!std::isfinite(metrics[(long)r * nm + k])) f |= ORL_HEALTH_NONFINITE_LOSS;
    if (f & ~health_host[r]) fresh = true;
    health_host[r] |= f;
  }
  steps_since_scan += steps_done > 0 ? steps_done : 0;
  if (split_scales() && (fresh || steps_done < 0 || steps_since_scan >= RANGE_SCAN_EVERY)) {
    steps_since_scan = 0;
    if (range_scan()) return -1;
    ORL_HIP(hipStreamSynchronize(stream));
    ORL_HIP(hipMemcpy(dv.data(), health, sizeof(unsigned int) * R, hipMemcpyDeviceToHost));
    for (int r = 0; r < R; ++r) health_host[r] |= dv[r];
  }
  unsigned int all = 0;
  for (int r = 0; r < R; ++r) all |= health_host[r];
  if (any) *any = all;
  if (all) {
    std::string msg = "unhealthy run(s):";
    int listed = 0;
    for (int r = 0; r < R && listed < 8; ++r) {
      if (!health_host[r]) continue;
      msg += " run " + std::to_string(r) + " [";
      if (health_host[r] & ORL_HEALTH_NONFINITE_LOSS) msg += " non-finite loss";
      if (health_host[r] & ORL_HEALTH_NONFINITE_GRAD) msg += " non-finite gradient";
      if (health_host[r] & ORL_HEALTH_SPLIT_RANGE) msg += " operand beyond the split-precision range (|x| >= 65504 or |w| >= 1023.5: use precision 0 or normalise the inputs)";
      msg += " ]";
      ++listed;
    }
    set_error(msg);
  }
  return 0;
}

#define ORL_LAUNCH(tag, kernel, grid, block, ...)                                      \
  do {                                                                                 \
    prof_begin(tag, 0);                                                                \
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);                   \
    prof_end();                                                                        \
    if (hipGetLastError() != hipSuccess) return fail(std::string(tag) + ": launch failed"); \
  } while (0)

template <int PA, int PB, int EPI>
static int run_gemm(Engine* e, int cfg, const GemmP& p, int nz, const char* tag, bool a_kpad = false) {
  const double flops = 2.0 * p.M * (double)p.N * p.K * nz;
  // algorithmic bytes: each operand read once, the result written once (split-K: one slab per split), mask read once
  const double bytes = 4.0 * nz * ((double)p.M * p.K + (double)p.N * p.K + (double)p.M * p.N * (EPI == E_WGRAD ? p.ksplit : 1) +
                                   (EPI == E_MASK ? (double)p.M * p.N / (p.aux_bits ? 32.0 : 1.0) : 0.0));
  double bytes_adj = bytes;
  if (EPI == E_MASK && p.w0_out) bytes_adj += 4.0 * nz * ((double)p.M * p.w0_xsr - (p.C ? 0.0 : (double)p.M * p.N));
  return e->timed("gemm", tag, false, flops + (EPI == E_MASK && p.w0_out ? 2.0 * p.M * (double)p.N * (p.w0_in + 1) * nz : 0.0), bytes_adj,
                  [&] { return launch_gemm<PA, PB, EPI>(cfg, p, nz, e->stream, a_kpad, e->force_scalar, e->mm_prec()); });
}

// gradient w.r.t. a layer output [M x out].  rank1: dz = (H > 0) ? rowv[m] * w_tail[n] : 0 (never materialised)
struct DY {
  bool rank1 = false;
  Mat m;     // plain: the gradient matrix ; rank1: post-ReLU activation H of the top hidden layer
  Mat rowv;  // rank1: dLoss/dq per row
  static DY plain(const Mat& m) { DY d; d.m = m; return d; }
  static DY virt(const Mat& H, const Mat& dq) { DY d; d.rank1 = true; d.m = H; d.rowv = dq; return d; }
};

// out[m] += the column-tile partial sums a fused single-output tail left in `part` ([nparts][M] per net)
int Engine::tail_add(const ZOut& out, long out_sm, const ZOut& part, int nparts, int M, int nz1, const char* tag) {
  TailAddP t;
  t.out = out.p; t.o_s0 = out.s0; t.o_s1 = out.s1; t.o_sm = out_sm;
  t.part = part.p; t.p_s0 = part.s0; t.p_s1 = part.s1; t.p_ts = M; t.nparts = nparts; t.M = M; t.nz1 = nz1;
  prof_begin((std::string(tag) + ".tail_add").c_str(), 0);
  hipLaunchKernelGGL(k_tail_add, dim3((M + 255) / 256, R * nz1), dim3(256), 0, stream, t);
  prof_end();
  return hipGetLastError() == hipSuccess ? 0 : fail("tail_add launch");
}

// Y = relu(X W^T + b) and the mask words of Y for a 256 x 256 layer; the caller adds the fused tail / first layer / three-plane scratch.
// dmask != null: the plain dgrad mode -- X = the gradient w.r.t. the layer's output, Y = (X B^T) (.) dmask with B = the weights viewed transposed
WsFwdP Engine::ws_fwd_p(const Mat& X, int M, const NetRef& nr, int layer, const Mat& Y, const Mat* dmask) const {
  const NetLayout& l = *nr.lay;
  const int in = l.layer_in(layer), out = l.layer_out(layer);
  WsFwdP w;
  memset(&w, 0, sizeof(w));
  w.X = X.z(); w.x_pitch = X.pitch;
  w.W = nr.w(layer);
  w.Y = Y.zo(); w.y_pitch = Y.pitch;
  if (dmask) {
    // B[n = input unit][k = output unit]: nn.Linear W (out, in) -> element (k, n) at k * in + n; EnsembleLinear (in, out) -> n * out + k
    if (l.ens) { w.w_sn = out; w.w_sk = 1; } else { w.w_sn = 1; w.w_sk = in; }
    w.dmask = dmask->zbits(); w.dm_g = dmask->bg;
    w.gscale = cur_gscale;
  } else {
    if (l.ens) { w.w_sn = 1; w.w_sk = out; } else { w.w_sn = in; w.w_sk = 1; }      // EnsembleLinear keeps (in, out)-major weights
    w.bias = nr.b(layer);
    w.mb = Y.zbits(); w.mb_g = Y.bg;
  }
  w.M = M; w.nz1 = nr.nz1; w.f32 = ws_f32();
  return w;
}

// fuse_X0 (layer == 1 only): X = hs[0] has not been computed yet; it is relu(fuse_X0 W0^T + b0).  The weight-stationary kernel
// produces it inside this launch (stores it to X for the backward pass); any other path first runs layer 0 on its own.
int Engine::linear_fwd(const Mat& X, int M, const NetRef& nr, int layer, const Mat& Y, int epi, const Mat* maskH,
                       const char* tag, int in_row0, int in_rows, const Mat* tail_out, bool* tail_fused, const Mat* fuse_X0, const char* tag0,
                       const float* x_dscale) {
  const NetLayout& l = *nr.lay;
  const int in = l.layer_in(layer), out = l.layer_out(layer);
  if (in_rows < 0) in_rows = in;
  if (!x_dscale) {                                    // an input / activation operand (scale 1): orl_health_check scans it for the fp16-plane range
    watch_range(X, M, in_rows, X.cs ? nr.nz1 : 1, tag);
    if (fuse_X0) watch_range(*fuse_X0, M, l.layer_in(0), fuse_X0->cs ? nr.nz1 : 1, tag0 ? tag0 : tag);
  }
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.b_scale = ORL_WSCALE; p.a_dscale = x_dscale;      // split precision: static scale of the weight operand, dynamic one of a gradient-like input
  p.A = X.z();
  p.a_sr = X.pitch; p.a_sk = 1;
  p.B = nr.w(layer);
  if (l.ens) { p.B.p += (long)in_row0 * out; p.b_sr = 1; p.b_sk = out; p.b_rlim = out & ~3; }
  else { p.B.p += in_row0; p.b_sr = in; p.b_sk = 1; }
  p.C = Y.p; p.c_s0 = Y.rs; p.c_s1 = Y.cs; p.c_sr = Y.pitch; p.c_sn = 1;
  p.M = M; p.N = out; p.K = in_rows;
  const bool a_kpad = X.pitch >= ((in_rows + 3) & ~3);   // input matrices are zero-padded to 16 B rows
  p.nz1 = nr.nz1; p.ksplit = 1;
  vals_dead.erase(Y.p);
  p.bias = nr.b(layer);
  if (maskH) {
    p.aux = maskH->z(); p.aux_sr = maskH->pitch;
    // the ReLU mask as packed bits (1/32 of the bytes) when the forward pass that produced the activation left them behind
    if (epi == E_MASK && !leaky && maskH->bits && bits_live.count(maskH->bits) && out == maskH->pitch && aligned16(maskH->p) && (maskH->pitch & 3) == 0) {
      p.aux_bits = maskH->bits; p.xb_s0 = maskH->brs; p.xb_s1 = maskH->bcs; p.xb_g = maskH->bg;
    }
  }
  const int nz = R * nr.nz1;
  int cfg = pick_cfg(p.M, p.N, p.K, nz);
  if (cfg == CFG_SQ) cfg = CFG_SQ8;          // forward products: the 8-wave flavour of the 128 x 128 tile measured faster
  // weight-stationary row-streaming kernel (csrc/ws_gemm.h) for the many-row 256 x 256 hidden layers in split-bf16 precision
  if (epi == E_BIAS_RELU && ws_precision_ok() && !no_ws && !force_scalar && in_row0 == 0 && in_rows == in &&
      Y.bits && Y.pitch == out && (long)M * nz >= ws_fwd_min_rows) {   // measured faster than the 16x64 tiles from 16 x 256 rows up
    WsFwdP w = ws_fwd_p(X, M, nr, layer, Y, nullptr);
    const bool want_tail = tail_out && tail_fused && layer == l.L - 1 && l.out_dim == 1;
    if (want_tail) { w.tw = nr.w(l.L); w.tb = nr.b(l.L); w.tq = tail_out->zo(); w.tq_sm = tail_out->pitch; }
    // With the single-output tail folded in, the backward pass of a many-row batch needs only the mask bits of this activation
    // (ws_dgrad_w0 / ws_wgrad's derived tail gradients): the activation itself then never goes to HBM.
    const bool elide = want_tail && layer >= 1 && (fwd_only || (elide_top && !l.ens && ws_wgrad_rows_ok(M, nz)));
    if (elide) w.Y.p = nullptr;
    const bool ws_ok = ws_fwd_supported(w, in, out);
    bool fused0 = false;
    if (ws_ok && fuse_X0 && layer == 1 && X.bits && X.pitch == in) {
      w.X0 = fuse_X0->z(); w.x0_pitch = fuse_X0->pitch; w.in0 = l.layer_in(0);
      w.W0 = nr.w(0);
      if (l.ens) { w.w0_sn = 1; w.w0_sk = l.layer_out(0); } else { w.w0_sn = l.layer_in(0); w.w0_sk = 1; }
      w.b0 = nr.b(0);
      w.mb0 = X.zbits(); w.mb0_g = X.bg;
      fused0 = ws_fwd01_supported(w) && aligned16(fuse_X0->p);
      if (!fused0) w.X0.p = nullptr;
      else if (fwd_only || (!want_tail && recompute_h0_ok(l, layer, M, nz))) w.x0_discard = 1;      // (a three-layer net's middle-layer wgrad rebuilds h0 from the input rows)
    }
    if (fuse_X0 && !fused0) {      // layer 0 on its own, then this layer
      if (linear_fwd(*fuse_X0, M, nr, 0, X, E_BIAS_RELU, nullptr, tag0 ? tag0 : tag)) return -1;
      fuse_X0 = nullptr;
    }
    if (ws_ok) {
      // precision 2: the fused first + second layer + tail forward of a many-row single-output net has a three-plane flavour (ws_fwd3.hip);
      // its two column halves leave two tail partial sums
      bool fwd3 = false;
      if (p3(1) && (fused0 || !w.X0.p) && ws_dump && (!want_tail || ws.count("tq_scratch"))) {
        bool room = true;
        if (want_tail) {
          const Mat& sc = ws.at("tq_scratch");
          room = (long)M <= sc.cs && nr.nz1 <= tq_scratch_nets;
          if (room) w.tq2 = sc.zo();
        }
        if (room) {
          w.np3 = 1; w.dump = ws_dump;
          fwd3 = ws_fwd3_supported(w, in, out);
          if (!fwd3) { w.np3 = 0; w.tq2.p = nullptr; w.dump = nullptr; }
        }
      }
      const double f0 = fused0 ? 2.0 * M * (double)in * (w.in0 + 1) * nz : 0.0;
      if (fused0) bits_live.insert(X.bits);
      if (w.x0_discard) vals_dead.insert(X.p);
      else if (fused0) vals_dead.erase(X.p);
      if (M >= 1024 && !fwd_only) w.lab_clk = lab_clk(64);      // (lab builds: the critic pass)
      if (timed("ws_fwd", tag, fwd3, f0 + 2.0 * M * (double)out * (in + (want_tail ? 1 : 0)) * nz,
                4.0 * nz * ((fused0 ? (double)M * w.x0_pitch : 0.0) + (w.x0_discard ? (double)M * in / 32 : (double)M * in) + (double)out * in +
                            (elide ? (double)M * out / 32 : (double)M * out)),
                [&] { return fwd3 ? launch_ws_fwd3(w, nz, ws_blocks_per_problem(M / WS_ROWS, 2 * nz, 10, 1 << 20, ws_geo), stream) : launch_ws_fwd(w, nz, stream, ws_geo); })) return -1;
      if (fwd3 && want_tail && tail_add(w.tq, w.tq_sm, w.tq2, 1, M, nr.nz1, tag)) return -1;
      bits_live.insert(Y.bits);
      if (elide) vals_dead.insert(Y.p);
      if (tail_fused) *tail_fused = want_tail;
      return 0;
    }
  }
  if (fuse_X0) {                   // no fused path: layer 0 first
    if (linear_fwd(*fuse_X0, M, nr, 0, X, epi, nullptr, tag0 ? tag0 : tag)) return -1;
  }
  if (Y.bits) {
    if (epi == E_BIAS_RELU && !force_scalar && out == Y.pitch && mb_supported(cfg, p)) {
      p.mb_out = Y.bits; p.mb_s0 = Y.brs; p.mb_s1 = Y.bcs; p.mb_g = Y.bg;
      bits_live.insert(Y.bits);
    } else bits_live.erase(Y.bits);
  }
  if (tail_fused) *tail_fused = false;
  int tq_parts = 0;
  if (tail_out && tail_fused && epi == E_BIAS_RELU && layer == l.L - 1 && l.out_dim == 1 && !force_scalar && ws.count("tq_scratch")) {
    const ZPtr tw = nr.w(l.L);
    tq_parts = tq_fused_parts(cfg, p, tw.p, tw.s0, tw.s1);
    const Mat& sc = ws.at("tq_scratch");
    if (tq_parts >= 1 && (long)(tq_parts - 1) * M <= sc.cs && nr.nz1 <= tq_scratch_nets) {
      p.tq_w = tw;
      p.tq_b = nr.b(l.L);
      p.tq_out = tail_out->p; p.tq_s0 = tail_out->rs; p.tq_s1 = tail_out->cs; p.tq_sm = tail_out->pitch;
      p.tq_part = sc.p; p.tq_ps0 = sc.rs; p.tq_ps1 = sc.cs; p.tq_ts = M;
      *tail_fused = true;
    } else tq_parts = 0;
  }
  if (tq_parts >= 1) {
    if (run_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_RELU>(this, cfg, p, nz, tag, a_kpad)) return -1;
    if (tq_parts > 1) return tail_add(tail_out->zo(), tail_out->pitch, ws.at("tq_scratch").zo(), tq_parts - 1, M, nr.nz1, tag);
    return 0;
  }
  switch (epi) {
    case E_BIAS_RELU: return run_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_RELU>(this, cfg, p, nz, tag, a_kpad);
    case E_BIAS: return run_gemm<PA_PLAIN, PB_PLAIN, E_BIAS>(this, CFG_AUTO, p, nz, tag, a_kpad);
    case E_MASK: return run_gemm<PA_PLAIN, PB_PLAIN, E_MASK>(this, CFG_AUTO, p, nz, tag, a_kpad);
    case E_BIAS_LEAKY: return run_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_LEAKY>(this, cfg, p, nz, tag, a_kpad);
    case E_LEAKY_MASK: return run_gemm<PA_PLAIN, PB_PLAIN, E_LEAKY_MASK>(this, CFG_AUTO, p, nz, tag, a_kpad);
    default: return run_gemm<PA_PLAIN, PB_PLAIN, E_PLAIN>(this, CFG_AUTO, p, nz, tag, a_kpad);
  }
}

// Weight-stationary dgrad into the first hidden activation (mask words maskH).  Incoming gradient: dy.rank1 -> (mask words of the top activation,
// dq, w_tail), else the materialised dz1 (PLAIN).  Result: w0_X != null -> the layer-0 gradient slabs (*slabs, one per workgroup), else dz0
// stored to dX.  max_blocks caps the workgroups per net.  Returns 1 when the kernels do not serve the shape (nothing enqueued), else 0 / -1.
int Engine::ws_dgrad(const DY& dy, int M, const NetRef& nr, int layer, const Mat& maskH, const Mat* w0_X, const Mat* dX, int max_blocks,
                     const char* tag, int* slabs) {
  const NetLayout& l = *nr.lay;
  const int in = l.layer_in(layer), out = l.layer_out(layer), nz = R * nr.nz1;
  WsDgradP w;
  memset(&w, 0, sizeof(w));
  if (dy.rank1) {
    w.abits = dy.m.zbits(); w.ab_g = dy.m.bg;
    w.dq = dy.rowv.z(); w.dq_sm = dy.rowv.pitch;
    w.wt = nr.w(l.L);
  } else { w.Z = dy.m.z(); w.z_pitch = dy.m.pitch; }
  w.xbits = maskH.zbits(); w.xb_g = maskH.bg;
  w.W = nr.w(layer);
  // nn.Linear keeps (out, in)-major weights, EnsembleLinear (in, out)-major ones: the same holds for the gradient slabs
  if (l.ens) { w.w_sn = out; w.w_sk = 1; } else { w.w_sn = 1; w.w_sk = in; }
  if (w0_X) {
    w.X = w0_X->z(); w.x_pitch = w0_X->pitch; w.in0 = l.layer_in(0);
    float* g = grads + nr.g_off;
    w.w0_out = g + l.w_off[0]; w.b0_out = g + l.b_off[0];
    w.o_rs = (long)max_slab * P_train; w.o_ms = l.w_ms[0]; w.ob_ms = l.b_ms[0]; w.o_ks = P_train;
    if (l.ens) { w.o_sr = 1; w.o_sc = l.layer_out(0); } else { w.o_sr = l.layer_in(0); w.o_sc = 1; }
    w.gscale = cur_gscale;
  } else { w.C = dX->zo(); w.c_pitch = dX->pitch; }      // (no dynamic scale: the stored values are the true ones)
  w.M = M; w.nz1 = nr.nz1; w.f32 = ws_f32();
  if (!ws_dgrad_supported(w, out, in)) return 1;
  const bool d3 = p3(2) && ws_dgrad3_supported(w, out, in);      // precision 2: three planes, two workgroups (column halves) per slab
  const int per_z = ws_dgrad_blocks(M, d3 ? 2 * nz : nz, max_blocks, ws_geo);
  const double flops = 2.0 * M * (double)in * (out + (w0_X ? w.in0 + 1 : 0)) * nz;
  const double bytes = nz * (4.0 * in * out + (dy.rank1 ? M * (double)(in + out) / 8 : 4.0 * M * (double)out + M * (double)in / 8) +
                             (w0_X ? 4.0 * M * (w.x_pitch + 1) + 4.0 * per_z * in * (w.in0 + 1) : 4.0 * M * (in + 1)));
  if (timed("ws_dgrad", tag, d3, flops, bytes, [&] { return d3 ? launch_ws_dgrad3_w0(w, nz, per_z, stream) : launch_ws_dgrad_w0(w, nz, per_z, stream); })) return -1;
  if (slabs) *slabs = per_z;
  return 0;
}

int Engine::linear_dgrad(const DY& dy, int M, const NetRef& nr, int layer, int col0, int ncols, const Mat* maskH,
                         const Mat& dX, const char* tag, const Mat* w0_X, bool store_dx, int* w0_slabs) {
  const NetLayout& l = *nr.lay;
  const int in = l.layer_in(layer), out = l.layer_out(layer);
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.a_dscale = cur_gscale; p.b_scale = ORL_WSCALE;     // split precision: A = a gradient matrix of the current backward pass, B = weights
  if (mm_prec() == P_SPLIT3) p.a_scale = ORL_GSCALE3;   // three planes: 2^5 more headroom above fp16's 2^-24 grid for the matrix's small elements
  p.A = dy.m.z();
  p.a_sr = dy.m.pitch; p.a_sk = 1;
  if (dy.rank1) {
    p.a_trans = 0;
    p.rowv = dy.rowv.z();
    p.colv = nr.w(l.L);
  }
  p.B = nr.w(layer);
  if (l.ens) { p.B.p += (long)col0 * out; p.b_sr = out; p.b_sk = 1; }
  else { p.B.p += col0; p.b_sr = 1; p.b_sk = in; p.b_rlim = (in - col0) & ~3; }
  p.C = dX.p; p.c_s0 = dX.rs; p.c_s1 = dX.cs; p.c_sr = dX.pitch; p.c_sn = 1;
  p.M = M; p.N = ncols; p.K = out;
  p.nz1 = nr.nz1; p.ksplit = 1;
  if (maskH) { p.aux = maskH->z(); p.aux_sr = maskH->pitch; }
  const int nz = R * nr.nz1;
  if (w0_slabs) *w0_slabs = 0;
  if (maskH && !leaky && maskH->bits && bits_live.count(maskH->bits) && ncols == maskH->pitch && aligned16(maskH->p) && (maskH->pitch & 3) == 0) {
    p.aux_bits = maskH->bits; p.xb_s0 = maskH->brs; p.xb_s1 = maskH->bcs; p.xb_g = maskH->bg;
  }
  // weight-stationary fused kernel (csrc/ws_gemm.h): top-layer dgrad from mask bits + layer-0 weight gradient, nothing stored
  if (w0_X && w0_slabs && !store_dx && maskH && dy.rank1 && layer == 1 && col0 == 0 && !l.ens && !force_scalar &&
      ws_precision_ok() && p.aux_bits && dy.m.bits && bits_live.count(dy.m.bits) && out == dy.m.pitch &&
      ncols == in && (long)M * nz >= ws_bwd_min_rows) {
    const int rc = ws_dgrad(dy, M, nr, layer, *maskH, w0_X, nullptr, max_slab, tag, w0_slabs);
    if (rc <= 0) return rc;
  }
  // same kernel, storing variant (no layer-0 gradient): e.g. the critic backward of the actor loss, where dz0 feeds dL/da
  if (!(w0_X && w0_slabs) && maskH && dy.rank1 && col0 == 0 && !force_scalar && ws_precision_ok() && p.aux_bits &&
      dy.m.bits && bits_live.count(dy.m.bits) && out == dy.m.pitch && ncols == in && dX.pitch >= in && (long)M * nz >= ws_bwd_min_rows) {
    const int rc = ws_dgrad(dy, M, nr, layer, *maskH, nullptr, &dX, 1 << 20, tag, nullptr);
    if (rc <= 0) return rc;
  }
  // the same fused kernel fed with a MATERIALISED gradient (a three-layer net's middle layer): dz0 = 1[h0 > 0] (dz1 W1) never leaves the
  // registers, dW0 / db0 come out as one slab per workgroup
  if (w0_X && w0_slabs && !store_dx && maskH && !dy.rank1 && layer == 1 && col0 == 0 && !force_scalar && ws_precision_ok() &&
      p.aux_bits && dy.m.pitch == out && ncols == in && (long)M * nz >= ws_dgrad_plain_min_rows) {
    const int rc = ws_dgrad(dy, M, nr, layer, *maskH, w0_X, nullptr, max_slab, tag, w0_slabs);
    if (rc <= 0) return rc;
  }
  if (w0_X && w0_slabs && maskH && layer == 1 && col0 == 0 && !l.ens && !force_scalar && !leaky) {      // (the fused epilogue bakes in the ReLU mask)
    // fuse the layer-0 weight / bias gradient into this launch's epilogue (one slab per row tile)
    const int slabs = w0_fused_slabs(p, nz, l.layer_in(0), w0_X->pitch, w0_X->p, w0_X->rs, w0_X->cs, max_slab);
    if (slabs > 0) {
      float* g = grads + nr.g_off;
      p.w0_x = w0_X->z(); p.w0_xsr = w0_X->pitch; p.w0_in = l.layer_in(0);
      p.w0_out = g + l.w_off[0]; p.w0_bias = g + l.b_off[0];
      p.w0_s0 = (long)max_slab * P_train; p.w0_s1 = l.w_ms[0]; p.w0_bs1 = l.b_ms[0]; p.w0_ks = P_train; p.w0_sr = l.layer_in(0);
      if (!store_dx) p.C = nullptr;
      *w0_slabs = slabs;
    }
  }
  // plain (materialised) dz through a 256 x 256 layer with the ReLU mask of the receiving activation: the weight-stationary kernel
  // in gradient mode (B = the weights viewed transposed, epilogue = mask from bits)
  if (!dy.rank1 && !p.w0_out && maskH && p.aux_bits && col0 == 0 && ncols == in && ws_precision_ok() && !force_scalar &&
      dy.m.pitch == out && dX.pitch == in && (long)M * nz >= ws_bwd_min_rows) {
    const WsFwdP w = ws_fwd_p(dy.m, M, nr, layer, dX, maskH);
    if (ws_fwd_supported(w, out, in)) {
      const bool f3 = p3(2) && ws_fwd3_supported(w, out, in);       // precision 2: three planes of dz and of the weights (column halves)
      return timed("ws dgrad", tag, f3, 2.0 * M * (double)in * out * nz, nz * (4.0 * M * out + 4.0 * in * out + 4.0 * M * in + M * (double)in / 8),
                   [&] { return f3 ? launch_ws_fwd3(w, nz, ws_blocks_per_problem(M / WS_ROWS, 2 * nz, 10, 1 << 20, ws_geo), stream) : launch_ws_fwd(w, nz, stream, ws_geo); });
    }
  }
  if (dy.rank1) {
    if (maskH && dy.m.bits && bits_live.count(dy.m.bits) && out == dy.m.pitch) {
      // the virtual dz of the top hidden layer from its packed ReLU mask: the activation matrix is not read at all
      GemmP q = p;
      q.a_bits = dy.m.bits; q.ab_s0 = dy.m.brs; q.ab_s1 = dy.m.bcs; q.ab_g = dy.m.bg;
      const int tcfg = pick_cfg(q.M, q.N, q.K, nz);
      if (rank1_bits_supported(tcfg, q, force_scalar)) {
        const double flops = 2.0 * q.M * (double)q.N * q.K * nz + (q.w0_out ? 2.0 * q.M * (double)q.N * (q.w0_in + 1) * nz : 0.0);
        const double bytes = nz * (4.0 * q.N * q.K + q.M * (double)q.K / 8 + (q.C ? 4.0 * q.M * q.N : 0.0) +
                                   (q.aux_bits ? q.M * (double)q.N / 8 : 4.0 * q.M * q.N) + (q.w0_out ? 4.0 * q.M * q.w0_xsr : 0.0));
        return timed("gemm", tag, false, flops, bytes, [&] { return launch_gemm_rank1_bits<E_MASK>(tcfg, q, nz, stream, mm_prec()); });
      }
    }
    if (vals_dead.count(dy.m.p)) return fail(std::string("dgrad ") + tag + ": the activation values were not stored by the forward pass");
    if (maskH) return run_gemm<PA_RANK1, PB_PLAIN, E_MASK>(this, CFG_AUTO, p, nz, tag);
    return run_gemm<PA_RANK1, PB_PLAIN, E_PLAIN>(this, CFG_AUTO, p, nz, tag);
  }
  if (maskH && leaky) return run_gemm<PA_PLAIN, PB_PLAIN, E_LEAKY_MASK>(this, CFG_AUTO, p, nz, tag);      // (a leaky net has two outputs: never rank-1)
  if (maskH) return run_gemm<PA_PLAIN, PB_PLAIN, E_MASK>(this, CFG_AUTO, p, nz, tag);
  return run_gemm<PA_PLAIN, PB_PLAIN, E_PLAIN>(this, CFG_AUTO, p, nz, tag);
}

// split-K factor for a weight gradient: enough workgroups to fill 256 CUs, chunk aligned
int Engine::wgrad_ksplit(int Mout, int Nout, int Krows, int nz) const {
  const int cfg = pick_cfg(Mout, Nout, Krows, nz);
  int TM, TN, TK;
  switch (cfg) {
    case CFG_SQ: TM = CfgSq::TM; TN = CfgSq::TN; TK = CfgSq::kTK; break;
    case CFG_WG: TM = CfgWg::TM; TN = CfgWg::TN; TK = CfgWg::kTK; break;
    case CFG_BIG: TM = CfgBig::TM; TN = CfgBig::TN; TK = CfgBig::kTK; break;
    case CFG_MID: TM = CfgMid::TM; TN = CfgMid::TN; TK = CfgMid::kTK; break;
    case CFG_SMALL: TM = CfgSmall::TM; TN = CfgSmall::TN; TK = CfgSmall::kTK; break;
    default: TM = CfgTall::TM; TN = CfgTall::TN; TK = CfgTall::kTK; break;
  }
  const int tiles = ((Mout + TM - 1) / TM) * ((Nout + TN - 1) / TN) * nz;
  const int kchunks = (Krows + TK - 1) / TK;
  int ks = (wgrad_wg_target + tiles - 1) / tiles;
  // many batched nets fill the CUs without split-K, but workgroups that all stream thousands of rows from the same offset of
  // equally strided matrices run 2x slower (measured at 256 nets x 7936 rows, fp32: 12.8 -> 5.4 ms): keep >= 4 k-ranges
  if (Krows >= 4096) ks = std::max(ks, wgrad_long_min);
  // 256-row wgrads of many nets: round 2 measured two k-ranges 1.5x faster than one -- with the item-major workgroup mapping, where the four
  // tiles of a net sat on four XCDs.  With the z-major mapping (gemm_kernel.h) one range wins: EDAC 15.4k -> 16.9k steps/s, IQL +2.5 %,
  // TD3+BC +2.5 % at 128 runs (Adam reads half the slabs).  ORL_WGRAD_SMALL_KS=2 restores the old rule for A/B runs.
  if (cfg == CFG_SQ && Krows < 1024 && kchunks >= 8) ks = std::max(ks, wgrad_small_ks);
  ks = std::max(1, std::min(ks, std::min(32, kchunks)));
  while (ks > 1 && (kchunks + ks - 1) / ks < 2) --ks;
  return ks;
}

// Output-stationary wgrad, one split-K slab per workgroup from slab 0 (*slabs).  dy.rank1: the top hidden layer -- dz^T from the packed ReLU mask,
// G = dq (.) X; the tail layer's gradients ride along, from the activation streamed through registers or, if the forward did not store it, derived
// from the accumulators.  Else dy.m = a materialised dZ; recompute_X0 != null: X is rebuilt from the net's input rows.  Returns as ws_dgrad.
int Engine::ws_wgrad(const DY& dy, const Mat& X, int M, const NetRef& nr, int layer, const Mat* recompute_X0, const char* tag, int* slabs) {
  const NetLayout& l = *nr.lay;
  const int in = l.layer_in(layer), out = l.layer_out(layer), nz = R * nr.nz1;
  const bool derived = dy.rank1 && vals_dead.count(dy.m.p) > 0;
  float* g = grads + nr.g_off;
  WsWgradP w;
  memset(&w, 0, sizeof(w));
  w.H0 = X.z(); w.h0_pitch = X.pitch;
  w.dW = g + l.w_off[layer]; w.db = g + l.b_off[layer];
  w.o_rs = (long)max_slab * P_train; w.o_msw = l.w_ms[layer]; w.o_msb = l.b_ms[layer]; w.o_ks = P_train;
  if (dy.rank1) {
    w.abits = dy.m.zbits(); w.ab_g = dy.m.bg;
    w.dq = dy.rowv.z(); w.dq_sm = dy.rowv.pitch;
    w.wt = nr.w(l.L);
    if (derived) { w.W1 = nr.w(layer); w.b1 = nr.b(layer); }
    else { w.H1 = dy.m.z(); w.h1_pitch = dy.m.pitch; }
    w.dwt = g + l.w_off[l.L]; w.dbt = g + l.b_off[l.L]; w.o_mswt = l.w_ms[l.L]; w.o_msbt = l.b_ms[l.L];
    w.np3 = p3(4) && derived;                                        // precision 2: three planes of G = dq (.) h0 (ws_wgrad_kernel<5>)
    w.lab_clk = lab_clk(72);
  } else {
    w.dZ = dy.m.z(); w.dz_pitch = dy.m.pitch;
    if (recompute_X0) {                            // h0 = relu(X0 W0^T + b0) is rebuilt inside the launch
      w.X0 = recompute_X0->z(); w.x0_pitch = recompute_X0->pitch; w.in0 = l.layer_in(0);
      w.W0 = nr.w(0); w.w0_sn = l.layer_in(0); w.w0_sk = 1;
      w.b0 = nr.b(0);
    }
  }
  w.M = M; w.nz1 = nr.nz1; w.f32 = ws_f32(); w.gscale = cur_gscale;
  if (!ws_wgrad_supported(w, out, in)) return 1;
  const bool w3 = !dy.rank1 && p3(4) && ws_wgrad3p_supported(w, out, in);      // precision 2: three planes of dZ and of H0, two workgroups (halves of the output rows) per slab
  // one round (prologue 1 << 20): the slab write + derived tail gradients per workgroup cost more than idle CUs (4 slabs at 192 nets: 540 us
  // either way, and Adam then reads 4 slabs)
  const int per_z = ws_dgrad_blocks(M, w3 ? 2 * nz : nz, dy.rank1 ? ws_wgrad_slab_cap : max_slab, ws_geo, 1 << 20);
  const double flops = 2.0 * M * (double)in * (dy.rank1 ? out + 2 : out + 1 + (recompute_X0 ? w.in0 + 1 : 0)) * nz;
  const double bytes = dy.rank1 ? nz * ((derived ? M * (double)out / 8 : 4.0 * M * (double)out) + 4.0 * M * (in + 1) + 4.0 * per_z * out * (in + 2))
                                : nz * (4.0 * M * (double)((recompute_X0 ? w.x0_pitch : in) + out) + 4.0 * per_z * out * (in + 1));
  if (timed("ws_wgrad", tag, w3 || w.np3, flops, bytes, [&] { return w3 ? launch_ws_wgrad3p(w, nz, per_z, stream) : launch_ws_wgrad(w, nz, per_z, stream); })) return -1;
  *slabs = per_z;
  return 0;
}

// slabs_out: number of split-K slabs actually written (== ksplit unless the weight-stationary kernel chose its own decomposition)
int Engine::linear_wgrad(const DY& dy, const Mat& X, int M, const NetRef& nr, int layer, int ksplit, int slab0, bool with_bias,
                         const char* tag, int in_row0, int in_rows, bool* fuse_tail, int* slabs_out, const float* x_dscale, const Mat* recompute_X0) {
  const NetLayout& l = *nr.lay;
  const int in = l.layer_in(layer), out = l.layer_out(layer);
  if (in_rows < 0) in_rows = in;
  if (slab0 + ksplit > max_slab) return fail("wgrad: slab budget exceeded");
  const bool x_dead = vals_dead.count(X.p) > 0;
  if (x_dead && !(recompute_X0 && layer == 1)) return fail(std::string("wgrad ") + tag + ": the input activation was not stored by the forward pass");
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.a_dscale = cur_gscale; p.b_dscale = x_dscale;      // split precision: A = dY^T of the current backward pass; B = X (an activation, or a gradient-like matrix with its own scale)
  if (mm_prec() == P_SPLIT3) { p.a_scale = ORL_GSCALE3; if (x_dscale) p.b_scale = ORL_GSCALE3; }
  p.A = dy.m.z();
  p.a_sr = 1; p.a_sk = dy.m.pitch;
  if (out == 1 && dy.m.pitch == 1 && !dy.rank1) p.a_sr = 4;   // a [1 x M] row vector: k-contiguous, any row stride -> vector loads
  if (dy.rank1) {
    p.a_trans = 1;
    p.rowv = dy.rowv.z();
    p.colv = nr.w(l.L);
  }
  p.B = X.z();
  p.b_sr = 1; p.b_sk = X.pitch;
  p.a_rlim = dy.m.pitch & ~3; p.b_rlim = X.pitch & ~3;
  p.ones_row = 1 << 30;
  p.M = out; p.N = in_rows; p.K = M;
  p.nz1 = nr.nz1; p.ksplit = ksplit;
  const long g_rs = (long)max_slab * P_train;
  float* g = grads + nr.g_off + (long)slab0 * P_train;
  if (l.ens) { p.C = g + l.w_off[layer] + (long)in_row0 * out; p.c_sr = 1; p.c_sn = out; }
  else { p.C = g + l.w_off[layer] + in_row0; p.c_sr = in; p.c_sn = 1; }
  p.c_s0 = g_rs; p.c_s1 = l.w_ms[layer]; p.c_ks = P_train;
  if (with_bias) { p.bias_out = g + l.b_off[layer]; p.bo_s0 = g_rs; p.bo_s1 = l.b_ms[layer]; p.bo_ks = P_train; }
  const int nz = R * nr.nz1;
  if (slabs_out) *slabs_out = ksplit;
  // output-stationary kernel (csrc/ws_gemm.h): dz^T from the packed ReLU mask, G = dq (.) X and the activation itself streamed once;
  // the tail layer's gradients ride along (*fuse_tail = true, same slabs)
  if (slabs_out && fuse_tail && dy.rank1 && with_bias && slab0 == 0 && ws_precision_ok() && !force_scalar && !l.ens &&
      dy.m.bits && bits_live.count(dy.m.bits) && out == dy.m.pitch && in_row0 == 0 && in_rows == in && X.pitch == in &&
      ws_wgrad_rows_ok(M, nz)) {
    const int rc = ws_wgrad(dy, X, M, nr, layer, nullptr, tag, slabs_out);
    if (rc == 0) *fuse_tail = true;
    if (rc <= 0) return rc;
  }
  // the same output-stationary kernel for a hidden layer BELOW the top one of a many-row batch: dZ is a materialised matrix (three products
  // per block instead of the rank-1 form's two, no mask / w_tail); one slab per workgroup
  if (slabs_out && !dy.rank1 && !leaky && with_bias && slab0 == 0 && ws_precision_ok() && !force_scalar && !l.ens && !x_dscale && in_row0 == 0 &&
      in_rows == in && X.pitch == in && dy.m.pitch == out && ws_wgrad_rows_ok(M, nz)) {
    const int rc = ws_wgrad(dy, X, M, nr, layer, x_dead ? recompute_X0 : nullptr, tag, slabs_out);
    if (rc <= 0) return rc;
  }
  if (x_dead) return fail(std::string("wgrad ") + tag + ": the input activation was not stored and the recomputing kernel does not serve this shape");
  if (dy.rank1 && vals_dead.count(dy.m.p)) return fail(std::string("wgrad ") + tag + ": the activation values were not stored by the forward pass");
  if (fuse_tail) {
    // the rank-1 kernel streams h and dq anyway: let it also emit the tail layer's dw / db (same split-K slabs)
    *fuse_tail = dy.rank1 && rank1_wgrad_is_fast(p, force_scalar);
    if (*fuse_tail) {
      p.tail_w_out = g + l.w_off[l.L]; p.tail_b_out = g + l.b_off[l.L];
      p.tw_s0 = g_rs; p.tw_s1 = l.w_ms[l.L]; p.tb_s1 = l.b_ms[l.L];
    }
  }
  if (dy.rank1) return run_gemm<PA_RANK1, PB_PLAIN, E_WGRAD>(this, CFG_AUTO, p, nz, tag);
  return run_gemm<PA_PLAIN, PB_PLAIN, E_WGRAD>(this, CFG_AUTO, p, nz, tag);
}

int Engine::adam(int net, int nnets, int lr_slot, const std::vector<std::pair<long, int>>& segs, int target_net, unsigned long long t_div) {
  AdamP a;
  memset(&a, 0, sizeof(a));
  const NetLayout& l = lay[net];
  a.params = net_ptr(0, net); a.p_s0 = P_train; a.p_s1 = l.stride();
  a.m = adam_m + net_off[net]; a.v = adam_v + net_off[net];
  a.g = grads + net_off[net]; a.g_s0 = (long)max_slab * P_train; a.g_s1 = l.stride(); a.g_ks = P_train;
  a.nseg = (int)segs.size();
  if (a.nseg > 12) return fail("too many adam segments");
  for (int i = 0; i < nnets && net + i < ORL_NUM_NETS; ++i) last_segs[net + i] = segs;
  for (int i = 0; i < a.nseg; ++i) { a.seg_end[i] = segs[i].first; a.seg_nslab[i] = segs[i].second; }
  if (target_net >= 0) { a.target = net_ptr(0, target_net); a.t_s0 = P_tgt; a.t_s1 = l.stride(); }
  a.P = l.size; a.lr_slot = lr_slot; a.hy = hyper;
  a.b1 = cfg.adam_beta1; a.b2 = cfg.adam_beta2; a.eps = cfg.adam_eps; a.tau = cfg.tau;
  a.gstep = gstep; a.t_div = t_div; a.health = health;
  // algorithmic bytes: every gradient slab read once, m / v / parameter read and written, the Polyak target read and written
  double bytes = 0.0;
  for (int i = 0; i < a.nseg; ++i) bytes += (double)(a.seg_end[i] - (i ? a.seg_end[i - 1] : 0)) * (4.0 * a.seg_nslab[i] + 24.0 + (a.target ? 8.0 : 0.0));
  prof_begin("adam", 0, bytes * nnets * R);
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((l.size + 1023) / 1024), nnets, R), dim3(256), 0, stream, a);    // four parameters per thread
  prof_end();
  if (hipGetLastError() != hipSuccess) return fail("adam: launch failed");
  return 0;
}

int Engine::polyak(int target_net, int src_net, int nnets) {
  const long P = lay[src_net].size, PS = lay[src_net].stride();
  prof_begin("polyak", 0, 12.0 * P * nnets * R);
  hipLaunchKernelGGL(k_polyak, dim3((unsigned)((P + 255) / 256), nnets, R), dim3(256), 0, stream, net_ptr(0, target_net), P_tgt, PS,
                     (const float*)net_ptr(0, src_net), P_train, PS, P, cfg.tau);
  prof_end();
  if (hipGetLastError() != hipSuccess) return fail("polyak: launch failed");
  return 0;
}

int Engine::assemble(const Mat& obs, const Mat* act, const Mat& X, int row0, int rows, int rep) {
  AssembleP a;
  memset(&a, 0, sizeof(a));
  a.obs = obs.p; a.obs_rs = obs.rs; a.OP = obs.pitch; a.od = od;
  if (act) { a.act = act->p; a.act_rs = act->rs; a.apitch = act->pitch; }
  a.ad = ad;
  a.X = X.p; a.x_rs = X.rs; a.XP = X.pitch; a.row0 = row0; a.rows = rows; a.rep = rep;
  ORL_LAUNCH("assemble", k_assemble, dim3((rows + 255) / 256, R), dim3(256), a);
  return 0;
}

// the whole [in0 -> 256 -> 256 -> out] pass of few batched rows as one launch (small_fwd.h); H0 / H1 null: the hidden activations are not stored.
// The caller adds the sampling jobs or the QG mode's gradient output.
SmallFwdP Engine::small_fwd_p(const Mat& X, int M, const NetRef& nr, const Mat* H0, const Mat* H1, const Mat& out) const {
  const NetLayout& l = *nr.lay;
  SmallFwdP w;
  memset(&w, 0, sizeof(w));
  w.X = X.z(); w.x_pitch = X.pitch; w.in0 = l.layer_in(0);
  w.W0 = nr.w(0); w.b0 = nr.b(0);
  w.W1 = nr.w(1); w.b1 = nr.b(1);
  w.Wt = nr.w(2); w.bt = nr.b(2);
  if (H0) w.H0 = H0->zo();
  if (H1) w.H1 = H1->zo();
  w.OUT = out.zo(); w.o_pitch = out.pitch; w.out_dim = l.out_dim;
  w.M = M; w.nz1 = nr.nz1; w.f32 = ws_f32();
  return w;
}

int Engine::mlp_forward(const Mat& X, int M, const NetRef& nr, std::vector<Mat>& hs, const Mat& out, const char* tag,
                        const SampleJob* jobs, int njobs, bool* jobs_done) {
  const NetLayout& l = *nr.lay;
  const int Ln = l.L;
  std::string t = tag;
  if (jobs_done) *jobs_done = false;
  // few batched rows (one to a few runs per engine): the whole pass as ONE launch (small_fwd.h) instead of layer 0 + layer 1 + tail
  if (small_fwd_on && !leaky && Ln == 2 && !l.ens && !no_ws && !force_scalar && l.H[0] == SF_N && l.H[1] == SF_N && hs[0].pitch == SF_N && hs[1].pitch == SF_N &&
      (long)M * R * nr.nz1 <= small_fwd_max_rows) {
    SmallFwdP w = small_fwd_p(X, M, nr, fwd_only ? nullptr : &hs[0], fwd_only ? nullptr : &hs[1], out);
    if (fuse_small && jobs && jobs_done && njobs >= 1 && njobs <= 3 && nr.nz1 == 1 && l.out_dim == 2 * ad && ad <= 8 && out.pitch == l.out_dim) {
      w.njobs = njobs; w.A = ad;
      for (int i = 0; i < njobs; ++i) w.job[i] = jobs[i];
      if (!small_fwd_supported(w)) w.njobs = 0;      // (e.g. more than 16 repeated actions per row: the pass stays one launch, the sampling its own)
    }
    if (small_fwd_supported(w)) {
      const int nz = R * nr.nz1;
      watch_range(X, M, w.in0, X.cs ? nr.nz1 : 1, tag);
      if (!fwd_only) watch_range(hs[0], M, SF_N, nr.nz1, tag);      // (h1 meets the tail weights in fp32 vector arithmetic)
      if (lab_slot < 4) w.lab_clk = lab_clk(16 + 12 * lab_slot++);
      if (timed("small_fwd", tag, false, 2.0 * M * (double)nz * (SF_N * (double)(w.in0 + 1) + (double)SF_N * SF_N + (double)SF_N * l.out_dim),
                4.0 * nz * (M * (double)(X.pitch + (fwd_only ? 0 : 2 * SF_N) + l.out_dim) + (double)SF_N * (w.in0 + SF_N + l.out_dim + 2)),
                [&] { return launch_small_fwd(w, nz, stream); })) return -1;
      if (w.njobs) *jobs_done = true;
      for (int i = 0; i < 2; ++i) {
        if (hs[i].bits) bits_live.erase(hs[i].bits);      // no packed masks from this path: the backward reads 1[h > 0] from the values
        if (fwd_only) vals_dead.insert(hs[i].p); else vals_dead.erase(hs[i].p);
      }
      return 0;
    }
  }
  bool tail_done = false;
  for (int i = 0; i < Ln; ++i) {
    if (i == 0 && Ln >= 2) continue;         // layer 0 is issued together with layer 1 (fused into it when the ws kernel applies)
    if (linear_fwd(i == 0 ? X : hs[i - 1], M, nr, i, hs[i], leaky ? E_BIAS_LEAKY : E_BIAS_RELU, nullptr, (t + ".fwd" + std::to_string(i)).c_str(), 0, -1,
                   i == Ln - 1 ? &out : nullptr, i == Ln - 1 ? &tail_done : nullptr, i == 1 ? &X : nullptr, (t + ".fwd0").c_str())) return -1;
  }
  if (tail_done) return 0;                 // single-output tail folded into the last hidden layer's epilogue
  return linear_fwd(hs[Ln - 1], M, nr, Ln, out, E_BIAS, nullptr, (t + ".tail").c_str());
}

int Engine::mlp_qgrad(const Mat& X, int M, const NetRef& nr, const Mat& q, const Mat& G, int gc0, int gn, const char* tag, bool* done) {
  const NetLayout& l = *nr.lay;
  *done = false;
  if (!(fuse_small && small_fwd_on && l.L == 2 && !l.ens && !no_ws && !force_scalar && l.H[0] == SF_N && l.H[1] == SF_N && l.out_dim == 1 &&
        (long)M * R * nr.nz1 <= small_fwd_max_rows)) return 0;
  SmallFwdP w = small_fwd_p(X, M, nr, nullptr, nullptr, q);
  w.G = G.zo(); w.g_pitch = G.pitch; w.gc0 = gc0; w.gn = gn;
  if (!small_fwd_supported(w)) return 0;
  const int nz = R * nr.nz1;
  watch_range(X, M, w.in0, X.cs ? nr.nz1 : 1, tag);
  // forward (layer 0, layer 1, tail) + the unit-seed backward through layer 1 and the gn input columns of layer 0
  if (lab_slot < 4) w.lab_clk = lab_clk(16 + 12 * lab_slot++);
  if (timed("small_qgrad", tag, false, 2.0 * M * (double)nz * (SF_N * (double)(w.in0 + 1) + 2.0 * SF_N * SF_N + SF_N + (double)SF_N * gn),
            4.0 * nz * (M * (double)(X.pitch + 1 + gn) + 2.0 * SF_N * SF_N + (double)SF_N * (w.in0 + 3)), [&] { return launch_small_fwd(w, nz, stream); })) return -1;
  *done = true;
  return 0;
}

int Engine::mlp_forward_only(const Mat& X, int M, const NetRef& nr, std::vector<Mat>& hs, const Mat& out, const char* tag,
                             const SampleJob* jobs, int njobs, bool* jobs_done) {
  struct Scope { Engine* e; ~Scope() { e->fwd_only = false; } } scope{this};
  fwd_only = true;
  return mlp_forward(X, M, nr, hs, out, tag, jobs, njobs, jobs_done);
}

int Engine::scale_inplace(const Mat& m, int rows, int cols, int nets, float s, const Mat* mask, const char* tag) {
  ORL_LAUNCH(tag, k_dropout, dim3((unsigned)(((long)rows * cols + 255) / 256), nets, R), dim3(256), m.p, m.rs, m.cs, m.pitch,
             (const float*)(mask ? mask->p : nullptr), mask ? mask->rs : 0L, rows, cols, s);
  return 0;
}

int Engine::mlp_forward_dropout(const Mat& X, int M, const NetRef& nr, std::vector<Mat>& hs, const Mat& out, const char* tag, float p,
                                const std::vector<Mat>& masks) {
  const NetLayout& l = *nr.lay;
  const std::string t = tag;
  const float inv_keep = 1.0f / (1.0f - p);
  struct Scope { Engine* e; ~Scope() { e->no_ws = false; } } scope{this};
  no_ws = true;                                            // one launch per layer: the dropout sits between them
  for (int i = 0; i < l.L; ++i) {
    if (linear_fwd(i == 0 ? X : hs[i - 1], M, nr, i, hs[i], E_BIAS_RELU, nullptr, (t + ".fwd" + std::to_string(i)).c_str())) return -1;
    if (scale_inplace(hs[i], M, l.layer_out(i), nr.nz1, inv_keep, &masks[i], (t + ".dropout" + std::to_string(i)).c_str())) return -1;
    if (hs[i].bits) bits_live.erase(hs[i].bits);           // the packed ReLU mask predates the dropout: the backward reads 1[h > 0] from the values
  }
  return linear_fwd(hs[l.L - 1], M, nr, l.L, out, E_BIAS, nullptr, (t + ".tail").c_str());
}

// Adam segment table: one (end offset, slab count) pair per weight tensor and per bias tensor
static std::vector<std::pair<long, int>> make_segs(const NetLayout& l, const std::vector<int>& ksW, const std::vector<int>& ksB) {
  std::vector<std::pair<long, int>> s;
  for (int i = 0; i <= l.L; ++i) {
    s.push_back({l.b_off[i], ksW[i]});   // weights of layer i end where its bias starts
    const long bend = l.b_off[i] + (l.ens ? (long)l.members * l.layer_out(i) : l.layer_out(i));
    s.push_back({bend, ksB[i]});
  }
  if (l.extra_off >= 0) s.push_back({l.size, 1});
  return s;
}

// generic backward through an MLP family.  dTail: [M x out_dim] gradient w.r.t. the tail output.
// dxin (optional): also the gradient w.r.t. the input columns [col0, col0 + ncols), written to *dX.
struct BwdOut { std::vector<int> ks; };
struct InputGrad { int col0, ncols; const Mat* dX; };
static int mlp_backward(Engine* e, const NetRef& nr, const Mat& X, const std::vector<Mat>& hs, int M, const Mat& dTail,
                        std::vector<Mat>& dz, bool want_w, const InputGrad* dxin, const char* tag, BwdOut* out,
                        const float* gscale_given = nullptr) {
  const bool want_dx = dxin != nullptr;
  const NetLayout& l = *nr.lay;
  const int L = l.L;
  const bool rank1 = (l.out_dim == 1);
  const int nz = e->R * nr.nz1;
  std::vector<int> ks(L + 1, 1);
  std::string t = tag;
  // split precision: every gradient matrix of this pass enters the MFMAs times one dynamic power-of-two scale per run, chosen from the seed
  struct ScaleScope { Engine* e; const float* prev; ~ScaleScope() { e->cur_gscale = prev; } } scope{e, e->cur_gscale};
  e->cur_gscale = gscale_given ? gscale_given : e->grad_scale(dTail, M, l.out_dim, nr.nz1, tag);
  if (e->split_scales() && !e->cur_gscale) return -1;
  if (want_w) {
    for (int i = 0; i <= L; ++i) ks[i] = e->wgrad_ksplit(l.layer_out(i), l.layer_in(i), M, nz);
    if (!rank1 && e->linear_wgrad(DY::plain(dTail), hs[L - 1], M, nr, L, ks[L], 0, true, (t + ".wgrad_tail").c_str())) return -1;
  }
  DY cur;
  bool w0_done = false;
  if (rank1) cur = DY::virt(hs[L - 1], dTail);
  else {
    if (e->linear_dgrad(DY::plain(dTail), M, nr, L, 0, l.layer_in(L), &hs[L - 1], dz[L - 1], (t + ".dgrad_tail").c_str())) return -1;
    if (e->bwd_scale != 1.0f && e->scale_inplace(dz[L - 1], M, l.layer_out(L - 1), nr.nz1, e->bwd_scale, nullptr, (t + ".dropout_bwd").c_str())) return -1;
    cur = DY::plain(dz[L - 1]);
  }
  for (int i = L - 1; i >= 0; --i) {
    const Mat& xin = (i == 0) ? X : hs[i - 1];
    if (want_w && !(i == 0 && w0_done)) {
      bool fused = false;
      const bool top = rank1 && (i == L - 1);
      int slabs = ks[i];
      if (e->linear_wgrad(cur, xin, M, nr, i, ks[i], 0, true, (t + ".wgrad" + std::to_string(i)).c_str(), 0, -1, top ? &fused : nullptr, &slabs, nullptr,
                          i == 1 ? &X : nullptr)) return -1;
      ks[i] = slabs;
      if (top) {
        if (fused) ks[L] = ks[i];           // the tail gradients were written into the same split-K slabs
        else if (e->linear_wgrad(DY::plain(dTail), hs[L - 1], M, nr, L, ks[L], 0, true, (t + ".wgrad_tail").c_str())) return -1;
      }
    }
    if (i > 0) {
      // the dgrad that produces dz0 can also produce dW0 / db0 (and then dz0 is only stored when dX is wanted)
      int w0_slabs = 0;
      if (e->linear_dgrad(cur, M, nr, i, 0, l.layer_in(i), &hs[i - 1], dz[i - 1], (t + ".dgrad" + std::to_string(i)).c_str(),
                          (want_w && i == 1) ? &X : nullptr, want_dx, &w0_slabs)) return -1;
      if (w0_slabs > 0) { w0_done = true; ks[0] = w0_slabs; }
      if (e->bwd_scale != 1.0f && e->scale_inplace(dz[i - 1], M, l.layer_out(i - 1), nr.nz1, e->bwd_scale, nullptr, (t + ".dropout_bwd").c_str())) return -1;
      cur = DY::plain(dz[i - 1]);
    } else if (want_dx) {
      if (e->linear_dgrad(cur, M, nr, 0, dxin->col0, dxin->ncols, nullptr, *dxin->dX, (t + ".dgrad_x").c_str())) return -1;
    }
  }
  if (out) out->ks = ks;
  return 0;
}

int Engine::train_net(const NetRef& nr, int net, int members, int opt, const Mat& X, const std::vector<Mat>& hs, int M, const Mat& seed,
                      std::vector<Mat>& dhs, const char* tag, const float* gs, int target_net, unsigned long long t_div) {
  BwdOut b;
  if (mlp_backward(this, nr, X, hs, M, seed, dhs, true, nullptr, tag, &b, gs)) return -1;
  return adam(net, members, opt, make_segs(*nr.lay, b.ks, b.ks), target_net, t_div);
}

// tanh-Gaussian sampling launch (up to 3 jobs)
static int launch_sample(Engine* e, const Mat& head, int A, const SampleJob* jobs, int njobs) {
  SampleP sp;
  memset(&sp, 0, sizeof(sp));
  sp.head = head.p; sp.head_rs = head.rs; sp.A = A;
  int maxrows = 0;
  for (int i = 0; i < njobs; ++i) { sp.job[i] = jobs[i]; maxrows = std::max(maxrows, jobs[i].rows); }
  e->prof_begin("tanh_sample", 0);
  const int AG = A <= 8 ? 8 : (A <= 16 ? 16 : 32);      // lanes per output row (k_tanh_sample)
  hipLaunchKernelGGL(k_tanh_sample, dim3((unsigned)(((long)maxrows * AG + 255) / 256), njobs, e->R), dim3(256), 0, e->stream, sp);
  e->prof_end();
  return hipGetLastError() == hipSuccess ? 0 : fail("tanh_sample launch");
}
static SampleJob make_job(int head_row0, int rows, int rep, const Mat& eps, const Mat& dst, int dst_col, int dst_row0, const Mat& logp) {
  SampleJob j;
  memset(&j, 0, sizeof(j));
  j.head_row0 = head_row0; j.rows = rows; j.rep = rep; j.eps = eps.p; j.eps_rs = eps.rs;
  j.dst = dst.p; j.dst_rs = dst.rs; j.dst_pitch = dst.pitch; j.dst_col = dst_col; j.dst_row0 = dst_row0;
  j.logp = logp.p; j.logp_rs = logp.rs;
  return j;
}

}  // namespace orl

#include "algo_cql.inc"
#include "algo_iql.inc"
#include "algo_td3bc.inc"
#include "algo_edac.inc"
#include "algo_sac.inc"
#include "algo_mcq.inc"
#include "algo_mobile.inc"
#include "algo_rcsl.inc"
#include "algo_rcsl_gauss.inc"
#include "algo_autoreg.inc"
#include "algo_rambo.inc"

namespace orl {

// ---------------------------------------------------------------------------------------------
// init / step driver
// ---------------------------------------------------------------------------------------------
int Engine::build_common() {
  // batch slots: obs and next_obs adjacent so [obs; next_obs] is one 2B-row matrix
  alloc("b_obs2", 2 * B, OP);
  alloc("b_act", B, AP); alloc("b_rew", B, 1); alloc("b_term", B, 1);
  alloc("ones", std::max(B, 16), 1);
  d_idx = (long long*)raw_alloc(sizeof(long long) * (size_t)R * B);
  if (!d_idx) return fail("hipMalloc minibatch indices");
  taps["b_obs"] = {W("b_obs2"), B, od};
  taps["b_nobs"] = {W("b_obs2").rows(B), B, od};
  taps["b_act"] = {W("b_act"), B, ad};
  taps["b_rew"] = {W("b_rew"), B, 1};
  taps["b_term"] = {W("b_term"), B, 1};
  // column-tile partial sums of fused single-output tails (linear_fwd): up to 3 extra parts of the longest row batch
  tq_scratch_nets = std::max(2, K);
  alloc("tq_scratch", 3L * (B + 3L * B * N), 1, tq_scratch_nets);
  if (cfg.algo == ORL_ALGO_CQL) {
    if (cfg.cql_cons_row0 < 0 || cfg.cql_cons_rows < 0 || cfg.cql_real_rows < 0 || cfg.cql_cons_row0 + cfg.cql_cons_rows > B || cfg.cql_real_rows > B)
      return fail("cql_cons_row0 / cql_cons_rows / cql_real_rows out of the batch");
  }
  return 0;
}

// every environment knob of the engine; they override the defaults of engine.h and the orl_config fields init() stored before
void Engine::read_env() {
  enum Kind { FLAG, NFLAG, POS_I, POS_L, ANY_I };      // != 0 / == 0 -> bool; a value > 0 -> int / long (anything else ignored); any int
  int cus = 0;
  const struct { const char* name; void* field; Kind kind; } knobs[] = {
      {"ORL_WS", &use_ws, FLAG},
      {"ORL_WS32", &use_ws32, FLAG},
      {"ORL_WS_KEEP_H1", &elide_top, NFLAG},
      {"ORL_WS_RECOMPUTE_H0", &recompute_h0, FLAG},
      {"ORL_WS_ONE_ROUND", &ws_geo.one_round, FLAG},
      {"ORL_WS_CUS", &cus, POS_I},
      {"ORL_WS_FWD_MIN", &ws_fwd_min_rows, POS_L},
      {"ORL_WS_BWD_MIN", &ws_bwd_min_rows, POS_L},
      {"ORL_WS_DGRAD_PLAIN_MIN", &ws_dgrad_plain_min_rows, POS_L},
      {"ORL_WS_WGRAD_MIN", &ws_wgrad_min_rows, POS_L},
      {"ORL_WS_WGRAD_MIN_M", &ws_wgrad_min_m, POS_I},
      {"ORL_WS_WGRAD_SLABS", &ws_wgrad_slab_cap, POS_I},
      {"ORL_SMALL_FWD", &small_fwd_on, FLAG},
      {"ORL_SMALL_FWD_MAX", &small_fwd_max_rows, POS_L},
      {"ORL_FUSE_SMALL", &fuse_small, FLAG},
      {"ORL_P3", &p3_mask, ANY_I},
      {"ORL_WGRAD_WG_TARGET", &wgrad_wg_target, POS_I},
      {"ORL_WGRAD_LONG_MIN", &wgrad_long_min, POS_I},
      {"ORL_WGRAD_SMALL_KS", &wgrad_small_ks, POS_I},
  };
  for (const auto& k : knobs) {
    const char* f = getenv(k.name);
    if (!f) continue;
    const long v = atol(f);
    switch (k.kind) {
      case FLAG: *(bool*)k.field = v != 0; break;
      case NFLAG: *(bool*)k.field = v == 0; break;
      case POS_I: if (v > 0) *(int*)k.field = (int)v; break;
      case POS_L: if (v > 0) *(long*)k.field = v; break;
      case ANY_I: *(int*)k.field = (int)v; break;
    }
  }
  ws_wgrad_slab_cap = std::min(ws_wgrad_slab_cap, max_slab);
  if (cus >= 8 && cus <= 256) ws_geo.cus = cus;
}

int Engine::init(const orl_config& c) {
  cfg = c;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device available: the update engine needs an MI355X (gfx950)");
  if (c.device < 0 || c.device >= ndev) return fail("bad device ordinal");
  dev = c.device;
  ORL_HIP(hipSetDevice(dev));
  if (c.precision < 0 || c.precision > 2) return fail("precision must be 0 (fp32 MFMA), 1 (split-precision MFMA: two fp16 planes) or 2 (three fp16 planes where a kernel has them, fp32 MFMA elsewhere)");
  if (c.actor_dropout != 0.f && (c.algo != ORL_ALGO_IQL || !(c.actor_dropout > 0.f && c.actor_dropout < 1.f)))
    return fail("actor_dropout: supported for IQL only (run_iql.py --dropout_rate), 0 < p < 1");
  if (build_layouts(c, lay, net_off, net_is_target, &P_train, &P_tgt)) return -1;
  ORL_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  // launch geometry of the weight-stationary kernels: config fields, overridden once (here) by the environment
  ws_geo.one_round = c.ws_one_round != 0;
  ws_geo.cus = (c.ws_cus >= 8 && c.ws_cus <= 256) ? c.ws_cus : 256;
  read_env();
  R = c.n_runs; B = c.batch_size; od = c.obs_dim; ad = c.act_dim;
  leaky = c.algo == ORL_ALGO_AUTOREG;
  N = c.num_repeat_actions > 0 ? c.num_repeat_actions : 1;
  // MOBILE: the longest row batch is the penalty pass's S * E * B rows; N sizes the tail scratch of build_common for it (9 B N >= 3 S E B)
  if (c.algo == ORL_ALGO_MOBILE) N = std::max(1, (std::max(c.mobile_num_samples, 1) * std::max(c.mobile_num_elites, 1) + 2) / 3);
  OP = rup(od, 4); AP = rup(ad, 4); XP = rup(od + ad, 4); L = c.n_hidden;
  K = (c.algo == ORL_ALGO_EDAC) ? c.num_critics : 2;
  const long arena_floats = (long)R * (P_train + P_tgt);
  if (c.external_arena) arena = c.external_arena;
  else { arena = raw_alloc(sizeof(float) * arena_floats); if (!arena) return fail("hipMalloc arena"); }
  adam_m = raw_alloc(sizeof(float) * R * P_train);
  adam_v = raw_alloc(sizeof(float) * R * P_train);
  grads = raw_alloc(sizeof(float) * (size_t)R * max_slab * P_train);
  scalars = (RunScalars*)raw_alloc(sizeof(RunScalars) * R);
  hyper = (Hyper*)raw_alloc(sizeof(Hyper));
  gstep = (unsigned long long*)raw_alloc(2 * sizeof(unsigned long long));
  gstep_pre = gstep ? gstep + 1 : nullptr;
  gscale_buf = raw_alloc(sizeof(float) * (size_t)GSCALE_SLOTS * R);
  gscale_inv_b = raw_alloc(sizeof(float) * (size_t)R);
  cql_ticket = (unsigned int*)raw_alloc(sizeof(unsigned int) * (size_t)R);
  aloss_part = raw_alloc(sizeof(float) * ((size_t)R * SB_MAXGROUPS * 2 + 192));
  health = (unsigned int*)raw_alloc(sizeof(unsigned int) * (size_t)R);
  health_host.assign(R, 0u);
  if (c.precision == 2) {
    ws_dump = raw_alloc(sizeof(float) * (size_t)WS_DUMP_SLOTS * WS_N);
    if (!ws_dump) return fail("hipMalloc scratch lines");
  }
  if (!adam_m || !adam_v || !grads || !scalars || !hyper || !gstep || !gscale_buf || !gscale_inv_b || !cql_ticket || !health || !aloss_part) return fail("hipMalloc state");
  {
    std::vector<float> inv(R, orl_pow2_scale(1.0f / (float)c.batch_size));
    ORL_HIP(hipMemcpyAsync(gscale_inv_b, inv.data(), sizeof(float) * R, hipMemcpyHostToDevice, stream));
    ORL_HIP(hipStreamSynchronize(stream));
  }
  memset(&hyper_host, 0, sizeof(hyper_host));
  hyper_host.lr[ORL_OPT_ACTOR] = c.actor_lr;
  hyper_host.lr[ORL_OPT_CRITIC] = c.critic_lr;
  hyper_host.lr[ORL_OPT_ALPHA] = c.alpha_lr;
  hyper_host.lr[ORL_OPT_CQL_ALPHA] = c.cql_alpha_lr;
  hyper_host.lr[ORL_OPT_CRITIC_V] = c.critic_v_lr;
  hyper_host.lr[ORL_OPT_VAE] = c.behavior_lr;
  ORL_HIP(hipMemcpyAsync(hyper, &hyper_host, sizeof(Hyper), hipMemcpyHostToDevice, stream));
  std::vector<RunScalars> sc(R);
  for (auto& s : sc) { memset(&s, 0, sizeof(s)); s.alpha = c.auto_alpha ? 1.0f : c.alpha; s.alpha_bwd = s.alpha; s.cons_scale = 1.f; }
  ORL_HIP(hipMemcpyAsync(scalars, sc.data(), sizeof(RunScalars) * R, hipMemcpyHostToDevice, stream));
  ORL_HIP(hipStreamSynchronize(stream));
  if (build_common()) return -1;
  int rc = -1;
  switch (c.algo) {
    case ORL_ALGO_CQL: rc = cql_build(); break;
    case ORL_ALGO_IQL: rc = iql_build(); break;
    case ORL_ALGO_TD3BC: rc = td3bc_build(); break;
    case ORL_ALGO_EDAC: rc = edac_build(); break;
    case ORL_ALGO_SAC: rc = sac_build(); break;
    case ORL_ALGO_MCQ: rc = mcq_build(); break;
    case ORL_ALGO_MOBILE: rc = mobile_build(); break;
    case ORL_ALGO_RCSL: rc = rcsl_build(); break;
    case ORL_ALGO_RCSL_GAUSS: rc = rcslg_build(); break;
    case ORL_ALGO_AUTOREG: rc = autoreg_build(); break;
  }
  if (rc) return rc;
  { Mat lc; lc.p = (float*)lab_clk(0); lc.pitch = 192; taps["lab_clk"] = {lc, 1, 192}; }      // shader-clock stamps of lab builds (small_bwd.hip)
  for (auto& ns : noise_slots) taps[ns.name] = {W(ns.name), ns.rows, ns.cols ? ns.cols : ad};      // the noise arrays of the last step
  nm = (int)metric_names.size();
  if (nm > ORL_MAX_METRICS) return fail("too many metrics");
  metrics_last = raw_alloc(sizeof(float) * R * nm);
  metrics_sum = raw_alloc(sizeof(float) * R * nm);
  {
    Mat ones = W("ones");
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((ones.rs * R + 255) / 256)), dim3(256), 0, stream, ones.p, ones.rs * R, 1.0f);
  }
  ORL_HIP(hipStreamSynchronize(stream));
  return 0;
}

int Engine::enqueue_sample() {
  if (is_epoch_algo(cfg.algo)) return 0;      // rcsl_step's / rcslg_step's / autoreg_step's own input launch gathers (k_rcsl_prepare, k_autoreg_prepare)
  if (!buf || !buf->obs) return fail("no replay buffer attached (orl_engine_attach_buffer)");
  GatherP g;
  memset(&g, 0, sizeof(g));
  g.src = *buf; g.n = buf->n;
  g.B = B; g.W = std::max(OP, AP);
  Mat o2 = W("b_obs2");
  g.b_obs = o2.p; g.b_nobs = o2.p + (long)B * OP; g.obs_rs = o2.rs; g.nobs_rs = o2.rs; g.d_op = OP;
  g.b_act = W("b_act").p; g.act_rs = W("b_act").rs; g.d_ap = AP;
  g.b_rew = W("b_rew").p; g.rew_rs = W("b_rew").rs; g.b_term = W("b_term").p; g.term_rs = W("b_term").rs;
  g.seed = cfg.seed; g.gstep = gstep;
  if (mbuf) { g.m = mbuf->model_src(); g.real_rows = mbuf_real_rows; }
  if (!mbufs.empty()) {      // per-run rings: the table carries the sources, m.obs only says that there is a model source
    g.m_tab = m_tab; g.m.obs = mbufs[0]->obs; g.real_rows = mbuf_real_rows;
  }
  ORL_LAUNCH("gather", k_gather, dim3((unsigned)(((long)B * g.W + 255) / 256), R), dim3(256), g);
  return 0;
}

int Engine::enqueue_noise() {
  uint32_t sid = 1;
  for (auto& s : noise_slots) {
    const long n = ws_len.at(s.name);
    ORL_LAUNCH("noise", k_noise, dim3((unsigned)((n / 4 + 256) / 256), R), dim3(256), W(s.name).p, n, s.kind,
               s.kind == 2 ? 1.0f - cfg.actor_dropout : cfg.act_low, cfg.act_high, cfg.seed, (const unsigned long long*)gstep, sid);
    ++sid;
  }
  return 0;
}

void Engine::add_prep(const Mat& dst, int row0, int col0, int rows, int width, int src, int rep, int mod, int ncopy, const Mat* buf,
                      unsigned stream_id, int need_sampling, int need_devnoise, int src_row0) {
  PrepSpec s;
  memset(&s, 0, sizeof(s));
  s.job.dst = dst.p; s.job.dst_rs = dst.rs; s.job.dst_pitch = dst.pitch; s.job.dst_row0 = row0; s.job.dst_col0 = col0;
  s.job.rows = rows; s.job.width = width; s.job.src = src; s.job.rep = rep; s.job.mod = mod; s.job.ncopy = ncopy;
  if (buf) { s.job.buf = buf->p; s.job.buf_rs = buf->rs; s.job.buf_pitch = buf->pitch; }
  s.job.stream_id = stream_id; s.job.src_row0 = src_row0;
  s.need_sampling = need_sampling; s.need_devnoise = need_devnoise;
  prep.push_back(s);
}

int Engine::enqueue_prepare(bool sampling, bool devnoise) {
  PrepP p;
  memset(&p, 0, sizeof(p));
  int blocks = 0;
  for (auto& s : prep) {
    if (s.need_sampling >= 0 && s.need_sampling != (int)sampling) continue;
    if (s.need_devnoise >= 0 && s.need_devnoise != (int)devnoise) continue;
    if (p.njobs >= 20) return fail("too many prepare jobs");
    PrepJob j = s.job;
    const long n_el = (long)j.rows * j.width;
    if (n_el > (1L << 30)) return fail("prepare job too large");
    // 16-byte units for gathers of >= 4 columns between 16-byte aligned rows (dataset / batch-slot rows are zero-padded to OP / AP)
    const bool gather = j.src == PS_OBS || j.src == PS_NOBS || j.src == PS_ACT;
    j.vec4 = gather && j.width >= 4 && (j.dst_col0 & 3) == 0 && (j.dst_pitch & 3) == 0 && (j.dst_rs & 3) == 0 && aligned16(j.dst) &&
             ((j.width + 3) & ~3) <= (j.src == PS_ACT ? AP : OP);
    j.units = (int)((j.src == PS_NORMAL || j.src == PS_UNIFORM) ? (n_el + 3) / 4 : (j.vec4 ? (long)j.rows * ((j.width + 3) / 4) : n_el));
    blocks += (j.units + 255) / 256;
    j.block_end = blocks;
    p.job[p.njobs++] = j;
  }
  if (p.njobs == 0) return tick_folded ? fail("prepare: no job to carry the step counter") : 0;
  p.blocks = blocks;
  if (sampling) {
    if (!buf || !buf->obs) return fail("no replay buffer attached (orl_engine_attach_buffer)");
    p.d_obs = buf->obs; p.d_nobs = buf->nobs; p.d_act = buf->act; p.d_rew = buf->rew; p.d_term = buf->term; p.n = buf->n;
    p.OP = buf->OP; p.AP = buf->AP;
    // the minibatch indices (np.random.randint(0, size, B), buffer.py:98) are drawn inside k_prepare by every consumer of a batch row
    // (same Philox counter -> same index) and recorded once in d_idx: no separate index-drawing node in front of the step
    p.idx = d_idx; p.idx_rs = B; p.draw = 1; p.idx_out = d_idx;
    if (mbuf) {
      p.m_obs = mbuf->obs; p.m_nobs = mbuf->nobs; p.m_act = mbuf->act; p.m_rew = mbuf->rew; p.m_term = mbuf->term;
      p.m_n = mbuf->d_n; p.real_rows = mbuf_real_rows;
    }
    if (!mbufs.empty()) {      // per-run rings: the table carries the sources, m_obs only says that there is a model source
      p.m_tab = m_tab; p.m_obs = mbufs[0]->obs; p.real_rows = mbuf_real_rows;
    }
  }
  Mat o2 = W("b_obs2");
  p.b_obs = o2.p; p.b_nobs = o2.p + (long)B * OP; p.bo_rs = o2.rs; p.b_op = OP;
  p.b_act = W("b_act").p; p.ba_rs = W("b_act").rs; p.b_ap = AP;
  p.b_rew = W("b_rew").p; p.b_term = W("b_term").p; p.br_rs = W("b_rew").rs;
  p.B = B; p.seed = cfg.seed; p.gstep = gstep; p.lo = cfg.act_low; p.hi = cfg.act_high;
  if (tick_folded) { p.gstep = gstep_pre; p.gstep_publish = gstep; }
  ORL_LAUNCH("prepare", k_prepare, dim3((unsigned)blocks, R), dim3(256), p);
  return 0;
}

int Engine::n_variants() const { return cfg.algo == ORL_ALGO_TD3BC ? 2 : 1; }
int Engine::step_variant() const {
  if (cfg.algo != ORL_ALGO_TD3BC) return 0;
  const int f = cfg.update_actor_freq > 0 ? cfg.update_actor_freq : 1;
  return (step_host % f == 0) ? 1 : 0;   // 1 = actor + target-sync step (td3bc.py:107)
}
int Engine::last_step_variant() const {
  if (cfg.algo != ORL_ALGO_TD3BC || step_host == 0) return 0;
  const int f = cfg.update_actor_freq > 0 ? cfg.update_actor_freq : 1;
  return ((step_host - 1) % f == 0) ? 1 : 0;
}

int Engine::enqueue_step(int variant) {
  int rc = -1;
  gscale_next = 0; cur_gscale = nullptr; lab_slot = 0;
  switch (cfg.algo) {
    case ORL_ALGO_CQL: rc = cql_step(); break;
    case ORL_ALGO_IQL: rc = iql_step(); break;
    case ORL_ALGO_TD3BC: rc = td3bc_step(variant == 1); break;
    case ORL_ALGO_EDAC: rc = edac_step(); break;
    case ORL_ALGO_SAC: rc = sac_step(); break;
    case ORL_ALGO_MCQ: rc = mcq_step(); break;
    case ORL_ALGO_MOBILE: rc = mobile_step(); break;
    case ORL_ALGO_RCSL: rc = rcsl_step(); break;
    case ORL_ALGO_RCSL_GAUSS: rc = rcslg_step(); break;
    case ORL_ALGO_AUTOREG: rc = autoreg_step(); break;
  }
  if (rc) return rc;
  gscale_count[variant == 1 ? 1 : 0] = gscale_next;      // (host bookkeeping of the "gscale" tap; a captured variant keeps its count)
  if (tick_folded) return 0;               // the step's own kernels advanced the counter
  hipLaunchKernelGGL(k_tick, dim3(1), dim3(1), 0, stream, gstep);
  return hipGetLastError() == hipSuccess ? 0 : fail("tick launch");
}

int Engine::run_steps(int slot0, long n_steps, bool with_inputs, float* metrics_mean, float* elapsed_ms) {
  const bool graphable = use_graph && !prof_on;
  if (graphable) {
    for (int v = 0; v < n_variants(); ++v) {
      if (graph_exec[slot0 + v]) continue;
      ORL_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
      const int rc = (with_inputs && enqueue_inputs()) || enqueue_step(v);
      const hipError_t ce = hipStreamEndCapture(stream, &graph[slot0 + v]);
      if (rc) return -1;
      if (ce != hipSuccess) return fail(std::string("graph capture: ") + hipGetErrorString(ce));
      ORL_HIP(hipGraphInstantiate(&graph_exec[slot0 + v], graph[slot0 + v], nullptr, nullptr, 0));
    }
  }
  LoopScope loop;
  if (loop_begin(loop, {})) return -1;
  for (long s = 0; s < n_steps; ++s) {
    const int v = step_variant();
    if (graphable) { ORL_HIP(hipGraphLaunch(graph_exec[slot0 + v], stream)); }
    else if ((with_inputs && enqueue_inputs()) || enqueue_step(v)) return -1;
    step_host++;
  }
  if (loop.end(0, "hipStreamSynchronize(stream)", elapsed_ms)) return -1;      // (the error text names the call that failed)
  return finish(metrics_sum, (float)n_steps, metrics_mean, n_steps);      // (a non-finite metric of ANY of the steps stays in its sum)
}

// Called after the stream has been synchronised.
int Engine::finish(const float* src, float divisor, float* metrics_out, long steps) {
  std::vector<float> m(R * nm);
  ORL_HIP(hipMemcpy(m.data(), src, sizeof(float) * m.size(), hipMemcpyDeviceToHost));
  if (metrics_out) {
    for (int r = 0; r < R; ++r)
      for (int k = 0; k < ORL_MAX_METRICS; ++k) metrics_out[r * ORL_MAX_METRICS + k] = k < nm ? m[r * nm + k] / divisor : 0.f;
  }
  unsigned int bad = 0;
  if (health_update(m.data(), steps, &bad)) return -1;
  return bad ? ORL_RC_UNHEALTHY : 0;
}

}  // namespace orl

// =================================================================================================
// C ABI
// =================================================================================================
using namespace orl;

struct orl_engine {
  Engine e;
};
extern "C" {

const char* orl_last_error(void) { return g_err.c_str(); }
#ifdef ORL_SPLIT_BF16
const char* orl_version(void) { return "orl-engine 0.5 (gfx950; fp32 MFMA + split-bf16 MFMA; CQL IQL TD3BC EDAC SAC(MOPO) COMBO MCQ MOBILE RCSL RCSL_GAUSS AUTOREG)"; }
#else
const char* orl_version(void) { return "orl-engine 0.5 (gfx950; fp32 MFMA + split-fp16 MFMA; CQL IQL TD3BC EDAC SAC(MOPO) COMBO MCQ MOBILE RCSL RCSL_GAUSS AUTOREG)"; }
#endif
int orl_split_bits(void) { return ORL_SPLIT_BITS; }

void orl_config_default(orl_config* c, int32_t algo) {
  memset(c, 0, sizeof(*c));
  c->algo = algo;
  c->obs_dim = 17; c->act_dim = 6;
  c->n_hidden = 2; c->hidden[0] = c->hidden[1] = 256;
  c->batch_size = 256; c->n_runs = 1; c->device = 0; c->precision = 0; c->seed = 0;
  c->gamma = 0.99f; c->tau = 0.005f;
  c->adam_beta1 = 0.9f; c->adam_beta2 = 0.999f; c->adam_eps = 1e-8f;
  c->auto_alpha = 1; c->alpha = 0.2f; c->target_entropy = -6.0f; c->alpha_lr = 1e-4f;
  c->actor_lr = 1e-4f; c->critic_lr = 3e-4f;
  c->cql_weight = 5.0f; c->temperature = 1.0f; c->max_q_backup = 0; c->deterministic_backup = 1; c->with_lagrange = 0;
  c->lagrange_threshold = 10.0f; c->cql_alpha_lr = 3e-4f; c->num_repeat_actions = 10; c->act_low = -1.0f; c->act_high = 1.0f;
  c->expectile = 0.7f; c->iql_temperature = 3.0f; c->critic_v_lr = 3e-4f;
  c->policy_noise = 0.2f; c->noise_clip = 0.5f; c->td3bc_alpha = 2.5f; c->max_action = 1.0f; c->update_actor_freq = 2;
  c->num_critics = 10; c->eta = 1.0f;
  if (algo == ORL_ALGO_IQL || algo == ORL_ALGO_TD3BC) { c->actor_lr = 3e-4f; }
  if (algo == ORL_ALGO_EDAC) { c->n_hidden = 3; c->hidden[2] = 256; c->deterministic_backup = 0; }
  if (algo == ORL_ALGO_SAC) { c->actor_lr = 1e-4f; c->critic_lr = 3e-4f; c->deterministic_backup = 0; }   /* run_mopo.py:33-34 */
  c->vae_hidden = 750; c->vae_latent = 2 * c->act_dim; c->mcq_lambda = 0.9f; c->behavior_lr = 1e-3f;   /* run_mcq.py:34-36, 93-99 */
  c->mobile_num_samples = 10; c->mobile_num_elites = 5; c->mobile_real_rows = 12; c->penalty_coef = 1.5f;   /* run_mobile.py:45-52: int(256 * 0.05) real rows */
  if (algo == ORL_ALGO_MOBILE) { c->deterministic_backup = 1; }                                             /* run_mobile.py:157 */
  if (algo == ORL_ALGO_RCSL) { c->n_hidden = 4; for (int i = 0; i < 4; ++i) c->hidden[i] = 200; c->actor_lr = 1e-3f; }   /* run_rcsl.py:125-127 */
  if (algo == ORL_ALGO_AUTOREG) { c->n_hidden = 4; for (int i = 0; i < 4; ++i) c->hidden[i] = 200; c->actor_lr = 1e-3f; }   /* run_regress.py */
  if (algo == ORL_ALGO_RCSL_GAUSS) { c->n_hidden = 4; for (int i = 0; i < 4; ++i) c->hidden[i] = 1024; c->actor_lr = 1e-3f; }   /* run_rcsl_gauss.py */
  if (algo == ORL_ALGO_MCQ) { c->hidden[0] = c->hidden[1] = 400; c->actor_lr = c->critic_lr = c->alpha_lr = 3e-4f; c->target_entropy = -(float)c->act_dim; }
}

int64_t orl_arena_floats(const orl_config* cfg) {
  NetLayout lay[ORL_NUM_NETS];
  long off[ORL_NUM_NETS], pt = 0, pg = 0;
  bool tg[ORL_NUM_NETS];
  if (build_layouts(*cfg, lay, off, tg, &pt, &pg)) return -1;
  return (int64_t)cfg->n_runs * (pt + pg);
}

int orl_engine_create(const orl_config* cfg, orl_engine** out) {
  if (!cfg || !out) return fail("null argument");
  orl_engine* h = new orl_engine();
  if (h->e.init(*cfg)) { delete h; *out = nullptr; return -1; }
  *out = h;
  return 0;
}

void orl_engine_destroy(orl_engine* h) { if (h) { hipSetDevice(h->e.dev); hipStreamSynchronize(h->e.stream); delete h; } }

int orl_engine_sync(orl_engine* h) { ORL_HIP(hipStreamSynchronize(h->e.stream)); return 0; }

int orl_net_present(orl_engine* h, int net) { return net >= 0 && net < ORL_NUM_NETS && h->e.lay[net].present; }
int64_t orl_net_floats(orl_engine* h, int net) { return orl_net_present(h, net) ? h->e.lay[net].size : -1; }
int orl_net_num_tensors(orl_engine* h, int net) { return orl_net_present(h, net) ? (int)h->e.lay[net].tensors.size() : -1; }
int orl_net_tensor(orl_engine* h, int net, int idx, char* name, int name_cap, int64_t* offset, int32_t* ndim, int64_t shape[4]) {
  if (!orl_net_present(h, net)) return fail("net not present");
  if (h->e.lay[net].tensors.query(idx, name, name_cap, offset, ndim, shape)) return fail("tensor index out of range");
  return 0;
}
float* orl_net_ptr(orl_engine* h, int run, int net) {
  if (run < 0 || run >= h->e.R) return nullptr;
  return h->e.net_ptr(run, net);
}
int orl_net_set(orl_engine* h, int run, int net, const float* host, int64_t n) {
  float* d = orl_net_ptr(h, run, net);
  if (!d || n != h->e.lay[net].size) return fail("orl_net_set: bad net/run/size");
  ORL_HIP(hipSetDevice(h->e.dev));
  ORL_HIP(hipMemcpyAsync(d, host, sizeof(float) * n, hipMemcpyHostToDevice, h->e.stream));
  ORL_HIP(hipStreamSynchronize(h->e.stream));
  return 0;
}
int orl_net_get(orl_engine* h, int run, int net, float* host, int64_t n) {
  float* d = orl_net_ptr(h, run, net);
  if (!d || n != h->e.lay[net].size) return fail("orl_net_get: bad net/run/size");
  ORL_HIP(hipSetDevice(h->e.dev));
  ORL_HIP(hipStreamSynchronize(h->e.stream));
  ORL_HIP(hipMemcpy(host, d, sizeof(float) * n, hipMemcpyDeviceToHost));
  return 0;
}
int orl_scalar_set(orl_engine* h, int run, int which, float v) {
  Engine& e = h->e;
  if (run < 0 || run >= e.R) return fail("bad run");
  RunScalars s;
  ORL_HIP(hipStreamSynchronize(e.stream));
  ORL_HIP(hipMemcpy(&s, e.scalars + run, sizeof(s), hipMemcpyDeviceToHost));
  if (which == ORL_SCALAR_LOG_ALPHA) { s.log_alpha = v; if (e.cfg.auto_alpha) s.alpha = expf(v); }   // sac.py:46 / edac.py:45
  else if (which == ORL_SCALAR_CQL_LOG_ALPHA) s.cql_log_alpha = v;
  else if (which == ORL_SCALAR_ALPHA) s.alpha = v;       // resume: EDAC / SAC keep a clamped alpha between steps (edac.py:110)
  else if (which == ORL_SCALAR_LOG_ALPHA_M) s.la_m = v;
  else if (which == ORL_SCALAR_LOG_ALPHA_V) s.la_v = v;
  else if (which == ORL_SCALAR_CQL_LOG_ALPHA_M) s.cla_m = v;
  else if (which == ORL_SCALAR_CQL_LOG_ALPHA_V) s.cla_v = v;
  else if (which == ORL_SCALAR_LAST_ACTOR_LOSS) s.last_actor_loss = v;
  else return fail("scalar not settable");
  ORL_HIP(hipMemcpy(e.scalars + run, &s, sizeof(s), hipMemcpyHostToDevice));
  return 0;
}
int orl_scalar_get(orl_engine* h, int run, int which, float* v) {
  Engine& e = h->e;
  if (run < 0 || run >= e.R) return fail("bad run");
  RunScalars s;
  ORL_HIP(hipStreamSynchronize(e.stream));
  ORL_HIP(hipMemcpy(&s, e.scalars + run, sizeof(s), hipMemcpyDeviceToHost));
  if (which == ORL_SCALAR_LOG_ALPHA) *v = s.log_alpha;
  else if (which == ORL_SCALAR_CQL_LOG_ALPHA) *v = s.cql_log_alpha;
  else if (which == ORL_SCALAR_ALPHA) *v = e.cfg.auto_alpha ? s.alpha : e.cfg.alpha;
  else if (which == ORL_SCALAR_LOG_ALPHA_M) *v = s.la_m;
  else if (which == ORL_SCALAR_LOG_ALPHA_V) *v = s.la_v;
  else if (which == ORL_SCALAR_CQL_LOG_ALPHA_M) *v = s.cla_m;
  else if (which == ORL_SCALAR_CQL_LOG_ALPHA_V) *v = s.cla_v;
  else if (which == ORL_SCALAR_LAST_ACTOR_LOSS) *v = s.last_actor_loss;
  else return fail("unknown scalar");
  return 0;
}
int orl_set_lr(orl_engine* h, int opt, float lr) {
  if (opt < 0 || opt >= 8) return fail("bad optimizer id");
  h->e.hyper_host.lr[opt] = lr;
  ORL_HIP(hipMemcpyAsync(h->e.hyper, &h->e.hyper_host, sizeof(Hyper), hipMemcpyHostToDevice, h->e.stream));
  ORL_HIP(hipStreamSynchronize(h->e.stream));
  return 0;
}
int orl_reset_optimizers(orl_engine* h) {
  Engine& e = h->e;
  ORL_HIP(hipMemsetAsync(e.adam_m, 0, sizeof(float) * e.R * e.P_train, e.stream));
  ORL_HIP(hipMemsetAsync(e.adam_v, 0, sizeof(float) * e.R * e.P_train, e.stream));
  ORL_HIP(hipMemsetAsync(e.gstep, 0, 2 * sizeof(unsigned long long), e.stream));
  e.step_host = 0;
  ORL_HIP(hipStreamSynchronize(e.stream));
  return 0;
}
static int adam_xfer(orl_engine* h, int run, int net, float* m, float* v, int64_t n, bool to_host) {
  Engine& e = h->e;
  if (run < 0 || run >= e.R || net < 0 || net >= ORL_NUM_NETS || !e.lay[net].present || e.net_is_target[net]) return fail("orl_adam: bad run / net");
  if (n != e.lay[net].size || !m || !v) return fail("orl_adam: bad size");
  ORL_HIP(hipSetDevice(e.dev));
  ORL_HIP(hipStreamSynchronize(e.stream));
  const long off = (long)run * e.P_train + e.net_off[net];
  if (to_host) {
    ORL_HIP(hipMemcpy(m, e.adam_m + off, sizeof(float) * n, hipMemcpyDeviceToHost));
    ORL_HIP(hipMemcpy(v, e.adam_v + off, sizeof(float) * n, hipMemcpyDeviceToHost));
  } else {
    ORL_HIP(hipMemcpy(e.adam_m + off, m, sizeof(float) * n, hipMemcpyHostToDevice));
    ORL_HIP(hipMemcpy(e.adam_v + off, v, sizeof(float) * n, hipMemcpyHostToDevice));
  }
  return 0;
}
int orl_adam_get(orl_engine* h, int run, int net, float* m, float* v, int64_t n) { return adam_xfer(h, run, net, m, v, n, true); }
int orl_adam_set(orl_engine* h, int run, int net, const float* m, const float* v, int64_t n) {
  return adam_xfer(h, run, net, const_cast<float*>(m), const_cast<float*>(v), n, false);
}
int orl_set_step_count(orl_engine* h, int64_t steps) {
  Engine& e = h->e;
  if (steps < 0) return fail("negative step count");
  ORL_HIP(hipSetDevice(e.dev));
  ORL_HIP(hipStreamSynchronize(e.stream));
  const unsigned long long s[2] = {(unsigned long long)steps, (unsigned long long)steps};      // (both cells: gstep and gstep_pre)
  ORL_HIP(hipMemcpy(e.gstep, s, sizeof(s), hipMemcpyHostToDevice));
  e.step_host = s[0];
  return 0;
}

int orl_engine_attach_buffer(orl_engine* h, orl_buffer* b) {
  if (!b) { h->e.buf = nullptr; h->e.drop_graphs(); return 0; }
  if (b->b.od != h->e.od || b->b.ad != h->e.ad) return fail("attach_buffer: obs/act dims differ from the engine's");
  if (b->b.dev != h->e.dev) return fail("attach_buffer: buffer lives on another device");
  // split precision multiplies fp16 hi + lo planes: an observation or action component of 65504 or more is +-inf there.  The dataset is
  // checked once per load (buffer_absmax: a reduction over the HBM arrays, cached), not per sampled batch.
  float amax = 0.f;
  char msg[256];
  if (h->e.split_scales() && b->b.obs) {
    if (buffer_absmax(b->b, false, &amax)) return -1;
    if (!(amax < 65504.0f)) {
      snprintf(msg, sizeof(msg), "attach_buffer: the dataset's observations / actions reach |x| = %g, beyond the operand range of precision 1 "
               "(fp16 hi + lo planes, |x| < 65504): normalise the observations (ReplayBuffer.normalize_obs) or use precision 0", (double)amax);
      return fail(msg);
    }
  }
  // the reward column holds the return-to-go, column obs_dim of the net's input: an MFMA operand like the observations
  if (h->e.split_scales() && is_rcsl(h->e.cfg.algo) && b->b.rew) {
    if (buffer_absmax(b->b, true, &amax)) return -1;
    if (!(amax < 65504.0f)) {
      snprintf(msg, sizeof(msg), "attach_buffer: the dataset's returns-to-go (reward column) reach |x| = %g, beyond the operand range of "
               "precision 1 (fp16 hi + lo planes, |x| < 65504): scale the returns or use precision 0", (double)amax);
      return fail(msg);
    }
  }
  h->e.buf = &b->b;
  h->e.buf_gen = b->b.gen; h->e.buf_n = b->b.n;
  h->e.drop_graphs();             // captured graphs hold the old dataset pointers
  return 0;
}

int orl_engine_attach_model_buffer(orl_engine* h, orl_buffer* m, int32_t real_rows) {
  Engine& e = h->e;
  if (!m) { if (e.mbuf || !e.mbufs.empty()) { e.mbuf = nullptr; e.mbufs.clear(); e.mbuf_real_rows = 0; e.drop_graphs(); } return 0; }
  if (is_epoch_algo(e.cfg.algo)) return fail("attach_model_buffer: not available for RCSL engines (one dataset, no real + model batch)");
  if (m->b.od != e.od || m->b.ad != e.ad) return fail("attach_model_buffer: obs/act dims differ from the engine's");
  if (m->b.dev != e.dev) return fail("attach_model_buffer: buffer lives on another device");
  if (!m->b.d_n || m->b.cap < 1) return fail("attach_model_buffer: the model buffer must be a ring (orl_buffer_reserve)");
  if (real_rows <= 0 || real_rows >= e.B) return fail("attach_model_buffer: real_rows must be in (0, batch_size)");
  e.mbuf = &m->b; e.mbuf_real_rows = real_rows; e.mbuf_gen = m->b.gen;
  e.mbufs.clear();
  e.drop_graphs();
  return 0;
}

// the per-run source table of k_gather / k_prepare (engine-owned: captured graphs hold its address)
int Engine::upload_model_table() {
  std::vector<ModelSrc> host(mbufs.size());
  mbufs_gen.resize(mbufs.size());
  for (size_t r = 0; r < mbufs.size(); ++r) {
    host[r] = mbufs[r]->model_src();
    mbufs_gen[r] = mbufs[r]->gen;
  }
  ORL_HIP(hipStreamSynchronize(stream));
  ORL_HIP(hipMemcpy(m_tab, host.data(), sizeof(ModelSrc) * host.size(), hipMemcpyHostToDevice));
  return 0;
}

int orl_engine_attach_model_buffers(orl_engine* h, orl_buffer* const* models, int32_t n, int32_t real_rows) {
  Engine& e = h->e;
  if (!models || n == 0) return orl_engine_attach_model_buffer(h, nullptr, 0);
  if (is_epoch_algo(e.cfg.algo)) return fail("attach_model_buffers: not available for RCSL engines (one dataset, no real + model batch)");
  char msg[192];
  if (n != e.cfg.n_runs) {
    snprintf(msg, sizeof(msg), "attach_model_buffers: %d rings for an engine of %d runs (one ring per run)", (int)n, (int)e.cfg.n_runs);
    return fail(msg);
  }
  for (int r = 0; r < n; ++r) {
    const char* why = nullptr;
    if (!models[r]) why = "null ring";
    else if (models[r]->b.od != e.od || models[r]->b.ad != e.ad) why = "obs/act dims differ from the engine's";
    else if (models[r]->b.dev != e.dev) why = "buffer lives on another device";
    else if (!models[r]->b.d_n || models[r]->b.cap < 1) why = "the model buffer must be a ring (orl_buffer_reserve)";
    if (why) { snprintf(msg, sizeof(msg), "attach_model_buffers: run %d: %s", r, why); return fail(msg); }
  }
  if (real_rows <= 0 || real_rows >= e.B) return fail("attach_model_buffers: real_rows must be in (0, batch_size)");
  ORL_HIP(hipSetDevice(e.dev));
  if (!e.m_tab) {
    e.m_tab = (ModelSrc*)e.raw_alloc(sizeof(ModelSrc) * e.R);
    if (!e.m_tab) return fail("attach_model_buffers: hipMalloc of the source table");
  }
  e.mbuf = nullptr;
  e.mbufs.clear();
  for (int r = 0; r < n; ++r) e.mbufs.push_back(&models[r]->b);
  e.mbuf_real_rows = real_rows;
  e.drop_graphs();
  return e.upload_model_table();
}

// ---- hot path ----
static int copy_rows(Engine& e, const Mat& dst, const float* src, int rows, int dim, bool on_device, long row0 = 0) {
  if (!src) return fail("null input array");
  for (int r = 0; r < e.R; ++r) {
    ORL_HIP(hipMemcpy2DAsync(dst.p + r * dst.rs + row0 * dst.pitch, sizeof(float) * dst.pitch, src + (long)r * rows * dim,
                             sizeof(float) * dim, sizeof(float) * dim, rows, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e.stream));
  }
  return 0;
}

int orl_step(orl_engine* h, const orl_batch* b, const orl_noise* nz, float* metrics) {
  Engine& e = h->e;
  ORL_HIP(hipSetDevice(e.dev));
  const int B = e.B;
  if (e.cfg.algo == ORL_ALGO_MOBILE && !e.mobile_pending)
    return fail("orl_step: a MOBILE engine needs the next-state samples of this batch first (orl_engine_set_next_samples; one step per call)");
  if (b) {
    const bool dv = b->on_device != 0;
    if (copy_rows(e, e.W("b_obs2"), b->observations, B, e.od, dv, 0)) return -1;
    const bool rcsl = is_epoch_algo(e.cfg.algo);      // (reads observations, actions and the return-to-go in `rewards` only)
    const bool no_rtg = e.cfg.algo == ORL_ALGO_AUTOREG;      // (... and the autoregressive policy not even that)
    if (!(rcsl && !b->next_observations) && copy_rows(e, e.W("b_obs2"), b->next_observations, B, e.od, dv, B)) return -1;
    if (copy_rows(e, e.W("b_act"), b->actions, B, e.ad, dv)) return -1;
    if (!(no_rtg && !b->rewards) && copy_rows(e, e.W("b_rew"), b->rewards, B, 1, dv)) return -1;
    if (!(rcsl && !b->terminals) && copy_rows(e, e.W("b_term"), b->terminals, B, 1, dv)) return -1;
  }
  e.rcsl_mode = RI_SLOTS;
  if (nz) {
    const bool dv = nz->on_device != 0;
    for (size_t i = 0; i < e.noise_slots.size(); ++i)
      if (copy_rows(e, e.W(e.noise_slots[i].name), nz->slot[i], e.noise_slots[i].rows, e.noise_slots[i].cols ? e.noise_slots[i].cols : e.ad, dv)) return -1;
  }
  if (!e.prep.empty()) { if (e.enqueue_prepare(false, nz == nullptr)) return -1; }
  else if (!nz) { if (e.enqueue_noise()) return -1; }
  e.mobile_pending = false;      // (consumed, also by a step that fails below: the borrowed pointer is not kept)
  if (e.enqueue_step(e.step_variant())) return -1;
  e.step_host++;
  ORL_HIP(hipStreamSynchronize(e.stream));
  e.mobile_samples = nullptr;
  return e.finish(e.metrics_last, 1.0f, metrics, 1);
}

int orl_learn_n(orl_engine* h, int n_steps, float* metrics_mean, float* elapsed_ms) {
  Engine& e = h->e;
  ORL_HIP(hipSetDevice(e.dev));
  if (n_steps <= 0) return fail("n_steps must be positive");
  if (e.cfg.algo == ORL_ALGO_MOBILE)
    return fail("orl_learn_n: not available for MOBILE engines (every step needs the dynamics' next-state samples of its batch: "
                "orl_dynsample_next, orl_engine_set_next_samples, orl_step)");
  if (!e.buf || !e.buf->obs || e.buf->n < 1) return fail("orl_learn_n: no replay buffer attached");
  for (size_t r = 0; r < e.mbufs.size(); ++r)
    if (!e.mbufs[r]->obs || e.mbufs[r]->n < 1) {
      char msg[160];
      snprintf(msg, sizeof(msg), "orl_learn_n: the model buffer of run %d is empty (roll the dynamics out into it first)", (int)r);
      return fail(msg);
    }
  if (e.mbuf || !e.mbufs.empty()) {
    if (e.mbuf && (!e.mbuf->obs || e.mbuf->n < 1)) return fail("orl_learn_n: the model buffer is empty (roll the dynamics out into it first)");
    if (e.cfg.algo == ORL_ALGO_CQL && e.mbuf_real_rows != e.cfg.cql_real_rows)
      return fail("orl_learn_n: the model buffer's real_rows differs from the engine's cql_real_rows (COMBO's row layout)");
  }
  e.rcsl_mode = RI_DRAWN;
  ORL_HIP(hipMemsetAsync(e.metrics_sum, 0, sizeof(float) * e.R * e.nm, e.stream));
  // the buffer was reloaded (or, a ring attached as the primary source, grew) since the graphs were captured: they hold freed pointers
  // and the old size.  The model ring's size is read from its device cell: growth needs no re-capture, only a new reserve / load does.
  bool rings_moved = false;
  for (size_t r = 0; r < e.mbufs.size(); ++r) rings_moved = rings_moved || e.mbufs_gen[r] != e.mbufs[r]->gen;
  if (e.buf_gen != e.buf->gen || e.buf_n != e.buf->n || (e.mbuf && e.mbuf_gen != e.mbuf->gen) || rings_moved) {
    ORL_HIP(hipStreamSynchronize(e.stream));
    e.drop_graphs();
    e.buf_gen = e.buf->gen; e.buf_n = e.buf->n;
    if (e.mbuf) e.mbuf_gen = e.mbuf->gen;
    if (rings_moved && e.upload_model_table()) return -1;      // (a reserve moved a ring's arrays: the table holds the old pointers)
  }
  return e.run_steps(0, n_steps, true, metrics_mean, elapsed_ms);
}

int orl_learn_epoch(orl_engine* h, const int64_t* order, int64_t order_len, int on_device, float* metrics_mean, float* elapsed_ms) {
  Engine& e = h->e;
  ORL_HIP(hipSetDevice(e.dev));
  if (!is_epoch_algo(e.cfg.algo))
    return fail("orl_learn_epoch: available for RCSL engines only (the other algorithms sample with replacement: orl_learn_n)");
  if (!order) return fail("orl_learn_epoch: null row order");
  if (!e.buf || !e.buf->obs || e.buf->n < 1) return fail("orl_learn_epoch: no replay buffer attached");
  const int B = e.B;
  if (order_len <= 0 || order_len % B != 0) return fail("orl_learn_epoch: order_len must be a positive multiple of batch_size (pad the tail with -1)");
  const long n_steps = order_len / B, total = (long)e.R * order_len, n = e.buf->n;
  static_assert(sizeof(long long) == sizeof(int64_t), "row orders are int64");
  if (!on_device) {
    for (int r = 0; r < e.R; ++r)
      for (long s = 0; s < n_steps; ++s) {
        bool any = false;
        const int64_t* o = order + (long)r * order_len + s * B;
        for (int b = 0; b < B; ++b) {
          if (o[b] >= n) {
            char msg[192];
            snprintf(msg, sizeof(msg), "orl_learn_epoch: run %d, step %ld: row %lld is beyond the buffer's %ld rows", r, s, (long long)o[b], n);
            return fail(msg);
          }
          any = any || o[b] >= 0;
        }
        if (!any) {
          char msg[160];
          snprintf(msg, sizeof(msg), "orl_learn_epoch: run %d, step %ld: every row is padding", r, s);
          return fail(msg);
        }
      }
  }
  // the engine's own copy of the order: grown when needed, and only then are the graphs (which hold its address) dropped
  ORL_HIP(hipStreamSynchronize(e.stream));
  if (total > e.d_order_cap) {
    e.drop_graphs();
    if (e.mem.grow(&e.d_order, &e.d_order_cap, total, e.stream)) return -1;
  }
  ORL_HIP(hipMemcpy(e.d_order, order, sizeof(long long) * total, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  if (on_device) {      // one checking launch with a flag word: nothing of the epoch is launched when it comes back raised
    ORL_HIP(hipMemsetAsync(e.order_flags, 0, sizeof(unsigned int), e.stream));
    hipLaunchKernelGGL(k_order_check, dim3((unsigned)n_steps, e.R), dim3(256), 0, e.stream, (const long long*)e.d_order, (long)order_len, B, n, e.order_flags);
    if (hipGetLastError() != hipSuccess) return fail("orl_learn_epoch: checking launch failed");
    unsigned int fl = 0;
    ORL_HIP(hipMemcpyAsync(&fl, e.order_flags, sizeof(fl), hipMemcpyDeviceToHost, e.stream));
    ORL_HIP(hipStreamSynchronize(e.stream));
    if (fl & 1u) return fail("orl_learn_epoch: the row order holds an entry beyond the buffer's rows");
    if (fl & 2u) return fail("orl_learn_epoch: the row order holds a step whose rows are all padding");
  }
  const EpochCell cell{e.step_host, (long long)n_steps, (long long)order_len};
  ORL_HIP(hipMemcpy(e.epoch_cell, &cell, sizeof(cell), hipMemcpyHostToDevice));
  e.rcsl_mode = RI_ORDER;
  ORL_HIP(hipMemsetAsync(e.metrics_sum, 0, sizeof(float) * e.R * e.nm, e.stream));
  if (e.buf_gen != e.buf->gen || e.buf_n != e.buf->n) {      // (reloaded since the graphs were captured: they hold freed pointers / the old size)
    e.drop_graphs();
    e.buf_gen = e.buf->gen; e.buf_n = e.buf->n;
  }
  return e.run_steps(1, n_steps, false, metrics_mean, elapsed_ms);      // (graph_exec[1]: the ordered step)
}

int orl_autoreg_sample(orl_engine* h, const float* obs, int64_t n, const float* eps, int on_device, float* act_out) {
  Engine& e = h->e;
  if (e.cfg.algo != ORL_ALGO_AUTOREG) return fail("orl_autoreg_sample: not an AUTOREG engine");
  if (!obs || !act_out) return fail("orl_autoreg_sample: null observations / output");
  if (n < 1 || n > (1 << 24)) return fail("orl_autoreg_sample: n must be in [1, 2^24] rows per run");
  ORL_HIP(hipSetDevice(e.dev));
  return e.autoreg_sample(obs, (long)n, eps, on_device != 0, act_out);
}

int orl_engine_set_next_samples(orl_engine* h, const float* samples, int on_device) {
  Engine& e = h->e;
  if (e.cfg.algo != ORL_ALGO_MOBILE) return fail("orl_engine_set_next_samples: not a MOBILE engine");
  if (!samples) return fail("orl_engine_set_next_samples: null samples");
  ORL_HIP(hipSetDevice(e.dev));
  const int M = e.cfg.mobile_num_samples * e.cfg.mobile_num_elites * e.B;
  if (on_device) { e.mobile_samples = samples; e.mobile_samples_rs = (long)M * e.od; }
  else {
    const Mat& in = e.W("samples_in");
    if (copy_rows(e, in, samples, M, e.od, false)) return -1;
    e.mobile_samples = in.p; e.mobile_samples_rs = in.rs;
  }
  e.mobile_pending = true;
  return 0;
}

int orl_engine_lcb_penalty(orl_engine* h, const float* eps_lcb, float* penalty_out, int on_device) {
  Engine& e = h->e;
  if (e.cfg.algo != ORL_ALGO_MOBILE) return fail("orl_engine_lcb_penalty: not a MOBILE engine");
  if (!penalty_out) return fail("orl_engine_lcb_penalty: null output");
  if (!e.mobile_pending) return fail("orl_engine_lcb_penalty: no pending samples (orl_engine_set_next_samples first)");
  ORL_HIP(hipSetDevice(e.dev));
  const int M = e.cfg.mobile_num_samples * e.cfg.mobile_num_elites * e.B;
  const Mat& eps = e.W("n_eps_lcb");
  if (eps_lcb) { if (copy_rows(e, eps, eps_lcb, M, e.ad, on_device != 0)) return -1; }
  else {
    // the draws of noise slot 0 at the current step counter (the next orl_step draws the same ones: the counter does not move here)
    const long n = e.ws_len.at("n_eps_lcb");
    hipLaunchKernelGGL(k_noise, dim3((unsigned)((n / 4 + 256) / 256), e.R), dim3(256), 0, e.stream, eps.p, n, 0, e.cfg.act_low, e.cfg.act_high,
                       e.cfg.seed, (const unsigned long long*)e.gstep, 1u);
    if (hipGetLastError() != hipSuccess) return fail("orl_engine_lcb_penalty: noise launch failed");
  }
  e.mobile_pending = false;
  e.gscale_next = 0; e.cur_gscale = nullptr; e.lab_slot = 0;
  if (e.mobile_penalty(0)) return -1;
  const Mat& pen = e.W("penalty");
  for (int r = 0; r < e.R; ++r)
    ORL_HIP(hipMemcpyAsync(penalty_out + (long)r * e.B, pen.p + r * pen.rs, sizeof(float) * e.B,
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e.stream));
  ORL_HIP(hipStreamSynchronize(e.stream));
  e.mobile_samples = nullptr;
  return 0;
}

// the refusals orl_engine_adv_advantage and the device loop share; `who` prefixes the message
static int adv_refuse(const Engine& e, long rows, int term_kind, const char* who) {
  const std::string w(who);
  if (e.cfg.algo != ORL_ALGO_SAC) return fail(w + ": not a SAC engine");
  if (rows < 2) return fail(w + ": rows must be >= 2 (the unbiased standard deviation of one advantage is NaN)");
  if (rows > (1 << 22)) return fail(w + ": more than 2^22 rows per run");
  return term_refusal(w, term_kind, e.od, "engine");
}

int orl_engine_adv_advantage(orl_engine* h, const float* obs, const float* act, const float* next_obs, const float* reward, int32_t rows,
                             int32_t term_kind, int32_t include_ent, float* advantage, float* stats, int on_device) {
  if (!h || !obs || !act || !next_obs || !reward) return fail("orl_engine_adv_advantage: bad arguments");
  Engine& e = h->e;
  if (adv_refuse(e, rows, term_kind, "orl_engine_adv_advantage")) return -1;
  ORL_HIP(hipSetDevice(e.dev));
  if (e.adv_room(rows)) return -1;
  const size_t n = (size_t)e.R * rows;
  if (stage_in(e.stream, obs, e.adv_in[0].p, n * e.od, on_device) || stage_in(e.stream, act, e.adv_in[1].p, n * e.ad, on_device) ||
      stage_in(e.stream, next_obs, e.adv_in[2].p, n * e.od, on_device) || stage_in(e.stream, reward, e.adv_in[3].p, n, on_device))
    return -1;
  if (e.adv_advantage(obs, act, next_obs, reward, rows, term_kind, include_ent != 0, nullptr)) return -1;
  const hipMemcpyKind out_kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (advantage) ORL_HIP(hipMemcpyAsync(advantage, e.adv_v[4].p, sizeof(float) * n, out_kind, e.stream));
  if (stats) ORL_HIP(hipMemcpyAsync(stats, e.adv_stats, sizeof(float) * 2 * e.R, out_kind, e.stream));
  ORL_HIP(hipStreamSynchronize(e.stream));
  return 0;
}

int orl_rambo_update_dynamics(orl_engine* h, orl_dynamics* d, orl_buffer* real, const orl_rambo_loop* a, float* metrics_mean, float* elapsed_ms) {
  const char* F = "orl_rambo_update_dynamics";
  if (!h || !d || !real || !a || !metrics_mean) return fail(std::string(F) + ": bad arguments");
  Engine& e = h->e;
  Buffer& b = real->b;
  DynAdvInfo di;
  if (dynadv_info(d, &di)) return -1;
  if (adv_refuse(e, a->rows, a->term_kind, F)) return -1;
  if (e.R != 1 || di.R != 1) return fail(std::string(F) + ": one run per policy and per dynamics ensemble (n_runs == 1 on both)");
  if (!di.on) return fail(std::string(F) + ": orl_dynadv_configure first");
  if (a->rows != di.Ba || a->rows != di.Bs) {
    char msg[224];
    snprintf(msg, sizeof(msg), "%s: rows = %d, the adversary is configured for %d rollout and %d dataset rows", F, (int)a->rows, di.Ba, di.Bs);
    return fail(msg);
  }
  if (di.dev != e.dev || b.dev != e.dev) return fail(std::string(F) + ": engine, dynamics and buffer must live on one device");
  if (di.od != e.od || di.ad != e.ad || b.od != e.od || b.ad != e.ad) return fail(std::string(F) + ": obs / act dims of engine, dynamics and buffer differ");
  if (!b.obs || b.n < 1) return fail(std::string(F) + ": empty buffer");
  if (a->n_segments < 1 || !a->segment_steps) return fail(std::string(F) + ": no segments");
  long total = 0;
  for (int s = 0; s < a->n_segments; ++s) {
    if (a->segment_steps[s] < 1) return fail(std::string(F) + ": a segment needs at least one step");
    total += a->segment_steps[s];
  }
  if (total > (1L << 30)) return fail(std::string(F) + ": too many steps");
  ORL_HIP(hipSetDevice(e.dev));
  return e.rambo_loop(d, di, b, a, metrics_mean, elapsed_ms);
}

int orl_mobile_learn_n(orl_engine* h, orl_dynamics* d, int n_steps, float* metrics_mean, float* elapsed_ms) {
  const std::string f("orl_mobile_learn_n");
  if (!h || !d) return fail(f + ": bad arguments");
  Engine& e = h->e;
  DynSampleInfo di;
  if (dynsample_info(d, &di)) return -1;
  if (e.cfg.algo != ORL_ALGO_MOBILE) return fail(f + ": not a MOBILE engine");
  if (e.R != 1 || di.R != 1) return fail(f + ": one run per policy and per dynamics ensemble (n_runs == 1 on both)");
  if (di.dev != e.dev) return fail(f + ": engine and dynamics must live on one device");
  if (di.od != e.od || di.ad != e.ad) return fail(f + ": obs / act dims of engine and dynamics differ");
  if (!di.with_reward) return fail(f + ": needs a dynamics with_reward (MOBILE's ensemble predicts the reward; its column is drawn and dropped)");
  if (di.n_elites < 2) return fail(f + ": needs at least 2 elites (the standard deviation over one elite is NaN)");
  if (di.n_elites != e.cfg.mobile_num_elites) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: the dynamics has %d elites, the engine's row layout is built for mobile_num_elites = %d", f.c_str(),
             di.n_elites, (int)e.cfg.mobile_num_elites);
    return fail(msg);
  }
  if (!e.buf || !e.buf->obs || e.buf->n < 1) return fail(f + ": no replay buffer attached (orl_engine_attach_buffer)");
  if (!e.mbuf) return fail(f + ": no model ring attached (orl_engine_attach_model_buffer)");
  if (!e.mbuf->obs || e.mbuf->n < 1) return fail(f + ": the model buffer is empty (roll the dynamics out into it first)");
  if (e.mbuf_real_rows != e.cfg.mobile_real_rows)
    return fail(f + ": the model buffer's real_rows differs from the engine's mobile_real_rows (the penalty is zeroed on the real rows)");
  if (n_steps < 1) return fail(f + ": n_steps must be positive");
  if (e.mobile_pending)
    return fail(f + ": samples of orl_engine_set_next_samples are pending (the next orl_step consumes them; the loop draws its own)");
  ORL_HIP(hipSetDevice(e.dev));
  return e.mobile_loop(d, di, n_steps, metrics_mean, elapsed_ms);
}

int orl_mbrcsl_rollout(orl_engine* h, orl_dynamics* d, orl_traj* store, const float* init_obs, int32_t n_traj, int32_t length, int32_t term_kind,
                       int32_t penalty_mode, float penalty_coef, const float* eps, int32_t lag, int64_t* rows, double* reward_sum,
                       double* returns_host, int32_t* steps_enqueued, float* elapsed_ms) {
  const char* F = "orl_mbrcsl_rollout";
  const std::string f(F);
  if (!h || !d || !store || !init_obs || n_traj < 1 || length < 1) return fail(f + ": bad arguments");
  Engine& e = h->e;
  DynStepInfo di;
  TrajInfo ti;
  if (dynstep_info(d, &di) || traj_info(store, &ti)) return -1;
  char msg[256];
  if (e.cfg.algo != ORL_ALGO_AUTOREG) return fail(f + ": not an AUTOREG engine");
  if (e.R != 1 || di.R != 1) return fail(f + ": one run per policy and per dynamics ensemble (n_runs == 1 on both)");
  if (di.dev != e.dev || ti.dev != e.dev) return fail(f + ": engine, dynamics and trajectory store must live on one device");
  if (di.od != e.od || di.ad != e.ad || ti.od != e.od || ti.ad != e.ad) return fail(f + ": obs / act dims of engine, dynamics and trajectory store differ");
  if (!di.with_reward) return fail(f + ": needs a dynamics with_reward (the step splits the reward off the last output)");
  if (penalty_mode < 0 || penalty_mode > 2) return fail(f + ": unknown penalty mode");
  if (term_refusal(f, term_kind, e.od, "engine")) return -1;
  if (lag < 0) return fail(f + ": lag must be >= 0 (the steps enqueued before a survivor count is read)");
  if (n_traj > (1 << 24)) return fail(f + ": more than 2^24 trajectories");
  if (n_traj > ti.n_traj_cap) {
    snprintf(msg, sizeof(msg), "%s: %d trajectories, the store was created for %lld", F, (int)n_traj, (long long)ti.n_traj_cap);
    return fail(msg);
  }
  if ((long)n_traj * length > ti.cap) {
    snprintf(msg, sizeof(msg), "%s: %d trajectories x %d steps need %lld rows, the store's capacity is %lld", F, (int)n_traj, (int)length,
             (long long)n_traj * length, (long long)ti.cap);
    return fail(msg);
  }
  ORL_HIP(hipSetDevice(e.dev));
  return e.mbrcsl_loop(d, di, store, ti, init_obs, n_traj, length, term_kind, penalty_mode, penalty_coef, eps, lag, rows, reward_sum,
                       returns_host, steps_enqueued, elapsed_ms);
}

int orl_health(orl_engine* h, uint32_t* flags_out) {
  Engine& e = h->e;
  unsigned int all = 0;
  for (int r = 0; r < e.R; ++r) { all |= e.health_host[r]; if (flags_out) flags_out[r] = e.health_host[r]; }
  return (int)all;
}
int orl_health_check(orl_engine* h, uint32_t* flags_out) {
  Engine& e = h->e;
  if (hipSetDevice(e.dev) != hipSuccess) { fail("hipSetDevice"); return -1; }
  if (hipStreamSynchronize(e.stream) != hipSuccess) { fail("sync"); return -1; }
  unsigned int all = 0;
  if (e.health_update(nullptr, -1, &all)) return -1;
  if (flags_out) for (int r = 0; r < e.R; ++r) flags_out[r] = e.health_host[r];
  return (int)all;
}
int orl_health_clear(orl_engine* h) {
  Engine& e = h->e;
  ORL_HIP(hipSetDevice(e.dev));
  ORL_HIP(hipMemsetAsync(e.health, 0, sizeof(unsigned int) * e.R, e.stream));
  ORL_HIP(hipStreamSynchronize(e.stream));
  e.health_host.assign(e.R, 0u);
  return 0;
}

int orl_num_metrics(orl_engine* h) { return h->e.nm; }
const char* orl_metric_name(orl_engine* h, int idx) { return (idx >= 0 && idx < h->e.nm) ? h->e.metric_names[idx].c_str() : ""; }
int64_t orl_step_count(orl_engine* h) { return (int64_t)h->e.step_host; }

int64_t orl_debug_read(orl_engine* h, int run, const char* name, float* host, int64_t cap) {
  Engine& e = h->e;
  if (run < 0 || run >= e.R) { fail("bad run"); return -1; }
  auto ht = e.host_taps.find(name);
  if (ht != e.host_taps.end()) {
    if (cap < (int64_t)ht->second.size()) { fail("tap buffer too small"); return -1; }
    std::copy(ht->second.begin(), ht->second.end(), host);
    return (int64_t)ht->second.size();
  }
  // "gscale": this run's dynamic gradient scales of the last step, one per backward pass; the count is the number of values returned
  // (0 at precision 0).  Order of the slots, per schedule (a seed kernel that is one workgroup per run publishes its own; the others
  // come from a k_grad_scale launch, "<tag>.gscale" in the profile):
  //   RCSL, Gaussian RCSL, AUTOREG   [0] the seed kernel's dpred / dz / ar_dz
  //   SAC, MOBILE                    [0] dq (k_td_loss / k_mobile_td_loss)  [1] dhead
  //   CQL                            [0] dhead  [1] dq (k_cql_loss_rows: the largest entry of both critics' seeds)
  //   EDAC                           [0] dhead  [1] dq (k_td_loss), with eta > 0:  [2] the tail weights (edac.delta)  [3] gamma
  //   TD3+BC                         [0] dq, on an actor step:  [1] dqpi (k_td3_actor_loss: lambda / B)  [2] dmraw
  //   IQL                            [0] dv  [1] dq  [2] dmraw
  //   MCQ                            [0] dm3  [1] dehead  [2] dq (these three by k_grad_scale)  [3] dhead
  // dhead: k_head_bwd's own up to 256 rows, k_grad_scale ("actor.bwd.gscale") beyond; no slot when the fused actor update applies.
  if (!strcmp(name, "gscale")) {
    const int64_t n = e.gscale_count[e.last_step_variant()];
    if (cap < n) { fail("tap buffer too small"); return -1; }
    if (hipStreamSynchronize(e.stream) != hipSuccess) { fail("sync"); return -1; }
    if (n > 0 && hipMemcpy2D(host, sizeof(float), e.gscale_buf + run, sizeof(float) * e.R, sizeof(float), (size_t)n,
                             hipMemcpyDeviceToHost) != hipSuccess) { fail("tap copy"); return -1; }
    return n;
  }
  auto it = e.taps.find(name);
  if (it == e.taps.end()) { fail(std::string("unknown tap ") + name); return -1; }
  const Engine::Tap& t = it->second;
  const int64_t n = t.rows * t.cols;
  if (cap < n) { fail("tap buffer too small"); return -1; }
  if (hipStreamSynchronize(e.stream) != hipSuccess) { fail("sync"); return -1; }
  if (hipMemcpy2D(host, sizeof(float) * t.cols, t.m.p + run * t.m.rs, sizeof(float) * t.m.pitch, sizeof(float) * t.cols, t.rows,
                  hipMemcpyDeviceToHost) != hipSuccess) { fail("tap copy"); return -1; }
  return n;
}

// packed ReLU-mask words of a hidden activation of the LAST step (one 32-bit word per (row, 32 columns), all members of the family):
// returns the number of words written, or < 0 (unknown workspace / no mask / the producing launch did not emit bits)
int64_t orl_debug_read_bits(orl_engine* h, int run, const char* name, uint32_t* host, int64_t cap) {
  Engine& e = h->e;
  auto it = e.ws.find(name);
  if (it == e.ws.end() || !it->second.bits) { fail(std::string("no mask bits for workspace ") + name); return -1; }
  if (run < 0 || run >= e.R) { fail("bad run"); return -1; }
  const Mat& m = it->second;
  if (!e.bits_live.count(m.bits)) { fail(std::string("mask bits of ") + name + " were not emitted by the last step's kernels"); return -1; }
  if (cap < m.brs) { fail("bits buffer too small"); return -1; }
  if (hipStreamSynchronize(e.stream) != hipSuccess) { fail("sync"); return -1; }
  if (hipMemcpy(host, m.bits + (long)run * m.brs, sizeof(uint32_t) * m.brs, hipMemcpyDeviceToHost) != hipSuccess) { fail("bits copy"); return -1; }
  return m.brs;
}

// gradient of the LAST step w.r.t. every parameter of `net` (state_dict order, orl_net_floats values): the split-K slabs the
// backward kernels wrote, summed per tensor group (double accumulation on the host; k_adam sums the same slabs in fp32)
int orl_debug_grads(orl_engine* h, int run, int net, float* host, int64_t n) {
  Engine& e = h->e;
  if (run < 0 || run >= e.R) return fail("bad run");
  if (net < 0 || net >= ORL_NUM_NETS || !e.lay[net].present || e.net_is_target[net]) return fail("orl_debug_grads: not a trainable net");
  const NetLayout& l = e.lay[net];
  if (n != l.size) return fail("orl_debug_grads: bad size");
  const auto& segs = e.last_segs[net];
  if (segs.empty()) return fail("orl_debug_grads: no optimizer step has run for this net yet");
  int maxs = 1;
  for (auto& sg : segs) maxs = std::max(maxs, sg.second);
  ORL_HIP(hipSetDevice(e.dev));
  ORL_HIP(hipStreamSynchronize(e.stream));
  std::vector<float> tmp((size_t)maxs * l.size);
  const float* src = e.grads + (long)run * e.max_slab * e.P_train + e.net_off[net];
  ORL_HIP(hipMemcpy2D(tmp.data(), sizeof(float) * l.size, src, sizeof(float) * e.P_train, sizeof(float) * l.size, maxs, hipMemcpyDeviceToHost));
  long i = 0;
  for (auto& sg : segs) {
    for (; i < sg.first && i < l.size; ++i) {
      double a = 0.0;
      for (int k = 0; k < sg.second; ++k) a += tmp[(size_t)k * l.size + i];
      host[i] = (float)a;
    }
  }
  for (; i < l.size; ++i) host[i] = tmp[i];
  return 0;
}

int orl_profile_enable(orl_engine* h, int on) { h->e.prof_on = on != 0; return 0; }
int orl_profile_query(orl_engine* h, int idx, char* name, int name_cap, double* total_ms, int64_t* launches, double* flops_per_launch,
                      double* bytes_per_launch) {
  Engine& e = h->e;
  if (hipStreamSynchronize(e.stream) != hipSuccess) return fail("sync");
  std::map<std::string, std::tuple<double, int64_t, double, double>> agg;
  for (auto& p : e.prof) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) != hipSuccess) continue;
    auto& a = agg[p.name];
    std::get<0>(a) += ms; std::get<1>(a) += 1; std::get<2>(a) += p.flops; std::get<3>(a) += p.bytes;
  }
  std::vector<std::pair<double, std::string>> order;
  for (auto& kv : agg) order.push_back({-std::get<0>(kv.second), kv.first});
  std::sort(order.begin(), order.end());
  if (idx < 0 || idx >= (int)order.size()) return 1;
  const auto& a = agg[order[idx].second];
  snprintf(name, name_cap, "%s", order[idx].second.c_str());
  *total_ms = std::get<0>(a); *launches = std::get<1>(a); *flops_per_launch = std::get<2>(a) / std::get<1>(a);      // means over the tag's launches
  if (bytes_per_launch) *bytes_per_launch = std::get<3>(a) / std::get<1>(a);
  return 0;
}

}  // extern "C"
