// algo_autoreg.inc — autoregressive behaviour policy (policy/others/autoregressive.py:64-124; tests/autoreg_oracle.py).  Included by engine.hip.
// One net [Linear, LeakyReLU(0.01)] x (L + 1) on [obs | masked act | one-hot], two outputs (mean, logstd) per expanded row.  A step:
// k_autoreg_prepare (B rows -> M = A * B expanded rows, targets, row indices), the forward on the tiled GEMM's E_BIAS_LEAKY flavour down to
// the plain-linear tail, k_autoreg_head (the output LeakyReLU, masked Gaussian NLL, dz_tail, metric, split-precision scale), the generic
// backward with E_LEAKY_MASK, one Adam step.  orl_autoreg_sample: A forward-only passes over n rows with k_autoreg_draw between them.
namespace orl {

int Engine::autoreg_build() {
  const int A = ad, M = A * B;
  metric_names = {"loss"};
  if (epoch_build(M)) return -1;
  alloc("ar_x", M, rup(od + 2 * A, 4));
  alloc("ar_z", M, 2); alloc("ar_dz", M, 2); alloc("ar_out", M, 2); alloc("ar_target", M, 1);
  ar_calls = (unsigned long long*)raw_alloc(sizeof(unsigned long long));
  if (!ar_calls) return fail("hipMalloc sample counter");
  if (hipMemset(ar_calls, 0, sizeof(unsigned long long)) != hipSuccess) return fail("hipMemset sample counter");
  taps["ar_x"] = {W("ar_x"), M, od + 2 * A};
  taps["ar_z"] = {W("ar_z"), M, 2};                 // k_autoreg_head's operand (tail pre-activation) and its seed
  taps["ar_dz"] = {W("ar_dz"), M, 2};
  taps["ar_out"] = {W("ar_out"), M, 2};
  taps["ar_target"] = {W("ar_target"), M, 1};
  return 0;
}

int Engine::autoreg_prepare(int mode) {
  AutoregPrepP p;
  memset(&p, 0, sizeof(p));
  const Mat x = W("ar_x"), o2 = W("b_obs2"), act = W("b_act"), rew = W("b_rew"), t = W("ar_target");
  p.b_obs = o2.p; p.bo_rs = o2.rs; p.b_act = act.p; p.ba_rs = act.rs; p.b_rew = rew.p; p.br_rs = rew.rs;
  p.X = x.p; p.x_rs = x.rs; p.XP = x.pitch; p.T = t.p; p.t_rs = t.rs; p.A = ad;
  static void (*const kern[3])(AutoregPrepP) = {k_autoreg_prepare<RI_SLOTS>, k_autoreg_prepare<RI_DRAWN>, k_autoreg_prepare<RI_ORDER>};
  return epoch_prepare("autoreg_prepare", p, p.d_rew, mode, dim3((unsigned)(((long)B * p.XP + 255) / 256), R), kern);
}

int Engine::autoreg_step() {
  return supervised_step(W("ar_x"), ad * B, W("ar_z"), W("ar_dz"), "autoreg", [&](float* gs, const long long* idx) {
    AutoregHeadP p; memset(&p, 0, sizeof(p));
    p.z = W("ar_z").p; p.z_rs = W("ar_z").rs; p.T = W("ar_target").p; p.t_rs = W("ar_target").rs;
    p.out = W("ar_out").p; p.dz = W("ar_dz").p;
    p.idx = idx; p.B = B; p.A = ad; p.m = mp(); p.slot = 0; p.gs_out = gs;
    ORL_LAUNCH("autoreg_head", k_autoreg_head, dim3(R), dim3(256), p);
    return 0;
  });
}

// workspaces of orl_autoreg_sample for n rows per run; regrown (never shrunk) when n grows
int Engine::autoreg_sample_room(long n) {
  if (n <= ar_cap) return 0;
  auto drop = [&](Mat& m) {
    if (!m.p) return;
    range_watch.erase(m.p);
    allocs.erase(std::remove(allocs.begin(), allocs.end(), (void*)m.p), allocs.end());
    hipFree(m.p);
    m = Mat();
  };
  auto make = [&](Mat& m, int pitch) {
    m = Mat();
    m.p = raw_alloc(sizeof(float) * (size_t)n * pitch * R);
    m.pitch = pitch;
    return m.p != nullptr;
  };
  ORL_HIP(hipStreamSynchronize(stream));
  drop(ar_sx); drop(ar_sz); drop(ar_seps); drop(ar_sobs);
  for (auto& m : ar_sh) drop(m);
  ar_sh.assign(L, Mat());
  ar_cap = 0;
  bool ok = make(ar_sx, rup(od + 2 * ad, 4)) && make(ar_sz, 2) && make(ar_seps, ad) && make(ar_sobs, od);
  for (int i = 0; i < L && ok; ++i) ok = make(ar_sh[i], cfg.hidden[i]);
  if (!ok) return fail("orl_autoreg_sample: hipMalloc workspaces");
  ar_cap = n;
  return 0;
}

int Engine::autoreg_sample(const float* obs, long n, const float* eps, bool on_device, float* act_out) {
  if (autoreg_sample_room(n)) return -1;
  const hipMemcpyKind in_kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const float* d_obs = obs;
  if (!on_device) {
    ORL_HIP(hipMemcpyAsync(ar_sobs.p, obs, sizeof(float) * (size_t)R * n * od, hipMemcpyHostToDevice, stream));
    d_obs = ar_sobs.p;
  }
  // (the noise is staged in the workspace for device callers too: the tap "ar_seps" reads it there)
  if (eps) ORL_HIP(hipMemcpyAsync(ar_seps.p, eps, sizeof(float) * (size_t)R * n * ad, in_kind, stream));
  if (autoreg_sample_launches(d_obs, n, eps ? ar_seps.p : nullptr, act_out, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost)) return -1;
  ORL_HIP(hipStreamSynchronize(stream));      // the only host synchronisation of the call
  return 0;
}

// The MBRCSL rollout loop's form: the launches of a call on device rows, nothing staged and no synchronisation.  The workspaces hold
// the rows already (autoreg_sample_room, once, for the most rows of the loop); the kernels read `eps` ([n][act_dim] normals) where it lies.
int Engine::autoreg_sample_enqueue(const float* obs, long n, const float* eps, float* act_out) {
  if (n > ar_cap) return fail("autoreg_sample_enqueue: more rows than autoreg_sample_room made room for");
  return autoreg_sample_launches(obs, n, eps, act_out, hipMemcpyDeviceToDevice);
}

// what both forms launch: obs / eps are DEVICE arrays of n rows per run (eps null: drawn into the workspace), act_out by `out_kind`
int Engine::autoreg_sample_launches(const float* d_obs, long n, const float* eps, float* act_out, hipMemcpyKind out_kind) {
  const int A = ad;
  // the n rows of every run lie packed at the front of the workspaces (which may hold more rows)
  auto view = [&](Mat m) { m.rs = n * m.pitch; m.cs = m.rs; return m; };
  const Mat x = view(ar_sx), z = view(ar_sz), ep = view(ar_seps);
  std::vector<Mat> hs;
  for (auto& m : ar_sh) hs.push_back(view(m));
  // the workspaces of THIS call as taps (a host map write, no launch): the input rows as the last draw left them, the tail of the last
  // pass and the noise, n rows each (the workspaces may be regrown by a later call, which registers them anew)
  taps["ar_sx"] = {x, n, x.pitch}; taps["ar_sz"] = {z, n, 2}; taps["ar_seps"] = {ep, n, A};
  if (!eps) {
    // device draws: Philox keyed by (seed, this entry point's call counter, run, element = row * A + dim) on a stream id no step uses
    hipLaunchKernelGGL(k_noise, dim3((unsigned)((n * A / 4 + 256) / 256), R), dim3(256), 0, stream, ep.p, n * A, 0, 0.f, 0.f, cfg.seed,
                       (const unsigned long long*)ar_calls, 0x5A5u);
    hipLaunchKernelGGL(k_tick, dim3(1), dim3(1), 0, stream, ar_calls);
    if (hipGetLastError() != hipSuccess) return fail("orl_autoreg_sample: noise launch failed");
  }
  AutoregDrawP d; memset(&d, 0, sizeof(d));
  d.z = z.p; d.z_rs = z.rs; d.eps = eps ? eps : ep.p; d.e_rs = ep.rs; d.obs = d_obs; d.o_rs = n * od;
  d.X = x.p; d.x_rs = x.rs; d.XP = x.pitch; d.n = n; d.od = od; d.A = A; d.first = 1;
  const dim3 grid((unsigned)((n + 255) / 256), R);
  ORL_LAUNCH("autoreg_draw", k_autoreg_draw, grid, dim3(256), d);
  d.first = 0;
  const NetRef net = net_ref(ORL_NET_ACTOR, 1);
  gscale_next = 0; cur_gscale = nullptr; lab_slot = 0;
  for (int j = 0; j < A; ++j) {
    if (mlp_forward_only(x, (int)n, net, hs, z, "autoreg.sample")) return -1;
    d.j = j;
    ORL_LAUNCH("autoreg_draw", k_autoreg_draw, grid, dim3(256), d);
  }
  ORL_HIP(hipMemcpy2DAsync(act_out, sizeof(float) * A, x.p + od, sizeof(float) * x.pitch, sizeof(float) * A, (size_t)R * n,
                           out_kind, stream));
  return 0;
}

}  // namespace orl
