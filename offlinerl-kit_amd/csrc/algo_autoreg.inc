// algo_autoreg.inc — autoregressive behaviour policy (policy/others/autoregressive.py:64-124; tests/autoreg_oracle.py).  Included by engine.hip.
// One net [Linear, LeakyReLU(0.01)] x (L + 1) on [obs | masked act | one-hot], two outputs (mean, logstd) per expanded row.  A step:
// k_autoreg_prepare (B rows -> M = A * B expanded rows, targets, row indices), the forward on the tiled GEMM's E_BIAS_LEAKY flavour down to
// the plain-linear tail, k_autoreg_head (the output LeakyReLU, masked Gaussian NLL, dz_tail, metric, split-precision scale), the generic
// backward with E_LEAKY_MASK, one Adam step.  orl_autoreg_sample: A forward-only passes over n rows with k_autoreg_draw between them.
namespace orl {

int Engine::autoreg_build() {
  const int A = ad, M = A * B;
  metric_names = {"loss"};
  for (int i = 0; i < L; ++i) {
    const int h = cfg.hidden[i];
    const std::string s = std::to_string(i);
    alloc("ah" + s, M, h); alloc("dah" + s, M, h);
  }
  alloc("ar_x", M, rup(od + 2 * A, 4));
  alloc("ar_z", M, 2); alloc("ar_dz", M, 2); alloc("ar_out", M, 2); alloc("ar_target", M, 1);
  epoch_cell = (EpochCell*)raw_alloc(sizeof(EpochCell));
  order_flags = (unsigned int*)raw_alloc(sizeof(unsigned int));
  ar_calls = (unsigned long long*)raw_alloc(sizeof(unsigned long long));
  if (!epoch_cell || !order_flags || !ar_calls) return fail("hipMalloc epoch cell");
  if (hipMemset(ar_calls, 0, sizeof(unsigned long long)) != hipSuccess) return fail("hipMemset sample counter");
  taps["ar_x"] = {W("ar_x"), M, od + 2 * A};
  taps["ar_out"] = {W("ar_out"), M, 2};
  taps["ar_target"] = {W("ar_target"), M, 1};
  return 0;
}

// the step's input launch: mode RI_SLOTS (orl_step), RI_DRAWN (orl_learn_n) or RI_ORDER (orl_learn_epoch)
int Engine::autoreg_prepare(int mode) {
  AutoregPrepP p;
  memset(&p, 0, sizeof(p));
  const Mat x = W("ar_x"), o2 = W("b_obs2"), act = W("b_act"), rew = W("b_rew"), t = W("ar_target");
  p.b_obs = o2.p; p.bo_rs = o2.rs; p.b_act = act.p; p.ba_rs = act.rs; p.b_rew = rew.p; p.br_rs = rew.rs;
  p.X = x.p; p.x_rs = x.rs; p.XP = x.pitch; p.T = t.p; p.t_rs = t.rs; p.OP = OP; p.AP = AP;
  p.idx_out = d_idx; p.B = B; p.od = od; p.A = ad;
  p.seed = cfg.seed; p.gstep = gstep;
  if (mode != RI_SLOTS) {
    if (!buf || !buf->obs) return fail("no replay buffer attached (orl_engine_attach_buffer)");
    p.d_obs = buf->obs; p.d_act = buf->act; p.d_rew = buf->rew; p.n = buf->n;
    p.order = d_order; p.cell = epoch_cell;
    if (mode == RI_ORDER && !d_order) return fail("ordered epoch without a row order");
  }
  const dim3 grid((unsigned)(((long)B * p.XP + 255) / 256), R);
  if (mode == RI_SLOTS) ORL_LAUNCH("autoreg_prepare", k_autoreg_prepare<RI_SLOTS>, grid, dim3(256), p);
  else if (mode == RI_DRAWN) ORL_LAUNCH("autoreg_prepare", k_autoreg_prepare<RI_DRAWN>, grid, dim3(256), p);
  else ORL_LAUNCH("autoreg_prepare", k_autoreg_prepare<RI_ORDER>, grid, dim3(256), p);
  return 0;
}

int Engine::autoreg_step() {
  const NetRef net = net_ref(ORL_NET_ACTOR, 1);
  const int M = ad * B;
  std::vector<Mat> ah, dah;
  for (int i = 0; i < L; ++i) { ah.push_back(W("ah" + std::to_string(i))); dah.push_back(W("dah" + std::to_string(i))); }
  const Mat x = W("ar_x"), z = W("ar_z");
  if (autoreg_prepare(rcsl_mode)) return -1;
  if (mlp_forward(x, M, net, ah, z, "autoreg")) return -1;
  float* gs = nullptr;
  {
    AutoregHeadP p; memset(&p, 0, sizeof(p));
    p.z = z.p; p.z_rs = z.rs; p.T = W("ar_target").p; p.t_rs = W("ar_target").rs;
    p.out = W("ar_out").p; p.dz = W("ar_dz").p;
    p.idx = rcsl_mode == RI_SLOTS ? nullptr : d_idx;      // (orl_step: every row of the caller's batch is valid)
    p.B = B; p.A = ad; p.m = mp(); p.m.nm = (int)metric_names.size(); p.slot = 0;
    p.gs_out = gs = gscale_slot();                        // (split precision: the seed kernel publishes the dynamic scale of its backward pass)
    ORL_LAUNCH("autoreg_head", k_autoreg_head, dim3(R), dim3(256), p);
  }
  BwdOut bo;
  if (mlp_backward(this, net, x, ah, M, W("ar_dz"), dah, true, false, 0, 0, nullptr, "autoreg.bwd", &bo, gs)) return -1;
  return adam(ORL_NET_ACTOR, 1, ORL_OPT_ACTOR, make_segs(*net.lay, bo.ks, bo.ks), -1);
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
  const int A = ad;
  const hipMemcpyKind in_kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // the n rows of every run lie packed at the front of the workspaces (which may hold more rows)
  auto view = [&](Mat m) { m.rs = n * m.pitch; m.cs = m.rs; return m; };
  const Mat x = view(ar_sx), z = view(ar_sz), ep = view(ar_seps);
  std::vector<Mat> hs;
  for (auto& m : ar_sh) hs.push_back(view(m));
  const float* d_obs = obs;
  if (!on_device) {
    ORL_HIP(hipMemcpyAsync(ar_sobs.p, obs, sizeof(float) * (size_t)R * n * od, hipMemcpyHostToDevice, stream));
    d_obs = ar_sobs.p;
  }
  if (eps) ORL_HIP(hipMemcpyAsync(ep.p, eps, sizeof(float) * (size_t)R * n * A, in_kind, stream));
  else {
    // device draws: Philox keyed by (seed, this entry point's call counter, run, element = row * A + dim) on a stream id no step uses
    hipLaunchKernelGGL(k_noise, dim3((unsigned)((n * A / 4 + 256) / 256), R), dim3(256), 0, stream, ep.p, n * A, 0, 0.f, 0.f, cfg.seed,
                       (const unsigned long long*)ar_calls, 0x5A5u);
    hipLaunchKernelGGL(k_tick, dim3(1), dim3(1), 0, stream, ar_calls);
    if (hipGetLastError() != hipSuccess) return fail("orl_autoreg_sample: noise launch failed");
  }
  AutoregDrawP d; memset(&d, 0, sizeof(d));
  d.z = z.p; d.z_rs = z.rs; d.eps = ep.p; d.e_rs = ep.rs; d.obs = d_obs; d.o_rs = n * od;
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
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  ORL_HIP(hipStreamSynchronize(stream));      // the only host synchronisation of the call
  return 0;
}

}  // namespace orl
