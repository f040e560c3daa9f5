// algo_rcsl_gauss.inc — Gaussian RCSL schedule (policy/rcsl/rcsl_gauss.py:123-154; tests/rcsl_gauss_oracle.py).  Included by engine.hip.
// One net: z = MLP([obs | rtg]) with a plain linear output of act_dim columns, then the two A x A heads of DiagGaussian (k_rcslg_head:
// mu, clamped log-variance, loss, dz, head gradients in one launch), the generic backward from dz, one Adam step over body and heads.
// Inputs, the ordered epoch and the return-to-go in the reward slot are RCSL's (algo_rcsl.inc: rcsl_prepare).
namespace orl {

int Engine::rcslg_build() {
  const int A = ad;
  if (A > RG_AMAX) return fail("RCSL_GAUSS: act_dim beyond the head kernel's 32");
  metric_names = {"loss"};
  for (int i = 0; i < L; ++i) {
    const int h = cfg.hidden[i];
    const std::string s = std::to_string(i);
    alloc("ah" + s, B, h); alloc("dah" + s, B, h);
  }
  alloc("rcsl_x", B, rup(od + 1, 4));
  alloc("z", B, A); alloc("dz", B, A); alloc("mu", B, A); alloc("logvar", B, A);
  epoch_cell = (EpochCell*)raw_alloc(sizeof(EpochCell));
  order_flags = (unsigned int*)raw_alloc(sizeof(unsigned int));
  if (!epoch_cell || !order_flags) return fail("hipMalloc epoch cell");
  taps["z"] = {W("z"), B, A};
  taps["mu"] = {W("mu"), B, A};
  taps["logvar"] = {W("logvar"), B, A};
  taps["rcsl_x"] = {W("rcsl_x"), B, od + 1};
  return 0;
}

int Engine::rcslg_step() {
  const NetRef net = net_ref(ORL_NET_ACTOR, 1);
  const NetLayout& l = *net.lay;
  std::vector<Mat> ah, dah;
  for (int i = 0; i < L; ++i) { ah.push_back(W("ah" + std::to_string(i))); dah.push_back(W("dah" + std::to_string(i))); }
  const Mat x = W("rcsl_x"), act = W("b_act"), z = W("z");
  if (rcsl_prepare(rcsl_mode)) return -1;
  if (mlp_forward(x, B, net, ah, z, "rcslg")) return -1;
  float* gs = nullptr;
  {
    RcslGaussP p; memset(&p, 0, sizeof(p));
    p.z = z.p; p.z_rs = z.rs; p.act = act.p; p.act_rs = act.rs; p.apitch = act.pitch;
    p.head = net.base + l.extra_off; p.head_rs = net.rs;
    p.g_head = grads + net.g_off + l.extra_off; p.gh_rs = (long)max_slab * P_train;
    p.dz = W("dz").p; p.mu = W("mu").p; p.logvar = W("logvar").p;
    p.idx = rcsl_mode == RI_SLOTS ? nullptr : d_idx;      // (orl_step: every row of the caller's batch is valid)
    p.B = B; p.A = ad; p.lo = -5.0f; p.hi = 2.0f;         // DiagGaussian's sigma_min / sigma_max defaults, the only ones the policy accepts
    p.m = mp(); p.m.nm = (int)metric_names.size(); p.slot = 0;
    p.gs_out = gs = gscale_slot();                        // (split precision: the seed kernel publishes the dynamic scale of its backward pass)
    ORL_LAUNCH("rcslg_head", k_rcslg_head, dim3(R), dim3(256), p);
  }
  BwdOut bo;
  if (mlp_backward(this, net, x, ah, B, W("dz"), dah, true, false, 0, 0, nullptr, "rcslg.bwd", &bo, gs)) return -1;
  return adam(ORL_NET_ACTOR, 1, ORL_OPT_ACTOR, make_segs(l, bo.ks, bo.ks), -1);
}

}  // namespace orl
