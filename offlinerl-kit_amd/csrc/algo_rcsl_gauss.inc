// algo_rcsl_gauss.inc — Gaussian RCSL schedule (policy/rcsl/rcsl_gauss.py:123-154; tests/rcsl_gauss_oracle.py).  Included by engine.hip.
// One net: z = MLP([obs | rtg]) with a plain linear output of act_dim columns, then the two A x A heads of DiagGaussian (k_rcslg_head:
// mu, clamped log-variance, loss, dz, head gradients in one launch), the generic backward from dz, one Adam step over body and heads.
// Inputs, the ordered epoch and the return-to-go in the reward slot are RCSL's (algo_rcsl.inc: rcsl_prepare).
namespace orl {

int Engine::rcslg_build() {
  const int A = ad;
  if (A > RG_AMAX) return fail("RCSL_GAUSS: act_dim beyond the head kernel's 32");
  metric_names = {"loss"};
  if (epoch_build(B)) return -1;
  alloc("rcsl_x", B, rup(od + 1, 4));
  alloc("z", B, A); alloc("dz", B, A); alloc("mu", B, A); alloc("logvar", B, A);
  taps["z"] = {W("z"), B, A};
  taps["dz"] = {W("dz"), B, A};                    // k_rcslg_head's seed; its head gradients are slab 0 of the arena (orl_debug_grads)
  taps["mu"] = {W("mu"), B, A};
  taps["logvar"] = {W("logvar"), B, A};
  taps["rcsl_x"] = {W("rcsl_x"), B, od + 1};
  return 0;
}

int Engine::rcslg_step() {
  return supervised_step(W("rcsl_x"), B, W("z"), W("dz"), "rcslg", [&](float* gs, const long long* idx) {
    const NetRef net = net_ref(ORL_NET_ACTOR, 1);
    const Mat act = W("b_act"), z = W("z");
    RcslGaussP p; memset(&p, 0, sizeof(p));
    p.z = z.p; p.z_rs = z.rs; p.act = act.p; p.act_rs = act.rs; p.apitch = act.pitch;
    p.head = net.base + net.lay->extra_off; p.head_rs = net.rs;
    p.g_head = grads + net.g_off + net.lay->extra_off; p.gh_rs = (long)max_slab * P_train;
    p.dz = W("dz").p; p.mu = W("mu").p; p.logvar = W("logvar").p;
    p.idx = idx; p.B = B; p.A = ad; p.lo = -5.0f; p.hi = 2.0f;         // DiagGaussian's sigma_min / sigma_max defaults, the only ones the policy accepts
    p.m = mp(); p.slot = 0; p.gs_out = gs;
    ORL_LAUNCH("rcslg_head", k_rcslg_head, dim3(R), dim3(256), p);
    return 0;
  });
}

}  // namespace orl
