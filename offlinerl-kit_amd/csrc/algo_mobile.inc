// algo_mobile.inc — MOBILE schedule (policy/model_based/mobile.py:130-196; tests/mobile_oracle.py): the SAC update of algo_sac.inc with
// the model-Bellman-inconsistency penalty in the TD target.  The penalty pass forwards the actor and the two TARGET critics on the
// S * E * B next-state samples orl_engine_set_next_samples handed over (orl_dynsample_next's row order) and reduces min(Q1, Q2) to
// mean over samples -> unbiased std over elites per batch row (k_lcb_penalty).  Then: critics first (target clamped at 0, one loss over
// both critics), the actor against the UPDATED critics, temperature clamped to [0, 1], Polyak with the critics' Adam.  Draw order of the
// reference: eps_lcb (compute_lcb's actforward), eps_next, eps_actor.  Included by engine.hip.
namespace orl {

int Engine::mobile_build() {
  const int A = ad, S = cfg.mobile_num_samples, E = cfg.mobile_num_elites;
  if (S < 1) return fail("MOBILE: mobile_num_samples must be >= 1");
  if (E < 2 || E > LCB_MAX_E) return fail("MOBILE: mobile_num_elites must be in [2, 64] (the standard deviation over one elite is NaN)");
  if (cfg.mobile_real_rows < 0 || cfg.mobile_real_rows > B) return fail("MOBILE: mobile_real_rows out of the batch");
  if ((long)S * E * B > (1L << 24)) return fail("MOBILE: more than 2^24 penalty rows");
  const int M = S * E * B;
  metric_names = {"loss/actor", "loss/critic"};
  add_sac_metrics(this);
  alloc("n_eps_lcb", M, A); alloc("n_eps_next", B, A); alloc("n_eps_actor", B, A);
  noise_slots = {{"n_eps_lcb", 0, M}, {"n_eps_next", 0, B}, {"n_eps_actor", 0, B}};      // mobile.py:153 (compute_lcb), :156, :170
  for (int i = 0; i < L; ++i) {
    const int h = cfg.hidden[i];
    const std::string s = std::to_string(i);
    alloc("ah" + s, B, h); alloc("dah" + s, B, h); alloc("an_h" + s, B, h);
    alloc("ca" + s, B, h, 2); alloc("dca" + s, B, h, 2);
    alloc("ct" + s, B, h, 2); alloc("q_h" + s, B, h, 2); alloc("dq_h" + s, B, h, 2);
    alloc("al_h" + s, M, h); alloc("cl_h" + s, M, h, 2);                               // the penalty pass: actor / target critics on M rows
  }
  alloc("head", B, 2 * A); alloc("head_n", B, 2 * A); alloc("dhead", B, 2 * A); alloc("head_l", M, 2 * A);
  alloc("xa", B, XP); alloc("xt", B, XP); alloc("xq", B, XP); alloc("xs", M, OP); alloc("xl", M, XP);
  alloc("logp_a", B, 1); alloc("logp_next", B, 1); alloc("logp_l", M, 1);
  alloc("qa", B, 1, 2); alloc("dqa", B, 1, 2); alloc("dxa", B, A, 2);
  alloc("qt", B, 1, 2); alloc("q", B, 1, 2); alloc("dq", B, 1, 2); alloc("target_q", B, 1);
  alloc("ql", M, 1, 2); alloc("lcb_q", M, 1); alloc("penalty", B, 1);
  alloc("samples_in", M, od);                                                            // a host array of orl_engine_set_next_samples lands here
  taps["q1"] = {W("q").net(0), B, 1};
  taps["q2"] = {W("q").net(1), B, 1};
  taps["q1a"] = {W("qa").net(0), B, 1};
  taps["q2a"] = {W("qa").net(1), B, 1};
  taps["logp_a"] = {W("logp_a"), B, 1};
  taps["target_q"] = {W("target_q"), B, 1};
  taps["penalty"] = {W("penalty"), B, 1};
  taps["lcb_q"] = {W("lcb_q"), M, 1};
  return 0;
}

// compute_lcb (mobile.py:130-142) on the pending samples; real_rows leading rows of the penalty are zeroed
int Engine::mobile_penalty(int real_rows) {
  const int A = ad, S = cfg.mobile_num_samples, E = cfg.mobile_num_elites, M = S * E * B;
  const NetRef actor = net_ref(ORL_NET_ACTOR, 1), tgt = net_ref(ORL_NET_CRITIC1_OLD, 2);
  std::vector<Mat> alh, clh;
  for (int i = 0; i < L; ++i) { alh.push_back(W("al_h" + std::to_string(i))); clh.push_back(W("cl_h" + std::to_string(i))); }
  Mat xs = W("xs"), xl = W("xl").shared();
  {
    MobileInP p; memset(&p, 0, sizeof(p));
    p.smp = mobile_samples; p.smp_rs = mobile_samples_rs;
    p.xs = xs.p; p.xs_rs = xs.rs; p.OP = xs.pitch;
    p.xl = xl.p; p.xl_rs = xl.rs; p.XP = xl.pitch;
    p.M = M; p.od = od; p.ad = ad;
    ORL_LAUNCH("lcb.assemble", k_mobile_assemble, dim3((M + 255) / 256, R), dim3(256), p);
  }
  {
    SampleJob j = make_job(0, M, 1, W("n_eps_lcb"), xl, od, 0, W("logp_l"));
    bool sampled = false;
    if (mlp_forward_only(xs, M, actor, alh, W("head_l"), "actor_lcb", &j, 1, &sampled)) return -1;
    if (!sampled && launch_sample(this, W("head_l"), A, &j, 1)) return -1;
  }
  if (mlp_forward_only(xl, M, tgt, clh, W("ql"), "target_lcb")) return -1;
  {
    LcbP p; memset(&p, 0, sizeof(p));
    p.ql = W("ql").p; p.ql_rs = W("ql").rs; p.ql_cs = W("ql").cs;
    p.qmin = W("lcb_q").p; p.qm_rs = W("lcb_q").rs;
    p.pen = W("penalty").p; p.pen_rs = W("penalty").rs;
    p.B = B; p.S = S; p.E = E; p.real_rows = real_rows; p.health = health;
    ORL_LAUNCH("lcb.penalty", k_lcb_penalty, dim3((B + 255) / 256, R), dim3(256), p);
  }
  return 0;
}

int Engine::mobile_step() {
  const int A = ad;
  const NetRef actor = net_ref(ORL_NET_ACTOR, 1), crit = net_ref(ORL_NET_CRITIC1, 2), tgt = net_ref(ORL_NET_CRITIC1_OLD, 2);
  Mat obs = W("b_obs2"), nobs = W("b_obs2").rows(B), act = W("b_act");
  std::vector<Mat> anh, ct, qh, dqh;
  for (int i = 0; i < L; ++i) {
    const std::string s = std::to_string(i);
    anh.push_back(W("an_h" + s)); ct.push_back(W("ct" + s)); qh.push_back(W("q_h" + s)); dqh.push_back(W("dq_h" + s));
  }
  Mat xt = W("xt").shared(), xq = W("xq").shared();
  const MetricsP m{metrics_last, metrics_sum, (int)metric_names.size()};

  // ---- penalty pass (mobile.py:153-154) ----
  if (mobile_penalty(cfg.mobile_real_rows)) return -1;
  // ---- TD target (mobile.py:156-162): a' ~ pi(s'), min Q_old(s', a') [- alpha logp'] ----
  if (mlp_forward_only(nobs, B, actor, anh, W("head_n"), "actor_next")) return -1;
  if (assemble(nobs, nullptr, xt, 0, B, 1)) return -1;
  {
    SampleJob j = make_job(0, B, 1, W("n_eps_next"), xt, od, 0, W("logp_next"));
    if (launch_sample(this, W("head_n"), A, &j, 1)) return -1;
  }
  if (mlp_forward_only(xt, B, tgt, ct, W("qt"), "target")) return -1;
  // ---- critics (mobile.py:151, 164-167) ----
  if (assemble(obs, &act, xq, 0, B, 1)) return -1;
  if (mlp_forward(xq, B, crit, qh, W("q"), "critic")) return -1;
  float* gs_dq = nullptr;
  {
    MobileTdP p; memset(&p, 0, sizeof(p));
    p.q = W("q").p; p.q_rs = W("q").rs; p.q_cs = W("q").cs; p.dq = W("dq").p;
    p.qt = W("qt").p; p.qt_rs = W("qt").rs; p.qt_cs = W("qt").cs;
    p.rew = W("b_rew").p; p.term = W("b_term").p; p.bt_rs = W("b_rew").rs;
    p.logp_next = W("logp_next").p; p.lpn_rs = W("logp_next").rs; p.use_alpha = cfg.deterministic_backup ? 0 : 1;
    p.pen = W("penalty").p; p.pen_rs = W("penalty").rs; p.pen_coef = cfg.penalty_coef;
    p.target_q = W("target_q").p; p.tq_rs = W("target_q").rs;
    p.B = B; p.gamma = cfg.gamma;
    p.sc = scalars; p.auto_alpha = cfg.auto_alpha; p.fixed_alpha = cfg.alpha; p.m = m; p.slot = 1;
    p.gs_out = gs_dq = gscale_slot();
    ORL_LAUNCH("td_loss", k_mobile_td_loss, dim3(R), dim3(256), p);
  }
  BwdOut bc;
  if (mlp_backward(this, crit, xq, qh, B, W("dq"), dqh, true, false, 0, 0, nullptr, "critic.bwd", &bc, gs_dq)) return -1;
  // critics_optim is ONE Adam over both critics; Polyak fused here is safe: nothing below reads the targets (mobile.py:185)
  if (adam(ORL_NET_CRITIC1, 2, ORL_OPT_CRITIC, make_segs(*crit.lay, bc.ks, bc.ks), ORL_NET_CRITIC1_OLD)) return -1;
  // ---- actor + temperature against the UPDATED critics (mobile.py:169-183; alpha clamped to [0, 1]) ----
  return sac_actor_phase(this, actor, crit, 2, true, 2);
}

}  // namespace orl
