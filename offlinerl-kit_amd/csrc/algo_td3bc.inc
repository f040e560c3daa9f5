// algo_td3bc.inc — TD3+BC schedule (policy/model_free/td3bc.py:83-124, td3.py:16-59; oracle/td3bc.py).
namespace orl {

int Engine::td3bc_build() {
  const int A = ad;
  metric_names = {"loss/actor", "loss/critic1", "loss/critic2"};
  alloc("n_eps_target", B, A);
  noise_slots = {{"n_eps_target", 0, B}};
  alloc_layers("ah", B); alloc_layers("dah", B); alloc_layers("ao_h", B);
  alloc_layers("ct", B, 2); alloc_layers("q_h", B, 2); alloc_layers("dq_h", B, 2);
  alloc_layers("cp_h", B); alloc_layers("dcp_h", B);
  alloc("xq", B, XP); alloc("xt", B, XP); alloc("xa", B, XP);
  alloc("mraw_t", B, A); alloc("mraw", B, A); alloc("dmraw", B, A); alloc("dxa", B, A);
  alloc("qt", B, 1, 2); alloc("q", B, 1, 2); alloc("dq", B, 1, 2); alloc("qpi", B, 1); alloc("dqpi", B, 1); alloc("target_q", B, 1);
  taps["q1"] = {W("q").net(0), B, 1};
  taps["q2"] = {W("q").net(1), B, 1};
  taps["target_q"] = {W("target_q"), B, 1};
  taps["q_pi"] = {W("qpi"), B, 1};
  // operands / results of k_det_action, k_td_loss, k_td3_actor_loss, k_td3_actor_bwd
  taps["qt1"] = {W("qt").net(0), B, 1};
  taps["qt2"] = {W("qt").net(1), B, 1};
  taps["dq1"] = {W("dq").net(0), B, 1};
  taps["dq2"] = {W("dq").net(1), B, 1};
  taps["mraw"] = {W("mraw"), B, A};
  taps["mraw_t"] = {W("mraw_t"), B, A};
  taps["xt"] = {W("xt"), B, XP};
  taps["xa"] = {W("xa"), B, XP};
  taps["dxa"] = {W("dxa"), B, A};
  taps["dqpi"] = {W("dqpi"), B, 1};
  taps["dmraw"] = {W("dmraw"), B, A};
  return 0;
}

int Engine::td3bc_step(bool actor_step) {
  const int A = ad;
  const NetRef actor = net_ref(ORL_NET_ACTOR, 1), actor_old = net_ref(ORL_NET_ACTOR_OLD, 1), crit = net_ref(ORL_NET_CRITIC1, 2),
               crit1 = net_ref(ORL_NET_CRITIC1, 1), tgt = net_ref(ORL_NET_CRITIC1_OLD, 2);
  Mat obs = W("b_obs2"), nobs = W("b_obs2").rows(B), act = W("b_act");
  std::vector<Mat> ah = layers("ah"), dah = layers("dah"), aoh = layers("ao_h"), ct = layers("ct"), qh = layers("q_h"), dqh = layers("dq_h"),
                   cph = layers("cp_h"), dcph = layers("dcp_h");
  Mat xq = W("xq").shared(), xt = W("xt").shared(), xa = W("xa").shared();
  const MetricsP m{metrics_last, metrics_sum, (int)metric_names.size()};

  // ---- target (td3bc.py:89-93): a' = clamp(pi_old(s') + clipped noise) ----
  if (mlp_forward_only(nobs, B, actor_old, aoh, W("mraw_t"), "actor_old")) return -1;
  if (assemble(nobs, nullptr, xt, 0, B, 1)) return -1;
  {
    DetActP p; memset(&p, 0, sizeof(p));
    p.mraw = W("mraw_t").p; p.mraw_rs = W("mraw_t").rs; p.eps = W("n_eps_target").p; p.eps_rs = W("n_eps_target").rs;
    p.X = xt.p; p.x_rs = xt.rs; p.XP = XP; p.od = od; p.B = B; p.A = A;
    p.max_action = cfg.max_action; p.policy_noise = cfg.policy_noise; p.noise_clip = cfg.noise_clip;
    ORL_LAUNCH("det_action", k_det_action, dim3((B * A + 255) / 256, R), dim3(256), p);
  }
  if (mlp_forward_only(xt, B, tgt, ct, W("qt"), "target")) return -1;
  float *gs_dq = nullptr, *gs_pi = nullptr, *gs_a = nullptr;
  // ---- critics (td3bc.py:88,95-104) ----
  if (assemble(obs, &act, xq, 0, B, 1)) return -1;
  if (mlp_forward(xq, B, crit, qh, W("q"), "critic")) return -1;
  if (td_loss(2, 2, 1, 0, 0, false, &gs_dq)) return -1;
  // on the delayed-update steps the critics' Polyak sync (td3bc.py:65-71, after both updates) rides in their Adam launch: the actor phase below
  // reads the ONLINE critic only, and the targets are not read again before the next step
  if (train_net(crit, ORL_NET_CRITIC1, 2, ORL_OPT_CRITIC, xq, qh, B, W("dq"), dqh, "critic.bwd", gs_dq, actor_step ? ORL_NET_CRITIC1_OLD : -1)) return -1;

  if (!actor_step) {
    ORL_LAUNCH("td3_report", k_td3_report_last, dim3(R), dim3(64), (const RunScalars*)scalars, m, 0);
    return 0;
  }
  // ---- delayed actor update + target sync (td3bc.py:106-116) ----
  if (mlp_forward(obs, B, actor, ah, W("mraw"), "actor")) return -1;
  if (assemble(obs, nullptr, xa, 0, B, 1)) return -1;
  {
    DetActP p; memset(&p, 0, sizeof(p));
    p.mraw = W("mraw").p; p.mraw_rs = W("mraw").rs; p.X = xa.p; p.x_rs = xa.rs; p.XP = XP; p.od = od; p.B = B; p.A = A;
    p.max_action = cfg.max_action;
    ORL_LAUNCH("det_action", k_det_action, dim3((B * A + 255) / 256, R), dim3(256), p);
  }
  if (mlp_forward(xa, B, crit1, cph, W("qpi"), "critic_pi")) return -1;      // UPDATED critic1
  {
    Td3ActorP p; memset(&p, 0, sizeof(p));
    p.q = W("qpi").p; p.q_rs = W("qpi").rs; p.dq = W("dqpi").p; p.xa = xa.p; p.xa_rs = xa.rs; p.XP = XP; p.od = od;
    p.act = act.p; p.act_rs = act.rs; p.apitch = act.pitch; p.B = B; p.A = A; p.alpha = cfg.td3bc_alpha; p.sc = scalars; p.m = m; p.slot = 0;
    p.gs_out = gs_pi = gscale_slot();
    ORL_LAUNCH("td3_actor_loss", k_td3_actor_loss, dim3(R), dim3(256), p);
  }
  Mat dxa = W("dxa");
  const InputGrad da{od, A, &dxa};
  if (mlp_backward(this, crit1, xa, cph, B, W("dqpi"), dcph, false, &da, "critic_pi.bwd", nullptr, gs_pi)) return -1;
  {
    Td3ActorBwdP p; memset(&p, 0, sizeof(p));
    p.dxa = dxa.p; p.dxa_rs = dxa.rs; p.dxa_pitch = A; p.xa = xa.p; p.xa_rs = xa.rs; p.XP = XP; p.od = od;
    p.act = act.p; p.act_rs = act.rs; p.apitch = act.pitch; p.dmraw = W("dmraw").p; p.dm_rs = W("dmraw").rs;
    p.B = B; p.A = A; p.max_action = cfg.max_action;
    p.gs_out = gs_a = gscale_slot();
    ORL_LAUNCH("td3_actor_bwd", k_td3_actor_bwd, dim3(R), dim3(256), p);
  }
  const unsigned long long f = cfg.update_actor_freq > 0 ? cfg.update_actor_freq : 1;
  return train_net(actor, ORL_NET_ACTOR, 1, ORL_OPT_ACTOR, obs, ah, B, W("dmraw"), dah, "actor.bwd", gs_a, ORL_NET_ACTOR_OLD, f);
}

}  // namespace orl
