// algo_iql.inc — IQL schedule (policy/model_free/iql.py:86-139; oracle/iql.py).  Included by engine.hip.
namespace orl {

int Engine::iql_build() {
  const int A = ad;
  metric_names = {"loss/actor", "loss/q1", "loss/q2", "loss/v"};
  alloc_layers("ah", B); alloc_layers("dah", B);
  alloc_layers("qo_h", B, 2); alloc_layers("q_h", B, 2); alloc_layers("dq_h", B, 2);
  alloc_layers("v_h", B); alloc_layers("dv_h", B); alloc_layers("v2_h", 2 * B);
  alloc("xq", B, XP);
  alloc("qo", B, 1, 2); alloc("q", B, 1, 2); alloc("dq", B, 1, 2);
  alloc("v", B, 1); alloc("dv", B, 1); alloc("v2", 2 * B, 1); alloc("qmin", B, 1); alloc("exp_a", B, 1); alloc("target_q", B, 1);
  alloc("mraw", B, A); alloc("dmraw", B, A);
  if (cfg.actor_dropout > 0.f) {      // keep masks of the actor backbone's nn.Dropout layers, one per hidden layer (run_iql.py:106)
    for (const std::string& n : alloc_layers("n_drop_a", B)) noise_slots.push_back({n, 2, B, W(n).pitch});
  }
  taps["q1"] = {W("q").net(0), B, 1};
  taps["q2"] = {W("q").net(1), B, 1};
  taps["v"] = {W("v"), B, 1};
  taps["target_q"] = {W("target_q"), B, 1};
  taps["exp_a"] = {W("exp_a"), B, 1};
  // operands / results of k_iql_v_loss, k_iql_q_loss, k_iql_actor_loss
  taps["qo1"] = {W("qo").net(0), B, 1};
  taps["qo2"] = {W("qo").net(1), B, 1};
  taps["qmin"] = {W("qmin"), B, 1};
  taps["v2"] = {W("v2"), 2 * B, 1};
  taps["dv"] = {W("dv"), B, 1};
  taps["dq1"] = {W("dq").net(0), B, 1};
  taps["dq2"] = {W("dq").net(1), B, 1};
  taps["mraw"] = {W("mraw"), B, A};
  taps["dmraw"] = {W("dmraw"), B, A};
  return 0;
}

int Engine::iql_step() {
  const int A = ad;
  const NetRef actor = net_ref(ORL_NET_ACTOR, 1), qn = net_ref(ORL_NET_CRITIC1, 2), qo = net_ref(ORL_NET_CRITIC1_OLD, 2),
               vn = net_ref(ORL_NET_CRITIC_V, 1);
  Mat obs = W("b_obs2"), obs2 = W("b_obs2"), act = W("b_act");
  std::vector<Mat> ah = layers("ah"), dah = layers("dah"), qoh = layers("qo_h"), qh = layers("q_h"), dqh = layers("dq_h"),
                   vh = layers("v_h"), dvh = layers("dv_h"), v2h = layers("v2_h");
  Mat xq = W("xq").shared();
  if (assemble(obs, &act, xq, 0, B, 1)) return -1;

  float *gs_v = nullptr, *gs_q = nullptr, *gs_a = nullptr;
  // ---- value net (iql.py:90-98) ----
  if (mlp_forward_only(xq, B, qo, qoh, W("qo"), "q_old")) return -1;
  if (mlp_forward(obs, B, vn, vh, W("v"), "v")) return -1;
  {
    IqlVP p; memset(&p, 0, sizeof(p));
    p.qo = W("qo").z(); p.v = W("v").p; p.v_rs = W("v").rs; p.dv = W("dv").p;
    p.qmin = W("qmin").p; p.qmin_rs = W("qmin").rs; p.B = B; p.expectile = cfg.expectile; p.m = mp(); p.m.nm = (int)metric_names.size(); p.slot = 3;
    p.gs_out = gs_v = gscale_slot();               // (split precision: the seed kernel publishes the dynamic scale of its backward pass)
    ORL_LAUNCH("iql_v_loss", k_iql_v_loss, dim3(R), dim3(256), p);
  }
  if (train_net(vn, ORL_NET_CRITIC_V, 1, ORL_OPT_CRITIC_V, obs, vh, B, W("dv"), dvh, "v.bwd", gs_v)) return -1;

  // ---- critics (iql.py:100-116): target from the UPDATED V ----
  if (mlp_forward(xq, B, qn, qh, W("q"), "q")) return -1;
  if (mlp_forward_only(obs2, 2 * B, vn, v2h, W("v2"), "v2")) return -1;
  {
    IqlQP p; memset(&p, 0, sizeof(p));
    p.q = W("q").z(); p.dq = W("dq").p;
    p.v2 = W("v2").p; p.v2_rs = W("v2").rs; p.qmin = W("qmin").p; p.qmin_rs = W("qmin").rs;
    p.rew = W("b_rew").p; p.term = W("b_term").p; p.bt_rs = W("b_rew").rs;
    p.exp_a = W("exp_a").p; p.ea_rs = W("exp_a").rs; p.target_q = W("target_q").p; p.tq_rs = W("target_q").rs;
    p.B = B; p.gamma = cfg.gamma; p.beta = cfg.iql_temperature; p.m = mp(); p.m.nm = (int)metric_names.size(); p.slot_q1 = 1; p.slot_q2 = 2;
    p.gs_out = gs_q = gscale_slot();
    ORL_LAUNCH("iql_q_loss", k_iql_q_loss, dim3(R), dim3(256), p);
  }
  // Polyak fused here is safe: the actor step below only needs exp_a, already computed from the old targets
  if (train_net(qn, ORL_NET_CRITIC1, 2, ORL_OPT_CRITIC, xq, qh, B, W("dq"), dqh, "q.bwd", gs_q, ORL_NET_CRITIC1_OLD)) return -1;

  // ---- actor (iql.py:118-131) ----
  const float pdrop = cfg.actor_dropout;
  if (pdrop > 0.f) {                   // policy.train() mode: the actor backbone's Dropout layers are active in this forward (iql.py:127)
    if (mlp_forward_dropout(obs, B, actor, ah, W("mraw"), "actor", pdrop, layers("n_drop_a"))) return -1;
  } else if (mlp_forward(obs, B, actor, ah, W("mraw"), "actor")) return -1;
  {
    IqlAP p; memset(&p, 0, sizeof(p));
    const NetLayout& al = lay[ORL_NET_ACTOR];
    p.mraw = W("mraw").p; p.mraw_rs = W("mraw").rs; p.act = act.p; p.act_rs = act.rs; p.apitch = act.pitch;
    p.exp_a = W("exp_a").p; p.ea_rs = W("exp_a").rs;
    p.sigma_param = net_ptr(0, ORL_NET_ACTOR) + al.extra_off; p.sp_rs = P_train;
    p.dmraw = W("dmraw").p;
    p.g_sigma = grads + net_off[ORL_NET_ACTOR] + al.extra_off; p.gs_rs = (long)max_slab * P_train;
    p.B = B; p.A = A; p.m = mp(); p.m.nm = (int)metric_names.size(); p.slot = 0;
    p.gs_out = gs_a = gscale_slot();
    ORL_LAUNCH("iql_actor_loss", k_iql_actor_loss, dim3(R), dim3(256), p);
  }
  bwd_scale = pdrop > 0.f ? 1.0f / (1.0f - pdrop) : 1.0f;
  const int rc_a = train_net(actor, ORL_NET_ACTOR, 1, ORL_OPT_ACTOR, obs, ah, B, W("dmraw"), dah, "actor.bwd", gs_a);
  bwd_scale = 1.0f;
  return rc_a;
}

}  // namespace orl
