// algo_sac.inc — plain SAC schedule (policy/model_free/sac.py:88-140; oracle/sac.py): the update MOPOPolicy.learn runs on the
// concatenation of a real and a model-generated batch (model_based/mopo.py:81-84).  Order of the reference: critics first (TD target
// with the CURRENT actor and alpha, stochastic backup always), then the actor against the UPDATED critics, temperature clamped to
// [0, 1], Polyak at the end.  Included by engine.hip.
namespace orl {

// SAC's workspaces and taps; MOBILE (algo_mobile.inc) adds its penalty pass to them.  The callers list the noise slots.
void Engine::sac_alloc() {
  const int A = ad;
  sac_family_alloc(2);
  alloc("n_eps_next", B, A);
  alloc_layers("an_h", B); alloc_layers("ct", B, 2); alloc_layers("q_h", B, 2); alloc_layers("dq_h", B, 2);
  alloc("head_n", B, 2 * A);
  alloc("xt", B, XP); alloc("xq", B, XP);
  alloc("logp_next", B, 1);
  alloc("qt", B, 1, 2); alloc("q", B, 1, 2); alloc("dq", B, 1, 2); alloc("target_q", B, 1);
  taps["q1"] = {W("q").net(0), B, 1};
  taps["q2"] = {W("q").net(1), B, 1};
  taps["q1a"] = {W("qa").net(0), B, 1};
  taps["q2a"] = {W("qa").net(1), B, 1};
  taps["target_q"] = {W("target_q"), B, 1};
  // operands and seed of the critic loss (k_td_loss / k_mobile_td_loss), named as CQL and TD3+BC name them
  taps["qt1"] = {W("qt").net(0), B, 1};
  taps["qt2"] = {W("qt").net(1), B, 1};
  taps["dq1"] = {W("dq").net(0), B, 1};
  taps["dq2"] = {W("dq").net(1), B, 1};
  taps["logp_next"] = {W("logp_next"), B, 1};
}

int Engine::sac_build() {
  metric_names = {"loss/actor", "loss/critic1", "loss/critic2"};
  add_sac_metrics(this);
  sac_alloc();
  noise_slots = {{"n_eps_next", 0, B}, {"n_eps_actor", 0, B}};      // the reference's draw order: actforward(next_obss) first (sac.py:95)
  return 0;
}

// TD target inputs (sac.py:94-100): a' ~ pi(s') with the CURRENT actor, then the target critics on (s', a')
int Engine::sac_td_target() {
  const NetRef actor = net_ref(ORL_NET_ACTOR, 1), tgt = net_ref(ORL_NET_CRITIC1_OLD, 2);
  Mat nobs = W("b_obs2").rows(B), xt = W("xt").shared();
  std::vector<Mat> anh = layers("an_h"), ct = layers("ct");
  if (mlp_forward_only(nobs, B, actor, anh, W("head_n"), "actor_next")) return -1;
  if (assemble(nobs, nullptr, xt, 0, B, 1)) return -1;
  SampleJob j = make_job(0, B, 1, W("n_eps_next"), xt, od, 0, W("logp_next"));
  if (launch_sample(this, W("head_n"), ad, &j, 1)) return -1;
  return mlp_forward_only(xt, B, tgt, ct, W("qt"), "target");
}

// critics (sac.py:93, 102-110): Q(s, a), loss_launch(gs) seeds dq and publishes its scale in gs, backward, Adam.  The Polyak update fused
// into the Adam launch is safe: nothing behind it reads the targets (sac.py:131 syncs after the actor step; same values either way)
template <class F>
int Engine::sac_critics(F loss_launch) {
  const NetRef crit = net_ref(ORL_NET_CRITIC1, 2);
  Mat obs = W("b_obs2"), act = W("b_act"), xq = W("xq").shared();
  std::vector<Mat> qh = layers("q_h"), dqh = layers("dq_h");
  if (assemble(obs, &act, xq, 0, B, 1)) return -1;
  if (mlp_forward(xq, B, crit, qh, W("q"), "critic")) return -1;
  float* gs_dq = nullptr;
  if (loss_launch(&gs_dq)) return -1;
  return train_net(crit, ORL_NET_CRITIC1, 2, ORL_OPT_CRITIC, xq, qh, B, W("dq"), dqh, "critic.bwd", gs_dq, ORL_NET_CRITIC1_OLD);
}

int Engine::sac_step() {
  // ---- TD target: y = r + gamma (1 - d) (min Q_old(s', a') - alpha logp'), then the critics ----
  if (sac_td_target()) return -1;
  if (sac_critics([&](float** gs) { return td_loss(2, 2, 1, 1, 0, true, gs); })) return -1;
  // ---- actor + temperature against the UPDATED critics (sac.py:112-129; alpha clamped to [0, 1]) ----
  return sac_actor_phase(net_ref(ORL_NET_ACTOR, 1), net_ref(ORL_NET_CRITIC1, 2), 2, true, 3);
}

}  // namespace orl
