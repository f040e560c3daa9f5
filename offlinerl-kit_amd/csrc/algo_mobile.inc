// algo_mobile.inc — MOBILE schedule (policy/model_based/mobile.py:130-196; tests/mobile_oracle.py): the SAC update of algo_sac.inc with
// the model-Bellman-inconsistency penalty in the TD target.  The penalty pass forwards the actor and the two TARGET critics on the
// S * E * B next-state samples orl_engine_set_next_samples handed over (orl_dynsample_next's row order) and reduces min(Q1, Q2) to
// mean over samples -> unbiased std over elites per batch row (k_lcb_penalty).  Then: critics first (target clamped at 0, one loss over
// both critics), the actor against the UPDATED critics, temperature clamped to [0, 1], Polyak with the critics' Adam.  Draw order of the
// reference: eps_lcb (compute_lcb's actforward), eps_next, eps_actor.  mobile_loop (the body of orl_mobile_learn_n) runs whole steps as one
// device loop: batch draw, noise, the dynamics' samples written into the penalty pass's operands, the step.  Included by engine.hip.
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
  sac_alloc();
  alloc("n_eps_lcb", M, A);
  noise_slots = {{"n_eps_lcb", 0, M}, {"n_eps_next", 0, B}, {"n_eps_actor", 0, B}};      // mobile.py:153 (compute_lcb), :156, :170
  alloc_layers("al_h", M); alloc_layers("cl_h", M, 2);                                  // the penalty pass: actor / target critics on M rows
  alloc("head_l", M, 2 * A); alloc("xs", M, OP); alloc("xl", M, XP); alloc("logp_l", M, 1);
  alloc("ql", M, 1, 2); alloc("lcb_q", M, 1); alloc("penalty", B, 1);
  alloc("samples_in", M, od);                                                            // a host array of orl_engine_set_next_samples lands here
  taps["penalty"] = {W("penalty"), B, 1};
  taps["lcb_q"] = {W("lcb_q"), M, 1};
  // the penalty pass's own operands: what k_mobile_assemble wrote (the action columns of xl are the sampling job's) and what
  // k_lcb_penalty read; no launch behind the penalty pass writes any of them
  taps["ql1"] = {W("ql").net(0), M, 1};
  taps["ql2"] = {W("ql").net(1), M, 1};
  taps["xs"] = {W("xs"), M, OP};
  taps["xl"] = {W("xl"), M, XP};
  taps["logp_l"] = {W("logp_l"), M, 1};
  return 0;
}

// compute_lcb (mobile.py:130-142) on the pending samples; real_rows leading rows of the penalty are zeroed.  rows_in_place: the
// samples already stand in xs and in the observation columns of xl with zeroed pads (orl::dynsample_enqueue wrote them): no assemble launch
int Engine::mobile_penalty(int real_rows, bool rows_in_place) {
  const int A = ad, S = cfg.mobile_num_samples, E = cfg.mobile_num_elites, M = S * E * B;
  const NetRef actor = net_ref(ORL_NET_ACTOR, 1), tgt = net_ref(ORL_NET_CRITIC1_OLD, 2);
  std::vector<Mat> alh = layers("al_h"), clh = layers("cl_h");
  Mat xs = W("xs"), xl = W("xl").shared();
  if (!rows_in_place) {
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
    p.ql = W("ql").z();
    p.qmin = W("lcb_q").p; p.qm_rs = W("lcb_q").rs;
    p.pen = W("penalty").p; p.pen_rs = W("penalty").rs;
    p.B = B; p.S = S; p.E = E; p.real_rows = real_rows; p.health = health;
    ORL_LAUNCH("lcb.penalty", k_lcb_penalty, dim3((B + 255) / 256, R), dim3(256), p);
  }
  return 0;
}

int Engine::mobile_step() {
  // ---- penalty pass (mobile.py:153-154) ----
  if (mobile_penalty(cfg.mobile_real_rows, mobile_rows_in_place)) return -1;
  // ---- TD target (mobile.py:156-162): a' ~ pi(s'), min Q_old(s', a') [- alpha logp'], then the critics (mobile.py:151, 164-167):
  // critics_optim is ONE Adam over both critics with the Polyak update fused (nothing below reads the targets, mobile.py:185) ----
  if (sac_td_target()) return -1;
  const auto loss = [&](float** gs) {
    MobileTdP p; memset(&p, 0, sizeof(p));
    td_operands(this, p);
    p.use_alpha = cfg.deterministic_backup ? 0 : 1;
    p.pen = W("penalty").p; p.pen_rs = W("penalty").rs; p.pen_coef = cfg.penalty_coef;
    p.B = B; p.gamma = cfg.gamma;
    p.sc = scalars; p.auto_alpha = cfg.auto_alpha; p.fixed_alpha = cfg.alpha; p.m = mp(); p.slot = 1;
    p.gs_out = *gs = gscale_slot();
    ORL_LAUNCH("td_loss", k_mobile_td_loss, dim3(R), dim3(256), p);
    return 0;
  };
  if (sac_critics(loss)) return -1;
  // ---- actor + temperature against the UPDATED critics (mobile.py:169-183; alpha clamped to [0, 1]) ----
  return sac_actor_phase(net_ref(ORL_NET_ACTOR, 1), net_ref(ORL_NET_CRITIC1, 2), 2, true, 2);
}

// n_steps whole MOBILE steps without coming back to the host (orl_mobile_learn_n has refused what it refuses): every launch of the engine
// and of the dynamics' sample call on the engine's stream, one synchronisation at the end.  Step i: the batch draw and the noise slots of
// orl_learn_n (k_gather on the dataset and the model ring, k_noise at the step counter), the dynamics' samples of the drawn rows written
// into xs / xl (dynsample_enqueue), mobile_step without its assemble launch.
int Engine::mobile_loop(orl_dynamics* d, const DynSampleInfo& di, int n_steps, float* metrics_mean, float* elapsed_ms) {
  const char* F = "orl_mobile_learn_n";
  if (dynstep_loop_begin(d, B)) return -1;      // (grows the step workspaces on the dynamics' own stream: before the lease)
  ORL_HIP(hipMemsetAsync(metrics_sum, 0, sizeof(float) * R * nm, stream));
  // whatever the dynamics' own stream still holds comes first; from here to the end every launch of both objects is on the engine's stream
  LoopScope loop;
  if (loop_begin(loop, {di.stream})) return -1;
  DynStreamLease lease(d, stream);
  const Mat o2 = W("b_obs2"), act = W("b_act"), xs = W("xs"), xl = W("xl");
  DynSampleRows rows;
  memset(&rows, 0, sizeof(rows));
  rows.obs = o2.p; rows.obs_rs = o2.rs; rows.obs_pitch = o2.pitch;
  rows.act = act.p; rows.act_rs = act.rs; rows.act_pitch = act.pitch;
  rows.n = B; rows.num_samples = cfg.mobile_num_samples;
  rows.xs = xs.p; rows.xs_rs = xs.rs; rows.OP = xs.pitch;
  rows.xl = xl.p; rows.xl_rs = xl.rs; rows.XP = xl.pitch;
  long done = 0;
  const auto body = [&]() -> int {
    for (int s = 0; s < n_steps; ++s) {
      if (enqueue_inputs()) return -1;
      if (dynsample_enqueue(d, rows, F)) return -1;
      if (enqueue_step(0)) return -1;
      step_host++;
      ++done;
    }
    return 0;
  };
  mobile_rows_in_place = true;
  const int rc = loop.end(body(), F, elapsed_ms);      // the one host synchronisation (also on an error path: the launches made so far ran)
  mobile_rows_in_place = false;
  if (rc) return -1;
  return finish(metrics_sum, (float)n_steps, metrics_mean, done);      // (a non-finite metric of ANY of the steps stays in its sum)
}

}  // namespace orl
