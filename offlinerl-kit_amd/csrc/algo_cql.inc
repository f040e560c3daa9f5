// algo_cql.inc — CQL schedule (policy/model_free/cql.py:87-207, sac.py:60-77; oracle/cql.py).  Included by engine.hip.
namespace orl {

static void add_sac_metrics(Engine* e) {
  if (e->cfg.auto_alpha) { e->metric_names.push_back("loss/alpha"); e->metric_names.push_back("alpha"); }
}

// COMBO (combo.py:110-241) is this schedule with Bc = cfg.cql_cons_rows conservative rows starting at batch row c0 and the -w mean Q
// term over the first Br = cfg.cql_real_rows rows; plain CQL: c0 = 0, Bc = Br = B.
static inline void cql_rows(const Engine* e, int& c0, int& Bc, int& Br) {
  c0 = e->cfg.cql_cons_rows > 0 ? e->cfg.cql_cons_row0 : 0;
  Bc = e->cfg.cql_cons_rows > 0 ? e->cfg.cql_cons_rows : e->B;
  Br = e->cfg.cql_real_rows > 0 ? e->cfg.cql_real_rows : e->B;
}

// What sac_actor_phase consumes, for Kc critics (CQL, EDAC, SAC, MCQ, MOBILE).  The noise-slot ORDER is each algorithm's own contract
// (the reference's draw order): the caller lists n_eps_actor in its noise_slots.
void Engine::sac_family_alloc(int Kc) {
  const int A = ad;
  alloc("n_eps_actor", B, A);
  alloc_layers("ah", B); alloc_layers("dah", B); alloc_layers("ca", B, Kc); alloc_layers("dca", B, Kc);
  alloc("head", B, 2 * A); alloc("dhead", B, 2 * A); alloc("xa", B, XP); alloc("logp_a", B, 1);
  alloc("qa", B, 1, Kc); alloc("dqa", B, 1, Kc); alloc("dxa", B, A, Kc);
  // operands / results of the actor phase's row kernels (k_tanh_sample, k_actor_loss, k_head_bwd), members stacked: [Kc][B]
  taps["head"] = {W("head"), B, 2 * A};
  taps["dhead"] = {W("dhead"), B, 2 * A};
  taps["xa"] = {W("xa"), B, XP};
  taps["logp_a"] = {W("logp_a"), B, 1};
  taps["dqa"] = {W("dqa"), (long)B * Kc, 1};
  taps["dxa"] = {W("dxa"), (long)B * Kc, A};
}

// the operands every TD-style critic loss reads the same way (TdLossP, MobileTdP, McqLossP, CqlLossP)
template <class P>
static void td_operands(Engine* e, P& p, bool with_logp_next = true) {
  p.q = e->W("q").z(); p.dq = e->W("dq").p; p.qt = e->W("qt").z();
  p.rew = e->W("b_rew").p; p.term = e->W("b_term").p; p.bt_rs = e->W("b_rew").rs;
  if (with_logp_next) { p.logp_next = e->W("logp_next").p; p.lpn_rs = e->W("logp_next").rs; }
  p.target_q = e->W("target_q").p; p.tq_rs = e->W("target_q").rs;
}

// twin / ensemble TD loss (k_td_loss) of SAC, EDAC and TD3+BC: seeds dq, metric slot(s) from 1; *gs_out: the dynamic scale it publishes
int Engine::td_loss(int Kc, int Kt, int rep, int use_alpha, int sum_over_k, bool with_logp_next, float** gs_out) {
  TdLossP p; memset(&p, 0, sizeof(p));
  td_operands(this, p, with_logp_next);
  p.Kt = Kt; p.use_alpha = use_alpha;
  p.B = B; p.K = Kc; p.rep = rep; p.gamma = cfg.gamma; p.sum_over_k = sum_over_k;
  p.sc = scalars; p.auto_alpha = cfg.auto_alpha; p.fixed_alpha = cfg.alpha; p.m = mp(); p.slot0 = 1;
  p.gs_out = *gs_out = gscale_slot();               // (split precision: the seed kernel publishes the dynamic scale of its backward pass)
  ORL_LAUNCH("td_loss", k_td_loss, dim3(R), dim3(256), p);
  return 0;
}

int Engine::cql_build() {
  int c0, Bc, Br;
  cql_rows(this, c0, Bc, Br);
  const int A = ad, BN = Bc * N, Mc = B + 3 * BN, Bt = cfg.max_q_backup ? B * N : B;
  metric_names = {"loss/actor", "loss/critic1", "loss/critic2"};
  add_sac_metrics(this);
  if (cfg.with_lagrange) { metric_names.push_back("loss/cql_alpha"); metric_names.push_back("cql_alpha"); }
  sac_family_alloc(2);
  alloc("n_eps_next", Bt, A); alloc("n_urand", BN, A);
  alloc("n_eps_pi", BN, A); alloc("n_eps_npi", BN, A);
  noise_slots = {{"n_eps_actor", 0, B}, {"n_eps_next", 0, Bt}, {"n_urand", 1, BN}, {"n_eps_pi", 0, BN}, {"n_eps_npi", 0, BN}};
  alloc_layers("ah2_", 2 * B); alloc_layers("ct", Bt, 2); alloc_layers("ch", Mc, 2); alloc_layers("dch", Mc, 2, L - 1);
  alloc("head2", 2 * B, 2 * A);
  alloc("xt", Bt, XP); alloc("xc", Mc, XP);
  alloc("logp_next", Bt, 1); alloc("logp_pi", BN, 1); alloc("logp_npi", BN, 1);
  alloc("qt", Bt, 1, 2); alloc("q", Mc, 1, 2); alloc("dq", Mc, 1, 2); alloc("target_q", B, 1);
  loss_nblk = std::max(1, std::min(32, (BN + 511) / 512));
  alloc("loss_part", 2L * loss_nblk, 4);
  {
    // one k_prepare launch replaces gather + 5 noise + 6 assemble launches
    Mat o2 = W("b_obs2"), xa = W("xa"), xc = W("xc"), xt = W("xt"), ur = W("n_urand");
    add_prep(o2, 0, 0, B, OP, PS_OBS, 1, 0, od, nullptr, 0, 1, -1);
    add_prep(o2, B, 0, B, OP, PS_NOBS, 1, 0, od, nullptr, 0, 1, -1);
    add_prep(W("b_act"), 0, 0, B, AP, PS_ACT, 1, 0, ad, nullptr, 0, 1, -1);
    add_prep(W("b_rew"), 0, 0, B, 1, PS_REW, 1, 0, 1, nullptr, 0, 1, -1);
    add_prep(W("b_term"), 0, 0, B, 1, PS_TERM, 1, 0, 1, nullptr, 0, 1, -1);
    add_prep(xa, 0, 0, B, od, PS_OBS, 1, 0, od, nullptr, 0, -1, -1);
    add_prep(xc, 0, 0, B, od, PS_OBS, 1, 0, od, nullptr, 0, -1, -1);
    add_prep(xc, 0, od, B, ad, PS_ACT, 1, 0, ad, nullptr, 0, -1, -1);
    add_prep(xc, B, 0, 3 * BN, od, PS_OBS, N, BN, od, nullptr, 0, -1, -1, c0);         // obs (rows c0 ..) repeated N times, three blocks
    add_prep(xc, B + 2 * BN, od, BN, ad, PS_UNIFORM, 1, 0, ad, nullptr, 3, -1, 1);     // random actions (cql.py:138-140)
    add_prep(xc, B + 2 * BN, od, BN, ad, PS_BUF, 1, 0, ad, &ur, 0, -1, 0);             //   teacher-forced: from the host array
    add_prep(xt, 0, 0, Bt, od, PS_NOBS, cfg.max_q_backup ? N : 1, 0, od, nullptr, 0, -1, -1);
    add_prep(W("n_eps_actor"), 0, 0, B, A, PS_NORMAL, 1, 0, A, nullptr, 1, -1, 1);
    add_prep(W("n_eps_next"), 0, 0, Bt, A, PS_NORMAL, 1, 0, A, nullptr, 2, -1, 1);
    add_prep(W("n_eps_pi"), 0, 0, BN, A, PS_NORMAL, 1, 0, A, nullptr, 4, -1, 1);
    add_prep(W("n_eps_npi"), 0, 0, BN, A, PS_NORMAL, 1, 0, A, nullptr, 5, -1, 1);
  }
  tick_folded = fuse_small;      // k_prepare publishes the step counter, k_cql_loss_rows advances it: no k_tick node
  taps["q1"] = {W("q").net(0), B, 1};
  taps["q2"] = {W("q").net(1), B, 1};
  taps["q1_all"] = {W("q").net(0), Mc, 1};
  taps["q2_all"] = {W("q").net(1), Mc, 1};
  taps["q1a"] = {W("qa").net(0), B, 1};
  taps["q2a"] = {W("qa").net(1), B, 1};
  taps["target_q"] = {W("target_q"), B, 1};
  taps["xc"] = {W("xc"), Mc, XP};
  taps["dq1"] = {W("dq").net(0), Mc, 1};
  taps["dq2"] = {W("dq").net(1), Mc, 1};
  // what k_tanh_sample (phase T) and k_cql_loss_rows read
  taps["head2"] = {W("head2"), 2 * B, 2 * A};
  taps["xt"] = {W("xt"), Bt, XP};
  taps["qt1"] = {W("qt").net(0), Bt, 1};
  taps["qt2"] = {W("qt").net(1), Bt, 1};
  taps["logp_next"] = {W("logp_next"), Bt, 1};
  taps["logp_pi"] = {W("logp_pi"), BN, 1};
  taps["logp_npi"] = {W("logp_npi"), BN, 1};
  return 0;
}

// SAC-style actor update shared by CQL and EDAC: a ~ pi(s), L = mean(alpha logp - min_k Q_k(s,a)), alpha step.
int Engine::sac_actor_phase(const NetRef& actor, const NetRef& crit, int Kc, bool clamp_alpha01, int slot_alpha_loss) {
  const int A = ad;
  Mat obs = W("b_obs2");
  std::vector<Mat> ah = layers("ah"), dah = layers("dah"), ca = layers("ca"), dca = layers("dca");
  Mat xa = W("xa").shared();
  // a ~ pi(s): the one-launch forward samples in its epilogue when it applies (few batched rows); otherwise a k_tanh_sample launch.
  // (the observation columns of xa are written before this point: k_prepare, or the assemble launch of engines without a job table)
  if (prep.empty() && assemble(obs, nullptr, xa, 0, B, 1)) return -1;
  SampleJob j = make_job(0, B, 1, W("n_eps_actor"), xa, od, 0, W("logp_a"));
  bool sampled = false;
  if (mlp_forward(obs, B, actor, ah, W("head"), "actor", &j, 1, &sampled)) return -1;
  if (!sampled && launch_sample(this, W("head"), A, &j, 1)) return -1;
  // Q_k(s, pi(s)) and, where the one-launch forward + backward applies (two 256-wide layers, few batched rows), dQ_k / da for a unit seed
  // in the same launch: the loss kernel below then only weighs the two gradients (-1/B on the smaller Q, cql.py:93-98)
  Mat dxa = W("dxa");
  bool qg = false;
  if (mlp_qgrad(xa, B, crit, W("qa"), dxa, od, A, "critic_a.qgrad", &qg)) return -1;
  if (!qg && mlp_forward(xa, B, crit, ca, W("qa"), "critic_a")) return -1;
  // actor loss + temperature step + head backward + actor backward as ONE launch when the unit-seed critic gradients exist and the actor is
  // two 256-wide layers on few batched rows (small_bwd.h): one split-K slab of every actor tensor per 32-row group
  if (qg && fuse_small && L == 2 && actor.lay->H[0] == SB_N && actor.lay->H[1] == SB_N && !vals_dead.count(ah[0].p) && !vals_dead.count(ah[1].p) &&
      B / SB_ROWS <= max_slab) {
    const NetLayout& al = *actor.lay;
    SmallABwdP w; memset(&w, 0, sizeof(w));
    w.X = obs.p; w.x_s0 = obs.rs; w.x_pitch = obs.pitch; w.in0 = al.layer_in(0);
    w.H0 = ah[0].p; w.h0_s0 = ah[0].rs; w.H1 = ah[1].p; w.h1_s0 = ah[1].rs;
    w.head = W("head").p; w.head_s0 = W("head").rs;
    w.eps = W("n_eps_actor").p; w.eps_s0 = W("n_eps_actor").rs;
    w.xa = xa.p; w.xa_s0 = xa.rs; w.xa_pitch = xa.pitch; w.xa_col = od;
    w.logp = W("logp_a").p; w.logp_s0 = W("logp_a").rs;
    w.qa = W("qa").z();
    w.ga = dxa.z(); w.ga_pitch = dxa.pitch; w.K = Kc;
    w.W1 = actor.base + al.w_off[1]; w.w1_s0 = actor.rs;
    w.Wh = actor.base + al.w_off[2]; w.wh_s0 = actor.rs;
    w.out = grads + actor.g_off; w.o_s0 = (long)max_slab * P_train; w.o_ks = P_train;
    w.off_w0 = al.w_off[0]; w.off_b0 = al.b_off[0]; w.off_w1 = al.w_off[1]; w.off_b1 = al.b_off[1]; w.off_wh = al.w_off[2]; w.off_bh = al.b_off[2];
    w.sc = scalars; w.hy = hyper; w.auto_alpha = cfg.auto_alpha; w.fixed_alpha = cfg.alpha;
    w.target_entropy = cfg.target_entropy; w.clamp_alpha01 = clamp_alpha01 ? 1 : 0;
    w.b1 = cfg.adam_beta1; w.b2 = cfg.adam_beta2; w.adam_eps = cfg.adam_eps; w.gstep = gstep;
    w.metrics_last = metrics_last; w.metrics_sum = metrics_sum; w.nm = (int)metric_names.size();
    w.m_actor = 0; w.m_alpha_loss = slot_alpha_loss; w.m_alpha = slot_alpha_loss + 1;
    w.part = aloss_part; w.ticket = cql_ticket;
    w.M = B; w.A = A; w.f32 = ws_f32();
    w.lab_clk = lab_clk(0);      // (16 stamps behind the partial sums; written by lab builds only)
    if (al.out_dim == 2 * A && small_abwd_supported(w)) {
      watch_range(ah[0], B, SB_N, 1, "actor.bwd");
      if (timed("small_abwd", "actor.bwd_fused", false, 2.0 * B * (double)R * (2.0 * SB_N * SB_N + 2.0 * SB_N * 2 * A + (double)SB_N * (w.in0 + 1)),
                   4.0 * R * (B * (double)(2 * SB_N + w.in0 + 6 * A + 4) + (double)SB_N * SB_N + (B / SB_ROWS) * (double)al.size),
                   [&] { return launch_small_abwd(w, R, stream); })) return -1;
      const std::vector<int> ks(L + 1, B / SB_ROWS);
      return adam(ORL_NET_ACTOR, 1, ORL_OPT_ACTOR, make_segs(al, ks, ks), -1);
    }
  }
  {
    ActorLossP p; memset(&p, 0, sizeof(p));
    p.qa = W("qa").z(); p.dqa = W("dqa").p;
    p.logp = W("logp_a").p; p.logp_rs = W("logp_a").rs; p.B = B; p.K = Kc;
    p.sc = scalars; p.hy = hyper; p.auto_alpha = cfg.auto_alpha; p.fixed_alpha = cfg.alpha;
    p.target_entropy = cfg.target_entropy; p.clamp_alpha01 = clamp_alpha01 ? 1 : 0;
    p.b1 = cfg.adam_beta1; p.b2 = cfg.adam_beta2; p.eps = cfg.adam_eps; p.gstep = gstep;
    p.metrics_last = metrics_last; p.metrics_sum = metrics_sum; p.nm = (int)metric_names.size();
    p.m_actor = 0; p.m_alpha_loss = slot_alpha_loss; p.m_alpha = slot_alpha_loss + 1;
    prof_begin("actor_loss", 0);
    hipLaunchKernelGGL(k_actor_loss, dim3(R), dim3(256), 0, stream, p);
    prof_end();
  }
  // (split precision: the seed dqa holds -1/B or 0 -- its scale is a constant of the engine; dhead's comes from k_head_bwd itself when
  // the batch is one workgroup)
  const InputGrad da{od, A, &dxa};
  if (!qg && mlp_backward(this, crit, xa, ca, B, W("dqa"), dca, false, &da, "critic_a.bwd", nullptr, split_scales() ? gscale_inv_b : nullptr)) return -1;
  float* gs_head = (split_scales() && B <= 256) ? gscale_slot() : nullptr;
  {
    HeadBwdP p; memset(&p, 0, sizeof(p));
    p.gs_out = gs_head;
    p.dxa = dxa.z(); p.dxa_pitch = A; p.K = Kc;
    if (qg) p.dqa = W("dqa").z();
    p.head = W("head").p; p.head_rs = W("head").rs; p.eps = W("n_eps_actor").p; p.eps_rs = W("n_eps_actor").rs;
    p.xa = xa.p; p.xa_rs = xa.rs; p.XP = XP; p.od = od; p.dhead = W("dhead").p; p.dhead_rs = W("dhead").rs;
    p.sc = scalars; p.auto_alpha = cfg.auto_alpha; p.fixed_alpha = cfg.alpha; p.B = B; p.A = A;
    prof_begin("head_bwd", 0);
    hipLaunchKernelGGL(k_head_bwd, dim3((B + 255) / 256, R), dim3(256), 0, stream, p);
    prof_end();
  }
  return train_net(actor, ORL_NET_ACTOR, 1, ORL_OPT_ACTOR, obs, ah, B, W("dhead"), dah, "actor.bwd", gs_head);
}

int Engine::cql_step() {
  int c0, Bc, Br;
  cql_rows(this, c0, Bc, Br);
  const int A = ad, BN = Bc * N, Mc = B + 3 * BN, Bt = cfg.max_q_backup ? B * N : B;
  const NetRef actor = net_ref(ORL_NET_ACTOR, 1), crit = net_ref(ORL_NET_CRITIC1, 2), tgt = net_ref(ORL_NET_CRITIC1_OLD, 2);
  Mat obs2 = W("b_obs2");
  std::vector<Mat> ah2 = layers("ah2_"), ct = layers("ct"), ch = layers("ch"), dch = layers("dch");
  Mat xt = W("xt").shared(), xc = W("xc").shared();

  // ---------------- phase A: actor + temperature (cql.py:92-106) ----------------
  if (sac_actor_phase(actor, crit, 2, false, 3)) return -1;

  // ---------------- phase T: targets + repeated-action sampling with the UPDATED actor ----------------
  // critic input rows (written by k_prepare): [0,B) (obs, a_data) ; [B,B+BN) (obs rep, a_pi) ; next BN (obs rep, a_next_pi) ;
  // last BN (obs rep, u_rand).  The sampled actions are filled in by the actor pass's epilogue (or the k_tanh_sample launch behind it).
  {
    SampleJob jobs[3] = {
        make_job(B, Bt, cfg.max_q_backup ? N : 1, W("n_eps_next"), xt, od, 0, W("logp_next")),  // next actions (cql.py:108-130)
        make_job(c0, BN, N, W("n_eps_pi"), xc, od, B, W("logp_pi")),                            // a ~ pi(tmp_obss)      (:149)
        make_job(B + c0, BN, N, W("n_eps_npi"), xc, od, B + BN, W("logp_npi")),                 // a ~ pi(tmp_next_obss) (:150)
    };
    bool sampled = false;
    if (mlp_forward_only(obs2, 2 * B, actor, ah2, W("head2"), "actor2", jobs, 3, &sampled)) return -1;
    if (!sampled && launch_sample(this, W("head2"), A, jobs, 3)) return -1;
  }
  if (mlp_forward_only(xt, Bt, tgt, ct, W("qt"), "target")) return -1;

  // ---------------- phase C: critics (cql.py:132-190) ----------------
  if (mlp_forward(xc, Mc, crit, ch, W("q"), "critic")) return -1;
  float* gs_dq = nullptr;
  {
    CqlLossP p; memset(&p, 0, sizeof(p));
    td_operands(this, p);
    p.logp_pi = W("logp_pi").p; p.logp_npi = W("logp_npi").p; p.lpp_rs = W("logp_pi").rs;
    p.B = B; p.N = N; p.A = A; p.Bc = Bc; p.Br = Br; p.gamma = cfg.gamma; p.w = cfg.cql_weight; p.T = cfg.temperature; p.thr = cfg.lagrange_threshold;
    p.max_q_backup = cfg.max_q_backup; p.det_backup = cfg.deterministic_backup; p.with_lagrange = cfg.with_lagrange;
    p.auto_alpha = cfg.auto_alpha; p.fixed_alpha = cfg.alpha;
    p.sc = scalars; p.hy = hyper; p.b1 = cfg.adam_beta1; p.b2 = cfg.adam_beta2; p.eps = cfg.adam_eps; p.gstep = gstep;
    p.metrics_last = metrics_last; p.metrics_sum = metrics_sum; p.nm = (int)metric_names.size();
    p.m_c1 = 1; p.m_c2 = 2; p.m_cqla_loss = cfg.auto_alpha ? 5 : 3; p.m_cqla = cfg.auto_alpha ? 6 : 4;
    p.part = W("loss_part").p; p.nblk = loss_nblk; p.ticket = cql_ticket;
    gs_dq = gscale_slot();
    p.gs_out = gs_dq;
    p.gstep_next = tick_folded ? gstep_pre : nullptr;
    ORL_LAUNCH("cql_loss", k_cql_loss_rows, dim3(loss_nblk, 2, R), dim3(256), p);      // (the last workgroup of a run to arrive finishes it)
  }
  return train_net(crit, ORL_NET_CRITIC1, 2, ORL_OPT_CRITIC, xc, ch, Mc, W("dq"), dch, "critic.bwd", gs_dq, ORL_NET_CRITIC1_OLD);
}

}  // namespace orl
