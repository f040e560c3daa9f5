// algo_mcq.inc — MCQ schedule (policy/model_free/mcq.py:48-126 over sac.py; behaviour policy nets/vae.py:8-66; oracle/mcq.py).
// Order of the reference: VAE step -> critics (TD on the batch + pseudo-targets max_n min_c Q_old(s, a_n) for actions the policy
// proposes on [s; s'], a_n decoded by the UPDATED VAE) -> actor / temperature against the updated critics -> Polyak.  Included by engine.hip.
namespace orl {

int Engine::mcq_build() {
  const int A = ad, Z = cfg.vae_latent, VH = cfg.vae_hidden, B2 = 2 * B, BN2 = 2 * B * N;
  const int DP = (od + Z + 3) & ~3;                       // decoder input pitch (obs | z)
  metric_names = {"loss/actor", "loss/critic1", "loss/critic2", "loss/behavior_policy"};
  add_sac_metrics(this);
  alloc("n_eps_vae", B, Z); alloc("n_eps_next", B, A); alloc("n_z_ood", BN2, Z); alloc("n_eps_ood", B2, A);
  sac_family_alloc(2);
  noise_slots = {{"n_eps_vae", 0, B, Z}, {"n_eps_next", 0, B, A}, {"n_z_ood", 0, BN2, Z}, {"n_eps_ood", 0, B2, A}, {"n_eps_actor", 0, B, A}};
  alloc_layers("ah2_", B2); alloc_layers("ct", B, 2); alloc_layers("cto", BN2, 2);
  alloc_layers("q_h", 3 * B, 2); alloc_layers("dq_h", 3 * B, 2);
  // (the VAE's two hidden layers are vae_hidden wide, whatever the policy nets are)
  alloc_layers("eh", B, 1, 2, VH); alloc_layers("deh", B, 1, 2, VH); alloc_layers("dh", B, 1, 2, VH); alloc_layers("ddh", B, 1, 2, VH);
  alloc_layers("doh", BN2, 1, 2, VH);
  alloc("ehead", B, 2 * Z); alloc("dehead", B, 2 * Z); alloc("vstd", B, Z); alloc("xd", B, DP); alloc("dxd", B, Z);
  alloc("m3", B, A); alloc("dm3", B, A); alloc("xdo", BN2, DP); alloc("m3o", BN2, A);
  alloc("head2", B2, 2 * A);
  alloc("xt", B, XP); alloc("xto", BN2, XP); alloc("xq3", 3 * B, XP);
  alloc("logp_next", B, 1); alloc("logp_ood", B2, 1);
  alloc("qt", B, 1, 2); alloc("qto", BN2, 1, 2); alloc("q", 3 * B, 1, 2); alloc("dq", 3 * B, 1, 2);
  alloc("target_q", B, 1); alloc("target_ood", B2, 1);
  taps["q1"] = {W("q").net(0), B, 1};
  taps["q1_ood"] = {W("q").net(0).rows(B), B2, 1};
  taps["q1a"] = {W("qa").net(0), B, 1};
  taps["target_q"] = {W("target_q"), B, 1};
  taps["target_ood"] = {W("target_ood"), B2, 1};
  taps["sampled_actions"] = {W("xto").cols(od), BN2, A};
  // operands / results of k_vae_latent, k_vae_loss, k_vae_head_bwd, k_clamp_latent, the OOD k_assemble / k_det_action and k_mcq_loss
  // (both nets stacked: [2][rows]).  Every workspace is its own allocation and no later launch of the step writes one of them.
  taps["ehead"] = {W("ehead"), B, 2 * Z};
  taps["vstd"] = {W("vstd"), B, Z};
  taps["xd"] = {W("xd"), B, DP};
  taps["m3"] = {W("m3"), B, A};
  taps["dm3"] = {W("dm3"), B, A};
  taps["dxd"] = {W("dxd"), B, Z};
  taps["dehead"] = {W("dehead"), B, 2 * Z};
  taps["xdo"] = {W("xdo"), BN2, DP};
  taps["m3o"] = {W("m3o"), BN2, A};
  taps["qt"] = {W("qt"), 2L * B, 1};
  taps["qto"] = {W("qto"), 2L * BN2, 1};
  taps["logp_next"] = {W("logp_next"), B, 1};
  taps["q"] = {W("q"), 6L * B, 1};
  taps["dq"] = {W("dq"), 6L * B, 1};
  return 0;
}

int Engine::mcq_step() {
  const int A = ad, Z = cfg.vae_latent, B2 = 2 * B, BN2 = 2 * B * N;
  const NetRef actor = net_ref(ORL_NET_ACTOR, 1), crit = net_ref(ORL_NET_CRITIC1, 2), tgt = net_ref(ORL_NET_CRITIC1_OLD, 2),
               enc = net_ref(ORL_NET_VAE_ENC, 1), dec = net_ref(ORL_NET_VAE_DEC, 1);
  Mat obs = W("b_obs2"), nobs = W("b_obs2").rows(B), obs2 = W("b_obs2"), act = W("b_act");
  std::vector<Mat> ah2 = layers("ah2_"), ct = layers("ct"), cto = layers("cto"), qh = layers("q_h"), dqh = layers("dq_h");
  std::vector<Mat> eh = layers("eh"), deh = layers("deh"), dh = layers("dh"), ddh = layers("ddh"), doh = layers("doh");
  Mat xq3 = W("xq3").shared(), xq = xq3, xs = W("xq3").shared().rows(B), xt = W("xt").shared(), xto = W("xto").shared();
  Mat xd = W("xd"), xdo = W("xdo");
  const MetricsP m{metrics_last, metrics_sum, (int)metric_names.size()};

  // ---- behaviour policy (mcq.py:52-60; vae.py:36-53) ----
  if (assemble(obs, &act, xq, 0, B, 1)) return -1;                       // (obs | act): encoder input AND the critics' in-distribution rows
  if (mlp_forward(xq, B, enc, eh, W("ehead"), "vae.enc")) return -1;
  {
    AssembleP a; memset(&a, 0, sizeof(a));                                // obs columns of the decoder input (pitch DP)
    a.obs = obs.p; a.obs_rs = obs.rs; a.OP = obs.pitch; a.od = od; a.ad = 0; a.X = xd.p; a.x_rs = xd.rs; a.XP = xd.pitch; a.rows = B; a.rep = 1;
    ORL_LAUNCH("vae.assemble", k_assemble, dim3((B + 255) / 256, R), dim3(256), a);
    VaeLatentP p; memset(&p, 0, sizeof(p));
    p.ehead = W("ehead").p; p.eh_rs = W("ehead").rs; p.eps = W("n_eps_vae").p; p.eps_rs = W("n_eps_vae").rs;
    p.xd = xd.p; p.xd_rs = xd.rs; p.xd_pitch = xd.pitch; p.od = od; p.stdv = W("vstd").p; p.std_rs = W("vstd").rs; p.B = B; p.Z = Z;
    ORL_LAUNCH("vae.latent", k_vae_latent, dim3((B * Z + 255) / 256, R), dim3(256), p);
  }
  if (mlp_forward(xd, B, dec, dh, W("m3"), "vae.dec")) return -1;
  {
    VaeLossP p; memset(&p, 0, sizeof(p));
    p.m3 = W("m3").p; p.m3_rs = W("m3").rs; p.act = act.p; p.act_rs = act.rs; p.apitch = act.pitch;
    p.ehead = W("ehead").p; p.eh_rs = W("ehead").rs; p.stdv = W("vstd").p; p.std_rs = W("vstd").rs; p.dm3 = W("dm3").p;
    p.B = B; p.A = A; p.Z = Z; p.max_action = cfg.max_action; p.m = m; p.slot = 3;
    ORL_LAUNCH("vae.loss", k_vae_loss, dim3(R), dim3(256), p);
  }
  BwdOut bd;
  Mat dxd = W("dxd");
  const InputGrad dz{od, Z, &dxd};
  if (mlp_backward(this, dec, xd, dh, B, W("dm3"), ddh, true, &dz, "vae.dec.bwd", &bd)) return -1;
  {
    VaeHeadBwdP p; memset(&p, 0, sizeof(p));
    p.dz = dxd.p; p.dz_rs = dxd.rs; p.ehead = W("ehead").p; p.eh_rs = W("ehead").rs; p.stdv = W("vstd").p; p.std_rs = W("vstd").rs;
    p.eps = W("n_eps_vae").p; p.eps_rs = W("n_eps_vae").rs; p.dehead = W("dehead").p; p.B = B; p.Z = Z;
    ORL_LAUNCH("vae.head_bwd", k_vae_head_bwd, dim3((B * Z + 255) / 256, R), dim3(256), p);
  }
  if (train_net(enc, ORL_NET_VAE_ENC, 1, ORL_OPT_VAE, xq, eh, B, W("dehead"), deh, "vae.enc.bwd", nullptr)) return -1;
  if (adam(ORL_NET_VAE_DEC, 1, ORL_OPT_VAE, make_segs(*dec.lay, bd.ks, bd.ks), -1)) return -1;

  // ---- one actor forward on [s; s'] serves the TD target's a' ~ pi(s') and the OOD actions pi([s; s']) (mcq.py:63, 80) ----
  if (mlp_forward_only(obs2, B2, actor, ah2, W("head2"), "actor2")) return -1;
  if (assemble(nobs, nullptr, xt, 0, B, 1)) return -1;
  if (assemble(obs2, nullptr, xs, 0, B2, 1)) return -1;
  {
    SampleJob jobs[2] = {
        make_job(B, B, 1, W("n_eps_next"), xt, od, 0, W("logp_next")),
        make_job(0, B2, 1, W("n_eps_ood"), xs, od, 0, W("logp_ood")),
    };
    if (launch_sample(this, W("head2"), A, jobs, 2)) return -1;
  }
  if (mlp_forward_only(xt, B, tgt, ct, W("qt"), "target")) return -1;
  // ---- pseudo-targets: N actions per state of [s; s'] decoded by the updated VAE from clamped latents (mcq.py:74-79) ----
  {
    AssembleP a; memset(&a, 0, sizeof(a));
    a.obs = obs2.p; a.obs_rs = obs2.rs; a.OP = obs2.pitch; a.od = od; a.ad = 0; a.X = xdo.p; a.x_rs = xdo.rs; a.XP = xdo.pitch; a.rows = BN2; a.rep = N;
    ORL_LAUNCH("ood.assemble", k_assemble, dim3((BN2 + 255) / 256, R), dim3(256), a);
    ORL_LAUNCH("ood.latent", k_clamp_latent, dim3((unsigned)(((long)BN2 * Z + 255) / 256), R), dim3(256), (const float*)W("n_z_ood").p, W("n_z_ood").rs,
               xdo.p, xdo.rs, xdo.pitch, od, BN2, Z);
  }
  if (mlp_forward_only(xdo, BN2, dec, doh, W("m3o"), "vae.decode")) return -1;
  if (assemble(obs2, nullptr, xto, 0, BN2, N)) return -1;
  {
    DetActP p; memset(&p, 0, sizeof(p));
    p.mraw = W("m3o").p; p.mraw_rs = W("m3o").rs; p.X = xto.p; p.x_rs = xto.rs; p.XP = XP; p.od = od; p.B = BN2; p.A = A; p.max_action = cfg.max_action;
    ORL_LAUNCH("ood.action", k_det_action, dim3((unsigned)(((long)BN2 * A + 255) / 256), R), dim3(256), p);
  }
  if (mlp_forward_only(xto, BN2, tgt, cto, W("qto"), "target_ood")) return -1;
  // ---- critics on [ (s, a) ; ([s; s'], a_ood) ] (mcq.py:68-94) ----
  if (mlp_forward(xq3, 3 * B, crit, qh, W("q"), "critic")) return -1;
  {
    McqLossP p; memset(&p, 0, sizeof(p));
    td_operands(this, p);
    p.qto = W("qto").z(); p.target_ood = W("target_ood").p; p.to_rs = W("target_ood").rs;
    p.B = B; p.N = N; p.gamma = cfg.gamma; p.lambda = cfg.mcq_lambda; p.sc = scalars; p.auto_alpha = cfg.auto_alpha; p.fixed_alpha = cfg.alpha;
    p.m = m; p.slot0 = 1;
    ORL_LAUNCH("mcq_loss", k_mcq_loss, dim3(R), dim3(256), p);
  }
  if (train_net(crit, ORL_NET_CRITIC1, 2, ORL_OPT_CRITIC, xq3, qh, 3 * B, W("dq"), dqh, "critic.bwd", nullptr, ORL_NET_CRITIC1_OLD)) return -1;
  // ---- actor + temperature against the UPDATED critics (mcq.py:96-111; alpha clamped to [0, 1]) ----
  return sac_actor_phase(actor, crit, 2, true, 4);
}

}  // namespace orl
