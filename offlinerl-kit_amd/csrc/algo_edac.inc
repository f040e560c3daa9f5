// algo_edac.inc — EDAC schedule (policy/model_free/edac.py:88-166; oracle/edac.py).  K ensemble critics in the
// EnsembleLinear layout, batched through blockIdx.z.  The gradient-diversity term's double backward is restated
// as: unit-seed backward (deltas) -> per-row gamma kernel -> masked forward sweep (t_l) -> extra wgrad slabs.
namespace orl {

int Engine::edac_build() {
  const int A = ad, Kc = cfg.num_critics;
  const int rep = cfg.max_q_backup ? 10 : 1, Bt = B * rep;   // edac.py:116 hard-codes 10 repeats
  metric_names = {"loss/actor", "loss/critics"};
  add_sac_metrics(this);
  sac_family_alloc(Kc);
  alloc("n_eps_next", Bt, A);
  noise_slots = {{"n_eps_actor", 0, B}, {"n_eps_next", 0, Bt}};
  alloc_layers("ah2_", B); alloc_layers("ct", Bt, Kc); alloc_layers("ch", B, Kc); alloc_layers("tt", B, Kc);
  alloc_layers("dch", B, Kc, L - 1); alloc_layers("dd", B, Kc, L - 1);
  alloc("head2", B, 2 * A);
  alloc("xt", Bt, XP); alloc("xq", B, XP);
  alloc("logp_next", Bt, 1);
  alloc("qt", Bt, 1, Kc); alloc("q", B, 1, Kc); alloc("dq", B, 1, Kc); alloc("target_q", B, 1);
  alloc("g", B, A, Kc); alloc("gamma", B, A, Kc);
  taps["qs"] = {W("q"), (long)B * Kc, 1};
  taps["qas"] = {W("qa"), (long)B * Kc, 1};
  taps["target_q"] = {W("target_q"), B, 1};
  taps["g"] = {W("g"), (long)B * Kc, A};
  taps["gamma"] = {W("gamma"), (long)B * Kc, A};
  taps["xq"] = {W("xq"), B, XP};                     // critic input rows (obs | act) of the TD / diversity passes
  taps["dqs"] = {W("dq"), (long)B * Kc, 1};          // dL_TD/dq of every member
  // what k_tanh_sample (target actions) and k_td_loss read: [Kc][Bt] target Q-values, Bt = B * rep rows
  taps["head2"] = {W("head2"), B, 2 * A};
  taps["xt"] = {W("xt"), Bt, XP};
  taps["qts"] = {W("qt"), (long)Bt * Kc, 1};
  taps["logp_next"] = {W("logp_next"), Bt, 1};
  // the first step of the diversity sweep: t_0 of every member, the stored first hidden activation (the mask source when no packed bits are
  // live) and, as a host tap, which launch made t_0 in the last step: {1 = k_edac_t0 / 0 = tiled GEMM with E_MASK, 1 = packed mask bits /
  // 0 = stored values}; {-1, -1} while no sweep has run (eta = 0)
  taps["tt0"] = {W("tt0"), (long)B * Kc, cfg.hidden[0]};
  taps["ch0"] = {W("ch0"), (long)B * Kc, cfg.hidden[0]};
  host_taps["edac.t0_path"] = {-1.f, -1.f};
  return 0;
}

int Engine::edac_step() {
  const int A = ad, Kc = cfg.num_critics;
  const int rep = cfg.max_q_backup ? 10 : 1, Bt = B * rep;
  const NetRef actor = net_ref(ORL_NET_ACTOR, 1), crit = net_ref(ORL_NET_CRITIC1, Kc), tgt = net_ref(ORL_NET_CRITIC1_OLD, Kc);
  Mat obs = W("b_obs2"), nobs = W("b_obs2").rows(B), act = W("b_act");
  std::vector<Mat> ah2 = layers("ah2_"), ct = layers("ct"), ch = layers("ch"), dch = layers("dch"), dd = layers("dd"), tt = layers("tt");
  Mat xt = W("xt").shared(), xq = W("xq").shared();
  const MetricsP m{metrics_last, metrics_sum, (int)metric_names.size()};

  // ---- actor + temperature (edac.py:96-110; alpha clamped to [0,1]) ----
  if (sac_actor_phase(actor, crit, Kc, true, 2)) return -1;

  // ---- target with the UPDATED actor (edac.py:112-131) ----
  if (mlp_forward_only(nobs, B, actor, ah2, W("head2"), "actor2")) return -1;
  if (assemble(nobs, nullptr, xt, 0, Bt, rep)) return -1;
  {
    SampleJob j = make_job(0, Bt, rep, W("n_eps_next"), xt, od, 0, W("logp_next"));
    if (launch_sample(this, W("head2"), A, &j, 1)) return -1;
  }
  if (mlp_forward_only(xt, Bt, tgt, ct, W("qt"), "target")) return -1;

  // ---- critics: TD part (edac.py:133-134) ----
  if (assemble(obs, &act, xq, 0, B, 1)) return -1;
  if (mlp_forward(xq, B, crit, ch, W("q"), "critic")) return -1;
  float* gs_dq = nullptr;
  if (td_loss(Kc, Kc, rep, (!cfg.max_q_backup && !cfg.deterministic_backup) ? 1 : 0, 1, true, &gs_dq)) return -1;
  BwdOut bc;
  if (mlp_backward(this, crit, xq, ch, B, W("dq"), dch, true, nullptr, "critic.bwd", &bc, gs_dq)) return -1;
  std::vector<int> ksW = bc.ks, ksB = bc.ks;

  // ---- gradient-diversity term (edac.py:136-149) ----
  if (cfg.eta > 0.f) {
    const NetLayout& cl = *crit.lay;
    Mat ones = W("ones"); ones.cs = 0;
    Mat g = W("g"), gam = W("gamma");
    // split precision: the deltas are w_tail-sized (run_edac.py:102: U(+-3e-3) at init), not seed-sized -- their dynamic scale comes from
    // max |w_tail|; gamma and the t_l of the sweep get their own from max |gamma|
    const float* s_delta = nullptr;
    if (split_scales()) {
      Mat wt; wt.p = crit.base + cl.w_off[L]; wt.rs = crit.rs; wt.cs = cl.w_ms[L]; wt.pitch = cl.layer_in(L);
      s_delta = grad_scale(wt, 1, cl.layer_in(L), Kc, "edac.delta");
      if (!s_delta) return -1;
    }
    // (1) unit-seed backward: delta_l = dQ_k/dz_l (top layer stays virtual), g = dQ_k/da
    const InputGrad da{od, A, &g};
    if (mlp_backward(this, crit, xq, ch, B, ones, dd, false, &da, "edac.delta", nullptr, s_delta)) return -1;
    // (2) gamma = d(eta * L_g)/dg ; adds eta*L_g to loss/critics
    float* s_gamma = nullptr;
    {
      EdacGP p; memset(&p, 0, sizeof(p));
      p.g = g.p; p.g_rs = g.rs; p.g_cs = g.cs; p.gpitch = A; p.gamma = gam.p; p.B = B; p.K = Kc; p.A = A; p.eta = cfg.eta; p.m = m; p.slot = 1;
      p.gs_out = s_gamma = gscale_slot();
      ORL_LAUNCH("edac_gamma", k_edac_gamma, dim3(R), dim3(256), p);
    }
    const int nz = R * Kc;
    if (split_scales() && !s_gamma) return -1;
    cur_gscale = s_delta;                                  // the A operands of the sweep's wgrads are the deltas
    auto delta = [&](int l) { return (l == L - 1) ? DY::virt(ch[L - 1], ones) : DY::plain(dd[l]); };
    // (3) adjoint sweep: dW_0[action rows] += gamma^T delta_0 ; t_0 = (gamma W_0[action rows]) (.) m_0
    int ks = wgrad_ksplit(cl.layer_out(0), A, B, nz);
    if (linear_wgrad(delta(0), gam, B, crit, 0, ks, ksW[0], false, "edac.wgrad0", od, A, nullptr, nullptr, s_gamma)) return -1;
    ksW[0] += ks;
    {
      const int N0 = cl.layer_out(0);
      const float* w0 = crit.base + cl.w_off[0] + (long)od * N0;
      const bool vec = cl.ens && (N0 & 3) == 0 && A <= EDAC_T0_AMAX && tt[0].pitch == N0 && ch[0].pitch == N0 && aligned16(w0) && (crit.rs & 3) == 0 && (cl.w_ms[0] & 3) == 0 &&
                       aligned16(tt[0].p) && (tt[0].rs & 3) == 0 && (tt[0].cs & 3) == 0 && aligned16(ch[0].p) && (ch[0].rs & 3) == 0 && (ch[0].cs & 3) == 0;
      // (test tap: which launch makes t_0 and where it takes the mask from -- linear_fwd's own condition for the tiled launch)
      const bool live = ch[0].bits && bits_live.count(ch[0].bits);
      host_taps["edac.t0_path"] = {vec ? 1.f : 0.f, (vec ? live : live && N0 == ch[0].pitch && aligned16(ch[0].p) && (ch[0].pitch & 3) == 0) ? 1.f : 0.f};
      if (vec) {            // A-wide product: one HBM-rate launch instead of a GEMM that is all epilogue
        EdacT0P t; memset(&t, 0, sizeof(t));
        t.gamma = gam.p; t.g_rs = gam.rs; t.g_cs = gam.cs; t.gpitch = gam.pitch;
        t.W = w0; t.w_rs = crit.rs; t.w_cs = cl.w_ms[0]; t.wpitch = N0;
        t.h0 = ch[0].p; t.h_rs = ch[0].rs; t.h_cs = ch[0].cs; t.hpitch = ch[0].pitch;
        if (ch[0].bits && bits_live.count(ch[0].bits)) { t.bits = ch[0].bits; t.b_rs = ch[0].brs; t.b_cs = ch[0].bcs; t.bg = ch[0].bg; }
        else if (vals_dead.count(ch[0].p)) return fail("edac.t0: the first hidden activation was not stored by the forward pass");
        t.out = tt[0].p; t.o_rs = tt[0].rs; t.o_cs = tt[0].cs; t.opitch = tt[0].pitch;
        t.B = B; t.A = A; t.N = N0; t.K = Kc;
        prof_begin("edac.t0", 2.0 * B * (double)N0 * A * nz, nz * (4.0 * B * N0 + B * (double)N0 / 8 + 4.0 * B * A + 4.0 * A * N0));
        hipLaunchKernelGGL(k_edac_t0, dim3((unsigned)((B + 4 * EDAC_T0_RB - 1) / (4 * EDAC_T0_RB)), Kc, R), dim3(256), 0, stream, t);   // four waves x 8 rows
        prof_end();
        if (hipGetLastError() != hipSuccess) return fail("edac.t0 launch");
      } else if (linear_fwd(gam, B, crit, 0, tt[0], E_MASK, &ch[0], "edac.t0", od, A, nullptr, nullptr, nullptr, nullptr, s_gamma)) return -1;
    }
    for (int l = 1; l < L; ++l) {
      ks = wgrad_ksplit(cl.layer_out(l), cl.layer_in(l), B, nz);
      if (linear_wgrad(delta(l), tt[l - 1], B, crit, l, ks, ksW[l], false, "edac.wgrad", 0, -1, nullptr, nullptr, s_gamma)) return -1;
      ksW[l] += ks;
      if (linear_fwd(tt[l - 1], B, crit, l, tt[l], E_MASK, &ch[l], "edac.t", 0, -1, nullptr, nullptr, nullptr, nullptr, s_gamma)) return -1;
    }
    // dw_tail += sum_b t_{L-1}
    ks = wgrad_ksplit(1, cl.layer_in(L), B, nz);
    cur_gscale = nullptr;                                  // A = ones
    if (linear_wgrad(DY::plain(ones), tt[L - 1], B, crit, L, ks, ksW[L], false, "edac.wgrad_tail", 0, -1, nullptr, nullptr, s_gamma)) return -1;
    ksW[L] += ks;
  }
  return adam(ORL_NET_CRITIC1, 1, ORL_OPT_CRITIC, make_segs(*crit.lay, ksW, ksB), ORL_NET_CRITIC1_OLD);
}

}  // namespace orl
