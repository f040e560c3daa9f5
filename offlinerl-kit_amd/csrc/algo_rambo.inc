// algo_rambo.inc — RAMBO's advantage on a SAC engine (policy/model_based/rambo.py:164-181) and the engine's share of the device loop of
// update_dynamics (rambo.py:95-127; rambo_loop, the body of orl_rambo_update_dynamics, strings it together with the dynamics' adversarial pair).
// Forward-only passes on workspaces of their own: no parameter, optimizer state, step counter or noise stream of orl_learn_n is touched.
//   advantage   k_adv_assemble ([s | a] and [s' | .] as ONE 2 Ba-row critic operand, s' as the actor's input), the actor pass with the
//               deterministic sampling job (a' = tanh(mu(s')) into the operand, logp' at the mode), ONE pass of both live critics over the
//               2 Ba rows, k_adv_norm (termination test, TD value, raw advantage, the two reductions, the normalisation)
//   action      k_adv_assemble (s as the actor's input), k_noise on the loop's own Philox stream, the actor pass with a sampling job
// Included by engine.hip.
namespace orl {

// the first `rows` rows of every run of a matrix allocated for more: runs packed at the front
static Mat adv_view(Mat m, long rows, int nets = 1) { m.cs = rows * m.pitch; m.rs = m.cs * nets; return m; }

// workspaces of orl_engine_adv_advantage for Ba rows per run; regrown (never shrunk) when Ba grows
int Engine::adv_room(long Ba) {
  RowScratch& s = adv_ws;
  if (s.mats.empty()) {
    s.what = "orl_engine_adv_advantage: hipMalloc workspaces";
    s.taps = {"adv.term", "adv.q_next", "adv.q_base", "adv.raw", "adv.norm", "adv.logp_next"};
    adv_ah.assign(L, Mat()); adv_ch.assign(L, Mat());
    s.add(adv_xs, OP); s.add(adv_xc, XP, 2); s.add(adv_head, 2 * ad); s.add(adv_logp, 1); s.add(adv_q, 1, 2, 2);
    s.add(adv_in[0], od); s.add(adv_in[1], ad); s.add(adv_in[2], od); s.add(adv_in[3], 1);
    for (Mat& m : adv_v) s.add(m, 1);
    for (int i = 0; i < L; ++i) { s.add(adv_ah[i], cfg.hidden[i]); s.add(adv_ch[i], cfg.hidden[i], 2, 2); }
  }
  if (room(s, Ba)) return -1;
  if (!adv_stats && !(adv_stats = raw_alloc(sizeof(float) * 2 * R))) return fail(s.what);
  return 0;
}

// every array is a packed DEVICE array of Ba rows per run; adv_dev ([R][Ba], may be null) also receives the normalised advantage
int Engine::adv_advantage(const float* obs, const float* act, const float* nobs, const float* rew, long Ba, int term_kind, int include_ent,
                          float* adv_dev) {
  const int A = ad, n = (int)Ba;
  const Mat xs = adv_view(adv_xs, Ba), xc = adv_view(adv_xc, 2 * Ba), head = adv_view(adv_head, Ba), logp = adv_view(adv_logp, Ba);
  const Mat q = adv_view(adv_q, 2 * Ba, 2);
  std::vector<Mat> ah, ch;
  for (auto& m : adv_ah) ah.push_back(adv_view(m, Ba));
  for (auto& m : adv_ch) ch.push_back(adv_view(m, 2 * Ba, 2));
  {
    AdvInP p; memset(&p, 0, sizeof(p));
    p.src = nobs; p.obs = obs; p.act = act;
    p.xs = xs.p; p.xs_rs = xs.rs; p.OP = xs.pitch;
    p.xc = xc.p; p.xc_rs = xc.rs; p.XP = xc.pitch;
    p.Ba = n; p.od = od; p.ad = ad;
    ORL_LAUNCH("adv.assemble", k_adv_assemble, dim3((n + 255) / 256, R), dim3(256), p);
  }
  gscale_next = 0; cur_gscale = nullptr; lab_slot = 0;
  {
    SampleJob j = make_job(0, n, 1, Mat(), xc, od, n, logp);      // no eps: the mode
    bool sampled = false;
    if (mlp_forward_only(xs, n, net_ref(ORL_NET_ACTOR, 1), ah, head, "adv.actor", &j, 1, &sampled)) return -1;
    if (!sampled && launch_sample(this, head, A, &j, 1)) return -1;
  }
  if (mlp_forward_only(xc.shared(), 2 * n, net_ref(ORL_NET_CRITIC1, 2), ch, q, "adv.critic")) return -1;
  Mat v[5];
  for (int i = 0; i < 5; ++i) v[i] = adv_view(adv_v[i], Ba);
  {
    AdvNormP p; memset(&p, 0, sizeof(p));
    p.q = q.z();
    p.logp = logp.p; p.lp_rs = logp.rs;
    p.nobs = nobs; p.rew = rew;
    p.term = v[0].p; p.qn = v[1].p; p.qb = v[2].p; p.raw = v[3].p; p.norm = v[4].p;
    p.adv_out = adv_dev; p.stats = adv_stats;
    p.Ba = n; p.od = od; p.kind = term_kind; p.include_ent = include_ent;
    p.gamma = cfg.gamma; p.sc = scalars; p.auto_alpha = cfg.auto_alpha; p.fixed_alpha = cfg.alpha;
    ORL_LAUNCH("adv.norm", k_adv_norm, dim3(R), dim3(256), p);
  }
  taps["adv.term"] = {v[0], Ba, 1}; taps["adv.q_next"] = {v[1], Ba, 1}; taps["adv.q_base"] = {v[2], Ba, 1};
  taps["adv.raw"] = {v[3], Ba, 1}; taps["adv.norm"] = {v[4], Ba, 1}; taps["adv.logp_next"] = {logp, Ba, 1};
  return 0;
}

// row buffers of the device loop for `rows` rows (one run)
int Engine::rambo_room(long rows) {
  RowScratch& s = rambo_ws;
  if (s.mats.empty()) {
    s.what = "orl_rambo_update_dynamics: hipMalloc row buffers";
    s.taps = {"loop.obs", "loop.act", "loop.sl_obs", "loop.sl_act", "loop.sl_next_obs", "loop.sl_rew", "loop.next_obs", "loop.reward"};
    s.add(rb_obs[0], od); s.add(rb_obs[1], od); s.add(rb_act, ad); s.add(rb_eps, ad); s.add(rb_rew, 1); s.add(rb_adv, 1);
    s.add(rb_sl[0], od); s.add(rb_sl[1], ad); s.add(rb_sl[2], od); s.add(rb_sl[3], 1); s.add(rb_sl[4], 1);
  }
  if (room(s, rows)) return -1;
  if (!rb_acc && !(rb_acc = raw_alloc(sizeof(float) * 8))) return fail(s.what);
  if (!rb_calls && !(rb_calls = (unsigned long long*)raw_alloc(sizeof(unsigned long long)))) return fail(s.what);
  return 0;
}

// update_dynamics without coming back to the host (orl_rambo_update_dynamics has refused what it refuses): every launch of the engine and
// of the dynamics' adversarial pair on the engine's stream, one synchronisation at the end
int Engine::rambo_loop(orl_dynamics* d, const DynAdvInfo& di, Buffer& b, const orl_rambo_loop* a, float* metrics_mean, float* elapsed_ms) {
  const char* F = "orl_rambo_update_dynamics";
  const int rows = a->rows;
  if (adv_room(rows) || rambo_room(rows)) return -1;
  if (dynadv_loop_begin(d)) return -1;
  // whatever the dynamics' own stream still holds comes first; from here to the end every launch of both objects is on the engine's stream
  LoopScope loop;
  if (loop_begin(loop, {di.stream})) return -1;
  DynStreamLease lease(d, stream);
  long done = 0;
  int cur = 0;
  const auto body = [&]() -> int {
    ORL_HIP(hipMemsetAsync(rb_acc, 0, sizeof(float) * 8, stream));
    for (int s = 0; s < a->n_segments; ++s) {
      // the segment's initial observations: one draw, of which the observation rows are kept
      if (buffer_gather(b, nullptr, rows, cfg.seed, rb_obs[cur].p, rb_sl[1].p, rb_sl[2].p, rb_sl[3].p, rb_sl[4].p, stream)) return -1;
      for (int k = 0; k < a->segment_steps[s]; ++k) {
        float* obs = rb_obs[cur].p;
        float* nxt = rb_obs[cur ^ 1].p;
        if (adv_act(obs, rows, rb_act.p)) return -1;
        if (buffer_gather(b, nullptr, rows, cfg.seed, rb_sl[0].p, rb_sl[1].p, rb_sl[2].p, rb_sl[3].p, rb_sl[4].p, stream)) return -1;
        if (dynadv_forward_enqueue(d, obs, rb_act.p, rb_sl[0].p, rb_sl[1].p, rb_sl[2].p, rb_sl[3].p, nxt, rb_rew.p)) return -1;
        if (adv_advantage(obs, rb_act.p, nxt, rb_rew.p, rows, a->term_kind, a->include_ent != 0, rb_adv.p)) return -1;
        if (dynadv_update_enqueue(d, rb_adv.p, (int)done)) return -1;
        hipLaunchKernelGGL(k_rambo_accum, dim3(1), dim3(1), 0, stream, rb_acc, di.metrics, (const float*)adv_stats);
        if (hipGetLastError() != hipSuccess) return fail(std::string(F) + ": accumulate launch failed");
        ++done;
        cur ^= 1;
      }
    }
    return 0;
  };
  const int rc = loop.end(body(), F, elapsed_ms);      // the one host synchronisation (also on an error path: the launches made so far ran)
  dynadv_loop_end(d, done);
  if (rc) return -1;
  // the last step's rows: cur now names the buffer its next_obs went to
  const auto tap = [&](const char* name, const Mat& m, int cols) { Mat v = m; v.rs = (long)rows * cols; taps[name] = {v, rows, cols}; };
  tap("loop.obs", rb_obs[cur ^ 1], od); tap("loop.next_obs", rb_obs[cur], od); tap("loop.act", rb_act, ad);
  tap("loop.sl_obs", rb_sl[0], od); tap("loop.sl_act", rb_sl[1], ad); tap("loop.sl_next_obs", rb_sl[2], od);
  tap("loop.sl_rew", rb_sl[3], 1); tap("loop.reward", rb_rew, 1);
  float acc[5];
  ORL_HIP(hipMemcpy(acc, rb_acc, sizeof(acc), hipMemcpyDeviceToHost));
  bool finite = true;
  for (int k = 0; k < 5; ++k) { finite = finite && std::isfinite(acc[k]); metrics_mean[k] = acc[k] / (float)done; }
  if (!finite) health_host[0] |= ORL_HEALTH_NONFINITE_LOSS;
  unsigned int bad = 0;
  if (health_update(nullptr, 0, &bad)) return -1;
  return bad ? ORL_RC_UNHEALTHY : 0;
}

// MOPOPolicy.select_action on device rows: a = tanh(mu + sigma eps), eps from Philox keyed by (seed, the loop's own call counter, run,
// element) on a stream id no step and no other entry point uses
int Engine::adv_act(const float* obs, long Ba, float* act_out) {
  const int A = ad, n = (int)Ba;
  const Mat xs = adv_view(adv_xs, Ba), head = adv_view(adv_head, Ba), logp = adv_view(adv_logp, Ba), eps = adv_view(rb_eps, Ba);
  std::vector<Mat> ah;
  for (auto& m : adv_ah) ah.push_back(adv_view(m, Ba));
  {
    AdvInP p; memset(&p, 0, sizeof(p));
    p.src = obs; p.xs = xs.p; p.xs_rs = xs.rs; p.OP = xs.pitch; p.Ba = n; p.od = od; p.ad = ad;
    ORL_LAUNCH("loop.assemble", k_adv_assemble, dim3((n + 255) / 256, R), dim3(256), p);
  }
  const long ne = Ba * A;
  hipLaunchKernelGGL(k_noise, dim3((unsigned)((ne / 4 + 256) / 256), R), dim3(256), 0, stream, eps.p, ne, 0, 0.f, 0.f, cfg.seed,
                     (const unsigned long long*)rb_calls, 0x5A6u);
  hipLaunchKernelGGL(k_tick, dim3(1), dim3(1), 0, stream, rb_calls);
  if (hipGetLastError() != hipSuccess) return fail("orl_rambo_update_dynamics: noise launch failed");
  gscale_next = 0; cur_gscale = nullptr; lab_slot = 0;
  Mat dst; dst.p = act_out; dst.pitch = A; dst.rs = Ba * A; dst.cs = dst.rs;
  SampleJob j = make_job(0, n, 1, eps, dst, 0, 0, logp);
  bool sampled = false;
  if (mlp_forward_only(xs, n, net_ref(ORL_NET_ACTOR, 1), ah, head, "loop.actor", &j, 1, &sampled)) return -1;
  if (!sampled && launch_sample(this, head, A, &j, 1)) return -1;
  return 0;
}

}  // namespace orl
