// algo_rambo.inc — RAMBO's advantage on a SAC engine (policy/model_based/rambo.py:164-181) and the engine's share of the device loop of
// update_dynamics (rambo.py:95-127; orl_rambo_update_dynamics in engine.hip strings it together with the dynamics' adversarial pair).
// Forward-only passes on workspaces of their own: no parameter, optimizer state, step counter or noise stream of orl_learn_n is touched.
//   advantage   k_adv_assemble ([s | a] and [s' | .] as ONE 2 Ba-row critic operand, s' as the actor's input), the actor pass with the
//               deterministic sampling job (a' = tanh(mu(s')) into the operand, logp' at the mode), ONE pass of both live critics over the
//               2 Ba rows, k_adv_norm (termination test, TD value, raw advantage, the two reductions, the normalisation)
//   action      k_adv_assemble (s as the actor's input), k_noise on the loop's own Philox stream, the actor pass with a sampling job
// Included by engine.hip.
namespace orl {

// the first `rows` rows of every run of a matrix allocated for more: runs packed at the front
static Mat adv_view(Mat m, long rows, int nets = 1) { m.cs = rows * m.pitch; m.rs = m.cs * nets; return m; }

static void adv_drop(Engine* e, Mat& m) {
  if (!m.p) return;
  e->range_watch.erase(m.p);
  e->vals_dead.erase(m.p);
  e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), (void*)m.p), e->allocs.end());
  hipFree(m.p);
  m = Mat();
}
static bool adv_make(Engine* e, Mat& m, long rows, int pitch, int nets = 1) {
  m = Mat();
  m.p = e->raw_alloc(sizeof(float) * (size_t)rows * pitch * nets * e->R);
  m.pitch = pitch;
  return m.p != nullptr;
}

// workspaces of orl_engine_adv_advantage for Ba rows per run; regrown (never shrunk) when Ba grows
int Engine::adv_room(long Ba) {
  if (Ba <= adv_cap) return 0;
  ORL_HIP(hipStreamSynchronize(stream));
  for (Mat* m : {&adv_xs, &adv_xc, &adv_head, &adv_logp, &adv_q}) adv_drop(this, *m);
  for (Mat& m : adv_v) adv_drop(this, m);
  for (Mat& m : adv_in) adv_drop(this, m);
  for (Mat& m : adv_ah) adv_drop(this, m);
  for (Mat& m : adv_ch) adv_drop(this, m);
  for (const char* t : {"adv.term", "adv.q_next", "adv.q_base", "adv.raw", "adv.norm", "adv.logp_next"}) taps.erase(t);
  adv_ah.assign(L, Mat()); adv_ch.assign(L, Mat());
  adv_cap = 0;
  bool ok = adv_make(this, adv_xs, Ba, OP) && adv_make(this, adv_xc, 2 * Ba, XP) && adv_make(this, adv_head, Ba, 2 * ad) &&
            adv_make(this, adv_logp, Ba, 1) && adv_make(this, adv_q, 2 * Ba, 1, 2) && adv_make(this, adv_in[0], Ba, od) &&
            adv_make(this, adv_in[1], Ba, ad) && adv_make(this, adv_in[2], Ba, od) && adv_make(this, adv_in[3], Ba, 1);
  for (Mat& m : adv_v) ok = ok && adv_make(this, m, Ba, 1);
  for (int i = 0; i < L && ok; ++i) ok = adv_make(this, adv_ah[i], Ba, cfg.hidden[i]) && adv_make(this, adv_ch[i], 2 * Ba, cfg.hidden[i], 2);
  if (ok && !adv_stats) ok = (adv_stats = raw_alloc(sizeof(float) * 2 * R)) != nullptr;
  if (!ok) return fail("orl_engine_adv_advantage: hipMalloc workspaces");
  adv_cap = Ba;
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
  if (rows <= rambo_cap) return 0;
  ORL_HIP(hipStreamSynchronize(stream));
  for (Mat* m : {&rb_obs[0], &rb_obs[1], &rb_act, &rb_eps, &rb_rew, &rb_adv}) adv_drop(this, *m);
  for (Mat& m : rb_sl) adv_drop(this, m);
  for (const char* t : {"loop.obs", "loop.act", "loop.sl_obs", "loop.sl_act", "loop.sl_next_obs", "loop.sl_rew", "loop.next_obs", "loop.reward"})
    taps.erase(t);
  rambo_cap = 0;
  bool ok = adv_make(this, rb_obs[0], rows, od) && adv_make(this, rb_obs[1], rows, od) && adv_make(this, rb_act, rows, ad) &&
            adv_make(this, rb_eps, rows, ad) && adv_make(this, rb_rew, rows, 1) && adv_make(this, rb_adv, rows, 1) &&
            adv_make(this, rb_sl[0], rows, od) && adv_make(this, rb_sl[1], rows, ad) && adv_make(this, rb_sl[2], rows, od) &&
            adv_make(this, rb_sl[3], rows, 1) && adv_make(this, rb_sl[4], rows, 1);
  if (ok && !rb_acc) ok = (rb_acc = raw_alloc(sizeof(float) * 8)) != nullptr;
  if (ok && !rb_calls) ok = (rb_calls = (unsigned long long*)raw_alloc(sizeof(unsigned long long))) != nullptr;
  if (!ok) return fail("orl_rambo_update_dynamics: hipMalloc row buffers");
  rambo_cap = rows;
  return 0;
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
