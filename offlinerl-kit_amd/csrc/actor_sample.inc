// actor_sample.inc — orl_actor_sample: the tanh-Gaussian actor of the SAC family (SAC / MOPO / RAMBO, CQL / COMBO, MCQ, EDAC, MOBILE)
// sampled for the model-based rollouts on the fused split-fp16 kernel of actor_fused.h: the weight pack and ONE launch per call.
// Nothing here is part of a training step; the planes, range words and workspaces are made at the first call.  Included by engine.hip.
namespace orl {

// The refusals (an actor that is not ActorProb + TanhDiagGaussian(conditioned_sigma), the kernel's widths) and, once, the planes, the two
// sticky range words with their pinned host copy, the live-count table and the call counter of the device draws.
int Engine::actor_sample_setup() {
  const std::string F = "orl_actor_sample";
  if (as_planes) return 0;
  switch (cfg.algo) {
    case ORL_ALGO_SAC: case ORL_ALGO_CQL: case ORL_ALGO_MCQ: case ORL_ALGO_EDAC: case ORL_ALGO_MOBILE: break;
    case ORL_ALGO_IQL:
      if (cfg.actor_dropout != 0.f) return fail(F + ": the actor's backbone has dropout; the fused kernel has no dropout masks");
      return fail(F + ": the IQL actor is a DiagGaussian with a state-independent sigma_param and no tanh, not a tanh-Gaussian with a state-conditioned sigma");
    case ORL_ALGO_TD3BC: return fail(F + ": the TD3+BC actor is deterministic: it has no Gaussian head to sample");
    case ORL_ALGO_RCSL: return fail(F + ": the RCSL policy is a deterministic return-conditioned MLP, not a tanh-Gaussian actor");
    case ORL_ALGO_RCSL_GAUSS: return fail(F + ": the Gaussian RCSL policy is return-conditioned and has no tanh, not a tanh-Gaussian actor");
    case ORL_ALGO_AUTOREG: return fail(F + ": the autoregressive policy samples through orl_autoreg_sample, not a tanh-Gaussian actor");
    default: return fail(F + ": not a tanh-Gaussian actor");
  }
  const int MAXW = ORL_ACTOR_FUSED_MAX_WIDTH, MAXA = ORL_ACTOR_FUSED_MAX_ACT;
  if (od > MAXW) return fail(F + ": obs_dim " + std::to_string(od) + " is wider than the " + std::to_string(MAXW) + " columns the fused kernel takes");
  for (int i = 0; i < L; ++i)
    if (cfg.hidden[i] > MAXW)
      return fail(F + ": a hidden layer of " + std::to_string(cfg.hidden[i]) + " units is wider than the " + std::to_string(MAXW) + " columns the fused kernel takes");
  if (ad > MAXA) return fail(F + ": act_dim " + std::to_string(ad) + " is more than the " + std::to_string(MAXA) + " action dimensions the fused kernel takes");
  const NetLayout& nl = lay[ORL_NET_ACTOR];
  AcfP f; memset(&f, 0, sizeof(f));
  f.g.R = R; f.g.K = 1; f.g.nl = L + 1;
  f.g.width[0] = od;
  for (int i = 0; i < L; ++i) f.g.width[i + 1] = cfg.hidden[i];
  f.g.width[L + 1] = 2 * ad;               // the arena's tail is [mu ; sigma], one [2A][H] matrix and one [2A] bias
  for (int l = 0; l <= L; ++l) { f.g.w_off[l] = nl.w_off[l]; f.g.b_off[l] = nl.b_off[l]; }
  f.g.params = net_ptr(0, ORL_NET_ACTOR); f.g.P = P_train;
  f.A = ad;
  const long halves = acf_layout(f);
  ORL_HIP(hipSetDevice(dev));
  hx_t* planes = (hx_t*)raw_alloc(sizeof(hx_t) * 2 * (size_t)halves);
  unsigned int* fl = (unsigned int*)raw_alloc(sizeof(unsigned int) * DYF_FLAGS);
  as_live = (int*)raw_alloc(sizeof(int) * (size_t)R);
  as_calls = (unsigned long long*)raw_alloc(sizeof(unsigned long long));
  if (!planes || !fl || !as_live || !as_calls) return fail(F + ": hipMalloc weight planes");
  if (!as_hflags) ORL_HIP(hipHostMalloc((void**)&as_hflags, sizeof(unsigned int) * DYF_FLAGS, hipHostMallocDefault));
  as_hflags[DYF_FLAG_ACT] = as_hflags[DYF_FLAG_W] = 0u;
  f.g.Bh = planes; f.g.Bl = planes + halves; f.g.flags = fl;
  as_ws.what = "orl_actor_sample: hipMalloc workspaces";
  as_ws.add(as_obs, od); as_ws.add(as_eps, ad); as_ws.add(as_act, ad);
  as_f = f; as_planes = planes;
  return 0;
}

// run < 0: every run, arrays [R][n][...]; run = r: that run's actor on arrays without the run dimension.  `live` is a HOST array (R
// counts, or one) whatever on_device says: it goes into a device table on the stream, as the rings' tables of a per-run append do.
int Engine::actor_sample(int run, const float* obs, long n, const float* eps, const int* live, bool det, bool on_device, float* act) {
  if (actor_sample_setup() || room(as_ws, n)) return -1;
  const int Rl = run < 0 ? R : 1, r0 = run < 0 ? 0 : run, A = ad;
  const size_t rows = (size_t)Rl * n;
  const float *d_obs = obs, *d_eps = det ? nullptr : eps;
  if (!on_device) {
    ORL_HIP(hipMemcpyAsync(as_obs.p, obs, sizeof(float) * rows * od, hipMemcpyHostToDevice, stream));
    d_obs = as_obs.p;
    if (d_eps) { ORL_HIP(hipMemcpyAsync(as_eps.p, eps, sizeof(float) * rows * A, hipMemcpyHostToDevice, stream)); d_eps = as_eps.p; }
  }
  if (!det && !eps) {
    // device draws for all R runs, so run r's normals are keyed by r in either form: Philox keyed by (seed, this entry point's call
    // counter, run, element = row * A + dim) on a stream id no step and no other sample call uses
    hipLaunchKernelGGL(k_noise, dim3((unsigned)((n * A / 4 + 256) / 256), R), dim3(256), 0, stream, as_eps.p, n * A, 0, 0.f, 0.f, cfg.seed,
                       (const unsigned long long*)as_calls, 0xAC7u);
    hipLaunchKernelGGL(k_tick, dim3(1), dim3(1), 0, stream, as_calls);
    if (hipGetLastError() != hipSuccess) return fail("orl_actor_sample: noise launch failed");
    d_eps = as_eps.p + (long)r0 * n * A;
  }
  if (live) ORL_HIP(hipMemcpyAsync(as_live, live, sizeof(int) * (size_t)Rl, hipMemcpyHostToDevice, stream));
  AcfP f = as_f;
  f.g.R = Rl; f.g.n = n;
  f.g.params += (long)r0 * f.g.P; f.g.Bh += (long)r0 * f.g.pmember; f.g.Bl += (long)r0 * f.g.pmember;
  f.deterministic = det ? 1 : 0;
  f.obs = d_obs; f.eps = d_eps; f.e_rs = n * A; f.live = live ? as_live : nullptr; f.act = on_device ? act : as_act.p;
  // the pack runs on every call: the arena is aliased by the caller's tensors and trained between rollouts
  if (timed("orl_actor_sample", "actor_pack_planes", false, 0, 0, [&] { return acf_pack(f, stream); })) return -1;
  if (timed("orl_actor_sample", "actor_fused_sample", false, 0, 0, [&] { return acf_sample(f, stream); })) return -1;
  if (!on_device) ORL_HIP(hipMemcpyAsync(act, as_act.p, sizeof(float) * rows * A, hipMemcpyDeviceToHost, stream));
  ORL_HIP(hipMemcpyAsync(as_hflags, f.g.flags, sizeof(unsigned int) * DYF_FLAGS, hipMemcpyDeviceToHost, stream));
  ORL_HIP(hipStreamSynchronize(stream));      // the only host synchronisation of the call
  return range_flags_check("orl_actor_sample", "actor", as_hflags, f.g.flags);
}

}  // namespace orl
