// algo_autoreg.inc — autoregressive behaviour policy (policy/others/autoregressive.py:64-124; tests/autoreg_oracle.py).  Included by engine.hip.
// One net [Linear, LeakyReLU(0.01)] x (L + 1) on [obs | masked act | one-hot], two outputs (mean, logstd) per expanded row.  A step:
// k_autoreg_prepare (B rows -> M = A * B expanded rows, targets, row indices), the forward on the tiled GEMM's E_BIAS_LEAKY flavour down to
// the plain-linear tail, k_autoreg_head (the output LeakyReLU, masked Gaussian NLL, dz_tail, metric, split-precision scale), the generic
// backward with E_LEAKY_MASK, one Adam step.  orl_autoreg_sample: A forward-only passes over n rows with k_autoreg_draw between them.
// mbrcsl_loop (the body of orl_mbrcsl_rollout): sampling, the model step and the trajectory store's append as one device loop.
namespace orl {

int Engine::autoreg_build() {
  const int A = ad, M = A * B;
  metric_names = {"loss"};
  if (epoch_build(M)) return -1;
  alloc("ar_x", M, rup(od + 2 * A, 4));
  alloc("ar_z", M, 2); alloc("ar_dz", M, 2); alloc("ar_out", M, 2); alloc("ar_target", M, 1);
  ar_calls = (unsigned long long*)raw_alloc(sizeof(unsigned long long));
  if (!ar_calls) return fail("hipMalloc sample counter");
  taps["ar_x"] = {W("ar_x"), M, od + 2 * A};
  taps["ar_z"] = {W("ar_z"), M, 2};                 // k_autoreg_head's operand (tail pre-activation) and its seed
  taps["ar_dz"] = {W("ar_dz"), M, 2};
  taps["ar_out"] = {W("ar_out"), M, 2};
  taps["ar_target"] = {W("ar_target"), M, 1};
  return 0;
}

int Engine::autoreg_prepare(int mode) {
  AutoregPrepP p;
  memset(&p, 0, sizeof(p));
  const Mat x = W("ar_x"), o2 = W("b_obs2"), act = W("b_act"), rew = W("b_rew"), t = W("ar_target");
  p.b_obs = o2.p; p.bo_rs = o2.rs; p.b_act = act.p; p.ba_rs = act.rs; p.b_rew = rew.p; p.br_rs = rew.rs;
  p.X = x.p; p.x_rs = x.rs; p.XP = x.pitch; p.T = t.p; p.t_rs = t.rs; p.A = ad;
  static void (*const kern[3])(AutoregPrepP) = {k_autoreg_prepare<RI_SLOTS>, k_autoreg_prepare<RI_DRAWN>, k_autoreg_prepare<RI_ORDER>};
  return epoch_prepare("autoreg_prepare", p, p.d_rew, mode, dim3((unsigned)(((long)B * p.XP + 255) / 256), R), kern);
}

int Engine::autoreg_step() {
  return supervised_step(W("ar_x"), ad * B, W("ar_z"), W("ar_dz"), "autoreg", [&](float* gs, const long long* idx) {
    AutoregHeadP p; memset(&p, 0, sizeof(p));
    p.z = W("ar_z").p; p.z_rs = W("ar_z").rs; p.T = W("ar_target").p; p.t_rs = W("ar_target").rs;
    p.out = W("ar_out").p; p.dz = W("ar_dz").p;
    p.idx = idx; p.B = B; p.A = ad; p.m = mp(); p.slot = 0; p.gs_out = gs;
    ORL_LAUNCH("autoreg_head", k_autoreg_head, dim3(R), dim3(256), p);
    return 0;
  });
}

// workspaces of orl_autoreg_sample for n rows per run; regrown (never shrunk) when n grows
int Engine::autoreg_sample_room(long n) {
  RowScratch& s = ar_ws;
  if (s.mats.empty()) {
    s.what = "orl_autoreg_sample: hipMalloc workspaces";
    ar_sh.assign(L, Mat());
    s.add(ar_sx, rup(od + 2 * ad, 4)); s.add(ar_sz, 2); s.add(ar_seps, ad); s.add(ar_sobs, od);
    for (int i = 0; i < L; ++i) s.add(ar_sh[i], cfg.hidden[i]);
  }
  return room(s, n);
}

int Engine::autoreg_sample(const float* obs, long n, const float* eps, bool on_device, float* act_out) {
  if (autoreg_sample_room(n)) return -1;
  const hipMemcpyKind in_kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const float* d_obs = obs;
  if (!on_device) {
    ORL_HIP(hipMemcpyAsync(ar_sobs.p, obs, sizeof(float) * (size_t)R * n * od, hipMemcpyHostToDevice, stream));
    d_obs = ar_sobs.p;
  }
  // (the noise is staged in the workspace for device callers too: the tap "ar_seps" reads it there)
  if (eps) ORL_HIP(hipMemcpyAsync(ar_seps.p, eps, sizeof(float) * (size_t)R * n * ad, in_kind, stream));
  if (autoreg_sample_launches(d_obs, n, eps ? ar_seps.p : nullptr, act_out, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost)) return -1;
  ORL_HIP(hipStreamSynchronize(stream));      // the only host synchronisation of the call
  return 0;
}

// The MBRCSL rollout loop's form: the launches of a call on device rows, nothing staged and no synchronisation.  The workspaces hold
// the rows already (autoreg_sample_room, once, for the most rows of the loop); the kernels read `eps` ([n][act_dim] normals) where it lies.
int Engine::autoreg_sample_enqueue(const float* obs, long n, const float* eps, float* act_out) {
  if (n > ar_ws.cap) return fail("autoreg_sample_enqueue: more rows than autoreg_sample_room made room for");
  return autoreg_sample_launches(obs, n, eps, act_out, hipMemcpyDeviceToDevice);
}

// row buffers, count slots and events of the MBRCSL rollout loop; the row buffers are zero-filled, so a row no step has written holds zeros
int Engine::mbrcsl_room(long n_traj, long length, long events) {
  RowScratch& s = ml_ws;
  if (s.mats.empty()) {
    s.what = "orl_mbrcsl_rollout: hipMalloc row buffers";
    s.add(ml_obs[0], od); s.add(ml_obs[1], od); s.add(ml_act, ad); s.add(ml_next, od); s.add(ml_rew, 1);
  }
  if (room(s, n_traj)) return -1;
  if (length > ml_counts_cap) {
    ORL_HIP(hipStreamSynchronize(stream));
    if (ml_counts) hipHostFree(ml_counts);
    ml_counts = nullptr; ml_counts_cap = 0;
    ORL_HIP(hipHostMalloc((void**)&ml_counts, sizeof(long long) * length, hipHostMallocDefault));
    ml_counts_cap = length;
  }
  while ((long)ml_events.size() < events) {
    hipEvent_t ev;
    ORL_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ml_events.push_back(ev);
  }
  return 0;
}

// The rollout without a host read per model step (orl_mbrcsl_rollout has refused what it refuses): every launch of the policy, the
// dynamics and the trajectory store on the engine's stream; the host reads survivor counts `lag` steps behind what it enqueues
int Engine::mbrcsl_loop(orl_dynamics* d, const DynStepInfo& di, orl_traj* store, const TrajInfo& ti, const float* init_obs, int n_traj, int length,
                        int term_kind, int penalty_mode, float penalty_coef, const float* eps, int lag, int64_t* rows, double* reward_sum,
                        double* returns_host, int32_t* steps_enqueued, float* elapsed_ms) {
  const char* F = "orl_mbrcsl_rollout";
  const long n_ev = std::min<long>((long)lag + 1, length);
  if (autoreg_sample_room(n_traj) || mbrcsl_room(n_traj, length, n_ev)) return -1;
  if (orl_traj_reset(store, n_traj)) return -1;
  if (dynstep_loop_begin(d, n_traj)) return -1;
  // the store's reset (null stream) and whatever the dynamics' own stream still holds come first; from here to the end every launch of
  // the three objects is on the engine's stream
  LoopScope loop;
  if (loop_begin(loop, {nullptr, di.stream})) return -1;
  DynStreamLease lease(d, stream);
  int enq = 0, cur = 0;
  const auto body = [&]() -> int {
    ORL_HIP(hipMemcpyAsync(ml_obs[0].p, init_obs, sizeof(float) * (size_t)n_traj * od, hipMemcpyDeviceToDevice, stream));
    long bound = n_traj;
    for (int t = 0; t < length; ++t) {
      // the newest survivor count the host may wait for without stalling on a step it has just enqueued: counts never increase, so it
      // bounds the live rows of step t
      const int k = t - 1 - lag;
      if (k >= 0) {
        ORL_HIP(hipEventSynchronize(ml_events[k % n_ev]));
        bound = (long)ml_counts[k];
      }
      if (bound == 0) break;
      float *obs = ml_obs[cur].p, *nxt = ml_obs[cur ^ 1].p;
      if (autoreg_sample_enqueue(obs, bound, eps ? eps + (size_t)t * n_traj * ad : nullptr, ml_act.p)) return -1;
      if (dynstep_enqueue(d, obs, ml_act.p, bound, penalty_mode, penalty_coef, ml_next.p, ml_rew.p)) return -1;
      if (traj_append_enqueue(store, stream, term_kind, obs, ml_act.p, ml_next.p, ml_rew.p, bound, nxt, F)) return -1;
      ORL_HIP(hipMemcpyAsync(ml_counts + t, ti.survivors, sizeof(long long), hipMemcpyDeviceToHost, stream));
      ORL_HIP(hipEventRecord(ml_events[t % n_ev], stream));
      ++enq;
      cur ^= 1;
    }
    return 0;
  };
  const int rc = loop.end(body(), F, elapsed_ms);      // the one unconditional host synchronisation (also on an error path)
  if (steps_enqueued) *steps_enqueued = enq;
  if (rc) return -1;
  return orl_traj_finish(store, rows, reward_sum, returns_host);
}

// what both forms launch: obs / eps are DEVICE arrays of n rows per run (eps null: drawn into the workspace), act_out by `out_kind`
int Engine::autoreg_sample_launches(const float* d_obs, long n, const float* eps, float* act_out, hipMemcpyKind out_kind) {
  const int A = ad;
  // the n rows of every run lie packed at the front of the workspaces (which may hold more rows)
  auto view = [&](Mat m) { m.rs = n * m.pitch; m.cs = m.rs; return m; };
  const Mat x = view(ar_sx), z = view(ar_sz), ep = view(ar_seps);
  std::vector<Mat> hs;
  for (auto& m : ar_sh) hs.push_back(view(m));
  // the workspaces of THIS call as taps (a host map write, no launch): the input rows as the last draw left them, the tail of the last
  // pass and the noise, n rows each (the workspaces may be regrown by a later call, which registers them anew)
  taps["ar_sx"] = {x, n, x.pitch}; taps["ar_sz"] = {z, n, 2}; taps["ar_seps"] = {ep, n, A};
  if (!eps) {
    // device draws: Philox keyed by (seed, this entry point's call counter, run, element = row * A + dim) on a stream id no step uses
    hipLaunchKernelGGL(k_noise, dim3((unsigned)((n * A / 4 + 256) / 256), R), dim3(256), 0, stream, ep.p, n * A, 0, 0.f, 0.f, cfg.seed,
                       (const unsigned long long*)ar_calls, 0x5A5u);
    hipLaunchKernelGGL(k_tick, dim3(1), dim3(1), 0, stream, ar_calls);
    if (hipGetLastError() != hipSuccess) return fail("orl_autoreg_sample: noise launch failed");
  }
  AutoregDrawP d; memset(&d, 0, sizeof(d));
  d.z = z.p; d.z_rs = z.rs; d.eps = eps ? eps : ep.p; d.e_rs = ep.rs; d.obs = d_obs; d.o_rs = n * od;
  d.X = x.p; d.x_rs = x.rs; d.XP = x.pitch; d.n = n; d.od = od; d.A = A; d.first = 1;
  const dim3 grid((unsigned)((n + 255) / 256), R);
  ORL_LAUNCH("autoreg_draw", k_autoreg_draw, grid, dim3(256), d);
  d.first = 0;
  const NetRef net = net_ref(ORL_NET_ACTOR, 1);
  gscale_next = 0; cur_gscale = nullptr; lab_slot = 0;
  for (int j = 0; j < A; ++j) {
    if (mlp_forward_only(x, (int)n, net, hs, z, "autoreg.sample")) return -1;
    d.j = j;
    ORL_LAUNCH("autoreg_draw", k_autoreg_draw, grid, dim3(256), d);
  }
  ORL_HIP(hipMemcpy2DAsync(act_out, sizeof(float) * A, x.p + od, sizeof(float) * x.pitch, sizeof(float) * A, (size_t)R * n,
                           out_kind, stream));
  return 0;
}

}  // namespace orl
