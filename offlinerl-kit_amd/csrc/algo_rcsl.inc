// algo_rcsl.inc — RCSL schedule (policy/rcsl/rcsl.py:123-151; tests/rcsl_oracle.py).  Included by engine.hip.
// One net: pred = MLP([obs | rtg]) with a plain linear output, loss = mean over (valid rows x act_dim) of (pred - act)^2, one Adam step.
// The return-to-go travels in the batch's `rewards` slot / the buffer's reward column.
namespace orl {

// ---- what the supervised policies share (RCSL, Gaussian RCSL, AUTOREG): one net, the ordered epoch, one step shape ----
int Engine::epoch_build(long rows) {
  alloc_layers("ah", rows); alloc_layers("dah", rows);
  epoch_cell = (EpochCell*)raw_alloc(sizeof(EpochCell));
  order_flags = (unsigned int*)raw_alloc(sizeof(unsigned int));
  return epoch_cell && order_flags ? 0 : fail("hipMalloc epoch cell");
}

// the step's input launch: kern[mode] with mode RI_SLOTS (orl_step: the batch slots), RI_DRAWN (orl_learn_n) or RI_ORDER (orl_learn_epoch);
// the last two read the attached dataset (d_rew: the parameter struct's reward / return-to-go column)
template <class P>
int Engine::epoch_prepare(const char* tag, P& p, const float*& d_rew, int mode, dim3 grid, void (*const kern[3])(P)) {
  static_assert(RI_SLOTS == 0 && RI_DRAWN == 1 && RI_ORDER == 2, "kern[] is indexed by the mode");
  p.idx_out = d_idx; p.B = B; p.od = od; p.OP = OP; p.AP = AP; p.seed = cfg.seed; p.gstep = gstep;
  if (mode != RI_SLOTS) {
    if (!buf || !buf->obs) return fail("no replay buffer attached (orl_engine_attach_buffer)");
    p.d_obs = buf->obs; p.d_act = buf->act; d_rew = buf->rew; p.n = buf->n;
    p.order = d_order; p.cell = epoch_cell;
    if (mode == RI_ORDER && !d_order) return fail("ordered epoch without a row order");
  }
  ORL_LAUNCH(tag, kern[mode], grid, dim3(256), p);
  return 0;
}

// prepare, forward of x (M rows) to `out`, head_launch(gs, idx) -- loss, metric, the seed `dseed` and its scale; idx: the rows' dataset
// indices, null when every row of the caller's batch is valid (orl_step) --, backward, Adam
template <class F>
int Engine::supervised_step(const Mat& x, int M, const Mat& out, const Mat& dseed, const char* tag, F head_launch) {
  const NetRef net = net_ref(ORL_NET_ACTOR, 1);
  std::vector<Mat> ah = layers("ah"), dah = layers("dah");
  if (cfg.algo == ORL_ALGO_AUTOREG ? autoreg_prepare(rcsl_mode) : rcsl_prepare(rcsl_mode)) return -1;
  if (mlp_forward(x, M, net, ah, out, tag)) return -1;
  float* gs = gscale_slot();                              // (split precision: the seed kernel publishes the dynamic scale of its backward pass)
  if (head_launch(gs, rcsl_mode == RI_SLOTS ? nullptr : d_idx)) return -1;
  return train_net(net, ORL_NET_ACTOR, 1, ORL_OPT_ACTOR, x, ah, M, dseed, dah, (std::string(tag) + ".bwd").c_str(), gs);
}

int Engine::rcsl_build() {
  const int A = ad;
  metric_names = {"loss"};
  if (epoch_build(B)) return -1;
  alloc("rcsl_x", B, rup(od + 1, 4));
  alloc("pred", B, A); alloc("dpred", B, A);
  taps["pred"] = {W("pred"), B, A};
  taps["dpred"] = {W("dpred"), B, A};              // k_rcsl_loss's seed (the backward pass reads it, nothing writes it again)
  taps["rcsl_x"] = {W("rcsl_x"), B, od + 1};
  return 0;
}

int Engine::rcsl_prepare(int mode) {
  RcslPrepP p;
  memset(&p, 0, sizeof(p));
  const Mat x = W("rcsl_x"), o2 = W("b_obs2"), act = W("b_act"), rtg = W("b_rew");
  p.b_obs = o2.p; p.bo_rs = o2.rs; p.b_act = act.p; p.ba_rs = act.rs; p.b_rtg = rtg.p; p.br_rs = rtg.rs;
  p.X = x.p; p.x_rs = x.rs; p.XP = x.pitch; p.W = std::max(x.pitch, AP);
  static void (*const kern[3])(RcslPrepP) = {k_rcsl_prepare<RI_SLOTS>, k_rcsl_prepare<RI_DRAWN>, k_rcsl_prepare<RI_ORDER>};
  return epoch_prepare("rcsl_prepare", p, p.d_rtg, mode, dim3((unsigned)(((long)B * p.W + 255) / 256), R), kern);
}

int Engine::rcsl_step() {
  return supervised_step(W("rcsl_x"), B, W("pred"), W("dpred"), "rcsl", [&](float* gs, const long long* idx) {
    const Mat act = W("b_act");
    RcslLossP p; memset(&p, 0, sizeof(p));
    p.pred = W("pred").p; p.pred_rs = W("pred").rs; p.act = act.p; p.act_rs = act.rs; p.apitch = act.pitch; p.dpred = W("dpred").p;
    p.idx = idx; p.B = B; p.A = ad; p.m = mp(); p.slot = 0; p.gs_out = gs;
    ORL_LAUNCH("rcsl_loss", k_rcsl_loss, dim3(R), dim3(256), p);
    return 0;
  });
}

}  // namespace orl
