// algo_rcsl.inc — RCSL schedule (policy/rcsl/rcsl.py:123-151; tests/rcsl_oracle.py).  Included by engine.hip.
// One net: pred = MLP([obs | rtg]) with a plain linear output, loss = mean over (valid rows x act_dim) of (pred - act)^2, one Adam step.
// The return-to-go travels in the batch's `rewards` slot / the buffer's reward column.
namespace orl {

int Engine::rcsl_build() {
  const int A = ad;
  metric_names = {"loss"};
  for (int i = 0; i < L; ++i) {
    const int h = cfg.hidden[i];
    const std::string s = std::to_string(i);
    alloc("ah" + s, B, h); alloc("dah" + s, B, h);
  }
  alloc("rcsl_x", B, rup(od + 1, 4));
  alloc("pred", B, A); alloc("dpred", B, A);
  epoch_cell = (EpochCell*)raw_alloc(sizeof(EpochCell));
  order_flags = (unsigned int*)raw_alloc(sizeof(unsigned int));
  if (!epoch_cell || !order_flags) return fail("hipMalloc epoch cell");
  taps["pred"] = {W("pred"), B, A};
  taps["rcsl_x"] = {W("rcsl_x"), B, od + 1};
  return 0;
}

// the step's input launch: mode RI_SLOTS (orl_step), RI_DRAWN (orl_learn_n) or RI_ORDER (orl_learn_epoch)
int Engine::rcsl_prepare(int mode) {
  RcslPrepP p;
  memset(&p, 0, sizeof(p));
  const Mat x = W("rcsl_x"), o2 = W("b_obs2"), act = W("b_act"), rtg = W("b_rew");
  p.b_obs = o2.p; p.bo_rs = o2.rs; p.b_act = act.p; p.ba_rs = act.rs; p.b_rtg = rtg.p; p.br_rs = rtg.rs;
  p.X = x.p; p.x_rs = x.rs; p.XP = x.pitch; p.OP = OP; p.AP = AP;
  p.idx_out = d_idx; p.B = B; p.od = od; p.W = std::max(x.pitch, AP);
  p.seed = cfg.seed; p.gstep = gstep;
  if (mode != RI_SLOTS) {
    if (!buf || !buf->obs) return fail("no replay buffer attached (orl_engine_attach_buffer)");
    p.d_obs = buf->obs; p.d_act = buf->act; p.d_rtg = buf->rew; p.n = buf->n;
    p.order = d_order; p.cell = epoch_cell;
    if (mode == RI_ORDER && !d_order) return fail("ordered epoch without a row order");
  }
  const dim3 grid((unsigned)(((long)B * p.W + 255) / 256), R);
  if (mode == RI_SLOTS) ORL_LAUNCH("rcsl_prepare", k_rcsl_prepare<RI_SLOTS>, grid, dim3(256), p);
  else if (mode == RI_DRAWN) ORL_LAUNCH("rcsl_prepare", k_rcsl_prepare<RI_DRAWN>, grid, dim3(256), p);
  else ORL_LAUNCH("rcsl_prepare", k_rcsl_prepare<RI_ORDER>, grid, dim3(256), p);
  return 0;
}

int Engine::rcsl_step() {
  const NetRef net = net_ref(ORL_NET_ACTOR, 1);
  std::vector<Mat> ah, dah;
  for (int i = 0; i < L; ++i) { ah.push_back(W("ah" + std::to_string(i))); dah.push_back(W("dah" + std::to_string(i))); }
  const Mat x = W("rcsl_x"), act = W("b_act");
  if (rcsl_prepare(rcsl_mode)) return -1;
  if (mlp_forward(x, B, net, ah, W("pred"), "rcsl")) return -1;
  float* gs = nullptr;
  {
    RcslLossP p; memset(&p, 0, sizeof(p));
    p.pred = W("pred").p; p.pred_rs = W("pred").rs; p.act = act.p; p.act_rs = act.rs; p.apitch = act.pitch; p.dpred = W("dpred").p;
    p.idx = rcsl_mode == RI_SLOTS ? nullptr : d_idx;      // (orl_step: every row of the caller's batch is valid)
    p.B = B; p.A = ad; p.m = mp(); p.m.nm = (int)metric_names.size(); p.slot = 0;
    p.gs_out = gs = gscale_slot();                        // (split precision: the seed kernel publishes the dynamic scale of its backward pass)
    ORL_LAUNCH("rcsl_loss", k_rcsl_loss, dim3(R), dim3(256), p);
  }
  BwdOut bo;
  if (mlp_backward(this, net, x, ah, B, W("dpred"), dah, true, false, 0, 0, nullptr, "rcsl.bwd", &bo, gs)) return -1;
  return adam(ORL_NET_ACTOR, 1, ORL_OPT_ACTOR, make_segs(*net.lay, bo.ks, bo.ks), -1);
}

}  // namespace orl
