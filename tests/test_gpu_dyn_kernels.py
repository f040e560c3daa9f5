"""GPU: the dynamics ensemble's own kernels (csrc/dynamics.hip) -- k_dyn_gather, k_dyn_step_input, k_dyn_nll, k_dyn_nll_reduce,
k_dyn_adam, k_dyn_loss, k_dyn_val_mse, k_dyn_head, k_dyn_sample_next, k_dyn_adv_input, k_dyn_adv_sample, k_dyn_adv_head,
k_dyn_adv_reduce, k_dyn_adv_metrics -- each against a float64 restatement of the same operation ON THE ENGINE'S OWN OPERANDS, read back
through ``Dynamics.debug_read`` after one real call, so that the engine's own launch geometry, strides and row counts are what is tested.

Bar, for EVERY element of every result:  |got - f64| <= 4 x (the first-order fp32 error bound that the restatement propagates through
its own arithmetic, tests/dyn_refs.py on tests/row_refs.py; proven against the numpy oracles and shown to catch sixteen planted defects
in tests/test_dyn_refs_cpu.py).  The input kernels (scaler, pads, targets, kept observations) are held bit for bit.

Cases (tests/dyn_cases.py) move one edge at a time from obs_dim 3, act_dim 2, hidden [32, 32], K 3, elites [2, 0], B 64, one run, with
per-layer decays [0, 0.1, 5e-4], a non-identity scaler and bootstrap indices with repeats that differ per member: train sizes 37 / 1 /
64 / 64 + 5 / 300; obs_dim 1, 2, 4, 63 (D = 2, 3, 5, 64); no reward column; K 1 and K 64; three runs with one inactive; Adam with
non-zero moments at t0 = 0, 1, 999, 10^6; a constant head that puts max - raw and l1 - min on -30 .. 30 across 9 columns with targets on,
next to and 1e3 away from the mean; validate at H = 1, 255, 257; step in all three penalty modes at every shape edge and n = 1, 255,
256, 257; sample_next with 1 and 3 samples; the adversarial pair at (Ba, Bs) = (1, 1), (37, 29), (5, 64), (130, 3) and
K D = 2, 12, 63, 65, 448, 1344, 4096 (4, 2 and 1 waves per workgroup).

Measured worst |err| / bound over the whole module (MI355X; the bar is 4, a correct kernel is expected below 1; the module prints them):
    k_dyn_gather / k_dyn_step_input / k_dyn_adv_input   bit for bit (scaled inputs, zero pads, targets, kept observations)
    k_dyn_nll          dout 0.69, lterm 0.50, gmax 0.73, gmin 0.60
    k_dyn_nll_reduce   nll 0.09, max_logvar gradient 0.24, min_logvar gradient 0.28
    k_dyn_adam         parameter 1.00 (0.9963), exp_avg 0.97, exp_avg_sq 0.98, decay partial sums 0.11; saved_* bit for bit
    k_dyn_loss         loss 0.90
    k_dyn_val_mse      mse 0.17
    k_dyn_head         next_obs 0.97, raw_reward 1.00 (0.9984), reward 0.60 (and raw - coef * penalty bit for bit),
                       penalty: aleatoric 0.21, pairwise-diff 0.64, ensemble_std 0.26
    k_dyn_sample_next  next_obs 0.97
    k_dyn_adv_sample   s 0.98
    k_dyn_adv_head     rowlp 0.13, dout 0.14 (rollout rows) / 0.44 (dataset rows), lterm 0.51, gmax 0.58, gmin 0.56
    k_dyn_adv_reduce   nll 0.09, max_logvar gradient 0.21, min_logvar gradient 0.23, advm 0.81
    k_dyn_adv_metrics  metrics 0.44
Every figure sits at or below 1, i.e. inside the first-order bound itself, a factor 4 inside the bar.

Found by this module: k_dyn_head's ``reward = raw - coef * penalty`` was compiled into one fused multiply-add (``__fmul_rn`` is a plain,
contractible product to the compiler) and differed from the two fp32 operations in the last bit on about a third of the rows; it now
goes through ``dyn_sub_mul`` with contraction switched off.  The two samplers' ``mean + eps * std`` is written the same way in the
kernels; whether it is fused cannot be told from the values (std passes through the device's expf and sqrtf), and either sits inside the
two-rounding bound held here.

Not covered here, with the reason: Adam's step index inside an epoch of several minibatches and the loss of such an epoch (the state
between minibatches cannot be read back; the 64 + 5 case runs with lr 0 so that the last minibatch's operands are known); the decay
partial sums of an inactive run (never written); the Philox streams' statistics (tests/test_gpu_dynamics.py, test_gpu_rambo.py,
test_gpu_mobile.py keep those).
"""
import numpy as np
import pytest

import dyn_cases as dc
import dyn_refs as dr
import row_refs as rr

pytestmark = pytest.mark.gpu
f32 = np.float32

WORST = {}            # kernel.result -> worst |err| / bound seen by this module


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print("\nworst |got - f64| / bound per dynamics-kernel result:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def holds(got, ref, key, *tag):
    return rr.holds(got, ref, (key,) + tuple(tag), WORST, key)


def cat(a, b):
    return rr.BV(np.concatenate([a.v, b.v], -1), np.concatenate([a.e, b.e], -1))


# ---------------------------------------------------------------------------------------------------------------------------------
# engines at the table's shapes
# ---------------------------------------------------------------------------------------------------------------------------------
class Ctx:
    pass


def make(c, seed=0, edge=False):
    from offlinerlkit import _engine
    assert "orl_dyn_debug_read" in _engine.ABI_SYMBOLS and hasattr(_engine.Dynamics, "debug_read"), \
        "this build has no orl_dyn_debug_read: nothing here can be checked"          # before any device object exists
    x = Ctx()
    x.c, x.R, x.K, x.D, x.od, x.ad = c, c["R"], c["K"], c["D"], c["od"], c["ad"]
    x.n_in, x.p0 = c["od"] + c["ad"], dr.rup4(c["od"] + c["ad"])
    cfg = _engine.default_dyn_config(obs_dim=c["od"], act_dim=c["ad"], hidden=list(c["hidden"]), num_ensemble=c["K"],
                                     num_elites=len(c["elites"]), weight_decay=list(c["decays"]), lr=c["lr"], batch_size=c["B"],
                                     logvar_loss_coef=c["coef"], n_runs=c["R"], with_reward=c["with_reward"], seed=seed + 11)
    x.cfg = cfg
    x.eng = eng = _engine.Dynamics(cfg)
    x.flatten = lambda d: _engine._flatten(eng.tensors, d, eng.P)
    x.wd, x.tr = dr.flat_layout(eng.tensors, c["decays"], eng.P)
    rng = x.rng = np.random.default_rng(1000 + seed)
    x.st, x.flat, x.mu, x.sd = [], [], [], []
    for r in range(x.R):
        st = {}
        for name, off, shape in eng.tensors:
            if name in ("max_logvar", "min_logvar"):
                continue
            a = rng.normal(size=shape)
            if name.endswith("weight"):
                a /= np.sqrt(shape[1])
            elif name == "output_layer.bias":
                a[..., :x.D] *= 0.3
                a[..., x.D:] = -1.5 + a[..., x.D:]
            else:
                a *= 0.2
            st[name] = a.astype(f32)
        st["max_logvar"], st["min_logvar"] = dc.logvar_bounds(rng, x.D)
        if edge:
            mean, raw, st["max_logvar"], st["min_logvar"] = dc.edge_head(("y1", "y2")[r])
            st["output_layer.weight"][:] = 0
            st["output_layer.bias"][:] = np.concatenate([mean, raw])
        eng.set_params(r, st)
        mu, sd = dc.scaler(rng, x.n_in)
        eng.set_scaler(r, mu, sd)
        eng.set_elites(r, list(c["elites"]))
        x.st.append(st), x.flat.append(x.flatten(st)), x.mu.append(mu), x.sd.append(sd)
    return x


def moments(x, rng):
    m = (1e-2 * rng.normal(size=x.eng.P)).astype(f32)
    v = ((1e-2 * rng.normal(size=x.eng.P)) ** 2 + 1e-8).astype(f32)
    keep = np.zeros(x.eng.P, bool)                  # the pads between tensors are not part of any tensor dict
    for name, off, shape in x.eng.tensors:
        keep[off:off + int(np.prod(shape))] = True
    return np.where(keep, m, 0).astype(f32), np.where(keep, v, 0).astype(f32)


def inputs(x, rng, n):
    """obs [R, n, od], act [R, n, ad] spread like each run's scaler"""
    z = rng.normal(size=(x.R, n, x.n_in))
    a = np.stack([x.mu[r] + x.sd[r] * z[r] for r in range(x.R)]).astype(f32)
    return np.ascontiguousarray(a[..., :x.od]), np.ascontiguousarray(a[..., x.od:])


def check_adam(x, r, flat0, m0, v0, G, t, lr, state, key, tag):
    """k_dyn_adam on one run's blocks: parameters and both moments against torch.optim.Adam with the decay term, everything outside
    the trainable tensors (saved_*) bit for bit"""
    cfg = x.cfg
    p, m, v = dr.adam(flat0, m0, v0, G, x.wd, x.tr, lr, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, t)
    gp, (gm, gv, gt) = x.flatten(x.eng.get_params(r)), state
    gm, gv = x.flatten(gm), x.flatten(gv)
    holds(gp, p, key + ".param", *tag), holds(gm, m, key + ".exp_avg", *tag), holds(gv, v, key + ".exp_avg_sq", *tag)
    for got, was, what in ((gp, flat0, "param"), (gm, m0, "exp_avg"), (gv, v0, "exp_avg_sq")):
        dr.same_bits(got[~x.tr], was[~x.tr], tag + (what, "outside the trainable tensors"))
    assert (gp[x.tr] != flat0[x.tr]).any() or lr == 0, tag
    assert gt == t, (tag, gt, t)


def check_untouched(x, r, flat0, m0, v0, t0, state, tag):
    gm, gv, gt = state
    dr.same_bits(x.flatten(x.eng.get_params(r)), flat0, tag + ("param",))
    dr.same_bits(x.flatten(gm), m0, tag + ("exp_avg",)), dr.same_bits(x.flatten(gv), v0, tag + ("exp_avg_sq",))
    assert gt == t0, (tag, gt, t0)


def check_nll_rows(x, r, out, T, dout, lterm, gmax, gmin, rows, key, tag):
    D, st = x.D, x.st[r]
    ref = dr.nll_elem(out[..., :D], out[..., D:], T, st["max_logvar"], st["min_logvar"], rows, D)
    holds(dout, cat(ref[0], ref[1]), key + ".dout", *tag)
    holds(lterm, ref[2], key + ".lterm", *tag), holds(gmax, ref[3], key + ".gmax", *tag), holds(gmin, ref[4], key + ".gmin", *tag)


# ---------------------------------------------------------------------------------------------------------------------------------
# learn_epoch: gather, nll, nll_reduce, adam, loss
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,c,train,ex", dc.LEARN, ids=[t[0] for t in dc.LEARN])
def test_learn_epoch(cid, c, train, ex):
    x = make(c, seed=len(cid) + train, edge=ex.get("edge", False))
    eng, rng, R, K, D, B = x.eng, x.rng, x.R, x.K, x.D, c["B"]
    tag = ("learn", cid)
    n_data = 50
    data_in = (3.0 * rng.normal(size=(n_data, x.n_in))).astype(f32)
    data_tg = rng.normal(size=(n_data, D)).astype(f32)
    idx = rng.integers(0, n_data, size=(R, K, train))
    if ex.get("edge"):                     # run r draws from its own half of the data: targets against its own constant head
        half = n_data // 2
        data_tg = np.concatenate([dc.edge_targets(rng, v, half) for v in ("y1", "y2")])
        idx = np.stack([r * half + rng.integers(0, half, size=(K, train)) for r in range(R)])
    else:                                  # repeats, and the first and the last dataset row in the minibatch the taps show
        idx[:, 0, -1] = n_data - 1
        idx[:, K - 1, max(train - 2, 0) if K == 1 else -1] = 0
        if train > 3:
            idx[:, :, -3] = idx[:, :, -1]
    eng.load_data(data_in, data_tg)
    t0 = list(ex.get("t0", [0] * R))
    active = ex.get("active")
    m0, v0 = [], []
    for r in range(R):
        m, v = moments(x, rng) if ex.get("moments") else (np.zeros(eng.P, f32), np.zeros(eng.P, f32))
        eng.set_adam_state(r, eng._unflat(m), eng._unflat(v), t0[r])
        m0.append(m), v0.append(v)
    loss = eng.learn_epoch(idx, active)
    nb = -(-train // B)
    rows = train - (nb - 1) * B
    for r in range(R):
        tg = tag + (r,)
        on = active is None or bool(active[r])
        X, T, out = eng.debug_read(r, "learn.x"), eng.debug_read(r, "learn.t"), eng.debug_read(r, "learn.out")
        assert X.shape == (K, rows, x.p0) and T.shape == (K, rows, D) and out.shape == (K, rows, 2 * D), (tg, X.shape, T.shape, out.shape)
        Xr, Tr = dr.gather(data_in, data_tg, idx[r][:, train - rows:], x.mu[r], x.sd[r])
        dr.same_bits(X, Xr, tg + ("k_dyn_gather X",)), dr.same_bits(T, Tr, tg + ("k_dyn_gather T",))
        assert not X[..., x.n_in:].any(), tg            # the forward GEMM reads the pad columns
        lterm, gmax, gmin = (eng.debug_read(r, "learn." + n) for n in ("lterm", "gmax", "gmin"))
        check_nll_rows(x, r, out, T, eng.debug_read(r, "learn.dout"), lterm, gmax, gmin, rows, "k_dyn_nll", tg)
        st = x.st[r]
        nll, g_mx, g_mn = dr.nll_reduce(lterm, gmax, gmin, st["max_logvar"], st["min_logvar"], c["coef"], rows)
        G = eng.debug_grads(r)
        got_nll = eng.debug_read(r, "learn.nll")
        holds(got_nll, nll, "k_dyn_nll_reduce.nll", *tg)
        holds(G["max_logvar"], g_mx, "k_dyn_nll_reduce.g_max_logvar", *tg), holds(G["min_logvar"], g_mn, "k_dyn_nll_reduce.g_min_logvar", *tg)
        state = eng.adam_state(r)
        if not on:
            check_untouched(x, r, x.flat[r], m0[r], v0[r], t0[r], state, tg + ("inactive",))
            assert loss[r] == 0
            continue
        dec = eng.debug_read(r, "learn.decay")
        assert dec.shape == ((eng.P + 1023) // 1024,)
        if nb == 1 or c["lr"] == 0:        # the decay loss of the weights the last minibatch read
            holds(dec, dr.decay(x.flat[r], x.wd), "k_dyn_adam.decay", *tg)
        if nb == 1:
            holds(loss[r], dr.loss_cell(got_nll, dec), "k_dyn_loss.loss", *tg)
            check_adam(x, r, x.flat[r], m0[r], v0[r], x.flatten(G), t0[r] + 1, c["lr"], state, "k_dyn_adam", tg)
        else:
            assert state[2] == t0[r] + nb
            if c["lr"] == 0:
                dr.same_bits(x.flatten(eng.get_params(r)), x.flat[r], tg + ("lr 0",))
    eng.close()


@pytest.mark.parametrize("H", [1, 255, 257])
def test_validate(H):
    x = make(dc.case(R=2), seed=H)
    eng, rng, D = x.eng, x.rng, x.D
    n_data = 40
    data_in, data_tg = (3.0 * rng.normal(size=(n_data, x.n_in))).astype(f32), rng.normal(size=(n_data, D)).astype(f32)
    eng.load_data(data_in, data_tg)
    idx = rng.integers(0, n_data, size=(x.R, H))
    idx[:, 0], idx[:, -1] = n_data - 1, 0
    mse = eng.validate(idx)
    for r in range(x.R):
        X, T, out = eng.debug_read(r, "step.x"), eng.debug_read(r, "step.t"), eng.debug_read(r, "step.out")
        Xr, Tr = dr.gather(data_in, data_tg, idx[r], x.mu[r], x.sd[r])
        dr.same_bits(X, Xr, ("validate", H, r, "X")), dr.same_bits(T, Tr, ("validate", H, r, "T"))
        assert out.shape == (x.K, H, 2 * D)
        holds(mse[r], dr.val_mse(out, T), "k_dyn_val_mse.mse", "validate", H, r)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# step / sample_next
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,c,n,ex", dc.STEP, ids=[t[0] for t in dc.STEP])
def test_step(cid, c, n, ex):
    x = make(c, seed=3 * len(cid) + n, edge=ex.get("edge", False))
    eng, rng, R, K, D, od = x.eng, x.rng, x.R, x.K, x.D, x.od
    coef = ex.get("step_coef", 2.5)
    obs, act = inputs(x, rng, n)
    for mode in dr.MODES:
        noise = rng.normal(size=(R, K, n, D)).astype(f32)
        midx = rng.choice(np.asarray(c["elites"]), size=(R, n))
        nxt, rew, raw, pen, mo = eng.step(obs, act, noise, midx, mode, coef)
        assert (mo == midx).all()
        for r in range(R):
            tg = ("step", cid, mode, r)
            X, out = eng.debug_read(r, "step.x"), eng.debug_read(r, "step.out")
            dr.same_bits(X, dr.scale_rows(np.concatenate([obs[r], act[r]], 1), x.mu[r], x.sd[r]), tg + ("k_dyn_step_input",))
            assert out.shape == (K, n, 2 * D)
            st = x.st[r]
            ref = dr.head(out, obs[r], noise[r], midx[r], st["max_logvar"], st["min_logvar"], mode, coef)
            holds(nxt[r], ref[0], "k_dyn_head.next_obs", *tg), holds(raw[r], ref[1], "k_dyn_head.raw_reward", *tg)
            holds(pen[r], ref[2], "k_dyn_head.penalty." + mode, *tg), holds(rew[r], ref[3], "k_dyn_head.reward", *tg)
            dr.same_bits(rew[r], raw[r] - f32(coef) * pen[r], tg + ("reward == raw - coef * penalty in fp32",))
            assert (pen[r] >= 0).all() and (coef != 0 or (rew[r] == raw[r]).all())
    with pytest.raises(RuntimeError, match="step.t"):
        eng.debug_read(0, "step.t")
    eng.close()


def test_step_device_draws():
    c = dc.case(R=2)
    x = make(c, seed=5)
    obs, act = inputs(x, x.rng, 300)
    seen = set()
    for _ in range(2):
        nxt, rew, raw, pen, mo = x.eng.step(obs, act, None, None, "aleatoric", 1.0)
        assert np.isin(mo, c["elites"]).all() and np.isfinite(nxt).all() and np.isfinite(rew).all()
        seen |= set(mo.ravel().tolist())
    assert seen == set(c["elites"])
    x.eng.close()


@pytest.mark.parametrize("cid,c,n,S", dc.SAMPLE, ids=[t[0] for t in dc.SAMPLE])
def test_sample_next(cid, c, n, S):
    x = make(c, seed=7 * len(cid) + n)
    eng, rng, R, D, od = x.eng, x.rng, x.R, x.D, x.od
    E = len(c["elites"])
    obs, act = inputs(x, rng, n)
    noise = rng.normal(size=(R, S, E, n, D)).astype(f32)
    got = eng.sample_next(obs, act, S, noise)                 # [R][S][E][n][od]: row (s * E + e) * n + b of the entry point's output
    assert got.shape == (R, S, E, n, od)
    for r in range(R):
        out = eng.debug_read(r, "step.out")
        dr.same_bits(eng.debug_read(r, "step.x"), dr.scale_rows(np.concatenate([obs[r], act[r]], 1), x.mu[r], x.sd[r]), ("sample_next", cid, "x"))
        st = x.st[r]
        holds(got[r], dr.sample_next(out, obs[r], noise[r], c["elites"], st["max_logvar"], st["min_logvar"]),
              "k_dyn_sample_next.next_obs", "sample_next", cid, r)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# RAMBO's adversarial pair
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,c,Ba,Bs,ex", dc.ADV, ids=[t[0] for t in dc.ADV])
def test_adv_forward_update(cid, c, Ba, Bs, ex):
    x = make(c, seed=5 * len(cid) + Ba, edge=ex.get("edge", False))
    eng, rng, R, K, D, od, N = x.eng, x.rng, x.R, x.K, x.D, x.od, Ba + Bs
    lr, aw, t0 = 3e-4, ex.get("adv_weight", 0.37), ex.get("t0", 0)
    active = ex.get("active")
    eng.adv_configure(lr, (0.9, 0.999), 1e-8, aw, Ba, Bs)
    own, m0, v0 = [], [], []
    for r in range(R):
        m, v = moments(x, rng)
        eng.set_adam_state(r, eng._unflat(m), eng._unflat(v), 17)          # learn_epoch's own optimizer: must not move
        own.append((m, v))
        m, v = moments(x, rng)
        eng.set_adv_adam_state(r, eng._unflat(m), eng._unflat(v), t0)
        m0.append(m), v0.append(v)
    obs, act = inputs(x, rng, Ba)
    sl_obs, sl_act = inputs(x, rng, Bs)
    sl_next = (sl_obs + 0.5 * rng.normal(size=sl_obs.shape)).astype(f32)
    sl_rew = rng.normal(size=(R, Bs)).astype(f32)
    if ex.get("edge"):                     # T = sl_next - 0 = the targets against run r's constant head
        sl_obs = np.zeros_like(sl_obs)
        tg_ = np.stack([dc.edge_targets(rng, v, Bs) for v in ("y1", "y2")])
        sl_next, sl_rew = np.ascontiguousarray(tg_[..., :od]), np.ascontiguousarray(tg_[..., od])
    noise = rng.normal(size=(R, K, Ba, D)).astype(f32)
    midx = rng.choice(np.asarray(c["elites"]), size=(R, Ba))
    nxt, rew, mo = eng.adv_forward(obs, act, sl_obs, sl_act, sl_next, sl_rew, noise, midx)
    assert (mo == midx).all()
    with pytest.raises(RuntimeError, match="adv.dout"):
        eng.debug_read(0, "adv.dout")
    adv = (rng.normal(size=(R, Ba)) * 2.0).astype(f32)
    fw = []
    for r in range(R):
        tg = ("adv", cid, r)
        st = x.st[r]
        X, T, ob, S, out = (eng.debug_read(r, "adv." + n) for n in ("x", "t", "obs", "s", "out"))
        Xr, Tr, obr = dr.adv_input(obs[r], act[r], sl_obs[r], sl_act[r], sl_next[r], sl_rew[r], x.mu[r], x.sd[r])
        dr.same_bits(X, Xr, tg + ("k_dyn_adv_input X",)), dr.same_bits(T, Tr, tg + ("k_dyn_adv_input T",))
        dr.same_bits(ob, obr, tg + ("k_dyn_adv_input obs",))
        assert out.shape == (K, N, 2 * D) and S.shape == (Ba, D)
        holds(S, dr.adv_sample(out, ob, noise[r], midx[r], st["max_logvar"], st["min_logvar"]), "k_dyn_adv_sample.s", *tg)
        dr.same_bits(nxt[r], S[:, :od], tg + ("next_obs",)), dr.same_bits(rew[r], S[:, od], tg + ("reward",))
        fw.append((T, ob, S, out))
    metrics = eng.adv_update(adv, active)
    for r in range(R):
        tg = ("adv", cid, r)
        st = x.st[r]
        on = active is None or bool(active[r])
        T, ob, S, out = fw[r]
        dr.same_bits(eng.debug_read(r, "adv.out"), out, tg + ("out kept",))
        dout, lterm, gmax, gmin = (eng.debug_read(r, "adv." + n) for n in ("dout", "lterm", "gmax", "gmin"))
        rowlp = dr.split_hi_lo(eng.debug_read(r, "adv.rowlp"))
        assert dout.shape == (K, N, 2 * D) and lterm.shape == (K, N, D) and rowlp.shape == (Ba,)
        h = dr.adv_head(out, ob, S, T, adv[r], c["elites"], st["max_logvar"], st["min_logvar"], aw)
        holds(rowlp, h["rowlp"], "k_dyn_adv_head.rowlp", *tg)
        holds(dout[:, :Ba], h["dout"][:, :Ba], "k_dyn_adv_head.dout", *tg), holds(dout[:, Ba:], h["dout"][:, Ba:], "k_dyn_adv_head.dout_sl", *tg)
        holds(lterm, h["lterm"], "k_dyn_adv_head.lterm", *tg)
        holds(gmax, h["gmax"], "k_dyn_adv_head.gmax", *tg), holds(gmin, h["gmin"], "k_dyn_adv_head.gmin", *tg)
        not_el = np.setdiff1d(np.arange(K), c["elites"])
        assert not dout[not_el, :Ba].any(), tg                 # weight exactly 0 outside the elites
        nll, g_mx, g_mn, advm = dr.adv_reduce(lterm, gmax, gmin, rowlp, adv[r], st["max_logvar"], st["min_logvar"], Ba)
        G = eng.debug_grads(r)
        got_nll, got_advm = eng.debug_read(r, "learn.nll"), eng.debug_read(r, "adv.advm")
        holds(got_nll, nll, "k_dyn_adv_reduce.nll", *tg), holds(got_advm, advm, "k_dyn_adv_reduce.advm", *tg)
        holds(G["max_logvar"], g_mx, "k_dyn_adv_reduce.g_max_logvar", *tg), holds(G["min_logvar"], g_mn, "k_dyn_adv_reduce.g_min_logvar", *tg)
        state = eng.adv_adam_state(r)
        om, ov, ot = eng.adam_state(r)
        dr.same_bits(x.flatten(om), own[r][0], tg + ("learn_epoch's exp_avg",)), dr.same_bits(x.flatten(ov), own[r][1], tg + ("learn_epoch's exp_avg_sq",))
        assert ot == 17
        if not on:
            check_untouched(x, r, x.flat[r], m0[r], v0[r], t0, state, tg + ("inactive",))
            assert not metrics[r].any()
            continue
        dec = eng.debug_read(r, "learn.decay")
        holds(dec, dr.decay(x.flat[r], x.wd), "k_dyn_adam.decay", *tg)
        holds(metrics[r], dr.adv_metrics(got_nll, dec, got_advm, aw), "k_dyn_adv_metrics.metrics", *tg)
        check_adam(x, r, x.flat[r], m0[r], v0[r], x.flatten(G), t0 + 1, lr, state, "k_dyn_adam", tg)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the tap's refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tap_refusals():
    x = make(dc.case(), seed=9)
    eng, rng = x.eng, x.rng

    def refused(run, name, words, cap=1 << 16):
        with pytest.raises(RuntimeError) as e:
            eng.debug_read(run, name, cap)
        assert name in str(e.value) and words in str(e.value), str(e.value)

    for name in ("learn.x", "learn.nll", "learn.decay", "step.x", "step.out", "step.t"):
        refused(0, name, "nothing recorded")
    for name in ("adv.x", "adv.dout", "adv.rowlp"):
        refused(0, name, "orl_dynadv_configure first")
    for name in ("learn.h", "step.", "adv.nll", "x", "", "learn.x "):
        refused(0, name, "unknown tap")
    refused(1, "learn.x", "run out of range"), refused(-1, "step.x", "run out of range")
    eng.load_data(rng.normal(size=(10, 5)).astype(f32), rng.normal(size=(10, 4)).astype(f32))
    eng.learn_epoch(rng.integers(0, 10, size=(1, 3, 7)))
    assert eng.debug_read(0, "learn.x").shape == (3, 7, 8)
    refused(0, "learn.x", "needs 168 floats", cap=167)
    assert eng.debug_read(0, "learn.x", cap=168).size == 168
    refused(0, "step.out", "nothing recorded")
    eng.adv_configure(1e-3, (0.9, 0.999), 1e-8, 0.1, 4, 3)
    for name in ("adv.x", "adv.out", "adv.dout", "adv.advm"):
        refused(0, name, "nothing recorded")
    obs, act = inputs(x, rng, 4)
    eng.step(obs, act, rng.normal(size=(1, 3, 4, 4)).astype(f32), np.zeros((1, 4), np.int64))
    assert eng.debug_read(0, "step.out").shape == (3, 4, 8)
    refused(0, "step.t", "nothing recorded")
    eng.close()
