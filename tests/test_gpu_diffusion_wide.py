"""GPU: DiffusionBC (csrc/diffusion.hip) against the float64 numpy oracle at the shapes it ships with -- GroupNorm groups of 33 .. 512
channels (every ``lane + 64 j`` register slab, the partial and the exact one), 1 and 16 groups, embedding / action / observation loops
that wrap a wave, the CFG_MID / CFG_BIG tiles and the K >= 1024 weight-gradient tiles on stacked and column-sliced operands, 3 and 4
gradient terms, row sums over 90 and 2048 rows, Adam / EMA at large step counts, the DDPM update on both sides of its clip.

Cases, references, bars and check functions: tests/diffusion_wide_cases.py; tests/test_diffusion_wide_cpu.py proves them on the CPU (the
oracle against float64 autograd, the checks against six planted defects).  The float64 oracle is fed the engine's own e0 tap, so every
stage downstream is compared on the same input, and e0 is held to its own derived bound.

Measured err / bar on an MI355X (bar = 4 x D32 for stages and gradients, 4 x the restatement's bound for e0, the loss cell, Adam and
the EMA; a ratio above 1 fails).  No kernel defect was found: every ratio is below 1 on the first run.
  A        e0 0.11, gf 0.57, mc 0.31, film 0.34, y1.0 .. out.11: 0.34 0.33 0.25 0.35 0.24 0.34 0.30 0.35 0.36 0.37 0.43 0.25 0.18 0.26 0.40
           0.40 0.46 0.54 0.70 0.43 0.51 0.63 0.32 0.43, yf 0.31, pred 0.56, gradients 0.35, loss cell 0.03
  B        e0 0.11, gf 0.45, mc 0.25, film 0.25, y1.0 .. out.3: 0.23 0.36 0.33 0.28 0.52 0.35 0.30 0.32, yf 0.39, pred 0.39, gradients 0.39,
           loss cell 0.01
  C        e0 0.11, gf 0.62, mc 0.57, film 0.26, y1.0 .. out.3: 0.24 0.38 0.27 0.41 0.21 0.46 0.62 0.37, yf 0.35, pred 0.22, gradients 0.26,
           loss cell 0.01
  D        e0 0.11, gf 0.24, mc 0.48, film 0.56, y1.0 .. out.7: 0.30 0.39 0.46 0.25 0.33 0.36 0.58 0.29 0.35 0.34 0.32 0.29 0.38 0.27 0.50
           0.65, yf 0.48, pred 0.35, gradients 0.30, loss cell 0.00
  E        e0 0.11, gf 0.20, mc 0.19, film 0.28, y1.0 .. out.7: 0.18 0.12 0.17 0.44 0.45 0.43 0.11 0.25 0.30 0.38 0.25 0.87 0.64 0.42 0.65
           0.45, yf 0.15, pred 0.23, gradients 0.15, loss cell 0.01
  F        e0 0.11, gf 0.50, mc 0.24, film 0.22, y1.0 .. out.7: 0.40 0.38 0.35 0.22 0.25 0.21 0.24 0.21 0.59 0.22 0.25 0.27 0.19 0.35 0.19
           0.36, yf 0.59, pred 0.37, gradients 0.69, loss cell 0.01
  F short  e0 0.11, gf 0.40, mc 0.32, film 0.30, y1.0 .. out.7: 0.34 0.23 0.28 0.20 0.38 0.33 0.28 0.26 0.35 0.24 0.20 0.20 0.38 0.90 0.32
           0.32, yf 0.18, pred 0.17, gradients 0.29, loss cell 0.03
  G        e0 0.11, gf 0.22, mc 0.19, film 0.22, y1.0 .. out.3: 0.34 0.34 0.39 0.39 0.21 0.36 0.51 0.38, yf 0.42, pred 0.29, gradients 0.30,
           loss cell 0.00
  H        e0 0.07, gf 0.46, mc 0.25, film 0.15, y1.0 .. out.7: 0.30 0.18 0.46 0.23 0.17 0.32 0.34 0.34 0.13 0.37 0.55 0.39 0.66 0.34 0.29
           0.34, yf 0.43, pred 0.50, gradients 0.29, loss cell 0.01
  I        e0 0.11, gf 0.53, mc 0.25, film 0.29, y1.0 .. out.11: 0.46 0.26 0.38 0.29 0.16 0.33 0.51 0.29 0.21 0.28 0.31 0.31 0.82 0.34 0.46
           0.27 0.09 0.42 0.22 0.34 0.28 0.43 0.44 0.32, yf 0.43, pred 0.76, gradients 0.43, loss cell 0.02
  D, N 100 e0 0.11; pred 7.6e-7 of scale (gate 1e-4)
  Adam/EMA k = 0, 1, 2, 215443, 215444, 1000000: parameters 0.25 at every k, EMA 0.10 0.08 0.21 0.25 0.25 0.25, exp_avg 0.24, exp_avg_sq 0.24
  sampling 2047 rows 0.39, 2048 rows 0.41 (D32 3.0e-5 / 2.1e-5); the 4-row calls 0.005 / 0.007, bitwise equal to rows 0 .. 3 of the large calls
D32 is computed by the test on the host that runs it (numpy's fp32 products), so a ratio moves with the host's BLAS; the engine's side of it
is deterministic.
"""
import numpy as np
import pytest

import diffusion_oracle as orc
import diffusion_wide_cases as wc
from helpers import scale_err
from test_gpu_diffusion import make_engine, pack, zero_like_grads

pytestmark = pytest.mark.gpu


def observe(eng, P, c, batch):
    """one teacher-forced step -> the taps, the loss and the gradients in the layout of ``wc.run_oracle``"""
    idx, t, eps = batch
    rows = len(idx)
    loss = eng.step(idx, t, eps)
    plan, _ = orc.block_plan(c["act_dim"], c["down_dims"])

    def rd(name, cols):
        return eng.debug_read(name, cap=rows * cols).reshape(rows, cols)
    got = dict(e0=rd("e0", c["dsed"]), gf=rd("gf", c["dsed"] + c["obs_dim"]), mc=rd("mc", c["dsed"] + c["obs_dim"]),
               film=rd("film", sum(2 * p[2] for p in plan)), yf=rd("yf", c["down_dims"][0]), pred=rd("pred", c["act_dim"]),
               eps=rd("eps", c["act_dim"]), x_t=rd("x_t", c["act_dim"]), t=eng.debug_read("t"), loss=loss)
    for b, p in enumerate(plan):
        got[f"y1.{b}"], got[f"out.{b}"] = rd(f"y1.{b}", p[2]), rd(f"out.{b}", p[2])
    full = zero_like_grads(eng, P)
    for k, v in full.items():                              # the off-centre taps: exactly zero
        if v.ndim == 3 and v.shape[2] > 1:
            assert not np.delete(v, v.shape[2] // 2, axis=2).any()
    got["grads"] = wc.centre_taps(full)
    return got


def check_engine_step(eng, ref, i, tag):
    c, P, batch = ref["c"], ref["P"], ref["batches"][i]
    got = observe(eng, P, c, batch)
    idx, t, eps = batch
    assert got["loss"] == float(eng.debug_read("loss")[0]) and np.isfinite(got["loss"])
    assert np.array_equal(got["eps"], eps) and np.array_equal(got["t"], t.astype(np.float32))
    assert scale_err(got["x_t"], ref["o64"][i]["x_t"]) < 1e-6
    ratios = {}
    wc.check_e0(got["e0"], t, c["dsed"], tag, ratios)
    o64 = wc.run_oracle(P, c, ref["data"], batch, np.float64, e0=got["e0"])
    wc.check_step(got, o64, ref["D32"][i], c, tag, ratios)
    print("    " + ", ".join(f"{k[len(tag) + 1:]} {v:.2f}" for k, v in ratios.items()))
    return got


@pytest.mark.parametrize("name", wc.STEP_CASES)
def test_one_step_against_the_float64_oracle(name):
    ref = wc.reference(name)
    c = ref["c"]
    eng, P = make_engine(c)
    try:
        assert all(np.array_equal(P[k], ref["P"][k]) for k in P)
        flat = pack(eng, P)
        check_engine_step(eng, ref, 0, name)
        # the first step has lr 0: the parameters are untouched, the EMA (decay 0) equals them
        assert np.array_equal(eng.get(eng.PARAMS), flat) and np.array_equal(eng.get(eng.EMA), flat) and eng.step_count == 1
        if name == "F":                                    # its short batch of 10 rows on the same (still unchanged) parameters
            assert len(ref["batches"][1][0]) == 10
            check_engine_step(eng, ref, 1, "F short")
    finally:
        eng.close()


def test_embedding_and_output_at_a_hundred_iterations():
    """case D with N = 100: arguments up to 99 in sinf / cosf; the e0 tap against its bound and pred against the project's gate"""
    ref = wc.reference("D100")
    c, P, batch = ref["c"], ref["P"], ref["batches"][0]
    eng, _ = make_engine(c)
    try:
        idx, t, eps = batch
        t = t.copy()
        t[2:] = [c["N"] - 2, 50, 73, 97][:len(t) - 2]      # the far end of the range, besides the forced 0 and N - 1
        batch = (idx, t, eps)
        got = observe(eng, P, c, batch)
        ratios = {}
        wc.check_e0(got["e0"], t, c["dsed"], "D100", ratios)
        o64 = wc.run_oracle(P, c, ref["data"], batch, np.float64, e0=got["e0"])
        err = scale_err(got["pred"], o64["pred"])
        print(f"D100: e0 err / bar {ratios['D100 e0']:.3f}; pred scale_err {err:.2e}")
        assert err < wc.GATE
    finally:
        eng.close()


def test_taps_and_shapes_that_are_refused():
    from offlinerlkit import _engine
    base = dict(obs_dim=5, act_dim=3, step_embed_dim=16, kernel_size=1, batch_size=6)
    for over, msg in ((dict(n_groups=1, down_dims=[520]), "wider than 512"), (dict(n_groups=17, down_dims=[136]), "n_groups must be in")):
        assert msg in wc.legal(dict(wc.CASES["B"], **over))
        with pytest.raises(RuntimeError, match=msg):
            _engine.Diffusion(_engine.default_diffusion_config(**dict(base, **over)))
    ref = wc.reference("H")
    eng, _ = make_engine(ref["c"])
    try:
        with pytest.raises(RuntimeError, match="nothing recorded"):
            eng.debug_read("y1.0")
        eng.step(*ref["batches"][0])
        nb = len(orc.block_plan(ref["c"]["act_dim"], ref["c"]["down_dims"])[0])
        assert eng.debug_read(f"out.{nb - 1}").size == 6 * 32 and eng.debug_read("y1.2").size == 6 * 16
        for bad in (f"y1.{nb}", f"out.{nb}", "out.-1", "y1.", "out.1x", "y1.01", "y1.99999", "y2.0", "e1", "bogus"):
            with pytest.raises(RuntimeError, match="unknown tap"):
                eng.debug_read(bad)
    finally:
        eng.close()


@pytest.mark.parametrize("k", wc.ADAM_STEPS)
def test_adam_and_ema_at_step(k):
    """random parameter, EMA and moment blocks, the step counter at k, an lr table that ends at lr[k] (its neighbour is half of it):
    the four blocks after one step against the float64 restatement applied to the engine's own gradient"""
    ref = wc.reference("H")
    eng, _ = make_engine(ref["c"])
    try:
        lr = wc.lr_table_for(k)
        eng.set_lr(lr)
        before = wc.adam_blocks(eng.floats, 40 + k % 101)
        which = (eng.PARAMS, eng.EMA, eng.EXP_AVG, eng.EXP_AVG_SQ)
        for w, x in zip(which, before):
            eng.set(w, x)
        eng.step_count = k
        loss = eng.step(*ref["batches"][0])
        g = eng.debug_grads()
        assert np.isfinite(loss) and np.isfinite(g).all() and np.count_nonzero(g) > 0.9 * g.size
        ratios = wc.check_adam_ema([eng.get(w) for w in which], before, g, lr[k], k, "H")
        print(f"Adam / EMA at k = {k} (decay {orc.ema_decay(k)!r}): err / bar " + ", ".join(f"{n} {v:.3f}" for n, v in ratios.items()))
        assert eng.step_count == k + 1
        with pytest.raises(RuntimeError, match="past the learning-rate table"):
            eng.step(*ref["batches"][0])
    finally:
        eng.close()


@pytest.mark.parametrize("rows", [2047, 2048])
def test_sampling_many_rows(rows):
    """net C, N = 3, teacher-forced z: 2047 rows run the 64 x 64 tiles past 1024 small tiles (CFG_MID), 2048 the 64 x 256 tile (CFG_BIG);
    rows 0 .. 3 also as a call of their own (16 x 64 tiles)"""
    s = wc.sample_reference(rows)
    eng, P = make_engine(s["c"])
    try:
        clipped = np.abs(s["x0"]) > 1
        assert 0.1 <= clipped.mean() <= 0.9 and (s["x0"] < -1).any() and (s["x0"] > 1).any()
        got = eng.sample(s["obs"], s["noise"].reshape(rows, -1), z=s["z"])
        wc.check_sample(got, s["a64"], s["D32"], f"sample {rows}")
        four = eng.sample(s["obs"][:4], s["noise"].reshape(rows, -1)[:4], z=np.ascontiguousarray(s["z"][:, :4]))
        scale, bar = np.abs(s["a64"]).max(), min(wc.BAR * s["D32"], wc.GATE)
        e4 = np.abs(four - s["a64"][:4]).max() / scale / bar
        print(f"    the 4-row call: err / bar {e4:.3f}; against rows 0 .. 3 of the {rows}-row call {np.abs(four - got[:4]).max() / scale:.2e}")
        assert e4 <= 1.0 and np.abs(four - got[:4]).max() / scale <= 2 * bar
        assert eng.step_count == 0 and np.array_equal(eng.get(eng.PARAMS), pack(eng, P))
    finally:
        eng.close()


def test_device_draws_at_a_wide_action():
    """case D without teacher forcing: 67 action columns are 17 Philox quads per row, past the 16 a wave's first trip covers"""
    from test_gpu_learn_n import _moments_ok
    ref = wc.reference("D")
    c = ref["c"]
    eng, _ = make_engine(c, total_steps=8)
    try:
        idx = np.arange(c["B"], dtype=np.int64)
        es, ts = [], []
        for _ in range(8):
            eng.step(idx)
            es.append(eng.debug_read("eps").reshape(c["B"], c["act_dim"])); ts.append(eng.debug_read("t"))
        e, t = np.stack(es).astype(np.float64), np.concatenate(ts)
        assert t.min() >= 0 and t.max() <= c["N"] - 1 and len(np.unique(t)) > 3
        assert len(np.unique(e)) > 0.99 * e.size            # no quad, row or step repeats another
        assert not np.array_equal(e[:, :, 64:67], e[:, :, 0:3]) and not np.array_equal(e[:, :, 64:67], e[:, :, 60:63])
        _moments_ok(e.ravel(), "eps")
        _moments_ok(e[:, :, 64:].ravel(), "eps of the columns past 64")
    finally:
        eng.close()
