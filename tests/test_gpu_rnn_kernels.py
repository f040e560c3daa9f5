"""GPU: the RNN dynamics kernels (csrc/rnn_dynamics.hip) -- k_rnn_gather, k_rnn_scan_fwd, k_rnn_ln_fwd, k_rnn_loss, k_rnn_ln_bwd,
k_rnn_swish_bwd, k_rnn_scan_bwd, k_rnn_colsum_part, k_rnn_colsum_fin, k_rnn_slab_sum, k_rnn_adam and every matrix product between
them -- each against the float64 restatement of the same operation (tests/rnn_refs.py) ON THE ENGINE'S OWN OPERANDS, read back through
``RnnDynamicsEngine.debug_read`` after one real training step and one real eval pass, so that the engine's own launch geometry,
pitches, run strides and row counts are what is tested.

Bar, for EVERY element of every result: |got - f64| <= 4 x (the first-order fp32 error bound that the restatement propagates through
its own arithmetic; proven against the oracle and autograd, and shown to catch 21 planted defects, in tests/test_rnn_refs_cpu.py).
The gathered rows, the saved h_{t-1}, the r | z columns shared by dgi and dgh, the two levels of column sums and the slab sum are held
bit for bit.

The steps run with ``debug_keep`` on, which gives every backward stage a matrix of its own; the first test shows that this changes no
bit of any result, so what is tested is what runs.  Cases: tests/rnn_kernel_cases.py (A .. H, case C's saturating twin, and case B as
run 1 of a two-run object).  The worst err / bound per check is printed by each test and, over the module, at its end; the figures
measured on an MI355X are in DESIGN.md ("Per-element tests of the RNN dynamics kernels")."""
import numpy as np
import pytest

import rnn_cases as rc
import rnn_kernel_cases as kc
import rnn_refs as rf
from test_rnn_refs_cpu import moments_of

pytestmark = pytest.mark.gpu

WORST = {}            # check -> worst |err| / bound seen by this module


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print("\nworst |got - f64| / bound per RNN-kernel check:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    by = {}
    for k, v in WORST.items():
        by[k.split(".")[0]] = max(by.get(k.split(".")[0], 0.0), v)
    print("per kernel:", {k: round(v, 4) for k, v in sorted(by.items())})


class Ctx:
    pass


def make(name, runs=1, keep=True, philox=False):
    """an engine at a case's shape with known parameters, moments and step count, its data loaded"""
    from offlinerlkit import _engine
    assert "orl_rnn_debug_keep" in _engine.ABI_SYMBOLS and hasattr(_engine.RnnDynamicsEngine, "debug_keep"), \
        "this build has no orl_rnn_debug_keep: nothing here can be checked"          # before any device object exists
    x = Ctx()
    x.c = c = kc.case(name[0])
    x.R, x.T, x.lr, x.t0, x.rows = runs, c["T"], 1e-3, 3, c["B"] * c["T"]
    cfg = _engine.default_rnn_config(input_dim=c["input_dim"], output_dim=c["output_dim"], hidden=c["hidden"], rnn_num_layers=c["L"],
                                     dropout_rate=c["p"], batch_size=c["B"], max_seq_len=c["T"], lr=x.lr, seed=5, n_runs=runs)
    x.eng = eng = _engine.RnnDynamicsEngine(cfg)
    x.tensors = eng.tensors()
    assert [(k, s) for k, _, s in x.tensors] == rc.shapes(c)
    x.data = kc.data(c)
    x.P, x.before = [], []
    for r in range(runs):
        P = rc.make_params(c, seed_offset=50 * r)
        if name == "Csat":
            P, xs = kc.saturated(P, x.data[0])
            x.data = (xs,) + x.data[1:]
        flat = _engine._flatten(x.tensors, P, eng.floats)
        m, v = moments_of(eng.floats, x.tensors, 3 + r)
        for which, a in ((eng.PARAMS, flat), (eng.EXP_AVG, m), (eng.EXP_AVG_SQ, v)):
            eng.set(which, a, r)
        x.P.append(P), x.before.append((flat, m, v))
    eng.step_count = x.t0
    eng.load_data(*x.data)
    if keep:
        eng.debug_keep(True)
    x.forced = c["p"] > 0 and not philox
    return x


def step(x, rows=None):
    """one training step of every run on its own rows (and forced masks) -> the losses"""
    c = x.c
    rows = c["B"] if rows is None else rows
    x.idx = np.stack([np.roll(kc.indices(c, rows), r) for r in range(x.R)])
    x.drop = np.stack([kc.drop_masks(c, rows, seed=r) for r in range(x.R)]) if x.forced else None
    x.rows = rows * c["T"]
    return x.eng.step_runs(x.idx, x.drop)


def tap(x, name, run=0, rows=None):
    rows = x.rows if rows is None else rows
    n = 1 if name == "loss" or name.startswith("slab.") else (rows + rf.CHUNK - 1) // rf.CHUNK if name == "chunk" else rows
    return x.eng.debug_read(name, run=run).reshape(n, -1)


def all_names(c):
    L, nb = c["L"], len(c["hidden"]) - 1
    names = ["x0", "tgt", "msk", "zmerge", "dpred", "dx", "dzm", "dcat", "part", "chunk", "slab.0", "pred", "in", "merge", "loss"]
    for l in range(L):
        names += [f"{k}.{l}" for k in ("gi", "gru", "r", "z", "n", "hn", "hp", "dgi", "dgh")] + ([f"dxl.{l}"] if l else [])
    for s in range(nb + 1):
        names += [f"zpre.{s}", f"act.{s}", f"drop.{s}", f"dz.{s}"] + ([f"mask.{s}"] if c["p"] > 0 else [])
    for i in range(nb):
        names += [f"block.{i}", f"du.{i}", f"dt.{i}"]
    return names


# ---- 1. the keep switch changes no bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "F"])
def test_keep_switch_changes_no_bit(name):
    """keep on against keep off: loss, gradients, parameters and both moments after the step are the same bits, and so is every tap
    that both modes can read (with keep off: all but the stages a later one overwrote)"""
    a, b = make(name, keep=True), make(name, keep=False)
    try:
        la, lb = step(a), step(b)
        assert np.array_equal(la, lb) and np.array_equal(a.eng.debug_grads(), b.eng.debug_grads())
        for w in (a.eng.PARAMS, a.eng.EXP_AVG, a.eng.EXP_AVG_SQ):
            assert np.array_equal(a.eng.get(w), b.eng.get(w)), w
        both, only_keep = 0, []
        for nm in all_names(a.c):
            got = tap(a, nm)
            try:
                other = tap(b, nm)
            except RuntimeError as e:
                assert "overwritten" in str(e), (nm, str(e))
                only_keep.append(nm)
                continue
            assert np.array_equal(got, other), nm
            both += 1
        print(f"case {name}: {both} taps identical in both modes; readable with keep only: {only_keep}")
        c = a.c
        want = [f"{k}.{l}" for l in range(1, c["L"]) for k in ("dgi", "dgh")] + [f"dz.{s}" for s in range(1, len(c["hidden"]))]
        want += [f"{k}.{i}" for i in range(1, len(c["hidden"]) - 1) for k in ("du", "dt")]
        assert sorted(only_keep) == sorted(want)
        # switching off again gives the shared buffers back: the next step is the same bits as the other engine's next step
        a.eng.debug_keep(False)
        with pytest.raises(RuntimeError, match="nothing recorded"):
            tap(a, "dpred")
        assert np.array_equal(step(a), step(b)) and np.array_equal(a.eng.debug_grads(), b.eng.debug_grads())
        assert np.array_equal(tap(a, "dgi.0"), tap(b, "dgi.0"))
    finally:
        a.eng.close(); b.eng.close()


# ---- 2. every kernel, per element ------------------------------------------------------------------------------------------------------------
def check_run(x, r, rec):
    c, eng, P = x.c, x.eng, x.P[r]

    def rd(name):
        return tap(x, name, r)
    want = rf.gather(x.data, x.idx[r])
    for k, w in zip(("x0", "tgt", "msk"), want):
        rec.same(rd(k), w, "k_rnn_gather." + k)
    if x.forced:
        for s in range(len(c["hidden"])):
            rec.same(rd(f"mask.{s}"), x.drop[r][s], "forced_mask", s)
    grads = eng.debug_grads(r)
    ns = rf.n_slabs(eng.floats, c["B"] * c["T"], x.rows)
    slabs = [rd(f"slab.{k}")[0] for k in range(ns)]
    if ns < 8:
        with pytest.raises(RuntimeError, match="slabs"):
            rd(f"slab.{ns}")
    rf.check_forward(rd, P, c, rec, train=True)
    rf.check_backward(rd, P, c, rec, grads, x.tensors, slabs)
    after = tuple(eng.get(w, r) for w in (eng.PARAMS, eng.EXP_AVG, eng.EXP_AVG_SQ))
    rf.check_adam(x.before[r], after, grads, x.t0 + 1, x.lr, rec)
    return ns


@pytest.mark.parametrize("name", kc.NAMES + ["Csat", "B2"])
def test_every_kernel_holds_per_element(name):
    runs = 2 if name == "B2" else 1
    x = make(name, runs=runs, philox=name == "F")
    try:
        losses = step(x)
        rec = rf.Rec()
        ns = check_run(x, runs - 1, rec)
        assert float(tap(x, "loss", runs - 1)[0, 0]) == float(losses[runs - 1])
        if name == "E":
            assert ns == 2 and tap(x, "chunk").shape[0] == 9 and x.rows % rf.CHUNK == 16
        # the eval launch of the scans (no saves) and the forward products at another row count, with the parameters Adam just wrote
        from offlinerlkit import _engine
        half = max(1, x.c["B"] // 2)
        x.eng.forward_runs(x.data[0][x.idx[runs - 1][:half]], run=runs - 1)
        Pn = _engine._unflatten(x.tensors, x.eng.get(x.eng.PARAMS, runs - 1))
        rf.check_forward(lambda nm: tap(x, nm, runs - 1, half * x.T), Pn, x.c, rec, train=False)
        by = {}
        for k, v in rec.worst.items():
            WORST[k] = max(WORST.get(k, 0.0), v)
            by[k.split(".")[0]] = max(by.get(k.split(".")[0], 0.0), v)
        print(f"case {name} ({ns} slab(s)): worst err / bound per kernel", {k: round(v, 3) for k, v in sorted(by.items())})
        print("   per check", {k: round(v, 3) for k, v in sorted(rec.worst.items())})
        rec.finish()
    finally:
        x.eng.close()


# ---- 3. refusals of the new names ----------------------------------------------------------------------------------------------------------
def test_new_taps_are_refused_by_name():
    x = make("B", runs=2, keep=False)
    try:
        for nm in ("dgi.0", "r.0", "tgt", "part", "slab.0"):
            with pytest.raises(RuntimeError, match="nothing recorded"):
                tap(x, nm)
        step(x)
        for nm in ("dgi.2", "dxl.0", "dxl.2", "du.2", "dz.3", "zpre.3", "slab.8", "slab.x", "hp.2", "dgi", "dcat.0"):
            with pytest.raises(RuntimeError, match="unknown tap"):
                tap(x, nm)
        for nm in ("dgi.1", "dgh.1", "dz.1", "dz.2", "du.1", "dt.1"):
            with pytest.raises(RuntimeError, match="overwritten " + nm.replace(".", r"\.")):
                tap(x, nm)
        for nm in ("dgi.0", "dgh.0", "dz.0", "du.0", "dt.0", "dxl.1"):           # the last writers stay readable
            assert tap(x, nm, 1).shape[0] == x.rows
        with pytest.raises(RuntimeError, match="slabs"):
            tap(x, "slab.1")
        with pytest.raises(RuntimeError, match="run out of range"):
            tap(x, "dpred", 2)
        x.eng.forward_runs(x.data[0][:4], run=0)
        for nm in ("r.0", "hp.1", "zpre.0", "zmerge", "tgt", "msk", "dpred", "dgi.0", "part", "chunk", "slab.0", "dz.0"):
            with pytest.raises(RuntimeError, match="only a training step"):
                tap(x, nm, 0, 4 * x.T)
        assert tap(x, "gi.0", 0, 4 * x.T).shape == (4 * x.T, 3 * x.c["H"]) and tap(x, "x0", 0, 4 * x.T).shape == (4 * x.T, x.c["input_dim"])
        with pytest.raises(RuntimeError, match="did not compute run 1"):
            tap(x, "gi.0", 1, 4 * x.T)
    finally:
        x.eng.close()


# ---- 4. a short batch after a full one -----------------------------------------------------------------------------------------------------
def test_short_batch_after_a_full_one_reads_nothing_stale_through_the_new_taps():
    a, b = make("B"), make("B")
    try:
        step(a)
        for w in (a.eng.PARAMS, a.eng.EXP_AVG, a.eng.EXP_AVG_SQ):
            b.eng.set(w, a.eng.get(w))
        b.eng.step_count = a.eng.step_count
        from offlinerlkit import _engine
        Pn = _engine._unflatten(a.tensors, a.eng.get(a.eng.PARAMS))
        la, lb = step(a, 3), step(b, 3)
        assert np.array_equal(la, lb) and np.array_equal(a.eng.debug_grads(), b.eng.debug_grads())
        for nm in all_names(a.c):
            u, v = tap(a, nm), tap(b, nm)
            assert np.array_equal(u, v), nm
            if nm not in ("loss", "chunk", "slab.0"):
                assert u.shape[0] == 3 * a.T, nm
        # ... and the short step itself holds per element on the engine that ran the full one first
        rec = rf.Rec()
        for k, w in zip(("x0", "tgt", "msk"), rf.gather(a.data, a.idx[0])):
            rec.same(tap(a, k), w, "k_rnn_gather." + k)
        rf.check_forward(lambda nm: tap(a, nm), Pn, a.c, rec, train=True)
        rf.check_backward(lambda nm: tap(a, nm), Pn, a.c, rec, a.eng.debug_grads(), a.tensors, [tap(a, "slab.0")[0]])
        rec.finish()
    finally:
        a.eng.close(); b.eng.close()
