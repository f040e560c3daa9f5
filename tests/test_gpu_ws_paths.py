"""GPU: every instantiation and every pipeline depth of the weight-stationary kernels (csrc/ws_*.hip), one launch per test through the
unit tap (orl_debug_ws), against the float64 numpy references of tests/ws_cases.py.  Shapes are the smallest the support predicates
admit (K = N = 256, M = 256 / 288 / 352 rows = 8 / 9 / 11 row groups, at most six problems), so that 32 wrong rows of one workgroup
cannot hide under an end-to-end bar.  Bars: componentwise, C = bound(precision) of tests/test_gpu_backward_f64.py (ws_cases.py).
After EVERY launch the words outside the logical results (pad columns, guard rows, slabs >= per_z, the space between problems, an
h0 that was to be discarded) still hold the sentinel bit for bit and every operand comes back bit-identical (ws_cases.check_guards)."""
import numpy as np
import pytest

import ws_cases as w

pytestmark = pytest.mark.gpu


def _launch(kw, name=None):
    c = w.build(**kw)
    w.run(c)
    if name is not None:
        assert c.report["flavour"] == name, ("the launch took another instantiation", c.report["flavour"], name)
    return c


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print("\nworst |got - f64| / (C * abs-sum) per stage:", {k: round(v, 4) for k, v in sorted(w.MEASURED.items())})


@pytest.mark.parametrize("name", sorted(w.FLAVOURS))
def test_every_instantiation_runs_once(name):
    """M = 256, per_z = 2, two problems: each entry of the tap's table of instantiations"""
    w.check(_launch(w.FLAVOURS[name], name))


@pytest.mark.parametrize("name,M,per_z", w.depth_cases(), ids=[f"{n}-M{M}-pz{p}" for n, M, p in w.depth_cases()])
def test_pipeline_depth(name, M, per_z):
    """workgroups that own 1, 2, 3, 4, 6|5, 2|1, 4|4|3 and 8 row groups: each takes its own way through prologue, steady body and drain
    and ends on another buffer parity; every split-K slab is held to the reference of exactly the rows its workgroup owns"""
    w.check(_launch(w.depth_kwargs(name, M, per_z), name))


@pytest.mark.parametrize("label,name,over", w.geometry_cases(), ids=[f"{n}-{l}".replace(" ", "_") for l, n, o in w.geometry_cases()])
def test_operand_geometry(label, name, over):
    """what the support predicates admit and the engines never set: in0 / x0_pitch at their ends, EnsembleLinear weight and slab strides,
    3 x 2 problems whose strides are no multiples of each other, padded pitches, strided tq / dq, the dynamic gradient scale"""
    w.check(_launch(w.geometry_kwargs(name, over), name))


# ---- flavours that must agree bit for bit ----
@pytest.mark.parametrize("f32", [0, 1])
def test_recompute_rebuilds_the_forwards_h0_bit_for_bit(f32):
    """ws_wgrad<4> rebuilds h0 = relu(X0 W0^T + b0) "with the forward's instruction sequence": its dW / db equal those of the plain
    flavour on the h0 the fused forward stored"""
    tag = "ws_wgrad32" if f32 else "ws_wgrad"
    rec = _launch(dict(w.FLAVOURS[f"{tag}<4>"], M=288, per_z=3, seed=41), f"{tag}<4>")
    fwd = w.build(**dict(w.FLAVOURS[f"ws_fwd<0,1,0,1,{f32},1>"], M=288, per_z=3, seed=42))
    for k in ("X0", "W0", "b0"):
        w.set_data(fwd, k, rec.d[k])
    w.run(fwd)
    w.check(fwd)
    pl = w.build(**dict(w.FLAVOURS[f"{tag}<3>"], M=288, per_z=3, seed=43))
    w.set_data(pl, "dZ", rec.d["dZ"])
    w.set_data(pl, "H0", fwd.arrays["X"].get()[:, :, 0])
    w.run(pl)
    for k in ("dW", "db"):
        assert np.array_equal(rec.arrays[k].raw, pl.arrays[k].raw), (k, "recompute and stored h0 give different bits")
    w.check(pl)
    w.check(rec)


@pytest.mark.parametrize("pair", [("ws_fwd<1,1,0,0,0,1>", "ws_fwd<1,1,0,0,0,0>"), ("ws_fwd<1,1,0,0,1,1>", "ws_fwd<1,1,0,0,1,0>"),
                                  ("ws_fwd<0,1,0,1,0,1>", "ws_fwd<0,1,0,1,0,0>"), ("ws_fwd3<1,0,1,1,0>", "ws_fwd3<1,0,0,1,0>"),
                                  ("ws_fwd3<0,1,1,1,0>", "ws_fwd3<0,1,0,1,0>")])
def test_storing_and_discarding_forward_agree_bit_for_bit(pair):
    """x0_discard only drops the h0 store: tq, the activation and both masks are the same bits"""
    a = _launch(dict(w.FLAVOURS[pair[0]], M=352, per_z=3, seed=44), pair[0])
    b = _launch(dict(w.FLAVOURS[pair[1]], M=352, per_z=3, seed=44), pair[1])
    for k in a.arrays:
        if a.arrays[k].result and k != "X":
            assert np.array_equal(a.arrays[k].raw, b.arrays[k].raw), (k, "storing and discarding forward differ")
    w.check(a)
    w.check(b)
