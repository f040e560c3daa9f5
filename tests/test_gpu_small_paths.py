"""GPU: every instantiation of the few-rows kernels -- small_fwd_kernel<F32, QG> (csrc/small_fwd.hip) and small_abwd_kernel<F32>
(csrc/small_bwd.hip) -- one launch per test through the unit tap (orl_debug_small), against the float64 numpy references of
tests/small_cases.py.  Shapes are the smallest the support predicates admit (M = 32 / 64 / 96 rows = 1 / 2 / 3 row groups; one case per
precision at 2048 rows = SB_MAXGROUPS), at the ends of what they admit and the engines never set: in0 1 .. 31 at both pitches, out_dim 1 ..
16, a tail-weight base that is not 16-byte aligned, gn 1 .. 8 at either end of the input row, rep 1 .. 16, jobs that start and end
inside a row group, deterministic jobs and jobs without a log-probability, A 1 .. 8, 3 x 2 problems with strides that are no multiples
of each other.  Bars: componentwise, stage counts of C = bound(precision) (small_cases.py).  After EVERY launch the words outside the
logical results (pad columns, guard rows, rows outside a job, the gaps inside a slab, slabs and part slots >= groups) still hold the
sentinel bit for bit and every operand comes back bit-identical."""
import numpy as np
import pytest

import small_cases as s

pytestmark = pytest.mark.gpu


def _launch(kind, kw, name=None):
    c = s.build(kind, **kw)
    s.run(c)
    if name is not None:
        assert c.report["flavour"] == name, ("the launch took another instantiation", c.report["flavour"], name)
    return c


def _ids(cases):
    return [label.replace(" ", "_") for label, _ in cases]


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print("\nworst |got - f64| / bound per stage:", {k: round(v, 4) for k, v in sorted(s.MEASURED.items())})


@pytest.mark.parametrize("name", sorted(s.FLAVOURS))
def test_every_instantiation_runs_once(name):
    kw = dict(s.FLAVOURS[name])
    s.check(_launch(kw.pop("kind"), kw, name))


@pytest.mark.parametrize("label,kw", s.fwd_geometry_cases(), ids=_ids(s.fwd_geometry_cases()))
def test_forward_geometry(label, kw):
    """M, in0 / x_pitch, out_dim (the vector tail at 1, the MFMA tail above), an unaligned tail-weight base, 3 x 2 problems"""
    s.check(_launch("fwd", kw))


@pytest.mark.parametrize("label,kw", s.qg_cases(), ids=_ids(s.qg_cases()))
def test_forward_with_unit_seed_backward(label, kw):
    """QG mode: q and G = dq / dx[:, gc0 : gc0 + gn] from the kernel's own masks, gn 1 .. 8 at either end of the input row"""
    c = _launch("fwd", kw)
    assert c.report["flavour"] == f"small_fwd<{kw.get('f32', 0)},1>"
    s.check(c)


@pytest.mark.parametrize("label,kw", s.sample_cases(), ids=_ids(s.sample_cases()))
def test_sampling_epilogue(label, kw):
    """one to three jobs on the head rows the launch produced: every rep class, jobs that start and end inside a row group and in the
    middle of a head row's repeats, null eps / logp, destination offsets, two runs, the clamp edges, saturated actions"""
    s.check(_launch("fwd", kw))


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("qg", [0, 1])
def test_storing_the_hidden_activations_changes_no_result_bit(qg, f32):
    """H0 / H1 given or null in all four combinations: OUT, G, the actions and the log-probabilities are the same bits"""
    kw = dict(out_dim=1, in0=23, gn=6, gc0=17) if qg else dict(out_dim=6, A=3, jobs=s._jobs(96, 3, 3, 3, 40))
    kw.update(M=96, f32=f32, nz0=2, wide=True, seed=700 + qg)
    full = _launch("fwd", kw)
    s.check(full)
    for h0, h1 in ((True, False), (False, True), (False, False)):
        c = _launch("fwd", dict(kw, h0=h0, h1=h1))
        assert c.report["flavour"] == full.report["flavour"]
        s.check(c, hidden=False)      # guards, operands, and the epilogue from the launch's own OUT
        for k, a in c.arrays.items():
            if a.result:
                assert np.array_equal(a.raw, full.arrays[k].raw), (k, "differs from the launch that stored H0 and H1", h0, h1)


@pytest.mark.parametrize("label,kw", s.abwd_cases(), ids=_ids(s.abwd_cases()))
def test_actor_backward(label, kw):
    """every slab against the float64 reference of exactly its own 32 rows; the loss partials, the metrics, the temperature step"""
    s.check(_launch("abwd", kw))


@pytest.mark.parametrize("label,kw", s.abwd_big_cases(), ids=_ids(s.abwd_big_cases()))
def test_actor_backward_at_the_largest_group_count(label, kw):
    """M = 2048: 64 row groups = SB_MAXGROUPS, every part slot in use, one ticket walked by 64 workgroups"""
    c = _launch("abwd", kw)
    assert c.report["groups"] == 64
    s.check(c)


@pytest.mark.parametrize("f32", [0, 1])
def test_a_second_launch_on_the_returned_buffers_gives_the_same_slabs(f32):
    """the ticket is back at 0 and serves the next launch; with a fixed alpha nothing the slabs depend on has changed"""
    c = _launch("abwd", dict(M=96, runs=2, f32=f32, auto_alpha=0, seed=210))
    s.check(c)
    first = {k: c.arrays[k].raw.copy() for k in ("out", "part", "metrics_last", "sc")}
    sums = c.arrays["metrics_sum"].get().copy()
    c.d["metrics_sum"] = sums[:, :, 0]      # the second launch adds to what the first left
    c.before = {k: a.raw.copy() for k, a in c.arrays.items()}
    s.run(c)
    s.check(c)
    for k, v in first.items():
        assert np.array_equal(c.arrays[k].raw, v), (k, "the second launch left other bits")
