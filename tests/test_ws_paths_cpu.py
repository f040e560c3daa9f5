"""CPU: (1) the float64 numpy references of tests/ws_cases.py against torch's float64 autograd on a two-layer and a three-layer critic --
a wrong reference must not certify a wrong kernel; (2) the per-slab row rule against a plain loop; (3) dry runs of every case list
through the unit tap of the weight-stationary kernels (orl_debug_ws): the cases reach every instantiation of the tap's table and every
pipeline-depth class of every launcher; (4) the tap's refusals, all of which come before any device call and therefore raise with
their message on a machine without a GPU; (5) the mask-flip share of float32 numpy against float64 on the seeds the GPU file uses;
(6) the checks themselves, on what a float32 numpy emulation of a correct kernel leaves in the arrays and on planted defects."""
import numpy as np
import pytest
import torch

import ws_cases as w
from offlinerlkit import _engine


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (np.abs(want).max() + 1e-300))


# ---- 1. references against autograd ----
@pytest.mark.parametrize("layers", [2, 3])
def test_references_match_torch_float64_autograd(layers):
    """critic: x -> relu(W0 x + b0) [-> relu(Wm . + bm)] -> relu(W1 . + b1) -> w_tail . + b_tail, loss = sum_m dq[m] q[m]"""
    rng = np.random.RandomState(layers)
    M, in0, H = 96, 7, 256
    x = rng.standard_normal((M, in0))
    dims = [in0] + [H] * layers
    Ws = [rng.uniform(-1, 1, (dims[i + 1], dims[i])) / 4 for i in range(layers)]
    bs = [rng.uniform(-1, 1, dims[i + 1]) / 4 for i in range(layers)]
    wt, tb, dq = rng.uniform(-1, 1, H) / 16, rng.uniform(-1, 1, 1), rng.standard_normal(M) / M
    tW, tB = [_t(a, True) for a in Ws], [_t(a, True) for a in bs]
    twt, ttb = _t(wt, True), _t(tb, True)
    h, acts = _t(x), []
    for W, b in zip(tW, tB):
        h = torch.relu(h @ W.T + b)
        acts.append(h)
    q = h @ twt + ttb
    (q * _t(dq)).sum().backward()
    # forward and masks
    zs, hs, xin = [], [], x
    for W, b in zip(Ws, bs):
        zs.append(w.ref_layer(xin, W, b))
        xin = np.maximum(zs[-1], 0)
        hs.append(xin)
    for z, a in zip(zs, acts):
        assert _rel(np.maximum(z, 0), a.detach().numpy()) < 1e-12
        assert np.array_equal(z > 0, a.detach().numpy() > 0)
        assert np.array_equal(w.unpack_mask(w.pack_mask(z > 0)), z > 0)
    assert _rel(w.ref_tail(hs[-1], wt, tb), q.detach().numpy()) < 1e-12
    rows = np.arange(M)
    masks = [z > 0 for z in zs]
    # the top hidden layer: rank-1 gradient from (mask bits, dq, w_tail)
    dW, db, G, g = w.ref_wgrad(masks[-1], dq, hs[-2], wt, rows)
    assert _rel(dW, tW[-1].grad.numpy()) < 1e-12 and _rel(db, tB[-1].grad.numpy()) < 1e-12
    dwt, dbt = w.ref_tails(dq, hs[-1], rows)
    assert _rel(dwt, twt.grad.numpy()) < 1e-12 and _rel(dbt, ttb.grad.numpy()) < 1e-12
    assert _rel(w.ref_derived(G, g, Ws[-1], bs[-1]), twt.grad.numpy()) < 1e-12      # the tail gradient derived from the accumulators
    dz = w.ref_dz0(masks[-1], masks[-2], dq, wt, Ws[-1])      # gradient w.r.t. the pre-activation below the top layer
    if layers == 3:      # the middle layer: materialised gradient (the PLAIN flavours)
        dWm, dbm = w.ref_wgrad_plain(dz, hs[0], rows)
        assert _rel(dWm, tW[1].grad.numpy()) < 1e-12 and _rel(dbm, tB[1].grad.numpy()) < 1e-12
        dz = w.ref_dz0_plain(masks[0], dz, Ws[1])
    dW0, db0 = w.ref_w0(dz, x, rows)
    assert _rel(dW0, tW[0].grad.numpy()) < 1e-12 and _rel(db0, tB[0].grad.numpy()) < 1e-12
    # split-K slabs: the slabs of any per_z sum to the whole
    for per_z in (1, 2, 3):
        parts = [w.ref_wgrad(masks[-1], dq, hs[-2], wt, w.slab_rows(M, per_z, s))[0] for s in range(per_z)]
        assert _rel(sum(parts), tW[-1].grad.numpy()) < 1e-12


# ---- 2. the per-slab row rule ----
@pytest.mark.parametrize("M,per_z", w.DEPTHS)
def test_slab_rows_match_a_plain_loop(M, per_z):
    """workgroup blockIdx.x = slab takes the groups g0, g0 + gridDim.x, ... of 32 rows (g0 = blockIdx.x, gs = gridDim.x in every kernel)"""
    owner = {}
    for slab in range(per_z):
        g = slab
        while g < M // 32:
            for r in range(32):
                owner[32 * g + r] = slab
            g += per_z
    assert sorted(owner) == list(range(M))
    for slab in range(per_z):
        assert list(w.slab_rows(M, per_z, slab)) == [m for m in range(M) if owner[m] == slab]
    assert w.groups_per_workgroup(M, per_z) == [sum(1 for m in range(0, M, 32) if owner[m] == s) for s in range(per_z)]


# ---- 3. dry runs over the case lists ----
def test_the_cases_reach_every_instantiation():
    table = _engine.ws_flavours()
    assert len(table) == len(set(table)) == 48
    reached = set()
    for name, kw in w.FLAVOURS.items():
        rep = w.run(w.build(**kw), dry_run=True)
        assert rep["flavour"] == name and table[rep["flavour_id"]] == name, (name, rep)
        assert rep["groups"] == 8 and 0 < rep["lds"] <= 160 * 1024
        assert rep["launcher"] == _engine.WS_KINDS[kw["kind"]]
        reached.add(name)
    # an instantiation that no launch can reach has to be listed by name with its reason
    assert reached | set(w.UNREACHED) == set(table), set(table) ^ (reached | set(w.UNREACHED))
    assert not (reached & set(w.UNREACHED))


def test_lds_bytes_of_the_report_are_the_launchers():
    """a few known sizes (csrc/ws_gemm.h): two bf16 planes x two buffers x 32 x 256 = 64 KB of A images in the forward"""
    lds = {n: w.run(w.build(**w.FLAVOURS[n]), dry_run=True)["lds"] for n in ("ws_fwd<0,0,0,1,0,1>", "ws_fwd<1,1,0,0,0,1>", "ws_fwd3<1,0,1,1,0>", "ws_wgrad<3>", "ws_wgrad<2>")}
    assert lds["ws_fwd<0,0,0,1,0,1>"] == 65536 + 4 * 2 * 8 * 32 + 2 * 32 * 68 + 4 * 2 * 256
    assert lds["ws_fwd<1,1,0,0,0,1>"] == lds["ws_fwd<0,0,0,1,0,1>"] + 4 * 2 * 32 * 36 + 2 * 32 * 68
    assert lds["ws_fwd3<1,0,1,1,0>"] > lds["ws_fwd<1,1,0,0,0,1>"]
    assert lds["ws_wgrad<3>"] == 2 * 4 * 32 * 256 * 2 + 2 * 2 * 32 * 16 * 2 and lds["ws_wgrad<2>"] == 2 * 3 * 32 * 256 * 2 + 2 * 2 * 32 * 16 * 2


def test_the_depth_sweep_reaches_every_depth_class_of_every_launcher():
    seen = {}
    for name, M, per_z in w.depth_cases():
        rep = w.run(w.build(**w.depth_kwargs(name, M, per_z)), dry_run=True)
        assert rep["flavour"] == name and rep["groups"] == M // 32
        counts = w.groups_per_workgroup(M, per_z)
        assert sum(counts) == rep["groups"] and min(counts) >= 1
        s = seen.setdefault(w.LAUNCHER_OF[name], set())
        s.update(min(c, 5) for c in counts)
        if len(set(counts)) > 1:
            s.add("uneven")
    assert set(seen) == set(_engine.WS_KINDS)
    for kind, s in seen.items():
        assert s == {1, 2, 3, 4, 5, "uneven"}, (kind, s)
    # the flavours bench.py runs are among them, with their exact and three-plane siblings, and a plain flavour per launcher
    for name in ("ws_fwd<1,1,0,0,0,1>", "ws_dgrad<1,0,0>", "ws_wgrad<2>", "ws_wgrad<5>", "ws_fwd<1,1,0,0,1,1>", "ws_dgrad32<1,0,0>", "ws_wgrad32<2>", "ws_fwd3<1,0,1,1,0>",
                 "ws_dgrad3<1,0>", "ws_wgrad3p"):
        assert name in w.DEPTH_FLAVOURS


def test_the_geometry_cases_pass_the_checks_of_the_tap_and_cover_the_list():
    labels = set()
    for label, name, over in w.geometry_cases():
        c = w.build(**w.geometry_kwargs(name, over))
        assert w.run(c, dry_run=True)["flavour"] == name, (label, name)
        labels.add(label)
        assert c.M in (256, 288, 352) and c.nz0 * c.nz1 <= 6
    for want in ("in0 3 pitch 4", "in0 23 pitch 24", "in0 31 pitch 32", "EnsembleLinear weights", "EnsembleLinear slabs", "3 x 2 problems, wide strides",
                 "pitches padded by 4", "pitches padded by 12", "tq_sm 1", "tq_sm 3", "dq_sm 1", "dq_sm 3", "gscale None", "gscale 0.015625", "gscale 512.0"):
        assert want in labels, want
    c = w.build(**w.geometry_kwargs("ws_wgrad<2>", dict(nz0=3, nz1=2, wide=True)))
    for a in c.arrays.values():      # s1 larger than the problem, s0 no multiple of s1
        assert a.s1 > a.idx[0, 0].max() - a.idx[0, 0].min() and a.s0 % a.s1


# ---- 4. refusals: every one before any device call ----
F = w.FLAVOURS
REFUSALS = [
    ("M = 224", dict(F["ws_fwd<1,1,0,0,0,1>"], M=224, per_z=1), "refused by ws_fwd_supported"),
    ("M = 224, dgrad", dict(F["ws_dgrad<1,0,0>"], M=224, per_z=1), "refused by ws_dgrad_supported"),
    ("M = 224, wgrad", dict(F["ws_wgrad<2>"], M=224, per_z=1), "refused by ws_wgrad_supported"),
    ("M % 32", dict(F["ws_fwd<0,0,0,1,0,1>"], ints=dict(M=300)), "M must be a multiple of 32"),
    ("M > 4096", dict(F["ws_fwd<0,0,0,1,0,1>"], ints=dict(M=4128)), "M must be 1..4096"),
    ("nz > 64", dict(F["ws_fwd<0,0,0,1,0,1>"], ints=dict(nz0=13, nz1=5)), "nz0 x nz1 must be 1..64"),
    ("per_z < 1", dict(F["ws_wgrad<0>"], ints=dict(per_z=0)), "per_z must be >= 1"),
    ("per_z > groups", dict(F["ws_dgrad<1,0,0>"], ints=dict(per_z=9)), "per_z exceeds the row groups"),
    ("in0 + 1 > 32", dict(F["ws_fwd<1,1,0,0,0,1>"], ints=dict(in0=32)), "in0 must be 1..31"),
    ("in0 + 1 > 32, dgrad", dict(F["ws_dgrad3<1,0>"], ints=dict(in0=32)), "in0 must be 1..31"),
    ("in0 >= x0_pitch", dict(F["ws_fwd<1,1,0,0,0,1>"], ints=dict(in0=24)), "in0 must be below x0_pitch"),
    ("in0 >= x0_pitch, fwd3", dict(F["ws_fwd3<1,0,1,1,0>"], ints=dict(in0=24)), "in0 must be below x0_pitch"),
    ("in0 >= x_pitch, dgrad", dict(F["ws_dgrad<1,0,1>"], ints=dict(in0=25)), "in0 must be below x_pitch"),
    ("in0 >= x0_pitch, recompute", dict(F["ws_wgrad<4>"], ints=dict(in0=24)), "in0 must be below x0_pitch"),
    ("misaligned X", dict(F["ws_fwd<0,0,0,1,0,1>"], off={"X": 1}), "refused by ws_fwd_supported"),
    ("misaligned W", dict(F["ws_fwd<0,0,0,1,1,1>"], off={"W": 2}), "refused by ws_fwd_supported"),
    ("misaligned bias", dict(F["ws_fwd<0,0,0,1,0,1>"], off={"bias": 3}), "refused by ws_fwd_supported"),
    ("misaligned Y", dict(F["ws_fwd<1,0,0,1,0,1>"], off={"Y": 1}), "refused by ws_fwd_supported"),
    ("misaligned tw", dict(F["ws_fwd<1,0,0,0,0,1>"], off={"tw": 1}), "refused by ws_fwd_supported"),
    ("misaligned X, fwd3", dict(F["ws_fwd3<0,1,0,0,0>"], off={"X": 1}), "refused by ws_fwd3_supported"),
    ("misaligned Z", dict(F["ws_dgrad<1,0,1>"], off={"Z": 1}), "refused by ws_dgrad_supported"),
    ("misaligned wt, dgrad", dict(F["ws_dgrad32<0,1,0>"], off={"wt": 2}), "refused by ws_dgrad_supported"),
    ("misaligned wt, dgrad3", dict(F["ws_dgrad3<1,0>"], off={"wt": 2}), "refused by ws_dgrad3_supported"),
    ("misaligned H0", dict(F["ws_wgrad<0>"], off={"H0": 1}), "refused by ws_wgrad_supported"),
    ("misaligned H1", dict(F["ws_wgrad32<1>"], off={"H1": 3}), "refused by ws_wgrad_supported"),
    ("misaligned wt, wgrad", dict(F["ws_wgrad<2>"], off={"wt": 1}), "refused by ws_wgrad_supported"),
    ("misaligned dZ", dict(F["ws_wgrad<3>"], off={"dZ": 1}), "refused by ws_wgrad_supported"),
    ("misaligned dZ, wgrad3p", dict(F["ws_wgrad3p"], off={"dZ": 1}), "refused by ws_wgrad3p_supported"),
    ("a pitch that is no multiple of 4", dict(F["ws_fwd<0,0,0,1,0,1>"], pad=2), "refused by ws_fwd_supported"),
    ("np3 with f32", dict(F["ws_wgrad<5>"], ints=dict(f32=1)), "np3 and f32 exclude each other"),
    ("f32 on a three-plane launcher", dict(F["ws_fwd3<1,0,1,1,0>"], ints=dict(f32=1)), "f32 does not go with a three-plane launcher"),
    ("X too short", dict(F["ws_fwd<0,0,0,1,0,1>"], short={"X": 1}), "X: the array is shorter"),
    ("Y too short", dict(F["ws_fwd<0,0,1,1,0,1>"], short={"Y": 5}), "Y: the array is shorter"),
    ("X0 too short", dict(F["ws_fwd<1,1,0,0,0,0>"], short={"X0": 5}), "X0: the array is shorter"),
    ("W0 too short", dict(F["ws_fwd3<1,1,1,1,0>"], short={"W0": 8}), "W0: the array is shorter"),
    ("mb too short", dict(F["ws_fwd<1,0,0,0,0,1>"], short={"mb": 8}), "mb: the array is shorter"),
    ("tq too short", dict(F["ws_fwd<1,0,0,0,0,1>"], tq_sm=3, short={"tq": 7}), "tq: the array is shorter"),
    ("dq too short", dict(F["ws_dgrad<1,0,0>"], dq_sm=3, short={"dq": 7}), "dq: the array is shorter"),
    ("abits too short", dict(F["ws_dgrad3<0,0>"], short={"abits": 9}), "abits: the array is shorter"),
    ("the last slab of w0_out does not fit", dict(F["ws_dgrad<1,0,0>"], ints=dict(per_z=4)), "w0_out: the array is shorter"),
    ("the last slab of dW does not fit", dict(F["ws_wgrad<2>"], ints=dict(per_z=4)), "dW: the array is shorter"),
    ("W1 too short", dict(F["ws_wgrad32<2>"], short={"W1": 5}), "W1: the array is shorter"),
    ("dbt too short", dict(F["ws_wgrad<1>"], short={"dbt": 66049}), "dbt: the array is shorter"),
    ("gscale shorter than the runs", dict(F["ws_wgrad<3>"], gscale=2.0, short={"gscale": 1}), "gscale: one float per run"),
    # combinations the launcher's table has no instantiation for (the predicates ask the launchers' selectors, csrc/ws_gemm.h)
    ("fwd3: tail, stored activation and discarded h0", dict(F["ws_fwd3<1,1,1,1,0>"], discard=True), "refused by ws_fwd3_supported"),
    ("fwd3: tail, stored activation and discarded h0, other depth", dict(F["ws_fwd3<1,1,1,1,0>"], discard=True, M=352, per_z=3), "refused by ws_fwd3_supported"),
    ("fwd3: neither tail nor Y", dict(F["ws_fwd3<0,1,0,0,0>"], sy=False), "refused by ws_fwd3_supported"),
    ("fwd3: neither tail nor Y, fused first layer", dict(F["ws_fwd3<0,1,1,1,0>"], sy=False), "refused by ws_fwd3_supported"),
    ("fwd: neither tail nor Y", dict(F["ws_fwd<0,0,0,1,0,1>"], sy=False), "refused by ws_fwd_supported"),
    ("wgrad: np3 with H1", dict(F["ws_wgrad<1>"], np3=1), "np3 is the derived-tail flavour"),
]


@pytest.mark.parametrize("label,kw,msg", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals_come_with_a_message_and_without_a_device(label, kw, msg):
    c = w.build(**kw)
    for dry in (0, 1):      # a real call is refused at the same check: it never reaches hipGetDeviceCount
        with pytest.raises(RuntimeError, match="orl_debug_ws failed: orl_debug_ws: .*" + msg):
            _engine.debug_ws(c.kind, c.arrays, dry_run=dry, **c.ints)
    for name, a in c.arrays.items():
        assert np.array_equal(a.raw, c.before[name]), name


def _drop(kw, *names, **add):
    c = w.build(**kw)
    for n in names:
        del c.arrays[n]
    return c, add


def test_refusals_of_array_combinations():
    for (c, add), msg in [
        (_drop(F["ws_fwd3<1,0,1,1,0>"], "tq2"), "tq needs tq2"),
        (_drop(F["ws_fwd<1,0,0,1,0,1>"], "tb"), "the fused tail needs tw, tb and tq together"),
        (_drop(F["ws_fwd<1,1,0,0,0,1>"], "mb0"), "the fused first layer needs X0, W0, b0 and mb0 together"),
        (_drop(F["ws_fwd<0,0,0,1,0,1>"], "mb"), "mb is required"),
        (_drop(F["ws_fwd<0,0,0,1,0,1>"], "Y"), "refused by ws_fwd_supported"),
        (_drop(F["ws_fwd3<0,1,0,0,1>"], "Y"), "refused by ws_fwd3_supported"),
        (_drop(F["ws_dgrad<1,0,0>"], "b0_out"), "w0_out and b0_out go together"),
        (_drop(F["ws_dgrad<0,1,0>"], "C"), "give either the dW0 / db0 slabs"),
        (_drop(F["ws_dgrad<1,0,0>"], "abits"), "ab_g .abits' pitch. must be 8 words"),
        (_drop(F["ws_wgrad<1>"], "dwt"), "dwt and dbt go with the tail gradients"),
        (_drop(F["ws_wgrad<2>"], "b1"), "W1 and b1 go together"),
        (_drop(F["ws_wgrad<4>"], "b0"), "recompute needs X0, W0 and b0 together"),
        (_drop(F["ws_wgrad3p"], "dZ"), "dZ is required"),
    ]:
        with pytest.raises(RuntimeError, match="orl_debug_ws failed: orl_debug_ws: .*" + msg):
            _engine.debug_ws(c.kind, c.arrays, **c.ints)
    # dgrad3: both or neither of w0_out and C -- no such instantiation (ws_dgrad3_flavour)
    c = w.build(**F["ws_dgrad3<0,0>"])
    del c.arrays["C"]
    with pytest.raises(RuntimeError, match="give either the dW0 / db0 slabs .w0_out, b0_out. or C .the stored dz0., not both and not neither"):
        _engine.debug_ws(c.kind, c.arrays, **c.ints)
    c, both = w.build(**F["ws_dgrad3<1,0>"]), w.build(**F["ws_dgrad3<0,0>"])
    c.arrays["C"] = both.arrays["C"]
    with pytest.raises(RuntimeError, match="give either the dW0 / db0 slabs .w0_out, b0_out. or C .the stored dz0., not both and not neither"):
        _engine.debug_ws(c.kind, c.arrays, **c.ints)
    # np3 with H1: the three-plane wgrad is the derived-tail flavour
    c = w.build(**dict(F["ws_wgrad<1>"], np3=1))
    with pytest.raises(RuntimeError, match="np3 is the derived-tail flavour"):
        _engine.debug_ws(c.kind, c.arrays, **c.ints)
    # dm_g != 8, mb0_g != 8, ab_g != 8
    for name, arr, msg in (("ws_fwd<0,0,1,1,0,1>", "dmask", "dm_g"), ("ws_fwd3<0,1,0,0,1>", "dmask", "dm_g"), ("ws_fwd<1,1,0,0,0,1>", "mb0", "mb0_g"),
                           ("ws_dgrad<1,0,0>", "xbits", "xb_g"), ("ws_wgrad<0>", "abits", "ab_g")):
        c = w.build(**F[name])
        c.arrays[arr].pitch = 12
        with pytest.raises(RuntimeError, match=msg + ".* must be 8 words"):
            _engine.debug_ws(c.kind, c.arrays, **c.ints)
    # arrays of another launcher
    c = w.build(**F["ws_wgrad<0>"])
    c.arrays["Y"] = c.arrays["H0"]
    with pytest.raises(RuntimeError, match="Y does not belong to this launcher"):
        _engine.debug_ws(c.kind, c.arrays, **c.ints)
    with pytest.raises(TypeError):
        _engine.debug_ws("wgrad", {"nonsense": None})


# ---- 5. the mask-flip share of float32 against float64 on the chosen seeds ----
def _forward_cases():
    out = [(n, kw) for n, kw in w.FLAVOURS.items() if kw["kind"] in ("fwd", "fwd3") and not kw.get("dgm")]
    out += [(n, w.depth_kwargs(n, M, pz)) for n, M, pz in w.depth_cases() if w.LAUNCHER_OF[n] in ("fwd", "fwd3")]
    out += [(n, w.geometry_kwargs(n, over)) for _, n, over in w.geometry_cases() if w.LAUNCHER_OF[n] in ("fwd", "fwd3") and not w.FLAVOURS[n].get("dgm")]
    return out


def test_float32_masks_stay_inside_the_flip_share_on_the_chosen_seeds():
    seen = set()
    worst = 0.0
    for name, kw in _forward_cases():
        key = (kw.get("seed", 0), kw.get("M", 256), kw.get("in0", 23), kw.get("l0", False), kw.get("nz0", 2), kw.get("nz1", 1), kw.get("ens", False))
        if key in seen:      # the data depend on these only
            continue
        seen.add(key)
        c = w.emulate(w.build(**kw))
        for (which, z), z32 in c.z32.items():
            if which == "z0":
                z64 = w.ref_layer(c.d["X0"][z][:, :c.in0], c.d["W0"][z], c.d["b0"][z])
            else:
                x = np.maximum(c.z32["z0", z], 0) if ("z0", z) in c.z32 else c.d["X"][z]
                z64 = w.ref_layer(x, c.d["W"][z], c.d["bias"][z])
            worst = max(worst, float(((z32 > 0) != (z64 > 0)).mean()))
    assert len(seen) >= 10
    assert worst < w.FLIP_SHARE, worst


# ---- 6. the checks pass on a correct result and bite on a planted defect ----
@pytest.mark.parametrize("name", sorted(w.FLAVOURS))
def test_checks_pass_on_the_float32_emulation(name):
    c = w.emulate(w.build(**dict(w.FLAVOURS[name], M=288, per_z=3)))
    res = w.check(c)
    assert res.worst() < 0.5, res.worst()      # float32 numpy sits well inside the exact-fp32 bar


def _fails(c, msg):
    with pytest.raises(AssertionError, match=msg):
        w.check(c)


def test_checks_bite_on_planted_defects():
    kw = dict(M=288, per_z=3)
    # the tail bias dropped in one column half of the three-plane forward
    c = w.emulate(w.build(**dict(F["ws_fwd3<1,0,1,1,0>"], **kw)))
    a = c.arrays["tq"]
    a.put(a.get() - c.d["tb"].reshape(2, 1, 1, 1, 1))
    _fails(c, "componentwise error")
    # a stale buffer: one row group of the stored activation is the previous group's
    c = w.emulate(w.build(**dict(F["ws_fwd<0,0,0,1,0,1>"], **kw)))
    y = c.arrays["Y"].get().copy()
    y[0, 0, 0, 64:96] = y[0, 0, 0, 32:64]
    c.arrays["Y"].put(y)
    _fails(c, "componentwise error|mb disagrees")
    # a mask bit flipped where |z| is large
    c = w.emulate(w.build(**dict(F["ws_fwd<1,1,0,0,0,1>"], **kw)))
    m = c.arrays["mb0"].get().copy()
    big = np.abs(c.z32["z0", (0, 0)]).argmax()
    m[0, 0, 0, big // 256, (big % 256) // 32] ^= np.uint32(1 << (big % 32))
    c.arrays["mb0"].put(m)
    _fails(c, "a mask bit differs")
    # one row group dropped from a workgroup's slab; a row group credited to the wrong slab (the sum still right)
    for name, arr in (("ws_dgrad<1,0,0>", "w0_out"), ("ws_wgrad<2>", "dW"), ("ws_wgrad<3>", "dW"), ("ws_wgrad3p", "dW")):
        c = w.emulate(w.build(**dict(F[name], **kw)))
        full = w.build(**dict(F[name], M=288, per_z=3))
        rows = np.arange(32, 64)      # group 1 belongs to slab 1
        if name.startswith("ws_dgrad"):
            dz0 = w.ref_dz0(c.d["abits_pos"][0, 0], c.d["xbits_pos"][0, 0], c.d["dq"][0, 0][:, 0], c.d["wt"][0, 0][0], c.d["W"][0, 0])
            part = w.ref_w0(dz0, c.d["X"][0, 0][:, :c.in0], rows)[0]
        elif "abits_pos" in c.d:
            part = w.ref_wgrad(c.d["abits_pos"][0, 0], c.d["dq"][0, 0][:, 0], c.d["H0"][0, 0], c.d["wt"][0, 0][0], rows)[0]
        else:
            part = w.ref_wgrad_plain(c.d["dZ"][0, 0], c.d["H0"][0, 0], rows)[0]
        g = c.arrays[arr].get().copy()
        g[0, 0, 1] -= part
        g[0, 0, 2] += part
        c.arrays[arr].put(g)
        with pytest.raises(AssertionError, match="slab 1"):
            w.check(c)
        del full
    # a word written outside the logical result, into a slab >= per_z, and into an operand
    c = w.emulate(w.build(**dict(F["ws_fwd<0,0,0,1,0,1>"], pad=4, **kw)))
    c.arrays["Y"].raw[c.arrays["Y"].idx[0, 0, 0, 5, 255] + 1] = 0
    _fails(c, "outside the logical result")
    c = w.emulate(w.build(**dict(F["ws_wgrad<0>"], **kw)))
    c.arrays["db"].raw[c.arrays["db"].idx[1, 0, 3, 0, 7]] = 0
    _fails(c, "a slab >= per_z was written")
    c = w.emulate(w.build(**dict(F["ws_wgrad<0>"], **kw)))
    c.arrays["H0"].raw[11] ^= 1
    _fails(c, "an operand came back changed")
    c = w.emulate(w.build(**dict(F["ws_fwd<1,1,0,0,0,0>"], **kw)))
    c.arrays["X"].raw[c.arrays["X"].idx[0, 0, 0, 40, 3]] = 0
    _fails(c, "h0 was stored")
