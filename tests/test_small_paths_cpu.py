"""CPU: (1) the float64 numpy references of tests/small_cases.py against torch's float64 autograd -- an actor [in0 -> 256 -> 256 -> 2A]
with the tanh-Gaussian head under L = mean(alpha logp - min(q0, q1)) with q_k linear in the action, a critic's dQ/da, torch's Adam on
log_alpha: a wrong reference must not certify a wrong kernel; (2) dry runs of every case list through the unit tap of the few-rows
kernels (orl_debug_small): together they reach all six instantiations; (3) the tap's refusals, all of which come before any device call
and therefore raise with their message on a machine without a GPU; (4) the mask-flip share and the K / Adam ratios of float32 numpy
against float64 on the seeds the GPU file uses; (5) the checks themselves, on what a float32 numpy emulation of a correct kernel leaves
in the arrays and on planted defects."""
import numpy as np
import pytest
import torch

import small_cases as s
from offlinerlkit import _engine


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (np.abs(want).max() + 1e-300))


# ---- 1. references against autograd ----
@pytest.mark.parametrize("A,in0,alpha", [(3, 11, 0.7), (1, 1, 0.2), (8, 31, 1.3)])
def test_actor_reference_matches_torch_float64_autograd(A, in0, alpha):
    rng = np.random.RandomState(A)
    M, H = 64, 256
    x = rng.standard_normal((M, in0))
    W0, b0, W1, b1 = rng.uniform(-1, 1, (H, in0)) / 4, rng.uniform(-1, 1, H) / 4, rng.uniform(-1, 1, (H, H)) / 8, rng.uniform(-1, 1, H) / 8
    Wh, bh = rng.uniform(-1, 1, (2 * A, H)) / 8, np.concatenate([rng.uniform(-1, 1, A), rng.uniform(-4, 1.5, A)])
    eps = rng.standard_normal((M, A))
    qc, ga = rng.standard_normal((2, M)), rng.standard_normal((2, M, A))
    qc[1, 1], ga[1, 1] = qc[0, 1], ga[0, 1]      # row 1: an exact tie
    tp = [_t(a, True) for a in (W0, b0, W1, b1, Wh, bh)]
    h0 = torch.relu(_t(x) @ tp[0].T + tp[1])
    h1 = torch.relu(h0 @ tp[2].T + tp[3])
    head = h1 @ tp[4].T + tp[5]
    # log sigma at and beyond both clamp ends on rows 2 / 3 (added behind the head so that the rows hit the values exactly)
    shift = np.zeros((M, 2 * A))
    hv = head.detach().numpy()
    for (r, col), want in {(2, A): -5.0, (3, A): -6.0, (7, 2 * A - 1): 2.0, (8, 2 * A - 1): 3.0}.items():
        sh = want - hv[r, col]
        for _ in range(8):      # the shift whose rounded sum is exactly the wanted value
            sh += want - (hv[r, col] + sh)
        shift[r, col] = sh
    head = head + _t(shift)
    assert head[2, A].item() == -5.0 and head[7, 2 * A - 1].item() == 2.0
    mu, ls_raw = head[:, :A], head[:, A:]
    ls = torch.clamp(ls_raw, -5.0, 2.0)
    sg = torch.exp(ls)
    u = mu + sg * _t(eps)
    act = torch.tanh(u)
    logp = ((-((u - mu) ** 2) / (2 * sg * sg) - ls - s.LOG_SQRT_2PI) - torch.log((1 - act * act) + 1e-6)).sum(1)
    q = [_t(qc[k]) + (_t(ga[k]) * act).sum(1) for k in range(2)]
    assert q[0][1].item() == q[1][1].item()
    L = (alpha * logp - torch.minimum(q[0], q[1])).mean()
    L.backward()
    # forward references
    a_ref, lp_ref, _, _ = s.ref_sample(mu.detach().numpy(), ls_raw.detach().numpy(), eps)
    assert _rel(a_ref, act.detach().numpy()) < 1e-12 and _rel(lp_ref, logp.detach().numpy()) < 1e-12
    # backward references from what the kernel is given
    dh, _ = s.ref_dhead(q[0].detach().numpy(), q[1].detach().numpy(), ga[0], ga[1], ls_raw.detach().numpy(), eps, act.detach().numpy(), alpha, M)
    parts = [s.ref_abwd_group(dh[g:g + 32], h1.detach().numpy()[g:g + 32], h0.detach().numpy()[g:g + 32], x[g:g + 32], Wh, W1) for g in range(0, M, 32)]
    tot = {k: sum(p[k] for p in parts) for k in s.STAGES}
    for k, t in (("w0", tp[0]), ("b0", tp[1]), ("w1", tp[2]), ("b1", tp[3]), ("wh", tp[4]), ("bh", tp[5])):
        assert _rel(tot[k], t.grad.numpy()) < 1e-11, k
    # the loss sums
    assert abs((alpha * lp_ref - np.minimum(q[0].detach().numpy(), q[1].detach().numpy())).sum() / M - L.item()) < 1e-12


def test_qg_reference_matches_torch_float64_autograd():
    rng = np.random.RandomState(5)
    M, in0, H, gc0, gn = 32, 23, 256, 17, 6
    x = _t(rng.standard_normal((M, in0)), True)
    W0, b0, W1, b1, wt = rng.uniform(-1, 1, (H, in0)) / 4, rng.uniform(-1, 1, H) / 4, rng.uniform(-1, 1, (H, H)) / 8, rng.uniform(-1, 1, H) / 8, rng.uniform(-1, 1, H)
    h0 = torch.relu(x @ _t(W0).T + _t(b0))
    h1 = torch.relu(h0 @ _t(W1).T + _t(b1))
    (h1 @ _t(wt) + 0.3).sum().backward()
    G = s.ref_qg(h0.detach().numpy() > 0, h1.detach().numpy() > 0, W0[:, gc0:gc0 + gn], wt, W1)
    assert _rel(G, x.grad.numpy()[:, gc0:gc0 + gn]) < 1e-12


@pytest.mark.parametrize("t0", [0, 999])
def test_adam_reference_matches_torch_adam(t0):
    b1, b2, eps, lr = [float(np.float32(v)) for v in (0.9, 0.999, 1e-8, 3e-4)]
    la = torch.tensor([-0.3], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([la], lr=lr, betas=(b1, b2), eps=eps)
    rng = np.random.RandomState(1)
    p, m, v = -0.3, 0.0, 0.0
    if t0:      # moments and step count of a run in progress
        m, v = 0.3, 0.05
        opt.zero_grad()
        (la * 0.0).sum().backward()
        opt.step()
        st = opt.state[la]
        st["exp_avg"].fill_(m), st["exp_avg_sq"].fill_(v)
        st["step"] = torch.tensor(float(t0)) if torch.is_tensor(st["step"]) else t0
        la.data.fill_(p)
    for k in range(4):
        mean_t = rng.standard_normal() - 1.0
        opt.zero_grad()
        (-(la * mean_t)).sum().backward()
        opt.step()
        (p, m, v), _ = s.ref_adam(p, m, v, -mean_t, lr, b1, b2, eps, t0 + k + 1)
        assert abs(p - la.item()) < 1e-13 and abs(m - opt.state[la]["exp_avg"].item()) < 1e-13 and abs(v - opt.state[la]["exp_avg_sq"].item()) < 1e-13


# ---- 2. dry runs over the case lists ----
ALL_LISTS = [("fwd", s.fwd_geometry_cases), ("fwd", s.qg_cases), ("fwd", s.sample_cases), ("abwd", s.abwd_cases), ("abwd", s.abwd_big_cases)]


def test_the_cases_reach_every_instantiation_and_cover_the_issue_list():
    table = _engine.small_flavours()
    assert table == ["small_fwd<0,0>", "small_fwd<1,0>", "small_fwd<0,1>", "small_fwd<1,1>", "small_abwd<0>", "small_abwd<1>"]
    for name, kw in s.FLAVOURS.items():
        rep = s.run(s.build(**kw), dry_run=True)
        assert rep["flavour"] == name and table[rep["flavour_id"]] == name and rep["groups"] == 2 and 0 < rep["lds"] <= 160 * 1024
    reached, labels = set(), set()
    seen = dict(M=set(), in0=set(), out_dim=set(), gn=set(), rep=set(), A=set(), njobs=set(), head_row0=set(), runs=set(), aA=set(), ain0=set())
    for kind, fn in ALL_LISTS:
        for label, kw in fn():
            c = s.build(kind, **kw)
            rep = s.run(c, dry_run=True)
            reached.add(rep["flavour"])
            assert rep["groups"] == c.M // 32 and label not in labels, label
            labels.add(label)
            assert c.M <= 96 or "2048" in label
            if kind == "fwd":
                seen["M"].add(c.M), seen["in0"].add((c.in0, c.arrays["X"].pitch)), seen["out_dim"].add(c.out_dim), seen["gn"].add((c.gn, c.gc0 == 0))
                assert c.arrays["OUT"].pitch > c.out_dim and ("G" not in c.arrays or c.arrays["G"].pitch > c.gn)
                for js in c.job_specs:
                    seen["rep"].add(js["rep"]), seen["head_row0"].add(js["head_row0"])
                    assert js["head_row0"] + -(-js["rows"] // js["rep"]) <= c.M
                if c.job_specs:
                    seen["A"].add(c.A), seen["njobs"].add(len(c.job_specs))
            else:
                seen["runs"].add(c.nz0), seen["aA"].add(c.A), seen["ain0"].add((c.in0, c.arrays["X"].pitch))
                assert c.arrays["ga"].pitch > c.A and c.ints["xa_col"] > 0
    assert reached == set(table)
    assert seen["M"] >= {32, 64, 96} and seen["out_dim"] >= {1, 2, 5, 12, 16}
    assert seen["in0"] >= {(i, p) for i in (1, 2, 14, 23, 31) for p in (i, 32)}
    assert seen["gn"] >= {(g, z) for g in (1, 3, 6, 8) for z in (True, False)}
    assert seen["rep"] >= {1, 2, 3, 10, 15, 16} and seen["A"] >= {1, 3, 6, 8} and seen["njobs"] == {1, 2, 3} and seen["head_row0"] >= {0, 32, 40}
    assert seen["runs"] >= {1, 3} and seen["aA"] >= {1, 3, 6, 8} and seen["ain0"] >= {(i, p) for i in (1, 11, 17, 31) for p in (i, 32)}
    # a job that ends in the middle of a head row's repeats, one without eps, one without logp
    specs = [js for _, kw in s.sample_cases() for js in s.build("fwd", **kw).job_specs]
    assert any(js["rows"] % js["rep"] for js in specs) and any(not js["eps"] for js in specs) and any(not js["logp"] for js in specs)
    assert any(js["dst_row0"] and js["dst_col"] and js["dst_pad"] for js in specs)
    c = s.build("fwd", **dict(s.fwd_geometry_cases()[-1][1]))
    for a in c.arrays.values():      # 3 x 2: s1 larger than the problem, s0 no multiple of s1
        assert a.s1 > a.idx[0, 0].max() - a.idx[0, 0].min() and a.s0 % a.s1


def test_base_actions_stay_inside_the_stated_range():
    for kind, fn in ALL_LISTS[3:]:
        for label, kw in fn():
            c = s.build(kind, **kw)
            assert np.abs(c.d["xa"]).max() <= 0.995, label
            q = c.d["qa"]
            assert np.any(q[:, 0] == q[:, 1]) and np.any(q[:, 0] < q[:, 1]) and np.any(q[:, 1] < q[:, 0])
            ls = c.d["head"][..., c.A:]
            assert np.any(ls == -5.0) and np.any(ls == 2.0) and np.any(ls < -5.0) and np.any(ls > 2.0)
            assert np.any(c.d["H0"] == 0) and not c.d["H0"][0, 0, 5].any() and not c.d["H1"][0, 0, 5].any()


# ---- 3. refusals: every one before any device call ----
F = s.FLAVOURS
PLAIN = dict(kind="fwd")
REFUSALS = [
    ("in0 = 0", dict(PLAIN, ints=dict(in0=0)), "refused by small_fwd_supported"),
    ("in0 = 0, abwd", dict(F["small_abwd<0>"], ints=dict(in0=0)), "refused by small_abwd_supported"),
    ("in0 = 32", dict(PLAIN, x_pitch=32, ints=dict(in0=32)), "refused by small_fwd_supported"),
    ("in0 = 32, abwd", dict(F["small_abwd<1>"], x_pitch=32, ints=dict(in0=32)), "refused by small_abwd_supported"),
    ("M = 48", dict(PLAIN, ints=dict(M=48)), "refused by small_fwd_supported"),
    ("M = 48, abwd", dict(F["small_abwd<0>"], ints=dict(M=48)), "refused by small_abwd_supported"),
    ("M > 2048", dict(PLAIN, ints=dict(M=2080)), "M must be 1..2048"),
    ("65 groups", dict(F["small_abwd<0>"], ints=dict(M=2080)), "M must be 1..2048"),
    ("nz0 x nz1 = 18", dict(PLAIN, ints=dict(nz0=6, nz1=3)), "nz0 x nz1 must be 1..16"),
    ("out_dim 17", dict(PLAIN, o_pad=20, ints=dict(out_dim=17)), "refused by small_fwd_supported"),
    ("o_pitch < out_dim", dict(PLAIN, ints=dict(out_dim=9)), "o_pitch .OUT's pitch. is below out_dim"),
    ("rep 17", dict(F["small_fwd<0,0>"], M=96, jobs=[dict(head_row0=0, rows=170, rep=17)]), "refused by small_fwd_supported"),
    ("jobs with nz1 = 2", dict(F["small_fwd<0,0>"], nz1=2), "refused by small_fwd_supported"),
    ("jobs together with G", dict(F["small_fwd<0,0>"], gn=3), "refused by small_fwd_supported"),
    ("out_dim != 2 A", dict(F["small_fwd<1,0>"], ints=dict(A=5)), "refused by small_fwd_supported"),
    ("gc0 + gn > in0", dict(F["small_fwd<0,1>"], gc0=18), "refused by small_fwd_supported"),
    ("gn 9", dict(F["small_fwd<0,1>"], g_pad=4, ints=dict(gn=9)), "refused by small_fwd_supported"),
    ("G with out_dim 2", dict(F["small_fwd<1,1>"], out_dim=2), "refused by small_fwd_supported"),
    ("K != 2", dict(F["small_abwd<0>"], ints=dict(K=3)), "refused by small_abwd_supported"),
    ("A = 9", dict(F["small_abwd<0>"], ints=dict(A=9)), "refused by small_abwd_supported"),
    ("ga_pitch < A", dict(F["small_abwd<0>"], ga_pad=-1), "refused by small_abwd_supported"),
    ("misaligned W1", dict(PLAIN, off={"W1": 1}), "refused by small_fwd_supported"),
    ("misaligned H0", dict(PLAIN, off={"H0": 2}), "refused by small_fwd_supported"),
    ("misaligned W1, abwd", dict(F["small_abwd<0>"], off={"W1": 1}), "refused by small_abwd_supported"),
    ("misaligned H1, abwd", dict(F["small_abwd<1>"], off={"H1": 3}), "refused by small_abwd_supported"),
    ("misaligned Wh, abwd", dict(F["small_abwd<0>"], off={"Wh": 2}), "refused by small_abwd_supported"),
    ("X too short", dict(PLAIN, short={"X": 1}), "X: the array is shorter"),
    ("Wt too short", dict(PLAIN, short={"Wt": 3}), "Wt: the array is shorter"),
    ("OUT too short", dict(PLAIN, short={"OUT": 1}), "OUT: the array is shorter"),
    ("H1 too short", dict(PLAIN, short={"H1": 2}), "H1: the array is shorter"),
    ("G too short", dict(F["small_fwd<0,1>"], short={"G": 1}), "G: the array is shorter"),
    ("job.dst too short", dict(F["small_fwd<0,0>"], short={"job0.dst": 1}), "job.0..dst: the array is shorter"),
    ("job.eps too short", dict(F["small_fwd<0,0>"], short={"job0.eps": 5}), "job.0..eps: the array is shorter"),
    ("job.logp too short", dict(F["small_fwd<1,0>"], short={"job0.logp": 1}), "job.0..logp: the array is shorter"),
    ("a job past the head rows", dict(F["small_fwd<0,0>"], jobs=[dict(head_row0=1, rows=64, rep=1)]), "a job draws from head rows past M"),
    ("head too short", dict(F["small_abwd<0>"], short={"head": 1}), "head: the array is shorter"),
    ("ga too short", dict(F["small_abwd<0>"], short={"ga": 1}), "ga: the array is shorter"),
    ("qa too short", dict(F["small_abwd<1>"], short={"qa": 1}), "qa: the array is shorter"),
    ("xa too short", dict(F["small_abwd<0>"], short={"xa": 1}), "xa: the array is shorter"),
    ("out too short", dict(F["small_abwd<0>"], short={"out": 80000}), "out: the array is shorter"),
    ("part too short", dict(F["small_abwd<0>"], short={"part": 1}), "part: the array is shorter"),
    ("off_w1 past o_ks", dict(F["small_abwd<0>"], ints=dict(off_w1=40000)), "off_w1: the tensor does not fit the slab stride"),
    ("off_bh negative", dict(F["small_abwd<0>"], ints=dict(off_bh=-1)), "off_bh: the tensor does not fit the slab stride"),
    ("off_b0 inside w1", dict(F["small_abwd<0>"], ints=dict(off_b0=1000)), "overlaps"),
    ("a metric slot past nm", dict(F["small_abwd<0>"], ints=dict(m_alpha=5)), "the metric slots must lie in .0, nm."),
    ("gstep at an odd offset", dict(F["small_abwd<0>"], off_gstep=1), "gstep: one 64-bit value"),
]


def _build(kw):
    kw = dict(kw)
    og = kw.pop("off_gstep", None)
    c = s.build(**kw)
    if og is not None:
        c.arrays["gstep"].off = og
    return c


@pytest.mark.parametrize("label,kw,msg", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals_come_with_a_message_and_without_a_device(label, kw, msg):
    c = _build(kw)
    for dry in (0, 1):      # a real call is refused at the same check: it never reaches hipGetDeviceCount
        with pytest.raises(RuntimeError, match="orl_debug_small failed: orl_debug_small: .*" + msg):
            s.run(c, dry_run=dry)
    assert not s.DEVICE_ERRORS
    for name, a in c.arrays.items():
        assert np.array_equal(a.raw, c.before[name]), name


def test_refusals_of_array_combinations():
    c = s.build(**PLAIN)
    del c.arrays["OUT"]
    with pytest.raises(RuntimeError, match="OUT is required"):
        s.run(c)
    c = s.build(**F["small_abwd<0>"])
    c.arrays["ticket"].put(np.ones((1, 1, 1, 1), np.uint32))
    with pytest.raises(RuntimeError, match="ticket must be zero before a launch"):
        s.run(c)
    c = s.build(**F["small_abwd<0>"])
    c.arrays["OUT"] = s.build(**PLAIN).arrays["OUT"]
    with pytest.raises(RuntimeError, match="OUT does not belong to this launcher"):
        s.run(c)
    c = s.build(**PLAIN)
    c.arrays["head"] = s.build(**F["small_abwd<0>"]).arrays["head"]
    with pytest.raises(RuntimeError, match="head does not belong to this launcher"):
        s.run(c)
    c = s.build(**F["small_abwd<0>"])
    del c.arrays["hy"]
    with pytest.raises(RuntimeError, match="hy: 8 floats"):
        s.run(c)
    c = s.build(**F["small_fwd<0,0>"])
    del c.jobs[0]["dst"]
    with pytest.raises(RuntimeError, match="job.dst is required"):
        s.run(c)
    with pytest.raises(TypeError):
        _engine.debug_small("fwd", {"nonsense": None})
    with pytest.raises(TypeError):
        _engine.debug_small("fwd", {}, nonsense=1)


# ---- 4. float32 numpy against float64 on the GPU file's seeds: mask flips, K, KA, ADAM_K ----
def test_float32_numpy_on_the_chosen_seeds_flip_share_and_the_measured_constants():
    """K_LOGP, K_ACT and ADAM_K are twice the worst ratio measured HERE (float32 numpy against float64, the bound without its constant)"""
    flips, raw = 0.0, {"act": 0.0, "logp": 0.0, "adam": 0.0}
    const = {"act": s.K_ACT, "logp": s.K_LOGP, "adam": s.ADAM_K}
    for kind, fn in ALL_LISTS[:4]:
        for label, kw in fn():
            c = s.emulate(s.build(kind, **kw))
            res = s.check(c)
            for tag, r in res.items:
                k = tag.split(" ")[0]
                if k in raw:
                    raw[k] = max(raw[k], r * const[k])
            if kind == "fwd":
                for z in s._zz(c):
                    z0 = s.ref_layer(c.d["X"][z], c.d["W0"][z], c.d["b0"][z])
                    z1 = s.ref_layer(np.maximum(c.z32["z0", z], 0), c.d["W1"][z], c.d["b1"][z])
                    flips = max(flips, float(((c.z32["z0", z] > 0) != (z0 > 0)).mean()), float(((c.z32["z1", z] > 0) != (z1 > 0)).mean()))
    print("\nfloat32 numpy / float64, worst ratio without the constant:", {k: round(v, 3) for k, v in raw.items()}, "flip share", flips)
    assert flips < s.FLIP_SHARE, flips
    for k, v in raw.items():      # the constants are twice the measured ratio, rounded up to two digits (numpy's float32 exp / tanh / log differ a little between CPU families)
        assert const[k] / 3.0 <= v <= 1.1 * const[k] / 2.0, (k, v, const[k])


# ---- 5. the checks pass on a correct result and bite on a planted defect ----
@pytest.mark.parametrize("name", sorted(s.FLAVOURS))
def test_checks_pass_on_the_float32_emulation(name):
    res = s.check(s.emulate(s.build(**dict(s.FLAVOURS[name], M=96))))
    assert res.worst() < 0.75, res.worst()      # float32 numpy sits inside every bar (the K bars by their factor two: 0.5 where they were measured)


def _fails(c, msg):
    with pytest.raises(AssertionError, match=msg):
        s.check(c)


def _abwd(**kw):
    return s.emulate(s.build(**dict(F["small_abwd<1>"], M=96, runs=2, **kw)))


def _slab_put(c, r, g, k, data):
    out = c.arrays["out"]
    base = out.idx[r, 0, g, 0, c.offs[k]]
    out.raw.view(np.float32)[base:base + data.size] = np.asarray(data, np.float32).ravel()


def test_checks_bite_on_planted_defects_of_the_actor_backward():
    # a dropped row group: one slab's dW1 is zero; one row missing from one slab's dW0
    c = _abwd()
    _slab_put(c, 1, 2, "w1", np.zeros((256, 256)))
    _fails(c, "w1 slab 2 run 1")
    c = _abwd()
    dh = s.dhead32(c, 0)
    rows = slice(32, 64)
    dz0 = (c.d["H0"][0, 0][rows] > 0) * (((c.d["H1"][0, 0][rows] > 0) * (dh[rows] @ c.d["Wh"][0, 0])) @ c.d["W1"][0, 0])
    dz0[7] = 0
    _slab_put(c, 0, 1, "w0", dz0.T @ c.d["X"][0, 0][rows])
    _fails(c, "w0 slab 1 run 0")
    # two slabs swapped (their sum is still right)
    c = _abwd()
    a, b = s.slab_view(c, 0, 0, "wh").copy(), s.slab_view(c, 0, 1, "wh").copy()
    _slab_put(c, 0, 0, "wh", b), _slab_put(c, 0, 1, "wh", a)
    _fails(c, "wh slab 0 run 0")
    # a missing db0 column: left unwritten, or written as zero
    c = _abwd()
    _slab_put(c, 0, 1, "b0", np.zeros(256))
    _fails(c, "b0 slab 1 run 0")
    c = _abwd()
    out = c.arrays["out"]
    out.raw[out.idx[0, 0, 1, 0, c.offs["b0"]:c.offs["b0"] + 256]] = s.GEMM_SENTINEL
    _fails(c, "left unwritten")
    # a tie split 1 / 0; the clamp edges taken exclusive
    for defect, tag in (("tie", "bh slab 0"), ("clamp", "bh slab 0")):
        s.DEFECT = defect
        try:
            c = _abwd()
        finally:
            s.DEFECT = None
        _fails(c, tag)
    # touched sentinels: a gap inside a slab, a head row >= 2A, a slab >= groups, a part slot >= groups, a ticket left at 1, an operand
    c = _abwd()
    out = c.arrays["out"]
    out.raw[out.idx[0, 0, 0, 0, c.offs["bh"] + 2 * c.A]] = 0
    _fails(c, "between the tensors of a slab")
    c = _abwd()
    out = c.arrays["out"]
    out.raw[out.idx[1, 0, 1, 0, c.offs["wh"] + 2 * c.A * 256 + 5]] = 0
    _fails(c, "between the tensors of a slab")
    c = _abwd()
    out = c.arrays["out"]
    out.raw[out.idx[1, 0, 3, 0, c.offs["w1"] + 9]] = 0
    _fails(c, "a slab >= groups was written")
    c = _abwd()
    p = c.arrays["part"]
    p.raw[p.idx[0, 0, 0, 3, 1]] = 0
    _fails(c, "a part slot >= groups was written")
    c = _abwd()
    c.arrays["ticket"].raw[c.arrays["ticket"].idx[1, 0, 0, 0, 0]] = 1
    _fails(c, "the ticket is not back at 0")
    c = _abwd()
    c.arrays["H1"].raw[11] ^= 1
    _fails(c, "an operand came back changed")
    # scalars: another RunScalars field touched, a stale alpha_bwd, a group's partial sums missing from the metric
    c = _abwd()
    sc = c.arrays["sc"]
    sc.raw[sc.idx[0, 0, 0, 0, 4]] ^= 1
    _fails(c, "RunScalars field changed")
    c = _abwd()
    sc = c.arrays["sc"]
    sc.raw.view(np.float32)[sc.idx[1, 0, 0, 0, s.SC["alpha_bwd"]]] = c.arrays["sc"].get()[1, 0, 0, 0, s.SC["alpha"]]
    _fails(c, "alpha_bwd is not the alpha the backward used")
    c = _abwd()
    ml = c.arrays["metrics_last"]
    ml.raw.view(np.float32)[ml.idx[0, 0, 0, 0, c.m_actor]] -= c.arrays["part"].get()[0, 0, 0, 2, 0] / 96
    _fails(c, "metric actor run 0")


def test_checks_bite_on_planted_defects_of_the_forward():
    kw = dict(F["small_fwd<1,0>"], M=96, jobs=[dict(head_row0=32, rows=100, rep=3, dst_row0=2, dst_col=1, dst_pad=1)])
    # a sample written one row late
    c = s.emulate(s.build(**kw))
    a = c.arrays["job0.dst"]
    v = a.get().copy()
    v[0, 0, 0, 1:] = v[0, 0, 0, :-1]
    a.put(v)
    _fails(c, "act job 0|a saturated action")
    # the log-probability of the neighbouring row
    c = s.emulate(s.build(**kw))
    a = c.arrays["job0.logp"]
    v = a.get().copy()
    v[0, 0, 0, 3:6] = v[0, 0, 0, 6:9]
    a.put(v)
    _fails(c, "logp job 0")
    # a stale row group of H1; the tail bias dropped; one G column from the neighbouring input column
    c = s.emulate(s.build(**kw))
    a = c.arrays["H1"]
    v = a.get().copy()
    v[0, 0, 0, 64:96] = v[0, 0, 0, 32:64]
    a.put(v)
    _fails(c, "H1|the sign of a unit differs")
    c = s.emulate(s.build(**kw))
    a = c.arrays["OUT"]
    a.put(a.get() - c.d["bt"].reshape(1, 1, 1, 1, -1))
    _fails(c, "OUT")
    c = s.emulate(s.build(**dict(F["small_fwd<0,1>"], M=96)))
    a = c.arrays["G"]
    v = a.get().copy()
    v[..., 2] = v[..., 3]
    a.put(v)
    _fails(c, "'G'")
    # touched sentinels: an OUT pad column, a dst column outside the job's, a row past job.rows, an operand
    c = s.emulate(s.build(**kw))
    c.arrays["OUT"].raw[c.arrays["OUT"].idx[0, 0, 0, 5, 11] + 1] = 0
    _fails(c, "outside the logical result")
    c = s.emulate(s.build(**kw))
    a = c.arrays["job0.dst"]
    a.raw[a.idx[0, 0, 0, 7, 0] - 1] = 0
    _fails(c, "outside the logical result")
    c = s.emulate(s.build(**kw))
    a = c.arrays["job0.dst"]
    a.raw[a.idx[0, 0, 0, 99, 0] + a.pitch] = 0
    _fails(c, "outside the logical result")
    c = s.emulate(s.build(**kw))
    c.arrays["W0"].raw[3] ^= 1
    _fails(c, "an operand came back changed")
