"""CPU: (1) the float64 numpy references of tests/gemm_cases.py against torch's float64 functions and autograd -- a wrong reference must
not certify a wrong kernel; (2) the refusals of the wide GEMM tap (orl_debug_gemm_ex): its argument checks run before any device call,
so every one of them raises with its message on a machine without a GPU; (3) the tap's report (loaders, mapping, store path), which is
computed on the host, for a few launches whose path is known from csrc/gemm.h."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as g


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64)


def test_swish_and_its_derivative_match_torch_autograd():
    z = np.concatenate([np.random.RandomState(0).standard_normal(500) * 4, [0.0, -0.0, 30.0, -30.0, 1e-8]])
    zt = _t(z).requires_grad_(True)
    h = F.silu(zt)
    h.sum().backward()
    assert np.abs(g.swish(z) - h.detach().numpy()).max() < 1e-14
    assert np.abs(g.dswish(z) - zt.grad.numpy()).max() < 1e-14


def test_leaky_and_its_rule_at_zero_match_torch():
    v = np.concatenate([np.random.RandomState(1).standard_normal(500), [0.0, -0.0]])
    vt = _t(v).requires_grad_(True)
    h = F.leaky_relu(vt, 0.01)
    h.sum().backward()
    assert np.abs(g.leaky(v) - h.detach().numpy()).max() < 1e-16
    # leaky_relu_backward gives the slope at zero; the kernel reads the rule off the stored activation h, which has v's sign
    assert np.array_equal(g.leaky_factor(h.detach().numpy()), vt.grad.numpy())
    assert vt.grad[-1].item() == 0.01 and vt.grad[-2].item() == 0.01
    assert np.array_equal(g.leaky_factor(np.array([0.0, -0.0, 1e-30, -1e-30], np.float32)), [0.01, 0.01, 1.0, 0.01])


@pytest.mark.parametrize("epi", [g.E_MASK, g.E_SWISH_GRAD, g.E_LEAKY_MASK])
def test_backward_epilogues_match_torch_autograd(epi):
    """C = dY W (.) act'(.) is autograd's input gradient of act(z) for upstream dY W"""
    rng = np.random.RandomState(2 + epi)
    acc, z = rng.standard_normal((7, 9)), rng.standard_normal((7, 9))
    zt = _t(z).requires_grad_(True)
    act = {g.E_MASK: torch.relu, g.E_SWISH_GRAD: F.silu, g.E_LEAKY_MASK: lambda x: F.leaky_relu(x, 0.01)}[epi](zt)
    act.backward(_t(acc))
    aux = z if epi == g.E_SWISH_GRAD else act.detach().numpy()      # the ReLU / LeakyReLU flavours read the stored activation
    c, _ = g.epilogue(epi, acc, aux=aux)
    assert np.abs(c - zt.grad.numpy()).max() < 1e-14


@pytest.mark.parametrize("epi", [g.E_BIAS, g.E_BIAS_RELU, g.E_BIAS_SWISH, g.E_BIAS_LEAKY])
def test_forward_epilogues_match_torch(epi):
    rng = np.random.RandomState(20 + epi)
    x, w, b = rng.standard_normal((5, 6)), rng.standard_normal((4, 6)), rng.standard_normal(4)
    lin = F.linear(_t(x), _t(w), _t(b))
    want = {g.E_BIAS: lin, g.E_BIAS_RELU: torch.relu(lin), g.E_BIAS_SWISH: F.silu(lin), g.E_BIAS_LEAKY: F.leaky_relu(lin, 0.01)}[epi]
    c, z = g.epilogue(epi, g.product(0, x, w), bias=b)
    assert np.abs(c - want.numpy()).max() < 1e-14
    if epi == g.E_BIAS_SWISH:
        assert np.abs(z - lin.numpy()).max() < 1e-14


def test_products_and_weight_gradient_match_torch_autograd():
    rng = np.random.RandomState(3)
    x, w, dy = rng.standard_normal((11, 6)), rng.standard_normal((4, 6)), rng.standard_normal((11, 4))
    xt, wt = _t(x).requires_grad_(True), _t(w).requires_grad_(True)
    bt = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    F.linear(xt, wt, bt).backward(_t(dy))
    assert np.abs(g.product(1, dy, w) - xt.grad.numpy()).max() < 1e-14              # dgrad: dY [M][K] W [K][N]
    assert np.abs(g.product(2, dy, x) - wt.grad.numpy()).max() < 1e-14              # wgrad: dY^T X
    assert np.abs(dy.sum(0) - bt.grad.numpy()).max() < 1e-14                        # bias_out


def test_mask_words_layout_and_round_trip():
    pos = np.random.RandomState(4).standard_normal((3, 5, 70)) > 0
    w = g.pack_mask(pos)
    assert w.shape == (3, 5, 3) and w.dtype == np.uint32
    for r, c in [(0, 0), (1, 31), (2, 32), (3, 63), (4, 69)]:
        assert bool((w[1, r, c // 32] >> np.uint32(c % 32)) & 1) == bool(pos[1, r, c])
    assert (w[..., 2] >> np.uint32(6)).max() == 0                                   # columns 70 .. 95 do not exist
    assert np.array_equal(g.unpack_mask(w, 70), pos)
    one = np.zeros((1, 64), bool)
    one[0, 33] = True
    assert g.pack_mask(one).tolist() == [[0, 2]]


def test_fused_tail_and_layer0_formulas_match_torch_autograd():
    rng = np.random.RandomState(5)
    x, w, b, wt, bt = rng.standard_normal((9, 6)), rng.standard_normal((8, 6)), rng.standard_normal(8), rng.standard_normal(8), 0.3
    q = F.linear(torch.relu(F.linear(_t(x), _t(w), _t(b))), _t(wt)[None], _t([bt]))[:, 0]
    assert np.abs(g.tail_q(x, w, b, wt, bt) - q.numpy()).max() < 1e-14
    # layer 0 of a two-layer net: h0 = relu(x0 W0^T + b0), upstream gradient dz1 through W1
    x0, w0, b0 = rng.standard_normal((9, 5)), rng.standard_normal((6, 5)), rng.standard_normal(6)
    w1, dz1 = rng.standard_normal((4, 6)), rng.standard_normal((9, 4))
    w0t, b0t = _t(w0).requires_grad_(True), _t(b0).requires_grad_(True)
    h0 = torch.relu(F.linear(_t(x0), w0t, b0t))
    F.linear(h0, _t(w1)).backward(_t(dz1))
    dz0, _ = g.epilogue(g.E_MASK, g.product(1, dz1, w1), aux=h0.detach().numpy())
    dw, db = g.w0_grad(dz0, x0)
    assert np.abs(dw - w0t.grad.numpy()).max() < 1e-14 and np.abs(db - b0t.grad.numpy()).max() < 1e-14


def test_rank1_operand_matches_old_tap_formula():
    rng = np.random.RandomState(6)
    h, dq, w = rng.standard_normal((7, 5)).astype(np.float32), rng.standard_normal(7).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    assert np.abs(g.rank1(h > 0, dq, w) - (h > 0) * np.outer(dq.astype(np.float64), w.astype(np.float64))).max() < 1e-6


# ---- refusals: raised by the argument checks, before the device is looked for ----
def _set(name, **kw):
    def extra(res, arrays, ints):
        for k, v in kw.items():
            setattr(arrays[name], k, v)
    return extra


def _add(**specs):
    """side-output arrays: name -> (rows, cols, kwargs)"""
    def extra(res, arrays, ints):
        from offlinerlkit._engine import GemmArray
        for name, (rows, cols, kw) in specs.items():
            arrays[name] = GemmArray(rows, cols, **kw)
    return extra


TAIL = dict(tq_w=(1, 40, {}), tq_b=(1, 1, {}), tq_out=(70, 1, {}), tq_part=(1, 70, {}))
W0 = dict(w0_x=(70, 12, {}), w0_out=(40, 11, {"nslab": 2}), w0_bias=(1, 40, {"nslab": 2, "kstride": 464}))      # (40 + 2) rows x 11 -> 464
REFUSALS = [
    ("cfg must be 0..6", dict(cfg=7, epi=g.E_PLAIN)),
    ("precision must be", dict(cfg=0, epi=g.E_PLAIN, precision=3)),
    ("epi must be 0..8", dict(cfg=0, epi=9, layout=0)),
    ("layout 2 goes with the weight-gradient", dict(cfg=0, epi=g.E_BIAS, layout=2)),
    ("layout 2 goes with the weight-gradient", dict(cfg=0, epi=g.E_WGRAD, layout=1)),
    ("rank-1 operand is instantiated for epi 0, 3 and 4", dict(cfg=0, epi=g.E_BIAS_RELU, pa=1)),
    ("nz0 x nz1 must be", dict(cfg=0, epi=g.E_PLAIN, ints=dict(nz0=0))),
    ("ksplit must be", dict(cfg=0, epi=g.E_WGRAD, ints=dict(ksplit=0))),
    ("split-K slabs exist for the weight-gradient", dict(cfg=0, epi=g.E_PLAIN, ints=dict(ksplit=2))),
    ("a_kpad is for a k-contiguous plain A", dict(cfg=0, epi=g.E_WGRAD, ints=dict(a_kpad=1))),
    ("transposed store belongs to the weight-gradient", dict(cfg=0, epi=g.E_PLAIN, ints=dict(c_trans=1))),
    ("C may be left out only with the fused layer-0", dict(cfg=0, epi=g.E_MASK, ints=dict(c_null=1))),
    ("A's pitch is below its width", dict(cfg=0, epi=g.E_PLAIN, extra=_set("A", pitch=22))),
    ("B's pitch is below its width", dict(cfg=0, epi=g.E_PLAIN, extra=_set("B", pitch=23))),
    ("C's pitch is below its width", dict(cfg=0, epi=g.E_PLAIN, extra=_set("C", pitch=39))),
    ("aux's pitch is below its width", dict(cfg=0, epi=g.E_MASK, extra=_set("aux", pitch=39))),
    ("C: the array is shorter", dict(cfg=0, epi=g.E_PLAIN, extra=_set("C", off=10 ** 6))),
    ("A: the array is shorter", dict(cfg=0, epi=g.E_PLAIN, extra=_set("A", s0=10 ** 6), nz=(2, 1))),
    ("bias: negative offset", dict(cfg=0, epi=g.E_BIAS, extra=_set("bias", off=-1))),
    ("C: problems or slabs of a result overlap", dict(cfg=0, epi=g.E_PLAIN, extra=_set("C", s1=8), nz=(1, 2))),
    ("z_out has C's geometry", dict(cfg=0, epi=g.E_BIAS_SWISH, extra=_set("z_out", n=16))),
    ("mask words are emitted by the ReLU forward", dict(cfg=0, epi=g.E_BIAS, extra=_add(mb_out=(70, 2, {"dtype": np.uint32})))),
    ("mask words need a tile with 8 lanes", dict(cfg=0, epi=g.E_BIAS_RELU, extra=_add(mb_out=(70, 2, {"dtype": np.uint32})))),      # N = 40
    ("mask words need a tile with 8 lanes", dict(cfg=g.CFG_TALL, epi=g.E_BIAS_RELU, shape=(70, 64, 24), extra=_add(mb_out=(70, 2, {"dtype": np.uint32})))),
    ("mask words need a tile with 8 lanes", dict(cfg=16, epi=g.E_BIAS_RELU, shape=(70, 64, 24), extra=_add(mb_out=(70, 2, {"dtype": np.uint32})))),
    ("mb_out's pitch is below its width", dict(cfg=0, epi=g.E_BIAS_RELU, shape=(70, 64, 24), extra=_add(mb_out=(70, 1, {"dtype": np.uint32})))),
    ("fused tail belongs to the ReLU forward", dict(cfg=0, epi=g.E_BIAS, extra=_add(**TAIL))),
    ("fused tail runs on CFG_BIG and CFG_SQ8", dict(cfg=g.CFG_MID, epi=g.E_BIAS_RELU, extra=_add(**TAIL))),
    ("fused tail runs on CFG_BIG and CFG_SQ8", dict(cfg=0, epi=g.E_BIAS_RELU, geo={"C": {"off": 1}}, extra=_add(**TAIL))),
    ("fused tail needs tq_w, tq_b and tq_out", dict(cfg=0, epi=g.E_BIAS_RELU, extra=_add(tq_w=(1, 40, {})))),
    ("aux_bits belongs to the mask epilogue", dict(cfg=0, epi=g.E_LEAKY_MASK, extra=_add(aux_bits=(70, 2, {"dtype": np.uint32})))),
    ("reads packed words only on the LDS-staged store", dict(cfg=0, epi=g.E_MASK, shape=(70, 38, 24), extra=_add(aux_bits=(70, 2, {"dtype": np.uint32})))),
    ("fused layer-0 gradient belongs to the mask epilogue", dict(cfg=0, epi=g.E_PLAIN, layout=1, extra=_add(**W0))),
    ("fused layer-0 gradient runs where pick_cfg chooses", dict(cfg=g.CFG_SQ8, epi=g.E_MASK, extra=_add(**W0), ints=dict(w0_in=11))),
    ("fused layer-0 gradient runs where pick_cfg chooses", dict(cfg=0, epi=g.E_MASK, extra=_add(**W0), ints=dict(w0_in=11))),      # pick_cfg: CFG_SMALL
    ("a_bits goes with pa 2", dict(cfg=0, epi=g.E_MASK, extra=_add(a_bits=(70, 2, {"dtype": np.uint32})))),
    ("mask words runs on CFG_BIG and CFG_SQ", dict(cfg=g.CFG_MID, epi=g.E_MASK, pa=2, shape=(70, 40, 64))),
    ("needs K % 32 == 0", dict(cfg=0, epi=g.E_MASK, pa=2, shape=(70, 40, 64), ints=dict(K=48))),
    ("refused by rank1_bits_supported", dict(cfg=0, epi=g.E_MASK, pa=2, shape=(70, 40, 64), geo={"colv": {"off": 1}})),
]


@pytest.mark.parametrize("idx", range(len(REFUSALS)), ids=[f"{i}-{r[0][:24].replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_tap_refuses_before_touching_a_device(idx):
    msg, kw = REFUSALS[idx]
    kw = dict(kw)
    kw.setdefault("shape", (70, 40, 24))
    # dry_run is NOT set: the refusal must come before the search for a device ("no HIP device" here)
    with pytest.raises(RuntimeError, match="orl_debug_gemm_ex failed: orl_debug_gemm_ex: .*" + msg):
        g.run_case(**kw)


def test_tap_passes_its_checks_then_asks_for_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        g.run_case(0, g.E_BIAS_RELU, (70, 40, 24))


# ---- the report, for launches whose path follows from csrc/gemm.h by hand ----
def _rep(*a, **kw):
    return g.run_case(*a, dry_run=True, **kw).report


def test_report_loaders():
    V, B4, VU, S = g.L_VECK, g.L_BLK4, g.L_VECKU, g.L_SCALAR
    r = _rep(0, g.E_BIAS, (70, 40, 24))                                          # k-contiguous, K % 4 == 0, aligned
    assert (r["la"], r["lb"]) == (V, V)
    r = _rep(0, g.E_BIAS, (70, 40, 23), a_kpad=True)                             # zero-padded A rows; B rows 23 floats long
    assert (r["la"], r["lb"]) == (V, VU)
    r = _rep(0, g.E_BIAS, (70, 40, 23))                                          # A would take VECKU, which no launch instantiates on A
    assert (r["la_pick"], r["lb_pick"], r["la"], r["lb"]) == (VU, VU, S, S)
    r = _rep(0, g.E_MASK, (70, 40, 24))                                          # dgrad: B row-contiguous
    assert (r["la"], r["lb"]) == (V, B4)
    r = _rep(0, g.E_MASK, (70, 40, 24), geo={"B": {"off": 1}})
    assert (r["la"], r["lb"]) == (V, S)
    r = _rep(0, g.E_WGRAD, (72, 40, 23))
    assert (r["la"], r["lb"]) == (B4, B4)
    r = _rep(0, g.E_WGRAD, (70, 40, 23))                                          # A's pitch 70 is no multiple of 4
    assert (r["la_pick"], r["lb_pick"], r["la"], r["lb"]) == (S, B4, S, S)
    r = _rep(16, g.E_BIAS, (70, 40, 24))
    assert (r["la_pick"], r["lb_pick"], r["la"], r["lb"]) == (V, V, S, S)
    r = _rep(0, g.E_PLAIN, (70, 40, 24), layout=1, pa=1, geo={"colv": {"off": 1}})   # rank-1: colv is read with the operand's vector shape
    assert (r["la_pick"], r["la"], r["lb"]) == (V, S, S)


def test_report_store_paths_and_mapping():
    assert _rep(2, g.E_BIAS, (70, 40, 24))["store"] == g.ST_LDS
    assert _rep(2, g.E_BIAS, (70, 38, 24), geo={"C": {"pad": 2}})["store"] == g.ST_VEC
    assert _rep(2, g.E_BIAS, (70, 38, 24))["store"] == g.ST_SCALAR
    assert _rep(2, g.E_BIAS, (70, 40, 24), geo={"C": {"off": 1}})["store"] == g.ST_SCALAR
    assert _rep(2, g.E_BIAS, (70, 40, 24), geo={"bias": {"off": 1}})["store"] == g.ST_SCALAR
    assert _rep(2, g.E_LEAKY_MASK, (70, 40, 24), geo={"aux": {"pad": 1}})["store"] == g.ST_SCALAR
    r = _rep(2, g.E_BIAS, (70, 40, 24), nz=(1, 2), geo={"C": {"stride_pad": 2}})      # every other problem starts 8 bytes off
    assert r["store"] == g.ST_LDS and r["store_mixed"] == 1
    assert _rep(g.CFG_MID, g.E_WGRAD, (64, 64, 100), c_trans=True)["store"] == g.ST_TRANS
    assert _rep(g.CFG_MID, g.E_WGRAD, (62, 64, 100), c_trans=True)["store"] == g.ST_SCALAR
    assert _rep(g.CFG_BIG, g.E_WGRAD, (64, 64, 100), c_trans=True)["store"] == g.ST_SCALAR      # no square tile
    assert _rep(g.CFG_WG, g.E_BIAS, (70, 40, 24), precision=2)["cfg"] == g.CFG_SQ
    # (70, 40, 23) on the 16 x 64 tile: 5 tiles.  z-major from 8 problems; never for a single work item per problem
    assert [_rep(2, g.E_BIAS, (70, 40, 23), nz=z)["zmajor"] for z in [(1, 2), (3, 2), (9, 1), (11, 1), (8, 2)]] == [0, 0, 1, 1, 1]
    assert _rep(2, g.E_BIAS, (13, 40, 23), nz=(9, 1))["zmajor"] == 0
    assert _rep(2, g.E_WGRAD, (13, 40, 70), nz=(9, 1), ksplit=3)["zmajor"] == 1
    assert _rep(g.CFG_BIG, g.E_BIAS, (300, 300, 23), nz=(9, 1))["zmajor"] == 1      # 5 x 2 tiles
    assert _rep(g.CFG_MID, g.E_BIAS, (300, 300, 23), nz=(9, 1))["zmajor"] == 0      # 25 tiles: above the z-major limit of 16


def test_case_lists_reach_every_path():
    """dry runs of what tests/test_gpu_gemm_paths.py launches: per epilogue x tile shape, store path x epilogue, loader pair x tile shape,
    workgroup mapping and side output, the tap reports the path taken at least once"""
    epi_cfg, store_epi, pair_cfg, mapping = set(), set(), set(), set()
    for cfg in g.ALL_CFGS:
        for mode in g.MODES:
            r = g.run_case(dry_run=True, **next(iter(g.tile_cases(cfg, mode, [(65, 68, 33)]))))
            epi_cfg.add((r.epi, r.report["cfg"], cfg >> 4))
    assert epi_cfg == {(e, c, s) for e in range(9) for c in range(7) for s in (0, 1)}
    for _, kw, path in g.store_cases():
        r = g.run_case(dry_run=True, **kw)
        assert r.report["store"] == path
        store_epi.add((r.epi, path))
    assert store_epi == {(e, p) for e in range(9) for p in (g.ST_LDS, g.ST_VEC, g.ST_SCALAR)}
    for _, kw, pick, pair in g.loader_cases():
        r = g.run_case(dry_run=True, **kw).report
        assert (r["la_pick"], r["lb_pick"], r["la"], r["lb"]) == pick + pair
        if kw["precision"] == 0:
            pair_cfg.add((pair, r["cfg"]))
    V, B4, VU, S = g.L_VECK, g.L_BLK4, g.L_VECKU, g.L_SCALAR
    assert pair_cfg == {(p, c) for p in [(V, V), (V, B4), (B4, B4), (V, VU), (V, S), (S, S)] for c in range(7)}      # all that launch_cfg instantiates
    for _, kw, zm in g.batch_cases():
        r = g.run_case(dry_run=True, **kw)
        assert r.report["zmajor"] == zm
        nz = kw["nz"][0] * kw["nz"][1]
        mapping.add((zm, nz % 8 == 0, r.epi == g.E_WGRAD and kw["ksplit"] == 3))
    assert {(1, False, False), (1, True, False), (0, False, False), (1, False, True), (1, True, True)} <= mapping
    # side outputs
    for cfg in (g.CFG_BIG, g.CFG_MID, g.CFG_SMALL, g.CFG_SQ, g.CFG_SQ8, g.CFG_WG):
        assert g.mask_words_case(cfg, 70, 96, nz=(2, 2), dry_run=True).report["mb"] == 1
        act = np.random.RandomState(0).standard_normal((1, 1, 1, 70, 96)).astype(np.float32)
        r = g.masked_dgrad_case(cfg, act, g.pack_mask(act > 0), dry_run=True).report
        assert r["aux_bits"] == 1 and r["store"] == g.ST_LDS
    for cfg in (g.CFG_BIG, g.CFG_SQ):
        assert g.rank1_bits_case(cfg, nz=(2, 3), dry_run=True).report["a_bits"] == 1
    assert g.fused_tail_case(g.CFG_BIG, dry_run=True).report["tq_parts"] == 2 and g.fused_tail_case(g.CFG_SQ8, dry_run=True).report["tq_parts"] == 3
    assert g.fused_w0_case(g.CFG_BIG, (1, 2), 23, True, M=2051, dry_run=True).report["w0_slabs"] == 33
    assert g.fused_w0_case(g.CFG_BIG, (1, 1), 11, False, True, dry_run=True).report["w0_slabs"] == 33
    for cfg in (g.CFG_MID, g.CFG_SQ, g.CFG_SQ8):
        assert g.transposed_case(cfg, (64, 64, 100), dry_run=True).report["store"] == g.ST_TRANS
        assert g.transposed_case(cfg, (62, 64, 100), dry_run=True).report["store"] == g.ST_SCALAR
