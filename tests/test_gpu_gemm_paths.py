"""GPU: every epilogue, tile shape, operand loader, store path, batch mapping and fused side output of the tiled GEMM template
(csrc/gemm_kernel.h) through the wide tap (orl_debug_gemm_ex), against float64 numpy (tests/gemm_cases.py) at the smallest shapes that
cross a tile edge.  Error measure and bars are those of tests/test_gpu_gemm.py: max abs error over max |ref| below 2e-5 (precision 0
and 2) / 2e-4 (precision 1).  Every problem of a batch has its own data and its own check.  After EVERY launch the words outside the
logical results (pad columns, guard rows, guard bands between problems and slabs, the band before an offset base) must still hold
the sentinel bit for bit, and a launch that was meant to take a path asserts from the tap's report that it did."""
import numpy as np
import pytest

import gemm_cases as g

pytestmark = pytest.mark.gpu


def _run_all(cases):
    """runs (label, kwargs, expectations) triples; reports every failing label at once"""
    bad = []
    for label, kw, expect in cases:
        res = g.run_case(**kw)
        try:
            for k, v in expect.items():
                assert res.report[k] == v, f"path not taken: report[{k}] = {res.report[k]}, wanted {v}"
            g.check_case(res)
        except AssertionError as e:
            bad.append(f"{label}: {e}")
    assert not bad, "\n".join(bad)


# ---- a. every tile shape at its own edges ----
@pytest.mark.parametrize("mode", list(g.MODES))
@pytest.mark.parametrize("cfg", g.ALL_CFGS)
def test_every_tile_and_epilogue_at_tile_edges(cfg, mode):
    _run_all((f"{kw['shape']} ksplit {kw['ksplit']}", kw, {"cfg": cfg & 15}) for kw in g.tile_cases(cfg, mode))


@pytest.mark.parametrize("precision", [1, 2])
@pytest.mark.parametrize("mode", list(g.MODES))
@pytest.mark.parametrize("cfg", list(range(7)) + [g.CFG_MID | 16])
def test_split_precisions_at_tile_edges(cfg, mode, precision):
    """two and three 16-bit planes; the 256 x 128 tile's three-plane buffers exceed the LDS, so the launcher reroutes it to 128 x 128"""
    ran = g.CFG_SQ if (cfg == g.CFG_WG and precision == 2) else cfg & 15
    _run_all((f"{kw['shape']} ksplit {kw['ksplit']}", kw, {"cfg": ran}) for kw in g.tile_cases(cfg, mode, g.SPLIT_SHAPES, precision))


# ---- b. the new epilogues where they branch ----
@pytest.mark.parametrize("cfg", [g.CFG_SMALL, g.CFG_SQ8, g.CFG_TALL | 16])
@pytest.mark.parametrize("variant", ["lds", "vec", "scalar_base"])
def test_leaky_forward_at_exact_zero(cfg, variant):
    """K = 1 with A = 1 and bias = -w makes the pre-activation an exact zero in every even column (-0.0 cannot be produced: the
    accumulator starts at +0.0); v > 0 is false there and the slope branch must return an exact zero, on each store path"""
    N, geo, path = {"lds": (72, {}, g.ST_LDS), "vec": (70, {"C": {"pad": 2}}, g.ST_VEC), "scalar_base": (72, {"C": {"off": 1}}, g.ST_SCALAR)}[variant]
    M = 19
    rng = np.random.RandomState(N + cfg)
    w = rng.standard_normal(N).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    b[0::2] = -w[0::2]
    data = g.Result()
    data.d = {"A": np.ones((1, 1, 1, M, 1), np.float32), "B": w.reshape(1, 1, 1, N, 1), "bias": b.reshape(1, 1, 1, 1, N)}
    res = g.run_case(cfg, g.E_BIAS_LEAKY, (M, N, 1), data=data, geo=geo)
    assert res.report["store"] == path
    g.check_case(res)
    c = res.arrays["C"].get()[0, 0, 0]
    assert np.all(c[:, 0::2] == 0.0)
    v = (w.astype(np.float64) + b)[1::2]
    assert np.allclose(c[:, 1::2], np.where(v > 0, v, 0.01 * v)[None], rtol=1e-6, atol=0)


@pytest.mark.parametrize("cfg", [g.CFG_SMALL, g.CFG_SQ8, g.CFG_TALL | 16])
@pytest.mark.parametrize("variant", ["lds", "vec", "scalar_base", "scalar_aux_base"])
def test_leaky_mask_takes_the_slope_at_zero_of_either_sign(cfg, variant):
    """the stored activation holds exact +0.0 and -0.0 among values of both signs: zero takes the 0.01 slope (leaky_relu_backward)"""
    N, geo, path = {"lds": (72, {}, g.ST_LDS), "vec": (70, {"C": {"pad": 2}, "aux": {"pad": 2}}, g.ST_VEC),
                    "scalar_base": (72, {"C": {"off": 1}}, g.ST_SCALAR), "scalar_aux_base": (72, {"aux": {"off": 1}}, g.ST_SCALAR)}[variant]
    res = g.run_case(cfg, g.E_LEAKY_MASK, (19, N, 24), zeros=True, geo=geo, seed=31 + cfg)
    assert res.report["store"] == path
    g.check_case(res)
    h = res.d["aux"][0, 0, 0]
    acc = g.product(1, res.d["A"][0, 0, 0], res.d["B"][0, 0, 0])
    c = res.arrays["C"].get()[0, 0, 0].astype(np.float64)
    zero = h == 0
    assert zero.sum() > 100 and np.signbit(h[zero]).any() and not np.signbit(h[zero]).all() and (h > 0).any() and (h < 0).any()
    assert g.rel_err(c[zero], 0.01 * acc[zero]) < 2e-5
    assert g.rel_err(c[h > 0], acc[h > 0]) < 2e-5 and g.rel_err(c[h < 0], 0.01 * acc[h < 0]) < 2e-5


@pytest.mark.parametrize("cfg", [g.CFG_SMALL, g.CFG_SQ8, g.CFG_BIG | 16])
@pytest.mark.parametrize("variant", ["lds", "vec", "scalar_base"])
def test_swish_pair_over_a_wide_range(cfg, variant):
    """h = z sigmoid(z) and the stored z on the three store paths, then the dgrad scaled by the closed form sigmoid(z)(1 + z(1 - sigmoid(z)))
    reading that z back, with pre-activations out to the saturated ends (|z| up to ~40: bias on a grid over [-30, 30]).  The kernel
    evaluates exp and the reciprocal with the hardware instructions; both epilogues are held to the 2e-5 bar of the fp32 kernels
    (measured on the MI355X: h and z 1e-7, the dgrad 5e-7 .. 9e-7 -- no wider bar is needed)."""
    N, geo, path = {"lds": (72, {}, g.ST_LDS), "vec": (70, {"C": {"pad": 2}, "aux": {"pad": 2}}, g.ST_VEC),
                    "scalar_base": (72, {"C": {"off": 1}}, g.ST_SCALAR)}[variant]
    M, K = 37, 24
    rng = np.random.RandomState(cfg + N)
    data = g.Result()
    data.d = {"A": rng.standard_normal((1, 1, 1, M, K)).astype(np.float32), "B": rng.standard_normal((1, 1, 1, N, K)).astype(np.float32),
              "bias": np.linspace(-30, 30, N).astype(np.float32).reshape(1, 1, 1, 1, N)}
    fwd = g.run_case(cfg, g.E_BIAS_SWISH, (M, N, K), data=data, geo=geo)
    assert fwd.report["store"] == path
    print("swish forward", variant, "h", g.rel_err(fwd.arrays["C"].get()[0, 0, 0], fwd.ref_c[0, 0]), "z", g.rel_err(fwd.arrays["z_out"].get()[0, 0, 0], fwd.ref_z[0, 0]))
    g.check_case(fwd)
    z = fwd.arrays["z_out"].get()[0, 0]      # what the forward stored is what the backward reads
    assert np.abs(z).max() > 30
    back = g.Result()
    back.d = {"aux": z.reshape(1, 1, 1, M, N)}
    bwd = g.run_case(cfg, g.E_SWISH_GRAD, (M, N, K), data=back, geo=geo, seed=5)
    assert bwd.report["store"] == path
    print("swish backward", variant, g.rel_err(bwd.arrays["C"].get()[0, 0, 0], bwd.ref_c[0, 0]))
    g.check_case(bwd)


# ---- c. pitches, alignment, guards ----
def test_every_epilogue_on_every_store_path():
    """row pitches above the logical width and bases off the 16-byte grid: the LDS-staged, the direct 16-byte and the scalar store of
    all nine epilogues (aux with exact zeros), each asserted from the report"""
    _run_all((label, kw, {"store": path, "store_mixed": 0}) for label, kw, path in g.store_cases())


def test_every_loader_pair_on_every_tile():
    """VECK / VECKU / BLK4 / scalar per operand from pitch, base alignment and a_kpad, for the plain and the rank-1 operand"""
    _run_all((label, kw, {"la_pick": pick[0], "lb_pick": pick[1], "la": pair[0], "lb": pair[1]}) for label, kw, pick, pair in g.loader_cases())


def test_a_misaligned_problem_in_an_aligned_batch():
    """z strides that are no multiple of 4: every other problem starts off the 16-byte grid and takes the scalar store and loaders' fall-back"""
    res = g.run_case(g.CFG_SMALL, g.E_BIAS_SWISH, (70, 72, 24), nz=(2, 2), geo={"C": {"stride_pad": 2}}, seed=77)
    assert res.report["store"] == g.ST_LDS and res.report["store_mixed"] == 1
    g.check_case(res)


# ---- d. batches ----
def test_batches_under_both_workgroup_mappings():
    _run_all((label, kw, {"zmajor": zm}) for label, kw, zm in g.batch_cases())


# ---- e. side outputs ----
@pytest.mark.parametrize("cfg", [g.CFG_BIG, g.CFG_MID, g.CFG_SMALL, g.CFG_SQ, g.CFG_SQ8, g.CFG_WG])
@pytest.mark.parametrize("N", [32, 96, 288])
def test_mask_words_and_the_dgrad_that_reads_them(cfg, N):
    M, nz = 70, (2, 2)
    fwd = g.mask_words_case(cfg, M, N, nz=nz, seed=N + cfg)
    assert fwd.report["mb"] == 1 and fwd.report["store"] == g.ST_LDS
    g.check_case(fwd)      # C itself to the float64 bar; guards of C and of the words
    act = fwd.arrays["C"].get()                    # [2][2][1][M][N] as stored
    words = fwd.arrays["mb_out"].get()
    assert np.array_equal(words, g.pack_mask(act > 0)), "mask words are not the packing of (stored C > 0)"
    assert 0.2 < (act > 0).mean() < 0.8
    # the masked dgrad through this activation: from the float matrix and from the words, bit for bit
    ref = g.masked_dgrad_case(cfg, act, None, nz=nz, seed=N)
    bits = g.masked_dgrad_case(cfg, act, words, nz=nz, seed=N)
    assert ref.report["aux_bits"] == 0 and bits.report["aux_bits"] == 1 and bits.report["store"] == g.ST_LDS
    g.check_case(ref)
    g.check_case(bits)
    assert np.array_equal(ref.arrays["C"].raw, bits.arrays["C"].raw)


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("cfg", [g.CFG_BIG, g.CFG_SQ])
def test_rank1_operand_from_mask_words(cfg, precision):
    """(70, 40, 64): a(m, k) = bit(m, k) ? rowv[m] colv[k] : 0 without an A matrix, against mode 3's formula; and bit for bit against
    the float-operand launch fed an A with the same signs"""
    res = g.rank1_bits_case(cfg, nz=(2, 3), precision=precision, seed=cfg)
    assert res.report["a_bits"] == 1 and res.report["la"] == g.L_VECK and res.report["lb"] == g.L_BLK4
    g.check_case(res)
    data = g.Result()
    data.d = {k: v for k, v in res.d.items() if k in ("B", "aux", "rowv", "colv")}
    data.d["A"] = np.where(res.d["pos"], 1.5, -0.5).astype(np.float32)
    flt = g.run_case(cfg, g.E_MASK, (70, 40, 64), layout=1, pa=1, nz=(2, 3), precision=precision, data=data, seed=cfg)
    assert (flt.report["la"], flt.report["lb"]) == (g.L_VECK, g.L_BLK4)
    g.check_case(flt)
    assert np.array_equal(flt.arrays["C"].get(), res.arrays["C"].get())


@pytest.mark.parametrize("cfg", [g.CFG_BIG, g.CFG_SQ8])
def test_fused_single_output_tail(cfg):
    """N = 260 is two column tiles of 256 and three of 128: tile 0 writes tq_out (+ the tail bias), the others their partial sums"""
    res = g.fused_tail_case(cfg, nz=(2, 2), seed=cfg)
    assert res.report["tq_parts"] == res.parts == {g.CFG_BIG: 2, g.CFG_SQ8: 3}[cfg] and res.report["store"] == g.ST_LDS
    g.check_case(res)
    for (z0, z1) in res.ref_c:
        q = res.arrays["tq_out"].get()[z0, z1, 0, :, 0].astype(np.float64) + res.arrays["tq_part"].get()[z0, z1, 0].astype(np.float64).sum(0)
        ref = g.tail_q(res.d["A"][z0, z1, 0], res.d["B"][z0, z1, 0], res.d["bias"][z0, z1, 0, 0], res.tq_w[z0, z1, 0, 0], res.tq_b[z0, z1, 0, 0, 0])
        assert g.rel_err(q, ref) < 2e-5, (z0, z1, g.rel_err(q, ref))


@pytest.mark.parametrize("words", [False, True])
@pytest.mark.parametrize("cfg,nz,in0", [(g.CFG_BIG, (1, 2), 23), (g.CFG_BIG, (1, 1), 11), (g.CFG_SQ, (10, 2), 11)])
def test_fused_layer0_gradient(cfg, nz, in0, words):
    """M = 2051 is what pick_cfg sends to CFG_BIG (few problems) or CFG_SQ (M nz >= 40000); one slab per row tile, summed here"""
    with_c = g.fused_w0_case(cfg, nz, in0, True, words, seed=in0)
    no_c = g.fused_w0_case(cfg, nz, in0, False, words, seed=in0)
    for r in (with_c, no_c):
        assert r.report["w0_slabs"] == r.slabs == (2051 + g.TILES[cfg][0] - 1) // g.TILES[cfg][0] and r.report["aux_bits"] == int(words)
    g.check_case(with_c)
    g.check_guards(no_c)
    assert np.all(no_c.arrays["C"].raw == np.uint32(0xDEADBEEF)), "C was written although it was not asked for"
    for a in ("w0_out", "w0_bias"):
        assert np.array_equal(with_c.arrays[a].raw, no_c.arrays[a].raw)      # the gradient does not depend on whether C is stored
    for (z0, z1), dz0 in with_c.ref_c.items():
        assert np.array_equal(with_c.arrays["C"].get()[z0, z1, 0] != 0, (dz0 != 0))
        dw, db = g.w0_grad(dz0, with_c.x[z0, z1, 0])
        got_w = with_c.arrays["w0_out"].get()[z0, z1].astype(np.float64).sum(0)
        got_b = with_c.arrays["w0_bias"].get()[z0, z1].astype(np.float64).sum(0)[0]
        assert g.rel_err(got_w, dw) < 2e-5 and g.rel_err(got_b, db) < 2e-5, (g.rel_err(got_w, dw), g.rel_err(got_b, db))


def test_fused_layer0_gradient_c_identical_with_words_and_without():
    a = g.fused_w0_case(g.CFG_BIG, (1, 1), 23, True, False, seed=3)
    b = g.fused_w0_case(g.CFG_BIG, (1, 1), 23, True, True, seed=3)
    assert np.array_equal(a.arrays["C"].raw, b.arrays["C"].raw) and np.array_equal(a.arrays["w0_out"].raw, b.arrays["w0_out"].raw)


@pytest.mark.parametrize("pa", [0, 1])
@pytest.mark.parametrize("cfg", [g.CFG_MID, g.CFG_SQ, g.CFG_SQ8])
def test_transposed_weight_gradient_store(cfg, pa):
    """(in, out)-major weight gradients: whole m-runs through LDS at M % 4 == 0, the scalar fall-back otherwise; both equal the row-major result transposed"""
    for shape, path in [((64, 64, 100), g.ST_TRANS), ((132, 72, 100), g.ST_TRANS), ((62, 64, 100), g.ST_SCALAR)]:
        tr = g.transposed_case(cfg, shape, True, pa=pa, seed=shape[0])
        rm = g.transposed_case(cfg, shape, False, pa=pa, seed=shape[0])
        assert tr.report["store"] == path and rm.report["store"] == g.ST_LDS, (tr.report, rm.report)
        g.check_case(tr)
        g.check_case(rm)
        assert np.array_equal(tr.arrays["C"].get()[0, 0].transpose(0, 2, 1), rm.arrays["C"].get()[0, 0])
        assert np.array_equal(tr.arrays["bias_out"].get(), rm.arrays["bias_out"].get())
