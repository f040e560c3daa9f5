"""Float64 references of everything the tiled GEMM template (csrc/gemm_kernel.h) computes, and the case runner the kernel-path tests
(tests/test_gpu_gemm_paths.py on the GPU, tests/test_gemm_paths_cpu.py without one) share.  The references are plain numpy in float64;
test_gemm_paths_cpu.py checks them against torch's float64 autograd so that a wrong reference cannot certify a wrong kernel."""
import numpy as np

E_PLAIN, E_BIAS, E_BIAS_RELU, E_MASK, E_WGRAD, E_BIAS_SWISH, E_SWISH_GRAD, E_BIAS_LEAKY, E_LEAKY_MASK = range(9)
CFG_BIG, CFG_MID, CFG_SMALL, CFG_TALL, CFG_SQ, CFG_SQ8, CFG_WG = range(7)
TILES = {CFG_BIG: (64, 256, 32), CFG_MID: (64, 64, 32), CFG_SMALL: (16, 64, 64), CFG_TALL: (64, 16, 32), CFG_SQ: (128, 128, 32),
         CFG_SQ8: (128, 128, 32), CFG_WG: (256, 128, 32)}      # (TM, TN, TK) of csrc/gemm.h
L_SCALAR, L_VECK, L_BLK4, L_VECKU = range(4)
ST_LDS, ST_VEC, ST_SCALAR, ST_TRANS = range(4)
LEAKY_SLOPE = 0.01
BIAS_EPIS = (E_BIAS, E_BIAS_RELU, E_BIAS_SWISH, E_BIAS_LEAKY)
AUX_EPIS = (E_MASK, E_SWISH_GRAD, E_LEAKY_MASK)
TOL = {0: 2e-5, 1: 2e-4, 2: 2e-5}      # the bars of tests/test_gpu_gemm.py per precision


# ---- references (float64) ----
def sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    return 1.0 / (1.0 + np.exp(-z))


def swish(z):
    z = np.asarray(z, dtype=np.float64)
    return z * sigmoid(z)


def dswish(z):
    """d/dz z sigmoid(z) = s (1 + z (1 - s))"""
    z = np.asarray(z, dtype=np.float64)
    s = sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


def leaky(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(v > 0, v, LEAKY_SLOPE * v)


def leaky_factor(h):
    """LeakyReLU' read off the stored activation: 1 where h > 0, the slope elsewhere -- zero (either sign) takes the slope"""
    return np.where(np.asarray(h) > 0, 1.0, LEAKY_SLOPE)


def pack_mask(pos):
    """[..., N] booleans -> [..., ceil(N / 32)] uint32 words: bit b of word w <-> column 32 w + b"""
    pos = np.asarray(pos, dtype=bool)
    n = pos.shape[-1]
    g = (n + 31) // 32
    padded = np.zeros(pos.shape[:-1] + (g * 32,), dtype=np.uint64)
    padded[..., :n] = pos
    w = (padded.reshape(pos.shape[:-1] + (g, 32)) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32)


def unpack_mask(words, n):
    words = np.asarray(words, dtype=np.uint32)
    bits = (words[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(words.shape[:-1] + (-1,))[..., :n].astype(bool)


def tail_q(x, w, b, w_tail, b_tail):
    """single-output tail behind a ReLU layer: relu(x w^T + b) . w_tail + b_tail"""
    h = np.maximum(np.asarray(x, np.float64) @ np.asarray(w, np.float64).T + np.asarray(b, np.float64), 0)
    return h @ np.asarray(w_tail, np.float64) + float(b_tail)


def w0_grad(dz0, x):
    """layer-0 weight / bias gradient from the masked gradient dz0 [M][N] and the input rows x [M][in]"""
    dz0, x = np.asarray(dz0, np.float64), np.asarray(x, np.float64)
    return dz0.T @ x, dz0.sum(0)


def product(layout, a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a @ b.T if layout == 0 else (a @ b if layout == 1 else a.T @ b)


def rank1(pos, rowv, colv):
    """the virtual operand pos ? rowv[r] * colv[c] : 0, multiplied in float32 as the loaders do"""
    return np.where(pos, np.outer(np.float32(rowv), np.float32(colv)).astype(np.float32), np.float32(0)).astype(np.float64)


def epilogue(epi, acc, bias=None, aux=None):
    """(C, z) of one problem: z = the Swish pre-activation (E_BIAS_SWISH only)"""
    if epi in BIAS_EPIS:
        acc = acc + np.asarray(bias, np.float64)
    if epi == E_BIAS_RELU:
        return np.maximum(acc, 0), None
    if epi == E_MASK:
        return acc * (np.asarray(aux) > 0), None
    if epi == E_BIAS_SWISH:
        return swish(acc), acc
    if epi == E_SWISH_GRAD:
        return acc * dswish(aux), None
    if epi == E_BIAS_LEAKY:
        return leaky(acc), None
    if epi == E_LEAKY_MASK:
        return acc * leaky_factor(aux), None
    return acc, None


def rel_err(got, ref):
    """the error measure of tests/test_gpu_gemm.py: max abs error over max |ref|"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-6))


# ---- one launch of the wide tap ----
class Result:
    pass


def result_guard(rows, pitch):
    """guard rows behind a result of `rows` rows: up to the end of the tallest tile (256 rows) and at least 256 elements, so that a
    store which lost its row or column guard lands in words the test looks at"""
    return max((-rows) % 256 + 2, (256 + pitch - 1) // pitch + 1)


def default_layout(epi):
    return 2 if epi == E_WGRAD else (1 if epi in AUX_EPIS else 0)


def run_case(cfg, epi, shape, layout=None, pa=0, precision=0, nz=(1, 1), ksplit=1, seed=0, geo=None, a_kpad=False, c_trans=False,
             zeros=False, bias_out=True, extra=None, ints=None, data=None, dry_run=False):
    """Builds random per-problem data (standard normal), lays every array out with guards (``geo``: array name -> GemmArray keyword
    overrides, ``pad`` = extra pitch), launches the tap and returns the arrays, the float64 references per problem and the report.
    ``zeros`` plants exact +0.0 / -0.0 in aux.  ``extra``: callable(res, arrays, ints) adding side-output arrays before the launch.
    ``data``: reuse the operands of an earlier Result."""
    from offlinerlkit._engine import GemmArray, debug_gemm_ex, GEMM_PAD_NAN
    M, N, K = shape
    nz0, nz1 = nz
    layout = default_layout(epi) if layout is None else layout
    geo = geo or {}
    rng = np.random.RandomState(seed)
    res = Result()
    res.shape, res.nz, res.epi, res.layout, res.ksplit, res.precision, res.c_trans = shape, nz, epi, layout, ksplit, precision, c_trans

    def arr(name, rows, cols, result=False, nslab=1, dtype=np.float32):
        kw = dict(geo.get(name, {}))
        pad = kw.pop("pad", 0)
        if "pitch" not in kw:
            kw["pitch"] = cols + pad
        if not result:
            kw.setdefault("fill", GEMM_PAD_NAN)
        else:
            kw.setdefault("guard", result_guard(rows, kw["pitch"]))
        return GemmArray(rows, cols, nz0, nz1, nslab, dtype=dtype, **kw)

    def rnd(a):
        return rng.standard_normal(a.idx.shape).astype(np.float32)

    arrays = {}
    a_shape = (K, M) if layout == 2 else (M, K)
    b_shape = (N, K) if layout == 0 else (K, N)
    if a_kpad:
        g = dict(geo.get("A", {}))
        g.setdefault("pitch", ((K + 3) & ~3) + g.pop("pad", 0))
        geo = dict(geo, A=g)
    d = data.d if data is not None else {}
    res.d = d
    if pa != 2:
        arrays["A"] = arr("A", *a_shape)
        d.setdefault("A", rnd(arrays["A"]))
    arrays["B"] = arr("B", *b_shape)
    d.setdefault("B", rnd(arrays["B"]))
    if epi in BIAS_EPIS:
        arrays["bias"] = arr("bias", 1, N)
        d.setdefault("bias", rnd(arrays["bias"]))
    if epi in AUX_EPIS:
        arrays["aux"] = arr("aux", M, N)
        if "aux" not in d:
            aux = rnd(arrays["aux"])
            if zeros:      # exact zeros of both signs among both signs of ordinary values
                flat = aux.reshape(-1)
                flat[0::5] = 0.0
                flat[2::5] = -0.0
                assert np.signbit(flat[2::5]).all() and not np.signbit(flat[0::5]).any()
            d["aux"] = aux
    if pa:
        arrays["rowv"] = arr("rowv", 1, a_shape[0])
        arrays["colv"] = arr("colv", 1, a_shape[1])
        d.setdefault("rowv", rnd(arrays["rowv"]))
        d.setdefault("colv", rnd(arrays["colv"]))
    if pa == 2:
        arrays["a_bits"] = arr("a_bits", M, K // 32, dtype=np.uint32)
        if "pos" not in d:
            d["pos"] = rng.standard_normal(arrays["a_bits"].idx.shape[:3] + (M, K)) > 0
        d["a_bits"] = pack_mask(d["pos"])
    for k, a in arrays.items():
        a.put(d[k])
    c_rows, c_cols = (N, M) if c_trans else (M, N)
    arrays["C"] = arr("C", c_rows, c_cols, result=True, nslab=ksplit)
    if epi == E_BIAS_SWISH:
        arrays["z_out"] = arr("C", c_rows, c_cols, result=True, nslab=ksplit)
    if epi == E_WGRAD and bias_out:
        arrays["bias_out"] = arr("bias_out", 1, M, result=True, nslab=ksplit)
    kw = dict(cfg=cfg, layout=layout, epi=epi, pa=pa, precision=precision, M=M, N=N, K=K, nz0=nz0, nz1=nz1, ksplit=ksplit,
              a_kpad=int(a_kpad), c_trans=int(c_trans), dry_run=int(dry_run))
    kw.update(ints or {})
    res.arrays = arrays
    if extra is not None:
        extra(res, arrays, kw)
    res.report = debug_gemm_ex(arrays, **kw)

    # float64 references per problem
    res.ref_c, res.ref_z, res.ref_bo = {}, {}, {}
    for z0 in range(nz0):
        for z1 in range(nz1):
            def pick(name):
                v = d[name]
                return v[z0, z1 if v.shape[1] > 1 else 0, 0]
            if pa:
                pos = pick("pos") if pa == 2 else pick("A") > 0
                a_eff = rank1(pos, pick("rowv")[0], pick("colv")[0])
            else:
                a_eff = pick("A").astype(np.float64)
            acc = product(layout, a_eff, pick("B"))
            c, z = epilogue(epi, acc, pick("bias")[0] if epi in BIAS_EPIS else None, pick("aux") if epi in AUX_EPIS else None)
            res.ref_c[z0, z1], res.ref_z[z0, z1] = c, z
            if epi == E_WGRAD:
                res.ref_bo[z0, z1] = a_eff.sum(0)
    return res


def outputs(res):
    """(C, z_out, bias_out) per problem as float64, split-K slabs summed"""
    out = {}
    for key in res.ref_c:
        z0, z1 = key
        c = res.arrays["C"].get()[z0, z1].astype(np.float64).sum(0)
        if res.c_trans:
            c = c.T
        z = res.arrays["z_out"].get()[z0, z1, 0].astype(np.float64) if "z_out" in res.arrays else None
        bo = res.arrays["bias_out"].get()[z0, z1].astype(np.float64).sum(0)[0] if "bias_out" in res.arrays else None
        out[key] = (c, z, bo)
    return out


RESULT_ARRAYS = ("C", "z_out", "bias_out", "mb_out", "tq_out", "tq_part", "w0_out", "w0_bias")


def check_guards(res):
    """every word of every result array that is no logical element still holds the sentinel, bit for bit"""
    from offlinerlkit._engine import GEMM_SENTINEL
    for name in RESULT_ARRAYS:
        a = res.arrays.get(name)
        if a is not None:
            out = a.outside()
            bad = np.flatnonzero(out != np.uint32(GEMM_SENTINEL))
            assert bad.size == 0, f"{name}: {bad.size} words outside the logical result were written (first at outside-index {bad[:4]})"


def check_case(res, tol=None):
    """guards + every problem of the batch against its own float64 reference"""
    check_guards(res)
    tol = TOL[res.precision] if tol is None else tol
    for key, (c, z, bo) in outputs(res).items():
        e = rel_err(c, res.ref_c[key])
        assert e < tol, f"C of problem {key}: {e}"
        if z is not None:
            e = rel_err(z, res.ref_z[key])
            assert e < tol, f"z_out of problem {key}: {e}"
        if bo is not None:
            e = rel_err(bo, res.ref_bo[key])
            assert e < tol, f"bias_out of problem {key}: {e}"


# ---- the case lists (tests/test_gpu_gemm_paths.py runs them, tests/test_gemm_paths_cpu.py dry-runs them for coverage) ----
ALL_CFGS = list(range(7)) + [c | 16 for c in range(7)]
# (M, N, K): for every tile (TM, TN, TK) the list holds M in {1, TM - 1, TM + 1}, N in {1, N % 4 != 0, TN - 4, TN + 4} and
# K in {1, 3, TK - 1, TK + 1, 2 TK + 4}
SHAPES = [(1, 1, 1), (3, 4, 5), (17, 20, 31), (65, 68, 33), (129, 132, 65), (257, 130, 36), (127, 260, 96), (260, 36, 64),
          (15, 12, 3), (63, 60, 68), (255, 124, 63), (33, 252, 132), (16, 64, 128)]
SPLIT_SHAPES = [(65, 68, 33), (129, 132, 65), (257, 130, 36), (127, 260, 96)]
# the five modes of the old tap and the rest of the instantiated (prologue, epilogue) pairs
MODES = {
    "fwd_relu": dict(epi=E_BIAS_RELU, layout=0), "dgrad_mask": dict(epi=E_MASK, layout=1), "wgrad": dict(epi=E_WGRAD, layout=2),
    "rank1_dgrad": dict(epi=E_PLAIN, layout=1, pa=1), "rank1_wgrad": dict(epi=E_WGRAD, layout=2, pa=1),
    "plain": dict(epi=E_PLAIN, layout=1), "bias": dict(epi=E_BIAS, layout=0), "swish": dict(epi=E_BIAS_SWISH, layout=0),
    "swish_grad": dict(epi=E_SWISH_GRAD, layout=1), "leaky": dict(epi=E_BIAS_LEAKY, layout=0), "leaky_mask": dict(epi=E_LEAKY_MASK, layout=1),
    "rank1_mask": dict(epi=E_MASK, layout=1, pa=1),
}


def tile_cases(cfg, mode, shapes=SHAPES, precision=0):
    """part a: one tile shape, one mode, every shape of the list at the tight pitches of the old tap (wgrad: ksplit 1, 3 and one beyond the K chunks)"""
    for si, shape in enumerate(shapes):
        splits = (1, 3) if MODES[mode]["epi"] == E_WGRAD else (1,)
        if MODES[mode]["epi"] == E_WGRAD and shape == (65, 68, 33):
            splits = (1, 3, 8)      # 33 k: two chunks (one on the 64-deep tile), eight slabs
        for ks in splits:
            yield dict(cfg=cfg, shape=shape, ksplit=ks, precision=precision, seed=1000 * list(MODES).index(mode) + 10 * si + ks, **MODES[mode])


# part c: (name, N, geometry, store path it must take, epilogues it applies to)
STORE_VARIANTS = [
    ("lds", 72, {"C": {"pad": 4}, "aux": {"pad": 8}}, ST_LDS, None),
    ("vec", 70, {"C": {"pad": 2}, "aux": {"pad": 6}}, ST_VEC, None),
    ("scalar_base", 72, {"C": {"off": 1}}, ST_SCALAR, None),
    ("scalar_pitch", 72, {"C": {"pad": 1}}, ST_SCALAR, None),
    ("scalar_aux_base", 72, {"aux": {"off": 3}}, ST_SCALAR, AUX_EPIS),
    ("scalar_aux_pitch", 72, {"aux": {"pad": 2}}, ST_SCALAR, AUX_EPIS),
    ("scalar_bias_base", 72, {"bias": {"off": 2}}, ST_SCALAR, BIAS_EPIS),
]
STORE_CFGS = (CFG_SMALL, CFG_MID, CFG_SQ8)


def store_cases():
    for cfg in STORE_CFGS:
        for epi in range(9):
            for name, n, geo, path, epis in STORE_VARIANTS:
                if epis is not None and epi not in epis:
                    continue
                kw = dict(cfg=cfg, epi=epi, shape=(70, n, 23), geo=geo, zeros=True, seed=7000 + 10 * epi + cfg)
                if epi == E_WGRAD:
                    kw.update(shape=(70, n, 150), ksplit=2)
                yield f"{name}-epi{epi}-cfg{cfg}", kw, path


# loader pairs: (name, kwargs, (la_pick, lb_pick), (la, lb))
def loader_cases():
    V, B4, VU, S = L_VECK, L_BLK4, L_VECKU, L_SCALAR
    base = [
        ("veck_veck", dict(epi=E_BIAS_SWISH, shape=(70, 72, 24)), (V, V), (V, V)),
        ("veck_veck_padded", dict(epi=E_BIAS_LEAKY, shape=(70, 72, 24), geo={"A": {"pad": 4}, "B": {"pad": 8}}), (V, V), (V, V)),
        ("kpad_vecku", dict(epi=E_BIAS_RELU, shape=(70, 72, 23), a_kpad=True), (V, VU), (V, VU)),
        ("kpad_wide_vecku", dict(epi=E_BIAS, shape=(70, 72, 21), a_kpad=True, geo={"A": {"pad": 4}, "B": {"pad": 2}}), (V, VU), (V, VU)),
        ("kpad_veck_b_base", dict(epi=E_BIAS, shape=(70, 72, 24), a_kpad=True, geo={"B": {"off": 1}}), (V, VU), (V, VU)),
        ("vecku_on_a", dict(epi=E_BIAS, shape=(70, 72, 23)), (VU, VU), (S, S)),
        ("veck_blk4", dict(epi=E_MASK, shape=(70, 72, 24)), (V, B4), (V, B4)),
        ("veck_blk4_padded", dict(epi=E_SWISH_GRAD, shape=(70, 70, 24), geo={"B": {"pad": 2}, "C": {"pad": 2}, "aux": {"pad": 2}}), (V, B4), (V, B4)),
        ("veck_scalar", dict(epi=E_LEAKY_MASK, shape=(70, 72, 24), geo={"B": {"off": 1}}), (V, S), (V, S)),
        ("veck_scalar_pitch", dict(epi=E_PLAIN, layout=1, shape=(70, 70, 24)), (V, S), (V, S)),
        ("blk4_blk4", dict(epi=E_WGRAD, shape=(72, 40, 70), ksplit=2), (B4, B4), (B4, B4)),
        ("blk4_blk4_padded", dict(epi=E_WGRAD, shape=(70, 38, 70), geo={"A": {"pad": 2}, "B": {"pad": 6}}), (B4, B4), (B4, B4)),
        ("scalar_a_base", dict(epi=E_WGRAD, shape=(72, 40, 70), geo={"A": {"off": 2}}), (S, B4), (S, S)),
        ("scalar_scalar", dict(epi=E_WGRAD, shape=(70, 38, 70)), (S, S), (S, S)),
        ("rank1_veck_blk4", dict(epi=E_PLAIN, layout=1, pa=1, shape=(70, 72, 24)), (V, B4), (V, B4)),
        ("rank1_mask_veck_blk4", dict(epi=E_MASK, layout=1, pa=1, shape=(70, 72, 24)), (V, B4), (V, B4)),
        ("rank1_colv_base", dict(epi=E_PLAIN, layout=1, pa=1, shape=(70, 72, 24), geo={"colv": {"off": 1}}), (V, B4), (S, S)),
        ("rank1_blk4_blk4", dict(epi=E_WGRAD, pa=1, shape=(72, 40, 70), ksplit=2), (B4, B4), (B4, B4)),
        ("rank1_blk4_blk4_padded", dict(epi=E_WGRAD, pa=1, shape=(70, 38, 70), geo={"A": {"pad": 2}, "B": {"pad": 6}}), (B4, B4), (B4, B4)),
        ("rank1_wgrad_colv_base", dict(epi=E_WGRAD, pa=1, shape=(72, 40, 70), geo={"colv": {"off": 1}}), (B4, B4), (S, S)),
    ]
    for cfg, prec in [(c, 0) for c in range(7)] + [(CFG_SMALL, 1), (CFG_SQ, 1), (CFG_SMALL, 2), (CFG_WG, 2)]:
        for i, (name, kw, pick, pair) in enumerate(base):
            yield f"{name}-cfg{cfg}-p{prec}", dict(kw, cfg=cfg, precision=prec, seed=8000 + 20 * cfg + i), pick, pair


BATCHES = [(1, 2), (3, 2), (9, 1), (11, 1), (8, 2)]


def batch_cases():
    """part d: every problem has its own data; the z strides of the arrays differ from each other (run-major and member-major
    interleavings, one A shared by the members of a run)"""
    for nz in BATCHES:
        many = nz[0] * nz[1] >= 8
        for M in (70, 13):      # five 16 x 64 tiles; one tile
            tiles = (M + 15) // 16
            yield (f"fwd-{nz}-M{M}", dict(cfg=CFG_SMALL, epi=E_BIAS_RELU, shape=(M, 40, 23), nz=nz, a_kpad=True, seed=9000 + M + nz[0],
                                          geo={"A": {"share_z1": True}, "C": {"z1_major": True, "pad": 4}, "bias": {"z1_major": True}}),
                   int(many and tiles > 1))
            yield (f"swish-{nz}-M{M}", dict(cfg=CFG_SMALL, epi=E_BIAS_SWISH, shape=(M, 40, 24), nz=nz, seed=9100 + M + nz[0],
                                            geo={"B": {"z1_major": True}, "C": {"z1_major": True}}), int(many and tiles > 1))
            yield (f"dgrad-{nz}-M{M}", dict(cfg=CFG_SMALL, epi=E_MASK, shape=(M, 40, 23), nz=nz, seed=9200 + M + nz[0],
                                            geo={"A": {"z1_major": True}, "aux": {"z1_major": True}, "C": {"stride_pad": 4}}),
                   int(many and tiles > 1))
            for K in (23, 150):      # one K chunk (slabs 1 and 2 hold zeros); three chunks
                yield (f"wgrad-ks3-{nz}-M{M}-K{K}", dict(cfg=CFG_SMALL, epi=E_WGRAD, shape=(M, 40, K), nz=nz, ksplit=3, seed=9300 + M + nz[0] + K,
                                                         geo={"A": {"z1_major": True}, "C": {"z1_major": True}, "bias_out": {"stride_pad": 4}}),
                       int(many))      # 3 or 15 work items per problem
        yield (f"rank1-wgrad-{nz}", dict(cfg=CFG_MID, epi=E_WGRAD, pa=1, shape=(72, 40, 70), nz=nz, ksplit=2, seed=9400 + nz[0],
                                         geo={"rowv": {"z1_major": True}, "C": {"z1_major": True}}), int(many))      # 2 tiles x 2 slabs


# ---- side outputs (part e) ----
def _ga(rows, cols, *a, **kw):
    from offlinerlkit._engine import GemmArray, GEMM_SENTINEL
    if kw.get("fill", GEMM_SENTINEL) == GEMM_SENTINEL:      # a result array
        kw.setdefault("guard", result_guard(rows, kw.get("pitch", cols)))
    return GemmArray(rows, cols, *a, **kw)


def mask_words_case(cfg, M, N, K=24, nz=(1, 1), precision=0, dry_run=False, seed=0):
    """E_BIAS_RELU emitting the packed mask of what it stores"""
    def extra(res, arrays, ints):
        arrays["mb_out"] = _ga(M, N // 32, nz[0], nz[1], pitch=N // 32 + 1, z1_major=True, dtype=np.uint32)
    return run_case(cfg, E_BIAS_RELU, (M, N, K), nz=nz, precision=precision, extra=extra, dry_run=dry_run, seed=seed, geo={"C": {"pad": 4}})


def masked_dgrad_case(cfg, act, words, dY=None, nz=(1, 1), K=24, dry_run=False, seed=0, data=None):
    """E_MASK over the activation `act` [nz0][nz1][1][M][N]: from the float matrix (words None) or from its packed words"""
    M, N = act.shape[-2:]

    def extra(res, arrays, ints):
        if words is not None:
            from offlinerlkit._engine import GEMM_PAD_NAN
            arrays["aux_bits"] = _ga(M, N // 32, nz[0], nz[1], pitch=N // 32 + 2, dtype=np.uint32, fill=0xFFFFFFFF).put(words)
            arrays["aux"].raw[:] = GEMM_PAD_NAN      # a launch that honours the words never looks at the float matrix
    d = Result()
    d.d = dict(data.d) if data is not None else {}
    d.d["aux"] = act
    return run_case(cfg, E_MASK, (M, N, K), nz=nz, extra=extra, dry_run=dry_run, seed=seed, data=d)


def rank1_bits_case(cfg, shape=(70, 40, 64), nz=(1, 1), precision=0, dry_run=False, seed=0):
    return run_case(cfg, E_MASK, shape, layout=1, pa=2, nz=nz, precision=precision, dry_run=dry_run, seed=seed,
                    geo={"a_bits": {"pad": 1, "z1_major": True}})


def fused_tail_case(cfg, M=70, N=260, K=24, nz=(1, 1), tq_sm=3, dry_run=False, seed=0):
    TN = TILES[cfg][1]
    parts = (N + TN - 1) // TN
    rng = np.random.RandomState(seed + 1)

    def extra(res, arrays, ints):
        from offlinerlkit._engine import GEMM_PAD_NAN
        res.tq_w = rng.standard_normal((nz[0], nz[1], 1, 1, N)).astype(np.float32)
        res.tq_b = rng.standard_normal((nz[0], nz[1], 1, 1, 1)).astype(np.float32)
        arrays["tq_w"] = _ga(1, N, nz[0], nz[1], fill=GEMM_PAD_NAN).put(res.tq_w)
        arrays["tq_b"] = _ga(1, 1, nz[0], nz[1], z1_major=True, fill=GEMM_PAD_NAN).put(res.tq_b)
        arrays["tq_out"] = _ga(M, 1, nz[0], nz[1], pitch=tq_sm)
        arrays["tq_part"] = _ga(max(parts - 1, 1), M, nz[0], nz[1], pitch=M + 2, z1_major=True)
        ints["tq_sm"] = tq_sm
    res = run_case(cfg, E_BIAS_RELU, (M, N, K), nz=nz, extra=extra, dry_run=dry_run, seed=seed)
    res.parts = parts
    return res


def fused_w0_case(cfg, nz, in0, store_c, words=False, M=2051, N=132, K=40, dry_run=False, seed=0):
    """E_MASK dgrad of hidden layer 1 that also leaves the layer-0 weight / bias gradient, one slab per row tile"""
    slabs = (M + TILES[cfg][0] - 1) // TILES[cfg][0]
    xp = (in0 + 4) & ~3
    rng = np.random.RandomState(seed + 1)

    def extra(res, arrays, ints):
        from offlinerlkit._engine import GEMM_PAD_NAN
        res.x = rng.standard_normal((nz[0], nz[1], 1, M, in0)).astype(np.float32)
        arrays["w0_x"] = _ga(M, in0, nz[0], nz[1], pitch=xp, guard=0, fill=GEMM_PAD_NAN).put(res.x)
        arrays["w0_out"] = _ga(N, in0, nz[0], nz[1], nslab=slabs, pitch=in0 + 1)
        arrays["w0_bias"] = _ga(1, N, nz[0], nz[1], nslab=slabs, guard=2, kstride=arrays["w0_out"].kstride)
        if words:
            arrays["aux_bits"] = _ga(M, (N + 31) // 32, nz[0], nz[1], dtype=np.uint32, fill=0).put(pack_mask(res.d["aux"] > 0))
        ints.update(w0_in=in0, c_null=int(not store_c))
    res = run_case(cfg, E_MASK, (M, N, K), nz=nz, extra=extra, dry_run=dry_run, seed=seed)
    res.slabs = slabs
    return res


def transposed_case(cfg, shape, trans=True, ksplit=2, pa=0, dry_run=False, seed=0, data=None):
    return run_case(cfg, E_WGRAD, shape, pa=pa, ksplit=ksplit, c_trans=trans, dry_run=dry_run, seed=seed, data=data, geo={"C": {"pad": 4}})
