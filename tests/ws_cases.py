"""Float64 references of what the weight-stationary kernels (csrc/ws_*.hip; formulas: csrc/ws_gemm.h) compute, the case lists and the
case runner that tests/test_gpu_ws_paths.py (GPU) and tests/test_ws_paths_cpu.py (no device) share.  Every launch goes through the
unit tap orl_debug_ws (offlinerlkit._engine.debug_ws); a case is a dict of keyword arguments of ``build``.

Bars are componentwise: |got - f64| <= C * (the same expression with every term replaced by its absolute value), C = bound(precision)
of tests/test_gpu_backward_f64.py.  A launch is one stage on its own inputs; a launch that hands h0 from the first to the second layer
without returning it (x0_discard, recompute) is two stages and gets 2 C.  Mask words are compared bit by bit with z_f64 > 0; a differing
bit must sit on |z_f64| <= C * abs-sum(z) and at most FLIP_SHARE of a problem's bits may differ; downstream references use the kernel's
own masks.  Operands are O(1): standard normal rows, weights U(+-1/16), dq ~ N(0, 1) / M.

Measured on an MI355X (fp16 hi + lo planes build) over every case of tests/test_gpu_ws_paths.py, worst |got - f64| / (C * abs-sum) per
stage = (launcher, precision 0 exact fp32 / 1 two planes / 2 three planes, case family):
  within C:   fwd p0 0.18, fwd p1 0.54, dgrad p0 0.14, dgrad p1 0.20, dgrad3 p2 0.40, wgrad p0 0.22 (families "in0 3" of dgrad / wgrad: < 0.23)
  above C:    wgrad p1 base 8.47 (ws_wgrad<2>, M = 256, per_z = 8), wgrad p2 base 16.94 (ws_wgrad<5>, the same case), wgrad3p p2 base 4.25,
              fwd3 p2 base 1.08 (ws_fwd3<0,1,0,0,1>, the plain dgrad mode), fwd p1 "in0 3" 1.98, fwd3 p2 "in0 3" 3.95,
              gscale = 2^-6: fwd p1 29.96, fwd3 p2 59.92, dgrad p1 4.63, dgrad3 p2 9.25, wgrad p1 89.99, wgrad p2 179.98, wgrad3p p2 106.31
None of these is a structural error: the exact-fp32 kernels of the same launchers pass the same cases, depths and slabs at 0.22 C, every
slab holds exactly its own rows, and with gscale = 2^9 the split kernels pass at C.  The excess is the absolute floor of the fp16 planes:
dq ~ N(0, 1) / M makes G = dq (.) h0 ~ 4e-3, whose lo plane (2^-11 of it) lies in fp16's subnormal range (step 6e-8), so a term carries
an absolute error of ~3e-8 whatever its size; a third plane adds nothing below that floor (p2 = exactly twice p1: the same error over
half the constant); gscale = 2^-6 pushes the hi plane there too; with in0 = 3 a pre-activation has four terms and a weight near zero
(U(+-1/16)) loses its lo plane.  The bar of these stages is BARS[stage] * C with BARS = twice the worst measured ratio (the factor two
allows for the order of the fp32 adds); the largest, 360 C = 7e-4 of the absolute sum, is still three orders of magnitude below what a dropped row group,
a swapped buffer or a missing bias leaves (tests/test_ws_paths_cpu.py plants such defects)."""
import numpy as np

from offlinerlkit import _engine
from offlinerlkit._engine import GEMM_PAD_NAN, GEMM_SENTINEL, OrlGemmBuf
from test_gpu_backward_f64 import bound

N = 256                      # K = N = 256 is fixed by the kernels
FLIP_SHARE = 2e-4            # share of a problem's mask bits that may differ from float64 (tests/test_gpu_grads.py)
DEPTHS = [(256, 8), (256, 4), (288, 3), (256, 2), (352, 2), (256, 5), (352, 3), (256, 1)]      # (M, per_z): 1, 2, 3, 4, 6|5, 2|1, 4|4|3, 8 groups per workgroup
MEASURED = {}                # stage -> worst |got - f64| / (C * abs-sum) seen by this process
# Stages whose kernels are structurally right (their exact-fp32 siblings pass the same cases at C, every slab holds exactly its rows)
# but exceed C in this operand domain: bar = BARS[stage] * C, BARS = twice the worst measured ratio (see the module docstring).
BARS = {"wgrad p1 base": 17.0, "wgrad p2 base": 34.0, "wgrad3p p2 base": 8.6, "fwd3 p2 base": 2.2, "fwd p1 in0 3": 4.0, "fwd3 p2 in0 3": 8.0,
        "fwd p1 gscale down": 60.0, "fwd3 p2 gscale down": 120.0, "dgrad p1 gscale down": 9.3, "dgrad3 p2 gscale down": 18.6,
        "wgrad p1 gscale down": 180.0, "wgrad p2 gscale down": 360.0, "wgrad3p p2 gscale down": 213.0}


def stage_of(kind, prec, family):
    return f"{kind} p{prec} {family}"


def precision_of(kind, f32=0, np3=0):
    """0 exact fp32, 1 two 16-bit planes, 2 three fp16 planes"""
    if kind in ("fwd3", "dgrad3", "wgrad3p") or np3:
        return 2
    return 0 if f32 else 1


# ---- the per-slab row rule ----
def slab_rows(M, per_z, slab):
    """rows a workgroup (= split-K slab) owns: the 32-row groups g = slab, slab + per_z, ..."""
    g = np.arange(M // 32)
    return (np.repeat(g % per_z == slab, 32)).nonzero()[0]


def groups_per_workgroup(M, per_z):
    return [len(range(s, M // 32, per_z)) for s in range(per_z)]


# ---- references (float64); every function is linear in its non-mask operands, so f(|args|) is its absolute-value twin ----
def f64(a):
    return np.asarray(a, dtype=np.float64)


def ref_layer(x, w, b):
    """z = x w^T + b, w (out, in)"""
    return f64(x) @ f64(w).T + f64(b)


def ref_tail(h, tw, tb):
    return f64(h) @ f64(tw) + float(np.asarray(tb).reshape(-1)[0])


def ref_dz0(ab, xb, dq, wt, w1):
    """dz0[m][n] = xb[m][n] dq[m] sum_k ab[m][k] wt[k] W1[k][n], W1 (k = output unit, n = input unit)"""
    return f64(xb) * f64(dq)[:, None] * ((f64(ab) * f64(wt)) @ f64(w1))


def ref_dz0_plain(xb, z, w1):
    return f64(xb) * (f64(z) @ f64(w1))


def ref_w0(dz0, x, rows):
    """dW0[n][c] = sum_m dz0[m][n] x[m][c], db0[n] = sum_m dz0[m][n] over `rows`"""
    d = f64(dz0)[rows]
    return d.T @ f64(x)[rows], d.sum(0)


def ref_wgrad(ab, dq, h0, wt, rows):
    """G[k][n] = sum_m ab[m][k] dq[m] h0[m][n], g[k] = sum_m ab[m][k] dq[m];  dW1 = wt (.) G, db1 = wt (.) g"""
    a = (f64(ab) * f64(dq)[:, None])[rows]
    G, g = a.T @ f64(h0)[rows], a.sum(0)
    return f64(wt)[:, None] * G, f64(wt) * g, G, g


def ref_tails(dq, h1, rows):
    return f64(dq)[rows] @ f64(h1)[rows], f64(dq)[rows].sum()


def ref_derived(G, g, w1, b1):
    """dw_tail[n] = sum_k W1[n][k] G[n][k] + b1[n] g[n], W1 (out, in)"""
    return (f64(w1) * G).sum(1) + f64(b1) * g


def ref_wgrad_plain(dz, h0, rows):
    return f64(dz)[rows].T @ f64(h0)[rows], f64(dz)[rows].sum(0)


def pack_mask(pos):
    pos = np.asarray(pos, dtype=bool)
    w = (pos.reshape(pos.shape[:-1] + (-1, 32)).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32)


def unpack_mask(words):
    words = np.asarray(words, dtype=np.uint32)
    bits = (words[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(words.shape[:-1] + (-1,)).astype(bool)


# ---- arrays ----
class Arr:
    """One array of the tap: logical [nz0][nz1][nslab][rows][cols] at off + z0 s0 + z1 s1 + ks kstride + r pitch + c in a flat 32-bit
    buffer; ``guard`` rows behind every slab, a pitch that may exceed cols, a guard band at the end.  ``wide``: s1 exceeds the problem
    and s0 is no multiple of s1.  Results are pre-filled with the sentinel, operands with a quiet NaN."""

    def __init__(self, rows, cols, nz0, nz1, nslab=1, pitch=None, off=0, guard=2, wide=False, result=False, dtype=np.float32, kstride=None, s0=None):
        self.dtype, self.result = np.dtype(dtype), result
        self.pitch, self.off = int(cols if pitch is None else pitch), int(off)
        self.kstride = int(kstride) if kstride is not None else (((rows + guard) * self.pitch + 3) & ~3)
        assert self.kstride >= (rows - 1) * self.pitch + cols
        prob = nslab * self.kstride
        self.s1 = prob + (40 if wide else 0)
        self.s0 = int(s0) if s0 is not None else nz1 * self.s1 + (20 if wide else 0)
        assert self.s0 >= nz1 * self.s1 and (not wide or nz1 < 2 or self.s0 % self.s1)
        self.n = self.off + nz0 * self.s0 + 4
        ix = np.ix_(*[np.arange(k, dtype=np.int64) for k in (nz0, nz1, nslab, rows, cols)])
        self.idx = self.off + ix[0] * self.s0 + ix[1] * self.s1 + ix[2] * self.kstride + ix[3] * self.pitch + ix[4]
        assert self.idx.max() < self.n
        self.fill = GEMM_SENTINEL if result else GEMM_PAD_NAN
        self.raw = np.full(self.n, self.fill, dtype=np.uint32)

    def put(self, data):
        self.raw.view(self.dtype)[self.idx] = np.asarray(data, dtype=self.dtype).reshape(self.idx.shape)
        return self

    def get(self):
        return self.raw.view(self.dtype)[self.idx]

    def outside(self):
        keep = np.ones(self.n, dtype=bool)
        keep[self.idx.ravel()] = False
        return self.raw[keep]

    def desc(self):
        return OrlGemmBuf(self.raw.ctypes.data, self.n, self.off, self.pitch, self.s0, self.s1, self.kstride)


class Case:
    pass


def h0_stored(flavour):
    """does this forward instantiation store h0 (template parameter XS)?"""
    p = flavour[flavour.index("<") + 1:-1].split(",")
    return (p[5] if flavour.startswith("ws_fwd<") else p[2]) == "1"


def _weights(rng, *shape):
    return ((rng.random_sample(shape) * 2 - 1) / 16).astype(np.float32)


def build(kind, M=256, per_z=2, nz0=2, nz1=1, f32=0, np3=0, seed=0, in0=23, x0_pitch=24, ens=False, slab_ens=False, pad=0, wide=False,
          tq_sm=1, dq_sm=1, gscale=None, l0=False, tq=False, sy=True, discard=False, dgm=False, w0=True, plain=False, tails=False,
          derived=False, recompute=False, off=None, short=None, ints=None, family="base"):
    """A launch: ``kind`` in _engine.WS_KINDS; l0 / tq / sy / discard / dgm pick the forward flavour, w0 (else the storing flavour) /
    plain the dgrad one, tails / derived / plain / recompute the wgrad one.  ens: EnsembleLinear weight layout; slab_ens: the dgrad
    slabs in that layout; pad: extra columns of every wide pitch; wide: see Arr; off / short: {array: base offset / elements missing at
    the end} (refusal tests); ints: overrides of the tap's integer fields."""
    c = Case()
    c.kind, c.M, c.per_z, c.nz0, c.nz1, c.in0 = kind, M, per_z, nz0, nz1, in0
    c.prec = precision_of(kind, f32, np3)
    c.stage = stage_of(kind, c.prec, family)
    c.C = bound(c.prec)
    c.bar = BARS.get(c.stage, 1.0)
    c.kw = dict(l0=l0, tq=tq, sy=sy, discard=discard, dgm=dgm, w0=w0, plain=plain, tails=tails, derived=derived, recompute=recompute, gscale=gscale)
    rng = np.random.RandomState(1000 + seed)
    Z = (nz0, nz1)
    fwd, dg = kind in ("fwd", "fwd3"), kind in ("dgrad", "dgrad3")
    A, d = {}, {}

    def arr(name, rows, cols, data=None, result=False, pitch=None, nslab=1, dtype=np.float32, **kw):
        a = Arr(rows, cols, nz0, nz1, nslab=nslab, pitch=pitch, off=(off or {}).get(name, 0), wide=wide, result=result, dtype=dtype, **kw)
        if data is not None:
            d[name] = np.asarray(data, dtype=dtype).reshape(nz0, nz1, rows, cols)
            a.put(d[name])
        A[name] = a
        return a

    def weight(name, out_dim, in_dim, transposed):
        """logical (out, in); nn.Linear stores it so, EnsembleLinear as (in, out).  Returns (stride of out, stride of in)."""
        w = _weights(rng, *Z, out_dim, in_dim)
        d[name] = w
        if transposed:
            A[name] = Arr(in_dim, out_dim, nz0, nz1, off=(off or {}).get(name, 0), wide=wide).put(np.swapaxes(w, -1, -2))
            return 1, out_dim
        A[name] = Arr(out_dim, in_dim, nz0, nz1, off=(off or {}).get(name, 0), wide=wide).put(w)
        return in_dim, 1

    def narrow(name):
        """[M][x0_pitch] input rows: every column of the pitch is read (column in0 is replaced by ones, later ones meet zero weights)"""
        x = rng.standard_normal(Z + (M, x0_pitch)).astype(np.float32)
        x[..., in0] = 7.0
        arr(name, M, x0_pitch, x)

    def bits(name, pos, result=False):
        if pos is not None:
            d[name + "_pos"] = pos
        return arr(name, M, 8, None if pos is None else pack_mask(pos), result=result, dtype=np.uint32)

    i = dict(M=M, nz0=nz0, nz1=nz1, per_z=per_z, f32=f32, np3=np3, in0=in0, tq_sm=tq_sm, dq_sm=dq_sm)
    P = N + pad
    if gscale is not None:
        g = Arr(1, nz0, 1, 1)
        g.put(np.full(nz0, gscale, np.float32))
        A["gscale"], d["gscale"] = g, gscale
    if fwd:
        i["w_sn"], i["w_sk"] = weight("W", N, N, ens)
        if dgm:
            arr("X", M, N, rng.standard_normal(Z + (M, N)) / M, pitch=P)
            bits("dmask", rng.random_sample(Z + (M, N)) < 0.5)
            arr("Y", M, N, result=True, pitch=P)
        else:
            arr("bias", 1, N, _weights(rng, *Z, 1, N))
            arr("mb", M, 8, result=True, pitch=8 + pad // 4, dtype=np.uint32)
            if l0:
                narrow("X0")
                i["w0_sn"], i["w0_sk"] = weight("W0", N, in0, ens)
                arr("b0", 1, N, _weights(rng, *Z, 1, N))
                bits("mb0", None, result=True)
                arr("X", M, N, result=True, pitch=P)      # h0, or untouched when it is discarded
                i["x0_discard"] = int(discard)
            else:
                arr("X", M, N, rng.standard_normal(Z + (M, N)), pitch=P)
            if sy:
                arr("Y", M, N, result=True, pitch=P)
            if tq:
                arr("tw", 1, N, _weights(rng, *Z, 1, N))
                arr("tb", 1, 1, _weights(rng, *Z, 1, 1))
                arr("tq", M, 1, result=True, pitch=tq_sm)
                if kind == "fwd3":
                    arr("tq2", M, 1, result=True)
    elif dg:
        # W1 (k = output unit, n = input unit) at W[n w_sn + k w_sk]: nn.Linear (out, in) gives w_sn = 1, w_sk = 256
        sk, sn = weight("W", N, N, ens)
        i["w_sn"], i["w_sk"] = sn, sk
        bits("xbits", rng.random_sample(Z + (M, N)) < 0.5)
        if plain:
            arr("Z", M, N, rng.standard_normal(Z + (M, N)) / M, pitch=P)
        else:
            bits("abits", rng.random_sample(Z + (M, N)) < 0.5)
            arr("dq", M, 1, rng.standard_normal(Z + (M, 1)) / M, pitch=dq_sm)
            arr("wt", 1, N, _weights(rng, *Z, 1, N))
        if w0:
            narrow("X")
            # a slab: dW0 element (unit n, input c) at n o_sr + c o_sc: nn.Linear (in0, 1), EnsembleLinear (1, 256)
            if slab_ens:
                i["o_sr"], i["o_sc"] = 1, N
                a = arr("w0_out", in0, N, result=True, nslab=per_z + 1)
            else:
                i["o_sr"], i["o_sc"] = in0 + pad // 4, 1
                a = arr("w0_out", N, in0, result=True, nslab=per_z + 1, pitch=in0 + pad // 4)
            arr("b0_out", 1, N, result=True, nslab=per_z + 1, kstride=a.kstride, s0=a.s0)
        else:
            arr("C", M, N, result=True, pitch=P)
    else:
        if plain or kind == "wgrad3p":
            arr("dZ", M, N, rng.standard_normal(Z + (M, N)) / M, pitch=P)
            if recompute:
                narrow("X0")
                i["w0_sn"], i["w0_sk"] = weight("W0", N, in0, ens)
                arr("b0", 1, N, _weights(rng, *Z, 1, N))
            else:
                arr("H0", M, N, rng.standard_normal(Z + (M, N)), pitch=P)
        else:
            h1 = np.maximum(rng.standard_normal(Z + (M, N)), 0).astype(np.float32)
            bits("abits", h1 > 0)      # the streamed-tails flavour reads the mask off h1 itself: keep both consistent
            arr("dq", M, 1, rng.standard_normal(Z + (M, 1)) / M, pitch=dq_sm)
            arr("H0", M, N, rng.standard_normal(Z + (M, N)), pitch=P)
            arr("wt", 1, N, _weights(rng, *Z, 1, N))
            if tails:
                arr("H1", M, N, h1, pitch=P)
            if derived or np3:
                arr("W1", N, N, _weights(rng, *Z, N, N))
                arr("b1", 1, N, _weights(rng, *Z, 1, N))
        a = arr("dW", N, N, result=True, nslab=per_z + 1)
        arr("db", 1, N, result=True, nslab=per_z + 1, kstride=a.kstride, s0=a.s0)
        if tails or derived or np3:
            arr("dwt", 1, N, result=True, nslab=per_z + 1, kstride=a.kstride, s0=a.s0)
            arr("dbt", 1, 1, result=True, nslab=per_z + 1, kstride=a.kstride, s0=a.s0)
    for name, cut in (short or {}).items():      # the array ends `cut` elements before its last logical element
        A[name].n = int(A[name].idx.max()) + 1 - cut
    i.update(ints or {})
    c.arrays, c.d, c.ints = A, d, i
    c.before = {k: a.raw.copy() for k, a in A.items()}
    return c


DEVICE_ERRORS = []      # a launch that failed on the device (not a refusal): nothing more is launched from this process


def run(c, dry_run=False):
    assert dry_run or not DEVICE_ERRORS, ("an earlier launch failed on the device; no further launches", DEVICE_ERRORS[0])
    try:
        c.report = _engine.debug_ws(c.kind, c.arrays, dry_run=int(dry_run), **c.ints)
    except RuntimeError as e:
        if "orl_debug_ws device:" in str(e) or "no HIP device" in str(e):
            DEVICE_ERRORS.append(str(e))
        raise
    return c.report


def set_data(c, name, data):
    """replaces the logical contents of an operand of a built case"""
    a = c.arrays[name]
    c.d[name] = np.asarray(data, dtype=a.dtype).reshape(c.d[name].shape)
    a.put(c.d[name])
    c.before[name] = a.raw.copy()


def emulate(c):
    """What a correct kernel leaves in the result arrays, computed in float32 numpy (no device): the CPU tests run ``check`` on it, so the
    checks themselves are tested -- they must pass on this and fail on a planted defect."""
    run(c, dry_run=True)
    A, d, M, in0, pz = c.arrays, c.d, c.M, c.in0, c.per_z
    f = lambda a: np.asarray(a, dtype=np.float32)
    c.z32 = {}

    def put(name, z, data, slab=None):
        a = A[name]
        idx = a.idx[z][0] if slab is None else a.idx[z][slab]
        a.raw.view(a.dtype)[idx] = np.asarray(data, dtype=a.dtype).reshape(idx.shape)

    for z in [(a, b) for a in range(c.nz0) for b in range(c.nz1)]:
        kw = c.kw
        if c.kind in ("fwd", "fwd3"):
            if kw["dgm"]:
                put("Y", z, d["dmask_pos"][z] * (f(d["X"][z]) @ f(d["W"][z]).T))
                continue
            if kw["l0"]:
                z0 = f(d["X0"][z][:, :in0]) @ f(d["W0"][z]).T + f(d["b0"][z])
                x = np.maximum(z0, 0)
                put("mb0", z, pack_mask(z0 > 0))
                if h0_stored(c.report["flavour"]):
                    put("X", z, x)
                c.z32["z0", z] = z0
            else:
                x = f(d["X"][z])
            z1 = x @ f(d["W"][z]).T + f(d["bias"][z])
            c.z32["z1", z] = z1
            y = np.maximum(z1, 0)
            put("mb", z, pack_mask(z1 > 0))
            if kw["sy"]:
                put("Y", z, y)
            if kw["tq"]:
                tw, tb = f(d["tw"][z][0]), f(d["tb"][z]).reshape(-1)[0]
                if c.kind == "fwd3":
                    put("tq", z, y[:, :128] @ tw[:128] + tb)
                    put("tq2", z, y[:, 128:] @ tw[128:])
                else:
                    put("tq", z, y @ tw + tb)
        elif c.kind in ("dgrad", "dgrad3"):
            w1, xb = f(d["W"][z]), f(d["xbits_pos"][z])
            if kw["plain"]:
                dz0 = xb * (f(d["Z"][z]) @ w1)
            else:
                dz0 = xb * f(d["dq"][z]) * ((f(d["abits_pos"][z]) * f(d["wt"][z][0])) @ w1)
            if not kw["w0"]:
                put("C", z, dz0)
                continue
            x1 = f(d["X"][z][:, :in0])
            for sl in range(pz):
                rows = slab_rows(M, pz, sl)
                g = dz0[rows].T @ x1[rows]
                put("w0_out", z, g.T if A["w0_out"].idx.shape[-1] == N else g, sl)
                put("b0_out", z, dz0[rows].sum(0), sl)
        else:
            plain = kw["plain"] or c.kind == "wgrad3p"
            h0 = np.maximum(f(d["X0"][z][:, :in0]) @ f(d["W0"][z]).T + f(d["b0"][z]), 0) if kw["recompute"] else f(d["H0"][z])
            for sl in range(pz):
                rows = slab_rows(M, pz, sl)
                if plain:
                    put("dW", z, f(d["dZ"][z])[rows].T @ h0[rows], sl)
                    put("db", z, f(d["dZ"][z])[rows].sum(0), sl)
                    continue
                dq, wt = f(d["dq"][z][:, 0]), f(d["wt"][z][0])
                a = (f(d["abits_pos"][z]) * dq[:, None])[rows]
                G, g = a.T @ h0[rows], a.sum(0)
                put("dW", z, wt[:, None] * G, sl)
                put("db", z, wt * g, sl)
                if kw["tails"]:
                    put("dwt", z, dq[rows] @ f(d["H1"][z])[rows], sl)
                    put("dbt", z, dq[rows].sum(), sl)
                elif "dwt" in A:
                    put("dwt", z, (f(d["W1"][z]) * G).sum(1) + f(d["b1"][z][0]) * g, sl)
                    put("dbt", z, dq[rows].sum(), sl)
    return c


# ---- checks ----
class Worst:
    """collects err / bound ratios; asserts at the end so that one run reports every figure"""

    def __init__(self):
        self.items = []

    def add(self, tag, got, ref, absref, C):
        err = np.abs(f64(got) - ref)
        ratio = float((err / (C * absref + 1e-300)).max()) if err.size else 0.0
        self.items.append((tag, ratio))

    def worst(self):
        return max((r for _, r in self.items), default=0.0)


def check_mask(tag, words, z, za, C, problems):
    """mask words against z_f64 > 0, per problem; returns the kernel's mask as booleans"""
    got = unpack_mask(words)
    flip = got != (z > 0)
    assert np.all(np.abs(z[flip]) <= C * za[flip]), (tag, "a mask bit differs from float64 where |z| exceeds the bar", float((np.abs(z[flip]) / (C * za[flip])).max()))
    share = flip.reshape(problems, -1).mean(1).max()
    assert share <= FLIP_SHARE, (tag, "share of mask bits that differ from float64", float(share))
    return got


def check_guards(c):
    """every word outside the logical results still holds the sentinel; operands come back bit-identical; slabs >= per_z are untouched"""
    written_x = c.kind in ("fwd", "fwd3") and c.kw["l0"]
    for name, a in c.arrays.items():
        if a.result:
            assert np.all(a.outside() == GEMM_SENTINEL), (name, "a word outside the logical result was written")
            if name in ("w0_out", "b0_out", "dW", "db", "dwt", "dbt"):
                extra = a.raw[a.idx[:, :, c.per_z:]]
                assert np.all(extra == GEMM_SENTINEL), (name, "a slab >= per_z was written")
        else:
            assert np.array_equal(a.raw, c.before[name]), (name, "an operand came back changed")
    if written_x and not h0_stored(c.report["flavour"]):
        assert np.all(c.arrays["X"].raw == GEMM_SENTINEL), "h0 was stored although x0_discard asked not to"


def check(c):
    """asserts the launch against float64 and the guard words; returns the Worst ratios"""
    check_guards(c)
    w = Worst()
    A, d, C, M, in0 = c.arrays, c.d, c.C, c.M, c.in0
    CM = c.bar * C      # the bar of the mask bits follows the stage's
    nzp = c.nz0 * c.nz1
    zz = [(a, b) for a in range(c.nz0) for b in range(c.nz1)]
    if c.kind in ("fwd", "fwd3"):
        kw = c.kw
        if kw["dgm"]:
            for z in zz:
                pos = d["dmask_pos"][z]
                ref, ra = pos * (f64(d["X"][z]) @ f64(d["W"][z]).T), pos * (np.abs(f64(d["X"][z])) @ np.abs(f64(d["W"][z])).T)
                w.add("Y", A["Y"].get()[z][0], ref, ra, C)
        else:
            stages = 1
            for z in zz:
                if kw["l0"]:
                    x0 = f64(d["X0"][z][:, :in0])
                    z0 = ref_layer(x0, d["W0"][z], d["b0"][z])
                    z0a = ref_layer(np.abs(x0), np.abs(d["W0"][z]), np.abs(d["b0"][z]))
                    m0 = check_mask("mb0", A["mb0"].get()[z][0], z0, z0a, CM, 1)
                    if h0_stored(c.report["flavour"]):
                        h0 = A["X"].get()[z][0]
                        w.add("h0", h0, m0 * z0, m0 * z0a, C)
                        assert np.array_equal(h0 > 0, m0), "mb0 disagrees with the stored h0"
                        x, xa = f64(h0), np.abs(f64(h0))
                    else:
                        x, xa, stages = m0 * z0, m0 * z0a, 2
                else:
                    x = f64(d["X"][z])
                    xa = np.abs(x)
                z1 = ref_layer(x, d["W"][z], d["bias"][z])
                z1a = ref_layer(xa, np.abs(d["W"][z]), np.abs(d["bias"][z]))
                m1 = check_mask("mb", A["mb"].get()[z][0], z1, z1a, stages * CM, 1)
                if kw["sy"]:
                    y = A["Y"].get()[z][0]
                    w.add("Y", y, m1 * z1, m1 * z1a, stages * C)
                    assert np.array_equal(y > 0, m1), "mb disagrees with the stored activation"
                if kw["tq"]:
                    got = f64(A["tq"].get()[z][0][:, 0])
                    if c.kind == "fwd3":
                        got = got + f64(A["tq2"].get()[z][0][:, 0])
                    w.add("tq", got, ref_tail(m1 * z1, d["tw"][z][0], d["tb"][z]),
                          ref_tail(m1 * z1a, np.abs(d["tw"][z][0]), np.abs(d["tb"][z])), stages * C)
    elif c.kind in ("dgrad", "dgrad3"):
        for z in zz:
            w1 = f64(d["W"][z])      # logical (out k, in n)
            xb = d["xbits_pos"][z]
            if c.kw["plain"]:
                dz0, dz0a = ref_dz0_plain(xb, d["Z"][z], w1), ref_dz0_plain(xb, np.abs(d["Z"][z]), np.abs(w1))
            else:
                args = (d["abits_pos"][z], xb, d["dq"][z][:, 0], d["wt"][z][0], w1)
                dz0, dz0a = ref_dz0(*args), ref_dz0(*[np.abs(f64(v)) for v in args])
            if not c.kw["w0"]:
                w.add("dz0", A["C"].get()[z][0], dz0, dz0a, C)
                continue
            x1 = f64(d["X"][z][:, :in0])
            gw = f64(A["w0_out"].get()[z][:c.per_z])
            if gw.shape[-1] == N:      # EnsembleLinear slab layout (in0, 256)
                gw = np.swapaxes(gw, -1, -2)
            gb = f64(A["b0_out"].get()[z][:c.per_z, 0])
            for s in range(c.per_z):
                rows = slab_rows(M, c.per_z, s)
                (rw, rb), (aw, ab) = ref_w0(dz0, x1, rows), ref_w0(dz0a, np.abs(x1), rows)
                w.add(f"dW0 slab {s}", gw[s], rw, aw, C)
                w.add(f"db0 slab {s}", gb[s], rb, ab, C)
            rows = np.arange(M)
            (rw, rb), (aw, ab) = ref_w0(dz0, x1, rows), ref_w0(dz0a, np.abs(x1), rows)
            w.add("dW0", gw.sum(0), rw, aw, C)
            w.add("db0", gb.sum(0), rb, ab, C)
    else:
        kw = c.kw
        plain = kw["plain"] or c.kind == "wgrad3p"
        tails, derived = kw["tails"], (kw["derived"] or c.ints["np3"]) and not kw["tails"]
        for z in zz:
            stages = 1
            if kw["recompute"]:
                x0 = f64(d["X0"][z][:, :in0])
                h0 = np.maximum(ref_layer(x0, d["W0"][z], d["b0"][z]), 0)
                h0a = ref_layer(np.abs(x0), np.abs(d["W0"][z]), np.abs(d["b0"][z]))
                stages = 2
            else:
                h0 = f64(d["H0"][z])
                h0a = np.abs(h0)
            gW, gb = f64(A["dW"].get()[z][:c.per_z]), f64(A["db"].get()[z][:c.per_z, 0])
            sets = [(f" slab {s}", slab_rows(M, c.per_z, s), lambda a, s=s: a[s]) for s in range(c.per_z)] + [("", np.arange(M), lambda a: a.sum(0))]
            for tag, rows, pick in sets:
                if plain:
                    (rw, rb), (aw, ab) = ref_wgrad_plain(d["dZ"][z], h0, rows), ref_wgrad_plain(np.abs(d["dZ"][z]), h0a, rows)
                else:
                    pos, dq, wt = d["abits_pos"][z], d["dq"][z][:, 0], d["wt"][z][0]
                    rw, rb, G, g = ref_wgrad(pos, dq, h0, wt, rows)
                    aw, ab, Ga, ga = ref_wgrad(pos, np.abs(dq), h0a, np.abs(wt), rows)
                w.add("dW" + tag, pick(gW), rw, aw, stages * C)
                w.add("db" + tag, pick(gb), rb, ab, stages * C)
                if tails or derived:
                    gt, gbt = pick(f64(A["dwt"].get()[z][:c.per_z, 0])), pick(f64(A["dbt"].get()[z][:c.per_z, 0, 0]))
                    if tails:
                        (rt, rbt), (at, abt) = ref_tails(dq, d["H1"][z], rows), ref_tails(np.abs(dq), d["H1"][z], rows)
                    else:
                        rt, at = ref_derived(G, g, d["W1"][z], d["b1"][z][0]), ref_derived(Ga, ga, np.abs(d["W1"][z]), np.abs(d["b1"][z][0]))
                        rbt, abt = f64(dq)[rows].sum(), np.abs(f64(dq))[rows].sum()
                    w.add("dwt" + tag, gt, rt, at, C)
                    w.add("dbt" + tag, gbt, rbt, abt, C)
    MEASURED[c.stage] = max(MEASURED.get(c.stage, 0.0), w.worst())
    bad = [(t, r) for t, r in w.items if not r < c.bar]
    assert not bad, ("componentwise error / (C * abs-sum), bar", c.bar, c.stage, c.report["flavour"], bad[:8])
    return w


# ---- case lists ----
# every instantiation of the tap's table -> the arguments that reach it (M = 256, per_z = 2, two problems)
def _fwd_flavours():
    out = {}
    for f32 in (0, 1):
        for tq, l0, dgm, sy, xs in [(1, 0, 0, 1, 1), (0, 0, 0, 1, 1), (1, 1, 0, 1, 1), (0, 1, 0, 1, 1), (0, 0, 1, 1, 1), (1, 1, 0, 0, 1), (1, 0, 0, 0, 1),
                                    (1, 1, 0, 0, 0), (0, 1, 0, 1, 0)]:
            out[f"ws_fwd<{tq},{l0},{dgm},{sy},{f32},{xs}>"] = dict(kind="fwd", f32=f32, tq=bool(tq), l0=bool(l0), dgm=bool(dgm), sy=bool(sy), discard=not xs)
    for tq, sy, xs, l0, dgm in [(1, 0, 1, 1, 0), (1, 1, 1, 1, 0), (0, 1, 1, 1, 0), (1, 0, 0, 1, 0), (0, 1, 0, 1, 0), (1, 0, 0, 0, 0), (1, 1, 0, 0, 0), (0, 1, 0, 0, 0),
                                (0, 1, 0, 0, 1)]:
        out[f"ws_fwd3<{tq},{sy},{xs},{l0},{dgm}>"] = dict(kind="fwd3", tq=bool(tq), sy=bool(sy), l0=bool(l0), dgm=bool(dgm), discard=bool(l0 and not xs))
    return out


def _bwd_flavours():
    out = {}
    for f32, name in ((0, "ws_dgrad"), (1, "ws_dgrad32")):
        out[f"{name}<1,0,0>"] = dict(kind="dgrad", f32=f32)
        out[f"{name}<0,1,0>"] = dict(kind="dgrad", f32=f32, w0=False)
        out[f"{name}<1,0,1>"] = dict(kind="dgrad", f32=f32, plain=True)
    out["ws_dgrad3<1,0>"] = dict(kind="dgrad3")
    out["ws_dgrad3<0,0>"] = dict(kind="dgrad3", w0=False)
    out["ws_dgrad3<1,1>"] = dict(kind="dgrad3", plain=True)
    for f32, name in ((0, "ws_wgrad"), (1, "ws_wgrad32")):
        out[f"{name}<0>"] = dict(kind="wgrad", f32=f32)
        out[f"{name}<1>"] = dict(kind="wgrad", f32=f32, tails=True)
        out[f"{name}<2>"] = dict(kind="wgrad", f32=f32, derived=True)
        out[f"{name}<3>"] = dict(kind="wgrad", f32=f32, plain=True)
        out[f"{name}<4>"] = dict(kind="wgrad", f32=f32, plain=True, recompute=True)
    out["ws_wgrad<5>"] = dict(kind="wgrad", np3=1, derived=True)
    out["ws_wgrad3p"] = dict(kind="wgrad3p", plain=True)
    return out


FLAVOURS = {**_fwd_flavours(), **_bwd_flavours()}
UNREACHED = {}      # instantiation -> why no launch reaches it (none: every instantiation has a case above)

# the depth sweep: the flavours bench.py runs, their exact / three-plane siblings, and one plain flavour per launcher
DEPTH_FLAVOURS = ["ws_fwd<1,1,0,0,0,1>", "ws_fwd<1,1,0,0,1,1>", "ws_fwd3<1,0,1,1,0>", "ws_fwd<0,0,0,1,0,1>", "ws_fwd3<0,1,0,0,0>",
                  "ws_dgrad<1,0,0>", "ws_dgrad32<1,0,0>", "ws_dgrad3<1,0>", "ws_dgrad<1,0,1>", "ws_dgrad3<1,1>",
                  "ws_wgrad<2>", "ws_wgrad32<2>", "ws_wgrad<5>", "ws_wgrad<3>", "ws_wgrad32<3>", "ws_wgrad3p"]
LAUNCHER_OF = {name: FLAVOURS[name]["kind"] for name in FLAVOURS}


def depth_cases():
    return [(name, M, per_z) for name in DEPTH_FLAVOURS for M, per_z in DEPTHS]


def depth_kwargs(name, M, per_z):
    return dict(FLAVOURS[name], M=M, per_z=per_z, nz0=1, nz1=2, seed=M + per_z)


# geometry: (label, flavour, overrides)
def geometry_cases():
    out = []
    fused = ["ws_fwd<1,1,0,1,0,1>", "ws_fwd<1,1,0,0,1,0>", "ws_fwd3<1,1,1,1,0>", "ws_dgrad<1,0,0>", "ws_dgrad32<1,0,0>", "ws_dgrad3<1,0>", "ws_wgrad<4>", "ws_wgrad32<4>"]
    for name in fused:
        for in0, xp in ((3, 4), (23, 24), (31, 32), (3, 32)):
            out.append((f"in0 {in0} pitch {xp}", name, dict(in0=in0, x0_pitch=xp, seed=in0, family="in0 3" if in0 == 3 else "base")))
    for name in ["ws_fwd<1,1,0,1,0,1>", "ws_fwd<0,0,0,1,1,1>", "ws_fwd<0,0,1,1,0,1>", "ws_fwd3<1,1,1,1,0>", "ws_fwd3<0,1,0,0,1>", "ws_dgrad<1,0,0>", "ws_dgrad32<0,1,0>",
                 "ws_dgrad<1,0,1>", "ws_dgrad3<1,0>", "ws_wgrad<4>"]:
        out.append(("EnsembleLinear weights", name, dict(ens=True, seed=5)))
    for name in ["ws_dgrad<1,0,0>", "ws_dgrad32<1,0,1>", "ws_dgrad3<1,0>", "ws_dgrad3<1,1>"]:
        out.append(("EnsembleLinear slabs", name, dict(slab_ens=True, ens=True, seed=6)))
    for name in ["ws_fwd<1,1,0,1,0,1>", "ws_fwd<1,0,0,1,1,1>", "ws_fwd<0,0,1,1,0,1>", "ws_fwd3<1,1,1,1,0>", "ws_dgrad<1,0,0>", "ws_dgrad32<0,1,0>", "ws_dgrad<1,0,1>",
                 "ws_dgrad3<1,0>", "ws_wgrad<1>", "ws_wgrad<2>", "ws_wgrad32<3>", "ws_wgrad<4>", "ws_wgrad<5>", "ws_wgrad3p"]:
        out.append(("3 x 2 problems, wide strides", name, dict(nz0=3, nz1=2, wide=True, seed=7)))
    for pad in (4, 12):
        for name in ["ws_fwd<1,1,0,1,0,1>", "ws_fwd<1,0,0,1,1,1>", "ws_fwd<0,0,1,1,0,1>", "ws_fwd3<1,1,1,1,0>", "ws_fwd3<1,1,0,0,0>", "ws_dgrad<0,1,0>", "ws_dgrad32<1,0,1>",
                     "ws_dgrad3<0,0>", "ws_dgrad3<1,1>", "ws_wgrad<1>", "ws_wgrad32<2>", "ws_wgrad<3>", "ws_wgrad<4>", "ws_wgrad<5>", "ws_wgrad3p"]:
            out.append((f"pitches padded by {pad}", name, dict(pad=pad, seed=8 + pad)))
    for sm in (1, 3):
        for name in ["ws_fwd<1,1,0,0,0,1>", "ws_fwd<1,0,0,1,1,1>", "ws_fwd3<1,0,1,1,0>"]:
            out.append((f"tq_sm {sm}", name, dict(tq_sm=sm, seed=20 + sm)))
        for name in ["ws_dgrad<1,0,0>", "ws_dgrad32<0,1,0>", "ws_dgrad3<1,0>", "ws_wgrad<2>", "ws_wgrad32<1>", "ws_wgrad<5>"]:
            out.append((f"dq_sm {sm}", name, dict(dq_sm=sm, seed=22 + sm)))
    for gs in (None, 2.0 ** -6, 2.0 ** 9):
        for name in ["ws_fwd<0,0,1,1,0,1>", "ws_fwd3<0,1,0,0,1>", "ws_dgrad<1,0,0>", "ws_dgrad<1,0,1>", "ws_dgrad3<1,0>", "ws_dgrad3<1,1>", "ws_wgrad<2>", "ws_wgrad<1>",
                     "ws_wgrad<3>", "ws_wgrad<4>", "ws_wgrad<5>", "ws_wgrad3p"]:
            out.append((f"gscale {gs}", name, dict(gscale=gs, seed=30, family="gscale down" if gs is not None and gs < 1 else "base")))
    return out


def geometry_kwargs(name, over):
    return {**FLAVOURS[name], **over}
