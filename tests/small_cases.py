"""Float64 references of what the few-rows kernels compute -- small_fwd_kernel<F32, QG> (csrc/small_fwd.hip: the whole
[in0 -> 256 -> 256 -> out] forward, the unit-seed backward G = dQ/da of QG mode, the tanh-Gaussian sampling epilogue) and
small_abwd_kernel<F32> (csrc/small_bwd.hip: actor loss + temperature Adam step + head backward + actor backward, one split-K slab per
32-row group) -- with the case lists and the case runner that tests/test_gpu_small_paths.py (GPU) and tests/test_small_paths_cpu.py (no
device) share.  Every launch goes through the unit tap orl_debug_small (offlinerlkit._engine.debug_small).  Arr, check_guards
and FLIP_SHARE are tests/ws_cases.py's (the kernels here return activations, not mask words: nothing to pack), bound(precision) is tests/test_gpu_backward_f64.py's.

Bars are componentwise: |got - f64| <= stages * C * (the same expression with every term replaced by its absolute value), C =
bound(precision).  One stage is one matrix product or one elementwise formula on operands the kernel was given or returned; a product
whose operand never leaves the chip adds a stage (ws_cases.py's rule).
  small_fwd (H0 and H1 stored): H0 against relu(X W0^T + b0), H1 against the kernel's own H0, OUT against the kernel's own H1: one
    stage each.  A mask difference H_got > 0 against z_f64 > 0 must sit on |z_f64| <= C * abs-sum; at most FLIP_SHARE of a problem's
    units may differ.  QG: G[m][a] = sum_j 1[H0_got > 0] W0[j][gc0 + a] sum_n 1[H1_got > 0] wt[n] W1[n][j], two stages.
  sampling epilogue, from the kernel's own OUT rows: act against tanh(mu + exp(clamp(ls, -5, 2)) eps) within KA * 2^-24 * ((|mu| +
    sigma |eps|) (1 - act^2) + |act|) (tanh' = 1 - act^2 carries the rounding of u, |act| the rounding of the result); logp against
    sample.h's formula evaluated in float64 on the returned act, within K * 2^-24 * (abs-sum of the terms + sum_a act^2 / (1 - act^2 +
    1e-6)), where the quadratic term's abs-sum is (|u| + |mu|)^2 / (2 sigma^2) (dm = u - mu is a difference of rounded numbers) and the
    last term is the condition number of log(1 - a^2 + 1e-6).
  small_abwd (every operand is an input, the masks are H0 > 0 and H1 > 0 of the given arrays: no flips): dhead per row follows
    small_bwd.hip's dhead block = oracle/nn.py tanh_gauss_bwd; its abs-sum replaces 1 - act^2 by 1 + act^2 in the numerators.  Slabs:
    off_bh 1 stage, off_wh 2, off_b1 2, off_w1 3, off_w0 / off_b0 4, each slab against the reference of exactly its own 32 rows.
    part[run][g] = the group's float64 sums (1 stage); metrics from the kernel's own part; the Adam step of log_alpha against
    torch-semantics Adam in float64 on the kernel's own part sums, within ADAM_K * 2^-24 * abs-sum.
K, KA and ADAM_K are twice the worst ratio of a float32 numpy evaluation of the same formulas against float64 on the GPU file's seeds
(tests/test_small_paths_cpu.py measures them and asserts the margin): measured 2.444 (logp), 1.823 (act), 1.591 (Adam) -> K = 4.9,
KA = 3.7, ADAM_K = 3.2.

Operands are O(1): standard normal rows, weights U(+-1/16), ga ~ N(0, 1), qa ~ N(0, 1), act = tanh(u) with |act| <= 0.995 in the base
cases.

Measured on an MI355X (fp16 hi + lo planes build) over the 162 launches of tests/test_gpu_small_paths.py, worst |got - f64| / bar per
stage (the bar = stages * C * abs-sum, or the K bound; p0 exact fp32, p1 split planes):
  small_fwd   p0: H0 0.18, H1 0.14, OUT 0.18, G 0.004; in0 <= 2: H0 0.06, H1 0.09, OUT 0.14; action 0.39, logp 0.43
              p1: H0 0.05, H1 0.06, OUT 0.09, G 0.002; in0 <= 2: H0 0.27, H1 0.06, OUT 0.05; action 0.40, logp 0.32
              saturated actions (|u| > 10): exactly +-1, logp 0.00 of its bound (the condition term dominates it)
  small_abwd  p0: bh 0.04, wh 0.04, b1 0.008, w1 0.03, w0 0.003, b0 0.001, part 0.07, metrics 0.30, Adam 0.22
              p1: bh 0.04, wh 0.02, b1 0.005, w1 0.85, w0 0.001, b0 0.0006, part 0.07, metrics 0.30, Adam 0.22
Every stage passes at its stage count of C, so BARS is empty: no split-precision stage needed the fp16-floor allowance of ws_cases.py
(the largest, dW1 of the split actor backward at 0.85 of 3 C, against 0.03 for its exact-fp32 twin on the same cases)."""
import numpy as np

from offlinerlkit import _engine
from offlinerlkit._engine import GEMM_SENTINEL, OrlGemmBuf
from test_gpu_backward_f64 import bound
from ws_cases import FLIP_SHARE, Arr, check_guards

N = 256
MAXGROUPS = 64
LOG_SQRT_2PI = 0.91893853320467274178
U24 = 2.0 ** -24
K_LOGP, K_ACT, ADAM_K = 4.9, 3.7, 3.2      # twice the float32-numpy ratios (module docstring; test_small_paths_cpu.py re-measures them)
MEASURED = {}                # stage -> worst ratio seen by this process
# stage -> bar in units of stages * C, for split-precision stages that exceed 1 only through the absolute floor of the fp16 planes (twice
# the worst measured ratio, next to the ratio of the exact-fp32 twin on the same cases): none was needed (module docstring)
BARS = {}


def f64(a):
    return np.asarray(a, dtype=np.float64)


def as32(a):
    return np.asarray(a, dtype=np.float32)


class Case:
    pass


class JobArr(Arr):
    """a job's dst: the logical elements are rows dst_row0 .. of columns dst_col .. dst_col + A; the tap is given the matrix's base"""

    def __init__(self, rows, A, nz0, row0, col, pad, base=0, wide=False):
        pitch = col + A + pad
        super().__init__(rows, A, nz0, 1, pitch=pitch, off=base + row0 * pitch + col, wide=wide, result=True)
        self.base = base

    def desc(self):
        return OrlGemmBuf(self.raw.ctypes.data, self.n, self.base, self.pitch, self.s0, self.s1, self.kstride)


def _weights(rng, *shape):
    return ((rng.random_sample(shape) * 2 - 1) / 16).astype(np.float32)


# =====================================================================================================================================
# references (float64)
# =====================================================================================================================================
def ref_layer(x, w, b):
    return f64(x) @ f64(w).T + f64(b)


def ref_qg(m0, m1, w0cols, wt, w1):
    """G[m][a] = sum_j m0[m][j] W0[j][gc0 + a] sum_n m1[m][n] wt[n] W1[n][j]"""
    return (f64(m0) * ((f64(m1) * f64(wt)) @ f64(w1))) @ f64(w0cols)


def ref_sample(mu, ls_raw, eps, act=None):
    """sample.h in float64.  Returns (act, logp terms summed over A, abs-sum of the logp terms incl. the condition term, bound scale of act);
    with ``act`` given the log-probability is evaluated on it (the kernel's returned action)."""
    mu, ls_raw, eps = f64(mu), f64(ls_raw), f64(eps)
    ls = np.clip(ls_raw, -5.0, 2.0)
    sg = np.exp(ls)
    u = mu + sg * eps
    a_ref = np.tanh(u)
    a = a_ref if act is None else f64(act)
    dm = u - mu
    om = (1.0 - a * a) + 1e-6
    terms = (-(dm * dm) / (2.0 * sg * sg) - ls - LOG_SQRT_2PI) - np.log(om)
    absum = (np.abs(u) + np.abs(mu)) ** 2 / (2.0 * sg * sg) + np.abs(ls) + LOG_SQRT_2PI + np.abs(np.log(om)) + a * a / om
    a_scale = (np.abs(mu) + sg * np.abs(eps)) * (1.0 - a_ref * a_ref) + np.abs(a_ref)
    return a_ref, terms.sum(-1), absum.sum(-1), a_scale


def ref_dhead(q0, q1, g0, g1, ls_raw, eps, act, alpha, M):
    """small_bwd.hip's dhead block / oracle/nn.py tanh_gauss_bwd, float64: returns (dhead [rows][2A], its absolute-value twin)"""
    q0, q1, g0, g1, ls_raw, eps, act = [f64(v) for v in (q0, q1, g0, g1, ls_raw, eps, act)]
    qmin = np.minimum(q0, q1)
    nmin = (q0 == qmin).astype(np.float64) + (q1 == qmin)
    w0, w1 = (q0 == qmin) * (-1.0 / M) / nmin, (q1 == qmin) * (-1.0 / M) / nmin
    da, da_a = w0[:, None] * g0 + w1[:, None] * g1, np.abs(w0)[:, None] * np.abs(g0) + np.abs(w1)[:, None] * np.abs(g1)
    dlogp = float(alpha) / M
    sg = np.exp(np.clip(ls_raw, -5.0, 2.0))
    om, om_a = 1.0 - act * act, 1.0 + act * act
    t, t_a = 2.0 * act * om / (om + 1e-6), 2.0 * np.abs(act) * om_a / (om + 1e-6)
    du, du_a = da * om + dlogp * t, da_a * om_a + abs(dlogp) * t_a
    gate = (ls_raw >= -5.0) & (ls_raw <= 2.0)
    dls, dls_a = (du * sg * eps - dlogp) * gate, (du_a * sg * np.abs(eps) + abs(dlogp)) * gate
    return np.concatenate([du, dls], 1), np.concatenate([du_a, dls_a], 1)


def ref_abwd_group(dh, h1, h0, x, wh, w1):
    """the six tensors of one 32-row group from its dhead rows: dict name -> array (linear in dh: the abs twin takes |.| of everything)"""
    dh, h1, h0, x, wh, w1 = [f64(v) for v in (dh, h1, h0, x, wh, w1)]
    dz1 = (h1 > 0) * (dh @ wh)
    dz0 = (h0 > 0) * (dz1 @ w1)
    return {"bh": dh.sum(0), "wh": dh.T @ h1, "b1": dz1.sum(0), "w1": dz1.T @ h0, "w0": dz0.T @ x, "b0": dz0.sum(0)}


def ref_abwd_group_abs(dh_a, h1, h0, x, wh, w1):
    dh_a, h1, h0, x, wh, w1 = [np.abs(f64(v)) for v in (dh_a, h1, h0, x, wh, w1)]
    dz1 = (h1 > 0) * (dh_a @ wh)
    dz0 = (h0 > 0) * (dz1 @ w1)
    return {"bh": dh_a.sum(0), "wh": dh_a.T @ h1, "b1": dz1.sum(0), "w1": dz1.T @ h0, "w0": dz0.T @ x, "b0": dz0.sum(0)}


STAGES = {"bh": 1, "wh": 2, "b1": 2, "w1": 3, "w0": 4, "b0": 4}


def ref_adam(p, m, v, g, lr, b1, b2, eps, t, dt=np.float64):
    """torch.optim.Adam, single tensor (csrc/scalars.h adam_scalar); dt = float32 gives the emulation the K measurement uses.  Returns
    (p, m, v) and the abs-sums of the three updates."""
    T = dt
    b1, b2, eps, lr = [float(np.float32(x)) for x in (b1, b2, eps, lr)]      # the kernel holds them as floats
    p, m, v, g = T(p), T(m), T(v), T(g)
    one = T(1.0)
    m2 = m + (g - m) * (one - T(b1))
    v2 = v * T(b2) + (one - T(b2)) * g * g
    bc1, bc2 = 1.0 - float(b1) ** int(t), 1.0 - float(b2) ** int(t)
    step, bc2s = T(float(lr) / bc1), T(np.sqrt(bc2))
    upd = step * (m2 / (np.sqrt(v2) / bc2s + T(eps)))
    p2 = p - upd
    sums = (abs(float(p)) + abs(float(upd)), abs(float(m)) + (abs(float(g)) + abs(float(m))) * (1.0 - float(b1)), abs(float(v)) * float(b2) + (1.0 - float(b2)) * float(g) ** 2)
    return (p2, m2, v2), sums


# RunScalars as 16 floats (csrc/scalars.h)
SC = {"log_alpha": 0, "la_m": 1, "la_v": 2, "alpha": 6, "alpha_bwd": 7}


# =====================================================================================================================================
# small_fwd cases
# =====================================================================================================================================
def build_fwd(M=64, nz0=1, nz1=1, f32=0, in0=14, x_pitch=None, out_dim=5, o_pad=3, h0=True, h1=True, gn=0, gc0=0, g_pad=2, A=0, jobs=(), wide=False,
              seed=0, off=None, short=None, ints=None, fix=None, family="base"):
    """One small_fwd launch.  gn > 0: QG mode (out_dim must be 1).  jobs: dicts (head_row0, rows, rep, eps=True, logp=True, dst_row0=0,
    dst_col=0, dst_pad=0).  fix: {output column: bias}: that column's tail weights are zero, so OUT there is exactly the bias (the clamp
    edges and the saturated actions).  off / short: {array: base offset / elements missing at the end}; ints: overrides of the tap's fields."""
    c = Case()
    c.kind, c.M, c.nz0, c.nz1, c.in0, c.out_dim, c.gn, c.gc0, c.A = "fwd", M, nz0, nz1, in0, out_dim, gn, gc0, A
    c.prec = 0 if f32 else 1
    c.C = bound(c.prec)
    c.family = family
    rng = np.random.RandomState(7000 + seed)
    Z = (nz0, nz1)
    xp = in0 if x_pitch is None else x_pitch
    arrays, d = {}, {}

    def arr(name, rows, cols, data=None, result=False, pitch=None):
        a = Arr(rows, cols, nz0, nz1, pitch=pitch, off=(off or {}).get(name, 0), wide=wide, result=result)
        if data is not None:
            d[name] = as32(data).reshape(nz0, nz1, rows, cols)
            a.put(d[name])
        arrays[name] = a
        return a

    arr("X", M, in0, rng.standard_normal(Z + (M, in0)), pitch=xp)
    arr("W0", N, in0, _weights(rng, *Z, N, in0))
    arr("b0", 1, N, _weights(rng, *Z, 1, N))
    arr("W1", N, N, _weights(rng, *Z, N, N))
    arr("b1", 1, N, _weights(rng, *Z, 1, N))
    wt, bt = _weights(rng, *Z, out_dim, N), rng.standard_normal(Z + (1, out_dim)).astype(np.float32) * 0.5
    if A:      # log sigma columns spread over the clamp's interior
        bt[..., A:] = rng.uniform(-4.0, 1.5, Z + (1, out_dim - A))
    for col, val in (fix or {}).items():
        wt[..., col, :] = 0
        bt[..., 0, col] = val
    arr("Wt", out_dim, N, wt)
    arr("bt", 1, out_dim, bt)
    if h0:
        arr("H0", M, N, result=True)
    if h1:
        arr("H1", M, N, result=True)
    arr("OUT", M, out_dim, result=True, pitch=out_dim + o_pad)
    if gn:
        arr("G", M, gn, result=True, pitch=gn + g_pad)
    c.jobs, c.job_specs = [], []
    for ji, js in enumerate(jobs):
        js = dict(dict(eps=True, logp=True, dst_row0=0, dst_col=0, dst_pad=0), **js)
        rows = js["rows"]
        job = dict(head_row0=js["head_row0"], rows=rows, rep=js["rep"], dst_row0=js["dst_row0"], dst_col=js["dst_col"])
        if js["eps"]:
            e = Arr(rows, A, nz0, 1, wide=wide)
            d[f"eps{ji}"] = rng.standard_normal((nz0, 1, rows, A)).astype(np.float32)
            e.put(d[f"eps{ji}"])
            job["eps"] = arrays[f"job{ji}.eps"] = e
        job["dst"] = arrays[f"job{ji}.dst"] = JobArr(rows, A, nz0, js["dst_row0"], js["dst_col"], js["dst_pad"], wide=wide)
        if js["logp"]:
            job["logp"] = arrays[f"job{ji}.logp"] = Arr(rows, 1, nz0, 1, wide=wide, result=True)
        c.jobs.append(job)
        c.job_specs.append(js)
    for name, cut in (short or {}).items():
        arrays[name].n = int(arrays[name].idx.max()) + 1 - cut
    c.ints = dict(M=M, nz0=nz0, nz1=nz1, f32=f32, in0=in0, out_dim=out_dim, gc0=gc0, gn=gn, A=A)
    c.ints.update(ints or {})
    c.arrays, c.d = arrays, d
    c.before = {k: a.raw.copy() for k, a in arrays.items()}
    # what ws_cases.check_guards reads
    c.per_z, c.kw = 0, {"l0": False}
    return c


DEVICE_ERRORS = []      # a launch that failed on the device (not a refusal): nothing more is launched from this process


def run(c, dry_run=False):
    assert dry_run or not DEVICE_ERRORS, ("an earlier launch failed on the device; no further launches", DEVICE_ERRORS[0])
    tap = {k: a for k, a in c.arrays.items() if not k.startswith("job")}
    try:
        c.report = _engine.debug_small(c.kind, tap, jobs=getattr(c, "jobs", ()), dry_run=int(dry_run), **c.ints)
    except RuntimeError as e:
        if "orl_debug_small device:" in str(e) or "no HIP device" in str(e):
            DEVICE_ERRORS.append(str(e))
        raise
    return c.report


def _zz(c):
    return [(a, b) for a in range(c.nz0) for b in range(c.nz1)]


class Worst:
    """collects err / bound ratios per stage; asserts at the end so that one run reports every figure"""

    def __init__(self, c):
        self.c, self.items = c, []

    def add(self, tag, got, ref, scale):
        """scale = the full bound (stages * C * abs-sum, or K * 2^-24 * abs-sum)"""
        err = np.abs(f64(got) - f64(ref))
        ratio = float((err / (f64(scale) + 1e-300)).max()) if err.size else 0.0
        if not np.all(np.isfinite(f64(got))):
            ratio = float("inf")
        self.items.append((tag, ratio))

    def worst(self):
        return max((r for _, r in self.items), default=0.0)

    def finish(self):
        c = self.c
        bad = []
        for tag, r in self.items:
            stage = f"{c.kind} p{c.prec} {c.family} {tag.split(' ')[0]}"
            MEASURED[stage] = max(MEASURED.get(stage, 0.0), r)
            if not r < BARS.get(stage, 1.0):
                bad.append((tag, r, BARS.get(stage, 1.0)))
        assert not bad, ("componentwise error / bound (tag, ratio, bar)", c.kind, c.report["flavour"], bad[:8])
        return self


def check_flips(tag, got, z, za, C):
    flip = (f64(got) > 0) != (z > 0)
    assert np.all(np.abs(z[flip]) <= C * za[flip]), (tag, "the sign of a unit differs from float64 where |z| exceeds the bar")
    assert flip.mean() <= FLIP_SHARE, (tag, "share of units whose sign differs from float64", float(flip.mean()))


def job_rows(js, ji=None):
    """head row of every output row of a job"""
    return js["head_row0"] + np.arange(js["rows"]) // js["rep"]


def check_fwd(c, hidden=True):
    """asserts a small_fwd launch against float64 and the guard words; hidden = False: a launch without stored H0 / H1 is held to the
    guards only (its OUT / G are compared bit for bit with the storing launch by the caller)"""
    check_guards(c)
    w = Worst(c)
    A, d, C = c.arrays, c.d, c.C
    for z in _zz(c):
        if not hidden or "H0" not in A or "H1" not in A:
            break
        x, w0, b0, w1, b1, wt, bt = [d[k][z] for k in ("X", "W0", "b0", "W1", "b1", "Wt", "bt")]
        H0, H1, OUT = A["H0"].get()[z][0], A["H1"].get()[z][0], A["OUT"].get()[z][0]
        z0, z0a = ref_layer(x, w0, b0), ref_layer(np.abs(x), np.abs(w0), np.abs(b0))
        check_flips("H0", H0, z0, z0a, C)
        w.add("H0", H0, np.maximum(z0, 0), C * z0a)
        z1, z1a = ref_layer(H0, w1, b1), ref_layer(np.abs(H0), np.abs(w1), np.abs(b1))
        check_flips("H1", H1, z1, z1a, C)
        w.add("H1", H1, np.maximum(z1, 0), C * z1a)
        w.add("OUT", OUT, ref_layer(H1, wt, bt), C * ref_layer(np.abs(H1), np.abs(wt), np.abs(bt)))
        if c.gn:
            cols = slice(c.gc0, c.gc0 + c.gn)
            ref, ra = ref_qg(H0 > 0, H1 > 0, w0[:, cols], wt[0], w1), ref_qg(H0 > 0, H1 > 0, np.abs(w0[:, cols]), np.abs(wt[0]), np.abs(w1))
            w.add("G", A["G"].get()[z][0], ref, 2 * C * ra)
    for ji, js in enumerate(c.job_specs):
        for r in range(c.nz0):
            OUT = f64(c.arrays["OUT"].get()[r, 0, 0])
            hr = job_rows(js)
            mu, ls = OUT[hr, :c.A], OUT[hr, c.A:2 * c.A]
            eps = d[f"eps{ji}"][r, 0] if js["eps"] else np.zeros_like(mu)
            act = c.arrays[f"job{ji}.dst"].get()[r, 0, 0]
            a_ref, lp, lp_abs, a_scale = ref_sample(mu, ls, eps, act)
            w.add(f"act job {ji}", act, a_ref, K_ACT * U24 * a_scale)
            sat = np.abs(mu + np.exp(np.clip(ls, -5, 2)) * eps) > 10.0
            assert np.all(np.abs(f64(act)[sat]) == 1.0), "a saturated action (|u| > 10) is not exactly +-1"
            if js["logp"]:
                w.add(f"logp job {ji}", c.arrays[f"job{ji}.logp"].get()[r, 0, 0, :, 0], lp, K_LOGP * U24 * lp_abs)
    return w.finish()


def emulate_fwd(c):
    """what a correct kernel leaves in the result arrays, in float32 numpy (no device)"""
    run(c, dry_run=True)
    A, d = c.arrays, c.d

    def put(name, z, data):
        a = A[name]
        a.raw.view(a.dtype)[a.idx[z][0]] = as32(data).reshape(a.idx[z][0].shape)

    c.z32 = {}
    for z in _zz(c):
        x, w0, b0, w1, b1, wt, bt = [d[k][z] for k in ("X", "W0", "b0", "W1", "b1", "Wt", "bt")]
        z0 = x @ w0.T + b0
        h0 = np.maximum(z0, 0)
        z1 = h0 @ w1.T + b1
        h1 = np.maximum(z1, 0)
        out = h1 @ wt.T + bt
        c.z32["z0", z], c.z32["z1", z] = z0, z1
        if "H0" in A:
            put("H0", z, h0)
        if "H1" in A:
            put("H1", z, h1)
        put("OUT", z, out)
        if c.gn:
            put("G", z, ((h0 > 0) * (((h1 > 0) * wt[0]) @ w1)) @ w0[:, c.gc0:c.gc0 + c.gn])
    for ji, js in enumerate(c.job_specs):
        for r in range(c.nz0):
            OUT = A["OUT"].get()[r, 0, 0]
            hr = job_rows(js)
            mu, ls = OUT[hr, :c.A], OUT[hr, c.A:2 * c.A]
            eps = d[f"eps{ji}"][r, 0] if js["eps"] else np.zeros_like(mu)
            act, lp = sample32(mu, ls, eps)
            put(f"job{ji}.dst", (r, 0), act)
            if js["logp"]:
                put(f"job{ji}.logp", (r, 0), lp)
    return c


def sample32(mu, ls_raw, eps):
    """sample.h's arithmetic, operation by operation in float32 numpy"""
    one, two = np.float32(1), np.float32(2)
    mu, ls_raw, eps = as32(mu), as32(ls_raw), as32(eps)
    ls = np.minimum(np.maximum(ls_raw, np.float32(-5)), two)
    sg = np.exp(ls)
    u = mu + sg * eps
    act = np.tanh(u)
    dm = u - mu
    terms = (-(dm * dm) / (two * (sg * sg)) - ls - np.float32(LOG_SQRT_2PI)) - np.log((one - act * act) + np.float32(1e-6))
    return act, terms.sum(-1, dtype=np.float32)


# =====================================================================================================================================
# small_abwd cases
# =====================================================================================================================================
def slab_layout(in0, A, shuffled=True):
    """offsets of the six tensors inside a slab, with gaps of odd sizes between them and room for 16 head rows; returns (offsets, o_ks)"""
    order = ["bh", "w1", "b0", "wh", "w0", "b1"] if shuffled else ["w0", "b0", "w1", "b1", "wh", "bh"]
    room = {"w0": N * in0, "b0": N, "w1": N * N, "b1": N, "wh": 16 * N, "bh": 16}
    offs, at = {}, 3
    for i, k in enumerate(order):
        offs[k] = at
        at += room[k] + 5 + 2 * i
    return offs, (at + 3) & ~3


def slab_len(k, in0, A):
    return {"w0": N * in0, "b0": N, "w1": N * N, "b1": N, "wh": 2 * A * N, "bh": 2 * A}[k]


def build_abwd(M=64, runs=1, f32=0, in0=17, x_pitch=None, A=6, ga_pad=2, xa_col=3, xa_pad=1, auto_alpha=1, clamp_alpha01=0, log_alpha=-0.3, gstep=0,
               seed=0, off=None, short=None, ints=None, family="base"):
    """One small_abwd launch.  Every case carries the edge rows: row 1 a tie q0 == q1, row 2 q1 < q0, row 6 q0 < q1, rows 2 / 3 / 4 log sigma at,
    below and one ulp below -5.0, rows 7 / 8 / 9 at, above and one ulp above 2.0, row 5 all-zero H0 / H1, exact zeros in H0 / H1 everywhere (ReLU outputs)."""
    c = Case()
    c.kind, c.M, c.nz0, c.nz1, c.in0, c.A = "abwd", M, runs, 1, in0, A
    c.prec = 0 if f32 else 1
    c.C = bound(c.prec)
    c.family = family
    c.groups = M // 32
    rng = np.random.RandomState(9000 + seed)
    xp = in0 if x_pitch is None else x_pitch
    arrays, d = {}, {}

    def arr(name, rows, cols, data=None, result=False, pitch=None, nslab=1, dtype=np.float32, nz1=1, **kw):
        a = Arr(rows, cols, runs, nz1, nslab=nslab, pitch=pitch, off=(off or {}).get(name, 0), result=result, dtype=dtype, **kw)
        if data is not None:
            d[name] = np.asarray(data, dtype=dtype).reshape(runs, nz1, rows, cols)
            a.put(d[name])
        arrays[name] = a
        return a

    R = (runs, 1)
    arr("X", M, in0, rng.standard_normal(R + (M, in0)), pitch=xp)
    h0, h1 = np.maximum(rng.standard_normal(R + (M, N)), 0), np.maximum(rng.standard_normal(R + (M, N)), 0)
    h0[..., 5, :] = 0
    h1[..., 5, :] = 0
    arr("H0", M, N, h0)
    arr("H1", M, N, h1)
    head = np.concatenate([rng.standard_normal(R + (M, A)) * 0.5, rng.uniform(-4.0, 1.5, R + (M, A))], -1)
    head[..., 2, A], head[..., 3, A], head[..., 4, A] = -5.0, -6.0, np.nextafter(np.float32(-5.0), np.float32(-6.0))
    head[..., 7, 2 * A - 1], head[..., 8, 2 * A - 1], head[..., 9, 2 * A - 1] = 2.0, 3.0, np.nextafter(np.float32(2.0), np.float32(3.0))
    arr("head", M, 2 * A, head)
    eps = rng.standard_normal(R + (M, A)).astype(np.float32)
    arr("eps", M, A, eps)
    hd = as32(head)
    act = np.tanh(f64(hd[..., :A]) + np.exp(np.clip(f64(hd[..., A:]), -5, 2)) * eps)
    # xa: the actions sit at columns xa_col .. of rows of pitch xa_col + A + xa_pad; the tap is given the matrix's base
    xa = Arr(M, A, runs, 1, pitch=xa_col + A + xa_pad, off=(off or {}).get("xa", 0) + xa_col)
    xa.base = (off or {}).get("xa", 0)
    d["xa"] = as32(np.clip(act, -0.995, 0.995)).reshape(runs, 1, M, A)
    xa.put(d["xa"])
    xa.desc = lambda: OrlGemmBuf(xa.raw.ctypes.data, xa.n, xa.base, xa.pitch, xa.s0, xa.s1, xa.kstride)
    arrays["xa"] = xa
    arr("logp", M, 1, rng.standard_normal(R + (M, 1)) - 1.0)
    qa = rng.standard_normal((runs, 2, M, 1)).astype(np.float32)
    qa[:, 1, 1] = qa[:, 0, 1]                                      # row 1: an exact tie
    qa[:, 1, 2] = qa[:, 0, 2] - 0.5                                # row 2: q1 < q0
    qa[:, 1, 6] = qa[:, 0, 6] + 0.5                                # row 6: q0 < q1
    arr("qa", M, 1, qa, nz1=2)
    arr("ga", M, A, rng.standard_normal((runs, 2, M, A)), pitch=A + ga_pad, nz1=2)
    arr("W1", N, N, _weights(rng, *R, N, N))
    arr("Wh", 2 * A, N, _weights(rng, *R, 2 * A, N))
    offs, o_ks = slab_layout(in0, A)
    c.offs, c.o_ks = offs, o_ks
    out = Arr(1, o_ks, runs, 1, nslab=c.groups + 1, kstride=o_ks, guard=0, result=True, off=(off or {}).get("out", 0))
    arrays["out"] = out
    sc = rng.standard_normal((runs, 1, 1, 16)).astype(np.float32)
    for r in range(runs):
        la = log_alpha + 0.1 * r
        sc[r, 0, 0, SC["log_alpha"]] = la
        sc[r, 0, 0, SC["alpha"]] = np.exp(np.float32(la))
        sc[r, 0, 0, SC["la_m"]] = 0.0 if gstep == 0 else 0.3 - 0.2 * r
        sc[r, 0, 0, SC["la_v"]] = 0.0 if gstep == 0 else 0.05 + 0.01 * r
    nm = 5
    c.nm, c.m_actor, c.m_alpha_loss, c.m_alpha = nm, 3, 0, 4
    for name, rows, cols, data in (("sc", 1, 16, sc), ("metrics_last", 1, nm, 7.0 + np.arange(runs * nm)), ("metrics_sum", 1, nm, 100.0 + np.arange(runs * nm)),
                                   ("part", MAXGROUPS, 2, None), ("ticket", 1, 1, None)):
        a = Arr(rows, cols, runs, 1, guard=0, result=True, kstride=rows * cols, dtype=np.uint32 if name == "ticket" else np.float32, off=(off or {}).get(name, 0))
        assert a.s0 == rows * cols
        if data is not None:
            d[name] = as32(data).reshape(runs, 1, rows, cols)
            a.put(d[name])
        arrays[name] = a
    arrays["ticket"].put(np.zeros((runs, 1, 1, 1), np.uint32))
    hy = Arr(1, 8, 1, 1)
    d["hy"] = as32([1e-3, 2e-3, 3e-4, 4e-3, 5e-3, 6e-3, 7e-3, 8e-3])
    hy.put(d["hy"])
    arrays["hy"] = hy
    gs = Arr(1, 2, 1, 1, dtype=np.uint32)
    gs.put(np.array([gstep & 0xFFFFFFFF, gstep >> 32], np.uint32))
    arrays["gstep"] = gs
    c.gstep = gstep
    c.hyper = dict(auto_alpha=auto_alpha, clamp_alpha01=clamp_alpha01, fixed_alpha=0.2, target_entropy=-float(A), adam_b1=0.9, adam_b2=0.999, adam_eps=1e-8)
    for name, cut in (short or {}).items():
        arrays[name].n = int(arrays[name].idx.max()) + 1 - cut
    c.ints = dict(M=M, nz0=runs, nz1=1, f32=f32, in0=in0, A=A, K=2, xa_col=xa_col, nm=nm, m_actor=c.m_actor, m_alpha_loss=c.m_alpha_loss, m_alpha=c.m_alpha,
                  off_w0=offs["w0"], off_b0=offs["b0"], off_w1=offs["w1"], off_b1=offs["b1"], off_wh=offs["wh"], off_bh=offs["bh"], **c.hyper)
    c.ints.update(ints or {})
    c.arrays, c.d = arrays, d
    c.before = {k: a.raw.copy() for k, a in arrays.items()}
    c.per_z, c.kw = 0, {"l0": False}
    return c


def abwd_alpha(c, r):
    """the alpha run r's backward uses, as the float32 the kernel reads"""
    return np.float32(c.d["sc"][r, 0, 0, SC["alpha"]]) if c.hyper["auto_alpha"] else np.float32(c.hyper["fixed_alpha"])


def abwd_dhead(c, r, dt=np.float64):
    d, M = c.d, c.M
    dh, dha = ref_dhead(d["qa"][r, 0, :, 0], d["qa"][r, 1, :, 0], d["ga"][r, 0], d["ga"][r, 1], d["head"][r, 0][:, c.A:], d["eps"][r, 0], d["xa"][r, 0],
                        abwd_alpha(c, r), M)
    return dh, dha


def slab_view(c, r, g, k, out=None):
    """tensor k of slab g of run r, as stored (out: c.arrays["out"].get(), when the caller walks many slabs)"""
    s = (c.arrays["out"].get() if out is None else out)[r, 0, g, 0]
    v = s[c.offs[k]:c.offs[k] + slab_len(k, c.in0, c.A)]
    return v.reshape({"w0": (N, c.in0), "w1": (N, N), "wh": (2 * c.A, N)}.get(k, (-1,)))


def check_abwd_guards(c):
    """ws_cases.check_guards (words outside the logical arrays, operands bit-identical) + inside the slabs: the gaps between the six
    tensors, head rows >= 2A and the slabs >= groups keep the sentinel; part slots >= groups too"""
    check_guards(c)
    raw = c.arrays["out"].raw
    idx = c.arrays["out"].idx      # [runs][1][groups + 1][1][o_ks]
    written = np.zeros(c.o_ks, dtype=bool)
    for k in STAGES:
        written[c.offs[k]:c.offs[k] + slab_len(k, c.in0, c.A)] = True
    assert np.all(raw[idx[:, 0, :c.groups, 0][..., ~written]] == GEMM_SENTINEL), "a word between the tensors of a slab (or a head row >= 2A) was written"
    assert np.all(raw[idx[:, 0, c.groups:]] == GEMM_SENTINEL), "a slab >= groups was written"
    assert np.all(raw[idx[:, 0, :c.groups, 0][..., written]] != GEMM_SENTINEL), "a word of a slab's tensors was left unwritten"
    p = c.arrays["part"]
    assert np.all(p.raw[p.idx[:, 0, 0, c.groups:]] == GEMM_SENTINEL), "a part slot >= groups was written"
    assert np.all(c.arrays["ticket"].get() == 0), "the ticket is not back at 0"


def check_abwd(c):
    """asserts a small_abwd launch against float64, the guard words and the scalars"""
    check_abwd_guards(c)
    w = Worst(c)
    d, C, M, A, in0 = c.d, c.C, c.M, c.A, c.in0
    C32 = bound(0)      # the loss sums, metrics and dhead run in fp32 in both precisions
    out = c.arrays["out"].get()
    for r in range(c.nz0):
        alpha = abwd_alpha(c, r)
        dh, dha = abwd_dhead(c, r)
        x, h0, h1, wh, w1 = d["X"][r, 0], d["H0"][r, 0], d["H1"][r, 0], d["Wh"][r, 0], d["W1"][r, 0]
        for g in range(c.groups):
            rows = slice(32 * g, 32 * g + 32)
            ref = ref_abwd_group(dh[rows], h1[rows], h0[rows], x[rows], wh, w1)
            ra = ref_abwd_group_abs(dha[rows], h1[rows], h0[rows], x[rows], wh, w1)
            for k, st in STAGES.items():
                cc = C32 if k == "bh" else C      # dhead and its column sums are fp32 VALU work in both precisions
                got = slab_view(c, r, g, k, out)
                w.add(f"{k} slab {g} run {r}", got, ref[k].reshape(got.shape), st * cc * ra[k].reshape(got.shape))
        # loss partials, metrics
        q0, q1, lp = f64(d["qa"][r, 0, :, 0]), f64(d["qa"][r, 1, :, 0]), f64(d["logp"][r, 0, :, 0])
        terms, terms_a = float(alpha) * lp - np.minimum(q0, q1), abs(float(alpha)) * np.abs(lp) + np.abs(np.minimum(q0, q1))
        part = f64(c.arrays["part"].get()[r, 0, 0, :c.groups])
        w.add(f"part run {r}", part[:, 0], terms.reshape(c.groups, 32).sum(1), C32 * terms_a.reshape(c.groups, 32).sum(1))
        w.add(f"part run {r}", part[:, 1], lp.reshape(c.groups, 32).sum(1), C32 * np.abs(lp).reshape(c.groups, 32).sum(1))
        ml, ms = f64(c.arrays["metrics_last"].get()[r, 0, 0, 0]), f64(c.arrays["metrics_sum"].get()[r, 0, 0, 0])
        ml0, ms0 = f64(d["metrics_last"][r, 0, 0]), f64(d["metrics_sum"][r, 0, 0])
        loss, loss_a = part[:, 0].sum() / M, np.abs(part[:, 0]).sum() / M
        w.add(f"metric actor run {r}", ml[c.m_actor], loss, C32 * loss_a)
        w.add(f"metric actor_sum run {r}", ms[c.m_actor], ms0[c.m_actor] + ml[c.m_actor], 2 * U24 * (abs(ms0[c.m_actor]) + abs(ml[c.m_actor])))
        # scalars
        sc_got, sc0 = c.arrays["sc"].get()[r, 0, 0, 0], d["sc"][r, 0, 0]
        changed = {SC["alpha_bwd"]} | ({SC["log_alpha"], SC["la_m"], SC["la_v"], SC["alpha"]} if c.hyper["auto_alpha"] else set())
        for i in range(16):
            if i not in changed:
                assert sc_got[i].view(np.uint32) == sc0[i].view(np.uint32), ("RunScalars field changed", i)
        assert sc_got[SC["alpha_bwd"]] == alpha, "alpha_bwd is not the alpha the backward used"
        free = [i for i in range(c.nm) if i != c.m_actor and not (c.hyper["auto_alpha"] and i in (c.m_alpha_loss, c.m_alpha))]
        assert np.array_equal(ml[free], ml0[free]) and np.array_equal(ms[free], ms0[free]), "a metric slot of another quantity was written"
        if c.hyper["auto_alpha"]:
            mean_t = part[:, 1].sum() / M + c.hyper["target_entropy"]
            mean_a = np.abs(part[:, 1]).sum() / M + abs(c.hyper["target_entropy"])
            la0 = float(sc0[SC["log_alpha"]])
            w.add(f"metric alpha_loss run {r}", ml[c.m_alpha_loss], -(la0 * mean_t), C32 * abs(la0) * mean_a)
            (p2, m2, v2), sums = ref_adam(sc0[SC["log_alpha"]], sc0[SC["la_m"]], sc0[SC["la_v"]], -mean_t, d["hy"][2], c.hyper["adam_b1"], c.hyper["adam_b2"],
                                          c.hyper["adam_eps"], c.gstep + 1)
            gerr = C32 * mean_a      # the gradient itself is one stage: its error moves m by (1 - b1) gerr, v by 2 (1 - b2) |g| gerr, p by at most lr / bc1 * (that, over sqrt v)
            sens_m = (1 - float(np.float32(c.hyper["adam_b1"]))) * gerr
            sens_v = 2 * (1 - float(np.float32(c.hyper["adam_b2"]))) * abs(mean_t) * gerr
            w.add(f"adam m run {r}", sc_got[SC["la_m"]], m2, ADAM_K * (U24 * sums[1] + sens_m))
            w.add(f"adam v run {r}", sc_got[SC["la_v"]], v2, ADAM_K * (U24 * sums[2] + sens_v))
            # p: evaluated from the kernel's own m and v (one elementwise formula on returned values)
            bc1, bc2 = 1.0 - float(np.float32(c.hyper["adam_b1"])) ** (c.gstep + 1), 1.0 - float(np.float32(c.hyper["adam_b2"])) ** (c.gstep + 1)
            upd = float(d["hy"][2]) / bc1 * (float(sc_got[SC["la_m"]]) / (np.sqrt(float(sc_got[SC["la_v"]])) / np.sqrt(bc2) + float(np.float32(c.hyper["adam_eps"]))))
            w.add(f"adam p run {r}", sc_got[SC["log_alpha"]], la0 - upd, ADAM_K * U24 * (abs(la0) + abs(upd)))
            na = np.exp(float(sc_got[SC["log_alpha"]]))
            if c.hyper["clamp_alpha01"]:
                na = min(max(na, 0.0), 1.0)
            w.add(f"adam alpha run {r}", sc_got[SC["alpha"]], na, ADAM_K * U24 * na)
            assert ml[c.m_alpha] == sc_got[SC["alpha"]], "the alpha metric is not the new alpha"
            w.add(f"metric alpha_sum run {r}", ms[c.m_alpha], ms0[c.m_alpha] + ml[c.m_alpha], 2 * U24 * (abs(ms0[c.m_alpha]) + abs(ml[c.m_alpha])))
            w.add(f"metric alpha_loss_sum run {r}", ms[c.m_alpha_loss], ms0[c.m_alpha_loss] + ml[c.m_alpha_loss], 2 * U24 * (abs(ms0[c.m_alpha_loss]) + abs(ml[c.m_alpha_loss])))
    return w.finish()


DEFECT = None      # test_small_paths_cpu.py plants "tie" (a tie split 1 / 0) or "clamp" (the clamp edges taken exclusive) into the emulation


def dhead32(c, r):
    """small_bwd.hip's dhead block operation by operation in float32 numpy"""
    d, M, A = c.d, c.M, c.A
    T = np.float32
    q0, q1 = d["qa"][r, 0, :, 0], d["qa"][r, 1, :, 0]
    g0, g1, ls, ep, act = d["ga"][r, 0], d["ga"][r, 1], d["head"][r, 0][:, A:], d["eps"][r, 0], d["xa"][r, 0]
    alpha = abwd_alpha(c, r)
    qmin = np.minimum(q0, q1)
    nmin = ((q0 == qmin).astype(T) + (q1 == qmin).astype(T))
    gq = T(-1.0) / T(M)
    c0, c1 = np.where(q0 == qmin, gq / nmin, T(0)), np.where(q1 == qmin, gq / nmin, T(0))
    if DEFECT == "tie":
        c0, c1 = np.where(q0 <= q1, gq, T(0)), np.where(q1 < q0, gq, T(0))
    da = c0[:, None] * g0 + c1[:, None] * g1
    dlogp = alpha / T(M)
    sg = np.exp(np.minimum(np.maximum(ls, T(-5)), T(2)))
    om = T(1) - act * act
    t = T(2) * act * om / (om + T(1e-6))
    du = da * om + dlogp * t
    dls = du * sg * ep - dlogp
    dl2 = np.where((ls > T(-5)) & (ls < T(2)) if DEFECT == "clamp" else (ls >= T(-5)) & (ls <= T(2)), dls, T(0))
    return np.concatenate([du, dl2], 1).astype(T)


def emulate_abwd(c):
    """what a correct kernel leaves in the result arrays, in float32 numpy (no device)"""
    run(c, dry_run=True)
    d, M, A = c.d, c.M, c.A
    T = np.float32
    out = c.arrays["out"]
    for r in range(c.nz0):
        alpha = abwd_alpha(c, r)
        dh = dhead32(c, r)
        x, h0, h1, wh, w1 = d["X"][r, 0], d["H0"][r, 0], d["H1"][r, 0], d["Wh"][r, 0], d["W1"][r, 0]
        lp, qmin = d["logp"][r, 0, :, 0], np.minimum(d["qa"][r, 0, :, 0], d["qa"][r, 1, :, 0])
        part = c.arrays["part"]
        for g in range(c.groups):
            rows = slice(32 * g, 32 * g + 32)
            dz1 = (h1[rows] > 0) * (dh[rows] @ wh)
            dz0 = (h0[rows] > 0) * (dz1 @ w1)
            vals = {"bh": dh[rows].sum(0, dtype=T), "wh": dh[rows].T @ h1[rows], "b1": dz1.sum(0, dtype=T), "w1": dz1.T @ h0[rows], "w0": dz0.T @ x[rows], "b0": dz0.sum(0, dtype=T)}
            for k, v in vals.items():
                base = out.idx[r, 0, g, 0, c.offs[k]]
                out.raw.view(T)[base:base + v.size] = as32(v).ravel()
            part.raw.view(T)[part.idx[r, 0, 0, g]] = [(alpha * lp[rows] - qmin[rows]).sum(dtype=T), lp[rows].sum(dtype=T)]
        ps = part.get()[r, 0, 0, :c.groups]
        tl, tp = ps[:, 0].sum(dtype=T), ps[:, 1].sum(dtype=T)
        sc, ml, ms = c.arrays["sc"], c.arrays["metrics_last"], c.arrays["metrics_sum"]
        scv, mlv, msv = sc.get().copy(), ml.get().copy(), ms.get().copy()
        loss = tl / T(M)
        mlv[r, 0, 0, 0, c.m_actor] = loss
        msv[r, 0, 0, 0, c.m_actor] += loss
        s = scv[r, 0, 0, 0]
        s[SC["alpha_bwd"]] = alpha
        if c.hyper["auto_alpha"]:
            mean_t = tp / T(M) + T(c.hyper["target_entropy"])
            aloss = -(s[SC["log_alpha"]] * mean_t)
            (p2, m2, v2), _ = ref_adam(s[SC["log_alpha"]], s[SC["la_m"]], s[SC["la_v"]], -mean_t, d["hy"][2], c.hyper["adam_b1"], c.hyper["adam_b2"],
                                       c.hyper["adam_eps"], c.gstep + 1, dt=np.float32)
            na = np.exp(T(p2))
            if c.hyper["clamp_alpha01"]:
                na = min(max(na, T(0)), T(1))
            s[SC["log_alpha"]], s[SC["la_m"]], s[SC["la_v"]], s[SC["alpha"]] = p2, m2, v2, na
            mlv[r, 0, 0, 0, c.m_alpha_loss] = aloss
            msv[r, 0, 0, 0, c.m_alpha_loss] += aloss
            mlv[r, 0, 0, 0, c.m_alpha] = na
            msv[r, 0, 0, 0, c.m_alpha] += na
        sc.put(scv), ml.put(mlv), ms.put(msv)
    return c


def check(c, **kw):
    return check_fwd(c, **kw) if c.kind == "fwd" else check_abwd(c)


def emulate(c):
    return emulate_fwd(c) if c.kind == "fwd" else emulate_abwd(c)


def build(kind="fwd", **kw):
    return build_fwd(**kw) if kind == "fwd" else build_abwd(**kw)


# =====================================================================================================================================
# case lists: (label, kwargs of build)
# =====================================================================================================================================
FLAVOURS = {
    "small_fwd<0,0>": dict(kind="fwd", f32=0, out_dim=12, A=6, jobs=[dict(head_row0=0, rows=64, rep=1)]),
    "small_fwd<1,0>": dict(kind="fwd", f32=1, out_dim=12, A=6, jobs=[dict(head_row0=0, rows=64, rep=1)]),
    "small_fwd<0,1>": dict(kind="fwd", f32=0, out_dim=1, in0=23, gn=6, gc0=17),
    "small_fwd<1,1>": dict(kind="fwd", f32=1, out_dim=1, in0=23, gn=6, gc0=17),
    "small_abwd<0>": dict(kind="abwd", f32=0),
    "small_abwd<1>": dict(kind="abwd", f32=1),
}


def fwd_geometry_cases():
    out = []
    for M in (32, 64, 96):
        for f in (0, 1):
            out.append((f"M {M} f32 {f}", dict(M=M, f32=f, seed=M)))
    for in0 in (1, 2, 14, 23, 31):
        for xp in (in0, 32):
            for f in (0, 1):
                out.append((f"in0 {in0} x_pitch {xp} f32 {f}", dict(in0=in0, x_pitch=xp, out_dim=2, f32=f, seed=100 + in0, family="in0 small" if in0 <= 2 else "base")))
    for od in (1, 2, 5, 12, 16):
        for f in (0, 1):
            out.append((f"out_dim {od} f32 {f}", dict(out_dim=od, in0=23, f32=f, seed=200 + od)))
    for od in (1, 5, 16):
        for f in (0, 1):
            out.append((f"Wt off by one float out_dim {od} f32 {f}", dict(out_dim=od, f32=f, off={"Wt": 1}, seed=300 + od)))
    for od in (1, 12):
        for f in (0, 1):
            out.append((f"3 x 2 problems, wide strides out_dim {od} f32 {f}", dict(out_dim=od, nz0=3, nz1=2, wide=True, f32=f, seed=400 + od)))
    return out


def qg_cases():
    out = []
    for gn in (1, 3, 6, 8):
        for gc0 in (0, 23 - gn):
            for f in (0, 1):
                out.append((f"gn {gn} gc0 {gc0} f32 {f}", dict(out_dim=1, in0=23, gn=gn, gc0=gc0, g_pad=2, f32=f, seed=500 + gn)))
    out.append(("QG 3 x 2 problems, wide strides", dict(out_dim=1, in0=11, gn=3, gc0=8, nz0=3, nz1=2, wide=True, seed=520)))
    out.append(("QG in0 = gn = 1", dict(out_dim=1, in0=1, gn=1, gc0=0, f32=1, x_pitch=32, seed=521, family="in0 small")))
    return out


def _jobs(M, A, rep, n, h):
    """n jobs: job 0 draws from head rows h .. with `rep` repeats and ends in the middle of a head row's repeats (rep > 1); job 1 is
    deterministic (no eps) with one repeat more or less; job 2 writes no log-probability, into a destination with row / column offsets"""
    k = M - h
    jobs = [dict(head_row0=h, rows=k * rep - rep // 2, rep=rep, dst_pad=1)]
    if n > 1:
        rep1 = rep - 1 if rep > 1 else 2
        jobs.append(dict(head_row0=0, rows=(M // 2) * rep1 - rep1 // 3, rep=rep1, eps=False, dst_col=2))
    if n > 2:
        jobs.append(dict(head_row0=min(h, 32), rows=5 * rep + (1 if rep > 1 else 0), rep=rep, logp=False, dst_row0=3, dst_col=1, dst_pad=2))
    return jobs


def sample_cases():
    out = []
    i = 0
    for A in (1, 3, 6, 8):
        for rep in (1, 2, 3, 10, 15, 16):
            n, h = 1 + i % 3, (0, 32, 40)[(i // 3 + i) % 3]
            out.append((f"A {A} rep {rep} njobs {n} head_row0 {h}", dict(M=96, out_dim=2 * A, A=A, in0=11 + A, f32=i % 2, jobs=_jobs(96, A, rep, n, h), seed=600 + i)))
            i += 1
    for f in (0, 1):
        out.append((f"two runs f32 {f}", dict(M=64, nz0=2, wide=True, out_dim=6, A=3, f32=f, jobs=_jobs(64, 3, 3, 3, 40), seed=640)))
        # log sigma below -5, exactly -5, exactly 2, above 2, one ulp outside either end
        edges = {6: -7.0, 7: -5.0, 8: 2.0, 9: 3.0, 10: float(np.nextafter(np.float32(-5), np.float32(-6))), 11: float(np.nextafter(np.float32(2), np.float32(3)))}
        out.append((f"clamp edges f32 {f}", dict(M=32, out_dim=12, A=6, f32=f, fix=edges, jobs=_jobs(32, 6, 2, 2, 0), seed=650)))
        # |u| > 10: mu = +-12 with log sigma = -1 (sigma |eps| < 2 on these seeds)
        out.append((f"saturated f32 {f}", dict(M=32, out_dim=6, A=3, f32=f, fix={0: 12.0, 1: -12.0, 3: -1.0, 4: -1.0}, jobs=[dict(head_row0=0, rows=64, rep=2)], seed=660,
                                             family="saturated")))
    return out


def abwd_cases():
    out = []
    for M in (32, 64, 96):
        for runs in (1, 3):
            for f in (0, 1):
                out.append((f"M {M} runs {runs} f32 {f}", dict(M=M, runs=runs, f32=f, seed=M + runs)))
    i = 0
    for A in (1, 3, 6, 8):
        for in0 in (1, 11, 17, 31):
            for xp in (in0, 32):
                out.append((f"A {A} in0 {in0} x_pitch {xp}", dict(M=64, A=A, in0=in0, x_pitch=xp, f32=(i // 2) % 2, seed=100 + i, runs=1 + (i % 4 == 3))))
                i += 1
    for f in (0, 1):
        out.append((f"fixed alpha f32 {f}", dict(auto_alpha=0, f32=f, seed=200)))
        out.append((f"clamp_alpha01 from exp(log_alpha) > 1 f32 {f}", dict(clamp_alpha01=1, log_alpha=0.5, f32=f, seed=201)))
        out.append((f"no clamp from exp(log_alpha) > 1 f32 {f}", dict(clamp_alpha01=0, log_alpha=0.5, f32=f, seed=201)))
        out.append((f"gstep 999 f32 {f}", dict(gstep=999, runs=3, f32=f, seed=202)))
        out.append((f"gstep 2^32 + 5 f32 {f}", dict(gstep=(1 << 32) + 5, f32=f, seed=203)))
    return out


def abwd_big_cases():
    return [("M 2048 (64 groups) f32 0", dict(M=2048, f32=0, seed=300)), ("M 2048 (64 groups) f32 1", dict(M=2048, f32=1, seed=301))]
