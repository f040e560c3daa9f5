"""Self-bounding float64 restatements of the engine's row kernels (csrc/kernels.h: sampling, loss, gradient-seed, head-backward and
optimizer kernels; then MCQ's VAE / critic-loss kernels and EDAC's gradient-diversity kernels; at the end of the file the supervised
heads -- RCSL, Gaussian RCSL, the autoregressive policy --, MOBILE's penalty and critic loss, and the dynamic power-of-two scale),
written from the formulas of the reference that the kernel comments cite -- not from the kernel code.

``BV`` is a float64 array that carries, element by element, a first-order bound on what fp32 arithmetic may lose when it evaluates
the same expression on the same fp32 operands (u = 2^-24, the unit roundoff of fp32):

    z = x op y :   e_z = |dz/dx| e_x + |dz/dy| e_y + u |z|          one correctly rounded operation (+ 2^-126 where the result
                                                                     can underflow: products, quotients, library calls)
    z = f(x)   :   e_z = |f'(x)| e_x + 2 u |z|                       a library call (exp, log, tanh, sqrt: 1 .. 2 ulp)
    z = sum x_i:   e_z = sum e_i + ceil(log2 n + n / 256 + 2) u sum |x_i|     n terms, a 256-thread strided loop followed by a tree
                   e_z = sum e_i + (n - 1) u sum |x_i|                         n terms added one after the other by one thread

Operands read back from the engine are exact (e = 0); so are comparisons, selections, min / max / clip / abs (they round nothing and do
not expand an error).  The bound widens by itself where the function is ill-conditioned (``log(1 - a^2 + 1e-6)`` near saturation,
``u - mu`` when sigma * eps is tiny against mu), so no tolerance is chosen by hand anywhere.  Discontinuous choices (min routing,
clamp gates, ``diff > 0``) are taken on the fp32 operands, where float64 takes the same branch.

A caller holds a kernel to ``|got - ref.v| <= FACTOR * ref.e`` with FACTOR = 4: the second-order terms the first-order propagation
drops, the 1-to-2-ulp spread of the device library's expf / logf / tanhf beyond the 2u above, and fused against separate multiply-add.
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126      # smallest normal fp32: what a product, quotient or library call may lose absolutely when its result underflows
FACTOR = 4.0
f32 = np.float32
LOG_SQRT_2PI = float(f32(math.log(math.sqrt(2.0 * math.pi))))


class BV:
    """value + first-order fp32 error bound, both float64 arrays of one shape"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    # ---- construction ----
    @staticmethod
    def exact(x):
        """an fp32 operand (an engine read-back, a constant the kernel holds in fp32, a small integer): no error"""
        if isinstance(x, BV):
            return x
        a = np.asarray(x)
        if a.dtype != np.float32:
            a = a.astype(np.float32)          # a constant is what fp32 holds of it
        return BV(a.astype(np.float64))

    @property
    def shape(self):
        return self.v.shape

    def __getitem__(self, idx):
        return BV(self.v[idx], self.e[idx])

    def reshape(self, *shape):
        return BV(self.v.reshape(*shape), self.e.reshape(*shape))

    # ---- arithmetic ----
    def __add__(self, o):
        o = BV.exact(o)
        z = self.v + o.v
        return BV(z, self.e + o.e + U * np.abs(z))

    __radd__ = __add__

    def __sub__(self, o):
        o = BV.exact(o)
        z = self.v - o.v
        return BV(z, self.e + o.e + U * np.abs(z))

    def __rsub__(self, o):
        return BV.exact(o) - self

    def __mul__(self, o):
        o = BV.exact(o)
        z = self.v * o.v
        return BV(z, np.abs(o.v) * self.e + np.abs(self.v) * o.e + U * np.abs(z) + TINY)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = BV.exact(o)
        z = self.v / o.v
        return BV(z, self.e / np.abs(o.v) + np.abs(z) * o.e / np.abs(o.v) + U * np.abs(z) + TINY)

    def __rtruediv__(self, o):
        return BV.exact(o) / self

    def __neg__(self):
        return BV(-self.v, self.e)


def _lib(z, de):
    return BV(z, de + 2.0 * U * np.abs(z) + TINY)


def exp(x):
    x = BV.exact(x)
    z = np.exp(x.v)
    return _lib(z, z * x.e)


def log(x):
    x = BV.exact(x)
    return _lib(np.log(x.v), x.e / np.abs(x.v))


def tanh(x):
    x = BV.exact(x)
    z = np.tanh(x.v)
    return _lib(z, (1.0 - z * z) * x.e)


def sqrt(x):
    x = BV.exact(x)
    z = np.sqrt(x.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(z > 0, x.e / (2.0 * np.where(z > 0, z, 1.0)), np.sqrt(x.e))      # sqrt(0 +- e) <= sqrt(e)
    return _lib(z, d)


def abs_(x):
    x = BV.exact(x)
    return BV(np.abs(x.v), x.e)


def _select(x, y, x_wins):
    """min / max: the operand whose whole interval (FACTOR x its bound) lies on the winning side is the result, with its own bound; where
    the intervals overlap either may win in fp32 and the result is within the larger bound of the float64 choice"""
    xv, yv, xe, ye = np.broadcast_arrays(x.v, y.v, x.e, y.e)
    sure_x = x_wins(xv + FACTOR * xe, yv - FACTOR * ye) & x_wins(xv - FACTOR * xe, yv + FACTOR * ye)
    sure_y = x_wins(yv + FACTOR * ye, xv - FACTOR * xe) & x_wins(yv - FACTOR * ye, xv + FACTOR * xe) & ~sure_x
    pick_x = x_wins(xv, yv) | (xv == yv)
    return BV(np.where(pick_x, xv, yv), np.where(sure_x, xe, np.where(sure_y, ye, np.maximum(xe, ye))))


def minimum(x, y):
    return _select(BV.exact(x), BV.exact(y), lambda a, b: a < b)


def maximum(x, y):
    return _select(BV.exact(x), BV.exact(y), lambda a, b: a > b)


def clip(x, lo, hi):
    return maximum(minimum(x, hi), lo)


def where(cond, x, y):
    x, y = BV.exact(x), BV.exact(y)
    cond = np.asarray(cond, bool)
    return BV(np.where(cond, x.v, y.v), np.where(cond, x.e, y.e))


def sum_terms(n):
    """rounding steps of an n-term sum by a 256-thread strided loop followed by a tree (wave shuffles, then the four wave sums)"""
    return float(math.ceil(math.log2(max(n, 1)) + n / 256.0 + 2.0))


def wave_terms(n):
    """rounding steps of an n-term sum by ONE wave: a 64-lane strided loop (ceil(n / 64) additions per lane), then the 6-step shuffle tree"""
    return float(math.ceil(max(n, 1) / 64.0) + 6)


def sum_(x, axis=None, sequential=False, stride=256):
    """sum over ``axis``; ``sequential``: one thread adds the terms one after the other (loops over the action or member index);
    ``stride`` 64: one wave's strided loop and shuffle tree (``wave_terms``) instead of a 256-thread block's (``sum_terms``)"""
    x = BV.exact(x)
    n = x.v.size if axis is None else x.v.shape[axis]
    assert stride in (64, 256), stride
    k = float(max(n - 1, 0)) if sequential else (wave_terms(n) if stride == 64 else sum_terms(n))
    return BV(x.v.sum(axis=axis), x.e.sum(axis=axis) + k * U * np.abs(x.v).sum(axis=axis))


def stack(xs, axis=0):
    xs = [BV.exact(x) for x in xs]
    return BV(np.stack([x.v for x in xs], axis), np.stack([x.e for x in xs], axis))


def ratio(got, ref):
    """worst |got - ref.v| / ref.e over every element (0 where both the error and the bound are 0; inf where only the bound is, or where
    the kernel's value is not finite)"""
    got = np.asarray(got, np.float64).reshape(ref.v.shape)
    err = np.abs(got - ref.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / ref.e)
    r = np.where(np.isfinite(got) & np.isfinite(ref.v) & ~np.isnan(r), r, np.inf)
    return float(r.max()) if r.size else 0.0


def holds(got, ref, tag, worst=None, key=None):
    """assert |got - ref| <= FACTOR * bound on every element; records the worst err / bound under ``key`` in ``worst``"""
    r = ratio(got, ref)
    if worst is not None:
        k = key or (tag[0] if isinstance(tag, tuple) else str(tag))
        worst[k] = max(worst.get(k, 0.0), r)
    assert r <= FACTOR, (tag, "err / bound", r)
    return r


# =====================================================================================================================================
# the restatements.  Arrays are fp32 engine read-backs (exact) unless said otherwise; scalars such as B enter as exact integers.
# =====================================================================================================================================

SIGMA_MIN, SIGMA_MAX, TANH_EPS = -5.0, 2.0, 1e-6


def tanh_sample(mu, ls_raw, eps, act=None):
    """TanhDiagGaussian.forward + TanhNormalWrapper.rsample / log_prob (dist_module.py:117-127, :17-42) for rows of (mu, log-std, eps):
    a = tanh(mu + sigma eps), logp = sum_a [log N(u; mu, sigma) - log(1 - a^2 + 1e-6)].  ``act``: the fp32 actions the kernel stored --
    the Jacobian term is then taken at them (the kernel computes it from the value it stores), which keeps the bound of logp from being
    dominated by the conditioning of 1 - tanh(u)^2 in u.  Returns (a [rows, A], logp [rows])."""
    mu, eps = BV.exact(mu), BV.exact(eps)
    ls = clip(ls_raw, SIGMA_MIN, SIGMA_MAX)
    sg = exp(ls)
    u = mu + sg * eps
    a = tanh(u)
    d = u - mu
    a_j = BV.exact(act) if act is not None else a
    term = (-(d * d) / (2.0 * (sg * sg)) - ls - LOG_SQRT_2PI) - log((1.0 - a_j * a_j) + TANH_EPS)
    return a, sum_(term, axis=1)           # a tree over the 8 / 16 / 32 lanes of the row: sum_terms(A) >= log2(32)


def min_route(qa, B):
    """backward of the minimum over the K members (cql.py:93-98: torch.min(q1a, q2a), ties split evenly; edac.py:98: min over dim 0) for
    dL/dmin = -1/B: members that hold the minimum share it.  qa [K, B] fp32.  Returns (qmin [B], dqa BV [K, B])."""
    qa = np.asarray(qa, np.float32)
    qmin = qa.min(axis=0)
    at = qa == qmin[None]
    share = (BV.exact(-1.0) / float(B)) / at.sum(axis=0).astype(np.float64)
    return qmin, where(at, BV(np.broadcast_to(share.v, at.shape), np.broadcast_to(share.e, at.shape)), 0.0)


def actor_loss(qa, logp, alpha, B):
    """L = mean(alpha logp - min_k Q_k(s, a))  (cql.py:92-98, edac.py:96-102)"""
    qmin, dqa = min_route(qa, B)
    loss = sum_(BV.exact(alpha) * BV.exact(logp) - BV.exact(qmin)) / float(B)
    return loss, dqa


def alpha_step(logp, log_alpha, m, v, target_entropy, lr, b1, b2, eps, t, B, clamp01):
    """alpha_loss = -(log_alpha (logp + target_entropy)).mean(), one Adam step on log_alpha, alpha = exp(log_alpha) (cql.py:100-106;
    clamped to [0, 1] by edac.py:110).  Returns (alpha_loss, new log_alpha, new m, new v, new alpha)."""
    mean_t = sum_(BV.exact(logp)) / float(B) + target_entropy
    aloss = -(BV.exact(log_alpha) * mean_t)
    p, m, v = adam(log_alpha, m, v, -mean_t, lr, b1, b2, eps, t)
    na = exp(p)
    if clamp01:
        na = clip(na, 0.0, 1.0)
    return aloss, p, m, v, na


def head_bwd(da, head, eps, act, alpha, B):
    """backward of (a, logp) = actforward(obs) through the rsample path for dL/da = ``da`` and dL/dlogp = alpha / B (autograd of
    dist_module.py:17-42, :117-127; oracle/nn.py tanh_gauss_bwd).  ``act``: the stored fp32 actions.  Returns dhead [B, 2A] = (dmu | dls_raw)."""
    head = np.asarray(head, np.float32)
    A = head.shape[1] // 2
    lsr = head[:, A:]
    a = BV.exact(act)
    sg = exp(clip(lsr, SIGMA_MIN, SIGMA_MAX))
    dlogp = BV.exact(alpha) / float(B)
    om = 1.0 - a * a
    t = 2.0 * a * om / (om + TANH_EPS)
    du = BV.exact(da) * om + dlogp * t
    dls = du * sg * BV.exact(eps) - dlogp
    gate = (lsr >= f32(SIGMA_MIN)) & (lsr <= f32(SIGMA_MAX))
    dls = where(gate, dls, 0.0)
    return BV(np.concatenate([du.v, dls.v], axis=1), np.concatenate([du.e, dls.e], axis=1))


def action_grad(dxa, dqa=None):
    """dL/da = sum over the K critics of their input gradients [K, B, A] (weighted by dqa [K, B] where dxa holds unit-seed gradients)"""
    x = BV.exact(dxa)
    if dqa is not None:
        x = BV.exact(np.asarray(dqa, np.float32)[:, :, None]) * x
    return sum_(x, axis=0, sequential=True)


def td_target(qt, rew, term, gamma, rep=1, logp_next=None, alpha=None):
    """y = r + gamma (1 - d) (min_k max_n Qt_k(s', a'_n) - alpha logp(a'))   (cql.py:108-132, edac.py:112-131, td3bc.py:89-93).
    qt [Kt, B * rep] fp32."""
    qt = np.asarray(qt, np.float32)
    Kt = qt.shape[0]
    nq = BV.exact(qt.reshape(Kt, -1, rep).max(axis=2).min(axis=0))
    if logp_next is not None:
        nq = nq - BV.exact(alpha) * BV.exact(logp_next)
    return BV.exact(rew) + BV.exact(gamma) * (1.0 - BV.exact(term)) * nq


def td_loss(q, y, B):
    """per member: L_k = mean((q_k - y)^2), dq_k = 2 (q_k - y) / B.  q [K, B] fp32; y: the fp32 target the kernel stored.  Returns (L [K], dq [K, B])"""
    d = BV.exact(q) - BV.exact(y)
    return sum_(d * d, axis=1) / float(B), 2.0 * d / float(B)


def cql_loss(q, y, logp_pi, logp_npi, B, BN, A, Br, w, T, thr, cs, with_lagrange):
    """conservative loss of one critic (cql.py:137-190): q [B + 3 BN] fp32 = data | pi | next-pi | random rows, y [B] the stored target.
    cs: cql_alpha (exp(cql_log_alpha) clamped to [0, 1e6]) as a BV, or 1.  Returns (loss, raw = cons - thr, dq [B + 3 BN]).
    The kernel splits the BN rows over ceil(BN / 512) workgroups and adds their partial sums one after the other; that is not modelled
    separately: the workgroups' count - 1 further additions stay below the n / 256 term of ``sum_terms`` (each workgroup's strided loop
    makes at most a 1 / workgroups share of those trips)."""
    q = np.asarray(q, np.float32)
    T, w, cs = BV.exact(T), BV.exact(w), BV.exact(cs)
    log_rand = log(BV.exact(0.5 ** A))
    qd = BV.exact(q[:B])
    d = qd - BV.exact(y)
    td = sum_(d * d) / float(B)
    z = stack([(BV.exact(q[B:B + BN]) - BV.exact(logp_pi)) / T, (BV.exact(q[B + BN:B + 2 * BN]) - BV.exact(logp_npi)) / T,
               (BV.exact(q[B + 2 * BN:]) - log_rand) / T], axis=1)                       # [BN, 3]
    zmax = BV(z.v.max(axis=1, keepdims=True), z.e.max(axis=1, keepdims=True))
    ez = exp(z - zmax)
    se = sum_(ez, axis=1, sequential=True).reshape(-1, 1)
    lse = log(se) + zmax
    soft = ez / se
    cons = (sum_(lse.reshape(-1)) / float(BN)) * w * T - (sum_(qd[:Br]) / float(Br)) * w
    raw = cons - thr
    loss = td + (cs * raw if with_lagrange else cons)
    real = (np.arange(B) < Br)
    dq_data = 2.0 * d / float(B) - where(real, cs * w / float(Br), 0.0)
    dq_rows = (cs * w / float(BN)) * soft
    dq = BV(np.concatenate([dq_data.v, dq_rows.v[:, 0], dq_rows.v[:, 1], dq_rows.v[:, 2]]),
            np.concatenate([dq_data.e, dq_rows.e[:, 0], dq_rows.e[:, 1], dq_rows.e[:, 2]]))
    return loss, raw, dq


def cql_alpha(cql_log_alpha):
    """(exp(cql_log_alpha), its clamp to [0, 1e6], whether the clamp passes the gradient)  (cql.py:170-178)"""
    e = exp(BV.exact(cql_log_alpha))
    return e, clip(e, 0.0, 1e6), bool(0.0 <= float(e.v) <= 1e6)


def lagrange_step(raw1, raw2, cql_log_alpha, m, v, lr, b1, b2, eps, t):
    """cql_alpha_loss = -(cql_alpha raw1 + cql_alpha raw2) / 2, one Adam step on cql_log_alpha (cql.py:170-178); the clamp gates the gradient"""
    e, cs, gate = cql_alpha(cql_log_alpha)
    loss = -(cs * raw1 + cs * raw2) * 0.5
    g = -(raw1 + raw2) * 0.5 * e if gate else BV.exact(0.0)
    p, m, v = adam(cql_log_alpha, m, v, g, lr, b1, b2, eps, t)
    return loss, cs, p, m, v


def iql_v_loss(qo, v, B, expectile):
    """iql.py:90-98, :82-84: diff = min(q1_old, q2_old) - v ; w = expectile if diff > 0 else 1 - expectile ; L = mean(w diff^2) ;
    dv = -2 w diff / B.  Returns (L, dv [B], qmin [B] exact)."""
    qo = np.asarray(qo, np.float32)
    qm = qo.min(axis=0)
    d = BV.exact(qm) - BV.exact(v)
    w = where(d.v > 0, BV.exact(expectile), 1.0 - BV.exact(expectile))
    return sum_(w * d * d) / float(B), -2.0 * w * d / float(B), qm


def iql_q_loss(v2, qmin, rew, term, B, gamma, beta):
    """iql.py:100-116, :118-122: y = r + gamma (1 - d) V(s') ; dq_i = 2 (q_i - y) / B ; exp_a = min(exp((min q_old - V(s)) beta), 100).
    v2 [2B] fp32: V(s) rows, then V(s') rows.  Returns (y [B], exp_a [B]); the losses and dq are ``td_loss`` on the stored y."""
    v2 = np.asarray(v2, np.float32)
    y = BV.exact(rew) + BV.exact(gamma) * (1.0 - BV.exact(term)) * BV.exact(v2[B:])
    return y, minimum(exp((BV.exact(qmin) - BV.exact(v2[:B])) * BV.exact(beta)), 100.0)


def iql_actor_loss(mraw, act, exp_a, sigma_param, B):
    """iql.py:118-131 with DiagGaussian(unbounded = False, conditioned_sigma = False) (dist_module.py:59-84): mu = tanh(m_raw),
    sigma = exp(sigma_param) ; L = -mean(exp_a logp(a_data)).  Returns (L, dmraw [B, A], g_sigma [A])."""
    mu = tanh(BV.exact(mraw))
    ls = BV.exact(np.asarray(sigma_param, np.float32).reshape(1, -1))
    sg = exp(ls)
    var = sg * sg
    d = BV.exact(act) - mu
    lp = sum_(-(d * d) / (2.0 * var) - ls - LOG_SQRT_2PI, axis=1, sequential=True)
    ea = BV.exact(exp_a)
    loss = -(sum_(ea * lp) / float(B))
    dlogp = (-ea / float(B)).reshape(-1, 1)
    dmraw = dlogp * d / var * (1.0 - mu * mu)
    g_sigma = sum_(dlogp * (d * d / var - 1.0), axis=0)
    return loss, dmraw, g_sigma


def det_action(mraw, max_action, eps=None, policy_noise=0.0, noise_clip=0.0):
    """td3bc.py:89-93 / td3.py: a = max_action tanh(m_raw) ; with target-policy noise: clamp(a + clamp(eps policy_noise, +-noise_clip), +-max_action)"""
    v = BV.exact(max_action) * tanh(BV.exact(mraw))
    if eps is not None:
        nz = clip(BV.exact(eps) * BV.exact(policy_noise), -noise_clip, noise_clip)
        v = clip(v + nz, -max_action, max_action)
    return v


def td3_actor_loss(q, a_pi, act, alpha, B, A):
    """td3bc.py:106-112: lambda = alpha / mean |q| ; L = -lambda mean(q) + mean((pi(s) - a)^2) ; dq = -lambda / B.  Returns (L, dq scalar)"""
    q = BV.exact(q)
    lm = BV.exact(alpha) / (sum_(abs_(q)) / float(B))
    d = BV.exact(a_pi) - BV.exact(act)
    loss = -lm * (sum_(q) / float(B)) + sum_((d * d).reshape(-1)) / float(B * A)
    return loss, -lm / float(B)


def td3_actor_bwd(dxa, a_pi, act, max_action, B, A):
    """d m_raw = (dQ/da + 2 (pi(s) - a) / (B A)) max_action (1 - tanh^2), tanh = pi(s) / max_action (autograd of td3bc.py:106-112)"""
    ap = BV.exact(a_pi)
    da = BV.exact(dxa) + 2.0 * (ap - BV.exact(act)) / float(B * A)
    th = ap / BV.exact(max_action)
    return da * BV.exact(max_action) * (1.0 - th * th)


def adam_consts(lr, b1, b2, t, torch_scalars=False):
    """the scalars of one Adam step as the tensors meet them: step_size = lr / (1 - b1^t) and sqrt(1 - b2^t) (doubles rounded to fp32
    once), the lerp weight 1 - b1, the decay b2 and the weight 1 - b2.
    The engine's configuration carries lr and the betas as fp32 numbers, and its Adam is Adam for THOSE betas: 1 - b is exact there
    (Sterbenz), the bias corrections use the widened fp32 betas.  ``torch_scalars``: torch.optim.Adam with Python-double
    hyper-parameters instead, each rounded to fp32 where it meets a tensor (1 - 0.999 -> fp32(0.001), which is 1.3e-5 relative above
    1 - fp32(0.999): the two Adams differ by that much in exp_avg_sq, far inside the engine's 1e-4 gates but far outside rounding)."""
    if torch_scalars:
        lr_, b1_, b2_ = float(lr), float(b1), float(b2)
        w1, w2 = BV.exact(1.0 - b1_), BV.exact(1.0 - b2_)
    else:
        lr_, b1_, b2_ = float(f32(lr)), float(f32(b1)), float(f32(b2))
        w1, w2 = BV(1.0 - b1_), BV(1.0 - b2_)
    step = lr_ / (1.0 - b1_ ** t)
    bc2s = math.sqrt(1.0 - b2_ ** t)
    return dict(step=BV(step, U * abs(step)), bc2s=BV(bc2s, U * abs(bc2s)), w1=w1, b2=BV.exact(b2_), w2=w2)


def adam(p, m, v, g, lr, b1, b2, eps, t, tau=None, target=None, torch_scalars=False):
    """torch.optim.Adam, single-tensor path, defaults (exp_avg.lerp_, mul_ + addcmul_, addcdiv_ with step_size = lr / (1 - b1^t) and
    denom = sqrt(v) / sqrt(1 - b2^t) + eps), then the Polyak sync target = target (1 - tau) + p tau (sac.py:60-64).
    Returns (p, m, v[, target])."""
    c = adam_consts(lr, b1, b2, t, torch_scalars)
    p, m, v, g = BV.exact(p), BV.exact(m), BV.exact(v), BV.exact(g)
    m = m + (g - m) * c["w1"]
    v = v * c["b2"] + c["w2"] * g * g
    p = p - c["step"] * (m / (sqrt(v) / c["bc2s"] + BV.exact(eps)))
    if target is None:
        return p, m, v
    tau = BV.exact(tau)
    return p, m, v, BV.exact(target) * (1.0 - tau) + p * tau


# =====================================================================================================================================
# MCQ (policy/model_free/mcq.py:48-126; behaviour policy nets/vae.py:36-58) and EDAC's gradient-diversity term (edac.py:136-149)
# =====================================================================================================================================
VAE_LS_MIN, VAE_LS_MAX, VAE_Z_CLIP = -4.0, 15.0, 0.5


def vae_latent(ehead, eps):
    """VAE.forward (vae.py:44-50): ehead [B, 2Z] = (mean | log-std), log-std clamped to [-4, 15] (on the fp32 operand: exact),
    std = exp(log-std), z = mean + std eps.  Returns (std [B, Z], z [B, Z])."""
    ehead = np.asarray(ehead, np.float32)
    Z = ehead.shape[1] // 2
    std = exp(clip(ehead[:, Z:], VAE_LS_MIN, VAE_LS_MAX))
    return std, BV.exact(ehead[:, :Z]) + std * BV.exact(eps)


def vae_loss(m3, act, ehead, std, max_action, B, A, Z):
    """mcq.py:53-56 on vae.py:51-53: u = max_action tanh(m3) ; L = mean((u - a)^2) - 0.5 mean(1 + log(std^2) - mean^2 - std^2) ;
    dL/dm3 = 2 (u - a) / (B A) max_action (1 - tanh^2).  ``std``: the fp32 values the latent kernel stored.  Both means are a
    256-strided sum over all B A (B Z) elements.  Returns (L, dm3 [B, A])."""
    th = tanh(BV.exact(m3))
    ma = BV.exact(max_action)
    d = ma * th - BV.exact(act)
    recon = sum_((d * d).reshape(-1)) / float(B * A)
    mean, sd = BV.exact(np.asarray(ehead, np.float32)[:, :Z]), BV.exact(std)
    kl = sum_((((1.0 + log(sd * sd)) - mean * mean) - sd * sd).reshape(-1)) / float(B * Z)
    dm3 = 2.0 * d / float(B * A) * ma * (1.0 - th * th)
    return recon - 0.5 * kl, dm3


def vae_head_bwd(dz, ehead, std, eps, B, Z):
    """autograd of vae.py:44-50 + the KL term of mcq.py:54 for dL/dz = ``dz``: d mean = dz + mean / (B Z) ;
    d log-std = dz std eps + (std^2 - 1) / (B Z), passed by the clamp where -4 <= raw <= 15 (BOTH ends included: torch.clamp's
    backward) and exactly 0 elsewhere.  Returns dehead [B, 2Z]."""
    ehead = np.asarray(ehead, np.float32)
    mean, lsr, sd = BV.exact(ehead[:, :Z]), ehead[:, Z:], BV.exact(std)
    dz = BV.exact(dz)
    dmean = dz + mean / float(B * Z)
    dls = dz * sd * BV.exact(eps) + (sd * sd - 1.0) / float(B * Z)
    dls = where((lsr >= f32(VAE_LS_MIN)) & (lsr <= f32(VAE_LS_MAX)), dls, 0.0)
    return BV(np.concatenate([dmean.v, dls.v], axis=1), np.concatenate([dmean.e, dls.e], axis=1))


def clamp_latent(z):
    """VAE.decode (vae.py:57-58): the drawn latent clamped to [-0.5, 0.5] -- exact"""
    return clip(z, -VAE_Z_CLIP, VAE_Z_CLIP)


def mcq_loss(q, qt, qto, rew, term, logp_next, alpha, gamma, lam, B, N, stored=None):
    """mcq.py:62-94.  q [2, 3B] fp32: the critics on the B data rows, then on the 2B rows ([s; s'], pi([s; s'])) ; qt [2, B]: the
    target critics on (s', a') ; qto [2, 2B N]: the target critics on the N decoded actions of each of the 2B states.
        y_in = r + gamma (1 - d) (min_c qt_c - alpha logp') ;  y_ood[j] = min_c max_n qto_c[j N + n]
        L_c = lam mean_B((q_c[:B] - y_in)^2) + (1 - lam) mean_2B((q_c[B:] - y_ood)^2) ;  dq_c accordingly.
    ``stored``: the fp32 (target_q, target_ood) the kernel stored -- the losses and dq are then taken at them, as the kernel does.
    Returns (y_in [B], y_ood [2B], dq [2, 3B], L [2])."""
    q, qt, qto = np.asarray(q, np.float32), np.asarray(qt, np.float32), np.asarray(qto, np.float32)
    nq = BV.exact(qt.min(axis=0)) - BV.exact(alpha) * BV.exact(logp_next)
    y_in = BV.exact(rew) + BV.exact(gamma) * (1.0 - BV.exact(term)) * nq
    y_ood = BV.exact(qto.reshape(2, 2 * B, N).max(axis=2).min(axis=0))
    ti, to = (y_in, y_ood) if stored is None else (BV.exact(stored[0]), BV.exact(stored[1]))
    lam = BV.exact(lam)
    d_in, d_ood = BV.exact(q[:, :B]) - ti.reshape(1, -1), BV.exact(q[:, B:]) - to.reshape(1, -1)
    loss = lam * (sum_(d_in * d_in, axis=1) / float(B)) + (1.0 - lam) * (sum_(d_ood * d_ood, axis=1) / float(2 * B))
    dq_in, dq_ood = lam * 2.0 * d_in / float(B), (1.0 - lam) * 2.0 * d_ood / float(2 * B)
    return y_in, y_ood, BV(np.concatenate([dq_in.v, dq_ood.v], axis=1), np.concatenate([dq_in.e, dq_ood.e], axis=1)), loss


def edac_gamma(g, eta, K, B):
    """edac.py:136-149 for g [K, B, A] = dQ_k / da: g^ = g / (|g| + 1e-10) ; L_g = mean_b sum_{i != j} <g^_i, g^_j> / (K - 1)
    (= |sum_k g^_k|^2 - sum_k |g^_k|^2 per row) ; gamma = d(eta L_g) / dg, whose projection term divides by |g| -- guarded where |g| is
    exactly 0 (autograd of sqrt at 0 would be NaN; the term it multiplies is 0 there).  Sums over the actions and the members are one
    thread's; the batch mean is a 256-strided sum.  Returns (gamma [K, B, A], eta L_g)."""
    g = BV.exact(g)
    A = g.shape[2]
    nrm = sqrt(sum_(g * g, axis=2, sequential=True)).reshape(K, B, 1)
    nk = nrm + 1e-10
    gh = g / nk
    S = sum_(gh, axis=0, sequential=True).reshape(1, B, A)
    gram_off = sum_((S * S).reshape(B, A), axis=1, sequential=True) - sum_(sum_(gh * gh, axis=2, sequential=True), axis=0, sequential=True)
    lg = BV.exact(eta) * (sum_(gram_off) / float(B)) / float(K - 1)
    c = (BV.exact(eta) * 2.0 / float((K - 1) * B)) * (S - gh)
    safe = where(nrm.v > 0, nrm, 1.0)
    gc = sum_(g * c, axis=2, sequential=True).reshape(K, B, 1)
    return c / nk - g * (gc / (nk * nk * safe)), lg


def edac_t0(gamma, w0_action_rows, mask):
    """first step of the adjoint sweep (oracle/edac.py: t_0 = (gamma W_0[action rows]) (.) m_0): gamma [K, B, A], the action rows of the
    ensemble's first layer [K, A, N0], mask [K, B, N0] = 1[h_0 > 0].  An A-term sum by one thread per element; exactly 0 where the mask is."""
    prod = BV.exact(np.asarray(gamma, np.float32)[:, :, :, None]) * BV.exact(np.asarray(w0_action_rows, np.float32)[:, None, :, :])
    return where(np.asarray(mask, bool), sum_(prod, axis=2, sequential=True), 0.0)


# =====================================================================================================================================
# the supervised heads -- RCSL (policy/rcsl/rcsl.py:123-151), Gaussian RCSL (rcsl_gauss.py:123-154 on dist_module.py:80-93), the
# autoregressive policy (policy/others/autoregressive.py:28-54, :64-96) -- and MOBILE (policy/model_based/mobile.py:130-167).
# ``valid`` (bool [B], default: every row): the rows of an ordered epoch's step that are no padding; every mean divides by
# valid rows x A, as the reference's partial last batch does.
# =====================================================================================================================================
RG_LO, RG_HI = -5.0, 2.0                  # DiagGaussian's sigma_min / sigma_max
LEAKY_SLOPE = 0.01                        # nn.LeakyReLU's default
HALF_LOG_2PI = float(f32(0.9189385332046727))
RG_HEAD = ("dist_net.mu.weight", "dist_net.mu.bias", "dist_net.sigma.weight", "dist_net.sigma.bias")      # the arena's order


def _valid(valid, B):
    return np.ones(B, bool) if valid is None else np.asarray(valid, bool).reshape(B)


def rcsl_loss(pred, act, valid=None):
    """rcsl.py:139-141: L = mean over (valid rows x A) of (pred - a)^2 ; dL/dpred = 2 (pred - a) / (valid rows x A), exactly 0 on a padding
    row.  pred, act [B, A] fp32.  Returns (L, dpred [B, A])."""
    pred = np.asarray(pred, np.float32)
    B, A = pred.shape
    v = _valid(valid, B)[:, None]
    cnt = float(int(v.sum()) * A)
    d = BV.exact(pred) - BV.exact(act)
    return sum_(where(v, d * d, 0.0).reshape(-1)) / cnt, where(v, 2.0 * d / cnt, 0.0)


def _chain(terms):
    """one thread's multiply-add chain over the last axis (``sequential`` sum of the products, the bias being the first term)"""
    return sum_(terms, axis=terms.v.ndim - 1, sequential=True)


def _affine(z, w, b):
    """z [B, K] fp32, w [A, K], b [A] -> b + z w^T [B, A]"""
    prod = BV.exact(np.asarray(z, np.float32)[:, None, :]) * BV.exact(np.asarray(w, np.float32)[None, :, :])
    bias = np.broadcast_to(np.asarray(b, np.float64).reshape(1, -1, 1), prod.v.shape[:2] + (1,))
    out = _chain(BV(np.concatenate([bias, prod.v], axis=2), np.concatenate([np.zeros_like(bias), prod.e], axis=2)))
    return BV(out.v, np.where((prod.v == 0).all(axis=2), 0.0, out.e))      # every product exactly 0 (a zeroed head): the bias itself, exact


def rcslg_head(z, act, head, valid=None, raw32=None, logvar32=None):
    """rcsl_gauss.py:139-146 on dist_module.py:80-93: mu = W_mu z + b_mu ; s = clamp(W_sigma z + b_sigma, -5, 2), read as a log-variance ;
    L = mean((mu - a)^2 e^-s) + mean(s) over valid rows x A ; and its autograd: dmu = 2 (mu - a) e^-s / cnt ; ds = (1 - (mu - a)^2 e^-s) / cnt
    where the clamp passes the gradient (-5 <= raw <= 2, BOTH ends included: torch.clamp's backward), exactly 0 elsewhere and on padding
    rows ; dz = dmu W_mu + ds W_sigma ; head gradients = sums over the rows (one thread adds them one after the other).
    The clamp's branch is the one fp32 took: ``raw32`` -- the fp32 pre-clamp values -- decides it where they are at hand (the CPU proof);
    the engine stores only the clamped value ``logvar32``: strictly inside (-5, 2) that IS the raw value and the gate is open; on an end
    the raw value was on or beyond it, and the gate is open only where the float64 raw value equals the end within its own bound (a
    constant head's raw value is its bias, with bound 0: the comparison is then exact).
    z, act [B, A] fp32 ; head: the four tensors by name.  Returns dict(mu, logvar, loss, dmu, ds, dz, grads{name: BV})."""
    z = np.asarray(z, np.float32)
    B, A = z.shape
    v = _valid(valid, B)[:, None]
    cnt = float(int(v.sum()) * A)
    w_mu, b_mu, w_sg, b_sg = (np.asarray(head[k], np.float32) for k in RG_HEAD)
    mu, raw = _affine(z, w_mu, b_mu), _affine(z, w_sg, b_sg)
    lo, hi = f32(RG_LO), f32(RG_HI)
    if raw32 is not None:
        r32 = np.asarray(raw32, np.float32).reshape(B, A)
        at_lo, at_hi, gate = r32 <= lo, r32 >= hi, (r32 >= lo) & (r32 <= hi)
    elif logvar32 is not None:
        s32 = np.asarray(logvar32, np.float32).reshape(B, A)
        at_lo, at_hi = s32 == lo, s32 == hi
        on_end = np.abs(raw.v - np.where(at_lo, RG_LO, RG_HI)) <= FACTOR * raw.e
        gate = ~(at_lo | at_hi) | on_end
    else:
        r32 = raw.v.astype(np.float32)
        at_lo, at_hi, gate = r32 <= lo, r32 >= hi, (r32 >= lo) & (r32 <= hi)
    s = where(at_lo, RG_LO, where(at_hi, RG_HI, raw))
    inv = BV.exact(1.0) / cnt
    d = mu - BV.exact(act)
    iv = exp(-s)
    q = d * d * iv
    loss = sum_(where(v, q + s, 0.0).reshape(-1)) * inv
    dmu = where(v, 2.0 * d * iv * inv, 0.0)
    ds = where(v & gate, (1.0 - q) * inv, 0.0)
    # dz[i, k] = sum_a W_mu[a, k] dmu[i, a] + W_sigma[a, k] ds[i, a]: 2 A products, one chain
    pm = dmu.reshape(B, 1, A) * BV.exact(w_mu.T[None])
    ps = ds.reshape(B, 1, A) * BV.exact(w_sg.T[None])
    dz = _chain(BV(np.stack([ps.v, pm.v], axis=3).reshape(B, A, 2 * A), np.stack([ps.e, pm.e], axis=3).reshape(B, A, 2 * A)))
    dz = where(v, dz, 0.0)                # (products with the exact zeros of a padding row add up to exactly 0)
    zb = BV.exact(z)
    grads = {}
    for name, g in zip(RG_HEAD, (dmu, dmu, ds, ds)):
        if name.endswith("weight"):
            t = g.reshape(B, A, 1) * zb.reshape(B, 1, A)                # [i, a, k]
            grads[name] = sum_(t, axis=0, sequential=True)
        else:
            grads[name] = sum_(g, axis=0, sequential=True)
    return dict(mu=mu, logvar=s, loss=loss, dmu=dmu, ds=ds, dz=dz, grads=grads, gate=gate)


def leaky(z):
    """nn.LeakyReLU(0.01) on fp32 operands: the branch is the operand's own sign, and exactly 0 takes the slope branch (torch: x > 0 ? x : 0.01 x).
    Returns (value, slope the backward multiplies by)."""
    z = np.asarray(z, np.float32)
    pos = z > 0
    return where(pos, BV.exact(z), BV.exact(LEAKY_SLOPE) * BV.exact(z)), where(pos, 1.0, BV.exact(LEAKY_SLOPE))


def autoreg_head(z, target, A, valid=None):
    """autoregressive.py:64-96 behind the net's last LeakyReLU: out = leaky(z_tail) = (mean, logstd) of expanded row m = j B + b ;
    L = mean over valid expanded rows of logstd + ((t - mean) e^-logstd)^2 / 2 + log(2 pi) / 2 ; dz_tail = dL/dout leaky'(z_tail).
    A padding batch row b invalidates its A expanded rows m = j B + b (m % B == b).  z [A B, 2], target [A B] fp32.
    Returns (out [M, 2], L, dz [M, 2])."""
    z = np.asarray(z, np.float32)
    M = z.shape[0]
    B = M // A
    v = np.tile(_valid(valid, B), A)
    inv = BV.exact(1.0) / float(int(v.sum()))
    out, slope = leaky(z)
    mean, ls = out[:, 0], out[:, 1]
    ist = exp(-ls)
    d = (BV.exact(target) - mean) * ist
    loss = sum_(where(v, ls + 0.5 * d * d + HALF_LOG_2PI, 0.0)) * inv
    g0 = where(v, -(d * ist) * inv * slope[:, 0], 0.0)
    g1 = where(v, (1.0 - d * d) * inv * slope[:, 1], 0.0)
    return out, loss, stack([g0, g1], axis=1)


def autoreg_draw(z, eps):
    """autoregressive.py:28-54, one pass: a_j = mean + e^logstd eps_j with (mean, logstd) = leaky(z_tail).  z [n, 2], eps [n] fp32."""
    out, _ = leaky(z)
    return out[:, 0] + exp(out[:, 1]) * BV.exact(eps)


def lcb_penalty(ql, B, S, E, real_rows):
    """compute_lcb (mobile.py:130-142) behind the target critics: ql [2, S E B] fp32 on the sample rows (s E + e) B + b.
    qmin = min(Q1, Q2) (exact) ; m[e, b] = mean over the S samples ; penalty[b] = the unbiased standard deviation of m over the E elites
    (torch.std), and the leading ``real_rows`` entries are 0 (mobile.py:154).  Returns (qmin [S E B] fp32, penalty [B])."""
    ql = np.asarray(ql, np.float32)
    qmin = ql.min(axis=0)
    m = sum_(BV.exact(qmin.reshape(S, E, B)), axis=0, sequential=True) / float(S)
    d = m - (sum_(m, axis=0, sequential=True) / float(E)).reshape(1, B)
    pen = sqrt(sum_(d * d, axis=0, sequential=True) / float(E - 1))
    return qmin, where(np.arange(B) < real_rows, 0.0, pen)


def mobile_td_loss(q, qt, rew, term, pen, gamma, pen_coef, B, logp_next=None, alpha=None, stored=None):
    """mobile.py:151-167: y = clamp((r - c pen) + gamma (1 - d) (min(Qt1, Qt2) [- alpha logp']), 0, None) ; ONE loss = mean over (2, B) of
    (q_c - y)^2, so dq_c = 2 (q_c - y) / (2 B).  ``stored``: the fp32 target the kernel stored -- loss and dq are then taken at it.
    q, qt [2, B] fp32.  Returns (y [B], L, dq [2, B])."""
    qt = np.asarray(qt, np.float32)
    nq = BV.exact(qt.min(axis=0))
    if logp_next is not None:
        nq = nq - BV.exact(alpha) * BV.exact(logp_next)
    y = maximum((BV.exact(rew) - BV.exact(pen_coef) * BV.exact(pen)) + BV.exact(gamma) * (1.0 - BV.exact(term)) * nq, 0.0)
    inv = BV.exact(1.0) / float(2 * B)
    d = BV.exact(q) - (y if stored is None else BV.exact(stored)).reshape(1, -1)
    return y, sum_(sum_(d * d, axis=1), sequential=True) * inv, 2.0 * d * inv


def pow2_scale(a):
    """the dynamic scale of a split-precision backward pass (csrc/kernels.h: 2^(3 - floor(log2 a)) for the seed's largest magnitude a, so
    that a * scale lands in [8, 16); 1 for 0 and for a non-finite a; the exponent is kept within +-100 so that the scale is an fp32
    number).  A power of two: exact, compared with ==."""
    a = float(np.float32(a))
    if not (a > 0.0) or not (a < 3.0e38):
        return 1.0
    e = math.frexp(a)[1] - 1                  # floor(log2 a), subnormals included
    return math.ldexp(1.0, 3 - max(-100, min(100, e)))
