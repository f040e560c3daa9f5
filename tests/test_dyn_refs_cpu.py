"""CPU: keeps tests/test_gpu_dyn_kernels.py honest.  On every case of tests/dyn_cases.py, with synthesised head operands in place of the
engine's read-backs:

(a) the VALUES of the float64 restatements (tests/dyn_refs.py) equal float64 torch autograd of the repository's own soft_clamp /
    EnsembleDynamicsModel loss, and of RAMBO's loss (the elite mixture's log-probability times the advantage plus the supervised NLL), through
    a head-only graph with ``out`` as the leaf; RAMBO's values also equal tests/rambo_oracle.py evaluated in float64.  Bar: 1e-12 relative
    (to the element, plus the magnitude that cancels in it where float64 itself cancels: 1 - sigmoid next to 1).
(b) the reference alone stays inside the bar: an fp32 evaluation of the same operations on the same operands (the numpy oracles dyn_oracle /
    rambo_oracle / mobile_oracle where they expose the result, their fp32 softplus pieces assembled in the kernels' summation order for
    the per-element results) holds err / bound <= 4 on every element of every case, value edges included.
(c) the checks have teeth: sixteen defects planted one at a time through the named seams of that fp32 evaluation each push err / bound
    above 4 on at least one case."""
import math
import zlib

import numpy as np
import pytest
import torch

import dyn_cases as dc
import dyn_oracle as orc
import dyn_refs as dr
import mobile_oracle as morc
import rambo_oracle as rorc
import row_refs as rr

F = np.float32
F64 = np.float64
LOG_SQRT_2PI = F(0.91893853320467274178)

DEFECTS = ("second_trip_dropped", "sum_over_B_rows", "scale_by_B", "gmax_gmin_swapped", "s1_for_s2", "softplus_branch_constant",
           "penalty_over_elites", "aleatoric_obs_dims_only", "pairwise_with_reward", "obs_added_to_reward", "sample_from_next_member",
           "adam_t_off_by_one", "adam_without_decay", "mixture_over_all_members", "pg_divided_by_all_rows", "rowlp_without_log_elites")


# =====================================================================================================================================
# the fp32 evaluation, with its seams
# =====================================================================================================================================
def e_softplus(y, defect):
    if defect == "softplus_branch_constant":
        return np.where(y > 20, F(math.log1p(math.exp(20.0))), np.log1p(np.exp(np.minimum(y, 20)))).astype(F)
    return orc._softplus(y)


def e_soft_clamp(raw, mx, mn, defect=None):
    y1 = (mx - raw).astype(F)
    l1 = (mx - e_softplus(y1, defect)).astype(F)
    y2 = (l1 - mn).astype(F)
    lv = (mn + e_softplus(y2, defect)).astype(F)
    s1 = orc._dsoftplus(y1)
    return lv, s1, (s1 if defect == "s1_for_s2" else orc._dsoftplus(y2))


def e_nll(out, t, mx, mn, rows, B, defect=None):
    D = out.shape[-1] // 2
    mean, raw = out[..., :D], out[..., D:]
    lv, s1, s2 = e_soft_clamp(raw, mx, mn, defect)
    inv = np.exp(-lv).astype(F)
    diff = (mean - t).astype(F)
    sq = (diff * diff * inv).astype(F)
    s = F(1) / (F(B if defect == "scale_by_B" else rows) * F(D))
    dlv = ((F(1) - sq) * s).astype(F)
    dl1 = (dlv * s2).astype(F)
    gmax, gmin = (dl1 * (F(1) - s1)).astype(F), (dlv * (F(1) - s2)).astype(F)
    if defect == "gmax_gmin_swapped":
        gmax, gmin = gmin, gmax
    return (F(2) * diff * inv * s).astype(F), (dl1 * s1).astype(F), (sq + lv).astype(F), gmax, gmin


def e_wave_sum(vals, defect=None):
    """[n, cols] fp32 -> [cols]: the 64-lane strided loop, then the xor shuffle tree"""
    n, cols = vals.shape
    trips = -(-n // 64)
    pad = np.zeros((trips * 64, cols), F)
    pad[:n] = vals
    acc = np.zeros((64, cols), F)
    for t in range(1 if defect == "second_trip_dropped" else trips):
        acc = (acc + pad[t * 64:(t + 1) * 64]).astype(F)
    o = 32
    while o:
        acc = (acc + acc[np.arange(64) ^ o]).astype(F)
        o >>= 1
    return acc[0]


def e_reduce(ws, rows, mx, mn, coef, defect=None):
    """ws: (lterm, gmax, gmin) workspaces [K, B, D] whose rows beyond ``rows`` hold an earlier minibatch's values"""
    take = ws[0].shape[1] if defect == "sum_over_B_rows" else rows
    D = ws[0].shape[-1]
    cs = [e_wave_sum(a[:, :take].reshape(-1, D), defect) for a in ws]
    ls = F(0)
    smax = smin = F(0)
    for d in range(D):
        ls, smax, smin = F(ls + cs[0][d]), F(smax + mx[d]), F(smin + mn[d])
    c = F(coef)
    return F(ls / (F(rows) * F(D)) + F(c * smax - c * smin)), (cs[1] + c).astype(F), (cs[2] - c).astype(F)


def e_decay(flat, wd):
    P = flat.size
    nblk = (P + 1023) // 1024
    w, s = np.zeros(nblk * 1024, F), np.zeros(nblk * 1024, F)
    w[:P], s[:P] = flat, wd
    w, s = w.reshape(-1, 4), s.reshape(-1, 4)[:, 0]
    q = np.zeros(w.shape[0], F)
    for j in range(4):
        q = (q + w[:, j] * w[:, j]).astype(F)
    q = (q * (F(0.5) * s)).astype(F)
    return np.array([e_wave_sum(b.reshape(4, 64).T).astype(F).sum(dtype=F) for b in q.reshape(nblk, 256)], F)


def e_adam(flat, m, v, G, wd, tr, lr, t, defect=None):
    """dyn_oracle.adam (the fp32 numpy torch.optim.Adam the fixtures are pinned to) on the trainable floats"""
    g = G if defect == "adam_without_decay" else (G + wd * flat).astype(F)
    st, opt = {"p": flat[tr].copy()}, {"t": (t if defect == "adam_t_off_by_one" else t - 1), ("m", "p"): m[tr].copy(), ("v", "p"): v[tr].copy()}
    orc.adam(st, {"p": g[tr]}, opt, lr)
    out = [flat.copy(), m.copy(), v.copy()]
    out[0][tr], out[1][tr], out[2][tr] = st["p"], opt[("m", "p")], opt[("v", "p")]
    return out


def e_head(out, obs, noise, midx, elites, mx, mn, mode, coef, defect=None):
    """ensemble_dynamics.py:45-80 in numpy: fp32 means and stds, the float64 sample and penalty rounded to fp32"""
    K, n, D = out.shape[0], out.shape[1], out.shape[2] // 2
    od = obs.shape[-1]
    mean = out[..., :D].copy()
    mean[..., :od] += obs[None]
    if defect == "obs_added_to_reward":
        mean[..., od] += obs[None, :, 0]
    std = np.sqrt(np.exp(e_soft_clamp(out[..., D:], mx, mn)[0]).astype(F)).astype(F)
    i = np.arange(n)
    mi = (midx + 1) % K if defect == "sample_from_next_member" else midx
    s = (mean[mi, i].astype(F64) + noise[mi, i].astype(F64) * std[mi, i].astype(F64)).astype(F)
    mem = np.asarray(elites) if defect == "penalty_over_elites" else np.arange(K)
    if mode == "aleatoric":
        sd = std[mem][..., :od] if defect == "aleatoric_obs_dims_only" else std[mem]
        pen = np.linalg.norm(sd.astype(F64), axis=2).max(0)
    else:
        mo = mean[mem] if defect == "pairwise_with_reward" and mode == "pairwise-diff" else mean[mem][..., :od]
        mb = mo.astype(F64).mean(0).astype(F)
        if mode == "pairwise-diff":
            pen = np.linalg.norm((mo - mb[None]).astype(F).astype(F64), axis=2).max(0)
        else:
            pen = np.sqrt(((mo.astype(F64) - mb.astype(F64)[None]) ** 2).mean(0).mean(1))
    pen = pen.astype(F)
    raw = s[:, od]
    return s[:, :od], raw, pen, (raw - (F(coef) * pen).astype(F)).astype(F)


def e_adv_head(out, obs, S, T, adv, elites, mx, mn, aw, defect=None):
    K, N, D = out.shape[0], out.shape[1], out.shape[2] // 2
    Ba = obs.shape[0]
    Bs = N - Ba
    o = out[:, :Ba]
    mean = o[..., :D].copy()
    mean[..., :obs.shape[1]] += obs[None]
    lv, s1, s2 = e_soft_clamp(o[..., D:], mx, mn)
    sd = np.sqrt(np.exp(lv).astype(F)).astype(F)
    z = (S[None] - mean).astype(F)
    lp = ((-(z * z) / (F(2) * (sd * sd)) - np.log(sd)).astype(F) - LOG_SQRT_2PI).astype(F).astype(F64).sum(-1)
    el = np.arange(K) if defect == "mixture_over_all_members" else np.asarray(elites)
    m = lp[el].max(0)
    ex = np.zeros_like(lp)
    ex[el] = np.exp(lp[el] - m)
    rowlp = m + np.log(ex.sum(0)) - (0.0 if defect == "rowlp_without_log_elites" else math.log(len(el)))
    w = (ex / ex.sum(0)).astype(F)
    c0 = (F(aw) * adv / F(N if defect == "pg_divided_by_all_rows" else Ba)).astype(F)
    c = (c0[None, :, None] * w[:, :, None]).astype(F)
    inv = np.exp(-lv).astype(F)
    dlv = (c * F(0.5) * ((z * z * inv).astype(F) - F(1))).astype(F)
    dl1 = (dlv * s2).astype(F)
    r = ((c * z * inv).astype(F), (dl1 * s1).astype(F), np.zeros_like(lv), (dl1 * (F(1) - s1)).astype(F), (dlv * (F(1) - s2)).astype(F))
    d = e_nll(out[:, Ba:], T[None], mx, mn, Bs, Bs)
    cat = [np.concatenate([a, b], 1) for a, b in zip(r, d)]
    return dict(rowlp=rowlp, dout=np.concatenate([cat[0], cat[1]], -1), lterm=cat[2], gmax=cat[3], gmin=cat[4])


def e_adv_reduce(h, adv, mx, mn, Ba):
    D = h["lterm"].shape[-1]
    Bs = h["lterm"].shape[1] - Ba
    ls = F(0)
    smax = smin = F(0)
    cl = e_wave_sum(h["lterm"][:, Ba:].reshape(-1, D))
    for d in range(D):
        ls, smax, smin = F(ls + cl[d]), F(smax + mx[d]), F(smin + mn[d])
    c = F(dr.SL_LOGVAR_COEF)
    nll = F(ls / (F(Bs) * F(D)) + F(c * smax - c * smin))
    advm = np.array([(h["rowlp"] * adv.astype(F64)).sum() / Ba, h["rowlp"].sum() / Ba]).astype(F)
    return nll, (e_wave_sum(h["gmax"].reshape(-1, D)) + c).astype(F), (e_wave_sum(h["gmin"].reshape(-1, D)) - c).astype(F), advm


# =====================================================================================================================================
# operands at the table's cases
# =====================================================================================================================================
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _runs(c, ex):
    return [(r, ("y1", "y2")[r] if ex.get("edge") else None) for r in range(c["R"])]


def nll_cases():
    """(tag, out, t, mx, mn, rows, B, stale workspaces)"""
    for cid, c, train, ex in dc.LEARN:
        B = c["B"]
        rows = train - (-(-train // B) - 1) * B
        for r, edge in _runs(c, ex):
            rng = _rng(cid, r)
            out, t, mx, mn = dc.head_operands(rng, c, rows, edge)
            so, st_, _, _ = dc.head_operands(rng, c, B, edge)
            stale = e_nll(so, st_, mx, mn, B, B)[2:] if train > B else [np.zeros((c["K"], B, c["D"]), F)] * 3
            yield (cid, r), c, out, t, mx, mn, rows, B, stale


def head_cases():
    for cid, c, n, ex in dc.STEP:
        for r, edge in _runs(c, ex):
            rng = _rng("step", cid, r)
            out, _, mx, mn = dc.head_operands(rng, c, n, edge)
            if edge is None:
                far = np.setdiff1d(np.arange(c["K"]), c["elites"])            # non-elites the farthest out and the widest
                out[far, :, :c["D"]] *= 3.0
                out[far, :, c["D"]:] += 1.0
            obs = (3.0 * rng.normal(size=(n, c["od"]))).astype(F)
            noise = rng.normal(size=(c["K"], n, c["D"])).astype(F)
            midx = rng.choice(np.asarray(c["elites"]), size=n)
            yield (cid, r), c, out, obs, noise, midx, mx, mn, ex.get("step_coef", 2.5)


def adv_cases():
    for cid, c, Ba, Bs, ex in dc.ADV:
        for r, edge in _runs(c, ex):
            rng = _rng("adv", cid, r)
            out, t, mx, mn = dc.head_operands(rng, c, Ba + Bs, edge)
            obs = (3.0 * rng.normal(size=(Ba, c["od"]))).astype(F)
            noise = rng.normal(size=(c["K"], Ba, c["D"])).astype(F)
            midx = rng.choice(np.asarray(c["elites"]), size=Ba)
            S = dr.adv_sample(out, obs, noise, midx, mx, mn).v.astype(F)
            adv = (2.0 * rng.normal(size=Ba)).astype(F)
            yield (cid, r), c, out, obs, S, t[0, Ba:], adv, mx, mn, ex.get("adv_weight", 0.37), Ba, noise, midx


def adam_cases():
    for t0 in (0, 1, 999, 10 ** 6):
        rng = np.random.default_rng(t0 % 1000)
        tensors = [("max_logvar", 0, (4,)), ("backbones.0.weight", 4, (3, 5, 8)), ("backbones.0.bias", 124, (3, 1, 8)),
                   ("backbones.0.saved_weight", 148, (3, 5, 8)), ("output_layer.weight", 268, (3, 8, 7)), ("output_layer.bias", 436, (3, 1, 7))]
        P = 460
        wd, tr = dr.flat_layout(tensors, (0.1, 5e-4), P)
        tr[457:] = False
        flat, G = rng.normal(size=P).astype(F), (0.1 * rng.normal(size=P)).astype(F)
        m, v = (1e-2 * rng.normal(size=P)).astype(F), ((1e-2 * rng.normal(size=P)) ** 2 + 1e-8).astype(F)
        yield t0, flat, m, v, G, wd, tr, t0 + 1


WORST = {}


def ratios(tag, pairs, into):
    for key, got, ref in pairs:
        into[key] = max(into.get(key, 0.0), rr.ratio(got, ref))


def cat(a, b):
    return rr.BV(np.concatenate([a.v, b.v], -1), np.concatenate([a.e, b.e], -1))


def eval_all(defect=None):
    """worst err / bound per result of the fp32 evaluation (with ``defect`` planted) against the restatements, over the whole table"""
    w = {}
    for tag, c, out, t, mx, mn, rows, B, stale in nll_cases():
        D = c["D"]
        e = e_nll(out, t, mx, mn, rows, B, defect)
        ref = dr.nll_elem(out[..., :D], out[..., D:], t, mx, mn, rows, D)
        ratios(tag, [("nll.dout", np.concatenate(e[:2], -1), cat(ref[0], ref[1])), ("nll.lterm", e[2], ref[2]), ("nll.gmax", e[3], ref[3]),
                     ("nll.gmin", e[4], ref[4])], w)
        ws = [np.concatenate([a, s[:, rows:]], 1) for a, s in zip(e_nll(out, t, mx, mn, rows, B)[2:], stale)]
        got = e_reduce(ws, rows, mx, mn, c["coef"], defect)
        ref = dr.nll_reduce(*[a[:, :rows] for a in ws], mx, mn, c["coef"], rows)
        ratios(tag, [("reduce.nll", got[0], ref[0]), ("reduce.g_max", got[1], ref[1]), ("reduce.g_min", got[2], ref[2])], w)
    for tag, c, out, obs, noise, midx, mx, mn, coef in head_cases():
        for mode in dr.MODES:
            got = e_head(out, obs, noise, midx, c["elites"], mx, mn, mode, coef, defect)
            ref = dr.head(out, obs, noise, midx, mx, mn, mode, coef)
            ratios(tag, [("head.next_obs", got[0], ref[0]), ("head.raw", got[1], ref[1]), ("head.penalty." + mode, got[2], ref[2]),
                         ("head.reward", got[3], ref[3])], w)
    for tag, c, out, obs, S, T, adv, mx, mn, aw, Ba, noise, midx in adv_cases():
        h = e_adv_head(out, obs, S, T, adv, c["elites"], mx, mn, aw, defect)
        ref = dr.adv_head(out, obs, S, T, adv, c["elites"], mx, mn, aw)
        ratios(tag, [("adv.rowlp", h["rowlp"], ref["rowlp"])] + [("adv." + k, h[k], ref[k]) for k in ("dout", "lterm", "gmax", "gmin")], w)
        h0 = h if defect is None else e_adv_head(out, obs, S, T, adv, c["elites"], mx, mn, aw)
        got = e_adv_reduce(h0, adv, mx, mn, Ba)
        ref = dr.adv_reduce(h0["lterm"], h0["gmax"], h0["gmin"], h0["rowlp"], adv, mx, mn, Ba)
        ratios(tag, [("adv_reduce.nll", got[0], ref[0]), ("adv_reduce.g_max", got[1], ref[1]), ("adv_reduce.g_min", got[2], ref[2]),
                     ("adv_reduce.advm", got[3], ref[3])], w)
    for t0, flat, m, v, G, wd, tr, t in adam_cases():
        got = e_adam(flat, m, v, G, wd, tr, 1e-3, t, defect)
        ref = dr.adam(flat, m, v, G, wd, tr, 1e-3, 0.9, 0.999, 1e-8, t, torch_scalars=True)
        ratios(t0, [("adam.param", got[0], ref[0]), ("adam.exp_avg", got[1], ref[1]), ("adam.exp_avg_sq", got[2], ref[2]),
                    ("adam.decay", e_decay(flat, wd), dr.decay(flat, wd))], w)
    return w


# =====================================================================================================================================
# (a) values against float64 autograd
# =====================================================================================================================================
def close(a, b, scale, tag):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    bad = np.abs(a - b) > 1e-12 * (np.abs(b) + scale)
    assert not bad.any(), (tag, a[bad][:3], b[bad][:3])


def _model(c, mx, mn):
    from offlinerlkit.modules import EnsembleDynamicsModel
    m = EnsembleDynamicsModel(c["od"], c["ad"], [2], c["K"], len(c["elites"]), with_reward=bool(c["with_reward"])).double()
    m.max_logvar.data, m.min_logvar.data = torch.tensor(mx.astype(F64)), torch.tensor(mn.astype(F64))
    return m


def _clamped(model, out):
    from offlinerlkit.modules import soft_clamp
    mean, logvar = torch.chunk(out, 2, dim=-1)
    return mean, soft_clamp(logvar, model.min_logvar, model.max_logvar)          # EnsembleDynamicsModel.forward's last two lines


def test_values_equal_float64_autograd_of_the_model_loss():
    for tag, c, out, t, mx, mn, rows, B, _ in nll_cases():
        D = c["D"]
        model = _model(c, mx, mn)
        o = torch.tensor(out.astype(F64), requires_grad=True)
        mean, logvar = _clamped(model, o)
        tt = torch.tensor(t.astype(F64))
        loss = (torch.pow(mean - tt, 2) * torch.exp(-logvar)).mean(dim=(1, 2)).sum() + logvar.mean(dim=(1, 2)).sum() + \
            c["coef"] * model.max_logvar.sum() - c["coef"] * model.min_logvar.sum()          # ensemble_dynamics.py:199-205 less the decay
        loss.backward()
        ref = dr.nll_elem(out[..., :D], out[..., D:], t, mx, mn, rows, D)
        s = 1.0 / (rows * D)
        close(np.concatenate([ref[0].v, ref[1].v], -1), o.grad.numpy(), s, tag + ("dout",))
        close(ref[2].v, (torch.pow(mean - tt, 2) * torch.exp(-logvar) + logvar).detach().numpy(), np.abs(logvar.detach().numpy()).max(),
              tag + ("lterm",))
        nll, gmx, gmn = dr.nll_reduce(rr.BV(ref[2].v), rr.BV(ref[3].v), rr.BV(ref[4].v), mx, mn, c["coef"], rows)
        # the restatement holds the coefficient as fp32, the model as a double: compare with the same number
        cf = float(F(c["coef"]))
        fix = (cf - c["coef"])
        close(nll.v, loss.item() + fix * float(mx.astype(F64).sum() - mn.astype(F64).sum()), np.abs(ref[2].v).sum() * s, tag + ("nll",))
        dl1 = np.abs(ref[1].v).sum() + np.abs(ref[3].v).sum()            # |dl1| = |dl1 s1| + |dl1 (1 - s1)|: what cancels in 1 - s1
        close(gmx.v, model.max_logvar.grad.numpy() + fix, dl1, tag + ("g_max",))
        close(gmn.v, model.min_logvar.grad.numpy() - fix, dl1 + np.abs(ref[4].v).sum(), tag + ("g_min",))


def test_values_equal_float64_autograd_of_the_rambo_loss():
    for tag, c, out, obs, S, T, adv, mx, mn, aw, Ba, _, _ in adv_cases():
        K, N, D, od = c["K"], out.shape[1], c["D"], c["od"]
        Bs = N - Ba
        model = _model(c, mx, mn)
        o = torch.tensor(out.astype(F64), requires_grad=True)
        mean, logvar = _clamped(model, o)
        shift = np.zeros((K, N, D))          # mean[:, :Ba, :od] += obs in fp32, as the reference's fp32 tensors hold it
        shift[:, :Ba, :od] = (out[:, :Ba, :od] + obs[None]).astype(F).astype(F64) - out[:, :Ba, :od].astype(F64)
        mean = mean + torch.tensor(shift)
        std = torch.sqrt(torch.exp(logvar))
        el = torch.tensor(list(c["elites"]))
        # rambo.py:162-176: the mixture over the elites
        lpe = torch.distributions.Normal(mean[el, :Ba], std[el, :Ba]).log_prob(torch.tensor(S.astype(F64))[None])
        lp = lpe.sum(-1)
        log_prob = torch.logsumexp(lp, 0) - math.log(len(el))
        lp_mag = lpe.detach().abs().sum(-1).max(0).values.numpy()
        A = torch.tensor(adv.astype(F64))
        adv_loss = (log_prob * A).mean()
        tt = torch.tensor(T.astype(F64))
        sl = (torch.pow(mean[:, Ba:] - tt, 2) * torch.exp(-logvar[:, Ba:])).mean(dim=(1, 2)).sum() + logvar[:, Ba:].mean(dim=(1, 2)).sum() + \
            0.001 * model.max_logvar.sum() - 0.001 * model.min_logvar.sum()
        (float(F(aw)) * adv_loss + sl).backward()
        ref = dr.adv_head(out, obs, S, T, adv, c["elites"], mx, mn, aw)
        # the restatement holds log sqrt(2 pi) as the fp32 number the reference's fp32 tensors meet, torch's float64 graph as a double
        lshift = -D * (float(LOG_SQRT_2PI) - 0.91893853320467274178)
        ashift = np.array([lshift * float(adv.astype(F64).mean()), lshift])
        close(ref["rowlp"].v, log_prob.detach().numpy() + lshift, lp_mag, tag + ("rowlp",))
        g = o.grad.numpy()
        c0 = np.abs(aw * adv / Ba).max()
        close(ref["dout"].v[:, :Ba], g[:, :Ba], c0, tag + ("dout",))
        close(ref["dout"].v[:, Ba:], g[:, Ba:], 1.0 / (Bs * D), tag + ("dout_sl",))
        nll, gmx, gmn, advm = dr.adv_reduce(rr.BV(ref["lterm"].v), rr.BV(ref["gmax"].v), rr.BV(ref["gmin"].v), ref["rowlp"].v, adv, mx, mn, Ba)
        fix = float(F(0.001)) - 0.001
        scale = np.abs(ref["dout"].v[..., D:]).sum() + np.abs(ref["gmax"].v).sum() + np.abs(ref["gmin"].v).sum()
        close(gmx.v, model.max_logvar.grad.numpy() + fix, scale, tag + ("g_max",))
        close(gmn.v, model.min_logvar.grad.numpy() - fix, scale, tag + ("g_min",))
        close(advm.v, np.array([adv_loss.item(), log_prob.mean().item()]) + ashift, lp_mag.mean() * max(np.abs(adv).max(), 1.0), tag + ("advm",))
        close(nll.v, sl.item() + fix * float(mx.astype(F64).sum() - mn.astype(F64).sum()), np.abs(ref["lterm"].v).sum() / (Bs * D), tag + ("nll",))
        # ... and tests/rambo_oracle.py in float64, through an identity output layer that passes ``out`` on
        m64, g64 = _rambo_oracle(c, out, obs, S, T, adv, mx, mn, float(F(aw)), Ba, F64)      # the weight as the fp32 number the engine holds
        close(ref["rowlp"].v, m64["log_prob"] + lshift, lp_mag, tag + ("rowlp vs rambo_oracle",))
        close(advm.v, np.array([m64["adv_loss"], m64["adv_log_prob"]]) + ashift, lp_mag.mean() * max(np.abs(adv).max(), 1.0), tag + ("advm vs rambo_oracle",))
        close(gmx.v, g64["max_logvar"] + fix, scale, tag + ("g_max vs rambo_oracle",))
        close(ref["dout"].v.sum(1)[:, None], g64["output_layer.bias"], np.abs(ref["dout"].v).sum(1).max() + c0, tag + ("dout row sums vs rambo_oracle",))


def _identity_state(K, O, mx, mn, T):
    return {"output_layer.weight": np.tile(np.eye(O, dtype=T)[None], (K, 1, 1)), "output_layer.bias": np.zeros((K, 1, O), T),
            "max_logvar": mx.astype(T), "min_logvar": mn.astype(T)}


def _rambo_oracle(c, out, obs, S, T, adv, mx, mn, aw, Ba, dtype):
    K, O = out.shape[0], out.shape[2]
    st = _identity_state(K, O, mx, mn, dtype)
    mean, lv, cache = rorc.forward(st, out, dtype)
    mean = mean.copy()
    mean[:, :Ba, :c["od"]] = (out[:, :Ba, :c["od"]] + obs[None]).astype(F).astype(dtype)      # += obs on the reference's fp32 tensors
    f = dict(mean=mean, lv=lv, cache=cache, sample=S, target=T, Ba=Ba)
    return rorc.step_grads(f, list(c["elites"]), adv, aw, [0.0], dtype)


# =====================================================================================================================================
# (b) the reference alone stays inside the bar
# =====================================================================================================================================
def test_fp32_evaluation_stays_inside_the_bar():
    w = eval_all()
    print("\nworst fp32-evaluation err / bound per result:", {k: round(v, 3) for k, v in sorted(w.items())})
    assert max(w.values()) <= rr.FACTOR, {k: v for k, v in w.items() if v > rr.FACTOR}
    assert len(w) >= 25


def test_fp32_oracles_stay_inside_the_bar():
    """dyn_oracle.loss_and_grads (whole chain: head, sums, loss), rambo_oracle.step_grads in fp32 and mobile_oracle.sample_next_obss on
    the same operands, through an identity (or bias-only) output layer; the restatements chained from ``out`` carry the bound"""
    worst = {}
    for tag, c, out, t, mx, mn, rows, B, _ in nll_cases():
        K, D = c["K"], c["D"]
        st = _identity_state(K, 2 * D, mx, mn, F)
        loss, g = orc.loss_and_grads(st, out, t, [0.0], c["coef"])
        ref = dr.nll_elem(out[..., :D], out[..., D:], t, mx, mn, rows, D)
        nll, gmx, gmn = dr.nll_reduce(ref[2], ref[3], ref[4], mx, mn, c["coef"], rows)
        ratios(tag, [("dyn_oracle.loss", loss, nll), ("dyn_oracle.g_max", g["max_logvar"], gmx), ("dyn_oracle.g_min", g["min_logvar"], gmn)], worst)
        for i in range(0, rows, max(rows // 7, 1)):          # one row at a time the bias gradient IS the row of dOUT (scale 1 / D)
            _, gi = orc.loss_and_grads(st, out[:, i:i + 1], t[:, i:i + 1], [0.0], c["coef"])
            ri = dr.nll_elem(out[:, i:i + 1, :D], out[:, i:i + 1, D:], t[:, i:i + 1], mx, mn, 1, D)
            ratios(tag, [("dyn_oracle.dout", gi["output_layer.bias"], cat(ri[0], ri[1]))], worst)
    for tag, c, out, obs, S, T, adv, mx, mn, aw, Ba, noise, midx in adv_cases():
        m32, g32 = _rambo_oracle(c, out, obs, S, T, adv, mx, mn, aw, Ba, F)
        ref = dr.adv_head(out, obs, S, T, adv, c["elites"], mx, mn, aw)
        nll, gmx, gmn, advm = dr.adv_reduce(ref["lterm"], ref["gmax"], ref["gmin"], ref["rowlp"].v, adv, mx, mn, Ba)
        advm_e = np.array([(ref["rowlp"].e * np.abs(adv)).mean(), ref["rowlp"].e.mean()])
        ratios(tag, [("rambo_oracle.log_prob", m32["log_prob"], ref["rowlp"]), ("rambo_oracle.g_max", g32["max_logvar"], gmx),
                     ("rambo_oracle.g_min", g32["min_logvar"], gmn), ("rambo_oracle.sl_loss", m32["sl_loss"], nll),
                     ("rambo_oracle.advm", [m32["adv_loss"], m32["adv_log_prob"]], rr.BV(advm.v, advm.e + advm_e))], worst)
    for cid, c, n, S_ in dc.SAMPLE:
        rng = np.random.default_rng(n + S_)
        n = min(n, 9)
        K, D, od, E = c["K"], c["D"], c["od"], len(c["elites"])
        out, _, mx, mn = dc.head_operands(rng, c, n)
        obs, act = (3.0 * rng.normal(size=(n, od))).astype(F), np.zeros((n, c["ad"]), F)
        noise = rng.normal(size=(S_, E, n, D)).astype(F)
        ref = dr.sample_next(out, obs, noise, c["elites"], mx, mn)
        for b in range(n):                                    # a zero weight and the row's output as the bias
            st = {"output_layer.weight": np.zeros((K, od + c["ad"], 2 * D), F), "output_layer.bias": out[:, b:b + 1].copy(),
                  "max_logvar": mx, "min_logvar": mn}
            got = morc.sample_next_obss(st, (np.zeros(od + c["ad"], F), np.ones(od + c["ad"], F)), c["elites"], obs[b:b + 1], act[b:b + 1],
                                        noise[:, :, b:b + 1])
            ratios(cid, [("mobile_oracle.sample_next", got, ref[:, :, b:b + 1])], worst)
    print("\nworst oracle err / bound per result:", {k: round(v, 3) for k, v in sorted(worst.items())})
    assert max(worst.values()) <= rr.FACTOR, {k: v for k, v in worst.items() if v > rr.FACTOR}


# =====================================================================================================================================
# (c) the checks have teeth
# =====================================================================================================================================
@pytest.fixture(scope="module")
def clean():
    return eval_all()


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_is_caught(defect, clean):
    w = eval_all(defect)
    caught = {k: v for k, v in w.items() if v > rr.FACTOR and clean[k] <= rr.FACTOR}
    assert caught, (defect, "no result of any case leaves the bar", {k: round(v, 3) for k, v in w.items()})
