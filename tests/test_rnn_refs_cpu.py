"""CPU: keeps tests/test_gpu_rnn_kernels.py honest.  On every case of tests/rnn_kernel_cases.py (and case C's saturating twin):

(a) the VALUES of the float64 restatements (tests/rnn_refs.py), chained through all stages, equal tests/rnn_oracle.py in float64 and
    float64 torch autograd of the repository's RNNModel: loss, predictions and every tensor's gradient to 1e-12 of the tensor's largest
    magnitude (an element's own magnitude can cancel to nothing; float64 rounds against the terms).
(b) the reference alone stays inside the bar: a numpy fp32 emulation of one training step, which emits the taps of
    ``RnnDynamicsEngine.debug_read`` under the same names (gathered rows, forward saves, every backward stage, row terms, chunks,
    slabs, gradients, Adam), holds err / bound <= 4 on every element of every check of rnn_refs.check_forward / check_backward /
    check_adam -- the very functions the GPU module runs on the engine's taps.  The eval pass likewise.
(c) the checks have teeth: DEFECTS planted one at a time in that emulation are each caught by the check of the kernel they sit in."""
import numpy as np
import pytest
import torch

import rnn_cases as rc
import rnn_kernel_cases as kc
import rnn_oracle as orc
import rnn_refs as rf

F = np.float32

# defect -> (the cases it is planted in, the kernel whose check has to catch it)
DEFECTS = {
    "gather_mask_of_step_0": ("B", "k_rnn_gather"),
    "gi_without_bias": ("A", "gemm"),
    "clamped_unit_to_last": ("C", "k_rnn_scan_fwd"),
    "one_row_block_stale": ("B", "k_rnn_scan_fwd"),
    "hp_is_ht": ("D", "k_rnn_scan_fwd"),
    "ln_over_h_minus_1": ("D", "k_rnn_ln_fwd"),
    "ln_without_eps": ("A", "k_rnn_ln_fwd"),
    "dropout_scale_missing_fwd": ("B", "k_rnn_ln_fwd"),
    "loss_over_rows_only": ("E", "k_rnn_loss"),
    "nterm_second_dropped": ("B", "k_rnn_ln_bwd"),
    "dz_without_dropout_scale": ("F", "k_rnn_ln_bwd"),
    "dgamma_dbeta_swapped": ("A", "k_rnn_ln_bwd"),
    "swish_bwd_second_dropped": ("C", "k_rnn_swish_bwd"),
    "dgh_n_without_r": ("C", "k_rnn_scan_bwd"),
    "carry_dropped_at_one_t": ("H", "k_rnn_scan_bwd"),
    "z_gate_sign": ("D", "k_rnn_scan_bwd"),
    "last_chunk_skipped": ("E", "k_rnn_colsum_part"),
    "fin_reversed": ("E", "k_rnn_colsum_fin"),
    "slab_1_dropped": ("E", "k_rnn_slab_sum"),
    "wgrad_last_row_dropped": ("E", "wgrad"),
    "adam_one_minus_beta_in_fp32": ("A", "k_rnn_adam"),
}


def _sig(x):
    with np.errstate(over="ignore"):                      # (exp overflows to inf at a saturated gate, and 1 / inf is the 0 it stands for)
        return (F(1) / (F(1) + np.exp(-x))).astype(F)


def _dsw(z):
    s = _sig(z)
    return (s * (F(1) + z * (F(1) - s))).astype(F)


def _stats(u, defect=None):
    H = u.shape[1]
    mean = (u.sum(1, dtype=F) / F(H))[:, None]
    d = (u - mean).astype(F)
    var = ((d * d).sum(1, dtype=F) / F(H - 1 if defect == "ln_over_h_minus_1" else H))[:, None]
    return d, (F(1) / np.sqrt(var + (F(0) if defect == "ln_without_eps" else F(1e-5)))).astype(F)


def emulate(P, c, data, idx, drop=None, train=True, defect=None, moments=None, t=1, lr=1e-3):
    """one step (train) or one eval pass in numpy float32 -> dict(taps, tensors, grads, slabs, before, after)"""
    H, L, T, nb, od = c["H"], c["L"], c["T"], len(c["hidden"]) - 1, c["output_dim"]
    tensors, PF = rf.layout(rc.shapes(c))
    P = {k: np.asarray(v, F) for k, v in P.items()}
    x0, tgt, msk = rf.gather(data, idx)
    if defect == "gather_mask_of_step_0":
        msk = np.repeat(data[2][np.asarray(idx)][:, :1], T, 1).reshape(-1, 1)
    B, N = len(idx), len(idx) * T
    tp = dict(x0=x0, tgt=tgt, msk=msk)
    scale = F(1) / (F(1) - F(c["p"]))
    masked = train and drop is not None
    X = x0
    for l in range(L):
        Wih, Whh, bih, bhh = (P[f"rnn_layer.{k}_l{l}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        gi = (X @ Wih.T).astype(F)
        if not (defect == "gi_without_bias" and l == 0):
            gi = (gi + bih).astype(F)
        g3 = gi.reshape(B, T, 3 * H)
        h = np.zeros((B, H), F)
        sv = {k: np.zeros((B, T, H), F) for k in ("r", "z", "n", "hn", "hp", "ho")}
        for s in range(T):
            gh = (h @ Whh.T).astype(F)
            hn = (gh[:, 2 * H:] + bhh[2 * H:]).astype(F)
            r = _sig(g3[:, s, :H] + (gh[:, :H] + bhh[:H]))
            z = _sig(g3[:, s, H:2 * H] + (gh[:, H:2 * H] + bhh[H:2 * H]))
            n = np.tanh(g3[:, s, 2 * H:] + r * hn).astype(F)
            hv = ((F(1) - z) * n + z * h).astype(F)
            if defect == "clamped_unit_to_last":          # the lane past H reads the zero pad column as h_{t-1} and lands on unit H - 1
                hv[:, H - 1] = ((F(1) - z) * n)[:, H - 1]
            for k, a in (("r", r), ("z", z), ("n", n), ("hn", hn), ("hp", hv if defect == "hp_is_ht" else h), ("ho", hv)):
                sv[k][:, s] = a
            h = hv
        if defect == "one_row_block_stale" and B % 16 == 1:
            sv["ho"][B - 1] = 0
        for k in ("r", "z", "n", "hn", "hp"):
            if train:
                tp[f"{k}.{l}"] = sv[k].reshape(N, H)
        tp[f"gi.{l}"], tp[f"gru.{l}"] = gi, sv["ho"].reshape(N, H)
        X = tp[f"gru.{l}"]

    def block(slot, Xin, res, key, out_name):
        zp = (Xin @ P[key + ".linear.weight"].T + P[key + ".linear.bias"]).astype(F)
        act = (zp * _sig(zp)).astype(F)
        y = act
        if masked:
            tp[f"mask.{slot}"] = drop[slot]
            y = (act * drop[slot]).astype(F) if defect == "dropout_scale_missing_fwd" else (act * drop[slot] * scale).astype(F)
        if res is not None:
            y = (res + y).astype(F)
        d, rstd = _stats(y, defect)
        out = (d * rstd * P[key + ".layer_norm.weight"] + P[key + ".layer_norm.bias"]).astype(F)
        if train:
            tp[f"zpre.{slot}"] = zp
        tp[f"act.{slot}"], tp[f"drop.{slot}"], tp[out_name] = act, y, out
        return out
    yin = block(0, x0, None, "input_layer", "in")
    ct = np.concatenate([yin, X], 1)
    zm = (ct @ P["merge_layer.weight"].T + P["merge_layer.bias"]).astype(F)
    y = tp["merge"] = (zm * _sig(zm)).astype(F)
    if train:
        tp["zmerge"] = zm
    for i in range(nb):
        y = block(1 + i, y, y, f"backbones.{i}", f"block.{i}")
    pred = tp["pred"] = (y @ P["output_layer.weight"].T + P["output_layer.bias"]).astype(F)
    out = dict(taps=tp, tensors=tensors)
    if not train:
        return out
    # ---- the loss and the backward ----
    inv = F(1) / F(N if defect == "loss_over_rows_only" else N * od)
    df = (pred - tgt).astype(F)
    tp["loss"] = np.array([[(df * df * msk).sum(dtype=F) * inv]], F)
    tp["dpred"] = (F(2) * df * msk * inv).astype(F)
    tp["dx"] = (tp["dpred"] @ P["output_layer.weight"]).astype(F)
    pn = (nb + 1) * 2 * H
    part = tp["part"] = np.zeros((N, pn), F)

    def norm_bwd(slot, dys, key):
        dy = dys[0] if len(dys) == 1 or defect == "nterm_second_dropped" else (dys[0] + dys[1]).astype(F)
        d, rstd = _stats(tp[f"drop.{slot}"])
        xh = (d * rstd).astype(F)
        pg, pb = (dy * xh).astype(F), dy
        if defect == "dgamma_dbeta_swapped":
            pg, pb = pb, pg
        part[:, slot * 2 * H:slot * 2 * H + H], part[:, slot * 2 * H + H:(slot + 1) * 2 * H] = pg, pb
        dxh = (dy * P[key + ".layer_norm.weight"]).astype(F)
        s1 = (dxh.sum(1, dtype=F) / F(H))[:, None]
        s2 = ((dxh * xh).sum(1, dtype=F) / F(H))[:, None]
        du = (rstd * (dxh - s1 - xh * s2)).astype(F)
        ds = du
        if masked:
            ds = (du * drop[slot]).astype(F) if defect == "dz_without_dropout_scale" else (du * drop[slot] * scale).astype(F)
        tp[f"dz.{slot}"] = (ds * _dsw(tp[f"zpre.{slot}"])).astype(F)
        return du
    for i in range(nb - 1, -1, -1):
        tp[f"du.{i}"] = norm_bwd(1 + i, [tp["dx"]] if i == nb - 1 else [tp[f"du.{i + 1}"], tp[f"dt.{i + 1}"]], f"backbones.{i}")
        tp[f"dt.{i}"] = (tp[f"dz.{1 + i}"] @ P[f"backbones.{i}.linear.weight"]).astype(F)
    a = tp["du.0"] if defect == "swish_bwd_second_dropped" else (tp["du.0"] + tp["dt.0"]).astype(F)
    tp["dzm"] = (a * _dsw(zm)).astype(F)
    dcat = tp["dcat"] = (tp["dzm"] @ P["merge_layer.weight"]).astype(F)
    norm_bwd(0, [dcat[:, :H]], "input_layer")
    chunk = rf.colsum_part(part)
    if defect == "last_chunk_skipped" and N % rf.CHUNK:
        chunk[-1] = 0
    tp["chunk"] = chunk
    fin = rf.colsum_fin(chunk[::-1] if defect == "fin_reversed" else chunk)
    dout = dcat[:, H:]
    for l in range(L - 1, -1, -1):
        Whh = P[f"rnn_layer.weight_hh_l{l}"]
        r, z, n, hn, hp = (tp[f"{k}.{l}"].reshape(B, T, H) for k in ("r", "z", "n", "hn", "hp"))
        dgi, dgh, carry = np.zeros((B, T, 3 * H), F), np.zeros((B, T, 3 * H), F), np.zeros((B, H), F)
        d3 = dout.reshape(B, T, H)
        for s in range(T - 1, -1, -1):
            dh = (d3[:, s] + carry).astype(F)
            gn = (dh * (F(1) - z[:, s]) * (F(1) - n[:, s] * n[:, s])).astype(F)
            gz = (dh * (hp[:, s] - n[:, s]) * z[:, s] * (F(1) - z[:, s])).astype(F)
            if defect == "z_gate_sign":
                gz = -gz
            gr = (gn * hn[:, s] * r[:, s] * (F(1) - r[:, s])).astype(F)
            dgi[:, s] = np.concatenate([gr, gz, gn], 1)
            dgh[:, s] = np.concatenate([gr, gz, gn if defect == "dgh_n_without_r" else (gn * r[:, s]).astype(F)], 1)
            carry = (dh * z[:, s] + (dgh[:, s] @ Whh).astype(F)).astype(F)
            if defect == "carry_dropped_at_one_t" and s == T // 2:
                carry = np.zeros((B, H), F)
        tp[f"dgi.{l}"], tp[f"dgh.{l}"] = dgi.reshape(N, 3 * H), dgh.reshape(N, 3 * H)
        if l:
            dout = tp[f"dxl.{l}"] = (tp[f"dgi.{l}"] @ P[f"rnn_layer.weight_ih_l{l}"]).astype(F)
    # ---- the slabs: k ranges of the rows; dgamma / dbeta in slab 0 ----
    ns = rf.n_slabs(PF, c["B"] * T, N)
    slabs = [np.zeros(PF, F) for _ in range(ns)]
    where = {nm: o for nm, o, _ in tensors}
    tp["cat"] = ct
    rows_end = N - 1 if defect == "wgrad_last_row_dropped" else N
    for wk, bk, dy, xn in rf.linears(c):
        for k in range(ns):
            rs = slice(N * k // ns, min(N * (k + 1) // ns, rows_end))
            w = (tp[dy][rs].T @ tp[xn][rs]).astype(F)
            slabs[k][where[wk]:where[wk] + w.size] = w.ravel()
            slabs[k][where[bk]:where[bk] + w.shape[0]] = tp[dy][rs].sum(0, dtype=F)
    del tp["cat"]
    for slot in range(nb + 1):
        key = "input_layer" if slot == 0 else f"backbones.{slot - 1}"
        slabs[0][where[key + ".layer_norm.weight"]:][:H] = fin[slot * 2 * H:slot * 2 * H + H]
        slabs[0][where[key + ".layer_norm.bias"]:][:H] = fin[slot * 2 * H + H:(slot + 1) * 2 * H]
    grads = rf.slab_sum(slabs[:1] if defect == "slab_1_dropped" else slabs)
    # ---- torch.optim.Adam, step t ----
    flat = np.zeros(PF, F)
    for nm, o, s in tensors:
        flat[o:o + P[nm].size] = P[nm].ravel()
    m0, v0 = moments if moments is not None else (np.zeros(PF, F), np.zeros(PF, F))
    b1, b2, eps = 0.9, 0.999, 1e-8
    w1, w2 = (F(1) - F(b1), F(1) - F(b2)) if defect == "adam_one_minus_beta_in_fp32" else (F(1.0 - b1), F(1.0 - b2))
    step, bc2s = F(lr / (1.0 - b1 ** t)), F(np.sqrt(1.0 - b2 ** t))
    m = (m0 + (grads - m0) * w1).astype(F)
    v = (v0 * F(b2) + w2 * grads * grads).astype(F)
    p = (flat - step * (m / (np.sqrt(v) / bc2s + F(eps)))).astype(F)
    out.update(grads=grads, slabs=slabs, before=(flat, m0, v0), after=(p, m, v), t=t, lr=lr)
    return out


def setup(name):
    """(c, P, data, idx, drop) of a case; "Csat": case C with saturating gates"""
    c = kc.case(name[0])
    P, data = rc.make_params(c), kc.data(c)
    if name == "Csat":
        P, x = kc.saturated(P, data[0])
        data = (x,) + data[1:]
    return c, P, data, kc.indices(c), kc.drop_masks(c)


def moments_of(PF, tensors, seed):
    rng = np.random.RandomState(seed)
    keep = np.zeros(PF, bool)
    for _, o, s in tensors:
        keep[o:o + int(np.prod(s))] = True
    m = np.where(keep, 1e-2 * rng.standard_normal(PF), 0).astype(F)
    v = np.where(keep, (1e-2 * rng.standard_normal(PF)) ** 2 + 1e-8, 0).astype(F)
    return m, v


def run_checks(e, P, c, data, idx, rec):
    tp = e["taps"]
    x0, tgt, msk = rf.gather(data, idx)
    for k, want in (("x0", x0), ("tgt", tgt), ("msk", msk)):
        rec.same(tp[k], want, "k_rnn_gather." + k)
    rf.check_forward(tp.__getitem__, P, c, rec, train=True)
    rf.check_backward(tp.__getitem__, P, c, rec, e["grads"], e["tensors"], e["slabs"])
    rf.check_adam(e["before"], e["after"], e["grads"], e["t"], e["lr"], rec)


ALL = kc.NAMES + ["Csat"]


@pytest.mark.parametrize("name", ALL)
def test_chained_restatements_equal_the_oracle_and_autograd(name):
    c, P, data, idx, drop = setup(name)
    x, tg, mk = (a[idx] for a in data)
    lo, pred, G = rf.chain(P, c, x, tg, mk, drop)
    lo64, pred64, G64, _ = orc.loss_and_grads(P, c, x, tg, mk, drop, np.float64)
    from offlinerlkit.nets import RNNModel
    m = RNNModel(c["input_dim"], c["output_dim"], list(c["hidden"]), c["L"], 0.0).double()
    m.load_state_dict({k: torch.from_numpy(v).double() for k, v in P.items()})
    if drop is not None:
        class Forced(torch.nn.Module):
            def __init__(self, keep):
                super().__init__()
                self.keep = torch.from_numpy(keep).double()

            def forward(self, v):
                return v * self.keep.reshape(v.shape) / (1.0 - c["p"])
        for s, b in enumerate([m.input_layer] + list(m.backbones)):
            b.dropout = Forced(drop[s])
    pr, _ = m(torch.from_numpy(x).double())
    lt = (((pr - torch.from_numpy(tg).double()) ** 2).mean(-1) * torch.from_numpy(mk).double()).mean()
    lt.backward()
    Gt = {k: v.grad.numpy() for k, v in m.named_parameters()}

    def close(a, b, what):
        s = max(float(np.abs(b).max()), 1e-300)
        assert float(np.abs(np.asarray(a) - b).max()) <= 1e-12 * s, (what, float(np.abs(np.asarray(a) - b).max()) / s)
    close(lo, np.float64(lo64), "loss"), close(lo, lt.detach().numpy(), "loss (torch)")
    close(pred, pred64, "pred"), close(pred, pr.detach().numpy(), "pred (torch)")
    assert set(G) == set(G64) == set(Gt)
    for k in G:
        close(G[k], G64[k], k), close(G[k], Gt[k], k + " (torch)")


@pytest.mark.parametrize("name", ALL)
def test_fp32_emulation_stays_inside_the_bar(name):
    c, P, data, idx, drop = setup(name)
    tensors, PF = rf.layout(rc.shapes(c))
    e = emulate(P, c, data, idx, drop, moments=moments_of(PF, tensors, 3), t=4)
    rec = rf.Rec()
    run_checks(e, P, c, data, idx, rec)
    ev = emulate(P, c, data, idx[:max(1, len(idx) // 2)], train=False)
    rf.check_forward(ev["taps"].__getitem__, P, c, rec, train=False)
    print(name, {k: round(v, 3) for k, v in sorted(rec.worst.items())})
    rec.finish()
    assert len(rec.worst) >= 30


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_is_caught(defect):
    name, kernel = DEFECTS[defect]
    c, P, data, idx, drop = setup(name)
    clean, bad = rf.Rec(), rf.Rec()
    run_checks(emulate(P, c, data, idx, drop), P, c, data, idx, clean)
    clean.finish()
    run_checks(emulate(P, c, data, idx, drop, defect=defect), P, c, data, idx, bad)
    print(defect, "->", bad.missed[:3])
    assert kernel in bad.kernels(), (defect, bad.kernels())


def test_every_kernel_has_a_defect():
    assert len(DEFECTS) == 21
    assert {k for _, k in DEFECTS.values()} == {"k_rnn_gather", "gemm", "k_rnn_scan_fwd", "k_rnn_ln_fwd", "k_rnn_loss", "k_rnn_ln_bwd",
                                                 "k_rnn_swish_bwd", "k_rnn_scan_bwd", "k_rnn_colsum_part", "k_rnn_colsum_fin",
                                                 "k_rnn_slab_sum", "wgrad", "k_rnn_adam"}
