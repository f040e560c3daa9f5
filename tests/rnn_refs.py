"""Self-bounding float64 restatements of the RNN dynamics kernels (csrc/rnn_dynamics.hip), one function per kernel, written from the
reference's formulas (nets/rnn.py: RNNModel; torch's GRU, LayerNorm and Adam definitions) on tests/row_refs.py's ``BV``: every value
carries a first-order bound on what fp32 may lose on the same operands, and a kernel is held to |got - ref.v| <= FACTOR * ref.e on
EVERY element.  Operands read back from the engine are exact.  A matrix product's element gets the any-order bound
K u sum |a_i b_i| (plus what its operands carry, plus the bias add): nothing is assumed about the order inside the MFMA or the tiles.
The column sums and the slab sum are pure fp32 additions in a documented order and are restated bit for bit in numpy float32.

``check_forward`` / ``check_backward`` run every restatement on the taps of one step, given a reader ``rd(name) -> [rows, cols]``:
the engine's ``debug_read`` on the GPU (tests/test_gpu_rnn_kernels.py), an fp32 emulation here (tests/test_rnn_refs_cpu.py).
``chain`` runs the same functions end to end in float64, which is what ties them to the oracle and to autograd."""
import numpy as np

import row_refs as rr
from row_refs import BV, TINY, U

f32 = np.float32
EPS_LN = 1e-5
CHUNK = 64          # rows of a first-level column sum
SLAB_ROWS = 256     # fewest rows of a split weight gradient's k range


def _bv(x):
    return BV.exact(x)


def cat(xs, axis=-1):
    xs = [_bv(x) for x in xs]
    return BV(np.concatenate([x.v for x in xs], axis), np.concatenate([x.e for x in xs], axis))


def tr(w):
    w = _bv(w)
    return BV(w.v.T, w.e.T)


def sigmoid(x):
    return 1.0 / (1.0 + rr.exp(-_bv(x)))


def swish(z):
    z = _bv(z)
    return z * sigmoid(z)


def dswish(z):
    z = _bv(z)
    s = sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


def matmul(A, W, bias=None):
    """A [M, K] times W^T (W [N, K]), plus the bias [N]: any summation order of the K products"""
    A, W = _bv(A), _bv(W)
    K = A.v.shape[1]
    aa, aw = np.abs(A.v), np.abs(W.v)
    y = BV(A.v @ W.v.T, K * U * (aa @ aw.T) + A.e @ aw.T + aa @ W.e.T + K * TINY)
    return y if bias is None else y + _bv(bias)


# ---- k_rnn_gather ------------------------------------------------------------------------------------------------------------------
def gather(data, idx):
    """the step's sequences, targets and loss masks as [rows * T, cols] (exact)"""
    x, tg, mk = data
    idx = np.asarray(idx, np.int64)
    return x[idx].reshape(-1, x.shape[-1]), tg[idx].reshape(-1, tg.shape[-1]), mk[idx].reshape(-1, 1)


# ---- k_rnn_scan_fwd: torch.nn.GRU's cell ---------------------------------------------------------------------------------------------
def gru_cell(gi, hp, whh, bhh):
    """r = s(W_ir x + b_ir + W_hr h + b_hr), z likewise, n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h' = (1 - z) n + z h, for rows of
    input projections gi [rows, 3H] and previous states hp [rows, H]; sigmoid as 1 / (1 + exp(-x))"""
    gi, hp = _bv(gi), _bv(hp)
    H = hp.shape[1]
    gh = matmul(hp, whh, bhh)
    r = sigmoid(gi[:, :H] + gh[:, :H])
    z = sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    hn = gh[:, 2 * H:]
    n = rr.tanh(gi[:, 2 * H:] + r * hn)
    return dict(r=r, z=z, n=n, hn=hn, h=(1.0 - z) * n + z * hp)


# ---- k_rnn_ln_fwd ------------------------------------------------------------------------------------------------------------------
def dropout_scale(p):
    """1 / (1 - p) for the fp32 rate the engine's configuration holds (a BV: that rate as given)"""
    return 1.0 / (1.0 - (p if isinstance(p, BV) else _bv(f32(p))))


def dropout_res(act, mask, p, res):
    """res + dropout(act): kept values times 1 / (1 - p)"""
    y = _bv(act)
    if mask is not None:
        y = y * _bv(mask) * dropout_scale(p)
    return y if res is None else _bv(res) + y


def ln_stats(u, eps=EPS_LN):
    """(u - mean, 1 / sqrt(var + eps)) of every row, biased variance; one wave sums a row"""
    u = _bv(u)
    H = u.shape[1]
    mean = (rr.sum_(u, axis=1, stride=64) / float(H)).reshape(-1, 1)
    d = u - mean
    var = (rr.sum_(d * d, axis=1, stride=64) / float(H)).reshape(-1, 1)
    return d, 1.0 / rr.sqrt(var + eps)


def layer_norm(u, gamma, beta, eps=EPS_LN):
    d, rstd = ln_stats(u, eps)
    return d * rstd * _bv(gamma) + _bv(beta)


# ---- k_rnn_loss --------------------------------------------------------------------------------------------------------------------
def loss(pred, tgt, msk):
    """(((pred - target)^2).mean(-1) * masks).mean() and its gradient 2 (pred - target) mask / (rows od)"""
    pred, tgt = _bv(pred), _bv(tgt)
    rows, od = pred.shape
    m = _bv(msk).reshape(-1, 1)
    inv = 1.0 / _bv(f32(rows * od))
    df = pred - tgt
    return rr.sum_((df * df * m).reshape(-1)) * inv, 2.0 * df * m * inv


# ---- k_rnn_ln_bwd, k_rnn_swish_bwd -----------------------------------------------------------------------------------------------------
def ln_bwd(dys, u, gamma, mask, p, zpre, eps=EPS_LN):
    """backward of LayerNorm(u), u = res + dropout(swish(zpre)), for dOut = the sum of ``dys``: the row's dgamma / dbeta terms, du
    (also the residual path's gradient) and dz = du mask / (1 - p) swish'(zpre)"""
    dy = _bv(dys[0])
    for more in dys[1:]:
        dy = dy + _bv(more)
    d, rstd = ln_stats(u, eps)
    H = d.shape[1]
    xh = d * rstd
    dxh = dy * _bv(gamma)
    s1 = (rr.sum_(dxh, axis=1, stride=64) / float(H)).reshape(-1, 1)
    s2 = (rr.sum_(dxh * xh, axis=1, stride=64) / float(H)).reshape(-1, 1)
    du = rstd * (dxh - s1 - xh * s2)
    ds = du if mask is None else du * _bv(mask) * dropout_scale(p)
    return dict(pg=dy * xh, pb=dy, du=du, dz=ds * dswish(zpre))


def swish_bwd(a, b, z):
    return (_bv(a) + _bv(b)) * dswish(z)


# ---- k_rnn_scan_bwd ----------------------------------------------------------------------------------------------------------------
def gru_bwd_cell(dout, carry, r, z, n, hn, hp, whh):
    """one step of the GRU cell's backward: dh = dout + carry; the gradients of the input-side pre-activations (r | z | n) and of the
    hidden-side ones (the n column times r); the carry to the step before, dh z + dGH W_hh"""
    r, z, n, hn, hp = (_bv(a) for a in (r, z, n, hn, hp))
    dh = _bv(dout) + carry
    gn = dh * (1.0 - z) * (1.0 - n * n)
    gz = dh * (hp - n) * z * (1.0 - z)
    gr = gn * hn * r * (1.0 - r)
    dgh = cat([gr, gz, gn * r])
    return cat([gr, gz, gn]), dgh, dh * z + matmul(dgh, tr(whh))


# ---- k_rnn_colsum_part, k_rnn_colsum_fin, k_rnn_slab_sum: fp32 additions, one term at a time -----------------------------------------
def colsum_part(part):
    """[rows, pn] -> [chunks, pn]: each chunk's 64 rows (the last one's fewer) added in row order from 0"""
    part = np.asarray(part, f32)
    rows, pn = part.shape
    out = np.zeros(((rows + CHUNK - 1) // CHUNK, pn), f32)
    for k in range(out.shape[0]):
        s = np.zeros(pn, f32)
        for r in range(k * CHUNK, min((k + 1) * CHUNK, rows)):
            s = (s + part[r]).astype(f32)
        out[k] = s
    return out


def colsum_fin(chunk):
    s = np.zeros(chunk.shape[1], f32)
    for k in range(chunk.shape[0]):
        s = (s + chunk[k]).astype(f32)
    return s


def slab_sum(slabs):
    s = np.asarray(slabs[0], f32).copy()
    for more in slabs[1:]:
        s = (s + more).astype(f32)
    return s


def n_slabs(P, cap_rows, rows):
    """k ranges of a step's weight gradients: at least SLAB_ROWS rows each, at most 8, and no more than 64 Mi floats of slabs"""
    return int(max(1, min(8, cap_rows // SLAB_ROWS, (64 << 20) // P, rows // SLAB_ROWS)))


# ---- the weight and bias gradients ---------------------------------------------------------------------------------------------------
def wgrad(dY, X):
    """dW [out, in] = dY^T X and db = the column sums of dY, over all rows in any order"""
    dY, X = _bv(dY), _bv(X)
    return matmul(tr(dY), tr(X)), matmul(tr(dY), np.ones((1, dY.shape[0]), f32)).reshape(-1)


# =====================================================================================================================================
# the layout and the drivers
# =====================================================================================================================================
def layout(shapes):
    """[(name, offset, shape)] of a parameter block: state_dict order, every tensor on 4 floats -> (tensors, floats)"""
    out, off = [], 0
    for name, shape in shapes:
        off = (off + 3) & ~3
        out.append((name, off, tuple(shape)))
        off += int(np.prod(shape))
    return out, (off + 3) & ~3


def unflatten(tensors, flat):
    return {n: flat[o:o + int(np.prod(s))].reshape(s) for n, o, s in tensors}


def linears(c):
    """[(weight key, bias key, dY tap, X tap or taps)] of every Linear and GRU product, what its weight gradient reduces over"""
    L, nb = c["L"], len(c["hidden"]) - 1
    out = [("output_layer.weight", "output_layer.bias", "dpred", f"block.{nb - 1}"), ("merge_layer.weight", "merge_layer.bias", "dzm", "cat"),
           ("input_layer.linear.weight", "input_layer.linear.bias", "dz.0", "x0")]
    for i in range(nb):
        out.append((f"backbones.{i}.linear.weight", f"backbones.{i}.linear.bias", f"dz.{1 + i}", f"block.{i - 1}" if i else "merge"))
    for l in range(L):
        out.append((f"rnn_layer.weight_hh_l{l}", f"rnn_layer.bias_hh_l{l}", f"dgh.{l}", f"hp.{l}"))
        out.append((f"rnn_layer.weight_ih_l{l}", f"rnn_layer.bias_ih_l{l}", f"dgi.{l}", f"gru.{l - 1}" if l else "x0"))
    return out


class Rec:
    """collects the worst err / bound per check and the checks that missed"""

    def __init__(self, worst=None):
        self.worst = {} if worst is None else worst
        self.missed = []

    def hold(self, got, ref, key, *tag):
        r = rr.ratio(got, ref)
        self.worst[key] = max(self.worst.get(key, 0.0), r)
        if not r <= rr.FACTOR:
            self.missed.append((key, tag, r))

    def same(self, got, want, key, *tag):
        """bit for bit (as values: -0 == 0)"""
        got, want = np.asarray(got), np.asarray(want)
        ok = got.shape == want.shape and np.array_equal(got, want)
        self.worst.setdefault(key, 0.0)
        if not ok:
            self.missed.append((key, tag, "bits"))

    def kernels(self):
        return sorted({k.split(".")[0] for k, _, _ in self.missed})

    def finish(self):
        assert not self.missed, self.missed[:8]


def reader(rd):
    """``rd`` behind a cache: every tap is read back once"""
    seen = {}

    def get(name):
        if name not in seen:
            seen[name] = rd(name)
        return seen[name]
    return get


def check_forward(rd, P, c, rec, train=True):
    """every forward kernel and product of one pass on its taps; train: the saves and pre-activations too"""
    H, L, T, nb = c["H"], c["L"], c["T"], len(c["hidden"]) - 1
    rd = reader(rd)
    x0 = rd("x0")
    B = x0.shape[0] // T
    X = x0
    for l in range(L):
        gi, ho = rd(f"gi.{l}"), rd(f"gru.{l}")
        rec.hold(gi, matmul(X, P[f"rnn_layer.weight_ih_l{l}"], P[f"rnn_layer.bias_ih_l{l}"]), "gemm.gi", l)
        shifted = np.concatenate([np.zeros((B, 1, H), f32), ho.reshape(B, T, H)[:, :-1]], 1).reshape(B * T, H)
        if train:
            rec.same(rd(f"hp.{l}"), shifted, "k_rnn_scan_fwd.hp", l)
        ref = gru_cell(gi, rd(f"hp.{l}") if train else shifted, P[f"rnn_layer.weight_hh_l{l}"], P[f"rnn_layer.bias_hh_l{l}"])
        rec.hold(ho, ref["h"], "k_rnn_scan_fwd.h", l)
        if train:
            for k in ("r", "z", "n", "hn"):
                rec.hold(rd(f"{k}.{l}"), ref[k], "k_rnn_scan_fwd." + k, l)
        X = ho
    masked = train and c["p"] > 0

    def block(slot, Xin, res, key, out_name):
        zp = matmul(Xin, P[key + ".linear.weight"], P[key + ".linear.bias"])
        if train:
            rec.hold(rd(f"zpre.{slot}"), zp, "gemm.zpre", slot)
            zp = rd(f"zpre.{slot}")
        act, u = rd(f"act.{slot}"), rd(f"drop.{slot}")
        rec.hold(act, swish(zp), "gemm.act", slot)
        rec.hold(u, dropout_res(act, rd(f"mask.{slot}") if masked else None, c["p"], res), "k_rnn_ln_fwd.drop", slot)
        rec.hold(rd(out_name), layer_norm(u, P[key + ".layer_norm.weight"], P[key + ".layer_norm.bias"]), "k_rnn_ln_fwd.out", slot)
        return rd(out_name)

    yin = block(0, x0, None, "input_layer", "in")
    zm = matmul(np.concatenate([yin, X], 1), P["merge_layer.weight"], P["merge_layer.bias"])
    if train:
        rec.hold(rd("zmerge"), zm, "gemm.zmerge")
        zm = rd("zmerge")
    y = rd("merge")
    rec.hold(y, swish(zm), "gemm.merge")
    for i in range(nb):
        y = block(1 + i, y, y, f"backbones.{i}", f"block.{i}")
    rec.hold(rd("pred"), matmul(y, P["output_layer.weight"], P["output_layer.bias"]), "gemm.pred")


def check_backward(rd, P, c, rec, grads, tensors, slabs):
    """the loss and every backward kernel and product of one training step on its taps.  grads: the flat gradient block; tensors: its
    layout; slabs: the flat slabs the step wrote, in order"""
    H, L, T, nb = c["H"], c["L"], c["T"], len(c["hidden"]) - 1
    base = reader(rd)

    def rd(name):
        return np.concatenate([base("in"), base(f"gru.{L - 1}")], 1) if name == "cat" else base(name)
    pred = rd("pred")
    B = pred.shape[0] // T
    masked = c["p"] > 0
    lo, dp = loss(pred, rd("tgt"), rd("msk"))
    rec.hold(rd("loss"), lo, "k_rnn_loss.loss")
    rec.hold(rd("dpred"), dp, "k_rnn_loss.dpred")
    rec.hold(rd("dx"), matmul(rd("dpred"), tr(P["output_layer.weight"])), "gemm.dx")
    part = rd("part")

    def norm_bwd(slot, dys, key, du_name):
        ref = ln_bwd(dys, rd(f"drop.{slot}"), P[key + ".layer_norm.weight"], rd(f"mask.{slot}") if masked else None, c["p"], rd(f"zpre.{slot}"))
        o = slot * 2 * H
        rec.hold(part[:, o:o + H], ref["pg"], "k_rnn_ln_bwd.part_gamma", slot)
        rec.hold(part[:, o + H:o + 2 * H], ref["pb"], "k_rnn_ln_bwd.part_beta", slot)
        if du_name:
            rec.hold(rd(du_name), ref["du"], "k_rnn_ln_bwd.du", slot)
        rec.hold(rd(f"dz.{slot}"), ref["dz"], "k_rnn_ln_bwd.dz", slot)

    for i in range(nb - 1, -1, -1):
        norm_bwd(1 + i, [rd("dx")] if i == nb - 1 else [rd(f"du.{i + 1}"), rd(f"dt.{i + 1}")], f"backbones.{i}", f"du.{i}")
        rec.hold(rd(f"dt.{i}"), matmul(rd(f"dz.{1 + i}"), tr(P[f"backbones.{i}.linear.weight"])), "gemm.dt", i)
    rec.hold(rd("dzm"), swish_bwd(rd("du.0"), rd("dt.0"), rd("zmerge")), "k_rnn_swish_bwd.dzm")
    dcat = rd("dcat")
    rec.hold(dcat, matmul(rd("dzm"), tr(P["merge_layer.weight"])), "gemm.dcat")
    norm_bwd(0, [dcat[:, :H]], "input_layer", None)
    # dgamma / dbeta: two levels of column sums into slab 0, then the slabs in order
    chunk = rd("chunk")
    rec.same(chunk, colsum_part(part), "k_rnn_colsum_part.chunk")
    fin, where = colsum_fin(chunk), {n: o for n, o, _ in tensors}
    for slot in range(nb + 1):
        key = "input_layer" if slot == 0 else f"backbones.{slot - 1}"
        for half, nm in enumerate((".layer_norm.weight", ".layer_norm.bias")):
            o = where[key + nm]
            rec.same(slabs[0][o:o + H], fin[slot * 2 * H + half * H:slot * 2 * H + (half + 1) * H], "k_rnn_colsum_fin.slab0", slot, nm)
    rec.same(grads, slab_sum(slabs), "k_rnn_slab_sum.grads")
    # the GRU layers, top down
    dout = dcat[:, H:]
    for l in range(L - 1, -1, -1):
        dgi, dgh = rd(f"dgi.{l}"), rd(f"dgh.{l}")
        rec.same(dgi[:, :2 * H], dgh[:, :2 * H], "k_rnn_scan_bwd.rz_columns", l)
        carry = BV(np.zeros((B, H)))
        sv = [rd(f"{k}.{l}") for k in ("r", "z", "n", "hn", "hp")]
        for t in range(T - 1, -1, -1):
            rows = np.arange(B) * T + t
            gi_t, gh_t, carry = gru_bwd_cell(dout[rows], carry, *[a[rows] for a in sv], P[f"rnn_layer.weight_hh_l{l}"])
            rec.hold(dgi[rows], gi_t, "k_rnn_scan_bwd.dgi", l, t)
            rec.hold(dgh[rows], gh_t, "k_rnn_scan_bwd.dgh", l, t)
        if l:
            dout = rd(f"dxl.{l}")
            rec.hold(dout, matmul(dgi, tr(P[f"rnn_layer.weight_ih_l{l}"])), "gemm.dxl", l)
    G = unflatten(tensors, grads)
    for wk, bk, dy, xn in linears(c):
        dW, db = wgrad(rd(dy), rd(xn))
        rec.hold(G[wk], dW, "wgrad.weight", wk)
        rec.hold(G[bk], db, "wgrad.bias", bk)


def check_adam(before, after, grads, t, lr, rec, b1=0.9, b2=0.999, eps=1e-8):
    """k_rnn_adam on flat blocks: before / after = (parameters, exp_avg, exp_avg_sq); t: Adam's step index, from 1"""
    p, m, v = rr.adam(before[0], before[1], before[2], grads, lr, b1, b2, eps, t, torch_scalars=True)
    rec.hold(after[0], p, "k_rnn_adam.param")
    rec.hold(after[1], m, "k_rnn_adam.exp_avg")
    rec.hold(after[2], v, "k_rnn_adam.exp_avg_sq")


def chain(P, c, x, tg, mk, drop=None):
    """the restatements end to end in float64 on float64 operands -> (loss, {tensor: gradient}) as plain arrays"""
    H, L, nb = c["H"], c["L"], len(c["hidden"]) - 1
    P = {k: BV(np.asarray(v, np.float64)) for k, v in P.items()}
    B, T, _ = x.shape
    x0 = BV(np.asarray(x, np.float64).reshape(B * T, -1))
    rows_t = [np.arange(B) * T + t for t in range(T)]

    def scatter(parts):                                   # T pieces of [B, cols] -> [B * T, cols]
        v = np.stack([q.v for q in parts], 1)
        return BV(v.reshape(B * T, -1))
    X, gru = x0, []
    for l in range(L):
        gi = matmul(X, P[f"rnn_layer.weight_ih_l{l}"], P[f"rnn_layer.bias_ih_l{l}"])
        h, steps = BV(np.zeros((B, H))), []
        for t in range(T):
            s = gru_cell(gi[rows_t[t]], h, P[f"rnn_layer.weight_hh_l{l}"], P[f"rnn_layer.bias_hh_l{l}"])
            s["hp"], h = h, s["h"]
            steps.append(s)
        gru.append(dict(X=X, steps=steps))
        X = scatter([s["h"] for s in steps])
    p, eps = BV(np.float64(c["p"])), BV(np.float64(EPS_LN))          # the doubles of the float64 oracle and of torch

    def block(slot, Xin, res, key):
        zp = matmul(Xin, P[key + ".linear.weight"], P[key + ".linear.bias"])
        u = dropout_res(swish(zp), None if drop is None else BV(np.asarray(drop[slot], np.float64)), p, res)
        return layer_norm(u, P[key + ".layer_norm.weight"], P[key + ".layer_norm.bias"], eps), dict(Xin=Xin, zp=zp, u=u, key=key, slot=slot)
    yin, cin = block(0, x0, None, "input_layer")
    ct = cat([yin, X])
    zm = matmul(ct, P["merge_layer.weight"], P["merge_layer.bias"])
    y, blocks = swish(zm), []
    for i in range(nb):
        y, cb = block(1 + i, y, y, f"backbones.{i}")
        blocks.append(cb)
    pred = matmul(y, P["output_layer.weight"], P["output_layer.bias"])
    lo, dpred = loss(pred, BV(np.asarray(tg, np.float64).reshape(B * T, -1)), BV(np.asarray(mk, np.float64).reshape(-1, 1)))
    G = {}

    def lin_grad(wk, bk, dY, Xin):
        G[wk], G[bk] = (a.v for a in wgrad(dY, Xin))
    lin_grad("output_layer.weight", "output_layer.bias", dpred, y)
    dys = [matmul(dpred, tr(P["output_layer.weight"]))]

    def block_bwd(cb, dys):
        key = cb["key"]
        ref = ln_bwd(dys, cb["u"], P[key + ".layer_norm.weight"], None if drop is None else BV(np.asarray(drop[cb["slot"]], np.float64)), p, cb["zp"], eps)
        G[key + ".layer_norm.weight"], G[key + ".layer_norm.bias"] = ref["pg"].v.sum(0), ref["pb"].v.sum(0)
        lin_grad(key + ".linear.weight", key + ".linear.bias", ref["dz"], cb["Xin"])
        return [ref["du"], matmul(ref["dz"], tr(P[key + ".linear.weight"]))]
    for i in range(nb - 1, -1, -1):
        dys = block_bwd(blocks[i], dys)
    dzm = swish_bwd(dys[0], dys[1], zm)
    lin_grad("merge_layer.weight", "merge_layer.bias", dzm, ct)
    dcat = matmul(dzm, tr(P["merge_layer.weight"]))
    block_bwd(cin, [dcat[:, :H]])
    dout = dcat[:, H:]
    for l in range(L - 1, -1, -1):
        carry, gis, ghs = BV(np.zeros((B, H))), [None] * T, [None] * T
        for t in range(T - 1, -1, -1):
            s = gru[l]["steps"][t]
            gis[t], ghs[t], carry = gru_bwd_cell(dout[rows_t[t]], carry, s["r"], s["z"], s["n"], s["hn"], s["hp"], P[f"rnn_layer.weight_hh_l{l}"])
        dgi, dgh = scatter(gis), scatter(ghs)
        lin_grad(f"rnn_layer.weight_hh_l{l}", f"rnn_layer.bias_hh_l{l}", dgh, scatter([s["hp"] for s in gru[l]["steps"]]))
        lin_grad(f"rnn_layer.weight_ih_l{l}", f"rnn_layer.bias_ih_l{l}", dgi, gru[l]["X"])
        dout = matmul(dgi, tr(P[f"rnn_layer.weight_ih_l{l}"]))
    return float(lo.v), pred.v.reshape(B, T, -1), G
