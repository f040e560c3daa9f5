"""Self-bounding float64 restatements of RNNDynamics' one-step path (csrc/rnn_dynamics.hip: k_rnn_roll_in, k_rnn_cell, the tail of the
window forward on n rows, k_rnn_roll_head), written from the reference's formulas (nets/rnn.py: ``RNNModel.forward(input, h_state)``
one time step at a time; torch's GRU cell; ``StandardScaler.transform``) on tests/row_refs.py's ``BV`` with tests/rnn_refs.py's
``matmul`` / ``layer_norm``.  ``check_step`` holds every stage of one step to its restatement ON THE STAGE'S OWN OPERANDS as read
back, |got - ref.v| <= FACTOR * ref.e on every element; copies (the new h into its slot, the reward column) and untouched slots are
held bit for bit.  ``carried`` runs the restatements end to end in float64, which is what ties them to the oracle's window forward;
``emulate`` is an fp32 numpy stand-in for the engine with switchable defects, which is what shows that the checks can fail.

Shapes of the GPU test (in / out / H / L / n_traj -> rows / runs): the smallest at which each guard of k_rnn_cell changes."""
import numpy as np

import rnn_oracle as ro
import rnn_refs as rf
import row_refs as rr
from row_refs import BV

f32 = np.float32
CASES = {
    # name: (in, out, H, L, n_traj, rows, runs)
    "one": (5, 4, 8, 1, 1, 1, 1),             # one row, half a unit tile, K = 5
    "tile": (7, 5, 20, 2, 16, 16, 1),         # a full row tile, a partial second unit tile, K = 7 then 20
    "default": (14, 12, 200, 3, 37, 17, 1),   # the default widths: a second row tile of one row, 13 unit tiles, a thinned index
    "wide": (14, 12, 512, 4, 33, 33, 1),      # the maximum: three row tiles, 32 unit tiles, four layers
    "runs": (6, 4, 72, 2, 20, 9, 2),          # two runs, one stepped alone and both together
}
DEFECTS = ("no_carry", "wrong_slot", "r_before_bhn", "inplace", "reward_swap", "std_ignored", "other_slots_zeroed", "h_to_row_slot")


def case(name):
    nin, nout, H, L, n_traj, rows, runs = CASES[name]
    return dict(name="roll_" + name, input_dim=nin, output_dim=nout, hidden=[H, H, H], H=H, L=L, p=0.0, n_traj=n_traj, rows=rows, runs=runs,
                seed=8200 + sum(name.encode()), obs_dim=nout - 1, act_dim=nin - (nout - 1))


def make_inputs(c, seed=0):
    """planted state [L, n_traj, H] in (-1, 1), obs / act of the rows, a scrambled non-monotone index, a scaler (mu != 0, std != 1)"""
    rng = np.random.RandomState(c["seed"] + 3 + seed)
    state = rng.uniform(-1.0, 1.0, size=(c["L"], c["n_traj"], c["H"])).astype(f32)
    obs = rng.standard_normal((c["rows"], c["obs_dim"])).astype(f32)
    act = np.tanh(rng.standard_normal((c["rows"], c["act_dim"]))).astype(f32)
    index = rng.permutation(c["n_traj"])[:c["rows"]].astype(np.int64)
    if c["rows"] >= 3 and np.all(np.diff(index) > 0):
        index[[0, -1]] = index[[-1, 0]]
    mu = (0.2 * rng.standard_normal(c["input_dim"])).astype(f32)
    std = (0.7 + 0.6 * rng.uniform(size=c["input_dim"])).astype(f32)
    return state, obs, act, index, mu, std


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def scale(obs, act, mu, std):
    """k_rnn_roll_in: ([obs | act] - mu) / std, a subtraction and a division"""
    return (rf.cat([obs, act]) - BV.exact(mu)) / BV.exact(std)


def cell(x, hp, wih, bih, whh, bhh):
    """k_rnn_cell: torch's GRU cell with the input projection folded in.  The r and z pre-activations are ONE product over [x | h]
    (any order of its K_in + H terms) plus the two biases; n keeps W_in x + b_in and W_hn h + b_hn apart, r multiplies the latter"""
    x, hp = BV.exact(x), BV.exact(hp)
    H = hp.shape[1]
    wih, whh, bih, bhh = (np.asarray(a.v if isinstance(a, BV) else a) for a in (wih, whh, bih, bhh))
    exact = BV if wih.dtype == np.float64 else BV.exact
    pre = rf.matmul(rf.cat([x, hp]), exact(np.concatenate([wih[:2 * H], whh[:2 * H]], 1))) + exact(bih[:2 * H]) + exact(bhh[:2 * H])
    r, z = rf.sigmoid(pre[:, :H]), rf.sigmoid(pre[:, H:])
    nx = rf.matmul(x, exact(wih[2 * H:]), exact(bih[2 * H:]))
    hn = rf.matmul(hp, exact(whh[2 * H:]), exact(bhh[2 * H:]))
    n = rr.tanh(nx + r * hn)
    return (1.0 - z) * n + z * hp


def head(pred, obs):
    """k_rnn_roll_head: next_obs = pred[:, :-1] + obs"""
    return BV.exact(pred)[:, :-1] + BV.exact(obs)


def tail(P, c, x, htop, eps=None, quant=False):
    """the tail of RNNModel on rows: the input block on x, the merge layer on [its output | the top layer's h], the residual blocks,
    the head -> {tap name: BV}; every stage from the stage before (end to end).  quant: every stage's result is rounded to fp32 before
    the next one reads it, as stored matrices are (``emulate``)"""
    nb = len(c["hidden"]) - 1
    eps = rf.EPS_LN if eps is None else eps
    q = (lambda b: BV.exact(b.v.astype(f32))) if quant else (lambda b: b)
    out = {}

    def block(slot, Xin, res, key, name):
        act = q(rf.swish(rf.matmul(Xin, P[key + ".linear.weight"], P[key + ".linear.bias"])))
        u = q(rf.dropout_res(act, None, c["p"], res))
        out[f"act.{slot}"], out[f"drop.{slot}"] = act, u
        out[name] = q(rf.layer_norm(u, P[key + ".layer_norm.weight"], P[key + ".layer_norm.bias"], eps))
        return out[name]
    yin = block(0, x, None, "input_layer", "in")
    y = out["merge"] = q(rf.swish(rf.matmul(rf.cat([yin, htop]), P["merge_layer.weight"], P["merge_layer.bias"])))
    for i in range(nb):
        y = block(1 + i, y, y, f"backbones.{i}", f"block.{i}")
    out["pred"] = q(rf.matmul(y, P["output_layer.weight"], P["output_layer.bias"]))
    return out


def carried(P, c, xs, h0=None):
    """k carried single steps in float64 on float64 operands: xs [B, k, in] (scaled), h0 [L, B, H] or None for zero ->
    (pred [B, k, out], h [L, B, H]) as plain arrays"""
    P = {k: BV(np.asarray(v, np.float64)) for k, v in P.items()}
    B, k, _ = xs.shape
    h = [BV(np.zeros((B, c["H"])) if h0 is None else np.asarray(h0[l], np.float64)) for l in range(c["L"])]
    preds = []
    for t in range(k):
        X = BV(np.asarray(xs[:, t], np.float64))
        x0 = X
        for l in range(c["L"]):
            h[l] = cell(X, h[l], P[f"rnn_layer.weight_ih_l{l}"], P[f"rnn_layer.bias_ih_l{l}"], P[f"rnn_layer.weight_hh_l{l}"],
                        P[f"rnn_layer.bias_hh_l{l}"])
            h[l] = BV(h[l].v)
            X = h[l]
        preds.append(tail(P, c, x0, X, BV(np.float64(rf.EPS_LN)))["pred"].v)
    return np.stack(preds, 1), np.stack([a.v for a in h])


def window_state(P, c, xs):
    """the oracle's float64 window forward over xs [B, T, in]: (pred [B, T, out], h of every layer after the last step [L, B, H])"""
    pred, cache = ro.forward(P, c, xs, dtype=np.float64)
    B, T, _ = xs.shape
    return pred, np.stack([cache["taps"][f"gru.{l}"].reshape(B, T, -1)[:, -1] for l in range(c["L"])])


# ---- the per-element check of one step ---------------------------------------------------------------------------------------------------
def check_step(rd, P, c, before, obs, act, index, mu, std, next_obs, reward, rec):
    """every stage of one step on its own operands.  rd(name) -> [rows, cols]: roll.x, roll.h.<l>, state.<l> (AFTER the step,
    [n_traj, H]), act.<s>, drop.<s>, in, merge, block.<i>, roll.pred; before: the state [L, n_traj, H] the step started from"""
    rd = rf.reader(rd)
    L, nb, n_traj = c["L"], len(c["hidden"]) - 1, before.shape[1]
    index = np.arange(len(obs)) if index is None else np.asarray(index)
    rest = np.setdiff1d(np.arange(n_traj), index)
    x = rd("roll.x")
    rec.hold(x, scale(obs, act, mu, std), "k_rnn_roll_in.x")
    X = x
    for l in range(L):
        h = rd(f"roll.h.{l}")
        ref = cell(X, before[l][index], P[f"rnn_layer.weight_ih_l{l}"], P[f"rnn_layer.bias_ih_l{l}"], P[f"rnn_layer.weight_hh_l{l}"],
                   P[f"rnn_layer.bias_hh_l{l}"])
        rec.hold(h, ref, "k_rnn_cell.h", l)
        after = rd(f"state.{l}")
        rec.hold(after[index], ref, "k_rnn_cell.state", l)
        rec.same(after[index], h, "k_rnn_cell.state_is_h", l)
        rec.same(after[rest], before[l][rest], "k_rnn_cell.other_slots", l)
        X = h

    def block(slot, Xin, res, key, name):
        a, u = rd(f"act.{slot}"), rd(f"drop.{slot}")
        rec.hold(a, rf.swish(rf.matmul(Xin, P[key + ".linear.weight"], P[key + ".linear.bias"])), "tail.act", slot)
        rec.hold(u, rf.dropout_res(a, None, c["p"], res), "tail.drop", slot)
        rec.hold(rd(name), rf.layer_norm(u, P[key + ".layer_norm.weight"], P[key + ".layer_norm.bias"]), "tail.norm", slot)
        return rd(name)
    yin = block(0, x, None, "input_layer", "in")
    y = rd("merge")
    rec.hold(y, rf.swish(rf.matmul(np.concatenate([yin, X], 1), P["merge_layer.weight"], P["merge_layer.bias"])), "tail.merge")
    for i in range(nb):
        y = block(1 + i, y, y, f"backbones.{i}", f"block.{i}")
    pred = rd("roll.pred")
    rec.hold(pred, rf.matmul(y, P["output_layer.weight"], P["output_layer.bias"]), "tail.pred")
    rec.hold(next_obs, head(pred, obs), "k_rnn_roll_head.next_obs")
    rec.same(np.asarray(reward).reshape(-1), pred[:, -1], "k_rnn_roll_head.reward")


# ---- an fp32 stand-in for the engine, with defects ---------------------------------------------------------------------------------------
def emulate(P, c, state, obs, act, index, mu, std, defect=None):
    """one step in numpy float32 -> (taps, next_obs, reward); ``state`` [L, n_traj, H] is updated in place as the engine's is.
    defect: one of DEFECTS, what a wrong kernel would do"""
    assert defect is None or defect in DEFECTS, defect
    H, L = c["H"], c["L"]
    index = np.arange(len(obs)) if index is None else np.asarray(index)
    n = len(obs)
    taps = {}
    xin = np.concatenate([obs, act], 1).astype(f32)
    x = (xin - mu).astype(f32) if defect == "std_ignored" else ((xin - mu).astype(f32) / std).astype(f32)
    taps["roll.x"] = x
    X = x
    slots = np.arange(n) if defect == "wrong_slot" else index
    for l in range(L):
        wih, whh = P[f"rnn_layer.weight_ih_l{l}"], P[f"rnn_layer.weight_hh_l{l}"]
        bih, bhh = P[f"rnn_layer.bias_ih_l{l}"], P[f"rnn_layer.bias_hh_l{l}"]
        hnew = np.zeros((n, H), f32)
        for j0 in range(0, H, 16):                        # a unit tile at a time, as the workgroups of a row
            j = np.arange(j0, min(j0 + 16, H))
            hp = np.zeros((n, H), f32) if defect == "no_carry" else state[l][slots]
            gi = (X @ wih.T + bih).astype(f32)
            gh = (hp @ whh.T).astype(f32)
            r = ro._sig((gi[:, j] + gh[:, j] + bhh[j]).astype(f32))
            z = ro._sig((gi[:, H + j] + gh[:, H + j] + bhh[H + j]).astype(f32))
            if defect == "r_before_bhn":
                nn = np.tanh(gi[:, 2 * H + j] + r * gh[:, 2 * H + j] + bhh[2 * H + j])
            else:
                nn = np.tanh(gi[:, 2 * H + j] + r * (gh[:, 2 * H + j] + bhh[2 * H + j]))
            hnew[:, j] = ((1 - z) * nn + z * hp[:, j]).astype(f32)
            if defect == "inplace":                       # the tile's units land in the row its neighbours are still reading
                state[l][slots[:, None], j[None, :]] = hnew[:, j]
        if defect == "other_slots_zeroed":
            state[l][np.setdiff1d(np.arange(state.shape[1]), index)] = 0
        state[l][np.arange(n) if defect == "h_to_row_slot" else index] = hnew
        taps[f"roll.h.{l}"] = hnew
        X = hnew
    Pf = {k: np.asarray(v, f32) for k, v in P.items()}
    for k, v in tail(Pf, c, x, X, quant=True).items():
        taps["roll.pred" if k == "pred" else k] = v.v.astype(f32)
    pred = taps["roll.pred"]
    if defect == "reward_swap":
        return taps, (pred[:, 1:] + obs).astype(f32), pred[:, 0].copy()
    return taps, (pred[:, :-1] + obs).astype(f32), pred[:, -1].copy()


def emulated_reader(taps, state):
    def rd(name):
        return state[int(name[6:])] if name.startswith("state.") else taps[name]
    return rd
