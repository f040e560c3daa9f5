"""CPU: the references and check functions of tests/test_gpu_diffusion_wide.py, proven before they judge a kernel.  The float64 oracle
against float64 autograd of ``nets.ConditionalUnet1D`` on every wide case (the gap must stay below a quarter of D32, so it cannot eat
the bar); every case a legal engine configuration without a one-channel group; the e0 and Adam / EMA restatements around numpy's own
fp32 evaluation; the check functions pass on the clean fp32 oracle and fail on six planted defects; the sampling inputs clip on both
sides."""
import numpy as np
import pytest
import torch

import diffusion_cases as dc
import diffusion_oracle as orc
import diffusion_wide_cases as wc
import row_refs as rr
from helpers import scale_err


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def test_every_case_is_a_legal_engine_configuration_without_a_one_channel_group():
    want = {"A": [8, 64, 65, 128], "B": [64, 512], "C": [33, 66], "D": [3, 4], "E": [3, 4], "F": [3, 4], "G": [33, 66], "H": [4, 8], "I": [3, 8]}
    for name, c in wc.CASES.items():
        assert wc.legal(c) is None, (name, wc.legal(c))
        assert min(wc.group_widths(c)) > 1, name
        if name in want:
            assert wc.group_widths(c) == want[name], (name, wc.group_widths(c))
    assert "wider than 512" in wc.legal(dict(wc.CASES["B"], down_dims=[520]))
    assert "n_groups must be in [1, 16]" in wc.legal(dict(wc.CASES["C"], n_groups=17, down_dims=[17 * 8]))
    # the batches: both ends of t in every batch, F with its short batch of 10
    for name in wc.STEP_CASES:
        c = wc.CASES[name]
        for idx, t, eps in wc.make_batches(c, 2):
            assert t[0] == 0 and t[1] == c["N"] - 1 and len(idx) >= 2
    assert [len(b[0]) for b in wc.reference("F")["batches"]] == [90, 10]
    # gradient terms a block's backward sums (the engine's DIFF_MAX_TERMS = 4): an increasing net reaches 3 (the last down block feeds an
    # identity mid block twice and a skip), H reaches 4 and has an identity residual that reads a concatenation
    def terms(c):
        plan, last = orc.block_plan(c["act_dim"], c["down_dims"])
        n = [0] * len(plan)
        n[last] += 1
        for nm, cin, cout, src, skip in plan:
            if src >= 0:
                n[src] += 1 + (cin == cout)
            if skip >= 0:
                n[skip] += 1 + (cin == cout)
        return max(n), any(skip >= 0 and cin == cout for nm, cin, cout, src, skip in plan)
    assert terms(wc.CASES["H"]) == (4, True) and terms(wc.CASES["I"])[0] == 3 and terms(wc.CASES["A"]) == (3, False)


# ---- the float64 oracle against float64 autograd -------------------------------------------------------------------------------------
def _autograd64(ref, batch):
    from offlinerlkit.nets import ConditionalUnet1D
    c, P = ref["c"], ref["P"]
    obs, act = ref["data"]
    idx, t, eps = batch
    net = ConditionalUnet1D(c["act_dim"], c["obs_dim"], **dc.net_kwargs(c))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    net = net.double()
    e0 = []
    net.diffusion_step_encoder[0].register_forward_hook(lambda m, i, o: e0.append(o.numpy()) or o.double())   # fp32 by definition
    acp = orc.alphas_cumprod(c["N"])
    xt = (np.sqrt(acp[t])[:, None] * act[idx] + np.sqrt(np.float32(1.0) - acp[t])[:, None] * eps).astype(np.float32)
    pred = net(torch.from_numpy(xt).unsqueeze(1).double(), torch.from_numpy(t), global_cond=torch.from_numpy(obs[idx]).double())
    loss = torch.nn.functional.mse_loss(pred, torch.from_numpy(eps).unsqueeze(1).double())
    loss.backward()
    return loss.item(), pred.detach().numpy()[:, 0], wc.centre_taps({k: p.grad.numpy() for k, p in net.named_parameters()}), e0[0]


@pytest.mark.parametrize("name", wc.STEP_CASES)
def test_float64_oracle_matches_float64_autograd(name):
    """the oracle is fed autograd's own fp32 embedding (torch's sin and numpy's differ in the last bit), as the GPU test feeds it the
    engine's: everything downstream of e0 is then the same function on the same input"""
    ref = wc.reference(name)
    for i, (batch, D32) in enumerate(zip(ref["batches"], ref["D32"])):
        loss, pred, grads, e0 = _autograd64(ref, batch)
        assert e0.dtype == np.float32 and scale_err(e0, ref["o64"][i]["e0"]) < 1e-5
        o64 = wc.run_oracle(ref["P"], ref["c"], ref["data"], batch, np.float64, e0=e0)
        gap, noise = orc.grad_distance(o64["grads"], grads)
        gap_pred, gap_loss = scale_err(o64["pred"], pred), abs(o64["loss"] - loss) / abs(loss)
        print(f"{name} ({len(batch[0])} rows): oracle - autograd {gap:.2e} (gradients), {gap_pred:.2e} (pred), {gap_loss:.2e} (loss); "
              f"D32 {D32['grads']:.2e} / {D32['pred']:.2e}; pred ptp {np.ptp(o64['pred'], axis=0).max():.2f}")
        assert noise == 0.0 and D32["noise"] == 0.0 and sorted(grads) == sorted(o64["grads"])          # every tensor has a gradient
        assert gap < 0.25 * D32["grads"], (gap, D32["grads"])
        assert gap_pred < 0.25 * D32["pred"] and gap_loss < 0.25 * D32["pred"]      # (a scalar's own fp32 distance may be 0 by luck)
        assert np.ptp(o64["pred"], axis=0).max() > 0.1                                # the output depends on the row
        assert np.array_equal(o64["x_t"], ref["o32"][i]["x_t"])


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsed,N", [(4, 10), (16, 10), (130, 10), (256, 10), (256, 100)])
def test_e0_bound_holds_numpys_fp32_embedding_and_is_first_order_small(dsed, N):
    t = np.arange(N)
    ref = orc.sinusoidal_ref(t, dsed)
    got = orc.sinusoidal(t, dsed, np.float32)
    half = dsed // 2
    assert ref.shape == got.shape == (N, dsed)
    assert rr.ratio(got, ref) <= rr.FACTOR
    # j = 0: the argument is the integer t, only the library call rounds
    assert np.array_equal(ref.v[:, 0], np.sin(t.astype(np.float64))) and (ref.e[:, 0] <= 2 * rr.U + rr.TINY).all()
    # elsewhere: the exponent j step carries 3 u (constant, division, product), the exponential turns that into 3 u j step <= 3 u ln 1e4
    # relative and adds its own 2 u, t f adds 1 u: at most (3 ln 1e4 + 3) u t on the argument, plus the sine's own 2 u
    assert (ref.e <= (3 * np.log(1e4) + 3) * rr.U * t[:, None] + 2 * rr.U + 4 * rr.TINY).all()
    # the bound has teeth: a frequency table with half in place of half - 1, or sin and cos swapped, is far outside
    if half > 2:
        wrong = np.exp(np.arange(half) * -(np.log(1e4) / half))
        assert rr.ratio(np.concatenate([np.sin(t[:, None] * wrong), np.cos(t[:, None] * wrong)], 1), ref) > 100 * rr.FACTOR
    assert rr.ratio(np.concatenate([got[:, half:], got[:, :half]], 1), ref) > 100 * rr.FACTOR


def test_ema_cap_starts_at_optimizer_step_215444():
    assert orc.ema_decay(215443) < 0.9999 and orc.ema_decay(215444) == 0.9999 == orc.ema_decay(1000000)
    assert 1.0 - (1.0 + 215443) ** -0.75 >= 0.9999 > 1.0 - (1.0 + 215442) ** -0.75
    assert {215443, 215444} <= set(wc.ADAM_STEPS)


@pytest.mark.parametrize("k", wc.ADAM_STEPS)
def test_adam_ema_restatement_and_its_planted_defects(k):
    before = wc.adam_blocks(5000, 7 + k % 97)
    g = (1e-3 * np.random.RandomState(k % 89).standard_normal(5000)).astype(np.float32)
    lr = wc.lr_table_for(k)
    assert len(lr) == k + 1 and (k == 0 or lr[k - 1] == 0.5 * lr[k])
    clean = orc.adam_ema_f32(*before, g, lr[k], k)
    r = wc.check_adam_ema(clean, before, g, lr[k], k, "fp32 oracle")
    assert max(r.values()) <= 1.0
    assert orc.ema_decay(k) == (0.0 if k < 2 else min(1.0 - float(k) ** -0.75, 0.9999))
    if k >= 1:                                                  # lr[k - 1] used for lr[k]
        with pytest.raises(AssertionError, match="params"):
            wc.check_adam_ema(orc.adam_ema_f32(*before, g, lr[k - 1], k), before, g, lr[k], k, "planted")
    if k == 1000000:                                            # the EMA decay without its cap
        with pytest.raises(AssertionError, match="ema"):
            wc.check_adam_ema(orc.adam_ema_f32(*before, g, lr[k], k, decay=1.0 - float(k) ** -0.75), before, g, lr[k], k, "planted")
    if k == 1:                                                  # the bias corrections of step k in place of k + 1
        with pytest.raises(AssertionError):
            wc.check_adam_ema(orc.adam_ema_f32(*before, g, lr[k], k - 1, decay=orc.ema_decay(k)), before, g, lr[k], k, "planted")


# ---- the check functions: clean fp32 oracle passes, planted defects fail ---------------------------------------------------------------
def _first_64_stats(h, gamma, beta, G):
    """GroupNorm whose statistics see only the first 64 channels of a group (a statistics loop without its j >= 1 slabs)"""
    B, C = h.shape
    hg = h.reshape(B, G, C // G)
    mean = hg[:, :, :64].mean(axis=2, keepdims=True)
    var = ((hg[:, :, :64] - mean) ** 2).mean(axis=2, keepdims=True)
    rstd = 1.0 / np.sqrt(var + h.dtype.type(1e-5))
    xh = ((hg - mean) * rstd).reshape(B, C)
    return xh * gamma + beta, (xh, rstd)


def _dgamma_without_last_slab(du, gamma, cache, G):
    dh, dg, db = _GN_BWD(du, gamma, cache, G)
    cg = du.shape[1] // G
    dg = dg.copy().reshape(G, cg)
    dg[:, 64 * ((cg - 1) // 64):] = 0.0
    return dh, dg.reshape(-1), db


_GN_BWD = orc.gn_bwd


@pytest.mark.parametrize("name", wc.STEP_CASES)
def test_check_step_passes_on_the_clean_fp32_oracle(name):
    ref = wc.reference(name)
    for o32, o64, D32 in zip(ref["o32"], ref["o64"], ref["D32"]):
        r = wc.check_step(o32, o64, D32, ref["c"], name)
        assert max(v for k, v in r.items() if k != "loss cell") == pytest.approx(1.0 / wc.BAR) and r["loss cell"] <= 1.0


@pytest.mark.parametrize("name,attr,defect,where", [
    ("A", "gn_fwd", _first_64_stats, "y1"), ("B", "gn_fwd", _first_64_stats, "y1"),
    ("A", "gn_bwd", _dgamma_without_last_slab, "grads"), ("B", "gn_bwd", _dgamma_without_last_slab, "grads"),
    ("C", "gn_bwd", _dgamma_without_last_slab, "grads"),                           # (the final norm's cg 66)
    ("A", "_skip_cols", lambda dX, c1: dX[:, :dX.shape[1] - c1], "grads"), ("H", "_skip_cols", lambda dX, c1: dX[:, :dX.shape[1] - c1], "grads"),
    ("I", "_skip_cols", lambda dX, c1: dX[:, :dX.shape[1] - c1], "grads"),
])
def test_check_step_fails_on_a_planted_defect(monkeypatch, name, attr, defect, where):
    ref = wc.reference(name)
    monkeypatch.setattr(orc, attr, defect)
    bad = wc.run_oracle(ref["P"], ref["c"], ref["data"], ref["batches"][0], np.float32)
    monkeypatch.undo()
    with pytest.raises(AssertionError, match=where):
        wc.check_step(bad, ref["o64"][0], ref["D32"][0], ref["c"], name + " planted")


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------
def test_sampling_inputs_clip_on_both_sides_and_the_check_sees_a_missing_clip(monkeypatch):
    s = wc.sample_reference(64)
    x0 = s["x0"]
    lo, hi = float((x0 < -1).mean()), float((x0 > 1).mean())
    print(f"x0 before the clip over {x0.shape}: {lo:.3f} below -1, {hi:.3f} above 1; D32 {s['D32']:.2e}")
    assert lo > 0 and hi > 0 and 0.1 <= lo + hi <= 0.9
    per_step = [float((np.abs(v) > 1).mean()) for v in x0]
    assert per_step[-1] > 0, per_step                           # also at t = 0, whose clipped x0 is the action
    assert wc.check_sample(s["a32"], s["a64"], s["D32"], "fp32 oracle") == pytest.approx(1.0 / wc.BAR)
    monkeypatch.setattr(orc, "_clip_x0", lambda x: x)           # clip at +-1 missing
    bad = orc.sample(s["P"], s["c"], s["obs"], s["noise"], s["z"])
    monkeypatch.undo()
    with pytest.raises(AssertionError, match="err / bar"):
        wc.check_sample(bad, s["a64"], s["D32"], "planted")
    # float64 sampling is the fp32 one widened: same schedule table, same clip
    assert scale_err(s["a32"], s["a64"]) < 1e-5 and np.abs(s["a64"]).max() <= 1.0
