"""The case table of the dynamics-kernel tests: the shapes that tests/test_gpu_dyn_kernels.py runs on the engine and that
tests/test_dyn_refs_cpu.py synthesises head operands for, so that the module that proves the bound and the module that uses it see the
same edges.  Everything moves one edge at a time from BASE.  Test infrastructure (numpy only)."""
import numpy as np

f32 = np.float32

BASE = dict(od=3, ad=2, hidden=(32, 32), K=3, elites=(2, 0), B=64, R=1, with_reward=1, decays=(0.0, 0.1, 5e-4), lr=1e-3, coef=0.01)


def case(**kw):
    c = dict(BASE, **kw)
    c["D"] = c["od"] + (1 if c["with_reward"] else 0)
    return c


K64 = dict(K=64, elites=(63, 5), hidden=(8,), decays=(0.1, 5e-4))
# obs_dim / act_dim and member-count edges (D = 2, 3, 5, 64: op = rup4(2 D) with 2 D = 6, 10 no multiple of 4; in = 2 with two pad columns,
# in = 65 with pitch 68; K * rows < 64 at K 1; lane < K covering the wave at K 64)
SHAPES = {
    "base": case(), "od1": case(od=1, ad=1), "od2": case(od=2, ad=1), "od4": case(od=4, ad=2), "od63": case(od=63, ad=2),
    "K1": case(K=1, elites=(0,)), "K64": case(**K64),
    "elite_last": case(elites=(2,)), "elite_all": case(elites=(1, 2, 0)),
}
# value edges of soft_clamp / softplus: max - raw ("y1") or l1 - min ("y2") on these values across the D = 9 columns
EDGE_Y = np.array([-30.0, -20.5, -20.0, -19.5, 0.0, 19.5, 20.0, 20.5, 30.0])
EDGE = case(od=8, ad=2, R=2)

# ---- learn_epoch: (id, case, train size, extras) ----
LEARN = [
    ("train37", case(), 37, {}), ("train1", case(), 1, {}), ("train64", case(), 64, {}),
    ("train64+5", case(lr=0.0), 69, {}),                 # lr 0 keeps the parameters the last minibatch read
    ("train300", case(B=300), 300, {}),
    ("od1", SHAPES["od1"], 37, {}), ("od2", SHAPES["od2"], 37, {}), ("od4", SHAPES["od4"], 37, {}), ("od63", SHAPES["od63"], 37, {}),
    ("noreward", case(od=5, with_reward=0), 37, {}),
    ("K1", SHAPES["K1"], 37, {}), ("K64", SHAPES["K64"], 3, {}),
    ("runs3", case(R=3), 37, dict(active=[1, 0, 1], t0=[3, 7, 11], moments=True)),
    ("adam_t0", case(), 37, dict(t0=[0], moments=True)), ("adam_t1", case(), 37, dict(t0=[1], moments=True)),
    ("adam_t999", case(), 37, dict(t0=[999], moments=True)), ("adam_t1e6", case(), 37, dict(t0=[10 ** 6], moments=True)),
    ("edge", EDGE, 40, dict(edge=True)),
]
# ---- step: (id, case, n, extras); every case runs the three penalty modes ----
STEP = [(k, SHAPES[k], 37, {}) for k in ("base", "od1", "od2", "od4", "od63", "K1", "K64", "elite_last", "elite_all")] + \
       [("n%d" % n, case(), n, {}) for n in (1, 255, 256, 257)] + \
       [("runs2", case(R=2), 37, {}), ("coef0", case(), 37, dict(step_coef=0.0)), ("edge", EDGE, 40, dict(edge=True))]
# ---- sample_next: (id, case, n, num_samples) ----
SAMPLE = [("S1", case(), 65, 1), ("S3", case(), 1, 3), ("E=K", SHAPES["elite_all"], 65, 3), ("od1", case(od=1, ad=1), 65, 3),
          ("od4", SHAPES["od4"], 1, 1), ("od63", SHAPES["od63"], 65, 3)]
# ---- adv_forward + adv_update: (id, case, Ba, Bs, extras).  wpb = max(1, min(4, 32768 // (8 (K D + 64)))) waves per workgroup ----
ADV = [
    ("1x1", case(), 1, 1, {}),                           # K D = 12: wpb 4, one workgroup with two invalid waves
    ("37x29", case(), 37, 29, {}),                       # wpb 4, 66 rows: the last workgroup has two invalid waves
    ("5x64", case(), 5, 64, {}),                         # wpb 4, 69 rows: three invalid waves
    ("130x3", case(), 130, 3, {}),                       # wpb 4, 133 rows; three trips of the adversarial means' lane loop
    ("KD2", case(od=1, ad=1, K=1, elites=(0,)), 37, 29, {}),                  # K D = 2: wpb 4
    ("KD63", case(od=2, ad=1, K=21, elites=(20, 0, 7)), 7, 6, {}),           # K D = 63: wpb 4, one trip of the lane loop, one lane idle
    ("KD65", case(od=4, ad=2, K=13, elites=(12, 3)), 7, 6, {}),              # K D = 65: wpb 4, second trip with one lane
    ("KD448", case(od=63, ad=2, K=7, elites=(6, 1, 2)), 7, 6, {}),           # K D = 448: wpb 4 (8 * 512 = 4096 bytes a wave), 7 trips
    ("KD1344", case(od=20, ad=2, **K64), 5, 4, {}),                          # K D = 1344: wpb 2 (11264 bytes a wave), 9 rows: one invalid wave
    ("KD4096", case(od=63, ad=2, **K64), 3, 2, {}),                          # K D = 4096: wpb 1 (33280 bytes a wave), 64 trips
    ("elite_last", SHAPES["elite_last"], 37, 29, {}), ("elite_all", SHAPES["elite_all"], 37, 29, {}),
    ("w0", case(), 37, 29, dict(adv_weight=0.0)), ("w1", case(), 37, 29, dict(adv_weight=1.0)),
    ("runs2", case(R=2), 37, 29, dict(active=[0, 1])),
    ("adam_t1e6", case(), 37, 29, dict(t0=10 ** 6)),
    ("edge", EDGE, 12, 40, dict(edge=True)),
]


def adv_wpb(K, D):
    return max(1, min(4, 32768 // (8 * (K * D + 64))))


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def logvar_bounds(rng, D):
    """(max_logvar, min_logvar): close enough that both soft clamps act on ordinary outputs"""
    return (0.5 + 0.3 * rng.normal(size=D)).astype(f32), (-3.0 + 0.5 * rng.normal(size=D)).astype(f32)


def scaler(rng, n_in):
    """a non-identity scaler: mu of order 1, std between 1e-2 and 1e2 per column"""
    return rng.normal(size=n_in).astype(f32), (10.0 ** rng.uniform(-2, 2, size=n_in)).astype(f32)


def edge_head(variant, D=9):
    """(mean bias, raw-logvar bias, max_logvar, min_logvar) [D] of a constant head that puts max - raw (variant "y1") or l1 - min
    (variant "y2") exactly on EDGE_Y: every value is a multiple of 0.5, so the fp32 subtractions are exact"""
    assert D == EDGE_Y.size
    mean = 0.25 * np.arange(D)
    mx = np.full(D, 0.5)
    if variant == "y1":
        raw, mn = mx - EDGE_Y, np.full(D, -10.0)
    else:
        raw = mx - 25.0                       # softplus(25) = 25: l1 = raw
        mn = raw - EDGE_Y
    return mean.astype(f32), raw.astype(f32), mx.astype(f32), mn.astype(f32)


def edge_targets(rng, variant, rows):
    """targets [rows, D] against the constant head, by row % 4: the mean itself (diff = 0); diff^2 exp(-lv) within 1e-3 of 1;
    1e3 away (at the lower logvar bound in the columns where lv = min_logvar); ordinary"""
    mean, raw, mx, mn = (a.astype(np.float64) for a in edge_head(variant))
    sp = lambda y: np.where(y > 20, y, np.log1p(np.exp(np.minimum(y, 20))))
    lv = mn + sp(mx - sp(mx - raw) - mn)
    t = np.tile(mean, (rows, 1))
    j = np.arange(rows) % 4
    t[j == 1] += np.sqrt(np.exp(lv)) * (1.0 + 4e-4) * np.where(rng.random((int((j == 1).sum()), mean.size)) < 0.5, -1.0, 1.0)
    t[j == 2] += 1e3
    t[j == 3] += rng.normal(size=(int((j == 3).sum()), mean.size))
    return t.astype(f32)


def head_operands(rng, c, rows, edge=None):
    """CPU stand-ins for one run's engine read-backs at case c: out [K, rows, 2D], targets [K, rows, D], max / min_logvar"""
    K, D = c["K"], c["D"]
    if edge:
        mean, raw, mx, mn = edge_head(edge)
        out = np.tile(np.concatenate([mean, raw])[None, None], (K, rows, 1)).astype(f32)
        t = np.stack([edge_targets(rng, edge, rows) for _ in range(K)])
        return out, t, mx, mn
    mx, mn = logvar_bounds(rng, D)
    out = np.concatenate([rng.normal(size=(K, rows, D)), -1.5 + 2.5 * rng.normal(size=(K, rows, D))], -1).astype(f32)
    t = (out[..., :D] + 0.7 * rng.normal(size=(K, rows, D))).astype(f32)
    return out, t, mx, mn
