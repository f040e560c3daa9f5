"""Cases of tests/test_gpu_mcq_edac_kernels.py (the MCQ row kernels and EDAC's gradient-diversity kernels held to the float64
restatements of tests/row_refs.py) -- shapes and value edges only, host arrays only: tests/test_mcq_edac_refs_cpu.py runs the numpy
oracle on the same inputs and requires it inside the restatements' bounds, which is the condition that the inputs are fair.

Every case is a keyword set of ``test_gpu_row_kernels.make`` / ``inputs``; one edge moves at a time from the base case."""
import numpy as np

f32 = np.float32


def _next(x, to):
    return float(np.nextafter(f32(x), f32(to)))


def case_id(d):
    return "-".join(f"{k}{v.__name__ if callable(v) else v}" for k, v in d.items() if k not in ("algo",)) or "base"


# ---------------------------------------------------------------------------------------------------------------------------------
# MCQ: base B = 32, A = 3, obs_dim = 5 (od + Z = 11: the decoder input rows carry one padding column), Z = 6, N = 3, one run, fp32,
# hidden [32, 32], VAE hidden 24
# ---------------------------------------------------------------------------------------------------------------------------------
MCQ_BASE = dict(B=32, A=3, od=5, Z=6, N=3, vae_hidden=24)
MCQ_SHAPES = [
    dict(),
    dict(B=1), dict(B=43), dict(B=129), dict(B=257),      # B Z = 258: second workgroup of k_vae_latent / k_vae_head_bwd; 2B > 256; B > 256 and B A = 771
    dict(A=1), dict(A=4), dict(A=32),                     # action pitch 4 without padding, 32; critic-input pitch 8 / 12 / 40
    dict(Z=1), dict(Z=5), dict(Z=64), dict(Z=7),          # od + Z = 6, 10, 69 (padded) and 12 (a multiple of four: no padding column)
    dict(N=1), dict(N=10),
    dict(max_action=0.5), dict(max_action=2.5),
    dict(mcq_lambda=0.7), dict(mcq_lambda=1.0), dict(mcq_lambda=0.0),
    dict(auto_alpha=0, alpha=0.2),
    dict(R=3),
    dict(precision=1), dict(B=257, precision=1), dict(vae_hidden=16, B=43, max_action=2.5),
]

LS_TABLE = [-4.0, _next(-4, -9), _next(-4, 9), 15.0, _next(15, -9), _next(15, 99), -10.0, 20.0]      # Z = 8: one column each
MEAN_TABLE = [0.0, 0.5, -0.5, 3.0, -3.0, 9.0, -20.0, 20.0]
Z_OOD_TABLE = [0.5, -0.5, _next(0.5, 1), _next(0.5, 0), _next(-0.5, -1), _next(-0.5, 0), 3.0, -3.0]


def constant_head_encoder(c):
    """zero head weights: the raw log-std of column j is LS_TABLE[j] on every row -- exactly on each clamp, one ulp outside and inside each, far
    beyond both -- and the mean MEAN_TABLE[j].  Where exp(15) = 3.3e6 is the std, the noise is 1e-6-sized beyond the first five rows (0, +-1,
    +-4 there), so that the decoder is not saturated on every row and dz std eps keeps its weight against the KL term in d log-std."""
    for st, n in zip(c.sts, c.noises):
        v = st["behavior_policy"]
        v["mean.weight"][:] = 0
        v["log_std.weight"][:] = 0
        v["log_std.bias"][:] = LS_TABLE[:c.Z]
        v["mean.bias"][:] = MEAN_TABLE[:c.Z]
        big = np.array(LS_TABLE[:c.Z]) > 10.0
        n["eps_vae"][:, big] *= f32(1e-6)
        n["eps_vae"][:5] = np.array([0.0, 1.0, -1.0, 4.0, -4.0], f32)[:, None]


def z_ood_on_and_beyond_the_clip(c):
    for n in c.noises:
        n["z_ood"][:16] = np.array(Z_OOD_TABLE, f32)[(np.arange(16)[:, None] + np.arange(c.Z)[None, :]) % 8]


def tied_target_critics(c):
    for st in c.sts:
        st["critic2_old"] = {k: v.copy() for k, v in st["critic1_old"].items()}


def saturated_decoder(c):
    """decoder outputs of +-30: tanh is exactly +-1 in fp32, 1 - tanh^2 and with it dm3 underflow to 0"""
    for st in c.sts:
        b = st["behavior_policy"]["d3.bias"]
        b[:] = np.where(np.arange(b.size) % 2 == 0, 30.0, -30.0).astype(f32)


def batch_edge(kind):
    def f(c):
        for b in c.batches:
            if kind == "terminal":
                b["terminals"][:] = 1
            elif kind == "alive":
                b["terminals"][:] = 0
            else:
                b["rewards"][:] = 1e3 * np.sign(b["rewards"] + f32(0.1))
    f.__name__ = kind
    return f


MCQ_EDGE_BASE = dict(B=64, Z=8)
MCQ_EDGES = [dict(mutate=constant_head_encoder), dict(mutate=z_ood_on_and_beyond_the_clip), dict(mutate=batch_edge("terminal")),
             dict(mutate=batch_edge("alive")), dict(mutate=tied_target_critics), dict(mutate=batch_edge("reward1e3")), dict(mutate=saturated_decoder)]


def mcq_kw(kw):
    base = dict(MCQ_BASE, **(MCQ_EDGE_BASE if "mutate" in kw else {}))
    return dict(base, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# EDAC with eta > 0: base B = 32, A = 3, obs_dim = 5, K = 4, hidden [32, 32], eta = 1.  ``vec``: whether k_edac_t0 (True) or the tiled GEMM
# with the mask epilogue (False) must make t_0; ``bits``: whether the mask must come from packed bits (the first hidden width is then a
# multiple of 128 -- only such activations have mask words) or from the stored activation
# ---------------------------------------------------------------------------------------------------------------------------------
EDAC_BASE = dict(B=32, A=3, od=5, K=4, hidden=(32, 32), eta=1.0)
EDAC_SHAPES = [
    dict(),
    dict(B=1), dict(B=7), dict(B=9), dict(B=33), dict(B=257),      # row clamp of an 8-row wave block; a part-filled block of four waves; second trip of k_edac_gamma
    dict(A=1), dict(A=7), dict(A=8), dict(A=9), dict(A=32),        # 8: the last vector case; 9, 32: tiled; 32 = the bound of S[32] in k_edac_gamma
    dict(hidden=(256, 32)), dict(hidden=(260, 32)), dict(hidden=(512, 32)), dict(hidden=(30, 32)),      # (32 is the base: 56 lanes idle in the column loop)
    dict(hidden=(256, 32), A=9), dict(hidden=(256, 32), B=9, A=8),
    dict(K=2), dict(K=3),
    dict(eta=5.0),
    dict(R=3),
    dict(precision=1), dict(precision=2), dict(precision=1, A=9), dict(precision=2, hidden=(30, 32)), dict(precision=1, hidden=(256, 32), B=33),
]


def edac_expect(kw):
    """(vector path, mask from packed bits) the host dispatch must take: k_edac_t0 for A <= 8 and a first hidden width that is a multiple
    of 4; packed bits exist only for widths that are a multiple of 128"""
    n0 = kw["hidden"][0]
    return kw["A"] <= 8 and n0 % 4 == 0, n0 % 128 == 0


def dead_member_and_twins(scale):
    """member 0: a dead first layer (zero weights, bias -100: h_0 = 0 on every row, so its action gradient g is exactly 0); members 1 and 2:
    identical parameters; member 3: tail weights times ``scale`` (its g rows are 1e-6- resp. 1e3-sized)"""
    def f(c):
        for st in c.sts:
            for net in (st["critics"], st["critics_old"]):
                for k, v in net.items():
                    v[2] = v[1]
            cr = st["critics"]
            cr["model.0.weight"][0] = 0
            cr["model.0.bias"][0] = -100.0
            last = f"model.{2 * len(c.hidden)}.weight"
            cr[last][3] = cr[last][3] * f32(scale)
    f.__name__ = f"dead_twins_{scale:g}"
    return f


EDAC_EDGE_BASE = dict(B=64, A=6)
EDAC_EDGES = [dict(mutate=dead_member_and_twins(1e-5)), dict(mutate=dead_member_and_twins(1e4)), dict(mutate=dead_member_and_twins(1e4), hidden=(256, 32))]


def edac_kw(kw):
    base = dict(EDAC_BASE, **(EDAC_EDGE_BASE if "mutate" in kw else {}))
    return dict(base, **kw)
