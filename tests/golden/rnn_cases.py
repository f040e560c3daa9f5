"""Inputs of the RNNDynamics fixtures (tests/golden/rnn_*.npz), regenerated identically by the generator and by the tests; only the
reference's outputs (and the dropout keep masks it drew) are stored.  Everything comes from numpy's RandomState, so no torch version
enters the inputs.

Cases (the smallest shapes at which the kernels can still go wrong):
  rnn_tiny     one GRU layer, one short row block (5 of 16 rows), every tensor's gradient stored
  rnn_t1       T = 1: the recurrent product is zero and only b_hh reaches the gates
  rnn_odd      3H = 120 and B = 37 divide by no tile; loss masks with zero entries and one all-zero row; recorded dropout
  rnn_default  the constructor's defaults at batch 64
  rnn_traj     20 Adam steps on 40 rows cycled in batches of 16 (the last of an epoch 8 rows short)
  rnn_trace    the whole train() (3 epochs over 20 sequences in batches of 8) and step() on 6 windows"""
import numpy as np

CASES = {
    "rnn_tiny": dict(input_dim=5, output_dim=4, hidden=[24, 24], L=1, B=5, T=3, p=0.0, n=5, seed=501, lengths=False),
    "rnn_t1": dict(input_dim=5, output_dim=4, hidden=[24, 24], L=2, B=3, T=1, p=0.0, n=3, seed=502, lengths=False),
    "rnn_odd": dict(input_dim=7, output_dim=5, hidden=[40, 40, 40], L=3, B=37, T=7, p=0.1, n=37, seed=503, lengths=True),
    "rnn_default": dict(input_dim=14, output_dim=12, hidden=[200, 200, 200, 200], L=3, B=64, T=20, p=0.1, n=64, seed=504, lengths=False),
    "rnn_traj": dict(input_dim=5, output_dim=4, hidden=[24, 24, 24], L=2, B=16, T=5, p=0.0, n=40, seed=505, lengths=True, steps=20, lr=1e-3),
    "rnn_trace": dict(input_dim=5, output_dim=4, hidden=[24, 24], L=1, B=8, T=4, p=0.0, n=20, seed=506, lengths=True, epochs=3, lr=1e-3,
                      obs_dim=3, act_dim=2, windows=6, torch_seed=1234),
}
for _name, _c in CASES.items():
    _c["name"] = _name
    _c["H"] = _c["hidden"][0]
PRED_STEPS = (0, 9, 19)         # rnn_default stores pred at these time steps
DIGEST = 512                    # rnn_default stores this many entries of every tensor's float64 gradient


def shapes(c):
    """[(state_dict key, shape)] of RNNModel in state_dict order"""
    H, out = c["H"], []
    for l in range(c["L"]):
        out += [(f"rnn_layer.weight_ih_l{l}", (3 * H, H if l else c["input_dim"])), (f"rnn_layer.weight_hh_l{l}", (3 * H, H)),
                (f"rnn_layer.bias_ih_l{l}", (3 * H,)), (f"rnn_layer.bias_hh_l{l}", (3 * H,))]
    out += [("input_layer.linear.weight", (H, c["input_dim"])), ("input_layer.linear.bias", (H,)),
            ("input_layer.layer_norm.weight", (H,)), ("input_layer.layer_norm.bias", (H,))]
    for i in range(len(c["hidden"]) - 1):
        out += [(f"backbones.{i}.linear.weight", (H, H)), (f"backbones.{i}.linear.bias", (H,)),
                (f"backbones.{i}.layer_norm.weight", (H,)), (f"backbones.{i}.layer_norm.bias", (H,))]
    out += [("merge_layer.weight", (H, 2 * H)), ("merge_layer.bias", (H,)), ("output_layer.weight", (c["output_dim"], H)),
            ("output_layer.bias", (c["output_dim"],))]
    return out


def make_params(c, seed_offset=0):
    """{key: float32 array}: GRU tensors U(-1, 1) / sqrt(H) (torch's own scale), Linear weights and biases U(-1, 1) / sqrt(fan_in),
    LayerNorm weights 1 + 0.3 U(-1, 1) and biases 0.3 U(-1, 1): no tensor sits at a value that hides an error (gamma = 1, beta = 0)"""
    rng = np.random.RandomState(c["seed"] + seed_offset)
    out, fan_in = {}, 1
    for key, shape in shapes(c):
        u = rng.uniform(-1.0, 1.0, size=shape)
        if ".layer_norm." in key:
            v = (1.0 if key.endswith("weight") else 0.0) + 0.3 * u
        elif key.startswith("rnn_layer."):
            v = u / np.sqrt(c["H"])
        else:
            if key.endswith("weight"):
                fan_in = shape[1]
            v = u / np.sqrt(fan_in)
        out[key] = v.astype(np.float32)
    return out


def make_data(c):
    """(inputs [n, T, in], targets [n, T, out], masks [n, T]).  With ``lengths`` every sequence is valid for a random number of
    leading steps (at least one) and the rest of its mask is zero; case rnn_odd also has one sequence whose mask is zero throughout."""
    rng = np.random.RandomState(c["seed"] + 1)
    n, T = c["n"], c["T"]
    inputs = rng.standard_normal((n, T, c["input_dim"])).astype(np.float32)
    targets = (0.5 * rng.standard_normal((n, T, c["output_dim"]))).astype(np.float32)
    masks = np.ones((n, T), np.float32)
    if c["lengths"]:
        length = rng.randint(1, T + 1, size=n)
        masks = (np.arange(T)[None, :] < length[:, None]).astype(np.float32)
        if c["name"] == "rnn_odd":
            masks[11] = 0.0
    return inputs, targets, masks


def make_steps(c):
    """rnn_traj: the row indices of its optimizer steps, the data set cycled in order in batches of B (the last of an epoch short)"""
    out = []
    while len(out) < c["steps"]:
        for s in range(0, c["n"], c["B"]):
            out.append(np.arange(s, min(s + c["B"], c["n"]), dtype=np.int64))
    return out[:c["steps"]]


def make_windows(c):
    """rnn_trace: obss [windows, T, obs_dim] and actions [windows, T, act_dim] for step(), and the scaler's (mu, std)"""
    rng = np.random.RandomState(c["seed"] + 2)
    obss = rng.standard_normal((c["windows"], c["T"], c["obs_dim"])).astype(np.float32)
    actions = np.tanh(rng.standard_normal((c["windows"], c["T"], c["act_dim"]))).astype(np.float32)
    mu = (0.2 * rng.standard_normal((1, c["input_dim"]))).astype(np.float32)
    std = (1.0 + 0.3 * rng.uniform(size=(1, c["input_dim"]))).astype(np.float32)
    return obss, actions, mu, std


TERMINAL_AT = 1.5


def terminal_fn(obs, act, next_obs):
    """rnn_trace's terminal function: the next observation leaves the box |x| <= 1.5"""
    return (np.abs(next_obs).max(axis=-1, keepdims=True) > TERMINAL_AT)


def digest_positions(c, key, size):
    """the entries of tensor ``key`` whose float64 gradient rnn_default stores"""
    rng = np.random.RandomState(c["seed"] + 7 + sum(key.encode()))
    return rng.choice(size, size=min(DIGEST, size), replace=False)


def pack_masks(m):
    """keep masks [norms, rows, H] of 0 / 1 -> packed bits"""
    return np.packbits(np.asarray(m, np.uint8).ravel())


def unpack_masks(bits, c, rows):
    norms = len(c["hidden"])
    return np.unpackbits(bits)[:norms * rows * c["H"]].reshape(norms, rows, c["H"]).astype(np.float32)
