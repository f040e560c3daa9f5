"""The shapes of tests/test_gpu_rnn_kernels.py and tests/test_rnn_refs_cpu.py: the smallest at which each guard of csrc/rnn_dynamics.hip
changes.  Columns (H, B, T, L, in, out, len(hidden), p):

  A  8, 1, 1, 1, 1, 1, 2, 0        half a unit tile; one row; no recurrent product
  B  12, 17, 3, 2, 3, 2, 3, 0.25   H no multiple of 8; a second row block of one row; nterm = 2; forced keep masks; lengths with one
                                   all-zero mask row.  Also as run 1 of a two-run object with other parameters per run
  C  20, 16, 2, 1, 2, 2, 2, 0      a partial second unit tile, 3H = 60.  Also with inputs and GRU weights scaled until the gates
                                   saturate (1 - n^2 and z (1 - z) cancel): the bound has to widen by itself
  D  68, 5, 4, 2, 4, 3, 2, 0       backward group 1 with one lane quad; LayerNorm slot j = 1 with four lanes
  E  132, 33, 16, 1, 6, 3, 3, 0    N = 528: two slabs, nine chunks with a last one of 16 rows; forward wave 0's second tile partial;
                                   three row blocks
  F  260, 17, 2, 3, 5, 4, 2, 0.1   five backward groups (wave 0 takes a second one); 17 forward tiles; both dXL buffers
  G  512, 16, 3, 1, 4, 3, 2, 0     the maximum: four tiles per forward wave, two groups per backward wave, 131 KB of LDS
  H  24, 2, 40, 1, 2, 2, 2, 0      a long recurrence: how the carried bound grows

Parameters and data come from rnn_cases.make_params / make_data (gamma never 1, beta never 0)."""
import numpy as np

import rnn_cases as rc

TABLE = {
    "A": (8, 1, 1, 1, 1, 1, 2, 0.0),
    "B": (12, 17, 3, 2, 3, 2, 3, 0.25),
    "C": (20, 16, 2, 1, 2, 2, 2, 0.0),
    "D": (68, 5, 4, 2, 4, 3, 2, 0.0),
    "E": (132, 33, 16, 1, 6, 3, 3, 0.0),
    "F": (260, 17, 2, 3, 5, 4, 2, 0.1),
    "G": (512, 16, 3, 1, 4, 3, 2, 0.0),
    "H": (24, 2, 40, 1, 2, 2, 2, 0.0),
}
NAMES = list(TABLE)
SATURATE = 12.0         # case C's second run: inputs and GRU tensors times this


def case(name):
    H, B, T, L, nin, nout, nh, p = TABLE[name]
    c = dict(name="kern_" + name, input_dim=nin, output_dim=nout, hidden=[H] * nh, H=H, L=L, B=B, T=T, p=p, n=B + 3, seed=7100 + ord(name),
             lengths=name == "B")
    return c


def data(c):
    """(inputs, targets, masks) of n = B + 3 sequences; case B: lengths, and sequence 2 masked out throughout"""
    x, tg, mk = rc.make_data(c)
    if c["lengths"]:
        mk[2] = 0.0
    return x, tg, mk


def indices(c, rows=None):
    """row indices of a step: out of order, with one repeat when there are at least two rows, and every case-B batch holds sequence 2"""
    rows = c["B"] if rows is None else rows
    idx = np.random.RandomState(c["seed"] + 5).permutation(c["n"])[:rows].astype(np.int64)
    if rows >= 2:
        idx[-1] = idx[0]
    if c["lengths"] and rows >= 3:
        idx[1] = 2
    return idx


def drop_masks(c, rows=None, seed=0):
    """forced keep masks [len(hidden), rows * T, H], or None without dropout"""
    if not c["p"] > 0:
        return None
    rows = c["B"] if rows is None else rows
    rng = np.random.RandomState(c["seed"] + 9 + seed)
    return (rng.uniform(size=(len(c["hidden"]), rows * c["T"], c["H"])) >= c["p"]).astype(np.float32)


def saturated(P, x):
    """case C's saturating twin: GRU tensors and inputs times SATURATE"""
    P = {k: (v * np.float32(SATURATE) if k.startswith("rnn_layer.") else v.copy()) for k, v in P.items()}
    return P, (x * np.float32(SATURATE)).astype(np.float32)
