"""Shared by tests/test_predict_dcn_cpu.py and tests/test_gpu_serving_dcn.py: the parameter recipe of the dcn.py serving
tests and its oracle.

The recipe is oracle/init.py's dcn_params plus the seeded noise of tests/test_gpu_serving.py::perturbed_params on gamma, beta
and every bias (out.b included): the oracle initialises gamma = 1, beta = 0 and the tower's biases = 0, so without it a wrong
batch-norm affine or a dropped bias would pass."""
import numpy as np

SMALL_ROWS = [7, 50, 3, 1000, 20]
# (tower, cross layers); (32, 18): out.W's cross part starts at 18 floats, which is not 16-byte aligned
CASES = (((100, 100), 3), ((32, 16), 1), ((64, 32, 16), 8), ((32, 18), 3))
COLS = ("small", "criteo39")
_PARAMS = {}


def row_off_of(cols):
    from oracle import criteo
    if cols == "criteo39":
        return criteo.row_offsets()
    return np.concatenate([[0], np.cumsum(SMALL_ROWS)]).astype(np.int64)


def perturbed_dcn_params(cols, layers, Lc, seed=0):
    """-> (P, row_off), cached and never modified by a test (the Criteo tables are 70 MB)."""
    from oracle import init
    key = (cols, tuple(layers), Lc, seed)
    if key not in _PARAMS:
        row_off = row_off_of(cols)
        P = init.dcn_params(seed, 16, tuple(layers), Lc, np.float32, row_off)
        rng = np.random.default_rng(1000 + seed)
        for k in sorted(P):
            leaf = k.split(".")[-1]
            if leaf.startswith("gamma"):
                P[k] = (P[k] + rng.uniform(-0.3, 0.3, P[k].shape)).astype(np.float32)
            elif leaf.startswith("beta") or k == "b1" or leaf in ("bout", "b") or (leaf.startswith("b") and leaf[1:].isdigit()):
                P[k] = (P[k] + rng.uniform(-0.2, 0.2, P[k].shape)).astype(np.float32)
        _PARAMS[key] = (P, row_off)
    return _PARAMS[key]


def oracle_prob(P, row_off, layers, ids):
    from oracle import models, nn
    return nn.sigmoid(models.DCN(P, row_off, len(layers), 0.0).forward(ids, train=False)).reshape(-1)
