"""Shared by tests/test_gpu_pair_rank.py and tests/test_pair_rank_cpu.py: the two small id columns, the weights recipe and the
oracle's answer for a (user, item) request."""
import numpy as np

ROWS = (300, 500)                                   # buckets of i_id (slot 0: input_layer sorts by name) and u_id (slot 1)
ROW_OFF = np.array([0, 300, 800], np.int64)
_PARAMS = {}


def pair_columns(D):
    from recsys_amd.feature_columns import Column
    emb = [Column("i_id_embedding", "i_id", "hash_embedding", ROWS[0], D),
           Column("u_id_embedding", "u_id", "hash_embedding", ROWS[1], D)]
    lin = [Column("i_id_indicator", "i_id", "hash_indicator", ROWS[0]), Column("u_id_indicator", "u_id", "hash_indicator", ROWS[1])]
    return lin, emb


def pair_params(D, layers, seed=0):
    """oracle/init.py weights with the noise of tests/test_gpu_serving.py::perturbed_params on gamma, beta and every bias, then
    made to SPREAD: tables x 4, w1 += 0.3 N(0, 1), |out.W[0]| raised by 0.5 (without it the first-order term is nearly
    invisible: out.W[0] = 0.014 at D = 32).  Cached; never modified by a test."""
    from oracle import init
    key = (D, tuple(layers), seed)
    if key not in _PARAMS:
        P = init.deepfm_params(seed, D, tuple(layers), np.float32, ROW_OFF)
        rng = np.random.default_rng(1000 + seed)
        for k in sorted(P):
            leaf = k.split(".")[-1]
            if leaf.startswith("gamma"):
                P[k] = (P[k] + rng.uniform(-0.3, 0.3, P[k].shape)).astype(np.float32)
            elif leaf.startswith("beta") or k == "b1" or leaf in ("bout", "b") or (leaf.startswith("b") and leaf[1:].isdigit()):
                P[k] = (P[k] + rng.uniform(-0.2, 0.2, P[k].shape)).astype(np.float32)
        P["tables"] = (P["tables"] * np.float32(4)).astype(np.float32)
        P["w1"] = (P["w1"] + 0.3 * rng.standard_normal(P["w1"].shape)).astype(np.float32)
        w = P["out.W"].copy()
        w[0] = np.where(w[0] < 0, w[0] - 0.5, w[0] + 0.5)
        P["out.W"] = w.astype(np.float32)
        _PARAMS[key] = P
    return _PARAMS[key]


def pair_ids(user, items, user_slot=1):
    """user [U], items [U, C] table-local -> the oracle's ids [U * C, 2] in slot order."""
    U, Cn = items.shape
    ids = np.empty((U * Cn, 2), np.int32)
    ids[:, user_slot] = np.repeat(user, Cn)
    ids[:, 1 - user_slot] = items.reshape(-1)
    return ids


def oracle_pair_prob(P, n_layers, user, items, user_slot=1):
    from oracle import models, nn
    z = models.DeepFM(P, ROW_OFF, n_layers, 0.0).forward(pair_ids(user, items, user_slot), train=False)
    return nn.sigmoid(z).reshape(items.shape).astype(np.float32)


def draw_pairs(rng, U, Cn, user_slot=1):
    """Table-local ids inside the buckets of the slot each field sits in."""
    return (rng.integers(0, ROWS[user_slot], U).astype(np.int32), rng.integers(0, ROWS[1 - user_slot], (U, Cn)).astype(np.int32))
