"""The exact, tie-aware ROC AUC without a GPU: metrics.exact_auc_host (the documented definition of rsx_auc_exact_*,
include/rsx.h) against an O(n^2) pair count written here, the key encoding's edge cases, and the --exact_auc plumbing."""
import importlib
import math

import numpy as np
import pytest

from recsys_amd import metrics
from recsys_amd._lib import RsxError

SUBNORMAL = np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]            # the smallest positive fp32
INVALID = np.array([np.nan, np.inf, -np.inf, -1e-9, 1.0000001], np.float32)


def pair_count(labels, prob):
    """(U2, P, N) over all (positive, negative) pairs: 2 for a positive that outscores the negative, 1 for a tie.  -0.0 == 0.0
    and subnormals compare as numbers in numpy's fp32, which is the contract."""
    y = np.asarray(labels, np.float32).reshape(-1) > np.float32(0.5)
    p = np.asarray(prob, np.float32).reshape(-1)
    ok = (p >= 0) & (p <= 1)
    pp, pn = p[ok & y], p[ok & ~y]
    gt = int((pp[:, None] > pn[None, :]).sum())
    eq = int((pp[:, None] == pn[None, :]).sum())
    return 2 * gt + eq, int(pp.size), int(pn.size)


def scores(rng, n, distinct):
    """n fp32 scores in [0, 1] drawn from `distinct` values that include 0.0, 1.0 and a subnormal when there is room."""
    special = np.array([0.0, 1.0, SUBNORMAL], np.float32)
    if distinct >= n:
        rest = np.setdiff1d(rng.random(4 * n + 8).astype(np.float32), special)
        vals = np.concatenate([special, rng.permutation(rest)])[:n]
        return rng.permutation(vals).astype(np.float32)
    pool = np.concatenate([special, rng.random(distinct).astype(np.float32)])[:distinct] if distinct >= 3 else \
        np.array([0.0, SUBNORMAL], np.float32)[:distinct]
    return pool[rng.integers(0, distinct, n)].astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 257, 2000])
@pytest.mark.parametrize("distinct", [1, 2, 7, None])
def test_host_reference_equals_pair_count(n, distinct):
    rng = np.random.default_rng(1000 * n + (distinct or 0))
    p = scores(rng, n, distinct or n)
    y = (rng.random(n) < 0.2 + 0.6 * p).astype(np.float32)
    res = metrics.exact_auc_host(y, p)
    u2, P, N = pair_count(y, p)
    assert (res["u2"], res["positives"], res["negatives"], res["invalid"]) == (u2, P, N, 0)
    if P * N:
        assert res["AUC_exact"] == u2 / (2 * P * N)
    else:
        assert math.isnan(res["AUC_exact"])


def test_distinct_scores_are_distinct():
    """The n-distinct cases above really hold n different scores (and the special values)."""
    p = scores(np.random.default_rng(0), 2000, 2000)
    assert np.unique(p).size == 2000 and {0.0, 1.0, float(SUBNORMAL)} <= set(map(float, p))


def test_negative_zero_ties_with_zero():
    y = np.array([1, 0, 1, 0], np.float32)
    p = np.array([-0.0, 0.0, 0.0, -0.0], np.float32)
    res = metrics.exact_auc_host(y, p)
    assert res["invalid"] == 0 and (res["u2"], res["positives"], res["negatives"]) == (4, 2, 2)
    assert res["AUC_exact"] == 0.5
    k = metrics.exact_auc_keys_host(y, p)
    assert list(k) == [1, 0, 1, 0]


def test_subnormals_stay_distinct_scores():
    two = np.frombuffer(np.uint32(2).tobytes(), np.float32)[0]
    res = metrics.exact_auc_host(np.array([0, 1, 0, 1], np.float32), np.array([0.0, SUBNORMAL, SUBNORMAL, two], np.float32))
    assert (res["u2"], res["positives"], res["negatives"]) == ((2 + 1) + 4, 2, 2)


def test_invalid_scores_are_counted_and_excluded():
    rng = np.random.default_rng(3)
    p = rng.random(300).astype(np.float32)
    y = (rng.random(300) < p).astype(np.float32)
    at = rng.choice(300, 2 * INVALID.size, replace=False)
    p2 = p.copy()
    p2[at] = np.tile(INVALID, 2)
    res = metrics.exact_auc_host(y, p2)
    keep = np.ones(300, bool)
    keep[at] = False
    ref = metrics.exact_auc_host(y[keep], p[keep])
    assert res["invalid"] == 2 * INVALID.size
    assert {k: res[k] for k in ("u2", "positives", "negatives", "AUC_exact")} == \
           {k: ref[k] for k in ("u2", "positives", "negatives", "AUC_exact")}
    assert (res["u2"], res["positives"], res["negatives"]) == pair_count(y, p2)
    assert np.all(metrics.exact_auc_keys_host(y, p2)[at] == metrics.EXACT_AUC_PAD)
    one = metrics.exact_auc_keys_host(np.array([1.0], np.float32), np.array([1.0], np.float32))
    assert int(one[0]) == (0x3F800000 << 1) | 1


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_one_class_gives_nan(label):
    p = np.random.default_rng(4).random(50).astype(np.float32)
    res = metrics.exact_auc_host(np.full(50, label, np.float32), p)
    assert math.isnan(res["AUC_exact"]) and res["u2"] == 0
    assert res["positives"] + res["negatives"] == 50 and res["positives"] * res["negatives"] == 0


def test_matches_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    for n, distinct in ((2000, 2000), (2000, 7), (257, 40)):
        p = scores(rng, n, distinct)
        y = (rng.random(n) < 0.2 + 0.6 * p).astype(np.float32)
        assert abs(metrics.exact_auc_host(y, p)["AUC_exact"] - skm.roc_auc_score(y, p)) <= 1e-12


@pytest.mark.parametrize("script", ["fm", "deepfm", "dcn", "xdeepfm", "din"])
def test_exact_auc_flag_on_every_script(script):
    mod = importlib.import_module("recsys_amd." + script)
    assert mod.define_flags().parse_args(["--exact_auc", "true"]).exact_auc is True
    assert mod.define_flags().parse_args([]).exact_auc is False


def test_run_config_default_and_world_check():
    from recsys_amd.estimator import RunConfig
    assert RunConfig().exact_auc is False
    metrics.check_single_replica("exact_auc", 1)
    with pytest.raises(RsxError, match="data-parallel evaluation is not supported"):
        metrics.check_single_replica("exact_auc", 2)


def test_cabi_envelope_is_checked_before_any_device_call():
    """rsx_auc_exact_*: tile, cap, the workspace formula of include/rsx.h, and RSX_EINVAL for what lies outside (checked on the
    host, before any HIP call: this runs without a GPU)."""
    import ctypes as C
    from recsys_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    T, cap = L.rsx_auc_exact_tile(), L.rsx_auc_exact_max_keys()
    assert T == 4096 and cap >= 1 << 27
    for n in (0, 1, T, T + 1, 51200, cap):
        assert L.rsx_auc_exact_workspace_bytes(n) == (4 * n + 255) // 256 * 256 + 1032 * ((n + T - 1) // T) + 4096
    assert L.rsx_auc_exact_workspace_bytes(cap + 1) == 0 and L.rsx_auc_exact_workspace_bytes(-1) == 0
    buf = (C.c_uint64 * 1024)()
    p = C.cast(buf, C.c_void_p)
    EINVAL = -1
    assert b"invalid" in L.rsx_strerror(EINVAL)
    assert L.rsx_auc_exact_finalize(p, cap + 1, p, 1 << 40, p, None) == EINVAL
    assert L.rsx_auc_exact_finalize(p, -1, p, 1 << 40, p, None) == EINVAL
    assert L.rsx_auc_exact_finalize(None, 8, p, 1 << 20, p, None) == EINVAL
    assert L.rsx_auc_exact_finalize(p, 8, None, 1 << 20, p, None) == EINVAL
    assert L.rsx_auc_exact_finalize(p, 8, p, 1 << 20, None, None) == EINVAL
    assert L.rsx_auc_exact_finalize(p, 8, p, L.rsx_auc_exact_workspace_bytes(8) - 1, p, None) == EINVAL
    assert L.rsx_auc_exact_finalize(C.c_void_p(p.value + 4), 8, p, 1 << 20, p, None) == EINVAL
    assert L.rsx_auc_exact_append(None, p, 8, p, p, None) == EINVAL
    assert L.rsx_auc_exact_append(p, p, -1, p, p, None) == EINVAL
    assert L.rsx_auc_exact_append(p, p, 8, p, None, None) == EINVAL
    assert L.rsx_auc_exact_append(p, p, 0, p, p, None) == 0
