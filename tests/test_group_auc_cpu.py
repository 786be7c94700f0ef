"""GAUC without a GPU: metrics.group_auc_records_host (the documented definition of rsx_auc_group_*, include/rsx.h) against an
O(n_g^2) pair count per group written here and against metrics.exact_auc_host on every group's subset; the one function that
divides against fractions.Fraction; the --group_auc_key plumbing and the C entries' envelope."""
import importlib
import math
from fractions import Fraction

import numpy as np
import pytest

from recsys_amd import metrics
from recsys_amd._lib import RsxError

INVALID = np.array([np.nan, np.inf, -np.inf, -1e-9, 1.0000001], np.float32)


def pair_count(labels, prob):
    """(P, N, U2) over all (positive, negative) pairs: 2 for a positive that outscores the negative, 1 for a tie."""
    y = np.asarray(labels, np.float32) > np.float32(0.5)
    p = np.asarray(prob, np.float32)
    pp, pn = p[y], p[~y]
    gt = int((pp[:, None] > pn[None, :]).sum())
    eq = int((pp[:, None] == pn[None, :]).sum())
    return int(pp.size), int(pn.size), 2 * gt + eq


def stream(rng, n, groups, distinct):
    g = rng.integers(0, groups, n).astype(np.int32)
    p = rng.random(n).astype(np.float32) if distinct is None else \
        np.concatenate([[0.0, 1.0], rng.random(distinct)]).astype(np.float32)[:distinct][rng.integers(0, distinct, n)]
    y = (rng.random(n) < 0.2 + 0.6 * p).astype(np.float32)
    return g, y, p


CASES = [(n, groups, distinct) for n in (1, 2, 37, 400) for groups in (1, 3, 12) for distinct in (None, 2, 8)]


@pytest.mark.parametrize("n,groups,distinct", CASES)
def test_records_equal_pair_count_and_exact_auc_per_group(n, groups, distinct):
    rng = np.random.default_rng(100 * n + 10 * groups + (distinct or 0))
    g, y, p = stream(rng, n, groups, distinct)
    rec, invalid = metrics.group_auc_records_host(g, y, p, group_bits=4)
    assert invalid == 0 and rec.dtype == np.uint64
    assert [int(v) for v in rec[:, 0]] == sorted(set(int(v) for v in g))
    for gid, P, N, U2 in ([int(v) for v in r] for r in rec):
        sel = g == gid
        assert (P, N, U2) == pair_count(y[sel], p[sel])
        e = metrics.exact_auc_host(y[sel], p[sel])
        assert (P, N, U2) == (e["positives"], e["negatives"], e["u2"])
    hdr = metrics.group_auc_header_host(rec, invalid)
    assert hdr[0] == n and hdr[2] == len(rec) and hdr[5] + hdr[6] == n and hdr[7] == 0


@pytest.mark.parametrize("distinct", [None, 3])
def test_one_group_is_the_exact_auc(distinct):
    rng = np.random.default_rng(5)
    _, y, p = stream(rng, 300, 1, distinct)
    rec, invalid = metrics.group_auc_records_host(np.full(300, 6), y, p, group_bits=3)
    e = metrics.exact_auc_host(y, p)
    assert invalid == 0 and [int(v) for v in rec[0]] == [6, e["positives"], e["negatives"], e["u2"]]
    assert metrics.group_auc_host(np.full(300, 6), y, p, 3)["GAUC"] == e["AUC_exact"]


def test_every_example_in_its_own_group_gives_nan():
    rng = np.random.default_rng(6)
    _, y, p = stream(rng, 50, 1, None)
    res = metrics.group_auc_host(np.arange(50), y, p, group_bits=6)
    assert math.isnan(res["GAUC"])
    assert res == {**res, "groups": 50, "mixed_groups": 0, "skipped_examples": 50, "invalid": 0}


def test_equal_scores_across_a_group_boundary_are_no_tie():
    """Group 0 ends with a negative at 0.5, group 1 begins with a positive at 0.5: the pair belongs to no group."""
    g = np.array([0, 0, 1, 1], np.int32)
    y = np.array([1, 0, 1, 0], np.float32)
    p = np.array([0.25, 0.5, 0.5, 0.75], np.float32)
    rec, _ = metrics.group_auc_records_host(g, y, p, 1)
    assert rec.tolist() == [[0, 1, 1, 0], [1, 1, 1, 0]]
    assert metrics.group_auc_host(g, y, p, 1)["GAUC"] == 0.0


def test_invalid_ids_and_probabilities_are_counted_and_excluded():
    rng = np.random.default_rng(7)
    g, y, p = stream(rng, 300, 8, None)
    g = g.astype(np.int64)
    bad_id = rng.choice(300, 12, replace=False)
    g2 = g.copy()
    g2[bad_id] = np.tile(np.array([8, 9, 1 << 31, (1 << 40) + 3, -1, -(1 << 33)], np.int64), 2)   # group_bits = 3: ids 0..7
    rest = np.setdiff1d(np.arange(300), bad_id)
    bad_p = rng.choice(rest, INVALID.size, replace=False)
    p2 = p.copy()
    p2[bad_p] = INVALID
    rec, invalid = metrics.group_auc_records_host(g2, y, p2, group_bits=3)
    keep = np.ones(300, bool)
    keep[bad_id] = keep[bad_p] = False
    ref, none = metrics.group_auc_records_host(g[keep], y[keep], p[keep], group_bits=3)
    assert invalid == 12 + INVALID.size and none == 0 and np.array_equal(rec, ref)
    keys = metrics.group_auc_keys_host(g2, y, p2, 3)
    assert np.all(keys[~keep] == np.uint64(metrics.GROUP_AUC_PAD)) and np.all(keys[keep] != np.uint64(metrics.GROUP_AUC_PAD))
    res = metrics.group_auc_host(g2, y, p2, 3)
    assert res["invalid"] == invalid and math.isnan(metrics.group_auc_reported(res)) and not math.isnan(res["GAUC"])
    one = metrics.group_auc_keys_host(np.array([(1 << 31) - 1]), np.array([1.0], np.float32), np.array([1.0], np.float32), 31)
    assert int(one[0]) == (((1 << 31) - 1) << 32) | (0x3F800000 << 1) | 1
    with pytest.raises(ValueError):
        metrics.group_auc_keys_host(g, y, p, 32)


def test_from_records_against_fractions():
    """GAUC = sum(n_g U2_g / (2 P_g N_g)) / sum(n_g) over the mixed groups.  The float takes two roundings per term (the
    quotient, the product with n_g), the numerator's exact sum is rounded once (fsum), the denominator is an integer below 2^53
    and exact, and the division rounds once: four roundings of positive terms, (1 + 2^-53)^4 - 1 < 5 * 2^-53 relative.  The third
    record's n_g * U2_g is 3.6e24, far past 2^53; so is its U2 itself."""
    big_p, big_n = (1 << 26) + 1, (1 << 27) - 3
    rec = np.array([[0, 3, 2, 7],
                    [1, 5, 0, 0],                                    # one class: passed over
                    [5, big_p, big_n, 2 * big_p * big_n - 12345],
                    [9, 1, 1, 1],
                    [11, 0, 4, 0]], np.uint64)
    hdr = metrics.group_auc_header_host(rec, 2)
    assert hdr == [5 + 5 + big_p + big_n + 2 + 4, 2, 5, 3, 9, 3 + 5 + big_p + 1, 2 + big_n + 1 + 4, 0]
    res = metrics.group_auc_from_records(rec, hdr)
    num, den = Fraction(0), 0
    for _, P, N, U2 in ([int(v) for v in r] for r in rec):
        if P and N:
            num += Fraction((P + N) * U2, 2 * P * N)
            den += P + N
    want = num / den
    assert abs(Fraction(res["GAUC"]) - want) <= want * Fraction(5, 1 << 53)
    assert (res["groups"], res["mixed_groups"], res["skipped_examples"], res["invalid"]) == (5, 3, 9, 2)
    assert int(rec[2, 3]) > 1 << 53
    only_mixed = rec[[0, 2, 3]]
    assert metrics.group_auc_from_records(only_mixed, hdr)["GAUC"] == res["GAUC"]
    # exact cases: a perfect and a reversed ranking, and no mixed group at all
    assert metrics.group_auc_from_records(np.array([[0, 2, 3, 12], [1, 1, 1, 2]], np.uint64), [7, 0, 2, 2, 0, 3, 4, 0])["GAUC"] == 1.0
    assert metrics.group_auc_from_records(np.array([[4, 2, 3, 0]], np.uint64), [5, 0, 1, 1, 0, 2, 3, 0])["GAUC"] == 0.0
    assert math.isnan(metrics.group_auc_from_records(np.zeros((0, 4), np.uint64), [0] * 8)["GAUC"])
    with pytest.raises(RsxError):
        metrics.group_auc_from_records(rec, [0, 0, 5, 4, 0, 0, 0, 0])


@pytest.mark.parametrize("script", ["fm", "deepfm", "dcn", "xdeepfm", "din"])
def test_group_auc_key_flag_on_every_script(script):
    mod = importlib.import_module("recsys_amd." + script)
    key = "i_cate" if script == "din" else "u_id"
    assert mod.define_flags().parse_args(["--group_auc_key", key]).group_auc_key == key
    assert mod.define_flags().parse_args([]).group_auc_key is None


def test_run_config_default_and_world_check():
    from recsys_amd.estimator import RunConfig
    assert RunConfig().group_auc_key is None
    metrics.check_single_replica("group_auc_key", 1)
    with pytest.raises(RsxError, match="data-parallel evaluation is not supported"):
        metrics.check_single_replica("group_auc_key", 2)


def test_cabi_envelope_is_checked_before_any_device_call():
    """rsx_auc_group_*: the cap, the workspace formula of include/rsx.h, and RSX_EINVAL for what lies outside (checked on the
    host, before any HIP call: this runs without a GPU)."""
    import ctypes as C
    from recsys_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    T, cap = L.rsx_auc_exact_tile(), L.rsx_auc_group_max_keys()
    assert cap == 1 << 27 == L.rsx_auc_exact_max_keys()
    for n in (0, 1, T, T + 1, 51200, cap):
        nT = (n + T - 1) // T
        want = (8 * n + 255) // 256 * 256 + (1044 * nT + 8192 + 255) // 256 * 256 + 16 * nT
        assert L.rsx_auc_group_workspace_bytes(n, 1) == want == L.rsx_auc_group_workspace_bytes(n, 31)
    for n, bits in ((cap + 1, 8), (-1, 8), (8, 0), (8, 32)):
        assert L.rsx_auc_group_workspace_bytes(n, bits) == 0
    buf = (C.c_uint64 * 1024)()
    p = C.cast(buf, C.c_void_p)
    EINVAL, big = -1, 1 << 40
    assert L.rsx_auc_group_finalize(p, cap + 1, 8, p, big, p, None) == EINVAL
    assert L.rsx_auc_group_finalize(p, -1, 8, p, big, p, None) == EINVAL
    assert L.rsx_auc_group_finalize(p, 8, 0, p, big, p, None) == EINVAL
    assert L.rsx_auc_group_finalize(p, 8, 32, p, big, p, None) == EINVAL
    assert L.rsx_auc_group_finalize(None, 8, 8, p, big, p, None) == EINVAL
    assert L.rsx_auc_group_finalize(p, 8, 8, None, big, p, None) == EINVAL
    assert L.rsx_auc_group_finalize(p, 8, 8, p, big, None, None) == EINVAL
    assert L.rsx_auc_group_finalize(p, 8, 8, p, L.rsx_auc_group_workspace_bytes(8, 8) - 1, p, None) == EINVAL
    assert L.rsx_auc_group_finalize(C.c_void_p(p.value + 8), 8, 8, p, big, p, None) == EINVAL
    assert L.rsx_auc_group_append(None, p, p, 1, 8, 8, p, p, None) == EINVAL
    assert L.rsx_auc_group_append(p, p, None, 1, 8, 8, p, p, None) == EINVAL
    assert L.rsx_auc_group_append(p, p, p, 0, 8, 8, p, p, None) == EINVAL
    assert L.rsx_auc_group_append(p, p, p, 1, -1, 8, p, p, None) == EINVAL
    assert L.rsx_auc_group_append(p, p, p, 1, 8, 0, p, p, None) == EINVAL
    assert L.rsx_auc_group_append(p, p, p, 1, 8, 32, p, p, None) == EINVAL
    assert L.rsx_auc_group_append(p, p, p, 1, 8, 8, p, None, None) == EINVAL
    assert L.rsx_auc_group_append(p, p, p, 39, 0, 8, p, p, None) == 0
    assert L.rsx_auc_group_records(None, 8, p, p, p, 4, None) == EINVAL
    assert L.rsx_auc_group_records(p, 8, None, p, p, 4, None) == EINVAL
    assert L.rsx_auc_group_records(p, 8, p, None, p, 4, None) == EINVAL
    assert L.rsx_auc_group_records(p, 8, p, p, None, 4, None) == EINVAL
    assert L.rsx_auc_group_records(p, 8, p, p, p, -1, None) == EINVAL
    assert L.rsx_auc_group_records(p, -1, p, p, p, 4, None) == EINVAL
    assert L.rsx_auc_group_records(p, 8, p, p, C.c_void_p(p.value + 8), 4, None) == EINVAL
    assert L.rsx_auc_group_records(p, 0, p, p, p, 4, None) == 0
    assert L.rsx_auc_group_records(p, 8, p, p, p, 0, None) == 0
