"""The calibration metrics without a GPU: the definitions of recsys_amd/metrics.py (calibration_bins_host, calibration_groups_host,
calibration_from_table, group_calibration_from_table) against the stated arithmetic evaluated independently with struct /
fractions / math; the --calibration_bins / --calibration_key plumbing and the C entry's envelope.  Integer equality everywhere."""
import importlib
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

from recsys_amd import metrics
from recsys_amd._lib import RsxError

ONE = 1 << 32
INVALID = np.array([np.nan, np.inf, -np.inf, -1e-9, 1.0000001], np.float32)


def f32(x):
    """A Python float or Fraction rounded to nearest-even fp32, by struct."""
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


def bin_by_fractions(p, N):
    """min(N - 1, trunc(fp32(p * N))): the product of a 24-bit and an 11-bit significand is exact as a Fraction and as a double,
    so one rounding to fp32 is the fp32 multiply."""
    prod = Fraction(float(p)) * N
    assert Fraction(float(prod)) == prod
    return min(N - 1, int(f32(prod)))


def edge_values(N):
    """k / N as fp32 and its two neighbours, for every k, kept inside [0, 1]."""
    k = np.arange(N + 1, dtype=np.float64)
    mid = (k / N).astype(np.float32)
    v = np.concatenate([mid, np.nextafter(mid, np.float32(-1)), np.nextafter(mid, np.float32(2))])
    return v[(v >= 0) & (v <= 1)].astype(np.float32)


@pytest.mark.parametrize("N", [2, 10, 1024])
def test_bin_edges_follow_the_fp32_arithmetic(N):
    p = edge_values(N)
    assert p.size >= 3 * N
    got = metrics.calibration_bin_host(p, N)
    assert got.dtype == np.int32 and got.tolist() == [bin_by_fractions(v, N) for v in p]
    assert got.min() == 0 and got.max() == N - 1
    table, invalid = metrics.calibration_bins_host(np.zeros(p.size, np.float32), p, N)
    assert invalid == 0 and table[:, 0].tolist() == np.bincount(got, minlength=N).tolist()
    ends = np.array([0.0, -0.0, 1.0], np.float32)
    assert metrics.calibration_bin_host(ends, N).tolist() == [0, 0, N - 1]
    t, bad = metrics.calibration_bins_host(np.ones(3, np.float32), ends, N)
    assert bad == 0 and t[0].tolist() == [2, 2, 0] and t[N - 1].tolist() == [1, 1, ONE]


def test_an_ulp_below_an_edge_may_land_in_the_upper_bin_and_that_is_the_definition():
    """0.7 in fp32 is below 7 / 10, yet fp32(0.7f * 10.0f) == 7.0f: bin 7, on both sides."""
    p = np.float32(0.7)
    assert Fraction(float(p)) < Fraction(7, 10) and bin_by_fractions(p, 10) == 7
    assert metrics.calibration_bin_host(np.array([p]), 10).tolist() == [7]


def test_fixed_point_probability():
    q = metrics.calibration_q_host
    assert q(np.array([1.0, 2.0 ** -33, 2.0 ** -32, 0.0, 0.5], np.float32)).tolist() == [ONE, 0, 1, 0, ONE >> 1]
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.random(500), rng.random(200) * 1e-6, np.float32(2.0) ** -rng.integers(20, 60, 50)]).astype(np.float32)
    got = q(p)
    assert got.dtype == np.uint64
    assert [int(v) for v in got] == [math.floor(Fraction(float(v)) * ONE) for v in p]


def by_hand(table, loss):
    """ECE / MCE / PCOC / CTR / mean_prob / NE of a table, in Fractions and math."""
    n = sum(r[0] for r in table)
    P = sum(r[1] for r in table)
    S = sum(r[2] for r in table)
    d = [abs(Fraction(r[2]) - r[1] * ONE) for r in table]
    ctr = float(Fraction(P, n))
    return {"ECE": float(sum(d) / (n * ONE)), "MCE": max(float(db / (r[0] * ONE)) for db, r in zip(d, table) if r[0]),
            "PCOC": float(Fraction(S, P * ONE)), "CTR": ctr, "mean_prob": float(Fraction(S, n * ONE)),
            "NE": loss / -(ctr * math.log(ctr) + (1 - ctr) * math.log(1 - ctr))}


def test_figures_of_a_hand_made_table():
    table = [[10, 1, 3 * ONE // 2 + 12345], [7, 3, 5 * ONE // 2 - 999], [0, 0, 0], [5, 4, 9 * ONE // 2 + 7]]
    res = metrics.calibration_from_table(np.array(table, np.int64), 0, loss=0.61)
    want = by_hand(table, 0.61)
    assert {k: res[k] for k in want} == want
    assert res["examples"] == 22 and res["invalid"] == 0
    assert set(res) == {"ECE", "MCE", "PCOC", "NE", "CTR", "mean_prob", "examples", "invalid"}
    # the largest bin error is the third non-empty bin's: |4.5 - 4| / 5 against 0.5 / 10 and 0.5 / 7
    assert res["MCE"] == float(Fraction(ONE // 2 + 7, 5 * ONE))
    assert math.isnan(metrics.calibration_from_table(np.array(table, np.int64), 0)["NE"])          # no loss: no NE
    rep = metrics.calibration_reported(res)
    assert set(rep) == set(metrics.CALIBRATION_FIGURES) and all(rep[k] == res[k] for k in rep)
    bad = metrics.calibration_from_table(np.array(table, np.int64), 3, loss=0.61)
    assert bad["invalid"] == 3 and bad["ECE"] == res["ECE"]
    assert all(math.isnan(v) for v in metrics.calibration_reported(bad).values())


def test_perfectly_calibrated_and_degenerate_tables():
    perfect = np.array([[8, 1, ONE], [8, 4, 4 * ONE], [8, 7, 7 * ONE]], np.int64)
    res = metrics.calibration_from_table(perfect, 0, loss=0.5)
    assert res["ECE"] == 0.0 and res["MCE"] == 0.0 and res["PCOC"] == 1.0 and res["CTR"] == 0.5 == res["mean_prob"]
    assert res["NE"] == 0.5 / math.log(2.0)
    none = metrics.calibration_from_table(np.array([[4, 0, ONE], [2, 0, ONE // 2]], np.int64), 0, loss=0.2)
    assert math.isnan(none["PCOC"]) and math.isnan(none["NE"]) and none["CTR"] == 0.0 and none["ECE"] == 0.25
    every = metrics.calibration_from_table(np.array([[4, 4, ONE], [2, 2, ONE]], np.int64), 0, loss=0.2)
    assert math.isnan(every["NE"]) and every["CTR"] == 1.0 and every["PCOC"] == float(Fraction(2, 6))
    empty = metrics.calibration_from_table(np.zeros((5, 3), np.int64), 2, loss=0.3)
    assert empty["examples"] == 0 and empty["invalid"] == 2
    assert all(math.isnan(empty[k]) for k in metrics.CALIBRATION_FIGURES)


def test_sums_beyond_a_float64_are_divided_as_integers():
    """2^31 examples of p = 1 - 2^-24 in one bin: q_sum is far past 2^53; the quotient is the Fraction's."""
    n, q = 1 << 31, ONE - 256
    table = np.array([[n, n - 3, n * q]], np.int64)
    res = metrics.calibration_from_table(table, 0)
    assert res["PCOC"] == float(Fraction(n * q, (n - 3) * ONE)) and res["ECE"] == float(Fraction(abs(n * q - (n - 3) * ONE), n * ONE))


def test_group_figures():
    table = np.array([[10, 1, 3 * ONE // 2], [0, 0, 0], [6, 6, 5 * ONE], [1, 0, 77]], np.int64)
    res = metrics.group_calibration_from_table(table, 0)
    assert res == {"GCE": float(Fraction(ONE // 2 + ONE + 77, 17 * ONE)), "GCE_groups": 3, "examples": 17, "invalid": 0}
    assert metrics.group_calibration_reported(res) == {"GCE": res["GCE"]}
    bad = metrics.group_calibration_from_table(table, 1)
    assert bad["GCE"] == res["GCE"] and math.isnan(metrics.group_calibration_reported(bad)["GCE"])
    full = 1 << 31                                         # positives_g 2^32 = 2^63: past int64, still exact
    big = metrics.group_calibration_from_table(np.array([[full, full, full * (ONE - 1)], [2, 1, ONE]], np.int64), 0)
    assert big["GCE"] == float(Fraction(full, (full + 2) * ONE)) and big["examples"] == full + 2
    none = metrics.group_calibration_from_table(np.zeros((3, 3), np.int64), 0)
    assert math.isnan(none["GCE"]) and none["GCE_groups"] == 0 and none["examples"] == 0


def stream(rng, n, n_groups):
    p = np.concatenate([[0.0, 1.0], rng.random(n)]).astype(np.float32)[rng.integers(0, n + 2, n)]
    y = (rng.random(n) < 0.1 + 0.8 * p).astype(np.float32)
    return rng.integers(0, n_groups, n).astype(np.int32), y, p


def count_plainly(g, y, p, rows, index):
    """(count, positives, q_sum) rows by a Python loop over the valid examples."""
    table = [[0, 0, 0] for _ in range(rows)]
    for gi, yi, pi in zip(g, y, p):
        r = table[index(gi, pi)]
        r[0] += 1
        r[1] += 1 if yi > 0.5 else 0
        r[2] += math.floor(Fraction(float(pi)) * ONE)
    return table


def test_invalid_examples_are_counted_and_enter_no_table():
    rng = np.random.default_rng(3)
    n, G, N = 600, 9, 10
    g, y, p = stream(rng, n, G)
    g = g.astype(np.int64)
    at = rng.choice(n, 2 * INVALID.size + 6, replace=False)
    p2, g2 = p.copy(), g.copy()
    p2[at[:2 * INVALID.size]] = np.tile(INVALID, 2)
    g2[at[2 * INVALID.size:]] = [-1, G, 1 << 40, -1, G, (1 << 31) + 3]
    keep_p = np.ones(n, bool)
    keep_p[at[:2 * INVALID.size]] = False
    keep = keep_p.copy()
    keep[at[2 * INVALID.size:]] = False
    bins, bad = metrics.calibration_bins_host(y, p2, N)
    assert bad == 2 * INVALID.size and int(bins[:, 0].sum()) == n - bad
    assert bins.tolist() == count_plainly(g[keep_p], y[keep_p], p[keep_p], N, lambda gi, pi: bin_by_fractions(pi, N))
    groups, bad = metrics.calibration_groups_host(g2, y, p2, G)
    assert bad == 2 * INVALID.size + 6 and int(groups[:, 0].sum()) == n - bad
    assert groups.dtype == np.int64 and groups.shape == (G, 3)
    assert groups.tolist() == count_plainly(g[keep], y[keep], p[keep], G, lambda gi, pi: int(gi))
    for v in INVALID:
        t, bad = metrics.calibration_bins_host([1.0], [v], 4)
        assert bad == 1 and not t.any()


def test_labels_classify_at_one_half():
    y = np.array([0, 0.5, 0.50001, 1], np.float32)
    t, _ = metrics.calibration_bins_host(y, np.full(4, 0.25, np.float32), 2)
    assert t.tolist() == [[4, 2, ONE], [0, 0, 0]]
    t, _ = metrics.calibration_groups_host(np.arange(4), y, np.full(4, 0.25, np.float32), 4)
    assert t[:, 1].tolist() == [0, 0, 1, 1]


def test_tables_do_not_depend_on_batches_or_order():
    rng = np.random.default_rng(4)
    n, G, N = 1000, 13, 20
    g, y, p = stream(rng, n, G)
    p[::97] = np.float32(np.nan)
    bins, bad_b = metrics.calibration_bins_host(y, p, N)
    groups, bad_g = metrics.calibration_groups_host(g, y, p, G)
    for order in (np.arange(n), rng.permutation(n), np.arange(n)[::-1]):
        sb, sg, ib, ig = np.zeros_like(bins), np.zeros_like(groups), 0, 0
        for i in range(0, n, 77):
            sel = order[i:i + 77]
            t, b = metrics.calibration_bins_host(y[sel], p[sel], N)
            sb, ib = sb + t, ib + b
            t, b = metrics.calibration_groups_host(g[sel], y[sel], p[sel], G)
            sg, ig = sg + t, ig + b
        assert np.array_equal(sb, bins) and np.array_equal(sg, groups) and (ib, ig) == (bad_b, bad_g)
    assert np.array_equal(bins.sum(0), groups.sum(0))                      # all ids are valid: both tables hold the same examples


@pytest.mark.parametrize("script", ["fm", "deepfm", "dcn", "xdeepfm", "din"])
def test_calibration_flags_on_every_script(script):
    mod = importlib.import_module("recsys_amd." + script)
    key = "i_cate" if script == "din" else "_c16"
    got = mod.define_flags().parse_args(["--calibration_bins", "20", "--calibration_key", key])
    assert got.calibration_bins == 20 and got.calibration_key == key
    off = mod.define_flags().parse_args([])
    assert off.calibration_bins == 0 and off.calibration_key is None


def test_run_config_defaults_and_world_check():
    from recsys_amd.estimator import RunConfig
    assert RunConfig().calibration_bins == 0 and RunConfig().calibration_key is None
    metrics.check_single_replica("calibration", 1)
    with pytest.raises(RsxError, match="data-parallel evaluation is not supported"):
        metrics.check_single_replica("calibration", 2)
    for n_bins in (0, 1, 1025):
        with pytest.raises(ValueError):
            metrics.calibration_bins_host([0.0], [0.5], n_bins)


def test_cabi_envelope_is_checked_before_any_device_call():
    """rsx_calibration_*: the caps of include/rsx.h, RSX_EINVAL / RSX_EUNSUPPORTED for what lies outside (checked on the host,
    before any HIP call: this runs without a GPU)."""
    import ctypes as C
    from recsys_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    assert L.rsx_calibration_max_bins() == 1024 and L.rsx_calibration_max_groups() == 1 << 22
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    EINVAL, EUNSUPPORTED = -1, -3
    up = L.rsx_calibration_update
    assert up(None, p, p, 1, 8, 10, 5, p, p, p, None) == EINVAL
    assert up(p, None, p, 1, 8, 10, 5, p, p, p, None) == EINVAL
    assert up(p, p, None, 1, 8, 10, 5, p, p, p, None) == EINVAL            # a group table needs the ids
    assert up(p, p, p, 1, 8, 10, 5, None, p, p, None) == EINVAL
    assert up(p, p, p, 1, 8, 10, 5, p, None, p, None) == EINVAL
    assert up(p, p, p, 1, 8, 10, 5, p, p, None, None) == EINVAL
    assert up(p, p, p, 0, 8, 10, 5, p, p, p, None) == EINVAL
    assert up(p, p, p, 1, -1, 10, 5, p, p, p, None) == EINVAL
    assert up(p, p, p, 1, 8, -1, 5, p, p, p, None) == EINVAL
    assert up(p, p, p, 1, 8, 10, -1, p, p, p, None) == EINVAL
    assert up(p, p, p, 1, 8, 0, 0, p, p, p, None) == EINVAL                # no table asked for
    assert up(p, p, p, 1, 8, 10, 5, C.c_void_p(p.value + 4), p, p, None) == EINVAL
    assert up(p, p, p, 1, 8, 1, 5, p, p, p, None) == EUNSUPPORTED
    assert up(p, p, p, 1, 8, 1025, 5, p, p, p, None) == EUNSUPPORTED
    assert up(p, p, p, 1, 8, 10, (1 << 22) + 1, p, p, p, None) == EUNSUPPORTED
    assert up(p, p, p, 1, (1 << 31) + 1, 10, 5, p, p, p, None) == EUNSUPPORTED
    # n == 0 is a no-op success, with either table alone too (the other's pointers are not needed)
    assert up(p, p, p, 1, 0, 10, 5, p, p, p, None) == 0
    assert up(p, p, None, 1, 0, 1024, 0, p, None, p, None) == 0
    assert up(p, p, p, 7, 0, 0, 1 << 22, None, p, p, None) == 0
