"""Isotonic calibration without a GPU: the definitions of recsys_amd/metrics.py (quantile_table_host, isotonic_from_table,
isotonic_apply_host) against the stated arithmetic evaluated independently with Python integers and fractions; IsotonicMap's
JSON; the flags; the C entries' envelopes; the bundle's optional file.  Integer and bit equality everywhere except the one
end-to-end recipe, whose bound the recipe's own numbers give."""
import importlib
import json
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from recsys_amd import metrics
from recsys_amd._lib import RsxError

ONE = 1 << 32
INVALID = np.array([np.nan, np.inf, -np.inf, -1e-9, 1.0000001, -1.0, 2.0], np.float32)


def bits_of(p):
    return struct.unpack("<I", struct.pack("<f", float(p)))[0]


def f32(x):
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


def table_by_loop(labels, prob, M):
    """The table by a per-example loop over Python integers: the keys sorted, the head of every position found by walking back."""
    keys = []
    for y, p in zip(labels, prob):
        u = bits_of(p)
        if u == 0x80000000:
            u = 0
        if u <= 0x3F800000:
            keys.append((u << 1) | (1 if y > 0.5 else 0))
    keys.sort()
    V = len(keys)
    table = [[0, 0, 0] for _ in range(M)]
    for i, k in enumerate(keys):
        h = i
        while h > 0 and keys[h - 1] >> 1 == k >> 1:
            h -= 1
        row = table[(h * M) // V]
        p = struct.unpack("<f", struct.pack("<I", k >> 1))[0]
        row[0] += 1
        row[1] += k & 1
        row[2] += math.floor(Fraction(p) * ONE)
    return table


def stream(rng, n, ties=None):
    p = rng.random(n).astype(np.float32)
    if ties:
        p = (np.round(p * ties) / ties).astype(np.float32)
    y = (rng.random(n) < 0.1 + 0.8 * p).astype(np.float32)
    return y, p


@pytest.mark.parametrize("n,M,ties", [(1, 2, None), (2, 10, None), (65, 10, None), (300, 2, None), (300, 1024, None),
                                      (257, 10, 8), (257, 64, 8), (200, 7, 1), (128, 10, 2)])
def test_quantile_table_matches_a_loop_over_python_integers(n, M, ties):
    rng = np.random.default_rng(100 * n + M)
    y, p = stream(rng, n, ties)
    got = metrics.quantile_table_host(y, p, M)
    assert got.dtype == np.int64 and got.shape == (M, 3)
    assert got.tolist() == table_by_loop(y, p, M)
    assert int(got[:, 0].sum()) == n


def test_quantile_table_ties_invalid_examples_and_the_ends():
    rng = np.random.default_rng(5)
    y, p = stream(rng, 400, ties=8)
    p[::37] = np.tile(INVALID, 3)[:p[::37].size]
    p[5], p[6] = np.float32(-0.0), np.float32(0.0)
    got = metrics.quantile_table_host(y, p, 10)
    assert got.tolist() == table_by_loop(y, p, 10)
    assert int(got[:, 0].sum()) == 400 - p[::37].size
    # one score: everything in bin 0; p = 1.0 has q = 2^32
    ones = np.ones(50, np.float32)
    t = metrics.quantile_table_host(ones, ones, 4)
    assert t.tolist() == [[50, 50, 50 * ONE], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    t = metrics.quantile_table_host(np.zeros(9, np.float32), np.zeros(9, np.float32), 3)
    assert t.tolist() == [[9, 0, 0], [0, 0, 0], [0, 0, 0]]
    # two scores, 3 + 5 examples, M = 4: heads at 0 and 3 -> bins 0 and (3 * 4) // 8 = 1
    p2 = np.array([0.25] * 3 + [0.75] * 5, np.float32)
    t = metrics.quantile_table_host(np.zeros(8, np.float32), p2, 4)
    assert t[:, 0].tolist() == [3, 5, 0, 0]
    # no valid example at all
    assert not metrics.quantile_table_host([1.0], [np.nan], 5).any()
    # the table is calibration_from_table's kind of table
    y, p = stream(rng, 500)
    t = metrics.quantile_table_host(y, p, 16)
    res = metrics.calibration_from_table(t, 0)
    assert res["examples"] == 500 and res["CTR"] == float(y.sum()) / 500
    for M in (1, 0, 1025):
        with pytest.raises(ValueError):
            metrics.quantile_table_host(y, p, M)


def test_quantile_table_does_not_depend_on_order():
    rng = np.random.default_rng(6)
    y, p = stream(rng, 600, ties=16)
    want = metrics.quantile_table_host(y, p, 20)
    for order in (rng.permutation(600), np.arange(600)[::-1]):
        assert np.array_equal(metrics.quantile_table_host(y[order], p[order], 20), want)


# ---- the fit ------------------------------------------------------------------------------------------------------------------
def isotonic_by_fractions(rows):
    """The weighted isotonic regression of the non-empty rows' means S / C (weights C), brute force over Fractions: the fitted
    value of row i is max over a <= i of min over b >= i of mean(a .. b).  -> the fitted value per non-empty row."""
    rows = [r for r in rows if r[0]]
    n = len(rows)

    def mean(a, b):
        return Fraction(sum(r[1] for r in rows[a:b + 1]), sum(r[0] for r in rows[a:b + 1]))
    return rows, [max(min(mean(a, b) for b in range(i, n)) for a in range(i + 1)) for i in range(n)]


def blocks_of(rows, fitted):
    """Consecutive rows of one fitted value -> blocks (C, S, Q, fitted value).  Brute force cannot tell two neighbouring blocks of
    EQUAL mean apart, so callers compare knots only on tables where distinct blocks have distinct means."""
    out = []
    for r, f in zip(rows, fitted):
        if out and out[-1][3] == f:
            c, s, q, _ = out[-1]
            out[-1] = (c + r[0], s + r[1], q + r[2], f)
        else:
            out.append((r[0], r[1], r[2], f))
    return out


def knots_of(blocks):
    return ([f32(Fraction(b[2], b[0] << 32)) for b in blocks], [f32(Fraction(b[1], b[0])) for b in blocks])


def q_of(p):
    return math.floor(Fraction(f32(p)) * ONE)


def check_fit(rows):
    x, y = metrics.isotonic_from_table(np.array(rows, np.int64))
    assert x.dtype == np.float32 and y.dtype == np.float32 and x.shape == y.shape and 1 <= x.size <= len(rows)
    assert bool(np.all(x[1:] > x[:-1])) and bool(np.all(y[1:] >= y[:-1]))
    return x, y


def test_fit_of_an_already_monotone_table():
    rows = [[10, 1, 10 * q_of(0.1)], [10, 3, 10 * q_of(0.3)], [10, 6, 10 * q_of(0.55)], [10, 9, 10 * q_of(0.9)]]
    x, y = check_fit(rows)
    live, fitted = isotonic_by_fractions(rows)
    assert fitted == [Fraction(r[1], r[0]) for r in rows]                  # nothing to pool
    wx, wy = knots_of(blocks_of(live, fitted))
    assert x.tolist() == wx and y.tolist() == wy and x.size == 4
    assert y.tolist() == [f32(0.1), f32(0.3), f32(0.6), f32(0.9)]


def test_fit_of_a_fully_reversed_table_is_one_knot():
    rows = [[10, 9, 10 * q_of(0.1)], [10, 6, 10 * q_of(0.3)], [10, 3, 10 * q_of(0.55)], [10, 1, 10 * q_of(0.9)]]
    x, y = check_fit(rows)
    live, fitted = isotonic_by_fractions(rows)
    assert len(set(fitted)) == 1
    wx, wy = knots_of(blocks_of(live, fitted))
    assert x.tolist() == wx and y.tolist() == wy and x.size == 1
    assert y.tolist() == [f32(Fraction(19, 40))] and x.tolist() == [f32(Fraction(sum(r[2] for r in rows), 40 << 32))]


def test_fit_skips_empty_rows_and_pools_violators():
    rows = [[0, 0, 0], [8, 2, 8 * q_of(0.05)], [0, 0, 0], [4, 3, 4 * q_of(0.2)], [12, 3, 12 * q_of(0.4)], [0, 0, 0],
            [6, 2, 6 * q_of(0.5)], [5, 5, 5 * q_of(0.97)], [0, 0, 0]]
    x, y = check_fit(rows)
    live, fitted = isotonic_by_fractions(rows)
    assert len(live) == 5
    # no two distinct blocks of this table share a mean, so blocks of equal fitted value are exactly the pooled ones
    wx, wy = knots_of(blocks_of(live, fitted))
    assert x.tolist() == wx and y.tolist() == wy
    assert x.size == 3 and y.tolist() == [f32(0.25), f32(Fraction(8, 22)), 1.0]
    with pytest.raises(ValueError):
        metrics.isotonic_from_table(np.zeros((4, 3), np.int64))


def test_fit_random_tables_against_brute_force():
    rng = np.random.default_rng(8)
    for _ in range(30):
        M = int(rng.integers(2, 12))
        c = rng.integers(0, 9, M)
        s = np.array([rng.integers(0, ci + 1) for ci in c])
        centres = np.sort(rng.random(M)).astype(np.float32)
        rows = [[int(ci), int(si), int(ci) * q_of(pi)] for ci, si, pi in zip(c, s, centres)]
        if not c.any():
            continue
        x, y = check_fit(rows)
        live, fitted = isotonic_by_fractions(rows)
        # every knot's y is a fitted value of the isotonic regression and every fitted value has its knot, whatever the
        # (unpooled) equal means do to the number of knots; the examples are all there
        assert sorted(set(y.tolist())) == sorted(set(f32(f) for f in fitted))
        assert x.size >= len(set(fitted))
        # the map evaluated at a row's own mean score lies between the fitted values of its neighbours in the regression
        got = metrics.isotonic_apply_host(np.array([f32(Fraction(r[2], r[0] << 32)) for r in live], np.float32), x, y)
        assert bool(np.all(got[1:] >= got[:-1])) and got[0] >= f32(fitted[0]) and got[-1] <= f32(fitted[-1])


def test_equal_means_are_not_pooled():
    rows = [[10, 5, 10 * q_of(0.2)], [20, 10, 20 * q_of(0.4)], [4, 2, 4 * q_of(0.6)], [10, 9, 10 * q_of(0.8)]]
    x, y = check_fit(rows)
    assert x.size == 4 and y.tolist() == [0.5, 0.5, 0.5, f32(0.9)]
    assert x.tolist() == [f32(0.2), f32(0.4), f32(0.6), f32(0.8)]
    # a violator pooled INTO an equal mean stays apart from its equal neighbour: (6, 4) + (2, 0) = (8, 4) next to (10, 5)
    rows = [[10, 5, 10 * q_of(0.2)], [6, 4, 6 * q_of(0.4)], [2, 0, 2 * q_of(0.5)], [10, 9, 10 * q_of(0.8)]]
    x, y = check_fit(rows)
    assert y.tolist() == [0.5, 0.5, f32(0.9)] and x.size == 3


def test_blocks_whose_x_collide_in_fp32_are_pooled():
    """Two bins whose mean scores differ by less than half an ulp of fp32: q sums that differ, x that do not."""
    p = np.float32(0.75)
    q = q_of(p)
    rows = [[4, 1, 4 * q_of(0.1)], [1 << 20, 1 << 18, (1 << 20) * q], [1 << 20, 1 << 19, (1 << 20) * q + 3], [4, 4, 4 * q_of(0.9)]]
    a, b = Fraction(rows[1][2], rows[1][0] << 32), Fraction(rows[2][2], rows[2][0] << 32)
    assert a < b and f32(a) == f32(b)                            # distinct means of p, one fp32
    x, y = check_fit(rows)
    assert x.size == 3
    assert x.tolist() == [f32(0.1), f32(Fraction(rows[1][2] + rows[2][2], 2 << 52)), f32(0.9)]
    assert y.tolist() == [0.25, f32(Fraction(3 << 18, 2 << 20)), 1.0]


# ---- the map ------------------------------------------------------------------------------------------------------------------
def apply_by_struct(p, x, y):
    """The map for one value, each operation rounded to fp32 through numpy scalars (the definition read literally)."""
    u = bits_of(p)
    if u == 0x80000000:
        u = 0
    if u > 0x3F800000:
        return bits_of(p) if not math.isnan(p) else None
    v = np.float32(struct.unpack("<f", struct.pack("<I", u))[0])
    K = len(x)
    if v <= x[0]:
        return bits_of(y[0])
    if v >= x[K - 1]:
        return bits_of(y[K - 1])
    j = max(i for i in range(K) if x[i] <= v)
    t = np.float32(np.float32(v - x[j]) / np.float32(x[j + 1] - x[j]))
    o = np.float32(y[j] + np.float32(t * np.float32(y[j + 1] - y[j])))
    return bits_of(min(o, y[j + 1]))


def neighbours(x):
    x = np.asarray(x, np.float32)
    v = np.concatenate([x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2))])
    return v[(v >= 0) & (v <= 1)].astype(np.float32)


def test_apply_at_knots_below_above_and_between():
    x = np.array([0.125, 0.25, 0.5, 0.75], np.float32)
    y = np.array([0.0625, 0.25, 0.25, 0.875], np.float32)
    assert metrics.isotonic_apply_host(x, x, y).tolist() == y.tolist()                # exact at every knot
    lo = np.array([0.0, -0.0, 1e-45, 0.1, 0.125], np.float32)
    assert metrics.isotonic_apply_host(lo, x, y).tolist() == [0.0625] * 5
    hi = np.array([0.75, 0.8, 1.0], np.float32)
    assert metrics.isotonic_apply_host(hi, x, y).tolist() == [0.875] * 3
    mid = np.array([0.1875, 0.3, 0.625], np.float32)
    assert metrics.isotonic_apply_host(mid, x, y).tolist() == [0.15625, 0.25, 0.5625]
    rng = np.random.default_rng(9)
    p = np.concatenate([rng.random(300).astype(np.float32), neighbours(x), np.array([1e-40, 2e-45], np.float32)])
    got = metrics.isotonic_apply_host(p, x, y)
    assert got.dtype == np.float32 and got.view(np.uint32).tolist() == [apply_by_struct(v, x, y) for v in p]
    # one knot: a constant; shapes are kept
    one = metrics.isotonic_apply_host(np.array([[0.0, 0.3], [1.0, np.inf]], np.float32), [0.4], [0.7])
    assert one.shape == (2, 2) and one.reshape(-1)[:3].tolist() == [f32(0.7)] * 3 and one[1, 1] == np.inf


def test_apply_returns_invalid_inputs_bit_for_bit():
    x, y = np.array([0.2, 0.6], np.float32), np.array([0.1, 0.9], np.float32)
    bits = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0xBF800000, 0x40000000, 0x3F800001, 0x80000001,
                     0x80000000, 0x00000000, 0x3F800000], np.uint32)
    got = metrics.isotonic_apply_host(bits.view(np.float32), x, y).view(np.uint32)
    assert got[:9].tolist() == bits[:9].tolist()                  # NaN payloads, infinities, -1, 2, 1 + ulp, -denormal
    assert got[9:].tolist() == [bits_of(f32(0.1)), bits_of(f32(0.1)), bits_of(f32(0.9))]      # -0.0 is +0.0: y[0]


def fitted_map(M, n=65836, seed=20190625):
    rng = np.random.default_rng(seed)
    s = 1.0 / (1.0 + np.exp(-rng.normal(-1.1, 1.2, 2 * n)))
    y = (rng.random(2 * n) < s).astype(np.float32)
    p = (s * s).astype(np.float32)
    x, yk = metrics.isotonic_from_table(metrics.quantile_table_host(y[:n], p[:n], M))
    return x, yk, y, p, n


def test_a_fitted_1024_bin_map_is_monotone_across_every_knot():
    x, y, _, p, n = fitted_map(1024)
    assert 2 <= x.size <= 1024
    v = np.sort(np.concatenate([neighbours(x), p[:4000], np.array([0.0, 1.0], np.float32)]))
    out = metrics.isotonic_apply_host(v, x, y)
    assert bool(np.all(out[1:] >= out[:-1]))
    assert out[0] == y[0] and out[-1] == y[-1]


def ece20(labels, prob):
    table, invalid = metrics.calibration_bins_host(labels, prob, 20)
    assert invalid == 0
    return metrics.calibration_from_table(table, 0)["ECE"]


@pytest.mark.parametrize("M", [16, 64, 256, 1024])
def test_fit_on_one_half_calibrates_the_other(M):
    """s = sigmoid(N(-1.1, 1.2)), labels Bernoulli(s), reported probability s^2: the held-out 20-bin ECE is 0.166 raw and
    0.007 .. 0.009 mapped (K = 16 / 45 / 67 / 83 knots at M = 16 / 64 / 256 / 1024 in the recipe's own run).  The bound -- a
    quarter of the raw figure -- leaves a factor of about 5 over what the definition alone achieves: it tests the plumbing."""
    x, yk, y, p, n = fitted_map(M)
    raw = ece20(y[n:], p[n:])
    cal = ece20(y[n:], metrics.isotonic_apply_host(p[n:], x, yk))
    print("M = %d: K = %d, held-out ECE raw %.4f -> calibrated %.4f" % (M, x.size, raw, cal))
    assert 0.1 < raw < 0.25
    assert cal < raw / 4
    assert 1 <= x.size <= M


# ---- IsotonicMap ----------------------------------------------------------------------------------------------------------------
def test_isotonic_map_json_round_trip():
    x, y, _, _, _ = fitted_map(64, n=4000)
    m = metrics.IsotonicMap(x, y, bins=64, examples=4000, positives=1234, global_step=77, script="deepfm")
    doc = json.loads(json.dumps(m.to_json()))
    assert doc["x_bits"] == [bits_of(v) for v in x] and doc["y_bits"] == [bits_of(v) for v in y]
    assert doc["x"] == [float(v) for v in x] and all(isinstance(v, int) for v in doc["x_bits"] + doc["y_bits"])
    for back in (metrics.IsotonicMap.from_json(doc), metrics.IsotonicMap.from_json(json.dumps(doc))):
        assert back.x.view(np.uint32).tolist() == x.view(np.uint32).tolist()
        assert back.y.view(np.uint32).tolist() == y.view(np.uint32).tolist()
        assert (back.bins, back.examples, back.positives, back.global_step, back.script) == (64, 4000, 1234, 77, "deepfm")
        assert back.knots == x.size
    # the readable floats are never read back: the bit patterns are the map
    doc2 = dict(doc, x=[0.0] * len(doc["x"]))
    assert metrics.IsotonicMap.from_json(doc2).x.tolist() == x.tolist()


def test_isotonic_map_save_and_load(tmp_path):
    m = metrics.IsotonicMap([0.25, 0.5], [0.125, 0.75], bins=2, examples=10, positives=4, global_step=3, script="din")
    path = str(tmp_path / "calibration-3.json")
    m.save(path)
    assert os.listdir(str(tmp_path)) == ["calibration-3.json"]
    back = metrics.IsotonicMap.load(path)
    assert back.to_json() == m.to_json()


def test_isotonic_map_refusals():
    good = metrics.IsotonicMap([0.25, 0.5], [0.125, 0.75]).to_json()

    def bad(**kw):
        with pytest.raises(ValueError):
            metrics.IsotonicMap.from_json(dict(good, **kw))
    b = bits_of
    bad(format="something.else")
    bad(format=None)
    bad(x_bits=[b(0.25)])                                         # unequal lengths
    bad(x_bits=[], y_bits=[])                                     # K = 0
    bad(x_bits=[b(f32(i / 2000)) for i in range(1025)], y_bits=[b(0.5)] * 1025)       # K = 1025
    bad(x_bits=[b(0.5), b(0.5)])                                  # not strictly increasing
    bad(x_bits=[b(0.5), b(0.25)])
    bad(y_bits=[b(0.75), b(0.125)])                               # y decreases
    bad(x_bits=[b(0.25), b(1.5)])                                 # outside [0, 1]
    bad(y_bits=[b(-0.5), b(0.75)])
    bad(y_bits=[b(0.125), 0x7FC00000])                            # NaN
    bad(x_bits=[b(0.25), 1 << 32])
    with pytest.raises(ValueError):
        metrics.IsotonicMap.from_json({k: v for k, v in good.items() if k != "x_bits"})
    with pytest.raises(ValueError):
        metrics.IsotonicMap([0.5, 0.25], [0.1, 0.2])
    assert metrics.IsotonicMap.from_json(dict(good, y_bits=[b(0.5), b(0.5)])).y.tolist() == [0.5, 0.5]      # equal y is fine
    full = [f32(i / 1024) for i in range(1024)]
    assert metrics.IsotonicMap(full, full).knots == 1024


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script", ["fm", "deepfm", "dcn", "xdeepfm", "din"])
def test_calibration_map_flags_on_every_script(script):
    mod = importlib.import_module("recsys_amd." + script)
    got = mod.define_flags().parse_args(["--calibration_fit", "64", "--calibration_apply", "true", "--export_calibration",
                                         "require"])
    assert got.calibration_fit == 64 and got.calibration_apply is True and got.export_calibration == "require"
    off = mod.define_flags().parse_args([])
    assert off.calibration_fit == 0 and off.calibration_apply is False and off.export_calibration == "auto"
    with pytest.raises(SystemExit):
        mod.define_flags().parse_args(["--export_calibration", "maybe"])


def test_run_config_defaults_and_world_check():
    from recsys_amd.estimator import RunConfig
    assert RunConfig().calibration_fit == 0 and RunConfig().calibration_apply is False
    metrics.check_single_replica("calibration map", 1)
    with pytest.raises(RsxError, match="data-parallel evaluation is not supported"):
        metrics.check_single_replica("calibration map", 2)


def test_symbols_are_exported_and_declared():
    from recsys_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rsx.h")).read()
    for name in ("rsx_calibration_quantile_table", "rsx_calibrate_apply"):
        assert name in _lib.exported_symbols()
        assert "int %s(" % name in header


def test_cabi_envelopes_are_checked_before_any_device_call():
    """RSX_EINVAL for everything outside the two entries' envelopes, and the n == 0 no-op of the apply: all of it returns before
    any HIP call, so it runs without a GPU."""
    import ctypes as C
    from recsys_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_uint64 * 64)()
    base = C.cast(buf, C.c_void_p).value
    base = (base + 15) & ~15
    p = C.c_void_p(base)
    EINVAL = -1
    qt = L.rsx_calibration_quantile_table
    assert qt(None, 8, 10, p, None) == EINVAL
    assert qt(p, 8, 10, None, None) == EINVAL
    assert qt(p, -1, 10, p, None) == EINVAL
    assert qt(p, L.rsx_auc_exact_max_keys() + 1, 10, p, None) == EINVAL
    for M in (-1, 0, 1, L.rsx_calibration_max_bins() + 1):
        assert qt(p, 8, M, p, None) == EINVAL
    assert qt(C.c_void_p(base + 4), 8, 10, p, None) == EINVAL               # the keys are read 16 bytes at a time
    assert qt(C.c_void_p(base + 8), 8, 10, p, None) == EINVAL
    assert qt(p, 8, 10, C.c_void_p(base + 4), None) == EINVAL               # the table holds 64-bit words
    ap = L.rsx_calibrate_apply
    assert ap(None, p, 4, p, p, 8, None) == EINVAL
    assert ap(p, None, 4, p, p, 8, None) == EINVAL
    assert ap(p, p, 4, None, p, 8, None) == EINVAL
    assert ap(p, p, 4, p, None, 8, None) == EINVAL
    assert ap(p, p, 4, p, p, -1, None) == EINVAL
    for K in (-1, 0, 1025):
        assert ap(p, p, K, p, p, 8, None) == EINVAL
    assert ap(p, p, 4, C.c_void_p(base + 2), p, 8, None) == EINVAL
    assert ap(p, p, 1, p, p, 0, None) == 0                                  # n == 0 is a no-op
    assert ap(p, p, 1024, C.c_void_p(base + 4), C.c_void_p(base + 12), 0, None) == 0


def tiny_bundle(tmp_path, extra=None):
    from recsys_amd import serving
    from recsys_amd.feature_columns import build_feature_columns
    lin, emb = build_feature_columns(4, "indicator_all")
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 4, "deep_layers": "8"}
    tensors = {"dense.b1": np.zeros(1, np.float32), "dense.out.W": np.arange(6, dtype=np.float32).reshape(2, 3)}
    manifest = serving.make_manifest("deepfm", params, 12, tensors)
    if extra is None:
        return serving.write_bundle(str(tmp_path), manifest, tensors), manifest, tensors
    return serving.write_bundle(str(tmp_path), manifest, tensors, extra), manifest, tensors


def test_bundle_without_a_map_holds_exactly_its_two_files(tmp_path):
    from recsys_amd import serving
    d, manifest, tensors = tiny_bundle(tmp_path)
    assert sorted(os.listdir(d)) == ["model.json", "variables.npz"]
    got, arrays = serving.read_bundle(d)
    assert got == json.loads(json.dumps(manifest)) and set(arrays) == set(tensors)
    assert "calibration" not in json.dumps(got)


def test_bundle_with_a_map_is_still_read(tmp_path):
    from recsys_amd import serving
    m = metrics.IsotonicMap([0.25, 0.5], [0.125, 0.75], bins=2, examples=10, positives=4, global_step=12, script="deepfm")
    d, manifest, tensors = tiny_bundle(tmp_path, {serving.CALIBRATION: json.dumps(m.to_json())})
    assert sorted(os.listdir(d)) == ["calibration.json", "model.json", "variables.npz"]
    got, arrays = serving.read_bundle(d)                          # the reader reads its two files and nothing else
    assert got == json.loads(json.dumps(manifest)) and all(np.array_equal(arrays[k], tensors[k]) for k in tensors)
    assert got["format_version"] == serving.FORMAT_VERSION
    assert metrics.IsotonicMap.load(os.path.join(d, serving.CALIBRATION)).to_json() == m.to_json()
    plain, _, _ = tiny_bundle(tmp_path)                           # the same manifest bytes with and without the extra file
    assert open(os.path.join(plain, "model.json")).read() == open(os.path.join(d, "model.json")).read()
    for name in ("model.json", "variables.npz", "a/b.json", ""):
        with pytest.raises(RsxError):
            tiny_bundle(tmp_path, {name: "{}"})
