"""The host side of `rank_candidates(top_k=k)`: serving.topk_rows_host -- the order contract of rsx_topk_rows in numpy, and
the checker of tests/test_gpu_topk.py / tests/test_gpu_din_rank_topk.py -- against a brute-force Python `sorted`, and the
argument checks of `top_k`.  No device."""
import math

import numpy as np
import pytest

bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
f32 = lambda u: np.array(u, np.uint32).view(np.float32)


def brute(row, k):
    """(values, indices) of the k best by the tuple key (isnan, -value, index)."""
    row = np.asarray(row, np.float32)
    order = sorted(range(len(row)), key=lambda i: (math.isnan(row[i]), 0.0 if math.isnan(row[i]) else -float(row[i]), i))[:k]
    return row[order], np.array(order, np.int32)


def special_rows():
    rng = np.random.default_rng(11)
    den = f32([1, 2, 0x007fffff, 0x80000001, 0x80000002])                       # +-denormals
    nans = f32([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fc12345])    # +-NaN, payloads
    rows = {
        "ties": rng.integers(0, 4, 41).astype(np.float32),
        "all_equal": np.full(17, 0.5, np.float32),
        "zeros": np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, -0.0], np.float32),
        "inf": np.array([np.inf, -np.inf, 1.0, np.inf, -np.inf, 0.0, 3e38, -3e38], np.float32),
        "denormals": np.concatenate([den, np.array([0.0, -0.0, 1e-38, -1e-38], np.float32)]),
        "nans": np.concatenate([nans[:2], np.array([0.25, 0.75, 0.25], np.float32), nans[2:], np.array([-np.inf, np.inf], np.float32)]),
        "only_nans": nans,
        "mixed": np.concatenate([rng.standard_normal(23).astype(np.float32), nans, den, np.array([0.0, -0.0, np.inf, -np.inf], np.float32)]),
    }
    rows["mixed"] = rows["mixed"][rng.permutation(len(rows["mixed"]))]
    return rows


@pytest.mark.parametrize("name", sorted(special_rows()))
def test_topk_rows_host_against_sorted(name):
    from recsys_amd import serving
    row = special_rows()[name]
    n = len(row)
    for k in (1, n - 1, n, n + 5):
        got = serving.topk_rows_host(row, k)
        wv, wi = brute(row, k)
        assert got["prob"].dtype == np.float32 and got["index"].dtype == np.int32
        assert got["prob"].shape == got["index"].shape == (min(k, n),)
        assert np.array_equal(got["index"], wi), (name, k)
        assert np.array_equal(bits(got["prob"]), bits(wv)), (name, k)               # the input's bits: -0.0, NaN payloads
        assert np.array_equal(bits(got["prob"]), bits(row[got["index"]]))


def test_topk_rows_host_rows_and_shapes():
    from recsys_amd import serving
    rng = np.random.default_rng(5)
    a = rng.integers(0, 6, (3, 29)).astype(np.float32)
    a[1, 4], a[1, 20], a[2, 0] = np.nan, -0.0, np.inf
    got = serving.topk_rows_host(a, 10)
    assert got["prob"].shape == got["index"].shape == (3, 10)
    for u in range(3):
        wv, wi = brute(a[u], 10)
        assert np.array_equal(got["index"][u], wi) and np.array_equal(bits(got["prob"][u]), bits(wv))
        one = serving.topk_rows_host(a[u], 10)
        assert np.array_equal(one["index"], wi) and one["prob"].shape == (10,)
    # np.lexsort((index, -score)) is the contract's own wording
    for u in range(3):
        assert np.array_equal(np.lexsort((np.arange(29), -a[u]))[:10], got["index"][u])
    with pytest.raises(serving._lib.RsxError):
        serving.topk_rows_host(np.zeros((2, 2, 2), np.float32), 1)
    with pytest.raises(serving._lib.RsxError):
        serving.topk_rows_host(np.zeros((2, 0), np.float32), 1)


@pytest.mark.parametrize("bad", [0, -1, 1.0, 2.5, "3", None, True, np.float32(2), [1], np.bool_(True)])
def test_top_k_argument_is_refused(bad):
    from recsys_amd import serving
    with pytest.raises(serving._lib.RsxError, match="top_k must be an integer >= 1"):
        serving.check_top_k(bad)
    if bad is not None:
        with pytest.raises(serving._lib.RsxError, match="top_k must be an integer >= 1"):
            serving.topk_rows_host(np.zeros(4, np.float32), bad)


def test_top_k_argument_is_accepted():
    from recsys_amd import serving
    assert serving.check_top_k(1) == 1 and serving.check_top_k(np.int64(7)) == 7 and serving.check_top_k(np.int32(2000)) == 2000
    assert isinstance(serving.check_top_k(np.int16(3)), int)


def test_rank_candidates_checks_top_k_without_a_device():
    """A Predictor cannot be loaded without a device; a bare instance stands in for it: the script check comes first (a
    non-din bundle raises what it raised before the argument existed), then the request and top_k checks, all before any
    device work."""
    from recsys_amd import serving
    p = object.__new__(serving.Predictor)
    p.script = "deepfm"
    with pytest.raises(serving._lib.RsxError, match="only din.py bundles rank candidates"):
        p.rank_candidates([1], [1], [1], [1], top_k=3)
    p.script, p.rank_path = "din", "fused"
    p.manifest = {"params": {"hist_len": 4, "n_item": 10, "n_cate": 5, "embedding_size": 16}}
    for bad in (0, 1.5, "2", True):
        with pytest.raises(serving._lib.RsxError, match="top_k must be an integer >= 1"):
            p.rank_candidates([1, 2], [1, 2], [1, 2, 3], [1, 1, 1], top_k=bad)
