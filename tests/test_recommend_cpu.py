"""serving.recommend_host -- the definition of Predictor.recommend -- against a brute-force loop, and check_catalogue's
refusals.  No device: pure numpy.  Everything is compared bit for bit (uint32 views of the scores, equality of the integers)."""
import numpy as np
import pytest

from recsys_amd import _lib, serving

bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
f32 = lambda u: np.asarray(u, np.uint32).view(np.float32)


def better(a, ia, b, ib):
    """Entry (a, ia) comes before (b, ib) in rsx_topk_rows' order: higher first, -0.0 == +0.0, NaN last, ties by index."""
    na, nb = np.isnan(a), np.isnan(b)
    if na or nb:
        return (not na) if na != nb else ia < ib
    return a > b or (a == b and ia < ib)


def brute(prob, cat, hist, excl, k, seen):
    """One user, with plain loops: eligible positions, then a selection sort by `better`."""
    out = set()
    for x in (list(hist) if seen else []) + (list(excl) if excl is not None else []):
        if x > 0:
            out.add(int(x))
    pos = [j for j in range(len(cat)) if int(cat[j]) not in out]
    picked = []
    while pos and len(picked) < k:
        best = pos[0]
        for j in pos[1:]:
            if better(prob[j], j, prob[best], best):
                best = j
        picked.append(best)
        pos.remove(best)
    return picked


def scores(rng, U, N):
    """Ties (four values), NaNs with different payloads, both zeros."""
    pool = f32([0x3e000000, 0x3f000000, 0x3f000001, 0x3f400000, 0x00000000, 0x80000000, 0x7fc00000, 0xffc00001, 0xbf800000])
    return pool[rng.integers(0, len(pool), (U, N))]


def expect(prob, cat, hist, excl, k, seen):
    U, N = prob.shape
    kk = min(k, N)
    want = {"prob": np.full((U, kk), np.nan, np.float32), "item": np.full((U, kk), -1, np.int32),
            "index": np.full((U, kk), -1, np.int32), "count": np.zeros(U, np.int32)}
    for u in range(U):
        p = brute(prob[u], cat, hist[u], None if excl is None else excl[u], k, seen)
        want["prob"][u, :len(p)], want["item"][u, :len(p)], want["index"][u, :len(p)] = prob[u, p], cat[p], p
        want["count"][u] = len(p)
    return want


def same(got, want):
    assert sorted(got) == ["count", "index", "item", "prob"]
    assert got["prob"].dtype == np.float32 and got["item"].dtype == np.int32 and got["index"].dtype == np.int32
    assert np.array_equal(np.asarray(got["count"]), np.asarray(want["count"]))
    assert np.array_equal(got["index"], want["index"]) and np.array_equal(got["item"], want["item"])
    assert np.array_equal(bits(got["prob"]), bits(want["prob"]))


@pytest.mark.parametrize("seen", [True, False])
@pytest.mark.parametrize("with_excl", [True, False])
def test_against_brute_force(seen, with_excl):
    """Random scores with ties, NaN and -0.0; a catalogue with duplicates and item 0; histories and exclude lists with
    padding (0 and negative) and duplicates; k below, at and above what is eligible."""
    rng = np.random.default_rng(11 + 2 * seen + with_excl)
    for (U, N, k) in ((1, 1, 1), (3, 40, 5), (2, 40, 39), (3, 40, 40), (2, 40, 64), (4, 90, 17)):
        prob = scores(rng, U, N)
        cat = rng.integers(0, 25, N).astype(np.int32)                 # 25 ids over N entries: duplicates
        hist = rng.integers(-1, 25, (U, 6))
        hist[:, 2] = 0
        excl = rng.integers(-2, 25, (U, 4)) if with_excl else None
        got = serving.recommend_host(prob, cat, hist, excl, k, exclude_seen=seen)
        same(got, expect(prob, cat, hist, excl, k, seen))
        assert got["prob"].shape == (U, min(k, N))
        one = serving.recommend_host(prob[0], cat, hist[0], None if excl is None else excl[0], k, exclude_seen=seen)
        c = int(got["count"][0])
        assert isinstance(one["count"], int) and one["count"] == c and one["prob"].shape == (c,)
        assert np.array_equal(one["index"], got["index"][0, :c]) and np.array_equal(one["item"], got["item"][0, :c])
        assert np.array_equal(bits(one["prob"]), bits(got["prob"][0, :c]))


def test_padding_ids_exclude_nothing_and_duplicates_leave_together():
    prob = np.float32([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4]])
    cat = np.int32([0, 7, 3, 7, 5, 7])                               # item 0 is an ordinary entry; item 7 three times
    got = serving.recommend_host(prob, cat, np.int64([[0, -4, 0]]), np.int64([[0, -7]]), 6)
    assert got["count"][0] == 6 and np.array_equal(got["index"][0], np.arange(6))
    got = serving.recommend_host(prob, cat, np.int64([[0, 7, 0]]), None, 6)
    assert got["count"][0] == 3 and np.array_equal(got["item"][0], [0, 3, 5, -1, -1, -1])
    assert np.array_equal(got["index"][0], [0, 2, 4, -1, -1, -1]) and np.isnan(got["prob"][0, 3:]).all()
    assert np.array_equal(bits(got["prob"][0, :3]), bits(np.float32([0.9, 0.7, 0.5])))
    off = serving.recommend_host(prob, cat, np.int64([[0, 7, 0]]), None, 6, exclude_seen=False)
    assert off["count"][0] == 6
    both = serving.recommend_host(prob, cat, np.int64([[7]]), np.int64([[3, 3]]), 2)
    assert np.array_equal(both["item"][0], [0, 5])


def test_short_and_empty_results():
    prob = np.float32([[0.1, 0.2, 0.3], [0.3, 0.2, 0.1]])
    cat = np.int32([4, 5, 6])
    got = serving.recommend_host(prob, cat, np.int64([[4, 5, 6], [5, 0, 0]]), None, 2)
    assert np.array_equal(got["count"], [0, 2]) and np.array_equal(got["item"], [[-1, -1], [4, 6]])
    assert np.isnan(got["prob"][0]).all() and np.array_equal(got["index"], [[-1, -1], [0, 2]])
    big = serving.recommend_host(prob, cat, np.int64([[0], [0]]), None, 10)             # k > N
    assert big["prob"].shape == (2, 3) and np.array_equal(big["count"], [3, 3])
    one = serving.recommend_host(prob[0], cat, np.int64([4, 5, 6]), None, 2)
    assert one["count"] == 0 and one["prob"].shape == (0,) and one["item"].shape == (0,) and one["index"].shape == (0,)


def test_over_fetch_then_filter_is_the_filtered_top_k():
    """What a caller without `recommend` does: the top (k + S) of everything, S = the excluded catalogue entries, then drop
    the excluded ones and cut to k."""
    rng = np.random.default_rng(5)
    for (N, k) in ((60, 7), (60, 50), (200, 20)):
        prob = scores(rng, 1, N)[0]
        cat = rng.integers(1, 40, N).astype(np.int32)
        hist = rng.integers(0, 40, 9)
        S = int(np.isin(cat, hist[hist > 0]).sum())
        top = serving.topk_rows_host(prob, k + S)
        keep = ~np.isin(cat[top["index"]], hist[hist > 0])
        want = serving.recommend_host(prob, cat, hist, None, k)
        assert np.array_equal(top["index"][keep][:k], want["index"])
        assert np.array_equal(bits(top["prob"][keep][:k]), bits(want["prob"]))


def test_recommend_host_refusals():
    prob, cat = np.zeros((2, 5), np.float32), np.arange(5)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(_lib.RsxError, match="top_k"):
            serving.recommend_host(prob, cat, np.zeros((2, 3), np.int64), None, bad)
    with pytest.raises(_lib.RsxError, match="catalogue"):
        serving.recommend_host(prob, np.arange(4), np.zeros((2, 3), np.int64), None, 2)
    with pytest.raises(_lib.RsxError, match="exclude"):
        serving.recommend_host(prob, cat, np.zeros((2, 3), np.int64), np.zeros((3, 2), np.int64), 2)
    with pytest.raises(_lib.RsxError, match="exclude"):
        serving.recommend_host(prob, cat, np.zeros((2, 3), np.int64), np.zeros(2, np.int64), 2)


def test_predictor_refusals_come_before_any_device_work():
    """A Predictor cannot be loaded without a device; a bare instance stands in for it."""
    hist = np.zeros((2, 3), np.int64)
    for script in ("fm", "deepfm", "dcn", "xdeepfm"):
        p = object.__new__(serving.Predictor)
        p.script = script
        with pytest.raises(_lib.RsxError, match=r"recommend: only din.py bundles .* this bundle is %s.py" % script):
            p.recommend(hist, hist, 5)
        with pytest.raises(_lib.RsxError, match=r"set_catalogue: only din.py bundles"):
            p.set_catalogue(np.arange(3), np.arange(3))
        assert p.recommend_path_for(5) is None
    p = object.__new__(serving.Predictor)
    p.script, p._cat = "din", None
    with pytest.raises(_lib.RsxError, match="no catalogue set"):
        p.recommend(hist, hist, 5)
    assert serving.Predictor._excl_capacity(0) == 0 and serving.Predictor._excl_capacity(1) == 32
    assert serving.Predictor._excl_capacity(33) == 64 and serving.Predictor._excl_capacity(256) == 256


def test_check_catalogue():
    ci, cc = serving.check_catalogue(np.int64([0, 5, 5, 299]), np.uint8([0, 1, 1, 19]), 300, 20)
    assert ci.dtype == np.int32 and cc.dtype == np.int32 and np.array_equal(ci, [0, 5, 5, 299]) and np.array_equal(cc, [0, 1, 1, 19])
    ci, _ = serving.check_catalogue([1, 2], [3, 4], 300, 20)
    assert np.array_equal(ci, [1, 2])
    for (a, b, what) in ((np.float32([1, 2]), np.int32([1, 2]), "integers"), (np.int32([1, 2]), np.float64([1, 2]), "integers"),
                         (np.zeros((2, 2), np.int32), np.zeros((2, 2), np.int32), "1-D"),
                         (np.int32([1, 2, 3]), np.int32([1, 2]), "equal length"), (np.int32([]), np.int32([]), "empty"),
                         (np.int32([1, 300]), np.int32([1, 2]), r"i_id holds ids outside \[0, 300\)"),
                         (np.int32([1, -1]), np.int32([1, 2]), "i_id holds ids outside"),
                         (np.int32([1, 2]), np.int32([1, 20]), r"i_cate holds ids outside \[0, 20\)")):
        with pytest.raises(_lib.RsxError, match=what):
            serving.check_catalogue(a, b, 300, 20)
