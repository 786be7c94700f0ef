"""The category rules of serving.recommend_host -- the definition of Predictor.recommend(categories=, exclude_categories=,
max_per_category=) -- against an independent brute force; the property that lets the device keep a running list of only k
entries under a cap (the capped top-k composes over chunks); the defaults; the refusals; the C ABI's envelope.  No device:
pure numpy, everything compared bit for bit."""
import numpy as np
import pytest

from recsys_amd import _lib, serving

bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
f32 = lambda u: np.asarray(u, np.uint32).view(np.float32)


def scores(rng, U, N):
    """Tie groups (four values), NaNs with different payloads, both zeros."""
    pool = f32([0x3e000000, 0x3f000000, 0x3f000001, 0x3f400000, 0x00000000, 0x80000000, 0x7fc00000, 0xffc00001, 0xbf800000])
    return pool[rng.integers(0, len(pool), (U, N))]


def sort_key(v, j):
    """Python's tuple order = rsx_topk_rows' order: numbers before NaNs, higher first (-0.0 == +0.0), ties by position."""
    return (1, 0.0, j) if np.isnan(v) else (0, -float(v), j)


def brute(prob, cat, cc, hist, excl, k, seen, only, deny, m):
    """One user: sort the eligible positions once, then walk them with a per-category counter."""
    out = set(int(x) for x in (list(hist) if seen else []) + (list(excl) if excl is not None else []) if x > 0)
    pos = [j for j in range(len(cat)) if int(cat[j]) not in out
           and (only is None or int(cc[j]) in [int(g) for g in only if g >= 0])
           and (deny is None or int(cc[j]) not in [int(g) for g in deny if g >= 0])]
    pos.sort(key=lambda j: sort_key(prob[j], j))
    count, picked = {}, []
    for j in pos:
        g = int(cc[j])
        if m is not None and count.get(g, 0) >= m:
            continue
        count[g] = count.get(g, 0) + 1
        picked.append(j)
        if len(picked) == k:
            break
    return picked


def expect(prob, cat, cc, hist, excl, k, seen, only, deny, m):
    U, N = prob.shape
    kk = min(k, N)
    want = {"prob": np.full((U, kk), np.nan, np.float32), "item": np.full((U, kk), -1, np.int32),
            "index": np.full((U, kk), -1, np.int32), "count": np.zeros(U, np.int32)}
    for u in range(U):
        p = brute(prob[u], cat, cc, hist[u], None if excl is None else excl[u], kk, seen,
                  None if only is None else only[u], None if deny is None else deny[u], m)
        want["prob"][u, :len(p)], want["item"][u, :len(p)], want["index"][u, :len(p)] = prob[u, p], cat[p], p
        want["count"][u] = len(p)
    return want


def same(got, want):
    assert sorted(got) == ["count", "index", "item", "prob"]
    assert got["prob"].dtype == np.float32 and got["item"].dtype == np.int32 and got["index"].dtype == np.int32
    assert np.array_equal(np.asarray(got["count"]), np.asarray(want["count"]))
    assert np.array_equal(got["index"], want["index"]) and np.array_equal(got["item"], want["item"])
    assert np.array_equal(bits(got["prob"]), bits(want["prob"]))


def lists(rng, U, n_cat, width):
    """[U, width] category lists with padding (negative) and duplicates, different per user."""
    x = rng.integers(-2, n_cat, (U, width))
    if width > 1:
        x[:, 1] = x[:, 0]
    return x


@pytest.mark.parametrize("with_only", [False, True])
@pytest.mark.parametrize("with_deny", [False, True])
@pytest.mark.parametrize("with_excl", [False, True])
def test_against_brute_force(with_only, with_deny, with_excl):
    rng = np.random.default_rng(101 + 4 * with_only + 2 * with_deny + with_excl)
    short = 0
    for trial in range(40):
        U, N = int(rng.integers(1, 4)), int(rng.integers(1, 60))
        k = int(rng.integers(1, N + 8))
        n_cat = int(rng.integers(1, 6))
        m = [None, 1, 2, 3, 4][int(rng.integers(0, 5))]
        prob = scores(rng, U, N)
        cat = rng.integers(0, 25, N).astype(np.int32)
        cc = rng.integers(0, n_cat, N).astype(np.int32)
        hist = rng.integers(-1, 25, (U, 5))
        excl = rng.integers(-2, 25, (U, 3)) if with_excl else None
        only = lists(rng, U, n_cat, 3) if with_only else None
        deny = lists(rng, U, n_cat, 2) if with_deny else None
        if m is None and only is None and deny is None:
            m = 2
        seen = bool(trial % 2)
        got = serving.recommend_host(prob, cat, hist, excl, k, exclude_seen=seen, cat_cate=cc, categories=only,
                                     exclude_categories=deny, max_per_category=m, n_cate=n_cat)
        want = expect(prob, cat, cc, hist, excl, k, seen, only, deny, m)
        same(got, want)
        if m is not None:
            free = serving.recommend_host(prob, cat, hist, excl, k, exclude_seen=seen, cat_cate=cc, categories=only,
                                          exclude_categories=deny)
            short += int((got["count"] < free["count"]).sum())
            for u in range(U):
                c = int(got["count"][u])
                assert c == 0 or np.bincount(cc[got["index"][u, :c]]).max() <= m
        one = serving.recommend_host(prob[0], cat, hist[0], None if excl is None else excl[0], k, exclude_seen=seen, cat_cate=cc,
                                     categories=None if only is None else only[0],
                                     exclude_categories=None if deny is None else deny[0], max_per_category=m)
        c = int(got["count"][0])
        assert isinstance(one["count"], int) and one["count"] == c and one["prob"].shape == (c,)
        assert np.array_equal(one["index"], got["index"][0, :c]) and np.array_equal(bits(one["prob"]), bits(got["prob"][0, :c]))
    assert short > 0                                                 # the cap did shorten lists that eligible entries could fill


def test_hand_made_cases():
    prob = np.float32([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4]])
    cat = np.int32([3, 7, 3, 8, 9, 7])                               # item 3 at two positions, item 7 at two
    cc = np.int32([0, 0, 0, 1, 1, 0])
    none = np.int64([[0]])
    got = serving.recommend_host(prob, cat, none, None, 6, cat_cate=cc, max_per_category=2)
    assert got["count"][0] == 4 and np.array_equal(got["index"][0], [0, 1, 3, 4, -1, -1])      # the cap counts entries
    got = serving.recommend_host(prob, cat, none, None, 2, cat_cate=cc, max_per_category=1)
    assert np.array_equal(got["index"][0], [0, 3]) and got["count"][0] == 2
    got = serving.recommend_host(prob, cat, none, None, 6, cat_cate=cc, categories=np.int64([[0, -1]]))   # category 0 is real
    assert np.array_equal(got["index"][0], [0, 1, 2, 5, -1, -1])
    got = serving.recommend_host(prob, cat, none, None, 6, cat_cate=cc, categories=np.zeros((1, 0), np.int64))
    assert got["count"][0] == 0                                      # an empty allow list allows nothing
    got = serving.recommend_host(prob, cat, none, None, 6, cat_cate=cc, categories=np.int64([[-1, -5]]))
    assert got["count"][0] == 0
    got = serving.recommend_host(prob, cat, none, None, 6, cat_cate=cc, exclude_categories=np.int64([[-1, -5]]))
    assert got["count"][0] == 6                                      # padding denies nothing
    got = serving.recommend_host(prob, cat, none, None, 6, cat_cate=cc, categories=np.int64([[0, 1]]),
                                 exclude_categories=np.int64([[0]]))
    assert np.array_equal(got["index"][0], [3, 4, -1, -1, -1, -1])
    got = serving.recommend_host(prob, cat, np.int64([[3]]), None, 6, cat_cate=cc, max_per_category=1)   # seen, then the cap
    assert np.array_equal(got["index"][0], [1, 3, -1, -1, -1, -1]) and np.array_equal(got["item"][0, :2], [7, 8])
    tie = serving.recommend_host(np.float32([[0.5, 0.5, 0.5]]), np.int32([4, 4, 5]), none, None, 3, cat_cate=np.int32([2, 2, 2]),
                                 max_per_category=2)
    assert np.array_equal(tie["index"][0], [0, 1, -1])               # equal scores: the lower positions are kept


def chunked(prob, cat, cc, hist, excl, k, seen, only, deny, m, cuts):
    """The device's running list, restated through recommend_host: after every chunk only the capped top-k of (the kept list
    + the chunk) survives.  Sub-arrays keep the catalogue's order, so ties go by catalogue position."""
    kept = np.zeros(0, np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        sub = np.concatenate([kept, np.arange(a, b)])
        assert np.all(np.diff(sub) > 0)
        got = serving.recommend_host(prob[sub], cat[sub], hist, excl, k, exclude_seen=seen, cat_cate=cc[sub], categories=only,
                                     exclude_categories=deny, max_per_category=m)
        kept = np.sort(sub[got["index"]])
    final = serving.recommend_host(prob[kept], cat[kept], hist, excl, k, exclude_seen=seen, cat_cate=cc[kept], categories=only,
                                   exclude_categories=deny, max_per_category=m) if len(kept) else None
    return kept if final is None else kept[final["index"]]


def test_capped_top_k_composes_over_chunks():
    """capped_topk(seen + chunk) == capped_topk(capped_topk(seen) + chunk), 600 random cases with tied scores: what
    rsx_topk_rows_rules relies on when it keeps k entries between calls and lets a later call displace them."""
    rng = np.random.default_rng(2024)
    displaced = 0
    for _ in range(600):
        N, n_cat = int(rng.integers(2, 50)), int(rng.integers(1, 6))
        k, m = int(rng.integers(1, 12)), int(rng.integers(1, 5))
        prob = scores(rng, 1, N)[0]
        cat = rng.integers(0, 20, N).astype(np.int32)
        cc = rng.integers(0, n_cat, N).astype(np.int32)
        hist = rng.integers(0, 20, 3)
        deny = rng.integers(-1, n_cat, 1) if rng.random() < 0.3 else None
        inner = np.sort(rng.choice(np.arange(1, N), int(rng.integers(0, min(N - 1, 5) + 1)), replace=False))
        cuts = [0, *inner.tolist(), N]
        want = serving.recommend_host(prob, cat, hist, None, k, cat_cate=cc, exclude_categories=deny, max_per_category=m)
        got = chunked(prob, cat, cc, hist, None, k, True, None, deny, m, cuts)
        assert np.array_equal(got, want["index"]), (N, k, m, cuts)
        if len(cuts) > 2:
            first = serving.recommend_host(prob[:cuts[1]], cat[:cuts[1]], hist, None, k, cat_cate=cc[:cuts[1]],
                                           exclude_categories=deny, max_per_category=m)["index"]
            displaced += int(len(np.setdiff1d(first, want["index"])) > 0)
    assert displaced > 100                                           # entries of the list did leave under later chunks


def test_defaults_are_the_function_without_rules():
    rng = np.random.default_rng(7)
    for (U, N, k) in ((1, 1, 1), (3, 40, 5), (2, 40, 64), (4, 90, 17)):
        prob = scores(rng, U, N)
        cat = rng.integers(0, 25, N).astype(np.int32)
        cc = rng.integers(0, 4, N).astype(np.int32)
        hist, excl = rng.integers(-1, 25, (U, 6)), rng.integers(-2, 25, (U, 4))
        want = expect(prob, cat, cc, hist, excl, k, True, None, None, None)
        same(serving.recommend_host(prob, cat, hist, excl, k), want)
        same(serving.recommend_host(prob, cat, hist, excl, k, True, None, None, None, None), want)
        same(serving.recommend_host(prob, cat, hist, excl, k, cat_cate=cc), want)                  # categories alone: no rule
        same(serving.recommend_host(prob, cat, hist, excl, k, cat_cate=cc, max_per_category=N + 1), want)   # a cap nobody reaches


def test_refusals():
    prob, cat, cc = np.zeros((2, 5), np.float32), np.arange(5), np.int32([0, 1, 2, 0, 1])
    hist = np.zeros((2, 3), np.int64)
    for bad in (0, -1, 1.5, True, np.bool_(True), "2", np.float32(2)):
        with pytest.raises(_lib.RsxError, match="max_per_category"):
            serving.recommend_host(prob, cat, hist, None, 2, cat_cate=cc, max_per_category=bad)
    assert serving.check_max_per_category(np.int64(3)) == 3 and serving.check_max_per_category(None) is None
    for name in ("categories", "exclude_categories"):
        with pytest.raises(_lib.RsxError, match=name + " must hold integers"):
            serving.recommend_host(prob, cat, hist, None, 2, cat_cate=cc, **{name: np.float32([[0.0], [1.0]])})
        with pytest.raises(_lib.RsxError, match=name + " must hold integers"):
            serving.recommend_host(prob, cat, hist, None, 2, cat_cate=cc, **{name: np.array([[True], [False]])})
        with pytest.raises(_lib.RsxError, match=name + r" .* does not match the histories"):
            serving.recommend_host(prob, cat, hist, None, 2, cat_cate=cc, **{name: np.int64([0, 1])})
        with pytest.raises(_lib.RsxError, match=name + r" .* does not match the histories"):
            serving.recommend_host(prob, cat, hist, None, 2, cat_cate=cc, **{name: np.zeros((3, 1), np.int64)})
        with pytest.raises(_lib.RsxError, match=name + r" .* does not match the histories"):
            serving.recommend_host(prob[0], cat, hist[0], None, 2, cat_cate=cc, **{name: np.zeros((1, 1), np.int64)})
        with pytest.raises(_lib.RsxError, match=name + r" holds ids outside \[0, 3\)"):
            serving.recommend_host(prob, cat, hist, None, 2, cat_cate=cc, n_cate=3, **{name: np.int64([[0], [3]])})
        serving.recommend_host(prob, cat, hist, None, 2, cat_cate=cc, n_cate=3, **{name: np.int64([[0], [-9]])})
    for kw in ({"max_per_category": 1}, {"categories": np.int64([[0], [1]])}, {"exclude_categories": np.int64([[0], [1]])}):
        with pytest.raises(_lib.RsxError, match="needs cat_cate"):
            serving.recommend_host(prob, cat, hist, None, 2, **kw)
        with pytest.raises(_lib.RsxError, match="needs cat_cate"):
            serving.recommend_host(prob, cat, hist, None, 2, cat_cate=cc[:4], **kw)
        with pytest.raises(_lib.RsxError, match="needs cat_cate"):
            serving.recommend_host(prob, cat, hist, None, 2, cat_cate=cc.astype(np.float32), **kw)


def test_category_bitmap():
    only = np.int64([[0, 33, -1], [5, 5, 64]])
    deny = np.int64([[33, -2], [-1, -1]])
    bm = serving.category_bitmap(only, None, 70)
    assert bm.dtype == np.uint32 and bm.shape == (2, 3)
    assert bm.tolist() == [[1, 2, 0], [32, 0, 1]]
    assert serving.category_bitmap(only, deny, 70).tolist() == [[1, 0, 0], [32, 0, 1]]
    assert serving.category_bitmap(None, deny, 70).tolist() == [[0xffffffff, 0xfffffffd, 0x3f], [0xffffffff, 0xffffffff, 0x3f]]
    assert serving.category_bitmap(np.zeros((1, 0), np.int64), None, 20).tolist() == [[0]]


def test_predictor_refusals_come_before_any_device_work():
    """A Predictor cannot be loaded without a device; a bare instance stands in for it."""
    hist = np.zeros((2, 3), np.int64)
    p = object.__new__(serving.Predictor)
    p.script = "fm"
    with pytest.raises(_lib.RsxError, match=r"recommend: only din.py bundles"):
        p.recommend(hist, hist, 5, max_per_category=2)
    assert p.recommend_path_for(5, 2) is None and p.recommend_path_for(5, rules=True) is None
    p = object.__new__(serving.Predictor)
    p.script, p._cat = "din", None
    with pytest.raises(_lib.RsxError, match="no catalogue set"):
        p.recommend(hist, hist, 5, categories=np.int64([[1], [2]]))
    with pytest.raises(_lib.RsxError, match="max_per_category"):
        p.recommend_path_for(5, 0)


def test_c_abi_and_envelope():
    L = _lib.lib()
    assert L.rsx_version() >= 106
    assert hasattr(L, "rsx_topk_rows_rules") and hasattr(L, "rsx_topk_rows_rules_supported")
    S = L.rsx_topk_rows_rules_supported
    assert S(4096, 100, 256, 802, 16) == 1
    assert S(4096, 100, 256, 802, 17) == 0 and S(16, 8, 0, 3, 17) == 0
    for k in (1, 100, 1024):
        for m in (1, 16):
            assert S(16384 - k, k, 0, 802, m) == 0, (k, m)           # the plan with 12.8 KB of thresholds and the cache
    assert S(16, 8, 4, 3, -1) == 0 and S(16, 8, 4, -1, 0) == 0 and S(16, 8, 4, 0, 1) == 0
    assert S(16, 8, 257, 3, 1) == 0 and S(16, 1025, 4, 3, 1) == 0 and S(0, 8, 4, 3, 1) == 0
    # without a cap the envelope is rsx_topk_rows_excl's
    for (n, k, E) in ((16384 - 1024, 1024, 256), (16384 - 1023, 1024, 4), (1, 1, 0), (16, 8, 257)):
        assert S(n, k, E, 802, 0) == L.rsx_topk_rows_excl_supported(n, k, E) == S(n, k, E, 0, 0), (n, k, E)
    # with one: 8 (n + k) + 16 k + 2 080 + 16 G + 2 (n + k) bytes of LDS, at most 160 KB
    for (k, G) in ((1024, 802), (100, 802), (8, 20)):
        edge = min(16384, (163840 - 16 * k - 2080 - 16 * G) // 10)
        assert S(edge - k, k, 256, G, 16) == 1 and (edge == 16384 or S(edge + 1 - k, k, 256, G, 16) == 0), (k, G)
