"""Category rules on the two-stage DIN recommendation, without a GPU: the numpy definitions
(serving.retrieve_candidates_host / recommend_two_stage_host with categories, exclude_categories, max_per_category) against
`recommend_host` on the user's candidate sub-catalogue, their edge cases, and the RSX_EINVAL / RSX_EUNSUPPORTED answers of
rsx_din_retrieve_candidates_rules and rsx_topk_lists_capped before any HIP call."""
import ctypes as C

import numpy as np
import pytest

from recsys_amd import _lib, serving

EINVAL, EUNSUPPORTED = -1, -3
P = C.c_void_p(0x1000)          # "some non-NULL pointer": never read
bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def L():
    from recsys_amd import build
    build.build(verbose=False)
    return _lib.lib()


def random_case(seed, N=120, n=6, U=4, Pn=5, G=7):
    """A random catalogue with duplicated ids, a random neighbour table, histories, scores with ties and NaNs."""
    rng = np.random.default_rng(seed)
    n_item = (7 * N) // 10
    cat = rng.integers(0, n_item, N).astype(np.int32)
    cc = rng.integers(0, G, N).astype(np.int32)
    pos = np.full((N, n), -1, np.int32)
    cnt = rng.integers(0, n + 1, N).astype(np.int32)
    for i in range(N):
        pos[i, :cnt[i]] = rng.choice(N, cnt[i], replace=False)
    hist = rng.integers(0, n_item, (U, Pn)).astype(np.int64)
    prob = np.round(rng.uniform(0, 1, (U, N)), 1).astype(np.float32)          # one decimal: ties everywhere
    prob[rng.random((U, N)) < 0.03] = np.nan
    excl = rng.integers(-1, n_item, (U, 3)).astype(np.int64)
    return rng, cat, cc, pos, cnt, hist, prob, excl, G


def same(got, want):
    assert sorted(got) == sorted(want)
    for key in want:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, key
        assert np.array_equal(bits(g), bits(w)) if g.dtype == np.float32 else np.array_equal(g, w), key


def old_retrieve(pos, cnt, cat, hist, exclude, exclude_seen):
    """`retrieve_candidates_host` as it was before the category arguments, restated from its docstring."""
    cat = np.asarray(cat).astype(np.int64)
    h = np.atleast_2d(np.asarray(hist)).astype(np.int64)
    ids, first = np.unique(cat, return_index=True)
    out = []
    for u in range(h.shape[0]):
        seeds = [int(first[np.searchsorted(ids, v)]) for v in h[u] if v > 0 and v in set(ids.tolist())]
        mark = np.zeros(len(cat), bool)
        for a in seeds:
            mark[pos[a, :cnt[a]]] = True
        named = [h[u]] if exclude_seen else []
        if not exclude_seen:
            mark |= np.isin(cat, cat[seeds])
        if exclude is not None:
            named.append(np.atleast_2d(np.asarray(exclude))[u].astype(np.int64))
        named = np.concatenate(named) if named else np.zeros(0, np.int64)
        mark &= ~np.isin(cat, named[named > 0])
        out.append(np.flatnonzero(mark).astype(np.int32))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_no_rule_given_is_the_present_output(seed):
    rng, cat, cc, pos, cnt, hist, prob, excl, G = random_case(seed)
    for seen in (True, False):
        for ex in (None, excl):
            want = old_retrieve(pos, cnt, cat, hist, ex, seen)
            got = serving.retrieve_candidates_host(pos, cnt, cat, hist, ex, seen)
            also = serving.retrieve_candidates_host(pos, cnt, cat, hist, ex, seen, cat_cate=cc, n_cate=G)
            assert len(got) == len(want) == len(also)
            for g, a, w in zip(got, also, want):
                assert g.dtype == np.int32 and np.array_equal(g, w) and np.array_equal(a, w)
            for k in (1, 7, 500):
                out = serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, ex, k, seen)
                same(serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, ex, k, seen, cat_cate=cc, n_cate=G), out)
                kk = min(k, len(cat))
                for u, w in enumerate(want):                           # the present output, restated: the order restricted
                    w = w.astype(np.int64)
                    order = w[np.lexsort((w, -prob[u, w]))][:kk]
                    assert out["count"][u] == len(order) and np.array_equal(out["index"][u, :len(order)], order)
                    assert np.array_equal(bits(out["prob"][u, :len(order)]), bits(prob[u, order]))
                    assert (out["index"][u, len(order):] == -1).all() and np.isnan(out["prob"][u, len(order):]).all()


def rule_sets(rng, U, G):
    allow = np.full((U, 4), -1, np.int64)
    deny = np.full((U, 3), -1, np.int64)
    for u in range(U):
        allow[u, :3] = rng.choice(G, 3, replace=False)                 # (one slot of padding stays)
        deny[u, :2] = rng.choice(G, 2, replace=False)
    return [dict(categories=allow), dict(exclude_categories=deny), dict(max_per_category=1), dict(max_per_category=2),
            dict(categories=allow, exclude_categories=deny, max_per_category=1),
            dict(exclude_categories=deny, max_per_category=2)]


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_sub_catalogue_identity(seed):
    """recommend_two_stage_host(rules) == recommend_host(rules) on the user's UNFILTERED candidate sub-catalogue, indices
    mapped back through the ascending candidate positions."""
    rng, cat, cc, pos, cnt, hist, prob, excl, G = random_case(seed)
    U, N = prob.shape
    seen_cut = seen_short = seen_filter = seen_tie = False
    for seen in (True, False):
        plain = serving.retrieve_candidates_host(pos, cnt, cat, hist, excl, seen)
        for rules in rule_sets(rng, U, G):
            filters = {k: v for k, v in rules.items() if k != "max_per_category"}
            for k in (3, 10, 200):
                got = serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, excl, k, seen, cat_cate=cc, n_cate=G, **rules)
                free = serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, excl, k, seen)
                cands = serving.retrieve_candidates_host(pos, cnt, cat, hist, excl, seen, cat_cate=cc, n_cate=G, **filters)
                kk = min(k, N)
                assert got["prob"].shape == (U, kk)
                for u in range(U):
                    Cu = plain[u].astype(np.int64)
                    c = int(got["count"][u])
                    assert set(cands[u].tolist()) <= set(Cu.tolist())
                    seen_filter |= 0 < len(cands[u]) < len(Cu)
                    if len(Cu) == 0:
                        assert c == 0
                        continue
                    one = {key: v[u] for key, v in filters.items()}
                    sub = serving.recommend_host(prob[u, Cu], cat[Cu], np.zeros(1, np.int64), None, kk, exclude_seen=False,
                                                 cat_cate=cc[Cu], n_cate=G, max_per_category=rules.get("max_per_category"), **one)
                    assert c == sub["count"] <= kk
                    assert np.array_equal(got["index"][u, :c], Cu[sub["index"]])
                    assert np.array_equal(got["item"][u, :c], sub["item"]) and np.array_equal(bits(got["prob"][u, :c]), bits(sub["prob"]))
                    assert (got["index"][u, c:] == -1).all() and (got["item"][u, c:] == -1).all() and np.isnan(got["prob"][u, c:]).all()
                    if "max_per_category" in rules:
                        m = rules["max_per_category"]
                        assert np.bincount(cc[got["index"][u, :c]], minlength=G).max(initial=0) <= m
                        if not filters:
                            fi = free["index"][u, :free["count"][u]]
                            seen_cut |= bool(set(fi.tolist()) - set(got["index"][u, :c].tolist()))
                            seen_short |= free["count"][u] == kk and c < kk
                    v = got["prob"][u, :c]
                    seen_tie |= bool(np.any((v[1:] == v[:-1]) & (got["index"][u, 1:c] > got["index"][u, :c - 1])))
    assert seen_cut and seen_short and seen_filter and seen_tie


def test_edge_cases():
    rng, cat, cc, pos, cnt, hist, prob, excl, G = random_case(21)
    U = prob.shape[0]
    r = lambda **kw: serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, None, 10, cat_cate=cc, n_cate=G, **kw)
    # an empty `categories` list allows nothing
    out = r(categories=np.zeros((U, 0), np.int64))
    assert out["count"].tolist() == [0] * U and (out["index"] == -1).all()
    assert all(len(x) == 0 for x in serving.retrieve_candidates_host(pos, cnt, cat, hist, cat_cate=cc, categories=np.zeros((U, 0), np.int64)))
    # padding -1 is ignored; 0 is a real category
    a = r(categories=np.int64([[0, 2]] * U), exclude_categories=np.int64([[3]] * U), max_per_category=2)
    b = r(categories=np.int64([[-1, 0, -7, 2, -1]] * U), exclude_categories=np.int64([[-1, 3, -1]] * U), max_per_category=2)
    same(a, b)
    assert a["count"].sum() > 0 and set(cc[a["index"][a["index"] >= 0]].tolist()) <= {0, 2}
    assert 0 in set(cc[a["index"][a["index"] >= 0]].tolist())
    # denying through padding only denies nothing
    same(r(exclude_categories=np.int64([[-1, -1]] * U)), serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, None, 10))
    # ids >= n_cate are refused; a rule without cat_cate is refused; a bad cap is refused
    for kw in (dict(categories=np.int64([[G]] * U)), dict(exclude_categories=np.int64([[1, G + 3]] * U))):
        with pytest.raises(_lib.RsxError, match="outside"):
            r(**kw)
        with pytest.raises(_lib.RsxError, match="outside"):
            serving.retrieve_candidates_host(pos, cnt, cat, hist, cat_cate=cc, n_cate=G, **kw)
    for kw in (dict(categories=np.int64([[1]] * U)), dict(exclude_categories=np.int64([[1]] * U)), dict(max_per_category=1)):
        with pytest.raises(_lib.RsxError, match="cat_cate"):
            serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, None, 10, **kw)
    with pytest.raises(_lib.RsxError, match="cat_cate"):
        serving.retrieve_candidates_host(pos, cnt, cat, hist, categories=np.int64([[1]] * U))
    with pytest.raises(_lib.RsxError, match="cat_cate"):
        serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, None, 10, cat_cate=cc[:-1], max_per_category=1)
    for bad in (0, -1, True, 1.5):
        with pytest.raises(_lib.RsxError, match="max_per_category"):
            r(max_per_category=bad)
    with pytest.raises(_lib.RsxError):                                    # [G'] for U users: the wrong shape
        r(categories=np.int64([1, 2]))
    # the one-user form is cut to count
    full = r(exclude_categories=np.int64([[1]] * U), max_per_category=1)
    one = serving.recommend_two_stage_host(prob[2], pos, cnt, cat, hist[2], None, 10, cat_cate=cc, n_cate=G,
                                           exclude_categories=np.int64([1]), max_per_category=1)
    c = int(full["count"][2])
    assert isinstance(one["count"], int) and one["count"] == c and 0 < c < 10 and one["index"].shape == (c,)
    assert np.array_equal(one["index"], full["index"][2, :c]) and np.array_equal(bits(one["prob"]), bits(full["prob"][2, :c]))
    assert np.array_equal(one["item"], full["item"][2, :c])
    # seeds are unaffected: denying the category of a history item keeps its neighbours
    shown = False
    for u in range(U):
        for v in hist[u]:
            at = np.flatnonzero(cat == v)
            if v > 0 and len(at) and cnt[at[0]] > 0:                      # a seed with neighbours: deny ITS category
                deny = np.int64([cc[at[0]]])
                kept = serving.retrieve_candidates_host(pos, cnt, cat, hist[u], cat_cate=cc, exclude_categories=deny)[0]
                allc = serving.retrieve_candidates_host(pos, cnt, cat, hist[u])[0]
                assert np.array_equal(kept, allc[cc[allc] != deny[0]])
                shown |= bool(set(pos[at[0], :cnt[at[0]]].tolist()) & set(kept.tolist())) and len(kept) < len(allc)
    assert shown


def _bare(**kw):
    p = object.__new__(serving.Predictor)
    p.script, p._cat, p._nbr = "din", None, None
    p.manifest = {"params": {"hist_len": 4, "n_item": 10, "n_cate": 3, "embedding_size": 16}}
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_predictor_argument_refusals():
    h = np.int64([1, 2])
    assert "not offered" not in serving.Predictor.recommend_two_stage.__doc__
    p = _bare()
    with pytest.raises(_lib.RsxError, match="set_catalogue"):
        p.recommend_two_stage(h, h, 3, categories=np.int64([1]), exclude_categories=np.int64([2]), max_per_category=1)
    with pytest.raises(_lib.RsxError, match="set_catalogue"):
        p.retrieve_candidates(h, h, categories=np.int64([1]), exclude_categories=np.int64([2]))
    d = _bare(script="deepfm")
    assert d.two_stage_path_for(3, None, 2, rules=True) is None and d.two_stage_path_for(3, max_per_category=1) is None
    # (the catalogue of tests/test_two_stage_cpu.py) with host tables only: the arguments are checked before any device is asked
    CAT = np.int32([5, 7, 5, 9, 0, 8])
    EMB = np.float32([[2, 0], [5, 0], [0, 3], [0, 0], [3, 4], [-1, 0]])
    pos, sim, cnt = serving.item_neighbours_host(serving.unit_rows_host(EMB), CAT, 2)
    cat = {"host": (CAT, np.int32([0, 1, 2, 0, 1, 2])), "first": serving.catalogue_first_positions(CAT)}
    p = _bare(_cat=cat, catalogue_size=6, _nbr={"n": 2, "host": (pos, sim, cnt)})
    for kw in (dict(categories=np.int64([3])), dict(exclude_categories=np.int64([0, 9])), dict(categories=np.float32([1.0])),
               dict(categories=np.int64([[1]]))):
        with pytest.raises(_lib.RsxError, match="categories"):
            p.recommend_two_stage(h, h, 3, **kw)
        with pytest.raises(_lib.RsxError, match="categories"):
            p.retrieve_candidates(h, h, **kw)
    for bad in (0, True, 1.5):
        with pytest.raises(_lib.RsxError, match="max_per_category"):
            p.recommend_two_stage(h, h, 3, max_per_category=bad)
        with pytest.raises(_lib.RsxError, match="max_per_category"):
            p.two_stage_path_for(3, max_per_category=bad)


def test_new_entries_refuse_before_any_hip_call(L):
    assert L.rsx_version() == 107
    names = {"rsx_din_retrieve_candidates_rules", "rsx_din_retrieve_candidates_rules_supported", "rsx_topk_lists_capped",
             "rsx_topk_lists_capped_supported"}
    assert names <= set(_lib.exported_symbols()) and all(hasattr(L, n) for n in names)
    # rsx_din_retrieve_candidates_rules(hist, P, first_pos, n_item, nbr_pos, nbr_count, n_nbr, cat_item, cat_cate, N, excl, E,
    #                                   seeds, allow, G, cand_pos, cand_item, cand_cate, n_cand, cap, U, stream)
    ok = [P, 100, P, 500, P, P, 32, P, P, 400, P, 32, 0, P, 802, P, P, P, P, 448, 2, None]

    def ret(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.rsx_din_retrieve_candidates_rules(*a)
    for i in (0, 2, 4, 5, 7, 8, 10, 15, 16, 17, 18):
        assert ret(**{"a%d" % i: None}) == EINVAL, i
        assert ret(**{"a%d" % i: None, "a13": None}) == EINVAL, i      # (allow == NULL: the old entry's answers)
    for i, v in ((1, 0), (3, 0), (6, 0), (9, 0), (11, -1), (19, 0), (20, 0), (14, 0), (14, -5)):
        assert ret(**{"a%d" % i: v}) == EINVAL, (i, v)
    for i, v in ((9, (1 << 20) + 1), (1, 129), (6, 65), (11, 257), (14, 65537)):
        assert ret(**{"a%d" % i: v}) == EUNSUPPORTED, (i, v)
    # the stated bound on G: 65 536 categories, an allow row of 8 KB -- on both sides, at the largest bitmap
    sup = L.rsx_din_retrieve_candidates_rules_supported
    assert sup(1 << 20, 128, 64, 256, 65536) == 1 and sup(1 << 20, 128, 64, 256, 65537) == 0
    assert sup(63001, 100, 32, 64, 802) == 1 and sup(63001, 100, 32, 64, 1) == 1 and sup(63001, 100, 32, 64, 0) == 0
    for old in ((1 << 20) + 1, 128, 64, 256), (63001, 129, 64, 0), (63001, 100, 65, 0), (63001, 100, 32, 257):
        assert sup(*old, 802) == 0 and L.rsx_din_retrieve_candidates_supported(*old) == 0
    assert 4 * (32768 + 3 * 128 + 2 * 256 + 16 + 65536 // 32) == 142912 <= 160 * 1024        # the plan the contract states

    # rsx_topk_lists_capped(scores, ld, n_valid, cate, ld_cate, G, m, U, n, k, out_val, out_idx, state, stream)
    ok = [P, 8, P, P, 8, 5, 2, 1, 8, 4, P, P, P, None]

    def cap(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.rsx_topk_lists_capped(*a)
    for i in (0, 2, 3, 10, 11, 12):
        assert cap(**{"a%d" % i: None}) == EINVAL, i
    for i, v in ((1, 7), (4, 7), (5, 0), (5, -1), (6, -1), (7, 0), (8, 0), (9, 0)):
        assert cap(**{"a%d" % i: v}) == EINVAL, (i, v)
    for i in (0, 2, 10, 11, 12):                                       # m == 0: rsx_topk_rows_counted's refusals; cate may be NULL
        assert cap(a6=0, a3=None, **{"a%d" % i: None}) == EINVAL, i
    assert cap(a6=0, a1=7) == EINVAL and cap(a6=0, a7=0) == EINVAL
    assert cap(a6=17) == EUNSUPPORTED and cap(a9=1025, a1=2000, a4=2000, a8=2000) == EUNSUPPORTED
    assert cap(a5=65536) == EUNSUPPORTED and cap(a1=16384, a4=16384, a8=16384, a9=1) == EUNSUPPORTED
    assert cap(a6=0, a3=None, a9=1025) == EUNSUPPORTED
    sup = L.rsx_topk_lists_capped_supported
    # the stated plan: 10 (n + k) + 16 k + 1 056 + 16 G <= 163 840
    fits = lambda n, k, G: 10 * (n + k) + 16 * k + 1056 + 16 * G <= 163840
    assert fits(13356 - 1024, 1024, 802) and not fits(13357 - 1024, 1024, 802)
    assert sup(13356 - 1024, 1024, 802, 1) == 1 and sup(13357 - 1024, 1024, 802, 1) == 0
    assert sup(13356 - 1024, 1024, 802, 16) == 1 and sup(13357 - 1024, 1024, 802, 16) == 0
    for n, k, G in ((3328, 1024, 802), (3328, 100, 802), (64, 1, 1), (100, 10, 65535), (12000, 1024, 2000), (9000, 500, 3000)):
        assert sup(n, k, G, 2) == (1 if fits(n, k, G) and n + k <= 16384 else 0), (n, k, G)
    assert 10 * (3328 + 1024) + 16 * 1024 + 1056 + 16 * 802 == 73792
    assert sup(3328, 1024, 802, 17) == 0 and sup(3328, 1024, 802, -1) == 0 and sup(3328, 1024, 65536, 1) == 0
    assert sup(3328, 1024, 0, 1) == 0 and sup(3328, 1024, -1, 0) == 0
    # m == 0: rsx_topk_rows' envelope, whatever G
    for n, k in ((15360, 1024), (15361, 1024), (8, 1025), (16383, 1), (16384, 1)):
        assert sup(n, k, 802, 0) == L.rsx_topk_rows_supported(n, k) == sup(n, k, 0, 0), (n, k)
