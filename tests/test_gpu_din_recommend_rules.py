"""`Predictor.recommend` with category rules on the GPU (categories / exclude_categories / max_per_category): the device request
-- rsx_topk_rows_rules in rsx_topk_rows_excl's place, one graph per request shape -- against serving.recommend_host with the
same rules over the probabilities `rank_candidates` gives for the catalogue, bit for bit (uint32 views of `prob`, equality of
the integers); what the rules visibly do; graph replay; the launch count; the plain request beside it; path selection."""
import numpy as np
import pytest

from tests.test_gpu_din_rank import N_CATE, bits, din_bundle
from tests.test_gpu_din_recommend import catalogue, histories, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def probabilities(p, hi, hc):
    ci, cc = p._cat["host"]
    U = hi.shape[0]
    return p.rank_candidates(hi, hc, np.tile(ci, (U, 1)), np.tile(cc, (U, 1)))["prob"]


def definition(p, prob, hi, k, exclude_seen=True, exclude=None, **rules):
    from recsys_amd import serving
    ci, cc = p._cat["host"]
    return serving.recommend_host(prob, ci, hi, exclude, k, exclude_seen, cat_cate=cc, n_cate=N_CATE, **rules)


def category_lists(rng, U):
    """Per-user allow and deny lists that differ between users, with padding and a duplicate; category 0 is in nobody's
    catalogue entry and is a legal id."""
    only = np.stack([np.concatenate([rng.permutation(np.arange(1, N_CATE))[:8], [-1, 0]]) for _ in range(U)])
    deny = np.stack([np.concatenate([rng.permutation(np.arange(1, N_CATE))[:3], [-4]]) for _ in range(U)])
    deny[:, 1] = only[:, 0]
    return only, deny


@pytest.mark.parametrize("K", [16, 32])
@pytest.mark.parametrize("max_c", [64, 1024])
def test_recommend_with_rules_equals_its_definition(tmp_path_factory, K, max_c):
    """max_candidates 64: five chunks, the last one short (299 = 4 x 64 + 43); 1024: one chunk."""
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, K, 30)
    p = serving.Predictor.load(d, max_batch_size=256, max_candidates=max_c)
    p.rules_on_device = True
    ci, cc = catalogue()
    p.set_catalogue(ci, cc)
    rng = np.random.default_rng(181 + K + max_c)
    for U in (1, 3):
        hi, hc = histories(rng, U, ["hole", "empty", "full"][:U])
        prob = probabilities(p, hi, hc)
        only, deny = category_lists(rng, U)
        extra = rng.integers(-1, 300, (U, 5))
        for k in (1, 10, 150):
            for m in (None, 1, 3):
                for lists in ({}, {"categories": only}, {"exclude_categories": deny}, {"categories": only, "exclude_categories": deny}):
                    if m is None and not lists:
                        continue
                    rules = dict(lists, max_per_category=m)
                    for seen, excl in ((True, None), (False, extra), (True, extra)):
                        want = definition(p, prob, hi, k, seen, excl, **rules)
                        got = p.recommend(hi, hc, k, exclude_seen=seen, exclude=excl, **rules)
                        assert p.recommend_path == "device" and p.recommend_path_for(k, m, rules=True) == "device"
                        same(got, want)
                        for u in range(U):
                            c = int(got["count"][u])
                            cats = cc[got["index"][u, :c]]
                            assert m is None or c == 0 or np.bincount(cats).max() <= m
                            assert "categories" not in lists or np.isin(cats, only[u]).all()
                            assert "exclude_categories" not in lists or not np.isin(cats, deny[u][deny[u] >= 0]).any()
                    if U == 1:                                       # the one-user form: 1-D in, arrays cut to count
                        one = p.recommend(hi[0], hc[0], k, **{key: (v[0] if key != "max_per_category" else v) for key, v in rules.items()})
                        want = definition(p, prob, hi, k, **rules)
                        c = int(want["count"][0])
                        assert isinstance(one["count"], int) and one["count"] == c and one["item"].shape == (c,)
                        assert np.array_equal(one["index"], want["index"][0, :c]) and np.array_equal(bits(one["prob"]), bits(want["prob"][0, :c]))


def test_what_the_rules_do(tmp_path_factory):
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64)
    p.rules_on_device = True
    ci, cc = catalogue()
    p.set_catalogue(ci, cc)
    rng = np.random.default_rng(183)
    hi, hc = histories(rng, 2, ["full", "hole"])
    free = p.recommend(hi, hc, 150)
    assert free["count"].tolist() == [150, 150]
    # m = 1: at most one entry per category -- 19 categories in this catalogue -- while the unconstrained request fills k
    one = p.recommend(hi, hc, 150, max_per_category=1)
    assert p.recommend_path == "device"
    for u in range(2):
        c = int(one["count"][u])
        cats = cc[one["index"][u, :c]]
        assert c <= 19 and len(set(cats.tolist())) == c and c < 150
        assert np.isnan(one["prob"][u, c:]).all() and (one["item"][u, c:] == -1).all() and (one["index"][u, c:] == -1).all()
        assert one["index"][u, 0] == free["index"][u, 0]
    three = p.recommend(hi, hc, 150, max_per_category=3)
    assert all(np.bincount(cc[three["index"][u, :int(three["count"][u])]]).max() == 3 for u in range(2))
    assert (three["count"] <= 57).all() and (three["count"] > one["count"]).all()
    # a deny list of the unconstrained top-3's categories removes exactly the entries of those categories
    top_cats = cc[free["index"][:, :3]]
    got = p.recommend(hi, hc, 150, exclude_categories=top_cats)
    for u in range(2):
        keep = ~np.isin(cc[free["index"][u]], top_cats[u])
        c = int(keep.sum())
        assert c < 150 and np.array_equal(got["index"][u, :c], free["index"][u][keep])
        assert np.array_equal(bits(got["prob"][u, :c]), bits(free["prob"][u][keep]))
        assert not np.isin(cc[got["index"][u, :int(got["count"][u])]], top_cats[u]).any()
    # an allow list of those categories alone: their entries, nothing else; an empty one: nothing
    got = p.recommend(hi, hc, 150, categories=top_cats)
    for u in range(2):
        c = int(got["count"][u])
        assert 0 < c < 150 and np.isin(cc[got["index"][u, :c]], top_cats[u]).all()
    none = p.recommend(hi, hc, 10, categories=np.zeros((2, 0), np.int64))
    assert p.recommend_path == "device" and none["count"].tolist() == [0, 0] and (none["index"] == -1).all()
    one_user = p.recommend(hi[0], hc[0], 10, categories=np.int64([]), max_per_category=2)
    assert one_user["count"] == 0 and one_user["prob"].shape == (0,)


def test_a_duplicated_item_counts_twice(tmp_path_factory):
    """The best item also at position 200 (chunk 3 of 64): equal scores go by position and both copies count toward the cap."""
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64)
    p.rules_on_device = True
    ci, cc = catalogue()
    p.set_catalogue(ci, cc)
    hi, hc = histories(np.random.default_rng(187), 1, ["full"])
    best = int(p.recommend(hi, hc, 1, exclude_seen=False)["index"][0, 0])
    at = 200 if best != 200 else 201
    ci[at], cc[at] = ci[best], cc[best]
    p.set_catalogue(ci, cc)
    prob = probabilities(p, hi, hc)
    lo, hi_pos = sorted((best, at))
    got = p.recommend(hi, hc, 30, exclude_seen=False, max_per_category=2)
    same(got, definition(p, prob, hi, 30, False, max_per_category=2))
    assert got["index"][0, :2].tolist() == [lo, hi_pos] and bits(got["prob"])[0, 0] == bits(got["prob"])[0, 1]
    assert (cc[got["index"][0, :int(got["count"][0])]] == cc[best]).sum() == 2        # the two copies are the category's two
    got = p.recommend(hi, hc, 30, exclude_seen=False, max_per_category=1)
    same(got, definition(p, prob, hi, 30, False, max_per_category=1))
    assert got["index"][0, 0] == lo and hi_pos not in got["index"][0].tolist()


def test_graph_replay_with_new_histories_and_a_new_bitmap(tmp_path_factory):
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    eager = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=False)
    graph = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=True)
    ci, cc = catalogue(150)
    rng = np.random.default_rng(189)
    for p in (eager, graph):
        p.rules_on_device = True
        p.set_catalogue(ci, cc)
    a, b = histories(rng, 2, ["full", "hole"]), histories(rng, 2, ["hole", "full"])
    la, lb = category_lists(rng, 2)[0], category_lists(rng, 2)[0]
    want_a = eager.recommend(*a, 40, categories=la, max_per_category=2)
    same(want_a, definition(eager, probabilities(eager, *a), a[0], 40, categories=la, max_per_category=2))
    for _ in range(3):                                               # eager, capture, replay
        same(graph.recommend(*a, 40, categories=la, max_per_category=2), want_a)
    assert "graph" in graph._graphs[("recommend", 2, 40, 32, True, 2)]
    want_b = eager.recommend(*b, 40, categories=lb, max_per_category=2)
    got_b = graph.recommend(*b, 40, categories=lb, max_per_category=2)       # a replay: another history, another bitmap
    same(got_b, want_b)
    assert not np.array_equal(got_b["index"], want_a["index"])
    same(graph.recommend(*a, 40, categories=lb, max_per_category=2), eager.recommend(*a, 40, categories=lb, max_per_category=2))
    same(graph.recommend(*a, 40, categories=la, max_per_category=2), want_a)
    # the cap alone is another graph (no bitmap), and another m another one
    for m in (2, 3):
        for _ in range(3):
            same(graph.recommend(*a, 40, max_per_category=m), eager.recommend(*a, 40, max_per_category=m))
        assert "graph" in graph._graphs[("recommend", 2, 40, 32, False, m)]
    # a new catalogue drops the graphs of rule requests too
    graph.set_catalogue(ci[::-1].copy(), cc[::-1].copy())
    assert not [k for k in graph._graphs if k[0] == "recommend"]
    eager.set_catalogue(ci[::-1].copy(), cc[::-1].copy())
    for _ in range(3):
        same(graph.recommend(*a, 40, categories=la, max_per_category=2), eager.recommend(*a, 40, categories=la, max_per_category=2))


def test_launch_count_plain_requests_and_buffers(tmp_path_factory):
    from recsys_amd import _lib, serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    L = _lib.lib()
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=False)
    p.rules_on_device = True
    rng = np.random.default_rng(191)
    hi, hc = histories(rng, 2, ["hole", "full"])
    only, deny = category_lists(rng, 2)
    for N, chunks in ((37, 1), (130, 3), (299, 5)):
        p.set_catalogue(*catalogue(N))
        before = p.recommend(hi, hc, 10)                             # the plain request, before any rule request
        assert p.recommend_path == "device"
        n0 = L.rsx_dbg_launch_count()
        p.recommend(hi, hc, 10)
        plain = L.rsx_dbg_launch_count() - n0
        assert plain == 2 * chunks
        for rules in ({"max_per_category": 2}, {"categories": only}, {"exclude_categories": deny, "max_per_category": 1}):
            n0 = L.rsx_dbg_launch_count()
            p.recommend(hi, hc, 10, **rules)
            assert L.rsx_dbg_launch_count() - n0 == plain and p.recommend_path == "device", (N, rules)
        same(p.recommend(hi, hc, 10), before)                        # ... and after: the same bits, the same path
        assert p.recommend_path == "device" and p.recommend_path_for(10) == "device"
    r = p._rank
    held = [*r["hist"], *r["cand"], r["prob"], r["rec"]["buf"], r["rec"]["excl"], r["rec"]["allow"], *p._cat["dev"]]
    assert p.recommend_buffer_bytes(2, 10, rules=True) == sum(t.numel() * t.element_size() for t in held)
    assert p.recommend_buffer_bytes(2, 10, rules=True) == p.recommend_buffer_bytes(2, 10) + 4 * 2 * ((N_CATE + 31) // 32)


def test_path_selection(tmp_path_factory):
    """rules_on_device = False, a cap above 16 and 257 exclusion ids take the host path: the same answer."""
    from recsys_amd import _lib, serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64)
    p.rules_on_device = True
    p.set_catalogue(*catalogue())
    rng = np.random.default_rng(193)
    hi, hc = histories(rng, 2, ["hole", "full"])
    prob = probabilities(p, hi, hc)
    only, deny = category_lists(rng, 2)
    assert [p.recommend_path_for(10, m) for m in (1, 16, 17)] == ["device", "device", "host"]
    assert p.recommend_path_for(10, rules=True) == "device" and p.recommend_path_for(1025, 2) == "host"
    assert p.recommend_path_for(10) == "device" and p.recommend_path_for(2000) == "host"
    rules = {"categories": only, "exclude_categories": deny, "max_per_category": 2}
    dev = p.recommend(hi, hc, 20, **rules)
    assert p.recommend_path == "device"
    same(dev, definition(p, prob, hi, 20, **rules))
    p.rules_on_device = False                                        # the switch
    assert p.recommend_path_for(10, 2) == "host" and p.recommend_path_for(10, rules=True) == "host"
    assert p.recommend_path_for(10) == "device"
    host = p.recommend(hi, hc, 20, **rules)
    assert p.recommend_path == "host"
    same(host, dev)
    one = p.recommend(hi[0], hc[0], 20, categories=only[0], max_per_category=2)
    assert p.recommend_path == "host" and isinstance(one["count"], int)
    plain = p.recommend(hi, hc, 20)
    assert p.recommend_path == "device"                              # a request without a rule is not the switch's business
    p.rules_on_device = True
    big = p.recommend(hi, hc, 20, max_per_category=17)               # a cap above the device's
    assert p.recommend_path == "host"
    same(big, definition(p, prob, hi, 20, max_per_category=17))
    same(big, plain)                                                 # (19 categories over 299 entries: 17 binds nowhere in 20)
    many = np.tile(np.arange(1000, 1257), (2, 1))                    # 257 distinct exclusion ids
    got = p.recommend(hi, hc, 20, exclude=many, **rules)
    assert p.recommend_path == "host"
    same(got, dev)
    with pytest.raises(_lib.RsxError, match=r"categories holds ids outside \[0, %d\)" % N_CATE):
        p.recommend(hi, hc, 5, categories=np.int64([[1], [N_CATE]]))
    with pytest.raises(_lib.RsxError, match="max_per_category"):
        p.recommend(hi, hc, 5, max_per_category=0)
