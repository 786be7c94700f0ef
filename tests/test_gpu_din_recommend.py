"""`Predictor.set_catalogue` / `Predictor.recommend` on the GPU: the device request (rsx_predict_din_rank_shared over the
resident catalogue and rsx_topk_rows_excl, one graph per request shape) against serving.recommend_host over the probabilities
`rank_candidates` gives for the same catalogue -- bit for bit (uint32 views of `prob`, equality of the integers) -- over
request shapes, chunked catalogues, the filter, short and empty results, ties across chunk borders, graph replay, a replaced
catalogue, the launch count, the host path and the refusals."""
import numpy as np
import pytest

from tests.test_gpu_din_rank import N_CATE, N_ITEM, bits, din_bundle, make_request

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def catalogue(n=N_ITEM - 1):
    """Items 1 .. n, each with a fixed category."""
    items = np.arange(1, n + 1, dtype=np.int64)
    return items, (items * 7) % (N_CATE - 1) + 1


def same(got, want):
    assert sorted(got) == ["count", "index", "item", "prob"]
    assert got["prob"].dtype == np.float32 and got["item"].dtype == np.int32 and got["index"].dtype == np.int32
    assert got["prob"].shape == want["prob"].shape, (got["prob"].shape, want["prob"].shape)
    assert np.array_equal(np.asarray(got["count"]), np.asarray(want["count"])), (got["count"], want["count"])
    assert np.array_equal(got["index"], want["index"]) and np.array_equal(got["item"], want["item"])
    assert np.array_equal(bits(got["prob"]), bits(want["prob"]))


def histories(rng, U, special, Pn=30):
    hi, hc, _, _ = make_request(rng, U, 1, Pn, special)
    return hi, hc


def definition(p, hi, hc, k, exclude_seen=True, exclude=None):
    """recommend_host over rank_candidates(history, the whole catalogue)."""
    from recsys_amd import serving
    ci, cc = p._cat["host"]
    U = hi.shape[0]
    prob = p.rank_candidates(hi, hc, np.tile(ci, (U, 1)), np.tile(cc, (U, 1)))["prob"]
    return serving.recommend_host(prob, ci, hi, exclude, k, exclude_seen), prob


@pytest.mark.parametrize("K", [16, 32])
@pytest.mark.parametrize("max_c", [64, 1024])
def test_recommend_equals_its_definition(tmp_path_factory, K, max_c):
    """max_candidates 64: five chunks, the last one short (299 = 4 x 64 + 43); 1024: one chunk."""
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, K, 30)
    p = serving.Predictor.load(d, max_batch_size=256, max_candidates=max_c)
    assert p.catalogue_size is None and p.recommend_path is None
    ci, cc = catalogue()
    p.set_catalogue(ci, cc)
    assert p.catalogue_size == 299
    rng = np.random.default_rng(81 + K + max_c)
    for U in (1, 3):
        hi, hc = histories(rng, U, ["hole", "empty", "full"][:U])
        for k in (1, 10, 150, 400):
            for seen in (True, False):
                want, _ = definition(p, hi, hc, k, seen)
                got = p.recommend(hi, hc, k, exclude_seen=seen)
                assert p.recommend_path == "device" and p.recommend_path_for(k) == "device"
                same(got, want)
                assert got["prob"].shape == (U, min(k, 299))
                ok = got["index"] >= 0
                assert np.array_equal(got["item"][ok], ci[got["index"][ok]])
                if U == 1:                                           # the one-user form: 1-D in, arrays cut to count
                    one = p.recommend(hi[0], hc[0], k, exclude_seen=seen)
                    c = int(want["count"][0])
                    assert isinstance(one["count"], int) and one["count"] == c and one["item"].shape == (c,)
                    assert np.array_equal(one["index"], want["index"][0, :c]) and np.array_equal(bits(one["prob"]), bits(want["prob"][0, :c]))


def test_the_filter_bites(tmp_path_factory):
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64)
    p.set_catalogue(*catalogue())
    rng = np.random.default_rng(83)
    hi, hc = histories(rng, 2, ["full", "hole"])
    free = p.recommend(hi, hc, 13, exclude_seen=False)
    top3 = free["item"][:, :3]
    got = p.recommend(hi, hc, 10, exclude_seen=False, exclude=top3)
    assert not np.isin(got["item"][0], top3[0]).any() and not np.isin(got["item"][1], top3[1]).any()
    assert np.array_equal(got["item"], free["item"][:, 3:]) and np.array_equal(got["index"], free["index"][:, 3:])
    assert np.array_equal(bits(got["prob"]), bits(free["prob"][:, 3:]))
    same(got, definition(p, hi, hc, 10, False, top3)[0])
    # exclude_seen: no returned item is in the history -- and the unfiltered answer did hold history items
    hi, hc = histories(rng, 1, ["full"])
    unfiltered = p.recommend(hi, hc, 150, exclude_seen=False)
    assert np.isin(unfiltered["item"][0], hi[0]).any()
    got = p.recommend(hi, hc, 150)
    assert int(got["count"][0]) == 150 and not np.isin(got["item"][0], hi[0]).any()
    same(got, definition(p, hi, hc, 150)[0])
    # both lists together, ids <= 0 in `exclude` are padding
    extra = np.int64([[int(got["item"][0, 0]), 0, -5, int(got["item"][0, 2])]])
    both = p.recommend(hi, hc, 20, exclude=extra)
    same(both, definition(p, hi, hc, 20, True, extra)[0])
    assert both["item"][0, 0] == got["item"][0, 1] and both["item"][0, 1] == got["item"][0, 3]


def test_short_and_empty_results(tmp_path_factory):
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64)
    ci, cc = catalogue(37)
    p.set_catalogue(ci, cc)
    rng = np.random.default_rng(85)
    hi = rng.permutation(ci)[None, :30].copy()                       # 30 of the 37 items seen
    hc = (hi * 7) % (N_CATE - 1) + 1
    got = p.recommend(hi, hc, 10)
    assert p.recommend_path == "device" and got["count"].tolist() == [7] and got["prob"].shape == (1, 10)
    assert np.isnan(got["prob"][0, 7:]).all() and not np.isnan(got["prob"][0, :7]).any()
    assert (got["item"][0, 7:] == -1).all() and (got["index"][0, 7:] == -1).all()
    assert sorted(got["item"][0, :7].tolist()) == sorted(set(ci.tolist()) - set(hi[0].tolist()))
    same(got, definition(p, hi, hc, 10)[0])
    one = p.recommend(hi[0], hc[0], 10)
    assert one["count"] == 7 and one["prob"].shape == (7,) and np.array_equal(one["item"], got["item"][0, :7])
    none = p.recommend(hi, hc, 10, exclude=ci[None, :])              # everything excluded
    assert none["count"].tolist() == [0] and np.isnan(none["prob"]).all() and (none["item"] == -1).all() and (none["index"] == -1).all()
    assert p.recommend_path == "device"
    one = p.recommend(hi[0], hc[0], 10, exclude=ci)
    assert one["count"] == 0 and one["prob"].shape == (0,)
    # two users, one of them with an all-padding history: it excludes nothing
    h2, c2 = np.concatenate([hi, np.zeros_like(hi)]), np.concatenate([hc, np.zeros_like(hc)])
    got = p.recommend(h2, c2, 50)
    assert got["count"].tolist() == [7, 37] and got["prob"].shape == (2, 37)
    same(got, definition(p, h2, c2, 50)[0])


def test_ties_across_chunk_borders(tmp_path_factory):
    """The best item at catalogue positions 3, 63, 64, 130, 199 (chunks 0, 0, 1, 2, 3 of 64): the copies share their bits and
    come in position order; excluding the item removes all of them."""
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64)
    ci, cc = catalogue(200)
    p.set_catalogue(ci, cc)
    hi, hc = histories(np.random.default_rng(87), 1, ["full"])
    first = p.recommend(hi, hc, 1, exclude_seen=False)
    best, at = int(first["index"][0, 0]), [3, 63, 64, 130, 199]
    ci[at], cc[at] = ci[best], cc[best]
    p.set_catalogue(ci, cc)
    copies = sorted(set(at) | {best})
    got = p.recommend(hi, hc, 20, exclude_seen=False)
    want, prob = definition(p, hi, hc, 20, False)
    same(got, want)
    assert got["index"][0, :len(copies)].tolist() == copies and len(set(bits(got["prob"])[0, :len(copies)].tolist())) == 1
    assert (got["item"][0, :len(copies)] == ci[best]).all()
    few = p.recommend(hi, hc, 3, exclude_seen=False)                 # the k-th place inside the tie group
    assert few["index"][0].tolist() == copies[:3]
    gone = p.recommend(hi, hc, 20, exclude_seen=False, exclude=np.int64([[ci[best]]]))
    assert not np.isin(gone["index"][0], copies).any() and int(gone["count"][0]) == 20
    same(gone, definition(p, hi, hc, 20, False, np.int64([[ci[best]]]))[0])


def test_graphs_a_new_history_and_a_new_catalogue(tmp_path_factory):
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    eager = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=False)
    graph = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=True)
    ci, cc = catalogue(150)
    eager.set_catalogue(ci, cc)
    graph.set_catalogue(ci, cc)
    rng = np.random.default_rng(89)
    a, b = histories(rng, 2, ["hole", "full"]), histories(rng, 2, ["full", "hole"])
    want = eager.recommend(*a, 40)
    same(want, definition(eager, *a, 40)[0])
    for _ in range(3):                                               # eager, capture, replay
        same(graph.recommend(*a, 40), want)
    assert "graph" in graph._graphs[("recommend", 2, 40, 32)]
    want_b = eager.recommend(*b, 40)
    got_b = graph.recommend(*b, 40)                                  # a replay over another history: its own answer
    same(got_b, want_b)
    assert not np.array_equal(got_b["index"], want["index"])
    same(graph.recommend(*a, 40), want)
    # a permuted catalogue: the old graphs go, the indices follow the permutation, the items and probabilities stay
    perm = rng.permutation(150)
    graph.set_catalogue(ci[perm], cc[perm])
    assert not [k for k in graph._graphs if k[0] == "recommend"]
    for _ in range(3):
        got = graph.recommend(*a, 40)
        assert np.array_equal(got["item"], want["item"]) and np.array_equal(bits(got["prob"]), bits(want["prob"]))
        assert np.array_equal(perm[got["index"]], want["index"]) and np.array_equal(got["count"], want["count"])
    assert "graph" in graph._graphs[("recommend", 2, 40, 32)]
    # rank_candidates, with and without top_k, answers as before beside it
    cand = np.tile(ci, (2, 1)), np.tile(cc, (2, 1))
    for _ in range(3):
        pe, pg = eager.rank_candidates(*a, *cand), graph.rank_candidates(*a, *cand)
        assert np.array_equal(bits(pe["prob"]), bits(pg["prob"]))
        te, tg = eager.rank_candidates(*a, *cand, top_k=9), graph.rank_candidates(*a, *cand, top_k=9)
        assert np.array_equal(te["index"], tg["index"]) and np.array_equal(bits(te["prob"]), bits(tg["prob"]))
        same(graph.recommend(*a, 40), got)
    # with nothing excluded, recommend is rank_candidates(top_k) plus the id mapping
    free = eager.recommend(*a, 9, exclude_seen=False)
    assert np.array_equal(free["index"], te["index"]) and np.array_equal(bits(free["prob"]), bits(te["prob"]))
    assert np.array_equal(free["item"], ci[te["index"]]) and free["count"].tolist() == [9, 9]


def test_launch_count_paths_and_buffers(tmp_path_factory):
    from recsys_amd import _lib, serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    L = _lib.lib()
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=False)
    rng = np.random.default_rng(91)
    hi, hc = histories(rng, 2, ["hole", "full"])
    for N, chunks in ((37, 1), (64, 1), (130, 3), (299, 5)):         # eagerly, a request is 2 x chunks library launches
        p.set_catalogue(*catalogue(N))
        p.recommend(hi, hc, 10)
        n0 = L.rsx_dbg_launch_count()
        p.recommend(hi, hc, 10)
        assert L.rsx_dbg_launch_count() - n0 == 2 * chunks, N
        assert p.recommend_path == "device"
    r = p._rank
    held = [*r["hist"], *r["cand"], r["prob"], r["rec"]["buf"], r["rec"]["excl"], *p._cat["dev"]]
    assert p.recommend_buffer_bytes(2, 10) == sum(t.numel() * t.element_size() for t in held)
    assert p.recommend_buffer_bytes(2, 10) == p.rank_buffer_bytes(2) + 8 * 299 + 4 * (2 * 2 * 10 + 2 * 2) + 4 * 2 * 256
    assert p.recommend_buffer_bytes(1, 2000) == p.rank_buffer_bytes(1) + 8 * 299
    # the host path: k above 1024 ...
    assert [p.recommend_path_for(k) for k in (1, 1024, 1025, 2000)] == ["device", "device", "host", "host"]
    dev_all = p.recommend(hi, hc, 1024)
    assert p.recommend_path == "device"
    host_all = p.recommend(hi, hc, 2000)                             # both are cut to the catalogue's 299: a k both can take
    assert p.recommend_path == "host"
    same(host_all, dev_all)
    same(host_all, definition(p, hi, hc, 2000)[0])
    # ... or more than 256 distinct positive exclusion ids for a user; 300 ids of which 200 are distinct still fit
    many = np.tile(np.arange(1, 261, dtype=np.int64), (2, 1))
    got = p.recommend(hi, hc, 10, exclude_seen=False, exclude=many)
    assert p.recommend_path == "host" and (got["item"] > 260).all()
    same(got, definition(p, hi, hc, 10, False, many)[0])
    dup = np.tile(np.concatenate([np.arange(1, 201), np.arange(1, 101)]).astype(np.int64), (2, 1))
    got = p.recommend(hi, hc, 10, exclude_seen=False, exclude=dup)
    assert p.recommend_path == "device" and (got["item"] > 200).all()
    same(got, definition(p, hi, hc, 10, False, dup)[0])
    assert p.recommend_path_for(5) == "device"
    d8, _ = din_bundle(tmp_path_factory, 8, 30)                      # outside the rank kernel's envelope: the host path
    p8 = serving.Predictor.load(d8, max_batch_size=64)
    p8.set_catalogue(*catalogue(37))
    assert p8.recommend_path_for(5) == "host"
    got = p8.recommend(hi, hc, 5)
    assert p8.recommend_path == "host"
    same(got, definition(p8, hi, hc, 5)[0])


def test_refusals(tmp_path_factory):
    from recsys_amd import _lib, serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64)
    hi, hc = histories(np.random.default_rng(93), 2, ["hole", "full"])
    L = _lib.lib()
    n0 = L.rsx_dbg_launch_count()
    with pytest.raises(_lib.RsxError, match="no catalogue set"):
        p.recommend(hi, hc, 5)
    with pytest.raises(_lib.RsxError, match="ids outside"):
        p.set_catalogue(np.int64([1, N_ITEM]), np.int64([1, 1]))
    assert p.catalogue_size is None
    p.set_catalogue(*catalogue(50))
    for bad in (0, -3, 2.5, True):
        with pytest.raises(_lib.RsxError, match="top_k must be an integer >= 1"):
            p.recommend(hi, hc, bad)
    for ex in (np.zeros((3, 4), np.int64), np.zeros(4, np.int64), np.zeros((2, 2, 2), np.int64)):
        with pytest.raises(_lib.RsxError, match="exclude .* does not match the histories"):
            p.recommend(hi, hc, 5, exclude=ex)
    with pytest.raises(_lib.RsxError, match="exclude .* does not match the histories"):
        p.recommend(hi[0], hc[0], 5, exclude=np.zeros((1, 4), np.int64))
    with pytest.raises(_lib.RsxError, match="does not fit this bundle's hist_len"):
        p.recommend(np.zeros((2, 31), np.int64), np.zeros((2, 31), np.int64), 5)
    assert L.rsx_dbg_launch_count() == n0                            # all of it before any device work
    for script in ("fm", "deepfm", "dcn", "xdeepfm"):               # a loaded Criteo Predictor (a bare instance stands in)
        q = object.__new__(serving.Predictor)
        q.script = script
        with pytest.raises(_lib.RsxError, match=r"only din.py bundles .* this bundle is %s.py" % script):
            q.recommend(hi, hc, 5)
        with pytest.raises(_lib.RsxError, match=r"only din.py bundles .* this bundle is %s.py" % script):
            q.set_catalogue(*catalogue(5))
