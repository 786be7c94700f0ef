"""`Predictor.evaluate_recommend` on the GPU: the device request (per block of users one graph: the targets' scores, then
rsx_predict_din_rank_shared and rsx_rank_count_rows over every chunk of the resident catalogue) against
serving.target_ranks_host over the probabilities `rank_candidates` gives for the same catalogue -- ranks by integer equality,
`target_prob` bit for bit, the metrics as `ranking_metrics` of those ranks -- over request shapes, user blocks, chunked
catalogues, the filter, ties across chunk borders, graph replay, the host path, the launch count and the refusals."""
import numpy as np
import pytest

from tests.test_gpu_din_rank import N_CATE, N_ITEM, bits, din_bundle, make_request

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ABSENT = 5000                                                        # an item id no catalogue of these tests holds
KS = (1, 10, 50)
SPECIAL = ["full", "hole", "empty", "full", "hole"]


def catalogue(n=N_ITEM - 1):
    """Items 1 .. n, each with a fixed category."""
    items = np.arange(1, n + 1, dtype=np.int64)
    return items, (items * 7) % (N_CATE - 1) + 1


def histories(rng, U, special=SPECIAL, Pn=30):
    hi, hc, _, _ = make_request(rng, U, 1, Pn, special[:U])
    return hi, hc


def scores(p, hi, hc):
    """rank_candidates(history, the whole catalogue): the probabilities the definition ranks."""
    ci, cc = p._cat["host"]
    U = hi.shape[0]
    return p.rank_candidates(hi, hc, np.tile(ci, (U, 1)), np.tile(cc, (U, 1)))["prob"]


def definition(p, prob, hi, held, ks=KS, exclude_seen=True, exclude=None):
    from recsys_amd import serving
    ci, _ = p._cat["host"]
    rank = serving.target_ranks_host(prob, ci, hi, held, exclude, exclude_seen)
    first = {int(i): int(np.flatnonzero(ci == i)[0]) for i in np.unique(ci)}
    tprob = np.full(rank.shape, np.nan, np.float32)
    for u, t in zip(*np.nonzero(rank >= 0)):
        tprob[u, t] = prob[u, first[int(held[u, t])]]
    return rank, tprob, serving.ranking_metrics(rank, ks)


def same(got, want):
    rank, tprob, metrics = want
    assert got["rank"].dtype == np.int32 and got["target_prob"].dtype == np.float32
    assert got["rank"].shape == rank.shape and np.array_equal(got["rank"], rank), (got["rank"], rank)
    assert np.array_equal(bits(got["target_prob"]), bits(tprob))
    assert np.isnan(got["target_prob"][rank < 0]).all() and not np.isnan(got["target_prob"][rank >= 0]).any()
    assert sorted(got) == sorted(list(metrics) + ["rank", "target_prob"])
    for key, v in metrics.items():
        assert got[key] == v or (np.isnan(got[key]) and np.isnan(v)), (key, got[key], v)


def held_out(p, rng, hi, hc, T, exclude_seen, exclude):
    """[U, T] with, for T >= 7, in every row: the item `recommend` puts first, one at place 70 of its list (past the first
    chunk of 64), an id no catalogue holds, an item of the history (where there is one), a padding slot, and distinct
    catalogue items behind them.  T = 1: row u holds kind u % 5 of that list."""
    U = hi.shape[0]
    top = p.recommend(hi, hc, 100, exclude_seen=exclude_seen, exclude=exclude)["item"]
    ci, _ = p._cat["host"]
    held = np.zeros((U, T), np.int64)
    for u in range(U):
        seen = [int(x) for x in hi[u] if x > 0 and x not in (top[u, 0], top[u, 70])]
        lead = [int(top[u, 0]), int(top[u, 70]), ABSENT, seen[0] if seen else int(top[u, 5]), 0]
        rest = [int(x) for x in rng.permutation(ci) if int(x) not in lead]
        row = (lead + rest)[:T] if T >= 7 else [lead[u % 5]]
        held[u] = row
    return held


def spread(rank, held, hi):
    """Which of the required kinds a request's answer shows."""
    kinds = set()
    if (rank == 0).any():
        kinds.add("first")
    if (rank >= 64).any():
        kinds.add("past the first chunk")
    if (rank[held == ABSENT] == -1).any():
        kinds.add("absent")
    if any(np.isin(held[u][held[u] > 0], hi[u][hi[u] > 0]).any() for u in range(len(held))):
        kinds.add("in the history")
    if (rank == -2).any():
        kinds.add("padding")
    return kinds


ALL_KINDS = {"first", "past the first chunk", "absent", "in the history", "padding"}


@pytest.mark.parametrize("K", [16, 32])
@pytest.mark.parametrize("max_c", [64, 1024])
def test_device_equals_the_definition(tmp_path_factory, K, max_c):
    """max_candidates 64: five chunks, the last one short (299 = 4 x 64 + 43); 1024: one chunk."""
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, K, 30)
    p = serving.Predictor.load(d, max_batch_size=256, max_candidates=max_c)
    assert p.evaluate_recommend_path is None
    p.set_catalogue(*catalogue())
    assert [p.evaluate_recommend_path_for(T) for T in (1, 32, 33)] == ["device", "device", "host"]
    rng = np.random.default_rng(101 + K + max_c)
    seen_kinds = set()
    for U in (1, 3, 5):
        hi, hc = histories(rng, U)
        prob = scores(p, hi, hc)
        extra = rng.integers(-1, N_ITEM, (U, 5)).astype(np.int64)     # an exclude list: hits, padding (0 and -1)
        for T in (1, 7, 32):
            for (seen, excl) in ((True, None), (False, None), (True, extra)):
                held = held_out(p, rng, hi, hc, T, seen, excl)
                want = definition(p, prob, hi, held, KS, seen, excl)
                kinds = spread(want[0], held, hi)
                if T >= 7:
                    assert kinds == ALL_KINDS, (U, T, kinds)
                    if seen:                                         # the history item is excluded: it has no rank
                        assert (want[0][:, 3][np.int64([len(h[h > 0]) for h in hi]) > 0] == -1).all()
                seen_kinds |= kinds
                for block in (2, 16):
                    got = p.evaluate_recommend(hi, hc, held, ks=KS, exclude_seen=seen, exclude=excl, user_block=block)
                    assert p.evaluate_recommend_path == "device"
                    same(got, want)
                if U == 1:                                           # the one-user form: 1-D in, 1-D out
                    one = p.evaluate_recommend(hi[0], hc[0], held[0], ks=KS, exclude_seen=seen, exclude=None if excl is None else excl[0])
                    assert one["rank"].shape == (T,) and np.array_equal(one["rank"], want[0][0])
                    assert np.array_equal(bits(one["target_prob"]), bits(want[1][0])) and one["MRR"] == want[2]["MRR"]
    assert seen_kinds == ALL_KINDS
    per = p.evaluate_recommend(hi, hc, held, ks=(3,), per_user=True)
    assert per["HR@3_user"].shape == (5,) and per["users"] == 5 and per["missing"] == int((per["rank"] == -1).sum())


def test_ties_across_chunk_borders(tmp_path_factory):
    """The best item at catalogue positions 3, 63, 64, 130, 199 (chunks 0, 0, 1, 2, 3 of 64): equal scores meet across chunks.
    The item's target entry is its lowest position, rank 0 -- none of its copies precedes it -- and every copy precedes the
    second-best item."""
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64)
    ci, cc = catalogue(200)
    p.set_catalogue(ci, cc)
    hi, hc = histories(np.random.default_rng(87), 1, ["full"])
    first = p.recommend(hi, hc, 2, exclude_seen=False)
    best, second, at = int(first["index"][0, 0]), int(first["item"][0, 1]), [3, 63, 64, 130, 199]
    assert ci[at].tolist().count(second) == 0 and second != ci[best]
    ci[at], cc[at] = ci[best], cc[best]
    p.set_catalogue(ci, cc)
    copies = sorted(set(at) | {best})
    held = np.int64([[ci[best], second, next(int(x) for x in ci[100:] if x not in (ci[best], second))]])
    for _ in range(3):                                               # eager, capture, replay
        got = p.evaluate_recommend(hi, hc, held, ks=(1, 10), exclude_seen=False)
        assert p.evaluate_recommend_path == "device"
        same(got, definition(p, scores(p, hi, hc), hi, held, (1, 10), False))
        assert got["rank"][0, :2].tolist() == [0, len(copies)]
    assert len(copies) >= 5 and copies[0] <= 3
    gone = p.evaluate_recommend(hi, hc, held, ks=(1,), exclude_seen=False, exclude=np.int64([[ci[best]]]))
    assert gone["rank"][0, :2].tolist() == [-1, 0] and gone["missing"] == 1


def test_replay_new_requests_and_the_host_path(tmp_path_factory):
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    eager = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=False)
    graph = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=True)
    for q in (eager, graph):
        q.set_catalogue(*catalogue(150))
    rng = np.random.default_rng(89)
    a, b = histories(rng, 3, ["hole", "full", "empty"]), histories(rng, 3, ["full", "hole", "full"])
    held_a = held_out(eager, rng, *a, 7, True, None)
    held_b = held_out(eager, rng, *b, 7, True, None)
    want_a = eager.evaluate_recommend(*a, held_a, ks=KS)
    same(want_a, definition(eager, scores(eager, *a), a[0], held_a))
    want = {k: want_a[k] for k in ("rank", "target_prob")}
    for _ in range(3):                                               # eager, capture, replay
        got = graph.evaluate_recommend(*a, held_a, ks=KS)
        assert np.array_equal(got["rank"], want["rank"]) and np.array_equal(bits(got["target_prob"]), bits(want["target_prob"]))
    assert "graph" in graph._graphs[("eval_recommend", 3, 8, 32)]
    got_b = graph.evaluate_recommend(*b, held_b, ks=KS)              # a replay over another request: its own answer
    same(got_b, definition(eager, scores(eager, *b), b[0], held_b))
    assert not np.array_equal(got_b["rank"], want["rank"])
    assert np.array_equal(graph.evaluate_recommend(*a, held_a, ks=KS)["rank"], want["rank"])
    graph.set_catalogue(*catalogue(150))                             # a new catalogue drops the graphs captured over the old one
    assert not [k for k in graph._graphs if k[0] == "eval_recommend"]
    # recommend and rank_candidates answer as before beside it
    r_e, r_g = eager.recommend(*a, 9), graph.recommend(*a, 9)
    assert np.array_equal(r_e["index"], r_g["index"]) and np.array_equal(bits(r_e["prob"]), bits(r_g["prob"]))
    # the host path: T = 33 -- the first 32 targets rank as they do alone on the device ...
    ci, _ = catalogue(150)
    held33 = np.stack([rng.permutation(ci)[:33] for _ in range(3)])
    dev32 = graph.evaluate_recommend(*a, held33[:, :32], ks=KS)
    assert graph.evaluate_recommend_path == "device"
    host33 = graph.evaluate_recommend(*a, held33, ks=KS, user_block=2)
    assert graph.evaluate_recommend_path == "host" and graph.evaluate_recommend_path_for(33) == "host"
    same(host33, definition(eager, scores(eager, *a), a[0], held33))
    assert np.array_equal(host33["rank"][:, :32], dev32["rank"])
    assert np.array_equal(bits(host33["target_prob"][:, :32]), bits(dev32["target_prob"]))
    # ... and 300 distinct exclusion ids for a user (ids 1000 .. 1299 exclude nothing; 1 .. 5 do)
    many = np.tile(np.concatenate([np.arange(1, 6), np.arange(1000, 1295)]).astype(np.int64), (3, 1))
    few = np.tile(np.arange(1, 6, dtype=np.int64), (3, 1))
    host = graph.evaluate_recommend(*a, held_a, ks=KS, exclude=many)
    assert graph.evaluate_recommend_path == "host"
    dev = graph.evaluate_recommend(*a, held_a, ks=KS, exclude=few)
    assert graph.evaluate_recommend_path == "device"
    same(host, definition(eager, scores(eager, *a), a[0], held_a, KS, True, many))
    same(dev, (host["rank"], host["target_prob"], {k: v for k, v in host.items() if k not in ("rank", "target_prob")}))


def test_launch_count(tmp_path_factory):
    from recsys_amd import _lib, serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    L = _lib.lib()
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=False)
    rng = np.random.default_rng(91)
    hi, hc = histories(rng, 5)
    held = np.stack([rng.permutation(np.arange(1, 38))[:7] for _ in range(5)]).astype(np.int64)
    for N, chunks in ((37, 1), (64, 1), (130, 3), (299, 5)):         # eagerly, a block of users is 1 + 2 x chunks library launches
        p.set_catalogue(*catalogue(N))
        p.evaluate_recommend(hi[:2], hc[:2], held[:2])
        n0 = L.rsx_dbg_launch_count()
        p.evaluate_recommend(hi[:2], hc[:2], held[:2])
        assert L.rsx_dbg_launch_count() - n0 == 1 + 2 * chunks, N
        assert p.evaluate_recommend_path == "device"
    n0 = L.rsx_dbg_launch_count()
    p.evaluate_recommend(hi, hc, held, user_block=2)                 # three blocks: 2 + 2 + 1 users
    assert L.rsx_dbg_launch_count() - n0 == 3 * (1 + 2 * 5)


def test_refusals(tmp_path_factory):
    from recsys_amd import _lib, serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64)
    hi, hc = histories(np.random.default_rng(93), 2)
    held = np.int64([[1, 2], [3, 0]])
    L = _lib.lib()
    n0 = L.rsx_dbg_launch_count()
    with pytest.raises(_lib.RsxError, match="no catalogue set"):
        p.evaluate_recommend(hi, hc, held)
    p.set_catalogue(*catalogue(50))
    with pytest.raises(_lib.RsxError, match="twice"):
        p.evaluate_recommend(hi, hc, np.int64([[1, 1], [3, 0]]))
    for bad in (np.int64([1, 2]), np.zeros((3, 2), np.int64), np.zeros((2, 0), np.int64)):
        with pytest.raises(_lib.RsxError, match="held_out .* does not match"):
            p.evaluate_recommend(hi, hc, bad)
    with pytest.raises(_lib.RsxError, match="integers"):
        p.evaluate_recommend(hi, hc, np.float32([[1, 2], [3, 0]]))
    for bad in ((0,), (2.5,), (True,)):
        with pytest.raises(_lib.RsxError, match="ks"):
            p.evaluate_recommend(hi, hc, held, ks=bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(_lib.RsxError, match="user_block"):
            p.evaluate_recommend(hi, hc, held, user_block=bad)
    with pytest.raises(_lib.RsxError, match="exclude .* does not match the histories"):
        p.evaluate_recommend(hi, hc, held, exclude=np.zeros((3, 4), np.int64))
    with pytest.raises(_lib.RsxError, match="does not fit this bundle's hist_len"):
        p.evaluate_recommend(np.zeros((2, 31), np.int64), np.zeros((2, 31), np.int64), held)
    for bad in (0, True, 1.5):
        with pytest.raises(_lib.RsxError, match="T must be an integer"):
            p.evaluate_recommend_path_for(bad)
    assert L.rsx_dbg_launch_count() == n0                            # all of it before any device work
    for script in ("fm", "deepfm", "dcn", "xdeepfm"):               # a loaded Criteo Predictor (a bare instance stands in)
        q = object.__new__(serving.Predictor)
        q.script = script
        with pytest.raises(_lib.RsxError, match=r"only din.py bundles .* this bundle is %s.py" % script):
            q.evaluate_recommend(hi, hc, held)
