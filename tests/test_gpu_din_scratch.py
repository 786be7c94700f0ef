"""The request kinds of a din.py `Predictor` share the rank buffers, the scratch entries beside them and the captured graphs:
every kind still answers its host definition, bit for bit, after ANOTHER kind has regrown the shared buffers, and what a
regrowth or a new catalogue drops is exactly what replays over the replaced memory.  uint32 views of the probabilities,
equality of the integers."""
import numpy as np
import pytest

from tests.test_gpu_din_rank import N_CATE, bits, din_bundle
from tests.test_gpu_din_recommend import catalogue, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KINDS = ("rank", "rank_topk", "recommend", "eval_recommend", "two_stage", "eval_two_stage")
SCRATCH = ("topk", "rec", "ts", "ets", "eval")
N, NBRS, T = 150, 8, 2


def kinds_in(p):
    return sorted({k[0] for k in p._graphs if isinstance(k, tuple) and k[0] in KINDS})


def request(rng, U):
    """Histories of P' = 2 catalogue items and two distinct held-out ids per user (the second may be outside the catalogue)."""
    hi = rng.integers(1, N + 1, (U, 2)).astype(np.int64)
    hc = (hi * 7) % (N_CATE - 1) + 1                                 # `catalogue`'s category of an item
    held = np.stack([rng.choice(N + 40, T, replace=False) + 1 for _ in range(U)]).astype(np.int64)
    return hi, hc, held


def check_all(p, ref, table, req):
    """The seven requests, three times each (eager, capture, replay), against their definitions over `ref`'s probabilities."""
    from recsys_amd import serving
    hi, hc, held = req
    U = hi.shape[0]
    ci, cc = p._cat["host"]
    pos, cnt = table
    cand = np.tile(ci, (U, 1)), np.tile(cc, (U, 1))
    prob = ref.rank_candidates(hi, hc, *cand)["prob"]              # computed once, by a Predictor that runs nothing else
    first = serving.catalogue_first_positions(ci)
    for _ in range(3):
        assert np.array_equal(bits(p.rank_candidates(hi, hc, *cand)["prob"]), bits(prob))
    want = serving.topk_rows_host(prob, 9)
    for _ in range(3):
        got = p.rank_candidates(hi, hc, *cand, top_k=9)
        assert np.array_equal(got["index"], want["index"]) and np.array_equal(bits(got["prob"]), bits(want["prob"]))
    want = serving.recommend_host(prob, ci, hi, None, 10)
    for _ in range(3):
        same(p.recommend(hi, hc, 10), want)
    want = serving.recommend_host(prob, ci, hi, None, 10, cat_cate=cc, max_per_category=2, n_cate=N_CATE)
    for _ in range(3):
        same(p.recommend(hi, hc, 10, max_per_category=2), want)
    want = serving.target_ranks_host(prob, ci, hi, held)
    at = serving._target_positions(first, held)
    want_prob = np.where(want >= 0, np.take_along_axis(prob, np.maximum(at, 0), 1), np.float32(np.nan)).astype(np.float32)
    for _ in range(3):
        got = p.evaluate_recommend(hi, hc, held, ks=(10,))
        assert got["rank"].dtype == np.int32 and np.array_equal(got["rank"], want)
        assert np.array_equal(bits(got["target_prob"]), bits(want_prob))
    want = serving.recommend_two_stage_host(prob, pos, cnt, ci, hi, None, 10)
    for _ in range(3):
        same(p.recommend_two_stage(hi, hc, 10), want)
    want = serving.two_stage_ranks_host(prob, pos, cnt, ci, hi, held)
    for _ in range(3):
        got = p.evaluate_two_stage(hi, hc, held, ks=(10,))
        for key in ("rank", "retrieved", "target_index", "n_candidates"):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
        assert np.array_equal(bits(got["target_prob"]), bits(want["target_prob"]))
    assert (p.topk_path, p.recommend_path, p.evaluate_recommend_path, p.two_stage_path, p.evaluate_two_stage_path) == ("device",) * 5


def test_every_kind_answers_after_another_kind_regrew_the_buffers(tmp_path_factory):
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, 32, 30)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=True)
    ref = serving.Predictor.load(d, max_batch_size=64, max_candidates=64, use_hip_graph=False)
    ci, cc = catalogue(N)                                            # 150 entries: three catalogue chunks of at most 64
    p.set_catalogue(ci, cc)
    p.build_neighbours(NBRS)
    assert p.rank_path == "fused" and p.neighbours_path == "device"
    emb = ref._est.store.embeddings["i_id"].table.detach().cpu().numpy()[:, :32]
    pos, _, cnt = serving.item_neighbours_host(serving.unit_rows_host(emb[ci]), ci, NBRS)
    assert np.array_equal(p._nbr["host"][0], pos) and np.array_equal(p._nbr["host"][2], cnt)
    assert serving.candidate_capacity(N, 2, NBRS) == 64              # ... so both two-stage kinds fit max_candidates
    assert p.topk_path_for(9) == "device" and p.recommend_path_for(10) == "device" and p.recommend_path_for(10, 2) == "device"
    assert p.evaluate_recommend_path_for(T) == "device"
    assert p.two_stage_path_for(10, 2) == "device" and p.evaluate_two_stage_path_for(T, 2) == "device"
    rng = np.random.default_rng(4100)
    one, three, grow = request(rng, 1), request(rng, 3), request(rng, 3)

    check_all(p, ref, (pos, cnt), one)
    assert kinds_in(p) == sorted(KINDS) and p._rank["U"] == 1 and all(name in p._rank for name in SCRATCH)
    assert all("graph" in g for k, g in p._graphs.items() if k[0] in KINDS)

    # ONE request of three users: the rank buffers regrow, every graph and every scratch entry over the old ones goes
    hi, hc, _ = grow
    prob = ref.rank_candidates(hi, hc, np.tile(ci, (3, 1)), np.tile(cc, (3, 1)))["prob"]
    same(p.recommend(hi, hc, 10), serving.recommend_host(prob, ci, hi, None, 10))
    assert [k for k in p._graphs if k[0] in KINDS] == [("recommend", 3, 10, 32)] and "graph" not in p._graphs[("recommend", 3, 10, 32)]
    assert p._n_graphs == len(p._graphs) == 1
    assert p._rank["U"] == 3 and [name for name in SCRATCH if name in p._rank] == ["rec"]

    for req in (one, three, one):
        check_all(p, ref, (pos, cnt), req)
    assert kinds_in(p) == sorted(KINDS) and p._n_graphs == len(p._graphs) <= p.MAX_GRAPHS

    # a permuted catalogue: what replays over the catalogue or the neighbour table goes, the plain ranking graphs stay
    perm = rng.permutation(N)
    p.set_catalogue(ci[perm], cc[perm])
    assert kinds_in(p) == ["rank", "rank_topk"] and p._nbr is None and p.neighbours_path is None
    assert all("graph" in g for g in p._graphs.values()) and p._n_graphs == len(p._graphs)
    hi, hc, _ = three
    for _ in range(2):
        got = p.recommend(hi, hc, 10)
        want = serving.recommend_host(ref.rank_candidates(hi, hc, np.tile(ci[perm], (3, 1)), np.tile(cc[perm], (3, 1)))["prob"],
                                      ci[perm], hi, None, 10)
        same(got, want)
