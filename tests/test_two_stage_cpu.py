"""The numpy definitions behind the two-stage DIN recommendation (serving.unit_rows_host, rows_dot_host, item_neighbours_host,
retrieve_candidates_host, recommend_two_stage_host), the argument refusals of the Predictor methods, and the RSX_EINVAL /
RSX_EUNSUPPORTED answers of the three device entries before any HIP call.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from recsys_amd import _lib, serving

EINVAL, EUNSUPPORTED = -1, -3
P = C.c_void_p(0x1000)          # "some non-NULL, 16-byte aligned pointer": never read
bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def L():
    from recsys_amd import build
    build.build(verbose=False)
    return _lib.lib()


# A hand-written catalogue of 6 positions in 2 dimensions.
#   pos 0: item 5, direction (1, 0)
#   pos 1: item 7, direction (1, 0)          -- the same direction as pos 0: a tie for whoever looks at both
#   pos 2: item 5, direction (0, 1)          -- a duplicate of item 5
#   pos 3: item 9, the zero row
#   pos 4: item 0, direction (3, 4) / 5      -- the padding id: never a seed, may be a neighbour
#   pos 5: item 8, direction (-1, 0)
CAT = np.int32([5, 7, 5, 9, 0, 8])
EMB = np.float32([[2, 0], [5, 0], [0, 3], [0, 0], [3, 4], [-1, 0]])


def test_unit_rows():
    u = serving.unit_rows_host(EMB)
    assert u.dtype == np.float32 and u.shape == (6, 2)
    assert np.array_equal(bits(u[3]), bits(np.float32([0, 0])))                        # a zero-norm row stays +0.0
    assert np.array_equal(u[0], [1, 0]) and np.array_equal(u[5], [-1, 0])
    assert np.array_equal(bits(u[4]), bits(np.float32([np.float64(3) / 5, np.float64(4) / 5])))
    for bad in (np.nan, np.inf):
        e = EMB.copy()
        e[2, 1] = bad
        with pytest.raises(_lib.RsxError):
            serving.unit_rows_host(e)


@pytest.mark.parametrize("K", [16, 32])
def test_rows_dot_host_against_float64(K):
    rng = np.random.default_rng(5 + K)
    u = serving.unit_rows_host(rng.standard_normal((200, K)))
    q = rng.integers(0, 200, 37)
    got = serving.rows_dot_host(u, q, 11, 150)
    assert got.dtype == np.float32 and got.shape == (37, 150)
    want = u[q].astype(np.float64) @ u[11:161].astype(np.float64).T
    assert np.abs(got - want).max() <= K * 2.0 ** -23
    # the restatement, element by element: one accumulator, ascending d, a rounded product and a rounded sum
    for qi, j in ((0, 0), (36, 149), (5, 77)):
        s = np.float32(0)
        for d in range(K):
            s = np.float32(s + np.float32(u[q[qi], d] * u[11 + j, d]))
        assert bits(got[qi, j]) == bits(s)
    with pytest.raises(_lib.RsxError):
        serving.rows_dot_host(u, q, 100, 101)


def test_item_neighbours_hand_written():
    u = serving.unit_rows_host(EMB)
    pos, sim, count = serving.item_neighbours_host(u, CAT, 3)
    assert pos.dtype == np.int32 and sim.dtype == np.float32 and count.dtype == np.int32
    # pos 0 (item 5): pos 2 is the same item and leaves with pos 0 itself.  Left: 1 (sim 1), 3 (0), 4 (0.6), 5 (-1)
    assert pos[0].tolist() == [1, 4, 3] and count[0] == 3
    assert np.array_equal(bits(sim[0]), bits(np.float32([1, np.float32(np.float64(3) / 5), 0])))
    # pos 1 (item 7): 0 (1), 4 (0.6), then the tie at 0 between pos 2 and pos 3 goes to the lower position
    assert pos[1].tolist() == [0, 4, 2]
    # pos 2 (item 5): 0 is out; 4 (0.8), then 1, 3, 5 tie at 0 (5 gives -0.0, which compares equal): lower positions first
    assert pos[2].tolist() == [4, 1, 3]
    # pos 3, the zero row: every similarity is 0, so the lowest other positions
    assert pos[3].tolist() == [0, 1, 2] and np.array_equal(sim[3], [0, 0, 0])
    # pos 4 has item id 0: an empty row -- but it IS a neighbour of others
    assert count[4] == 0 and pos[4].tolist() == [-1, -1, -1] and np.isnan(sim[4]).all()
    assert pos[5].tolist() == [2, 3, 4]                                                   # 0, 0, -0.6; then -1 twice
    # n >= N - 1: short rows
    pos, sim, count = serving.item_neighbours_host(u, CAT, 6)
    assert count.tolist() == [4, 5, 4, 5, 0, 5]
    assert pos[0].tolist() == [1, 4, 3, 5, -1, -1] and np.isnan(sim[0, 4:]).all() and not np.isnan(sim[0, :4]).any()
    for bad in (0, 65, True, 2.0):
        with pytest.raises(_lib.RsxError):
            serving.item_neighbours_host(u, CAT, bad)


def _table():
    return serving.item_neighbours_host(serving.unit_rows_host(EMB), CAT, 2)


def test_retrieve_candidates_hand_written():
    pos, _, cnt = _table()
    assert pos.tolist() == [[1, 4], [0, 4], [4, 1], [0, 1], [-1, -1], [2, 3]]
    r = lambda h, **kw: [x.tolist() for x in serving.retrieve_candidates_host(pos, cnt, CAT, np.int64(h), **kw)]
    # item 7 (pos 1) -> {0, 4}; item 6 is not in the catalogue, 0 and -3 are padding
    assert r([[7, 6, 0, -3]]) == [[0, 4]]
    # item 5 resolves to its LOWEST position 0 -> {1, 4}; with item 7 -> {0, 1, 4}; seen items leave: 0 (item 5), 1 (item 7)
    assert r([[5, 7]]) == [[4]]
    assert r([[5, 7]], exclude_seen=False) == [[0, 1, 2, 4]]                              # the seeds join, BOTH positions of item 5
    # an exclusion id removes both positions of the duplicated item
    assert r([[8, 7]], exclude_seen=False) == [[0, 1, 2, 3, 4, 5]]
    assert r([[8, 7]], exclude_seen=False, exclude=np.int64([[5, 0]])) == [[1, 3, 4, 5]]
    assert r([[8, 7]], exclude=np.int64([[5, 0]])) == [[3, 4]]
    # an empty history, a history of unknown ids, and U users at once
    assert r([[0, 0]]) == [[]] and r([[6, 299]]) == [[]]
    assert r([[7, 0], [0, 0], [9, 9]]) == [[0, 4], [], [0, 1]]
    one = serving.retrieve_candidates_host(pos, cnt, CAT, np.int64([7, 0]))
    assert len(one) == 1 and one[0].dtype == np.int32 and one[0].tolist() == [0, 4]
    with pytest.raises(_lib.RsxError):
        serving.retrieve_candidates_host(pos[:5], cnt[:5], CAT, np.int64([7]))


def test_recommend_two_stage_host_hand_written():
    pos, _, cnt = _table()
    prob = np.float32([[0.5, 0.9, 0.9, 0.1, 0.7, 0.2], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]])
    hist = np.int64([[8, 7], [0, 0]])
    out = serving.recommend_two_stage_host(prob, pos, cnt, CAT, hist, None, 3, exclude_seen=False)
    assert out["count"].tolist() == [3, 0] and out["prob"].shape == (2, 3)
    assert out["index"][0].tolist() == [1, 2, 4]                                          # 0.9 twice: the lower position first
    assert out["item"][0].tolist() == [7, 5, 0] and np.array_equal(bits(out["prob"][0]), bits(prob[0, [1, 2, 4]]))
    assert out["index"][1].tolist() == [-1, -1, -1] and np.isnan(out["prob"][1]).all() and out["item"][1].tolist() == [-1, -1, -1]
    # the candidates decide, not the scores: position 1 scores best and is seen
    out = serving.recommend_two_stage_host(prob, pos, cnt, CAT, hist, np.int64([[5], [0]]), 10)
    assert out["prob"].shape == (2, 6) and out["count"].tolist() == [2, 0] and out["index"][0, :2].tolist() == [4, 3]
    # the restriction of recommend_host's order to the candidates
    full = serving.recommend_host(prob[0], CAT, hist[0], None, 6, exclude_seen=False)
    cand = serving.retrieve_candidates_host(pos, cnt, CAT, hist[0], exclude_seen=False)[0]
    one = serving.recommend_two_stage_host(prob[0], pos, cnt, CAT, hist[0], None, 6, exclude_seen=False)
    assert one["count"] == 6 and one["index"].tolist() == [i for i in full["index"].tolist() if i in set(cand.tolist())]
    with pytest.raises(_lib.RsxError):
        serving.recommend_two_stage_host(prob[:, :5], pos, cnt, CAT, hist, None, 3)


def test_candidate_capacity():
    assert serving.candidate_capacity(63001, 100, 32) == 3328 and serving.candidate_capacity(300, 100, 32) == 320
    assert serving.candidate_capacity(10, 0, 32) == 64 and serving.candidate_capacity(64, 1, 63) == 64


def _bare(script, **kw):
    p = object.__new__(serving.Predictor)
    p.script, p._cat, p._nbr = script, None, None
    p.manifest = {"params": {"hist_len": 4, "n_item": 10, "n_cate": 3, "embedding_size": 16}}
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_argument_refusals():
    h = np.int64([1, 2])
    for name, args in (("build_neighbours", ()), ("similar_items", (h, 1)), ("retrieve_candidates", (h, h)),
                       ("recommend_two_stage", (h, h, 3))):
        with pytest.raises(_lib.RsxError, match="din.py"):
            getattr(_bare("deepfm"), name)(*args)
        with pytest.raises(_lib.RsxError, match="set_catalogue"):
            getattr(_bare("din"), name)(*args)
    cat = {"host": (CAT, CAT * 0), "first": serving.catalogue_first_positions(CAT)}
    for name, args in (("similar_items", (h, 1)), ("retrieve_candidates", (h, h)), ("recommend_two_stage", (h, h, 3))):
        with pytest.raises(_lib.RsxError, match="build_neighbours"):
            getattr(_bare("din", _cat=cat, catalogue_size=6), name)(*args)
    for bad in (0, 65, -1, 1.5, True, None):
        with pytest.raises(_lib.RsxError, match="n_neighbours"):
            _bare("din", _cat=cat, catalogue_size=6).build_neighbours(bad)
    pos, sim, cnt = _table()
    p = _bare("din", _cat=cat, catalogue_size=6, _nbr={"n": 2, "host": (pos, sim, cnt)})
    with pytest.raises(_lib.RsxError, match="exceeds"):
        p.similar_items(h, 3)
    with pytest.raises(_lib.RsxError):
        p.similar_items(np.float32([1.0]), 1)
    got = p.similar_items(np.int64([5, 6, 0, 8]), 2)                                      # (host tables only: no device needed)
    assert got["index"].tolist() == [[1, 4], [-1, -1], [-1, -1], [2, 3]] and got["count"].tolist() == [2, 0, 0, 2]
    assert got["item"].tolist() == [[7, 0], [-1, -1], [-1, -1], [5, 9]]
    assert np.array_equal(bits(got["sim"][0]), bits(sim[0])) and np.isnan(got["sim"][1:3]).all()
    for bad in (0, True, 2.5):
        with pytest.raises(_lib.RsxError):
            p.recommend_two_stage(h, h, bad)
    assert _bare("deepfm").two_stage_path_for(3) is None


def test_entries_refuse_before_any_hip_call(L):
    assert L.rsx_version() == 107
    # rsx_rows_dot(unit, N, K, q_rows, Q, first, n, scores, ld, stream)
    ok = [P, 100, 32, P, 8, 10, 50, P, 50, None]

    def dot(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.rsx_rows_dot(*a)
    for i in (0, 3, 7):
        assert dot(**{"a%d" % i: None}) == EINVAL
    assert dot(a0=C.c_void_p(0x1004)) == EINVAL                                           # not 16-byte aligned
    for i, v in ((1, 0), (4, 0), (5, -1), (6, 0), (6, 91), (8, 49), (2, 0)):
        assert dot(**{"a%d" % i: v}) == EINVAL, (i, v)
    for K in (8, 24, 64):
        assert dot(a2=K) == EUNSUPPORTED and L.rsx_rows_dot_supported(K) == 0
    assert L.rsx_rows_dot_supported(16) == 1 and L.rsx_rows_dot_supported(32) == 1
    # rsx_topk_rows_counted(scores, ld, n_valid, U, n, k, out_val, out_idx, state, stream)
    assert L.rsx_topk_rows_counted(P, 8, None, 1, 8, 4, P, P, P, None) == EINVAL
    assert L.rsx_topk_rows_counted(None, 8, P, 1, 8, 4, P, P, P, None) == EINVAL
    assert L.rsx_topk_rows_counted(P, 7, P, 1, 8, 4, P, P, P, None) == EINVAL            # ld < n
    assert L.rsx_topk_rows_counted(P, 8, P, 0, 8, 4, P, P, P, None) == EINVAL
    assert L.rsx_topk_rows_counted(P, 8, P, 1, 8, 1025, P, P, P, None) == EUNSUPPORTED
    assert L.rsx_topk_rows_counted(P, 16384, P, 1, 16384, 1, P, P, P, None) == EUNSUPPORTED
    # rsx_din_retrieve_candidates(hist, P, first_pos, n_item, nbr_pos, nbr_count, n_nbr, cat_item, cat_cate, N, excl, E, seeds,
    #                             cand_pos, cand_item, cand_cate, n_cand, cap, U, stream)
    ok = [P, 100, P, 500, P, P, 32, P, P, 400, P, 32, 0, P, P, P, P, 448, 2, None]

    def ret(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.rsx_din_retrieve_candidates(*a)
    for i in (0, 2, 4, 5, 7, 8, 10, 13, 14, 15, 16):
        assert ret(**{"a%d" % i: None}) == EINVAL, i
    for i, v in ((1, 0), (3, 0), (6, 0), (9, 0), (11, -1), (17, 0), (18, 0)):
        assert ret(**{"a%d" % i: v}) == EINVAL, (i, v)
    for i, v in ((9, (1 << 20) + 1), (1, 129), (6, 65), (11, 257)):
        assert ret(**{"a%d" % i: v}) == EUNSUPPORTED, (i, v)
    assert L.rsx_din_retrieve_candidates_supported(1 << 20, 128, 64, 256) == 1
    assert L.rsx_din_retrieve_candidates_supported((1 << 20) + 1, 128, 64, 256) == 0
    assert L.rsx_din_retrieve_candidates_supported(63001, 129, 64, 0) == 0
    assert L.rsx_din_retrieve_candidates_supported(63001, 100, 65, 0) == 0
    assert L.rsx_din_retrieve_candidates_supported(63001, 100, 32, 257) == 0
