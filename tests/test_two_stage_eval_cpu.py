"""The numpy definitions behind `Predictor.evaluate_two_stage` (serving.two_stage_ranks_host, two_stage_metrics,
narrow_neighbours_host), the argument refusals of the Predictor method, and the RSX_EINVAL / RSX_EUNSUPPORTED answers of
rsx_rank_count_lists before any HIP call.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from recsys_amd import _lib, serving

EINVAL, EUNSUPPORTED = -1, -3
P = C.c_void_p(0x1000)          # "some non-NULL pointer": never read
bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
N, NBR = 40, 9


@pytest.fixture(scope="module")
def L():
    from recsys_amd import build
    build.build(verbose=False)
    return _lib.lib()


def catalogue():
    """40 entries: item id 0 at position 0, items 1 .. 38 behind it, and item 5 a second time at position 39."""
    return np.concatenate([np.arange(N - 1), [5]]).astype(np.int32)


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(41)
    cat = catalogue()
    unit = serving.unit_rows_host(rng.standard_normal((N, 8)))
    pos, _, cnt = serving.item_neighbours_host(unit, cat, NBR)
    return rng, cat, unit, pos, cnt


def tied_scores(rng, U):
    """Four distinct values plus both zeros and NaN: ties dominate."""
    pool = np.float32([0.25, 0.5, 0.75, 0.9, 0.0, -0.0, np.nan])
    return pool[rng.integers(0, len(pool), (U, N))]


def held_out_of_every_kind(rng, cat, cands, excl_ids):
    """One user's list: a retrieved id, an eligible id that was not retrieved, an id outside the catalogue, an excluded id,
    and two paddings -- shuffled."""
    got = np.unique(cat[cands][cat[cands] > 0])
    free = np.setdiff1d(np.setdiff1d(cat[cat > 0], got), excl_ids)
    ex = np.intersect1d(excl_ids, cat[cat > 0])
    assert len(got) and len(free) and len(ex)
    h = np.int64([rng.choice(got), rng.choice(free), 100, rng.choice(ex), 0, -3])
    return h[rng.permutation(len(h))]


@pytest.mark.parametrize("seen", [True, False])
def test_rank_is_the_index_in_the_two_stage_list(world, seen):
    rng, cat, _, pos, cnt = world
    U = 5
    hist = rng.integers(0, 45, (U, 4)).astype(np.int64)                   # ids 39 .. 44 are outside the catalogue, 0 is padding
    hist[:, 0] = rng.integers(1, 39, U)                                  # at least one seed
    exclude = rng.integers(-1, 39, (U, 3)).astype(np.int64)
    exclude[:, 0] = rng.integers(1, 39, U)
    cands = serving.retrieve_candidates_host(pos, cnt, cat, hist, exclude, seen)
    ids = serving._exclusion_ids(hist, exclude, U, seen)
    held = np.stack([held_out_of_every_kind(rng, cat, cands[u], ids[u][ids[u] > 0]) for u in range(U)])
    prob = tied_scores(rng, U)
    out = serving.two_stage_ranks_host(prob, pos, cnt, cat, hist, held, exclude, seen)
    assert sorted(out) == ["n_candidates", "rank", "retrieved", "target_index", "target_prob"]
    assert out["rank"].dtype == np.int32 and out["retrieved"].dtype == np.int8 and out["target_index"].dtype == np.int32
    assert out["target_prob"].dtype == np.float32 and out["n_candidates"].dtype == np.int32
    assert out["rank"].shape == (U, 6) and out["n_candidates"].tolist() == [len(x) for x in cands]
    full = serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, exclude, N, seen)
    for u in range(U):
        assert sorted(out["retrieved"][u].tolist()) == [-2, -2, -1, -1, 0, 1]                 # every code, every user
        listed = full["index"][u, :full["count"][u]].tolist()
        for t in range(6):
            h, g, r, ix = held[u, t], out["retrieved"][u, t], out["rank"][u, t], out["target_index"][u, t]
            if g == 1:
                assert listed[r] == ix and cat[ix] == h
                assert ix == min(p for p in cands[u] if cat[p] == h)                         # the lowest CANDIDATE copy
                assert bits(out["target_prob"][u, t]) == bits(prob[u, ix])
                continue
            assert ix == -1 and np.isnan(out["target_prob"][u, t])
            if g == 0:
                assert r == serving.RANK_MISSING and h in cat and h not in ids[u] and h not in cat[cands[u]]
            elif g == -1:
                assert r == serving.RANK_MISSING and (h not in cat or h in ids[u])
            else:
                assert g == -2 and r == serving.RANK_PAD and h <= 0
    # the one-user form drops the leading axis
    one = serving.two_stage_ranks_host(prob[2], pos, cnt, cat, hist[2], held[2], exclude[2], seen)
    assert isinstance(one["n_candidates"], int) and one["n_candidates"] == len(cands[2])
    for key in ("rank", "retrieved", "target_index"):
        assert one[key].shape == (6,) and np.array_equal(one[key], out[key][2])
    assert np.array_equal(bits(one["target_prob"]), bits(out["target_prob"][2]))


def test_every_candidate_ranks_where_the_list_shows_it(world):
    """held_out = every distinct item among a user's candidates: the ranks are a permutation read off the list, NaN scores and
    both zeros included."""
    rng, cat, _, pos, cnt = world
    hist = np.int64([3, 17, 5, 30])
    cand = serving.retrieve_candidates_host(pos, cnt, cat, hist, None, False)[0]
    items = np.unique(cat[cand][cat[cand] > 0])
    assert 5 in items and {5, 39} <= set(cand.tolist())                   # the duplicated item is there twice: a seed's copies
    prob = tied_scores(rng, 1)[0]
    out = serving.two_stage_ranks_host(prob, pos, cnt, cat, hist, items, None, False)
    listed = serving.recommend_two_stage_host(prob, pos, cnt, cat, hist, None, N, False)["index"].tolist()
    assert (out["retrieved"] == 1).all()
    assert [listed[r] for r in out["rank"]] == out["target_index"].tolist()
    assert out["target_index"][items.tolist().index(5)] == 5              # both copies are candidates: the lower one


def test_duplicate_rule_by_hand():
    """Item 5 sits at positions 0 and 2.  The only seed's row names position 2 and not position 0: the target is retrieved, at
    the HIGHER copy's position."""
    cat = np.int32([5, 7, 5, 9, 0, 8])
    pos = np.int32([[-1, -1], [2, 3], [-1, -1], [-1, -1], [-1, -1], [-1, -1]])
    cnt = np.int32([0, 2, 0, 0, 0, 0])
    prob = np.float32([0.9, 0.1, 0.3, 0.3, 0.8, 0.7])
    out = serving.two_stage_ranks_host(prob, pos, cnt, cat, np.int64([7]), np.int64([5, 9, 8]))
    assert out["n_candidates"] == 2
    assert out["retrieved"].tolist() == [1, 1, 0] and out["target_index"].tolist() == [2, 3, -1]
    assert out["rank"].tolist() == [0, 1, -1]                             # 0.3 twice: the lower position first
    assert np.array_equal(bits(out["target_prob"][:2]), bits(prob[[2, 3]])) and np.isnan(out["target_prob"][2])
    # `target_ranks_host` would have named position 0, which the list never shows
    assert serving.recommend_two_stage_host(prob, pos, cnt, cat, np.int64([7]), None, 6)["index"].tolist() == [2, 3]


def test_retrieved_codes_by_hand():
    cat = np.int32([5, 7, 5, 9, 0, 8])
    pos = np.int32([[1, 4], [0, 4], [4, 1], [0, 1], [-1, -1], [2, 3]])
    cnt = np.int32([2, 2, 2, 2, 0, 2])
    prob = np.float32([[0.5, np.nan, 0.9, np.nan, -0.0, 0.0]])
    # seed 8 (position 5) -> {2, 3}; exclude_seen=False adds position 5; `exclude` takes item 9 (position 3) out
    out = serving.two_stage_ranks_host(prob, pos, cnt, cat, np.int64([[8, 0]]), np.int64([[5, 8, 7, 9, 6, 0, -1]]),
                                       np.int64([[9]]), False)
    assert out["n_candidates"].tolist() == [2]
    assert out["retrieved"].tolist() == [[1, 1, 0, -1, -1, -2, -2]]
    assert out["rank"].tolist() == [[0, 1, -1, -1, -1, -2, -2]]
    assert out["target_index"].tolist() == [[2, 5, -1, -1, -1, -1, -1]]
    # a NaN target comes after every number, NaNs by position
    prob = np.float32([[0.5, np.nan, np.nan, np.nan, -0.0, 0.0]])
    out = serving.two_stage_ranks_host(prob, pos, cnt, cat, np.int64([[8, 0]]), np.int64([[5, 8, 9]]), None, False)
    assert out["rank"].tolist() == [[1, 0, 2]] and out["retrieved"].tolist() == [[1, 1, 1]]
    assert np.isnan(out["target_prob"][0, [0, 2]]).all()                  # retrieved NaN targets keep their NaN


def same_number(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_two_stage_metrics_by_hand():
    rank = np.int32([[0, -1, -2], [-1, -1, -2], [-2, -2, -2], [3, 0, -1]])
    retrieved = np.int8([[1, 0, -2], [-1, -1, -2], [-2, -2, -2], [1, 1, 0]])
    n_cand = np.int32([4, 0, 2, 7])
    out = serving.two_stage_metrics(rank, retrieved, n_cand, (1, 10), per_user=True)
    base = serving.ranking_metrics(rank, (1, 10), per_user=True)
    for key, v in base.items():                                           # ranking_metrics, unchanged
        assert np.array_equal(out[key], v, equal_nan=True) if isinstance(v, np.ndarray) else same_number(out[key], v), key
    assert sorted(set(out) - set(base)) == ["CandRecall", "CandRecall_user", "CandRecall_users", "candidates_mean"]
    # user 0: 1 of 2; user 1 has slots but none eligible, user 2 has none: neither counts; user 3: 2 of 3
    assert out["CandRecall_users"] == 2 and out["CandRecall"] == (0.5 + 2.0 / 3.0) / 2
    assert np.array_equal(out["CandRecall_user"], [0.5, np.nan, np.nan, 2.0 / 3.0], equal_nan=True)
    assert out["candidates_mean"] == 3.25 and out["users"] == 3           # (ranking_metrics counts user 1: its slots are misses)
    assert "CandRecall_user" not in serving.two_stage_metrics(rank, retrieved, n_cand, (1,))
    # nobody has an eligible slot
    out = serving.two_stage_metrics(rank[1:3], retrieved[1:3], n_cand[1:3], (5,))
    assert np.isnan(out["CandRecall"]) and out["CandRecall_users"] == 0 and out["candidates_mean"] == 1.0
    # the one-user form
    out = serving.two_stage_metrics(rank[3], retrieved[3], 7, (5,))
    assert out["CandRecall"] == 2.0 / 3.0 and out["candidates_mean"] == 7.0 and out["CandRecall_users"] == 1
    for bad in (retrieved[:, :2], retrieved.astype(np.float32), np.int8([[2, 0, -2]] * 4), np.int8([[-3, 0, -2]] * 4)):
        with pytest.raises(_lib.RsxError):
            serving.two_stage_metrics(rank, bad, n_cand, (1,))
    for bad in (n_cand[:3], n_cand.astype(np.float64), np.int32([1, 2, 3, -1])):
        with pytest.raises(_lib.RsxError):
            serving.two_stage_metrics(rank, retrieved, bad, (1,))


@pytest.mark.parametrize("m", [1, 7, NBR])
def test_narrowed_table_is_the_table_built_with_m(world, m):
    _, cat, unit, pos, cnt = world
    want_pos, _, want_cnt = serving.item_neighbours_host(unit, cat, m)
    got_pos, got_cnt = serving.narrow_neighbours_host(pos, cnt, m)
    assert got_pos.dtype == np.int32 and got_cnt.dtype == np.int32 and got_pos.flags["C_CONTIGUOUS"]
    assert np.array_equal(got_pos, want_pos) and np.array_equal(got_cnt, want_cnt)
    assert cnt[0] == 0 and got_cnt[0] == 0 and got_cnt[1:].min() == m     # item 0's row is empty, every other row is full


def test_narrowing_a_short_table():
    """n >= N - 1: rows shorter than n, and shorter than m."""
    cat = np.int32([5, 7, 5, 9, 0, 8])
    unit = serving.unit_rows_host(np.float32([[2, 0], [5, 0], [0, 3], [0, 0], [3, 4], [-1, 0]]))
    pos, _, cnt = serving.item_neighbours_host(unit, cat, 6)
    for m in (1, 4, 5, 6):
        want_pos, _, want_cnt = serving.item_neighbours_host(unit, cat, m)
        got_pos, got_cnt = serving.narrow_neighbours_host(pos, cnt, m)
        assert np.array_equal(got_pos, want_pos) and np.array_equal(got_cnt, want_cnt)


def test_argument_errors(world):
    rng, cat, _, pos, cnt = world
    prob, hist = tied_scores(rng, 2), np.int64([[3, 4], [5, 6]])
    ok = np.int64([[1, 2], [3, 0]])
    serving.two_stage_ranks_host(prob, pos, cnt, cat, hist, ok)
    for bad_prob in (prob[:, :39], prob[None], prob[0]):                  # wrong N, three axes, one row for two histories
        with pytest.raises(_lib.RsxError):
            serving.two_stage_ranks_host(bad_prob, pos, cnt, cat, hist, ok)
    for bad in (np.int64([[1, 1], [3, 0]]), np.float32([[1, 2], [3, 0]]), ok[0], ok[:, :0], ok[:1]):
        with pytest.raises(_lib.RsxError):
            serving.two_stage_ranks_host(prob, pos, cnt, cat, hist, bad)
    with pytest.raises(_lib.RsxError):
        serving.two_stage_ranks_host(prob, pos[:39], cnt[:39], cat, hist, ok)
    for bad in (0, NBR + 1, -1, True, 2.0, None):
        with pytest.raises(_lib.RsxError, match="n_neighbours"):
            serving.narrow_neighbours_host(pos, cnt, bad)
    with pytest.raises(_lib.RsxError):
        serving.narrow_neighbours_host(pos, cnt[:5], 2)


def _bare(script, **kw):
    p = object.__new__(serving.Predictor)
    p.script, p._cat, p._nbr = script, None, None
    p.manifest = {"params": {"hist_len": 4, "n_item": 10, "n_cate": 3, "embedding_size": 16}}
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_predictor_refusals():
    h = np.int64([1, 2])
    with pytest.raises(_lib.RsxError, match="din.py"):
        _bare("deepfm").evaluate_two_stage(h, h, h)
    with pytest.raises(_lib.RsxError, match="set_catalogue"):
        _bare("din").evaluate_two_stage(h, h, h)
    cat6 = np.int32([5, 7, 5, 9, 0, 8])
    cat = {"host": (cat6, cat6 * 0), "first": serving.catalogue_first_positions(cat6)}
    with pytest.raises(_lib.RsxError, match="build_neighbours"):
        _bare("din", _cat=cat, catalogue_size=6).evaluate_two_stage(h, h, h)
    pos = np.int32([[1, 4], [0, 4], [4, 1], [0, 1], [-1, -1], [2, 3]])
    nbr = {"n": 2, "host": (pos, np.zeros((6, 2), np.float32), np.int32([2, 2, 2, 2, 0, 2]))}
    p = _bare("din", _cat=cat, catalogue_size=6, _nbr=nbr)
    for bad in (0, 3, True, 1.0, -1):
        with pytest.raises(_lib.RsxError, match="n_neighbours"):
            p.evaluate_two_stage(h, h, h, n_neighbours=bad)
        with pytest.raises(_lib.RsxError, match="n_neighbours"):
            p.evaluate_two_stage_path_for(1, n_neighbours=bad)
    for bad in (0, True, 2.5):
        with pytest.raises(_lib.RsxError, match="user_block"):
            p.evaluate_two_stage(h, h, h, user_block=bad)
        with pytest.raises(_lib.RsxError):
            p.evaluate_two_stage_path_for(bad)
    with pytest.raises(_lib.RsxError):
        p.evaluate_two_stage(h, h, h, ks=(0,))
    assert _bare("deepfm").evaluate_two_stage_path_for(3) is None
    assert _bare("din").evaluate_two_stage_path_for(3) == "host"          # no table yet: nothing to run on the device


def test_entry_refuses_before_any_hip_call(L):
    assert L.rsx_rank_count_lists_supported(1, 1) == 1 and L.rsx_rank_count_lists_supported(4096, 32) == 1
    assert L.rsx_rank_count_lists_supported(1 << 30, 8) == 1
    for n, T in ((0, 1), (-1, 1), (64, 0), (64, 33), (64, -1)):
        assert L.rsx_rank_count_lists_supported(n, T) == 0, (n, T)
    # rsx_rank_count_lists(scores, ld, cand_id, cand_pos, n_valid, tgt_id, T, out_count, out_pos, out_score, U, n, stream)
    ok = [P, 64, P, P, P, P, 8, P, P, P, 2, 64, None]
    for at in (0, 2, 3, 4, 5, 7, 8, 9):
        a = list(ok)
        a[at] = None
        assert L.rsx_rank_count_lists(*a) == EINVAL, at
    for at, bad in ((1, 63), (6, 0), (6, -2), (10, 0), (10, -1), (11, 0)):
        a = list(ok)
        a[at] = bad
        assert L.rsx_rank_count_lists(*a) == EINVAL, (at, bad)
    a = list(ok)
    a[6] = 33
    assert L.rsx_rank_count_lists(*a) == EUNSUPPORTED
