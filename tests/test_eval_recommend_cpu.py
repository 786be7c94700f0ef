"""serving.target_ranks_host and serving.ranking_metrics -- the definitions behind Predictor.evaluate_recommend -- against
recommend_host's order, hand-computed values and an independent dense formulation; the refusals; the new C ABI entries.
No device: pure numpy.  Ranks are compared by integer equality, metrics to a few ulps of float64."""
import math
import os
import re

import numpy as np
import pytest

from recsys_amd import _lib, serving

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda u: np.asarray(u, np.uint32).view(np.float32)
MISSING, PAD = serving.RANK_MISSING, serving.RANK_PAD


def scores(rng, U, N):
    """Random scores with forced ties (three repeated values), both zeros, +-inf and NaNs of two payloads."""
    a = rng.random((U, N), dtype=np.float32)
    pool = f32([0x3f000000, 0x3f000000, 0x3e000000, 0x3f400000, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001])
    m = rng.random((U, N)) < 0.5
    a[m] = pool[rng.integers(0, len(pool), int(m.sum()))]
    return a


def held_rows(rng, U, T, n_ids):
    """Distinct ids per row out of 1 .. n_ids + 5 (the last five are in no catalogue), with padding (0 and negative)."""
    h = np.stack([rng.permutation(np.arange(1, n_ids + 6))[:T] for _ in range(U)]).astype(np.int64)
    h[rng.random((U, T)) < 0.2] = 0
    h[rng.random((U, T)) < 0.1] = -3
    return h


@pytest.mark.parametrize("seen", [True, False])
@pytest.mark.parametrize("with_excl", [True, False])
def test_rank_is_the_index_in_recommend_host(seen, with_excl):
    """The identity that defines the rank: position p of a ranked target stands at recommend_host(top_k=N)['index'][rank];
    a target without a rank is padding, absent from the catalogue, or excluded."""
    rng = np.random.default_rng(31 + 2 * seen + with_excl)
    kinds = set()
    for (U, N, T) in ((1, 1, 1), (3, 40, 6), (2, 90, 12), (4, 200, 25)):
        n_ids = max(1, N // 2)                                       # duplicates: an id sits at about two positions
        prob = scores(rng, U, N)
        cat = rng.integers(0, n_ids + 1, N).astype(np.int32)          # item 0 is an ordinary entry nobody can hold out
        hist = rng.integers(-1, n_ids + 1, (U, 6))
        hist[:, 2] = 0
        excl = rng.integers(-2, n_ids + 1, (U, 4)) if with_excl else None
        held = held_rows(rng, U, T, n_ids)
        rank = serving.target_ranks_host(prob, cat, hist, held, excl, exclude_seen=seen)
        assert rank.dtype == np.int32 and rank.shape == (U, T)
        full = serving.recommend_host(prob, cat, hist, excl, N, exclude_seen=seen)
        for u in range(U):
            out = set(int(x) for x in (list(hist[u]) if seen else []) + (list(excl[u]) if with_excl else []) if x > 0)
            for t in range(T):
                hid, r = int(held[u, t]), int(rank[u, t])
                if hid <= 0:
                    assert r == PAD
                    kinds.add("pad")
                elif hid not in cat:
                    assert r == MISSING
                    kinds.add("absent")
                elif hid in out:
                    assert r == MISSING
                    kinds.add("excluded")
                else:
                    p = int(np.flatnonzero(cat == hid)[0])           # the lowest position that holds the id
                    assert 0 <= r < int(full["count"][u]) and int(full["index"][u, r]) == p, (u, t, r, p)
                    kinds.add("nan" if np.isnan(prob[u, p]) else "ranked")
                    if np.count_nonzero(cat == hid) > 1:
                        kinds.add("duplicate")
        one = serving.target_ranks_host(prob[0], cat, hist[0], held[0], None if excl is None else excl[0], exclude_seen=seen)
        assert one.shape == (T,) and np.array_equal(one, rank[0])
    want = {"pad", "absent", "ranked", "nan", "duplicate"} | ({"excluded"} if seen or with_excl else set())
    assert kinds == want, kinds


def test_ties_zeros_and_nans_by_hand():
    #                 pos:  0     1     2      3       4     5     6
    prob = np.float32([0.5, 0.0, 0.5, np.nan, -0.0, np.inf, np.nan])
    cat = np.int32([1, 2, 3, 4, 5, 6, 7])
    # order: 5 (inf), 0, 2 (0.5 by position), 1, 4 (zeros by position), 3, 6 (NaNs by position)
    rank = serving.target_ranks_host(prob, cat, np.int64([0]), np.int64([6, 1, 3, 2, 5, 4, 7, 9, 0]), exclude_seen=False)
    assert rank.tolist() == [0, 1, 2, 3, 4, 5, 6, MISSING, PAD]
    # item 1 excluded: everything behind it moves up by one, and item 1 itself has no rank
    rank = serving.target_ranks_host(prob, cat, np.int64([1, 0]), np.int64([6, 1, 3, 7]))
    assert rank.tolist() == [0, MISSING, 1, 5]
    # the target entry is the LOWEST position of an id; its copy at a higher position with the same score is not ahead of it
    cat2 = np.int32([9, 8, 9, 4, 5, 6, 7])
    rank = serving.target_ranks_host(prob, cat2, np.int64([0]), np.int64([9, 8]), exclude_seen=False)
    assert rank.tolist() == [1, 3]


def test_ranking_metrics_by_hand():
    # user 0: one item at rank 0; user 1: one item at rank 3; user 2: two items at ranks 0 and 2, one padding slot
    rank = np.int32([[0, PAD, PAD], [3, PAD, PAD], [2, 0, PAD]])
    m = serving.ranking_metrics(rank, (1, 2, 3, 4), per_user=True)
    assert m["users"] == 3 and m["missing"] == 0
    for k in (1, 2, 3, 4):                                           # rank 0: everything is 1 at every k
        assert m["HR@%d_user" % k][0] == m["Recall@%d_user" % k][0] == m["NDCG@%d_user" % k][0] == 1.0
    assert m["MRR_user"].tolist() == [1.0, 0.25, 1.0]
    for k in (1, 2, 3):                                              # rank k gives 0 at k ...
        assert m["HR@%d_user" % k][1] == m["Recall@%d_user" % k][1] == m["NDCG@%d_user" % k][1] == 0.0
    assert m["HR@4_user"][1] == m["Recall@4_user"][1] == 1.0         # ... and counts at k + 1
    assert m["NDCG@4_user"][1] == pytest.approx(1.0 / math.log2(5.0), rel=1e-15)
    # ranks 0 and 2 at k = 2: one hit of two; DCG 1 over the ideal 1 + 1 / log2 3
    assert m["HR@2_user"][2] == 1.0 and m["Recall@2_user"][2] == 0.5
    assert m["NDCG@2_user"][2] == pytest.approx(1.0 / (1.0 + 1.0 / math.log2(3.0)), rel=1e-15)
    assert m["Recall@1_user"][2] == 1.0 and m["NDCG@1_user"][2] == 1.0     # min(k, n_u) = 1
    assert m["Recall@3_user"][2] == 1.0
    assert m["NDCG@3_user"][2] == pytest.approx((1.0 + 0.5) / (1.0 + 1.0 / math.log2(3.0)), rel=1e-15)
    assert m["MRR"] == pytest.approx((1.0 + 0.25 + 1.0) / 3.0, rel=1e-15)
    assert m["Recall@2"] == pytest.approx((1.0 + 0.0 + 0.5) / 3.0, rel=1e-15)
    assert "HR@2_user" not in serving.ranking_metrics(rank, (2,))
    # a missing slot stays in the denominators; a user of padding only is left out of the means
    m = serving.ranking_metrics(np.int32([[0, MISSING], [PAD, PAD]]), [2], per_user=True)
    assert m["users"] == 1 and m["missing"] == 1
    assert m["Recall@2"] == 0.5 and m["HR@2"] == 1.0 and m["MRR"] == 1.0
    assert m["NDCG@2"] == pytest.approx(1.0 / (1.0 + 1.0 / math.log2(3.0)), rel=1e-15)
    assert np.isnan(m["Recall@2_user"][1]) and np.isnan(m["MRR_user"][1])
    m = serving.ranking_metrics(np.int32([MISSING, MISSING]), [5])   # one user, nothing found
    assert m == {"users": 1, "missing": 2, "HR@5": 0.0, "Recall@5": 0.0, "NDCG@5": 0.0, "MRR": 0.0}
    assert np.isnan(serving.ranking_metrics(np.int32([[PAD]]), [5])["MRR"])


def test_metrics_against_a_dense_formulation():
    """The textbook form: scores with -inf on the excluded entries, an argsort, a binary relevance matrix; tie-free scores,
    a catalogue without duplicates."""
    rng = np.random.default_rng(41)
    U, N, T = 7, 120, 9
    ks = (1, 5, 10, 50, 200)
    cat = rng.permutation(np.arange(1, N + 1)).astype(np.int32)
    prob = rng.permutation(U * N).reshape(U, N).astype(np.float32) / np.float32(U * N)      # all distinct
    hist = rng.integers(0, N + 1, (U, 8))
    held = held_rows(rng, U, T, N)
    held[3] = 0                                                      # a user without held-out items
    rank = serving.target_ranks_host(prob, cat, hist, held)
    got = serving.ranking_metrics(rank, ks, per_user=True)
    dense = np.where(np.stack([np.isin(cat, h[h > 0]) for h in hist]), -np.inf, prob.astype(np.float64))
    order = np.argsort(-dense, axis=1)                               # excluded entries sink to the end
    n_elig = (dense > -np.inf).sum(1)
    rel = np.stack([np.isin(cat, h[h > 0]) for h in held])[np.arange(U)[:, None], order]     # relevance along the ranked list
    rel &= np.arange(N)[None, :] < n_elig[:, None]                   # a held-out item that is excluded is no hit
    n_u = (held > 0).sum(1)
    users = n_u > 0
    disc = 1.0 / np.log2(np.arange(N) + 2.0)
    assert got["users"] == int(users.sum()) == U - 1
    assert got["missing"] == int(n_u.sum() - rel.sum())
    for k in ks:
        hits = rel[:, :k].sum(1)
        hr, rec, nd = np.zeros(U), np.zeros(U), np.zeros(U)
        for u in np.flatnonzero(users):
            hr[u] = float(hits[u] > 0)
            rec[u] = hits[u] / min(k, n_u[u])
            nd[u] = (rel[u, :k] * disc[:k]).sum() / disc[:min(k, n_u[u])].sum()
        for key, v in (("HR@%d" % k, hr), ("Recall@%d" % k, rec), ("NDCG@%d" % k, nd)):
            assert np.allclose(got[key + "_user"][users], v[users], rtol=1e-13, atol=0), key
            assert got[key] == pytest.approx(v[users].mean(), rel=1e-13), key
    first = np.where(rel.any(1), rel.argmax(1), -1)
    mrr = np.where(first >= 0, 1.0 / (1.0 + np.maximum(first, 0)), 0.0)
    assert np.allclose(got["MRR_user"][users], mrr[users], rtol=1e-13, atol=0)
    assert 0.0 < got["MRR"] < 1.0 and got["Recall@200"] > got["Recall@5"]


def test_refusals():
    prob, cat, hist = np.zeros((2, 5), np.float32), np.arange(1, 6), np.zeros((2, 3), np.int64)
    with pytest.raises(_lib.RsxError, match="twice"):
        serving.target_ranks_host(prob, cat, hist, np.int64([[1, 2, 1], [1, 2, 3]]))
    serving.target_ranks_host(prob, cat, hist, np.int64([[0, 0, -1], [-1, -1, 3]]))          # padding may repeat
    with pytest.raises(_lib.RsxError, match="catalogue"):
        serving.target_ranks_host(prob, np.arange(4), hist, np.int64([[1], [2]]))
    with pytest.raises(_lib.RsxError, match="integers"):
        serving.target_ranks_host(prob, cat, hist, np.float32([[1], [2]]))
    for bad in (np.int64([1, 2]), np.int64([[1], [2], [3]]), np.zeros((2, 0), np.int64), np.zeros((2, 1, 1), np.int64)):
        with pytest.raises(_lib.RsxError, match="held_out .* does not match"):
            serving.target_ranks_host(prob, cat, hist, bad)
    with pytest.raises(_lib.RsxError, match="held_out .* does not match"):
        serving.target_ranks_host(prob[0], cat, hist[0], np.int64([[1]]))
    with pytest.raises(_lib.RsxError, match="exclude"):
        serving.target_ranks_host(prob, cat, hist, np.int64([[1], [2]]), exclude=np.zeros((3, 2), np.int64))
    rank = np.int32([[0, 1]])
    for bad in ((0,), (3, -1), (2.5,), (True,), 5):
        with pytest.raises(_lib.RsxError, match="ks"):
            serving.ranking_metrics(rank, bad)
    for bad in (np.float32([[0.0]]), np.int32([[-3]]), np.zeros((1, 1, 1), np.int32), np.zeros((2, 0), np.int32)):
        with pytest.raises(_lib.RsxError, match="rank must be integers"):
            serving.ranking_metrics(bad, (1,))


def test_predictor_refusals_come_before_any_device_work():
    hist = np.zeros((2, 3), np.int64)
    for script in ("fm", "deepfm", "dcn", "xdeepfm"):
        p = object.__new__(serving.Predictor)
        p.script = script
        with pytest.raises(_lib.RsxError, match=r"evaluate_recommend: only din.py bundles .* this bundle is %s.py" % script):
            p.evaluate_recommend(hist, hist, np.int64([[1], [2]]))
        assert p.evaluate_recommend_path_for(5) is None
    p = object.__new__(serving.Predictor)
    p.script, p._cat = "din", None
    with pytest.raises(_lib.RsxError, match="no catalogue set"):
        p.evaluate_recommend(hist, hist, np.int64([[1], [2]]))
    assert [serving.Predictor._target_capacity(T) for T in (1, 2, 8, 9, 32)] == [1, 8, 8, 32, 32]


def test_header_bindings_and_version():
    L = _lib.lib()
    assert L.rsx_version() >= 105
    hdr = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert re.search(r"int rsx_rank_count_rows_supported\(int n, int T, int E\);", hdr)
    proto = re.search(r"int rsx_rank_count_rows\(([^;]*)\);", hdr).group(1)
    assert len(proto.split(",")) == 13 == len(_lib._SIGS["rsx_rank_count_rows"][1])
    assert len(_lib._SIGS["rsx_rank_count_rows_supported"][1]) == 3
    assert {"rsx_rank_count_rows", "rsx_rank_count_rows_supported"} <= set(_lib.exported_symbols())
    assert serving.RANK_MAX_T == 32 and (MISSING, PAD) == (-1, -2)
    # the envelope answers without a device
    assert L.rsx_rank_count_rows_supported(1, 1, 0) == 1 and L.rsx_rank_count_rows_supported(1 << 20, 32, 256) == 1
    for (n, T, E) in ((0, 1, 0), (1, 0, 0), (1, 33, 0), (1, 1, -1), (1, 1, 257)):
        assert L.rsx_rank_count_rows_supported(n, T, E) == 0, (n, T, E)
