"""Offline evaluation of the two-stage DIN list on the GPU: rsx_rank_count_lists (csrc/rank_count_lists.hip) through ctypes
against a numpy restatement by lexsort -- integers by equality, scores by their bits -- and `Predictor.evaluate_two_stage`:
the device path == the host path == `two_stage_ranks_host` over the probabilities `rank_candidates` gives for the whole
catalogue, and its ranks against the list `recommend_two_stage` returns."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_din_rank import bits, make_request
from tests.test_gpu_two_stage import N_CATE, N_ITEM, catalogue, load, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

f32 = lambda u: np.asarray(u, np.uint32).view(np.float32)
# five distinct values (0.5 twice as often), both zeros, both infinities, two NaN patterns: ties dominate
POOL = f32([0x3f000000, 0x3f000000, 0x3e800000, 0x3f400000, 0x3dcccccd, 0xbf000000, 0x00000000, 0x80000000, 0x7f800000, 0xff800000,
            0x7fc00000, 0xffc00001])
SENT_I, SENT_F, GUARD = -77, 0xdeadbeef, 8
NAN_BITS = 0x7fc00000


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def expected(scores, cand_id, cand_pos, n_valid, tgt):
    """numpy: a stable lexsort by (-score, column) of the row's live columns is the list; a target stands where the lowest
    live column with its id stands."""
    U, T = tgt.shape
    count, pos = np.full((U, T), -1, np.int32), np.full((U, T), -1, np.int32)
    score = np.full((U, T), NAN_BITS, np.uint32)
    for u in range(U):
        nv = int(n_valid[u])
        s = scores[u, :nv]
        place = np.empty(nv, np.int64)
        place[np.lexsort((np.arange(nv), -s))] = np.arange(nv)
        for t in range(T):
            cols = np.flatnonzero(cand_id[u, :nv] == tgt[u, t]) if tgt[u, t] > 0 else []
            if len(cols):
                c = cols[0]
                count[u, t], pos[u, t], score[u, t] = place[c], cand_pos[u, c], s[c:c + 1].view(np.uint32)[0]
    return count, pos, score


def lists_case(rng, n, T, rep):
    """U = 3 rows with 0, 1 or n - 1, and n live columns.  Slot kinds rotate with (t, u, rep): the id at column 0, the id at the
    last live column, an id that two live columns hold, an id that only a dead column holds, 0 and -1."""
    U = 3
    n_valid = np.int32([0, 1 if rep % 2 == 0 else n - 1, n])
    scores = POOL[rng.integers(0, len(POOL), (U, n))]
    cand_id = rng.integers(11, 11 + max(2, n // 2), (U, n)).astype(np.int32)
    cand_pos = np.cumsum(rng.integers(1, 4, (U, n)), axis=1).astype(np.int32)              # ascending, with gaps
    tgt = np.zeros((U, T), np.int32)
    twice, dead = np.zeros(U, np.int32), np.int32([7, 8, 9])
    for u in range(U):
        nv = int(n_valid[u])
        if nv >= 2:
            a, b = sorted(rng.choice(nv, 2, replace=False))
            cand_id[u, b] = cand_id[u, a]
            twice[u] = cand_id[u, a]
        if nv < n:                                                       # a dead column: an id no live column holds, the best score
            cand_id[u, nv], scores[u, nv] = dead[u], np.inf
        for t in range(T):
            kind = (t + u + rep) % 6
            if kind == 0 and nv:
                tgt[u, t] = cand_id[u, 0]
            elif kind == 1 and nv:
                tgt[u, t] = cand_id[u, nv - 1]
            elif kind == 2:
                tgt[u, t] = twice[u] if twice[u] else (cand_id[u, 0] if nv else 5)
            elif kind == 3:
                tgt[u, t] = dead[u]
            elif kind == 4:
                tgt[u, t] = 0
            else:
                tgt[u, t] = -1
    return scores, cand_id, cand_pos, n_valid, tgt


def run_lists(scores, cand_id, cand_pos, n_valid, tgt, pad):
    """One call -> (count, pos, score bits), each [U, T], read out of buffers with guard words around [U, T]; rows padded to
    ld = n + pad with +inf, which would precede every target if it were read."""
    from recsys_amd import _lib
    U, n = scores.shape
    T = tgt.shape[1]
    host = np.full((U, n + pad), np.inf, np.float32)
    host[:, :n] = scores
    sc, cid, cp, nv, tg = dev(host, np.float32), dev(cand_id, np.int32), dev(cand_pos, np.int32), dev(n_valid, np.int32), dev(tgt, np.int32)
    outs = [torch.full((U * T + 2 * GUARD,), SENT_I, dtype=torch.int32, device="cuda") for _ in range(2)]
    outs.append(dev(np.full(U * T + 2 * GUARD, SENT_F, np.uint32).view(np.float32), np.float32))
    at = [o.data_ptr() + 4 * GUARD for o in outs]
    _lib.check(_lib.lib().rsx_rank_count_lists(sc.data_ptr(), n + pad, cid.data_ptr(), cp.data_ptr(), nv.data_ptr(), tg.data_ptr(), T,
                                               at[0], at[1], at[2], U, n, torch.cuda.current_stream().cuda_stream), "rsx_rank_count_lists")
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    got[2] = got[2].view(np.uint32)
    for g, sentinel in zip(got, (SENT_I, SENT_I, SENT_F)):
        assert (g[:GUARD] == sentinel).all() and (g[-GUARD:] == sentinel).all()              # the guard words are untouched
    return [g[GUARD:-GUARD].reshape(U, T) for g in got]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1000, 4096])
def test_lists_kernel_against_lexsort(n):
    from recsys_amd import _lib
    rng = np.random.default_rng(5000 + n)
    found = twice_hit = dead_miss = 0
    for T in (1, 8, 9, 32):
        assert _lib.lib().rsx_rank_count_lists_supported(n, T) == 1
        for pad in (0, 5):
            for rep in range(6 if T == 1 else 2):
                args = lists_case(rng, n, T, rep)
                count, pos, score = run_lists(*args, pad=pad)
                w_count, w_pos, w_score = expected(*args)
                where = (n, T, pad, rep)
                # every slot overwritten: a count and a position are >= -1, a score is the column's bits or the one NaN
                assert (count != SENT_I).all() and (pos != SENT_I).all() and (score != SENT_F).all(), where
                assert np.array_equal(count, w_count), (where, count, w_count)
                assert np.array_equal(pos, w_pos), where
                assert np.array_equal(score, w_score), where
                tgt, cand_id, n_valid = args[4], args[1], args[3]
                assert (count[tgt <= 0] == -1).all() and (count[0] == -1).all()          # padding slots; the row without a live column
                found += int((count >= 0).sum())
                for u in range(3):
                    nv = int(n_valid[u])
                    for t in range(T):
                        if tgt[u, t] > 0 and nv < n and tgt[u, t] == cand_id[u, nv]:
                            dead_miss += int(count[u, t] == -1)
                        if tgt[u, t] > 0 and np.count_nonzero(cand_id[u, :nv] == tgt[u, t]) > 1:
                            twice_hit += 1
    assert found and dead_miss                                           # not vacuous: hits, and ids only a dead column holds
    assert twice_hit or n == 1


def test_lists_kernel_by_hand():
    #                 j:  0     1     2      3       4     5      6       7 (dead)
    sc = np.float32([[0.5, 0.0, 0.5, np.nan, -0.0, np.inf, np.nan, 0.9]])
    # order of the live columns: 5 | 0 2 | 1 4 | 3 6
    cid = np.int32([[21, 22, 21, 24, 25, 26, 24, 29]])
    cp = np.int32([[3, 9, 10, 40, 41, 77, 90, 95]])
    nv = np.int32([7])
    tgt = np.int32([[26, 21, 22, 25, 24, 29, 0, 23, -5]])
    count, pos, score = run_lists(sc, cid, cp, nv, tgt, pad=2)
    assert count.tolist() == [[0, 1, 3, 4, 5, -1, -1, -1, -1]]
    assert pos.tolist() == [[77, 3, 9, 41, 40, -1, -1, -1, -1]]
    assert score[0, :5].tolist() == bits(sc[0, [5, 0, 1, 4, 3]]).tolist() and (score[0, 5:] == NAN_BITS).all()
    # with the dead column alive it is found, and it precedes the 0.5s
    count, pos, _ = run_lists(sc, cid, cp, np.int32([8]), tgt, pad=0)
    assert count.tolist() == [[0, 2, 4, 5, 6, 1, -1, -1, -1]] and pos[0, 5] == 95
    # a count outside [0, n] is clamped into it
    count, _, _ = run_lists(sc, cid, cp, np.int32([50]), tgt, pad=3)
    assert count.tolist() == [[0, 2, 4, 5, 6, 1, -1, -1, -1]]
    count, _, _ = run_lists(sc, cid, cp, np.int32([-3]), tgt, pad=0)
    assert (count == -1).all()


def test_lists_refusals_happen_before_any_launch():
    from recsys_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -3
    sc = torch.zeros(2, 16, device="cuda")
    ints = [torch.ones(2, 16, dtype=torch.int32, device="cuda") for _ in range(2)]
    nv, tg = torch.full((2,), 16, dtype=torch.int32, device="cuda"), torch.ones(2, 32, dtype=torch.int32, device="cuda")
    oc, op = (torch.full((2, 32), SENT_I, dtype=torch.int32, device="cuda") for _ in range(2))
    os_ = torch.full((2, 32), -7.0, device="cuda")
    s, ci, cp, n_, t_, a, b, c = (x.data_ptr() for x in (sc, ints[0], ints[1], nv, tg, oc, op, os_))
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    n0 = L.rsx_dbg_launch_count()
    #     scores ld cand_id cand_pos n_valid tgt_id T count pos score U n
    ok = (s, 16, ci, cp, n_, t_, 8, a, b, c, 2, 16)
    for at, bad in ((0, None), (2, None), (3, None), (4, None), (5, None), (7, None), (8, None), (9, None), (1, 15), (6, 0), (6, -1),
                    (10, 0), (11, 0)):
        args = list(ok)
        args[at] = bad
        assert L.rsx_rank_count_lists(*args, stream) == EINVAL, (at, bad)
    args = list(ok)
    args[6] = 33
    assert L.rsx_rank_count_lists(*args, stream) == EUNSUPPORTED and L.rsx_rank_count_lists_supported(16, 33) == 0
    assert L.rsx_dbg_launch_count() == n0
    torch.cuda.synchronize()
    assert (oc.cpu().numpy() == SENT_I).all() and (op.cpu().numpy() == SENT_I).all() and (os_.cpu().numpy() == -7.0).all()
    _lib.check(L.rsx_rank_count_lists(*ok, stream), "rsx_rank_count_lists")
    assert L.rsx_dbg_launch_count() == n0 + 1
    torch.cuda.synchronize()
    flat = oc.cpu().numpy().reshape(-1)                                  # [U = 2, T = 8], contiguous: the first 16 words
    assert (flat[:16] == 0).all() and (flat[16:] == SENT_I).all()


# ---- Predictor -----------------------------------------------------------------------------------------------------------
N = 500
KINDS = ("retrieved", "lost", "outside", "excluded", "pad", "duplicate")
OUTSIDE = 499                             # the bundle has 501 items, the catalogue holds items 0 .. 498


def eval_request(rng, ci, cc, table, U, T, seen, rep, salt=0):
    """Histories, `exclude` and held-out lists [U, T] built from `retrieve_candidates_host`, so that the slots' kinds are known:
    user 0 (never an empty history) is given a seed whose neighbour row names a copy of the duplicated item 5.  T >= 6: every
    user gets one slot of every kind it can have, user 0 all six.  T = 1: the kind rotates with (user, rep, salt).
    -> (hi, hc, exclude, held, kinds [U, T] of indices into KINDS, -1 for filler)."""
    from recsys_amd import serving
    pos, cnt = table
    special = (["full", "empty", "hole", "full", None] if rep != 1 else ["hole", "full", None, "empty", "full"])[:U]
    hi, hc, _, _ = make_request(rng, U, 1, 30, special, N_ITEM, N_CATE)
    exclude = rng.integers(-1, N - 1, (U, 9)).astype(np.int64)
    exclude[:, 0] = rng.integers(1, N - 1, U)
    rows = np.flatnonzero([(np.isin(pos[i, :cnt[i]], (5, N - 1))).any() and ci[i] != 5 for i in range(N)])
    only_high = [i for i in rows if 5 not in pos[i, :cnt[i]]]           # (the higher copy a neighbour, the lowest not: rare)
    seed = int(only_high[0] if only_high else rows[rep % len(rows)])
    hi[0, 0], hc[0, 0] = ci[seed], cc[seed]
    hi[0, 1:][hi[0, 1:] == 5] = 6
    exclude[0][np.isin(exclude[0], (5, ci[seed]))] = 0
    if exclude[0, 0] == 0:                                               # (every user keeps a positive exclusion id)
        exclude[0, 0] = 7 if ci[seed] != 7 else 8
    cands = serving.retrieve_candidates_host(pos, cnt, ci, hi, exclude, seen)
    ids = serving._exclusion_ids(hi, exclude, U, seen)
    held = np.zeros((U, T), np.int64)
    kinds = np.full((U, T), -1, np.int64)
    for u in range(U):
        ex = ids[u][(ids[u] > 0) & (ids[u] < N - 1)]
        got = np.setdiff1d(np.unique(ci[cands[u]]), [0, 5])
        lost = np.setdiff1d(np.arange(1, N - 1), np.concatenate([ci[cands[u]], ex, [5]]))
        pick = {"retrieved": int(rng.choice(got)) if len(got) else 0, "lost": int(rng.choice(lost)), "outside": OUTSIDE,
                "excluded": int(rng.choice(ex)), "pad": -1 if u % 2 else 0, "duplicate": 5 if u == 0 else 0}
        if T == 1:
            k = (u + rep + salt) % 6
            held[u, 0], kinds[u, 0] = pick[KINDS[k]], k
            continue
        slots = rng.permutation(T)
        for k, name in enumerate(KINDS):
            held[u, slots[k]], kinds[u, slots[k]] = pick[name], k
        more = rng.permutation(np.setdiff1d(np.concatenate([got, lost[:20]]), held[u]))[:T - 6]
        held[u, slots[6:6 + len(more)]] = more
    return hi, hc, exclude, held, kinds


def same_eval(got, want, metrics, one=False):
    for key, dtype in (("rank", np.int32), ("retrieved", np.int8), ("target_index", np.int32)):
        assert got[key].dtype == dtype and np.array_equal(got[key], want[key]), (key, got[key], want[key])
    assert got["target_prob"].dtype == np.float32 and np.array_equal(bits(got["target_prob"]), bits(want["target_prob"]))
    if one:
        assert isinstance(got["n_candidates"], int) and got["n_candidates"] == want["n_candidates"]
    else:
        assert got["n_candidates"].dtype == np.int32 and np.array_equal(got["n_candidates"], want["n_candidates"])
    assert sorted(got) == sorted(list(metrics) + ["rank", "retrieved", "target_index", "target_prob", "n_candidates"])
    for key, v in metrics.items():
        assert np.array_equal(np.asarray(got[key]), np.asarray(v), equal_nan=True), (key, got[key], v)


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("K", [16, 32])
def test_evaluate_two_stage_equals_its_definition(tmp_path_factory, K, graph):
    """The device path == the host path == two_stage_ranks_host over rank_candidates(whole catalogue), at N = 500 with
    user_block = 2: U = 5 is three blocks with a ragged last one.  Three requests per shape: with graphs the first runs
    eagerly (the second block of two users already captures), the later ones replay over other data."""
    from recsys_amd import serving
    ci, cc = catalogue(N)
    p = load(tmp_path_factory, K, 512, graph)                          # cap = 512 fits one rank launch: the device path
    ph = load(tmp_path_factory, K, 100, graph)                         # cap > max_candidates: the host path
    for q in (p, ph):
        q.set_catalogue(ci, cc)
        q.build_neighbours(32)
        assert q.evaluate_two_stage_path is None
    assert p.evaluate_two_stage_path_for(9) == "device" and ph.evaluate_two_stage_path_for(9) == "host"
    assert p.evaluate_two_stage_path_for(33) == "host" and p.evaluate_two_stage_path_for(32, n_neighbours=8) == "device"
    assert ph.evaluate_two_stage_path_for(1, hist_len=1) == "device"   # cap = 33 -> 64 <= 100
    pos, _, cnt = p._nbr["host"]
    rng = np.random.default_rng(23 + K)
    ks = (1, 10, 50)
    kinds_seen_T1 = set()
    for U, T, seen in [(U, T, seen) for U in (1, 3, 5) for T in (1, 9) for seen in (True, False)]:
        for rep in range(3):
            hi, hc, exclude, held, kinds = eval_request(rng, ci, cc, (pos, cnt), U, T, seen, rep, salt=U)
            prob = p.rank_candidates(hi, hc, np.tile(ci, (U, 1)), np.tile(cc, (U, 1)))["prob"]
            want = serving.two_stage_ranks_host(prob, pos, cnt, ci, hi, held, exclude, seen)
            # the comparison is not vacuous: the definition sees every kind of slot where the request was built to hold it
            code = want["retrieved"]
            for k, name in enumerate(KINDS):
                at = kinds == k
                if name == "retrieved":
                    ok = (code[at] == 1) | (held[at] == 0)             # (a user without a candidate has no such slot)
                elif name == "duplicate":
                    ok = (code[at] == 1) | (held[at] == 0)
                else:
                    ok = code[at] == {"lost": 0, "outside": -1, "excluded": -1, "pad": -2}[name]
                assert ok.all(), (name, U, T, seen, rep)
            if T == 9:
                assert (code == 1).sum() >= 2 and (code == 0).any() and (code == -1).sum() >= 2 * U and (code == -2).any()
                assert code[0][held[0] == 5].tolist() == [1]            # the duplicated item, retrieved for user 0
            else:
                kinds_seen_T1 |= {(KINDS[kinds[u, 0]], int(code[u, 0])) for u in range(U) if held[u, 0] or KINDS[kinds[u, 0]] == "pad"}
            metrics = serving.two_stage_metrics(want["rank"], want["retrieved"], want["n_candidates"], ks, per_user=True)
            got = p.evaluate_two_stage(hi, hc, held, ks, exclude_seen=seen, exclude=exclude, user_block=2, per_user=True)
            assert p.evaluate_two_stage_path == "device"
            same_eval(got, want, metrics)
            # the rank is the index in the list recommend_two_stage returns
            listed = p.recommend_two_stage(hi, hc, 1024, exclude_seen=seen, exclude=exclude)["index"]
            hit = got["retrieved"] == 1
            assert (got["rank"][hit] < 1024).all()
            for u, t in zip(*np.nonzero(hit)):
                assert listed[u, got["rank"][u, t]] == got["target_index"][u, t]
            if rep == 0:
                slow = ph.evaluate_two_stage(hi, hc, held, ks, exclude_seen=seen, exclude=exclude, user_block=2, per_user=True)
                assert ph.evaluate_two_stage_path == "host"
                same_eval(slow, want, metrics)
            if U == 1 and rep == 0:                                    # the one-user form: 1-D in, the leading axis dropped
                one = p.evaluate_two_stage(hi[0], hc[0], held[0], ks, exclude_seen=seen, exclude=exclude[0], user_block=2)
                w1 = {key: (int(v[0]) if key == "n_candidates" else v[0]) for key, v in want.items()}
                same_eval(one, w1, serving.two_stage_metrics(w1["rank"], w1["retrieved"], w1["n_candidates"], ks), one=True)
        if graph:
            for Ub in {min(U, 2), 1 if U % 2 else 2}:
                assert "graph" in p._graphs[("eval_two_stage", Ub, 1 if T == 1 else 32, 64 if seen else 32, 512, not seen, 32)]
    assert {("retrieved", 1), ("lost", 0), ("outside", -1), ("excluded", -1), ("pad", -2), ("duplicate", 1)} <= kinds_seen_T1
    assert not graph or p._n_graphs < p.MAX_GRAPHS                     # (no shape above ran eagerly for want of a slot)
    # without `exclude`
    hi, hc, _, held, _ = eval_request(rng, ci, cc, (pos, cnt), 3, 9, True, 0)
    prob = p.rank_candidates(hi, hc, np.tile(ci, (3, 1)), np.tile(cc, (3, 1)))["prob"]
    want = serving.two_stage_ranks_host(prob, pos, cnt, ci, hi, held)
    got = p.evaluate_two_stage(hi, hc, held)
    same_eval(got, want, serving.two_stage_metrics(want["rank"], want["retrieved"], want["n_candidates"], (10, 50, 100)))


def test_evaluate_two_stage_narrowed_tables_and_neighbours(tmp_path_factory):
    from recsys_amd import _lib, serving
    K = 16
    ci, cc = catalogue(N)
    p, p8 = load(tmp_path_factory, K, 512), load(tmp_path_factory, K, 512)
    for q, n in ((p, 32), (p8, 8)):
        q.set_catalogue(ci, cc)
        q.build_neighbours(n)
    pos, _, cnt = p._nbr["host"]
    rng = np.random.default_rng(77)
    hi, hc, exclude, held, _ = eval_request(rng, ci, cc, (pos, cnt), 5, 9, True, 0)
    tiled = (np.tile(ci, (5, 1)), np.tile(cc, (5, 1)))
    # the other entries give the same bits before and after
    before = (p.recommend(hi, hc, 10, exclude=exclude), p.recommend_two_stage(hi, hc, 10, exclude=exclude),
              p.evaluate_recommend(hi, hc, held, exclude=exclude))
    base = 500 * 32 * 8 + 500 * 4 + 4 * N_ITEM
    assert p.neighbours_buffer_bytes() == base
    # n_neighbours = 8 on the table built with 32 == a Predictor that built 8 == the definition over the narrowed table
    prob = p.rank_candidates(hi, hc, *tiled)["prob"]
    npos, ncnt = serving.narrow_neighbours_host(pos, cnt, 8)
    assert np.array_equal(npos, p8._nbr["host"][0]) and np.array_equal(ncnt, p8._nbr["host"][2])
    want = serving.two_stage_ranks_host(prob, npos, ncnt, ci, hi, held, exclude)
    metrics = serving.two_stage_metrics(want["rank"], want["retrieved"], want["n_candidates"], (10, 50, 100))
    for rep in range(3):                                               # eager, captured, replayed
        got = p.evaluate_two_stage(hi, hc, held, exclude=exclude, n_neighbours=8)
        assert p.evaluate_two_stage_path == "device"
        same_eval(got, want, metrics)
    same_eval(p8.evaluate_two_stage(hi, hc, held, exclude=exclude), want, metrics)
    same_eval(p8.evaluate_two_stage(hi, hc, held, exclude=exclude, n_neighbours=8), want, metrics)
    assert (want["retrieved"] == 1).any() and (want["retrieved"] == 0).any()
    full = p.evaluate_two_stage(hi, hc, held, exclude=exclude)
    assert (full["n_candidates"] >= got["n_candidates"]).all() and full["n_candidates"].sum() > got["n_candidates"].sum()
    assert sorted(p._nbr["narrow"]) == [8] and p.neighbours_buffer_bytes() == base + 500 * 8 * 4 + 500 * 4
    assert "narrow" not in p8._nbr
    same_eval(p.evaluate_two_stage(hi, hc, held, exclude=exclude, n_neighbours=32), full,
              {k: v for k, v in full.items() if k not in ("rank", "retrieved", "target_index", "target_prob", "n_candidates")})
    for bad in (0, 33, True):
        with pytest.raises(_lib.RsxError, match="n_neighbours"):
            p.evaluate_two_stage(hi, hc, held, n_neighbours=bad)
    # more than 256 distinct exclusion ids: the host path, the same answer
    many = np.tile(np.arange(200, 200 + 260), (5, 1))
    want_many = serving.two_stage_ranks_host(prob, pos, cnt, ci, hi, held, many)
    got = p.evaluate_two_stage(hi, hc, held, exclude=many)
    assert p.evaluate_two_stage_path == "host"
    same_eval(got, want_many, serving.two_stage_metrics(want_many["rank"], want_many["retrieved"], want_many["n_candidates"], (10, 50, 100)))
    after = (p.recommend(hi, hc, 10, exclude=exclude), p.recommend_two_stage(hi, hc, 10, exclude=exclude),
             p.evaluate_recommend(hi, hc, held, exclude=exclude))
    same(after[0], before[0])
    same(after[1], before[1])
    assert np.array_equal(after[2]["rank"], before[2]["rank"]) and np.array_equal(bits(after[2]["target_prob"]), bits(before[2]["target_prob"]))
    assert all(np.array_equal(np.asarray(after[2][k]), np.asarray(before[2][k]), equal_nan=True) for k in before[2] if k != "target_prob")
    # a replaced catalogue drops the table and the narrowed copies with it
    p.set_catalogue(ci[:400], cc[:400])
    assert p._nbr is None and p.neighbours_buffer_bytes() == 0
    assert not [k for k in p._graphs if isinstance(k, tuple) and k[0] == "eval_two_stage"]
    with pytest.raises(_lib.RsxError, match="build_neighbours"):
        p.evaluate_two_stage(hi, hc, held)
    p.build_neighbours(16)
    assert "narrow" not in p._nbr
    held4 = np.where(held >= 399, 0, held)
    prob = p.rank_candidates(hi, hc, np.tile(ci[:400], (5, 1)), np.tile(cc[:400], (5, 1)))["prob"]
    pos, _, cnt = p._nbr["host"]
    want = serving.two_stage_ranks_host(prob, pos, cnt, ci[:400], hi, held4, exclude)
    same_eval(p.evaluate_two_stage(hi, hc, held4, exclude=exclude), want,
              serving.two_stage_metrics(want["rank"], want["retrieved"], want["n_candidates"], (10, 50, 100)))
    assert p.evaluate_two_stage_path == "device"
