"""rsx_rank_count_rows (csrc/rank_count.hip) through ctypes against numpy's lexsort: the number of kept columns that precede
each target in the order of rsx_topk_rows, by integer equality -- over the three target capacities, one and several column
slices, padded rows, a first_index, special scores, duplicates of a target, skipped slots, accumulation over calls, an
ignored list, and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

f32 = lambda u: np.asarray(u, np.uint32).view(np.float32)
SHAPES = [(1, 1, 1, 0), (1, 63, 1, 0), (2, 257, 5, 4), (3, 4097, 32, 256)]
SENTINEL = -77
POOL = f32([0x3f000000, 0x3f000000, 0x3e800000, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001])


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def run(scores, cand_id, first, excl, tgt_score, tgt_pos, count0, pad=0, null_excl=False):
    """One call -> count [U, T].  Rows are padded to ld = n + pad with +inf, which would be counted for every target if read."""
    from recsys_amd import _lib
    U, n = scores.shape
    T, E = tgt_pos.shape[1], excl.shape[1]
    host = np.full((U, n + pad), np.inf, np.float32)
    host[:, :n] = scores
    sc, cid, ex = dev(host, np.float32), dev(cand_id, np.int32), dev(excl if excl.size else np.zeros((U, 1)), np.int32)
    ts, tp, cnt = dev(tgt_score, np.float32), dev(tgt_pos, np.int32), dev(count0, np.int32)
    _lib.check(_lib.lib().rsx_rank_count_rows(sc.data_ptr(), n + pad, cid.data_ptr(), first, None if null_excl else ex.data_ptr(), E,
                                              ts.data_ptr(), tp.data_ptr(), T, cnt.data_ptr(), U, n,
                                              torch.cuda.current_stream().cuda_stream), "rsx_rank_count_rows")
    torch.cuda.synchronize()
    return cnt.cpu().numpy()


def expected(scores, cand_id, first, excl, tgt_score, tgt_pos, count0):
    """numpy: the target goes IN FRONT of the row's kept columns, a stable lexsort by (-score, index) orders them, and the place
    the target lands at is the number of columns that precede it (its own column, an equal key, stays behind it)."""
    U, n = scores.shape
    want = count0.copy()
    idx = first + np.arange(n)
    for u in range(U):
        kept = ~np.isin(cand_id, excl[u][excl[u] > 0])
        for t in np.flatnonzero(tgt_pos[u] >= 0):
            s = np.concatenate([[tgt_score[u, t]], scores[u, kept]]).astype(np.float32)
            i = np.concatenate([[tgt_pos[u, t]], idx[kept]])
            want[u, t] += int(np.flatnonzero(np.lexsort((i, -s)) == 0)[0])
    return want


def special_scores(rng, U, n, share=0.5):
    a = rng.random((U, n), dtype=np.float32)
    m = rng.random((U, n)) < share
    a[m] = POOL[rng.integers(0, len(POOL), int(m.sum()))]
    return a


def case(rng, U, n, T, E, first, recipe=special_scores):
    """Scores, ids that repeat, exclusion lists that hit (with padding and duplicates), and targets of every kind: columns of
    this call (their own score), positions before and behind the call's range with scores of the special pool, skipped slots."""
    scores = recipe(rng, U, n)
    n_ids = max(2, n // 3)
    cand_id = rng.integers(0, n_ids, n)
    excl = rng.integers(-1, n_ids, (U, E))
    if E > 1:
        excl[:, 1] = excl[:, 0]
    tgt_pos = np.empty((U, T), np.int64)
    tgt_score = np.empty((U, T), np.float32)
    for u in range(U):
        for t in range(T):
            kind = (t + u) % 4 if T > 1 else 0
            if kind in (0, 1):                                       # a column of this call
                j = int(rng.integers(0, n))
                tgt_pos[u, t], tgt_score[u, t] = first + j, scores[u, j]
            elif kind == 2:                                          # outside the range: an earlier or a later chunk's entry
                tgt_pos[u, t] = int(rng.integers(0, first)) if first and rng.random() < 0.5 else first + n + int(rng.integers(0, 50))
                tgt_score[u, t] = POOL[rng.integers(0, len(POOL))] if rng.random() < 0.7 else scores[u, int(rng.integers(0, n))]
            else:
                tgt_pos[u, t], tgt_score[u, t] = -1, 0.75
    count0 = rng.integers(0, 5, (U, T)).astype(np.int32)             # += : what earlier chunks left
    count0[tgt_pos < 0] = SENTINEL
    return scores, cand_id, first, excl, tgt_score, tgt_pos, count0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "U%d_n%d_T%d_E%d" % s)
@pytest.mark.parametrize("first", [0, 1000])
def test_against_lexsort(shape, first):
    from recsys_amd import _lib
    U, n, T, E = shape
    assert _lib.lib().rsx_rank_count_rows_supported(n, T, E) == 1
    rng = np.random.default_rng(n + T + first)
    for recipe in (special_scores, lambda r, U, n: r.random((U, n), dtype=np.float32)):
        args = case(rng, U, n, T, E, first, recipe)
        got = run(*args, pad=3)
        want = expected(*args)
        assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)
        skipped = args[5] < 0
        assert (got[skipped] == SENTINEL).all()
    if n > 1:
        assert (want[~skipped] > args[6][~skipped]).any()            # something was counted
    if E:
        assert np.isin(args[1], args[3][0][args[3][0] > 0]).any()   # ... and the list excluded something


def test_special_scores_by_hand():
    """One row: ties, both zeros, both infinities and NaNs among the scores and among the targets."""
    #               j:  0     1     2      3       4      5       6      7     8
    sc = np.float32([[0.5, 0.0, 0.5, np.nan, -0.0, np.inf, -np.inf, np.nan, 0.5]])
    # order: 5 | 0 2 8 | 1 4 | 6 | 3 7
    cid = np.arange(1, 10)
    none = np.zeros((1, 0), np.int64)
    tp = np.int64([[5, 0, 2, 8, 1, 4, 6, 3, 7]])
    got = run(sc, cid, 0, none, sc[0, tp[0]][None, :], tp, np.zeros((1, 9), np.int32))
    assert got.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7, 8]]
    # targets that are no column of the row, positions 20 .. 26 (behind every column):
    ts = np.float32([[np.inf, 0.5, -0.0, 0.0, -np.inf, np.nan, 0.25]])
    got = run(sc, cid, 0, none, ts, np.int64([[20, 21, 22, 23, 24, 25, 26]]), np.zeros((1, 7), np.int32))
    assert got.tolist() == [[1, 4, 6, 6, 7, 9, 4]]
    # ... and in front of every column (the columns start at index 100): an equal score no longer precedes
    got = run(sc, cid, 100, none, ts, np.int64([[20, 21, 22, 23, 24, 25, 26]]), np.zeros((1, 7), np.int32))
    assert got.tolist() == [[0, 1, 4, 4, 6, 7, 4]]
    # with the 0.5 of column 2 and the zero of column 1 excluded
    got = run(sc, cid, 0, np.int64([[3, 2, 0]]), ts, np.int64([[20, 21, 22, 23, 24, 25, 26]]), np.zeros((1, 7), np.int32))
    assert got.tolist() == [[1, 3, 4, 4, 5, 7, 3]]


def test_duplicates_of_a_target():
    """The target is column 4 (index 104); its score also sits at columns 1 and 7.  The copy at the lower index precedes it,
    the copy at the higher one does not, and its own column compares equal."""
    sc = np.float32([[0.1, 0.6, 0.9, 0.2, 0.6, 0.3, 0.95, 0.6]])
    cid = np.int64([1, 5, 2, 3, 5, 4, 6, 5])
    got = run(sc, cid, 100, np.zeros((1, 0), np.int64), np.float32([[0.6, 0.6, 0.6]]), np.int64([[104, 101, 107]]), np.zeros((1, 3), np.int32))
    assert got.tolist() == [[3, 2, 4]]
    args = (sc, cid, 100, np.zeros((1, 0), np.int64), np.float32([[0.6]]), np.int64([[104]]), np.zeros((1, 1), np.int32))
    assert np.array_equal(run(*args), expected(*args))


def test_two_halves_accumulate_to_the_whole_row():
    rng = np.random.default_rng(7)
    for (U, n, T, E, cut) in ((2, 900, 7, 32, 300), (1, 2000, 32, 0, 1024)):
        sc, cid, first, ex, ts, tp, c0 = case(rng, U, n, T, E, 50)
        whole = run(sc, cid, first, ex, ts, tp, c0)
        half = run(sc[:, :cut], cid[:cut], first, ex, ts, tp, c0, pad=n - cut)
        both = run(sc[:, cut:], cid[cut:], first + cut, ex, ts, tp, half, pad=1)
        assert np.array_equal(both, whole) and np.array_equal(whole, expected(sc, cid, first, ex, ts, tp, c0))
        assert not np.array_equal(half, whole)


def test_rows_are_independent_and_E0_ignores_the_list():
    from recsys_amd import _lib
    rng = np.random.default_rng(9)
    sc, cid, first, ex, ts, tp, c0 = case(rng, 3, 700, 8, 16, 10)
    three = run(sc, cid, first, ex, ts, tp, c0)
    alone = run(sc[2:], cid, first, ex[2:], ts[2:], tp[2:], c0[2:])
    assert np.array_equal(three[2:], alone)
    # E = 0 with a list that would exclude everything, and with no list at all
    U, n, T = 2, 300, 4
    sc, cid, first, _, ts, tp, c0 = case(rng, U, n, T, 0, 0)
    none = np.zeros((U, 0), np.int64)
    want = expected(sc, cid, first, none, ts, tp, c0)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    t = [dev(sc, np.float32), dev(cid, np.int32), dev(np.tile(np.arange(n), (U, 1)), np.int32), dev(ts, np.float32), dev(tp, np.int32),
         dev(c0, np.int32)]
    s, c, e, a, b, k = (x.data_ptr() for x in t)
    _lib.check(L.rsx_rank_count_rows(s, n, c, first, e, 0, a, b, T, k, U, n, stream), "rsx_rank_count_rows")
    torch.cuda.synchronize()
    assert np.array_equal(t[5].cpu().numpy(), want)
    assert np.array_equal(run(sc, cid, first, none, ts, tp, c0, null_excl=True), want)


def test_refusals_happen_before_any_launch():
    from recsys_amd import _lib
    L = _lib.lib()
    assert L.rsx_rank_count_rows_supported(1, 1, 0) == 1 and L.rsx_rank_count_rows_supported(1 << 24, 32, 256) == 1
    for (n, T, E) in ((0, 1, 0), (16, 0, 4), (16, 33, 4), (16, 8, -1), (16, 8, 257)):
        assert L.rsx_rank_count_rows_supported(n, T, E) == 0, (n, T, E)
    sc = torch.zeros(2, 16, device="cuda")
    cid, ex = torch.ones(16, dtype=torch.int32, device="cuda"), torch.zeros(2, 256, dtype=torch.int32, device="cuda")
    ts, tp = torch.zeros(2, 32, device="cuda"), torch.zeros(2, 32, dtype=torch.int32, device="cuda")
    cnt = torch.full((2, 32), SENTINEL, dtype=torch.int32, device="cuda")
    s, c, e, a, b, k = (t.data_ptr() for t in (sc, cid, ex, ts, tp, cnt))
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    n0 = L.rsx_dbg_launch_count()
    EINVAL, EUNSUPPORTED = -1, -3
    #        scores ld cand first excl E tgt_score tgt_pos T count U n
    ok = (s, 16, c, 0, e, 4, a, b, 8, k, 2, 16)
    for at, bad in ((0, None), (2, None), (4, None), (6, None), (7, None), (9, None), (1, 15), (3, -1), (5, -1), (8, 0), (8, -2),
                    (10, 0), (11, 0)):
        args = list(ok)
        args[at] = bad
        assert L.rsx_rank_count_rows(*args, stream) == EINVAL, (at, bad)
    for at, bad in ((5, 257), (8, 33), (3, 2 ** 31 - 1 - 16), (3, 2 ** 31 - 2)):
        args = list(ok)
        args[at] = bad
        assert L.rsx_rank_count_rows(*args, stream) == EUNSUPPORTED, (at, bad)
    assert L.rsx_dbg_launch_count() == n0
    torch.cuda.synchronize()
    assert (cnt.cpu().numpy() == SENTINEL).all()
    cnt.zero_()
    _lib.check(L.rsx_rank_count_rows(*ok, stream), "rsx_rank_count_rows")
    _lib.check(L.rsx_rank_count_rows(s, 16, c, 2 ** 31 - 2 - 16, None, 0, a, b, 8, k, 2, 16, stream), "rsx_rank_count_rows")
    assert L.rsx_dbg_launch_count() == n0 + 2
    torch.cuda.synchronize()
