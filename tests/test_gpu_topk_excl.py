"""rsx_topk_rows_excl (csrc/topk_excl.hip) and rsx_predict_din_rank_shared (csrc/predict_din.hip) through ctypes, bit for bit:
the filtered selection against rsx_topk_rows where nothing is excluded and against numpy (the order of serving.recommend_host
with a running list) where something is, over both workgroup forms and the envelope's edge; rows independent; the refusals;
the shared rank launch against rsx_predict_din_rank on the replicated candidates.  uint32 views of the values, equality of
the integers, no tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
f32 = lambda u: np.asarray(u, np.uint32).view(np.float32)
SIZES = [(1, 16, 8, 4), (3, 37, 10, 30), (2, 1000, 24, 256), (2, 1000, 100, 32), (1, 16384 - 1024, 1024, 256)]


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


class Rows:
    """Device buffers of one sequence of calls over U rows (out_val / out_idx [U, k], state [U, 2] zeroed) and the host's
    record of everything fed: the scores and which of them were kept."""

    def __init__(self, U, k):
        self.U, self.k = U, k
        self.val = torch.full((U, k), -7.0, dtype=torch.float32, device="cuda")
        self.idx = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
        self.state = torch.zeros(U, 2, dtype=torch.int32, device="cuda")
        self.fed = np.zeros((U, 0), np.float32)
        self.kept = np.zeros((U, 0), bool)

    def feed(self, scores, cand_id=None, excl=None, pad=0):
        """One call.  excl None: rsx_topk_rows; else rsx_topk_rows_excl with excl [U, E] (E may be 0)."""
        from recsys_amd import _lib
        U, n = scores.shape
        host = np.full((U, n + pad), np.inf, np.float32)
        host[:, :n] = scores
        sc = dev(host, np.float32)
        stream = torch.cuda.current_stream().cuda_stream
        tail = (U, n, self.k, self.val.data_ptr(), self.idx.data_ptr(), self.state.data_ptr(), stream)
        if excl is None:
            _lib.check(_lib.lib().rsx_topk_rows(sc.data_ptr(), n + pad, *tail), "rsx_topk_rows")
            kept = np.ones((U, n), bool)
        else:
            E = excl.shape[1]
            cid, ex = dev(cand_id, np.int32), dev(excl if E else np.zeros((U, 1)), np.int32)
            _lib.check(_lib.lib().rsx_topk_rows_excl(sc.data_ptr(), n + pad, cid.data_ptr(), ex.data_ptr() if E else None, E, *tail),
                       "rsx_topk_rows_excl")
            kept = np.stack([~np.isin(cand_id, excl[u][excl[u] > 0]) for u in range(U)])
        torch.cuda.synchronize()
        self.fed, self.kept = np.concatenate([self.fed, scores], 1), np.concatenate([self.kept, kept], 1)
        return self

    def result(self):
        return self.val.cpu().numpy(), self.idx.cpu().numpy(), self.state.cpu().numpy()


def check(rows):
    """The device's list against numpy over everything fed so far: the kept entries in the order of recommend_host."""
    val, idx, st = rows.result()
    for u in range(rows.U):
        pos = np.flatnonzero(rows.kept[u])
        order = pos[np.lexsort((pos, -rows.fed[u, pos]))][:rows.k]
        c = len(order)
        assert tuple(st[u]) == (c, rows.fed.shape[1]), (u, st[u], c)
        assert np.array_equal(idx[u, :c], order), u
        assert np.array_equal(bits(val[u, :c]), bits(rows.fed[u, order])), u
    return val, idx, st


def r_mixed(rng, U, n):
    """Probabilities with NaNs of several payloads, both zeros and a tie group."""
    a = rng.random((U, n), dtype=np.float32)
    pool = f32([0x7fc00000, 0xffc00001, 0x00000000, 0x80000000, 0x3f000000, 0x3f000000])
    m = rng.random((U, n)) < 0.3
    a[m] = pool[rng.integers(0, len(pool), int(m.sum()))]
    return a


def r_equal(rng, U, n):
    return np.full((U, n), 0.25, np.float32)


def excl_rows(rng, U, E, ids):
    """[U, E], different per row: ids of `ids` (so that some scores leave), ids nobody has, padding (0, negative), duplicates."""
    ex = np.zeros((U, E), np.int64)
    for u in range(U):
        take = rng.choice(ids, E)
        take[rng.random(E) < 0.25] = 0
        take[rng.random(E) < 0.1] = -3
        take[rng.random(E) < 0.1] = 10 ** 6 + u
        if E > 1:
            take[1] = take[0]
        ex[u] = take
    return ex


@pytest.mark.parametrize("chained", [1, 3])
def test_nothing_excluded_is_rsx_topk_rows(chained):
    """E = 0, and E > 0 with only padding in excl: the outputs (the first `filled` pairs) and the state of rsx_topk_rows."""
    rng = np.random.default_rng(3 + chained)
    for (U, n, k, E) in SIZES[:4] + [(2, 300, 1024, 8)]:
        for Ex in (0, E):
            plain, fil = Rows(U, k), Rows(U, k)
            for _ in range(chained):
                a = r_mixed(rng, U, n)
                cid = rng.integers(0, 50, n)
                plain.feed(a, pad=2)
                fil.feed(a, cid, -rng.integers(0, 3, (U, Ex)), pad=2)
            (pv, pi, ps), (fv, fi, fs) = plain.result(), fil.result()
            assert np.array_equal(ps, fs), (U, n, k, Ex)
            c = int(ps[0, 0])
            assert c == min(k, chained * n)
            assert np.array_equal(pi[:, :c], fi[:, :c]) and np.array_equal(bits(pv[:, :c]), bits(fv[:, :c])), (U, n, k, Ex)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "U%d_n%d_k%d_E%d" % s)
@pytest.mark.parametrize("recipe", [r_mixed, r_equal], ids=["mixed", "equal"])
def test_against_numpy(size, recipe):
    """Two chained calls with different ids and scores; excl with duplicates, padding and ids that hit.  (2, 1000, 100, 32)
    takes the 1024-thread form, (2, 1000, 24, 256) the 256-thread one."""
    from recsys_amd import _lib
    U, n, k, E = size
    L = _lib.lib()
    assert L.rsx_topk_rows_excl_supported(n, k, E) == 1
    assert L.rsx_topk_rows_threads(n, k) == (256 if n + k <= 1024 else 1024)
    if size == (2, 1000, 100, 32):
        assert L.rsx_topk_rows_threads(n, k) == 1024
    rng = np.random.default_rng(n + k)
    rows = Rows(U, k)
    n_ids = max(4, min(n // 2, 600))                                # ids repeat: equal ids leave together
    for call in range(2):
        cid = rng.integers(0, n_ids, n)
        cid[0], cid[1] = 0, 1                                       # id 0 is never excluded; id 1 always is
        ex = excl_rows(rng, U, E, np.arange(1, n_ids))
        ex[:, 0] = 1
        rows.feed(recipe(rng, U, n), cid, ex, pad=1)
        check(rows)
        assert rows.kept[:, call * n].all() and not rows.kept.all()


def test_every_new_score_excluded_leaves_the_list():
    rng = np.random.default_rng(21)
    for (U, n, k) in ((2, 40, 16), (1, 1500, 100)):
        rows = Rows(U, k)
        rows.feed(r_mixed(rng, U, n), rng.integers(1, 9, n), np.full((U, 3), 99))
        v0, i0, s0 = check(rows)
        rows.feed(rng.random((U, n), dtype=np.float32) + 5.0, rng.integers(1, 9, n), np.tile(np.arange(0, 12), (U, 1)))
        v1, i1, s1 = check(rows)
        assert not rows.kept[:, n:].any()
        c = int(s0[0, 0])
        assert np.array_equal(i0[:, :c], i1[:, :c]) and np.array_equal(bits(v0[:, :c]), bits(v1[:, :c]))
        assert np.array_equal(s1, np.stack([s0[:, 0], s0[:, 1] + n], 1))
    rows = Rows(2, 8)                                               # ... and with an empty list: count 0
    rows.feed(rng.random((2, 20), dtype=np.float32), np.full(20, 4), np.full((2, 2), 4))
    _, _, st = check(rows)
    assert np.array_equal(st, [[0, 20], [0, 20]])


def test_fewer_kept_than_k_while_the_union_is_longer():
    """filled + kept < k < filled + n, in both workgroup forms."""
    rng = np.random.default_rng(22)
    for (n1, n2, k, keep) in ((4, 16, 10, 3), (30, 1200, 100, 17), (0, 50, 20, 5)):
        rows = Rows(2, k)
        if n1:
            rows.feed(r_mixed(rng, 2, n1), np.arange(1, n1 + 1), np.zeros((2, 1)))
        cid = np.full(n2, 7)
        cid[rng.permutation(n2)[:keep]] = 8
        rows.feed(r_mixed(rng, 2, n2), cid, np.int64([[7, 0], [0, 7]]))
        _, _, st = check(rows)
        assert np.array_equal(st[:, 0], [n1 + keep, n1 + keep]) and n1 + keep < k < n1 + n2


def test_rows_are_independent():
    """cand_id shared, excl per row: the row alone has the bits it has as row 2 of 3."""
    rng = np.random.default_rng(23)
    for (n, k, E) in ((200, 32, 16), (1500, 100, 64)):
        three, alone = Rows(3, k), Rows(1, k)
        for _ in range(2):
            a, cid, ex = r_mixed(rng, 3, n), rng.integers(0, 80, n), excl_rows(rng, 3, E, np.arange(1, 80))
            three.feed(a, cid, ex)
            alone.feed(a[2:3], cid, ex[2:3])
        (v3, i3, s3), (v1, i1, s1) = check(three), check(alone)
        c = int(s1[0, 0])
        assert np.array_equal(s3[2], s1[0]) and np.array_equal(i3[2, :c], i1[0, :c]) and np.array_equal(bits(v3[2, :c]), bits(v1[0, :c]))
        assert not np.array_equal(i3[0, :c], i3[2, :c])


def test_refusals_happen_before_any_launch():
    from recsys_amd import _lib
    L = _lib.lib()
    assert L.rsx_topk_rows_excl_supported(16384 - 1024, 1024, 256) == 1 and L.rsx_topk_rows_excl_supported(1, 1, 0) == 1
    for (n, k, E) in ((16, 8, -1), (16, 8, 257), (16384 - 1023, 1024, 4), (16, 1025, 4), (0, 1, 0), (1, 0, 0)):
        assert L.rsx_topk_rows_excl_supported(n, k, E) == 0, (n, k, E)
    assert L.rsx_topk_rows_threads(16384, 8) == 0 and L.rsx_topk_rows_threads(16, 8) == 256
    rows = Rows(2, 8)
    sc = torch.zeros(2, 16, device="cuda")
    cid, ex = torch.ones(16, dtype=torch.int32, device="cuda"), torch.zeros(2, 256, dtype=torch.int32, device="cuda")
    s, c, e, v, i, st = (t.data_ptr() for t in (sc, cid, ex, rows.val, rows.idx, rows.state))
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    n0 = L.rsx_dbg_launch_count()
    EINVAL, EUNSUPPORTED = -1, -3
    for args in ((None, 16, c, e, 4, 2, 16, 8, v, i, st), (s, 16, None, e, 4, 2, 16, 8, v, i, st), (s, 16, c, None, 4, 2, 16, 8, v, i, st),
                 (s, 16, c, e, 4, 2, 16, 8, None, i, st), (s, 16, c, e, 4, 2, 16, 8, v, None, st), (s, 16, c, e, 4, 2, 16, 8, v, i, None),
                 (s, 16, c, e, -1, 2, 16, 8, v, i, st), (s, 15, c, e, 4, 2, 16, 8, v, i, st), (s, 16, c, e, 4, 0, 16, 8, v, i, st),
                 (s, 16, c, e, 4, 2, 0, 8, v, i, st), (s, 16, c, e, 4, 2, 16, 0, v, i, st)):
        assert L.rsx_topk_rows_excl(*args, stream) == EINVAL, args
    for (n, k, E) in ((16, 8, 257), (16, 1025, 4), (16384, 8, 4), (16384 - 7, 8, 0)):
        assert L.rsx_topk_rows_excl(s, n, c, e, E, 2, n, k, v, i, st, stream) == EUNSUPPORTED, (n, k, E)
    assert L.rsx_dbg_launch_count() == n0
    torch.cuda.synchronize()
    assert np.all(rows.val.cpu().numpy() == -7.0) and np.all(rows.state.cpu().numpy() == 0)
    _lib.check(L.rsx_topk_rows_excl(s, 16, c, e, 4, 2, 16, 8, v, i, st, stream), "rsx_topk_rows_excl")
    _lib.check(L.rsx_topk_rows_excl(s, 16, c, None, 0, 2, 16, 8, v, i, st, stream), "rsx_topk_rows_excl")
    assert L.rsx_dbg_launch_count() == n0 + 2


@pytest.mark.parametrize("K", [16, 32])
@pytest.mark.parametrize("shape", [(1, 1, 30), (3, 37, 30), (2, 200, 100)], ids=lambda s: "U%d_C%d_P%d" % s)
def test_rank_shared_is_rank_on_replicated_candidates(tmp_path_factory, K, shape):
    from recsys_amd import _lib, serving
    from tests.test_gpu_din_rank import din_bundle, make_request
    U, Cn, P = shape
    d, _ = din_bundle(tmp_path_factory, K, P)
    pred = serving.Predictor.load(d, max_candidates=1024)
    model = pred._rank_setup(U)["model"]
    hi, hc, ci, cc = make_request(np.random.default_rng(K + Cn), U, Cn, P, ("hole", "empty", "full")[:U])
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    t = {k: dev(x, np.int32) for k, x in (("hi", hi), ("hc", hc), ("ci", np.tile(ci[0], (U, 1))), ("cc", np.tile(cc[0], (U, 1))))}
    rep = torch.full((U, Cn), -1.0, device="cuda")
    sh = torch.full((U, Cn), -2.0, device="cuda")
    torch.cuda.synchronize()
    n0 = L.rsx_dbg_launch_count()
    _lib.check(L.rsx_predict_din_rank(C.byref(model), t["hi"].data_ptr(), t["hc"].data_ptr(), t["ci"].data_ptr(), t["cc"].data_ptr(),
                                      rep.data_ptr(), U, Cn, P, stream), "rsx_predict_din_rank")
    _lib.check(L.rsx_predict_din_rank_shared(C.byref(model), t["hi"].data_ptr(), t["hc"].data_ptr(), t["ci"].data_ptr(),
                                             t["cc"].data_ptr(), sh.data_ptr(), U, Cn, P, stream), "rsx_predict_din_rank_shared")
    assert L.rsx_dbg_launch_count() == n0 + 2
    torch.cuda.synchronize()
    a, b = rep.cpu().numpy(), sh.cpu().numpy()
    assert np.array_equal(bits(a), bits(b)) and a.min() > 0.0 and a.max() < 1.0
    if U > 1:
        assert not np.array_equal(bits(a[0]), bits(a[-1]))          # the users' histories differ, so do their rows
    assert L.rsx_predict_din_rank_shared(C.byref(model), t["hi"].data_ptr(), t["hc"].data_ptr(), None, t["cc"].data_ptr(),
                                         sh.data_ptr(), U, Cn, P, stream) == -1
    assert L.rsx_predict_din_rank_shared(C.byref(model), t["hi"].data_ptr(), t["hc"].data_ptr(), t["ci"].data_ptr(),
                                         t["cc"].data_ptr(), sh.data_ptr(), U, Cn, 129, stream) == -3
