"""rsx_topk_rows_rules (csrc/topk_rules.hip) through ctypes, bit for bit: the selection with an allow bitmap and a per-category
cap against the numpy greedy definition over everything fed (the order of serving.recommend_host with a running list), over both
workgroup forms and the envelope's edge; without rules against rsx_topk_rows_excl / rsx_topk_rows; rows independent; the
refusals.  uint32 views of the values, equality of the integers, no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
f32 = lambda u: np.asarray(u, np.uint32).view(np.float32)
SHAPES = [(1, 16, 8, 4, 3, 1), (3, 37, 10, 30, 5, 2), (2, 1000, 24, 256, 20, 3), (2, 1000, 100, 32, 802, 16)]   # U n k E G m


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bitmap(ok):
    """bool [U, G] -> uint32 [U, ceil(G / 32)], bit g of row u = ok[u, g]."""
    U, G = ok.shape
    full = np.zeros((U, 32 * ((G + 31) // 32)), bool)
    full[:, :G] = ok
    return np.packbits(full.reshape(U, -1, 32), axis=-1, bitorder="little").view(np.uint32).reshape(U, -1)


class Rows:
    """Device buffers of one sequence of calls over U rows (out_val / out_idx [U, k], state [U, 2] zeroed), the categories of
    every entry the sequence will feed (cate, by absolute index), and the host's record of everything fed: the scores and
    which of them were eligible (not excluded, category inside [0, G) and allowed)."""

    def __init__(self, U, k, cate, G):
        self.U, self.k, self.G = U, k, G
        self.cate = np.asarray(cate, np.int64)
        self.fed = np.zeros((U, 0), np.float32)
        self.ok = np.zeros((U, 0), bool)
        self.alloc()

    def alloc(self):
        U, k = self.U, self.k
        self.cate_dev = dev(self.cate, np.int32)
        self.val = torch.full((U, k), -7.0, dtype=torch.float32, device="cuda")
        self.idx = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
        self.state = torch.zeros(U, 2, dtype=torch.int32, device="cuda")

    def feed(self, scores, cand_id, excl, allow, m, pad=0, entry="rules"):
        """One call.  allow: bool [U, G] or None.  entry "excl" / "plain": the same scores through rsx_topk_rows_excl /
        rsx_topk_rows (no rules)."""
        U, n = scores.shape
        a0 = self.fed.shape[1]
        assert a0 + n <= len(self.cate)
        self.launch(scores, cand_id, excl, allow, m, pad, entry)
        c = self.cate[a0:a0 + n]
        ok = np.stack([~np.isin(cand_id, excl[u][excl[u] > 0]) for u in range(U)])
        if allow is not None or m > 0:
            ok &= ((c >= 0) & (c < self.G))[None, :]
        if allow is not None:
            ok &= allow[:, np.clip(c, 0, self.G - 1)]
        self.fed, self.ok = np.concatenate([self.fed, scores], 1), np.concatenate([self.ok, ok], 1)
        return self

    def launch(self, scores, cand_id, excl, allow, m, pad, entry):
        from recsys_amd import _lib
        L = _lib.lib()
        U, n = scores.shape
        host = np.full((U, n + pad), np.inf, np.float32)
        host[:, :n] = scores
        sc = dev(host, np.float32)
        E = excl.shape[1]
        cid, ex = dev(cand_id, np.int32), dev(excl if E else np.zeros((U, 1)), np.int32)
        al = None if allow is None else dev(bitmap(allow).view(np.int32), np.int32)
        tail = (U, n, self.k, self.val.data_ptr(), self.idx.data_ptr(), self.state.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if entry == "rules":
            _lib.check(L.rsx_topk_rows_rules(sc.data_ptr(), n + pad, cid.data_ptr(), ex.data_ptr() if E else None, E,
                                             self.cate_dev.data_ptr(), self.G, None if al is None else al.data_ptr(), m, *tail),
                       "rsx_topk_rows_rules")
        elif entry == "excl":
            _lib.check(L.rsx_topk_rows_excl(sc.data_ptr(), n + pad, cid.data_ptr(), ex.data_ptr() if E else None, E, *tail), "rsx_topk_rows_excl")
        else:
            _lib.check(L.rsx_topk_rows(sc.data_ptr(), n + pad, *tail), "rsx_topk_rows")
        torch.cuda.synchronize()

    def result(self):
        return self.val.cpu().numpy(), self.idx.cpu().numpy(), self.state.cpu().numpy()


def greedy(rows, u, m):
    """-> (the capped list of row u over everything fed, the eligible positions in order)."""
    pos = np.flatnonzero(rows.ok[u])
    order = pos[np.lexsort((pos, -rows.fed[u, pos]))]
    if m == 0:
        return order[:rows.k], order
    taken, keep = {}, []
    for p in order:
        g = int(rows.cate[p])
        if taken.get(g, 0) < m:
            taken[g] = taken.get(g, 0) + 1
            keep.append(p)
            if len(keep) == rows.k:
                break
    return np.asarray(keep, np.int64), order


def check(rows, m):
    val, idx, st = rows.result()
    lists = []
    for u in range(rows.U):
        want, _ = greedy(rows, u, m)
        c = len(want)
        assert tuple(st[u]) == (c, rows.fed.shape[1]), (u, st[u], c)
        assert np.array_equal(idx[u, :c], want), u
        assert np.array_equal(bits(val[u, :c]), bits(rows.fed[u, want])), u
        lists.append(want)
    return val, idx, st, lists


def r_mixed(rng, U, n):
    """Probabilities with NaNs of several payloads, both zeros and a tie group."""
    a = rng.random((U, n), dtype=np.float32)
    pool = f32([0x7fc00000, 0xffc00001, 0x00000000, 0x80000000, 0x3f000000, 0x3f000000])
    m = rng.random((U, n)) < 0.3
    a[m] = pool[rng.integers(0, len(pool), int(m.sum()))]
    return a


def skewed(rng, G, total):
    """Categories in [0, G), the low ones frequent and half of the entries in the first two: the caps of the shapes here bind."""
    c = (rng.integers(0, G, total) ** 2) // G
    low = rng.random(total) < 0.5
    c[low] = rng.integers(0, min(G, 2), int(low.sum()))
    return c


def excl_rows(rng, U, E, ids):
    ex = np.zeros((U, E), np.int64)
    for u in range(U):
        take = rng.choice(ids, E)
        take[rng.random(E) < 0.25] = 0
        take[rng.random(E) < 0.1] = -3
        if E > 1:
            take[1] = take[0]
        ex[u] = take
    return ex


def run_three(rng, U, n, k, E, G, m, with_allow, cate=None):
    lens = (n, n // 2 + 1, n // 3 + 1)
    total = sum(lens)
    rows = Rows(U, k, skewed(rng, G, total) if cate is None else cate, G)
    allow = None
    if with_allow:
        allow = rng.random((U, G)) < 0.7
        allow[:, 0] = True
    n_ids = max(4, min(n // 2, 600))
    displaced = 0
    seen_lists = []
    for ln in lens:
        cid = rng.integers(0, n_ids, ln)
        ex = excl_rows(rng, U, E, np.arange(1, n_ids))
        rows.feed(r_mixed(rng, U, ln), cid, ex, allow, m, pad=1)
        seen_lists.append(check(rows, m)[3])
    final = seen_lists[-1]
    for u in range(U):
        _, order = greedy(rows, u, m)
        rank = {int(p): i for i, p in enumerate(order)}
        last = rank[int(final[u][-1])] if len(final[u]) == k else len(order)
        for earlier in seen_lists[:-1]:
            gone = np.setdiff1d(earlier[u], final[u])
            displaced += sum(1 for p in gone if rank[int(p)] < last)    # left although the uncapped cut would have kept it
    return rows, displaced


@pytest.mark.parametrize("with_allow", [False, True], ids=["all", "bitmap"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "U%d_n%d_k%d_E%d_G%d_m%d" % s)
def test_against_numpy(shape, with_allow):
    """Three chained calls of unequal length; excl with duplicates, padding and ids that hit; skewed categories, so that a
    later call pushes entries of the running list out of their category's top m.  (2, 1000, 100, 32, ...) takes the
    1024-thread form, (2, 1000, 24, 256, ...) the 256-thread one."""
    from recsys_amd import _lib
    U, n, k, E, G, m = shape
    L = _lib.lib()
    assert L.rsx_topk_rows_rules_supported(n, k, E, G, m) == 1
    rng = np.random.default_rng(n + k + G + 7 * with_allow)
    rows, displaced = run_three(rng, U, n, k, E, G, m, with_allow)
    assert displaced > 0 and not rows.ok.all()


def test_the_largest_n_of_the_envelope():
    """k = 1024, G = 802, m = 16: the largest n rsx_topk_rows_rules_supported accepts, found by probing."""
    from recsys_amd import _lib
    S = _lib.lib().rsx_topk_rows_rules_supported
    k, E, G, m = 1024, 256, 802, 16
    lo, hi = 1, 16384
    assert S(lo, k, E, G, m) == 1 and S(hi, k, E, G, m) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if S(mid, k, E, G, m) else (lo, mid)
    n = lo
    assert S(n, k, E, G, m) == 1 and S(n + 1, k, E, G, m) == 0 and 8000 < n < 16384 - k
    rows, displaced = run_three(np.random.default_rng(5), 1, n, k, E, G, m, True)
    assert displaced > 0 and rows.result()[2][0, 0] == k


def test_one_category_and_cap_one():
    """Every entry in one category, m = 1: exactly one survivor, the best of everything fed (every atomic of a round on one
    address); with equal scores the lowest index."""
    rng = np.random.default_rng(31)
    for (n, k) in ((40, 8), (3000, 100)):
        for recipe in (r_mixed, lambda r, U, c: np.full((U, c), 0.25, np.float32)):
            rows = Rows(2, k, np.full(3 * n, 4), 6)
            for _ in range(3):
                rows.feed(recipe(rng, 2, n), np.arange(1, n + 1), np.zeros((2, 0), np.int64), None, 1)
            _, idx, st, lists = check(rows, 1)
            assert np.array_equal(st, [[1, 3 * n], [1, 3 * n]]) and all(len(x) == 1 for x in lists)


def test_a_category_with_fewer_than_m_entries():
    rng = np.random.default_rng(32)
    cate = np.int64([0, 1, 1, 2, 1, 1, 0, 1, 1, 1, 1, 1])               # categories 0 and 2 hold fewer than m = 3
    rows = Rows(1, 8, cate, 3)
    for a, b in ((0, 5), (5, 12)):
        rows.feed(rng.random((1, b - a), dtype=np.float32), np.arange(1, b - a + 1), np.zeros((1, 0), np.int64), None, 3)
    _, idx, st, lists = check(rows, 3)
    assert st[0, 0] == 6 and sorted(cate[lists[0]].tolist()) == [0, 0, 1, 1, 1, 2]


def test_a_bitmap_that_allows_nothing():
    rng = np.random.default_rng(33)
    for (n, k) in ((20, 8), (1500, 100)):
        rows = Rows(2, k, rng.integers(0, 7, 2 * n), 7)
        for _ in range(2):
            rows.feed(r_mixed(rng, 2, n), np.arange(1, n + 1), np.zeros((2, 0), np.int64), np.zeros((2, 7), bool), 2)
        _, _, st, _ = check(rows, 2)
        assert np.array_equal(st, [[0, 2 * n], [0, 2 * n]])


def test_rows_are_independent():
    """cand_id and cate shared, excl and the bitmap per row: the row alone has the bits it has as row 2 of 3."""
    rng = np.random.default_rng(34)
    for (n, k, E, G, m) in ((200, 32, 16, 6, 2), (1500, 100, 64, 40, 3)):
        cate = skewed(rng, G, 2 * n)
        three, alone = Rows(3, k, cate, G), Rows(1, k, cate, G)
        allow = rng.random((3, G)) < 0.6
        allow[0], allow[2, :2] = ~allow[2], True
        for _ in range(2):
            a, cid, ex = r_mixed(rng, 3, n), rng.integers(0, 80, n), excl_rows(rng, 3, E, np.arange(1, 80))
            three.feed(a, cid, ex, allow, m)
            alone.feed(a[2:3], cid, ex[2:3], allow[2:3], m)
        (v3, i3, s3, _), (v1, i1, s1, _) = check(three, m), check(alone, m)
        c = int(s1[0, 0])
        assert np.array_equal(s3[2], s1[0]) and np.array_equal(i3[2, :c], i1[0, :c]) and np.array_equal(bits(v3[2, :c]), bits(v1[0, :c]))
        assert not np.array_equal(i3[0, :5], i3[2, :5])


@pytest.mark.parametrize("E", [0, 30])
def test_without_rules_is_rsx_topk_rows_excl(E):
    """allow = NULL and m = 0: the outputs and the state of rsx_topk_rows_excl (cate NULL or garbage alike); with E = 0 as
    well those of rsx_topk_rows."""
    from recsys_amd import _lib
    rng = np.random.default_rng(35 + E)
    for (U, n, k) in ((1, 16, 8), (3, 37, 10), (2, 1000, 24), (2, 1000, 100), (2, 300, 1024)):
        rules, other = Rows(U, k, np.full(3 * n, -5), 9), Rows(U, k, np.zeros(3 * n), 9)
        for _ in range(3):
            a, cid, ex = r_mixed(rng, U, n), rng.integers(0, 50, n), excl_rows(rng, U, E, np.arange(1, 50))
            rules.feed(a, cid, ex, None, 0, pad=2)
            other.feed(a, cid, ex, None, 0, pad=2, entry="excl" if E else "plain")
        (rv, ri, rs), (ov, oi, os_) = rules.result(), other.result()
        assert np.array_equal(rs, os_), (U, n, k)
        for u in range(U):
            c = int(rs[u, 0])
            assert c == min(k, int(rules.ok[u].sum()))
            assert np.array_equal(ri[u, :c], oi[u, :c]) and np.array_equal(bits(rv[u, :c]), bits(ov[u, :c])), (U, n, k, u)
        check(rules, 0)
    # ... and with cate = NULL
    rows = Rows(1, 4, np.zeros(8), 3)
    sc, cid = dev(np.float32([[3, 1, 2, 5, 4, 0, 7, 6]]), np.float32), dev(np.arange(8), np.int32)
    L = _lib.lib()
    _lib.check(L.rsx_topk_rows_rules(sc.data_ptr(), 8, cid.data_ptr(), None, 0, None, 0, None, 0, 1, 8, 4, rows.val.data_ptr(),
                                     rows.idx.data_ptr(), rows.state.data_ptr(), torch.cuda.current_stream().cuda_stream), "rsx_topk_rows_rules")
    torch.cuda.synchronize()
    assert rows.idx.cpu().numpy().tolist() == [[6, 7, 3, 4]] and rows.state.cpu().numpy().tolist() == [[4, 8]]


def test_a_category_outside_the_range_is_dropped():
    rng = np.random.default_rng(36)
    for m, allow in ((2, None), (0, np.ones((2, 5), bool)), (1, np.ones((2, 5), bool))):
        cate = rng.integers(0, 5, 120)
        cate[rng.random(120) < 0.3] = (-1, 5, 70000)[m]
        cate[::7] = 5
        cate[3::11] = -2 ** 31
        rows = Rows(2, 16, cate, 5)
        for a, b in ((0, 50), (50, 120)):
            rows.feed(r_mixed(rng, 2, b - a), np.arange(1, b - a + 1), np.zeros((2, 0), np.int64), allow, m)
        _, idx, st, lists = check(rows, m)
        assert all(((cate[x] >= 0) & (cate[x] < 5)).all() and len(x) > 0 for x in lists) and not rows.ok.all()


def test_two_identical_sequences_give_identical_bits():
    outs = []
    for _ in range(2):
        rng = np.random.default_rng(37)
        rows, _ = run_three(rng, 2, 1500, 100, 32, 11, 2, True)
        outs.append(rows.result())
    c = outs[0][2][:, 0]
    assert np.array_equal(outs[0][2], outs[1][2])
    for u in range(2):
        assert np.array_equal(outs[0][1][u, :c[u]], outs[1][1][u, :c[u]])
        assert np.array_equal(bits(outs[0][0][u, :c[u]]), bits(outs[1][0][u, :c[u]]))


def test_refusals_happen_before_any_launch():
    from recsys_amd import _lib
    L = _lib.lib()
    rows = Rows(2, 8, np.zeros(16), 3)
    sc = torch.zeros(2, 16, device="cuda")
    cid, ex = torch.ones(16, dtype=torch.int32, device="cuda"), torch.zeros(2, 256, dtype=torch.int32, device="cuda")
    al = torch.full((2, 1), -1, dtype=torch.int32, device="cuda")
    s, c, e, g, a, v, i, st = (t.data_ptr() for t in (sc, cid, ex, rows.cate_dev, al, rows.val, rows.idx, rows.state))
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    n0 = L.rsx_dbg_launch_count()
    EINVAL, EUNSUPPORTED = -1, -3
    ok = (s, 16, c, e, 4, g, 3, a, 2, 2, 16, 8, v, i, st)
    for at, bad in ((0, None), (2, None), (3, None), (12, None), (13, None), (14, None),       # needed pointers
                    (5, None),                                                                  # cate with a rule
                    (4, -1), (1, 15), (9, 0), (10, 0), (11, 0), (8, -1), (6, 0), (6, -3)):      # E, ld, U, n, k, m, G
        args = list(ok)
        args[at] = bad
        assert L.rsx_topk_rows_rules(*args, stream) == EINVAL, (at, bad)
    assert L.rsx_topk_rows_rules(s, 16, c, e, 4, None, 3, a, 0, 2, 16, 8, v, i, st, stream) == EINVAL     # a bitmap alone needs cate
    assert L.rsx_topk_rows_rules(s, 16, c, e, 4, g, 0, None, 1, 2, 16, 8, v, i, st, stream) == EINVAL     # a cap alone needs G
    for (n, k, E, G, m) in ((16, 8, 4, 3, 17), (16, 8, 257, 3, 1), (16, 1025, 4, 3, 1), (16384 - 8, 8, 4, 802, 1), (16384, 8, 4, 3, 0),
                            (16, 8, 4, 20000, 1)):
        assert L.rsx_topk_rows_rules(s, n, c, e, E, g, G, a, m, 2, n, k, v, i, st, stream) == EUNSUPPORTED, (n, k, E, G, m)
        assert L.rsx_topk_rows_rules_supported(n, k, E, G, m) == 0
    assert L.rsx_dbg_launch_count() == n0
    torch.cuda.synchronize()
    assert np.all(rows.val.cpu().numpy() == -7.0) and np.all(rows.state.cpu().numpy() == 0)
    _lib.check(L.rsx_topk_rows_rules(*ok, stream), "rsx_topk_rows_rules")
    _lib.check(L.rsx_topk_rows_rules(s, 16, c, None, 0, None, 0, None, 0, 2, 16, 8, v, i, st, stream), "rsx_topk_rows_rules")
    assert L.rsx_dbg_launch_count() == n0 + 2
