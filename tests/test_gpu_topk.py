"""rsx_topk_rows (csrc/topk.hip) through ctypes against serving.topk_rows_host, bit for bit: uint32 views of the values,
equality of the indices, no tolerance.  Sizes around the wave (64) and workgroup (256 / 1024 threads, the switch at n + k = 1024)
edges, k > n, rows with a leading dimension whose padding holds +inf, score recipes that put the k-th place inside a tie group,
the running list over unequal chunks, row independence, and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096]
KS = [1, 2, 3, 64, 100, 1000, 1024]
bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
f32 = lambda u: np.asarray(u, np.uint32).view(np.float32)


class Rows:
    """Device buffers of one sequence of calls over U rows: out_val / out_idx [U, k] and state [U, 2] (zeroed)."""

    def __init__(self, U, k):
        self.U, self.k = U, k
        self.val = torch.full((U, k), -7.0, dtype=torch.float32, device="cuda")
        self.idx = torch.full((U, k), -7, dtype=torch.int32, device="cuda")
        self.state = torch.zeros(U, 2, dtype=torch.int32, device="cuda")

    def feed(self, scores, pad=0):
        """scores: float32 [U, n] -> one call; `pad` extra columns of +inf behind every row (ld = n + pad)."""
        from recsys_amd import _lib
        U, n = scores.shape
        assert U == self.U
        host = np.full((U, n + pad), np.inf, np.float32)
        host[:, :n] = scores
        dev = torch.from_numpy(host).cuda()
        _lib.check(_lib.lib().rsx_topk_rows(dev.data_ptr(), n + pad, U, n, self.k, self.val.data_ptr(), self.idx.data_ptr(),
                                            self.state.data_ptr(), torch.cuda.current_stream().cuda_stream), "rsx_topk_rows")
        torch.cuda.synchronize()
        return self

    def result(self):
        st = self.state.cpu().numpy()
        return self.val.cpu().numpy(), self.idx.cpu().numpy(), st


def check(rows, full):
    """The device's list after all calls against the host selection over `full` [U, C] (everything fed so far)."""
    from recsys_amd import serving
    val, idx, st = rows.result()
    want = serving.topk_rows_host(full, rows.k)
    kk = want["index"].shape[1]
    assert kk == min(rows.k, full.shape[1])
    assert np.array_equal(st[:, 0], np.full(rows.U, kk)) and np.array_equal(st[:, 1], np.full(rows.U, full.shape[1])), st
    assert np.array_equal(idx[:, :kk], want["index"]), (full.shape, rows.k)
    assert np.array_equal(bits(val[:, :kk]), bits(want["prob"])), (full.shape, rows.k)
    return val[:, :kk], idx[:, :kk]


# ---- score recipes: (rng, U, n) -> float32 [U, n], different rows ---------------------------------------------------------------
def r_uniform(rng, U, n):
    return rng.random((U, n), dtype=np.float32)


def r_all_equal(rng, U, n):
    return np.repeat(np.float32([0.25, 0.5, -3.0])[:U, None], n, 1)


def r_four_values(rng, U, n):                    # the k-th place falls inside a tie group for almost every k
    return np.float32([0.125, 0.5, 0.5000001, 0.75])[rng.integers(0, 4, (U, n))]


def r_low_bit(rng, U, n):                        # neighbours in the lowest mantissa bit
    return f32((0x3f000000 + rng.integers(0, 3, (U, n))).astype(np.uint32))


def r_signs(rng, U, n):                          # +-0, +-denormals, +-tiny
    pool = f32([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000])
    return pool[rng.integers(0, len(pool), (U, n))]


def r_inf(rng, U, n):
    a = rng.standard_normal((U, n)).astype(np.float32)
    c = rng.integers(0, 4, (U, n))
    a[c == 0], a[c == 1] = np.inf, -np.inf
    return a


def r_nan(share):
    def make(rng, U, n):
        a = rng.random((U, n), dtype=np.float32)
        pool = f32([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fc12345])
        m = rng.random((U, n)) < share
        a[m] = pool[rng.integers(0, len(pool), int(m.sum()))]
        return a
    return make


RECIPES = {"uniform": r_uniform, "all_equal": r_all_equal, "four_values": r_four_values, "low_bit": r_low_bit, "signs": r_signs,
           "inf": r_inf, "nan_few": r_nan(0.05), "nan_most": r_nan(0.95), "nan_all": r_nan(2.0)}


@pytest.mark.parametrize("n", NS)
def test_sizes_around_wave_and_workgroup_edges(n):
    """Every (n, k), U in {1, 3}, ld > n with +inf in the padding (never selected: every selected index is < n and its
    value is the row's own)."""
    rng = np.random.default_rng(100 + n)
    for k in KS:
        for U in (1, 3):
            a = r_four_values(rng, U, n) if (k + U) % 2 else r_uniform(rng, U, n)
            val, idx = check(Rows(U, k).feed(a, pad=5), a)
            assert idx.max() < n and not np.isinf(val).any()


@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_score_recipes(recipe):
    """Each recipe at several (n, k): k below, inside and above the number of finite scores / the tie groups; both
    workgroup sizes (n + k <= 1024 and above)."""
    rng = np.random.default_rng(sum(map(ord, recipe)))
    for (n, k) in ((37, 10), (64, 64), (257, 100), (1000, 3), (1000, 1024), (4096, 100), (4096, 1024), (700, 324), (701, 324)):
        for U in (1, 3):
            a = RECIPES[recipe](rng, U, n)
            check(Rows(U, k).feed(a, pad=3), a)


def test_nan_counts_around_k():
    """More numbers than k, exactly k, fewer than k, none: the NaNs fill the tail in index order with their own bits."""
    rng = np.random.default_rng(9)
    n, k = 300, 100
    for numbers in (200, 100, 99, 7, 0):
        a = r_nan(2.0)(rng, 3, n)
        for u in range(3):
            at = rng.permutation(n)[:numbers]
            a[u, at] = rng.random(numbers, dtype=np.float32)
        val, idx = check(Rows(3, k).feed(a), a)
        assert int(np.isnan(val).sum()) == 3 * max(0, k - numbers)


@pytest.mark.parametrize("recipe", ["uniform", "four_values", "nan_few", "all_equal", "signs"])
def test_running_list_over_chunks(recipe):
    """A row fed as 3 and as 7 unequal chunks == the single call; a first and a last chunk shorter than k; the indices come
    from the device state alone (the host passes no base)."""
    rng = np.random.default_rng(7 + len(recipe))
    for (C, k, cuts) in ((1000, 100, (40, 700)), (1000, 100, (3, 60, 61, 400, 410, 950)), (5000, 1024, (500, 4600)),
                         (300, 64, (1, 2, 3, 130, 131, 298)), (150, 200, (20, 90))):
        for U in (1, 3):
            a = RECIPES[recipe](rng, U, C)
            whole = Rows(U, k).feed(a)
            wv, wi = check(whole, a)
            parts = Rows(U, k)
            edges = (0,) + cuts + (C,)
            for s, e in zip(edges[:-1], edges[1:]):
                parts.feed(a[:, s:e], pad=2)
                check(parts, a[:, :e])                       # the list is right after every chunk
            pv, pi = check(parts, a)
            assert np.array_equal(pi, wi) and np.array_equal(bits(pv), bits(wv))


def test_second_request_shows_no_trace_of_the_first():
    rng = np.random.default_rng(13)
    rows = Rows(3, 50)
    a = rng.random((3, 400), dtype=np.float32) + 10.0             # a first request of large scores
    rows.feed(a[:, :250]).feed(a[:, 250:])
    check(rows, a)
    rows.state.zero_()                                           # the list's old entries stay in out_val / out_idx
    b = rng.random((3, 90), dtype=np.float32)
    rows.feed(b[:, :20]).feed(b[:, 20:])
    val, idx = check(rows, b)
    assert val.max() < 1.0 and idx.max() < 90


def test_rows_are_independent():
    """Row 1 of 3 has the bits it has alone, over a chunked sequence."""
    rng = np.random.default_rng(17)
    for (C, k) in ((900, 100), (3000, 1000)):
        a = r_four_values(rng, 3, C)
        three, alone = Rows(3, k), Rows(1, k)
        for s, e in ((0, C // 3), (C // 3, C)):
            three.feed(a[:, s:e])
            alone.feed(a[1:2, s:e])
        v3, i3 = check(three, a)
        v1, i1 = check(alone, a[1:2])
        assert np.array_equal(i3[1], i1[0]) and np.array_equal(bits(v3[1]), bits(v1[0]))


def test_refusals_happen_before_any_launch():
    from recsys_amd import _lib
    L = _lib.lib()
    assert L.rsx_topk_rows_supported(4096, 100) == 1 and L.rsx_topk_rows_supported(16384 - 1024, 1024) == 1
    assert L.rsx_topk_rows_supported(1, 1) == 1
    for (n, k) in ((4096, 1025), (16384, 1), (16384 - 1023, 1024), (0, 1), (1, 0), (-1, 5)):
        assert L.rsx_topk_rows_supported(n, k) == 0, (n, k)
    rows = Rows(2, 8)
    sc = torch.zeros(2, 16, device="cuda")
    s, v, i, st = sc.data_ptr(), rows.val.data_ptr(), rows.idx.data_ptr(), rows.state.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    n0 = L.rsx_dbg_launch_count()
    EINVAL, EUNSUPPORTED = -1, -3
    for args in ((None, 16, 2, 16, 8, v, i, st), (s, 16, 2, 16, 8, None, i, st), (s, 16, 2, 16, 8, v, None, st),
                 (s, 16, 2, 16, 8, v, i, None), (s, 16, 0, 16, 8, v, i, st), (s, 16, -1, 16, 8, v, i, st),
                 (s, 16, 2, 0, 8, v, i, st), (s, 16, 2, 16, 0, v, i, st), (s, 15, 2, 16, 8, v, i, st)):
        assert L.rsx_topk_rows(*args, stream) == EINVAL, args
    for (n, k) in ((16, 1025), (16384, 8), (16384 - 7, 8)):
        assert L.rsx_topk_rows(s, n, 2, n, k, v, i, st, stream) == EUNSUPPORTED, (n, k)
    assert L.rsx_dbg_launch_count() == n0
    torch.cuda.synchronize()
    assert np.all(rows.val.cpu().numpy() == -7.0) and np.all(rows.state.cpu().numpy() == 0)
    _lib.check(L.rsx_topk_rows(s, 16, 2, 16, 8, v, i, st, stream), "rsx_topk_rows")
    assert L.rsx_dbg_launch_count() == n0 + 1
