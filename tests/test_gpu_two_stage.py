"""Two-stage DIN recommendation on the GPU: rsx_rows_dot, rsx_topk_rows_counted and rsx_din_retrieve_candidates against their
numpy definitions in recsys_amd/serving_din.py -- bit for bit (uint32 views of the floats, equality of the integers) -- and
`Predictor.build_neighbours` / `similar_items` / `retrieve_candidates` / `recommend_two_stage` against `item_neighbours_host`
and `recommend_two_stage_host` over the probabilities `rank_candidates` gives for the whole catalogue.
Embeddings are drawn from a normal distribution and some rows zeroed: every non-zero component of a unit row is far above
2^-60, so no product is subnormal."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_din_rank import bits, din_bundle, make_request

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_ITEM, N_CATE = 501, 20


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def unit_rows(rng, N, K):
    from recsys_amd import serving
    e = rng.standard_normal((N, K)).astype(np.float32)
    e[rng.choice(N, max(1, N // 10), replace=False)] = 0
    return serving.unit_rows_host(e)


@pytest.mark.parametrize("K", [16, 32])
def test_rows_dot_equals_its_restatement(K):
    from recsys_amd import _lib, serving
    L = _lib.lib()
    rng = np.random.default_rng(300 + K)
    N, first = 400, 7
    unit = unit_rows(rng, N, K)
    unit_d = dev(unit)
    for Q in (1, 63, 65):
        q = rng.integers(0, N, Q).astype(np.int32)
        q_d = dev(q)
        for n in (1, 63, 64, 65, 257):
            ld = n + 3
            out = torch.full((Q, ld), -7.0, dtype=torch.float32, device="cuda")
            _lib.check(L.rsx_rows_dot(ptr(unit_d), N, K, ptr(q_d), Q, first, n, ptr(out), ld, stream()), "rsx_rows_dot")
            got = out.cpu().numpy()
            want = serving.rows_dot_host(unit, q, first, n)
            assert np.array_equal(bits(got[:, :n]), bits(want)), (K, Q, n)
            assert (got[:, n:] == -7.0).all()                          # the padding of a row is never written


def _scores(rng, U, n):
    s = np.round(rng.uniform(0, 1, (U, n)), 2).astype(np.float32)     # two decimals: plenty of ties
    s[rng.random((U, n)) < 0.01] = np.nan
    return s


def _expected_list(pairs, k):
    """pairs: (score [m], absolute index [m]) of the valid entries -> the first k in rsx_topk_rows' order."""
    v, ix = pairs
    order = np.lexsort((ix, -v))[:k]
    return v[order], ix[order]


@pytest.mark.parametrize("n,k", [(300, 1), (300, 100), (900, 100), (1000, 100), (1023, 1), (1024, 1)])
def test_topk_rows_counted(n, k):
    """n + k on both sides of 1024, the thread-count switch: (900, 100) and (1023, 1) run 256 threads, the others 1024."""
    from recsys_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n + k)
    U, ld = 4, n + 5
    sc = [np.full((U, ld), 9.0, np.float32) for _ in range(2)]
    for s in sc:
        s[:, :n] = _scores(rng, U, n)
    sc_d = [dev(s) for s in sc]

    def run(fn, valid):
        """One request of len(valid) chunks -> (out_val, out_idx, state) as numpy."""
        val = torch.full((U, k), -3.0, dtype=torch.float32, device="cuda")
        idx = torch.full((U, k), -3, dtype=torch.int32, device="cuda")
        state = torch.zeros((U, 2), dtype=torch.int32, device="cuda")
        for c, nv in enumerate(valid):
            if nv is None:
                _lib.check(L.rsx_topk_rows(ptr(sc_d[c]), ld, U, n, k, ptr(val), ptr(idx), ptr(state), stream()), "rsx_topk_rows")
            else:
                nv_d = dev(np.int32(nv))
                _lib.check(fn(ptr(sc_d[c]), ld, ptr(nv_d), U, n, k, ptr(val), ptr(idx), ptr(state), stream()), "counted")
        return val.cpu().numpy(), idx.cpu().numpy(), state.cpu().numpy()

    # every score valid: rsx_topk_rows, bit for bit -- outputs and state, one chunk and two
    full = [n, n + 5, 2 ** 30, n]
    for chunks in (1, 2):
        a = run(L.rsx_topk_rows_counted, [full] * chunks)
        b = run(None, [None] * chunks)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # mixed counts per row, one chunk and two chunks with a running list; a negative count is clamped to 0
    for valid in ([[0, 1, n - 1, n]], [[n - 1, 0, 1, n], [1, 0, n, n - 1]], [[0, 0, -4, 1], [0, 2, 0, n]]):
        val, idx, state = run(L.rsx_topk_rows_counted, valid)
        for u in range(U):
            vs, ixs = [], []
            for c, nv in enumerate(valid):
                m = max(0, min(n, nv[u]))
                vs.append(sc[c][u, :m])
                ixs.append(np.arange(c * n, c * n + m))
            ev, ei = _expected_list((np.concatenate(vs), np.concatenate(ixs)), k)
            f = len(ev)
            assert state[u].tolist() == [f, n * len(valid)], (valid, u, state[u])
            assert np.array_equal(idx[u, :f], ei) and np.array_equal(bits(val[u, :f]), bits(ev)), (valid, u)


def _neighbour_table(rng, N, n):
    """A random table in `item_neighbours_host`'s format: the kernel and its definition take any."""
    pos = np.full((N, n), -1, np.int32)
    cnt = rng.integers(0, min(n, N) + 1, N).astype(np.int32)
    for i in range(N):
        pos[i, :cnt[i]] = rng.choice(N, cnt[i], replace=False)
    return pos, cnt


@pytest.mark.parametrize("N", [1, 31, 32, 33, 1000])
def test_retrieve_candidates_kernel(N):
    from recsys_amd import _lib, serving
    L = _lib.lib()
    rng = np.random.default_rng(900 + N)
    n_item = max(3, (7 * N) // 10 + 2)                                # fewer ids than positions: duplicates; id 0 occurs
    cat_i = rng.integers(0, n_item, N).astype(np.int32)
    cat_c = rng.integers(0, 9, N).astype(np.int32)
    ids, first = serving.catalogue_first_positions(cat_i)
    first_pos = np.full(n_item, -1, np.int32)
    first_pos[ids] = first
    cat_i_d, cat_c_d, first_d = dev(cat_i), dev(cat_c), dev(first_pos)
    for n in (1, 32, 64):
        pos, cnt = _neighbour_table(rng, N, n)
        pos_d, cnt_d = dev(pos), dev(cnt)
        for Pn in (1, 100, 128):
            cap = serving.candidate_capacity(N, Pn, n)
            for U in (1, 3):
                for E in (0, 32, 256):
                    for seen in (True, False):                         # exclude_seen; the kernel's include_seeds is `not seen`
                        # with exclude_seen the list must hold the history: few enough distinct ids to fit E (none at E = 0)
                        pool = {0: 0, 32: 20, 256: 128}[E] if seen else 200
                        hist = np.zeros((U, Pn), np.int64)
                        if pool:
                            hist = rng.choice(rng.integers(0, n_item, pool), (U, Pn))
                        if U == 3:
                            hist[1] = 0                                # a user with no seed
                        extra = rng.integers(-2, n_item, (U, {0: 0, 32: 12, 256: 120}[E]))
                        excl = np.zeros((U, E), np.int32)
                        for u in range(U):
                            row = np.concatenate([np.unique(hist[u][hist[u] > 0]) if seen else np.zeros(0, np.int64), extra[u]])
                            excl[u, :len(row)] = row
                        out = [torch.full((U, cap), -9, dtype=torch.int32, device="cuda") for _ in range(3)]
                        ncand = torch.full((U,), -9, dtype=torch.int32, device="cuda")
                        hist_d, excl_d = dev(hist.astype(np.int32)), dev(excl)
                        _lib.check(L.rsx_din_retrieve_candidates(ptr(hist_d), Pn, ptr(first_d), n_item, ptr(pos_d), ptr(cnt_d), n,
                                                                 ptr(cat_i_d), ptr(cat_c_d), N, ptr(excl_d) if E else None, E,
                                                                 0 if seen else 1, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                                                 ptr(ncand), cap, U, stream()), "rsx_din_retrieve_candidates")
                        got_p, got_i, got_c = (x.cpu().numpy() for x in out)
                        got_n = ncand.cpu().numpy()
                        want = serving.retrieve_candidates_host(pos, cnt, cat_i, hist, extra if E else None, seen)
                        for u in range(U):
                            w, c = want[u], len(want[u])
                            where = (N, n, Pn, U, E, seen, u)
                            assert got_n[u] == c, where
                            assert np.array_equal(got_p[u, :c], w) and (got_p[u, c:] == -1).all(), where
                            assert np.array_equal(got_i[u, :c], cat_i[w]) and (got_i[u, c:] == 0).all(), where
                            assert np.array_equal(got_c[u, :c], cat_c[w]) and (got_c[u, c:] == 0).all(), where


def catalogue(N):
    """N entries over items 0 .. N - 2: item 0 (the padding id) is an entry, and item 5 is there twice."""
    items = np.concatenate([np.arange(N - 1), [5]]).astype(np.int64)
    return items, (items * 7) % (N_CATE - 1) + 1


def load(tmp_path_factory, K, max_c, graph=True):
    """A Predictor over the 501-item bundle with a tenth of the item embedding rows zeroed (consistently: the rank kernel
    reads the same table)."""
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, K, 30, N_ITEM, N_CATE)
    p = serving.Predictor.load(d, max_batch_size=64, max_candidates=max_c, use_hip_graph=graph)
    with torch.no_grad():
        p._est.store.embeddings["i_id"].table[torch.arange(3, N_ITEM, 10, device="cuda")] = 0
    return p


def same_table(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)


@pytest.mark.parametrize("K", [16, 32])
def test_build_neighbours_equals_its_definition(tmp_path_factory, K):
    """N = 300 with max_candidates = 128: three chunks and three query blocks.  N = 20 with n = 32 >= N - 1: short rows."""
    from recsys_amd import _lib, serving
    p = load(tmp_path_factory, K, 128)
    emb = p._est.store.embeddings["i_id"].table.detach().cpu().numpy()[:, :K]
    assert p.neighbours_path is None and p.neighbours_buffer_bytes() == 0
    for N, n in ((300, 32), (300, 64), (20, 32)):
        ci, cc = catalogue(N)
        p.set_catalogue(ci, cc)
        with pytest.raises(_lib.RsxError, match="build_neighbours"):
            p.similar_items(ci[:2], 1)
        p.build_neighbours(n)
        assert p.neighbours_path == "device"
        assert p.neighbours_buffer_bytes() == N * n * 8 + N * 4 + 4 * N_ITEM
        want = serving.item_neighbours_host(serving.unit_rows_host(emb[ci]), ci, n)
        same_table(p._nbr["host"], want)
        same_table([x.cpu().numpy() for x in p._nbr["dev"]], want)
        assert want[2][0] == 0 and want[2][1:].min() > 0              # item 0's row is empty; nobody else's
        if N == 20:
            assert want[2].max() == N - 1 and want[2][5] == N - 2    # short rows; item 5 loses its duplicate too
        # similar_items: rows of the table for the lowest position of each id
        q = np.int64([5, 0, 7, N + 50, 1])
        got = p.similar_items(q, min(n, 10))
        kk = min(n, 10)
        assert got["index"].shape == (5, kk) and got["count"].tolist()[1] == 0 and got["count"].tolist()[3] == 0
        for r, i in ((0, 5), (2, 7), (4, 1)):                          # (id i sits at position i first)
            c = min(kk, want[2][i])
            assert got["count"][r] == c and np.array_equal(got["index"][r, :c], want[0][i, :c])
            assert np.array_equal(bits(got["sim"][r, :c]), bits(want[1][i, :c])) and np.array_equal(got["item"][r, :c], ci[want[0][i, :c]])
        assert (got["index"][[1, 3]] == -1).all() and np.isnan(got["sim"][[1, 3]]).all() and (got["item"][[1, 3]] == -1).all()
        with pytest.raises(_lib.RsxError):
            p.similar_items(q, n + 1)


def same(got, want):
    assert sorted(got) == ["count", "index", "item", "prob"]
    assert got["prob"].dtype == np.float32 and got["item"].dtype == np.int32 and got["index"].dtype == np.int32
    assert got["prob"].shape == want["prob"].shape, (got["prob"].shape, want["prob"].shape)
    assert np.array_equal(np.asarray(got["count"]), np.asarray(want["count"])), (got["count"], want["count"])
    assert np.array_equal(got["index"], want["index"]) and np.array_equal(got["item"], want["item"])
    assert np.array_equal(bits(got["prob"]), bits(want["prob"]))


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("K", [16, 32])
def test_recommend_two_stage_equals_its_definition(tmp_path_factory, K, graph):
    """The device path == the host path == recommend_two_stage_host over rank_candidates(whole catalogue), at N = 500.  Three
    requests per shape: with graphs the first runs eagerly, the second captures and replays, the third replays over other
    histories."""
    from recsys_amd import _lib, serving
    N = 500
    ci, cc = catalogue(N)
    p = load(tmp_path_factory, K, 512, graph)                          # cap = 512 fits one rank launch: the device path
    ph = load(tmp_path_factory, K, 100, graph)                         # cap > max_candidates: the host path
    for q in (p, ph):
        q.set_catalogue(ci, cc)
        with pytest.raises(_lib.RsxError, match="build_neighbours"):
            q.recommend_two_stage(np.int64([1, 2]), np.int64([1, 2]), 3)
    rng = np.random.default_rng(17 + K)
    hi, hc, _, _ = make_request(rng, 3, 1, 30, ["hole", "empty", "full"], N_ITEM, N_CATE)
    before = p.recommend(hi, hc, 10)
    for q in (p, ph):
        q.build_neighbours(32)
        assert q.neighbours_path == "device" and q.two_stage_path is None
    same_table(p._nbr["host"], ph._nbr["host"])                        # one chunk and five chunks: the same table
    after = p.recommend(hi, hc, 10)
    same(after, before)                                                # `recommend` is untouched by the table
    assert p.two_stage_path_for(10) == "device" and ph.two_stage_path_for(10) == "host" and p.two_stage_path_for(1025) == "host"
    pos, _, cnt = p._nbr["host"]
    for U, k, seen in [(U, k, seen) for U in (1, 3) for k in (1, 10, 1024) for seen in (True, False)]:
        for rep in range(3):                                       # one graph key: the same shapes, other histories and ids
            hi, hc, _, _ = make_request(rng, U, 1, 30, ["full", "empty", "hole"][:U] if rep != 1 else ["hole", "full", None][:U],
                                        N_ITEM, N_CATE)
            exclude = rng.integers(-1, N_ITEM, (U, 9))
            prob = p.rank_candidates(hi, hc, np.tile(ci, (U, 1)), np.tile(cc, (U, 1)))["prob"]
            want = serving.recommend_two_stage_host(prob, pos, cnt, ci, hi, exclude, k, seen)
            got = p.recommend_two_stage(hi, hc, k, exclude_seen=seen, exclude=exclude)
            assert p.two_stage_path == "device"
            same(got, want)
            assert got["prob"].shape == (U, min(k, N))
            cand = p.retrieve_candidates(hi, hc, exclude_seen=seen, exclude=exclude)
            ref = serving.retrieve_candidates_host(pos, cnt, ci, hi, exclude, seen)
            assert cand["index"].shape == (U, 512) and cand["count"].tolist() == [len(x) for x in ref]
            for u in range(U):
                assert np.array_equal(cand["index"][u, :len(ref[u])], ref[u]) and (cand["index"][u, len(ref[u]):] == -1).all()
                assert want["count"][u] == min(k, len(ref[u]))
            if rep == 0:
                slow = ph.recommend_two_stage(hi, hc, k, exclude_seen=seen, exclude=exclude)
                assert ph.two_stage_path == "host"
                same(slow, want)
                hc_ = ph.retrieve_candidates(hi, hc, exclude_seen=seen, exclude=exclude)
                assert np.array_equal(hc_["index"], cand["index"]) and np.array_equal(hc_["count"], cand["count"])
            if U == 1:                                             # the one-user form: 1-D in, arrays cut to count
                one = p.recommend_two_stage(hi[0], hc[0], k, exclude_seen=seen, exclude=None if exclude is None else exclude[0])
                c = int(want["count"][0])
                assert isinstance(one["count"], int) and one["count"] == c and one["item"].shape == (c,)
                assert np.array_equal(one["index"], want["index"][0, :c]) and np.array_equal(bits(one["prob"]), bits(want["prob"][0, :c]))
        if graph:                                                  # the second request captured the shape, the third replayed
            assert "graph" in p._graphs[("two_stage", U, k, 64 if seen else 32, 512, not seen)]
            assert "graph" in p._graphs[("two_stage", U, 0, 64 if seen else 32, 512, not seen)]
    assert not graph or p._n_graphs < p.MAX_GRAPHS                     # (no shape above ran eagerly for want of a slot)
    # without `exclude`
    prob = p.rank_candidates(hi, hc, np.tile(ci, (3, 1)), np.tile(cc, (3, 1)))["prob"]
    same(p.recommend_two_stage(hi, hc, 10), serving.recommend_two_stage_host(prob, pos, cnt, ci, hi, None, 10))
    # more than 256 distinct exclusion ids: the host path, the same bits
    hi, hc, _, _ = make_request(rng, 1, 1, 30, ["full"], N_ITEM, N_CATE)
    many = np.arange(200, 200 + 260)[None, :]
    prob = p.rank_candidates(hi, hc, ci[None, :], cc[None, :])["prob"]
    got = p.recommend_two_stage(hi, hc, 10, exclude=many)
    assert p.two_stage_path == "host"
    same(got, serving.recommend_two_stage_host(prob, pos, cnt, ci, hi, many, 10))
    # a replaced catalogue drops the table: refused until it is rebuilt
    p.set_catalogue(ci[:400], cc[:400])
    assert p.neighbours_path is None and p.neighbours_buffer_bytes() == 0
    with pytest.raises(_lib.RsxError, match="build_neighbours"):
        p.recommend_two_stage(hi, hc, 10)
    p.build_neighbours(16)
    prob = p.rank_candidates(hi, hc, ci[None, :400], cc[None, :400])["prob"]
    pos, _, cnt = p._nbr["host"]
    got = p.recommend_two_stage(hi, hc, 10)
    assert p.two_stage_path == "device"
    same(got, serving.recommend_two_stage_host(prob, pos, cnt, ci[:400], hi, None, 10))
