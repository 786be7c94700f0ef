"""Category rules on the two-stage DIN recommendation, on the GPU: rsx_din_retrieve_candidates_rules against
`retrieve_candidates_host` with category lists, rsx_topk_lists_capped against a Python greedy walk, and
`Predictor.recommend_two_stage` / `retrieve_candidates` with rules -- device path == host path == `recommend_two_stage_host` over
the probabilities `rank_candidates` gives for the whole catalogue.  Integers compared for equality, floats by their bits."""
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
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack(ok):
    """bool [U, G] -> uint32 [U, ceil(G / 32)], bit g of row u = ok[u, g]: the layout of `category_bitmap`."""
    U, G = ok.shape
    full = np.zeros((U, 32 * ((G + 31) // 32)), bool)
    full[:, :G] = ok
    return np.packbits(full.reshape(U, -1, 32), axis=-1, bitorder="little").view(np.uint32).reshape(U, -1)


# ---- the retrieval kernel -----------------------------------------------------------------------------------------------------
def retrieval_case(N, G):
    """The inputs of one retrieval case (U = 4, P = 8, n_nbr = 4) and its allow rows: all ones, all zero, two mixed ones."""
    from recsys_amd import serving
    rng = np.random.default_rng(7000 + 10 * N + G)
    U, Pn, n = 4, 8, 4
    n_item = (7 * N) // 10 + 2
    cat_i = rng.integers(0, n_item, N).astype(np.int32)
    cat_c = rng.integers(0, G, N).astype(np.int32)
    cat_c[rng.choice(N, 6, replace=False)] = np.int32([0, G - 1, G - 1, min(31, G - 1), min(32, G - 1), 0])   # the edge bits occur
    dirty = cat_c.copy()                                               # the same catalogue with categories outside [0, G)
    out = rng.choice(N, N // 5, replace=False)
    dirty[out[::2]], dirty[out[1::2]] = -1, G
    ids, first = serving.catalogue_first_positions(cat_i)
    first_pos = np.full(n_item, -1, np.int32)
    first_pos[ids] = first
    pos = np.full((N, n), -1, np.int32)
    cnt = rng.integers(1, n + 1, N).astype(np.int32)
    for i in range(N):
        pos[i, :cnt[i]] = rng.choice(N, cnt[i], replace=False)
    hist = rng.integers(1, n_item, (U, Pn)).astype(np.int64)
    hist[:, 5] = 0
    extra = rng.integers(-2, n_item, (U, 10)).astype(np.int64)
    mine = serving.retrieve_candidates_host(pos, cnt, cat_i, hist, extra, True)[0]      # user 0 meets both kinds for certain
    dirty[mine[0]], dirty[mine[-1]] = -1, G
    ok = np.zeros((U, G), bool)
    ok[0] = True
    ok[2] = rng.random(G) < 0.5
    ok[3] = rng.random(G) < 0.8
    ok[2, G - 1], ok[3, G - 1] = True, False
    if G > 32:
        ok[2, 31], ok[2, 32], ok[3, 31], ok[3, 32] = True, False, False, True
    return dict(U=U, Pn=Pn, n=n, n_item=n_item, cat_i=cat_i, cat_c=cat_c, dirty=dirty, first_pos=first_pos, pos=pos, cnt=cnt,
                hist=hist, extra=extra, ok=ok)


def allowed_lists(ok):
    """bool [U, G] -> int64 [U, G]: the allowed categories of every row, padded with -1 (`check_category_list`'s form)."""
    out = np.full(ok.shape, -1, np.int64)
    for u, row in enumerate(ok):
        g = np.flatnonzero(row)
        out[u, :len(g)] = g
    return out


@pytest.mark.parametrize("G", [5, 32, 33, 65])
@pytest.mark.parametrize("N", [70, 501])
def test_retrieve_rules_kernel(N, G):
    from recsys_amd import _lib, serving
    L = _lib.lib()
    c = retrieval_case(N, G)
    U, Pn, n, n_item = c["U"], c["Pn"], c["n"], c["n_item"]
    first_d, pos_d, cnt_d, cat_i_d = dev(c["first_pos"]), dev(c["pos"]), dev(c["cnt"]), dev(c["cat_i"])
    hist_d = dev(c["hist"].astype(np.int32))
    full_cap = serving.candidate_capacity(N, Pn, n)
    TAIL = 16
    some_filtered = False

    for seen in (True, False):
        E = 32
        excl = np.zeros((U, E), np.int32)
        for u in range(U):
            row = np.concatenate([np.unique(c["hist"][u][c["hist"][u] > 0]) if seen else np.zeros(0, np.int64), c["extra"][u]])
            excl[u, :len(row)] = row
        excl_d = dev(excl)

        def run(cate, allow, cap, old=False):
            """-> (cand_pos, cand_item, cand_cate as [U * cap + TAIL], n_cand [U + 2]); sentinels -9 everywhere first."""
            outs = [torch.full((U * cap + TAIL,), -9, dtype=torch.int32, device="cuda") for _ in range(3)]
            ncand = torch.full((U + 2,), -9, dtype=torch.int32, device="cuda")
            cate_d = dev(cate)
            head = (ptr(hist_d), Pn, ptr(first_d), n_item, ptr(pos_d), ptr(cnt_d), n, ptr(cat_i_d), ptr(cate_d), N, ptr(excl_d), E,
                    0 if seen else 1)
            tail = (ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(ncand), cap, U, stream())
            if old:
                _lib.check(L.rsx_din_retrieve_candidates(*head, *tail), "rsx_din_retrieve_candidates")
            else:
                allow_d = None if allow is None else dev(allow)
                _lib.check(L.rsx_din_retrieve_candidates_rules(*head, ptr(allow_d), G, *tail), "rsx_din_retrieve_candidates_rules")
            torch.cuda.synchronize()
            return [x.cpu().numpy() for x in outs] + [ncand.cpu().numpy()]

        def check(got, cate, want, cap):
            gp, gi, gc, gn = got
            for x in (gp, gi, gc):
                assert (x[U * cap:] == -9).all()                       # nothing behind row U - 1
            assert (gn[U:] == -9).all()
            gp, gi, gc = (x[:U * cap].reshape(U, cap) for x in (gp, gi, gc))
            for u in range(U):
                w = want[u][:cap]                                      # a cap below the count: the lowest cap positions
                k = len(w)
                assert gn[u] == k, (N, G, seen, u, gn[u], k)
                assert np.array_equal(gp[u, :k], w) and (gp[u, k:] == -1).all()
                assert np.array_equal(gi[u, :k], c["cat_i"][w]) and (gi[u, k:] == 0).all()
                assert np.array_equal(gc[u, :k], cate[w]) and (gc[u, k:] == 0).all()

        old = run(c["cat_c"], None, full_cap, old=True)
        plain = serving.retrieve_candidates_host(c["pos"], c["cnt"], c["cat_i"], c["hist"], c["extra"], seen)
        check(old, c["cat_c"], plain, full_cap)
        # allow == NULL and all ones: the old entry, bit for bit
        for allow in (None, pack(np.ones((U, G), bool))):
            got = run(c["cat_c"], allow, full_cap)
            assert all(np.array_equal(a, b) for a, b in zip(got, old)), (N, G, seen, allow is None)
        # rows of all ones, all zero and mixed; then the same over categories -1 and G, which are left out
        for cate in (c["cat_c"], c["dirty"]):
            want = serving.retrieve_candidates_host(c["pos"], c["cnt"], c["cat_i"], c["hist"], c["extra"], seen, cat_cate=cate,
                                                    categories=allowed_lists(c["ok"]))
            assert len(want[1]) == 0 and len(plain[1]) > 0             # the all-zero row: n_cand == 0, padding only
            for u in (2, 3):
                some_filtered |= 0 < len(want[u]) < len(plain[u])
            if cate is c["dirty"]:
                assert len(want[0]) < len(plain[0]) and not np.isin(cate[want[0]], [-1, G]).any()
            else:
                assert np.array_equal(want[0], plain[0])
            check(run(cate, pack(c["ok"]), full_cap), cate, want, full_cap)
            small = max(1, min(len(want[0]), len(want[3])) // 2)       # below the count of rows 0 and 3
            assert small < len(want[0])
            check(run(cate, pack(c["ok"]), small), cate, want, small)
    assert some_filtered                                               # a filter that removes some, not all, of a user's candidates


# ---- the capped selection -----------------------------------------------------------------------------------------------------
def greedy(values, index, cates, G, m, k):
    """The live entries (score, absolute index, category) -> (values, indices) of the capped list: rsx_topk_rows' order, an
    entry kept unless m kept entries of its category precede it, k at most; a category outside [0, G) leaves first."""
    inside = (cates >= 0) & (cates < G)
    values, index, cates = values[inside], index[inside], cates[inside]
    taken, keep = {}, []
    for i in np.lexsort((index, -values)):
        g = int(cates[i])
        if taken.get(g, 0) < m:
            taken[g] = taken.get(g, 0) + 1
            keep.append(i)
            if len(keep) == k:
                break
    keep = np.asarray(keep, np.int64)
    return values[keep], index[keep].astype(np.int32)


def capped_case(n, k, m, G, one_category=False):
    """Two chunks of scores [U, ld] and one cate row per user [U, 2 n + 3] (U = 4), and the live counts of both feeds."""
    rng = np.random.default_rng(100000 + 1000 * n + 7 * k + 31 * m + G)
    U, ld, ldc = 4, n + 5, 2 * n + 3
    valid = [[0, 1, n // 2, n], [n // 2, n, 0, 1]]
    sc = [np.full((U, ld), np.nan, np.float32) for _ in range(2)]
    cate = np.where(rng.random((U, ldc)) < 0.5, -5, G + 9).astype(np.int32)    # beyond the counts: categories never read
    for c in range(2):
        for u in range(U):
            nv = valid[c][u]
            s = np.round(rng.uniform(0, 1, nv), 2).astype(np.float32)          # two decimals: ties
            s[rng.random(nv) < 0.01] = np.nan
            sc[c][u, :nv] = s
            g = np.zeros(nv, np.int32) if one_category else rng.integers(0, G, nv).astype(np.int32)
            if G > 1 and not one_category:
                bad = rng.random(nv) < 0.02                                    # live entries outside [0, G): left out
                g[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, G)
            cate[u, c * n:c * n + nv] = g
    return U, ld, ldc, valid, sc, cate


def capped_expected(n, k, m, G, case, chunks):
    U, ld, ldc, valid, sc, cate = case
    out = []
    for u in range(U):
        v = np.concatenate([sc[c][u, :valid[c][u]] for c in range(chunks)])
        ix = np.concatenate([np.arange(c * n, c * n + valid[c][u]) for c in range(chunks)])
        out.append(greedy(v, ix, cate[u, ix], G, m, k) + (greedy(v, ix, cate[u, ix], G, len(v) + 1, k),))
    return out


@pytest.mark.parametrize("G", [1, 7, 802])
@pytest.mark.parametrize("m", [1, 2, 16])
@pytest.mark.parametrize("n,k", [(64, 1), (300, 10), (900, 100), (1000, 100)])
def test_topk_lists_capped(n, k, m, G):
    """(900, 100) runs 256 threads, (1000, 100) runs 1024.  One request fed in one call, and in two with a running list."""
    from recsys_amd import _lib
    L = _lib.lib()
    assert L.rsx_topk_rows_threads(900, 100) == 256 and L.rsx_topk_rows_threads(1000, 100) == 1024
    assert L.rsx_topk_lists_capped_supported(n, k, G, m) == 1

    def run(case, chunks, cap, counted=False):
        U, ld, ldc, valid, sc, cate = case
        val = torch.full((U, k), -3.0, dtype=torch.float32, device="cuda")
        idx = torch.full((U, k), -3, dtype=torch.int32, device="cuda")
        state = torch.zeros((U, 2), dtype=torch.int32, device="cuda")
        cate_d = dev(cate)
        for c in range(chunks):
            sc_d, nv_d = dev(sc[c]), dev(np.int32(valid[c]))
            if counted:
                _lib.check(L.rsx_topk_rows_counted(ptr(sc_d), ld, ptr(nv_d), U, n, k, ptr(val), ptr(idx), ptr(state), stream()),
                           "rsx_topk_rows_counted")
            else:
                _lib.check(L.rsx_topk_lists_capped(ptr(sc_d), ld, ptr(nv_d), ptr(cate_d) if cap else None, ldc, G, cap, U, n, k,
                                                   ptr(val), ptr(idx), ptr(state), stream()), "rsx_topk_lists_capped")
        torch.cuda.synchronize()
        return val.cpu().numpy(), idx.cpu().numpy(), state.cpu().numpy()

    case = capped_case(n, k, m, G)
    U = case[0]
    dropped = short = tie = False
    for chunks in (1, 2):
        # m == 0: rsx_topk_rows_counted, bit for bit -- outputs (the unwritten slots included) and state
        a, b = run(case, chunks, 0), run(case, chunks, 0, counted=True)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        val, idx, state = run(case, chunks, m)
        for u, (ev, ei, (fv, fi)) in enumerate(capped_expected(n, k, m, G, case, chunks)):
            f = len(ei)
            assert state[u].tolist() == [f, n * chunks], (chunks, u, state[u], f)
            assert np.array_equal(idx[u, :f], ei) and np.array_equal(bits(val[u, :f]), bits(ev)), (chunks, u)
            dropped |= bool(set(fi.tolist()) - set(ei.tolist()))
            short |= len(fi) == k and f < k
            tie |= bool(np.any((ev[1:] == ev[:-1]) & (ei[1:] > ei[:-1])))
    # what keeps the comparison from passing vacuously, from the inputs alone
    if G * m < k:                                                      # (pigeonhole: a full uncapped list must lose entries)
        assert dropped and short, (n, k, m, G)
    if (n, k, m, G) in ((900, 100, 16, 7), (1000, 100, 16, 802), (1000, 100, 2, 802)):
        assert tie                                                     # equal scores inside a kept list, the lower index first
    if (k, m, G) == (100, 1, 802):
        assert dropped                                                 # 802 categories: the cap still drops from the top 100

    # all entries in one category: filled == min(m, n_valid, k)
    one = capped_case(n, k, m, G, one_category=True)
    val, idx, state = run(one, 1, m)
    want = capped_expected(n, k, m, G, one, 1)
    for u in range(U):
        nv = one[3][0][u]
        assert state[u, 0] == min(m, nv, k) == len(want[u][1])
        assert np.array_equal(idx[u, :state[u, 0]], want[u][1])


# ---- Predictor end to end ----------------------------------------------------------------------------------------------------
def shuffled_catalogue(N, seed):
    """N entries in a shuffled order: items 0 .. N - 4 (the padding id 0 is an entry) and items 5, 9, 17 a second time; every
    category of [0, N_CATE) occurs, 0 included."""
    rng = np.random.default_rng(seed)
    items = np.concatenate([np.arange(N - 3), [5, 9, 17]]).astype(np.int64)
    cates = (items * 7 + items // 19) % N_CATE
    order = rng.permutation(N)
    return items[order], cates[order]


def load(tmp_path_factory, K, max_c):
    from recsys_amd import serving
    d, _ = din_bundle(tmp_path_factory, K, 30, N_ITEM, N_CATE)
    return serving.Predictor.load(d, max_batch_size=64, max_candidates=max_c)


def same(got, want):
    assert sorted(got) == ["count", "index", "item", "prob"]
    assert got["prob"].dtype == np.float32 and got["item"].dtype == np.int32 and got["index"].dtype == np.int32
    assert got["prob"].shape == want["prob"].shape, (got["prob"].shape, want["prob"].shape)
    assert np.array_equal(np.asarray(got["count"]), np.asarray(want["count"])), (got["count"], want["count"])
    assert np.array_equal(got["index"], want["index"]) and np.array_equal(got["item"], want["item"])
    assert np.array_equal(bits(got["prob"]), bits(want["prob"]))


@pytest.mark.parametrize("U,K", [(1, 32), (3, 16)])
def test_recommend_two_stage_with_rules(tmp_path_factory, U, K):
    """Device == host path (rules_on_device = False) == recommend_two_stage_host over rank_candidates' whole-catalogue
    probabilities.  Per rule set: request A three times (eager, captured, replayed), then request B of the same shape."""
    from recsys_amd import serving
    N = 500
    ci, cc = shuffled_catalogue(N, 5 + U)
    p, ph = load(tmp_path_factory, K, 512), load(tmp_path_factory, K, 512)
    ph.rules_on_device = False
    for q in (p, ph):
        q.set_catalogue(ci, cc)
        q.build_neighbours(32)
    pos, _, cnt = p._nbr["host"]
    rng = np.random.default_rng(40 + U)
    allow = np.full((U, 9), -1, np.int64)
    deny = np.full((U, 5), -1, np.int64)
    for u in range(U):
        allow[u, [0, 2, 3, 5, 6, 8]] = rng.choice(N_CATE, 6, replace=False)      # padded lists: -1 between the ids
        deny[u, [1, 3]] = rng.choice(N_CATE, 2, replace=False)
    allow[0, 0] = 0                                                    # 0 is a real category
    rule_sets = [dict(categories=allow), dict(exclude_categories=deny), dict(max_per_category=1), dict(max_per_category=2),
                 dict(categories=allow, exclude_categories=deny, max_per_category=2),
                 dict(exclude_categories=deny, max_per_category=1, exclude_seen=False),
                 dict(categories=np.zeros((U, 0), np.int64), max_per_category=1)]
    specials = [["full", "hole", "full"][:U], ["hole", "full", "empty"][:U]]
    requests = []
    for sp in specials:
        hi, hc, _, _ = make_request(rng, U, 1, 30, sp, N_ITEM, N_CATE)
        prob = p.rank_candidates(hi, hc, np.tile(ci, (U, 1)), np.tile(cc, (U, 1)))["prob"]
        requests.append((hi, hc, rng.integers(-1, N_ITEM, (U, 9)), prob))
    assert p.two_stage_path_for(50, 30, 2, rules=True) == "device" and ph.two_stage_path_for(50, 30, 2, rules=True) == "host"
    assert p.two_stage_path_for(50, 30, 17) == "host" and p.two_stage_path_for(50, 30) == "device" == ph.two_stage_path_for(50, 30)
    dropped = short = filtered = False
    for k in (5, 50):
        for rules in rule_sets:
            rules = dict(rules)
            seen = rules.pop("exclude_seen", True)
            filters = {key: v for key, v in rules.items() if key != "max_per_category"}
            for a, (hi, hc, exclude, prob) in enumerate([requests[0]] * 3 + [requests[1]]):
                want = serving.recommend_two_stage_host(prob, pos, cnt, ci, hi, exclude, k, seen, cat_cate=cc, n_cate=N_CATE, **rules)
                got = p.recommend_two_stage(hi, hc, k, exclude_seen=seen, exclude=exclude, **rules)
                assert p.two_stage_path == "device"
                same(got, want)
                if a in (0, 3):
                    slow = ph.recommend_two_stage(hi, hc, k, exclude_seen=seen, exclude=exclude, **rules)
                    assert ph.two_stage_path == "host"
                    same(slow, want)
                    free = serving.recommend_two_stage_host(prob, pos, cnt, ci, hi, exclude, k, seen)
                    plain = serving.retrieve_candidates_host(pos, cnt, ci, hi, exclude, seen)
                    ref = serving.retrieve_candidates_host(pos, cnt, ci, hi, exclude, seen, cat_cate=cc, n_cate=N_CATE, **filters)
                    for q in (p, ph) if filters else ():
                        cand = q.retrieve_candidates(hi, hc, exclude_seen=seen, exclude=exclude, **filters)
                        assert cand["index"].shape == (U, 512) and cand["count"].tolist() == [len(x) for x in ref]
                        for u in range(U):
                            assert np.array_equal(cand["index"][u, :len(ref[u])], ref[u]) and (cand["index"][u, len(ref[u]):] == -1).all()
                    for u in range(U):
                        c, fc = int(want["count"][u]), int(free["count"][u])
                        filtered |= 0 < len(ref[u]) < len(plain[u])
                        if "max_per_category" in rules and not filters:
                            dropped |= bool(set(free["index"][u, :fc].tolist()) - set(want["index"][u, :c].tolist()))
                            short |= fc == k and c < k
                    if "categories" in rules and rules["categories"].shape[1] == 0:
                        assert want["count"].tolist() == [0] * U      # an empty allow list
                if U == 1 and a == 0:                                  # the one-user form: 1-D in, arrays cut to count
                    one = p.recommend_two_stage(hi[0], hc[0], k, exclude_seen=seen, exclude=exclude[0],
                                                **{key: (v[0] if key != "max_per_category" else v) for key, v in rules.items()})
                    c = int(want["count"][0])
                    assert isinstance(one["count"], int) and one["count"] == c and one["item"].shape == (c,)
                    assert np.array_equal(one["index"], want["index"][0, :c]) and np.array_equal(bits(one["prob"]), bits(want["prob"][0, :c]))
            how = (bool(filters), rules.get("max_per_category", 0))
            assert "graph" in p._graphs[("two_stage", U, k, 64 if seen else 32, 512, not seen) + how]
    assert p._n_graphs < p.MAX_GRAPHS                                  # (no shape above ran eagerly for want of a slot)
    # 19 or 20 categories, k = 50: a full uncapped list must lose entries under m <= 2, and 2 * 20 < 50 keeps the list short
    assert dropped and short and filtered
    # a request without a rule: what recommend_two_stage returns without the new arguments, through today's graph key
    hi, hc, exclude, prob = requests[0]
    for _ in range(3):
        a = p.recommend_two_stage(hi, hc, 50, exclude_seen=True, exclude=exclude)
        b = p.recommend_two_stage(hi, hc, 50, True, exclude, None, None, None)
        same(a, b)
        same(a, serving.recommend_two_stage_host(prob, pos, cnt, ci, hi, exclude, 50))
    assert "graph" in p._graphs[("two_stage", U, 50, 64, 512, False)]
    # the switch: rules_on_device = False sends the same request to the host path, with the same bits
    p.rules_on_device = False
    got = p.recommend_two_stage(hi, hc, 50, exclude=exclude, exclude_categories=deny, max_per_category=2)
    assert p.two_stage_path == "host"
    same(got, serving.recommend_two_stage_host(prob, pos, cnt, ci, hi, exclude, 50, cat_cate=cc, n_cate=N_CATE,
                                               exclude_categories=deny, max_per_category=2))
    assert p.recommend_two_stage(hi, hc, 50, exclude=exclude)["count"].tolist() == a["count"].tolist() and p.two_stage_path == "device"
