"""Item ranking of uid_iid deepfm.py bundles on the GPU: rsx_predict_pair_rank (csrc/predict_pair.hip) against the oracle's
inference forward through the C ABI, a pair's bits independent of its company, 16-bit tables, `Predictor.rank_items` against
`predict` on the expansion, launches per request, the device top-k and `recommend_items` against their numpy definitions, the
`layers` fallback outside the envelope, and deepfm.py's own train -> export -> rank chain.

The checker is nn.sigmoid(models.DeepFM(P, row_off, L, 0.0).forward(ids, train=False)) on weights that make the
probabilities SPREAD (tests/pair_util.py::pair_params: noise on gamma / beta / every bias, tables x 4, w1 += 0.3 N(0, 1),
|out.W[0]| + 0.5).  On that recipe, at (U, C) = (3, 37), the probabilities have std 0.21 / 0.31 / 0.16 for D = 32 / 16 / 8 and
every mistake this file exists for (a dropped first-order term, a neighbour's user row, a dropped FM term or tower) moves some
probability by at least 1e-3, a hundred times the 1e-5 bar; the spread is asserted (std >= 0.05) on that case of every D."""
import ctypes as C

import numpy as np
import pytest

from tests.pair_util import ROW_OFF, ROWS, draw_pairs, oracle_pair_prob, pair_columns, pair_params

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODELS = [(32, (200, 200, 200)), (16, (64, 32)), (8, (32, 18)), (16, (100,))]
SHAPES = [(1, 1), (1, 17), (3, 37), (2, 200)]
_BUNDLES = {}
bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)


def device_pair_model(P, D, layers, tables=None, table_dtype=0):
    """-> (rsx_predict_model over device copies of the oracle's parameters, the tensors that keep them alive).  tables: the
    table in its stored form (fp32, float16, or bfloat16 bit patterns as uint16) when it is not P's."""
    from recsys_amd import _lib
    t = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1)).cuda() for k, v in P.items() if k != "tables"}
    tab = P["tables"] if tables is None else tables
    t["tables"] = torch.from_numpy(np.ascontiguousarray(tab.view(np.int16) if tab.dtype == np.uint16 else tab)).cuda()
    t["row_off"] = torch.from_numpy(np.asarray(ROW_OFF[:-1], np.int32)).cuda()
    m = _lib.PredictModel()
    m.tables, m.w1, m.row_off = t["tables"].data_ptr(), t["w1"].data_ptr(), t["row_off"].data_ptr()
    for l, n in enumerate(layers):
        m.W[l], m.b[l] = t["dnn.W%d" % l].data_ptr(), t["dnn.b%d" % l].data_ptr()
        m.gamma[l], m.beta[l] = t["dnn.gamma%d" % l].data_ptr(), t["dnn.beta%d" % l].data_ptr()
        m.widths[l] = n
    m.wd, m.bd = t["dnn.Wout"].data_ptr(), t["dnn.bout"].data_ptr()
    m.c0, m.wo, m.bo = t["b1"].data_ptr(), t["out.W"].data_ptr(), t["out.b"].data_ptr()
    m.w1_field_mask, m.bn_eps, m.F, m.D, m.L, m.table_dtype = 3, 1e-3, 2, D, len(layers), table_dtype
    return m, t


def launch(m, user, items, user_slot=1, ld=None, guard=64):
    """user [U], items [Cn] (shared, item_ld = 0) or [U, Cn]; ld > Cn pads every row with VALID other ids (a kernel that read
    the padding would give wrong probabilities, not a fault) -> prob [U, Cn]; the guard behind prob must keep its bits."""
    from recsys_amd import _lib
    U, Cn = len(user), items.shape[-1]
    if items.ndim == 1:
        buf, item_ld = items, 0
    else:
        item_ld = Cn if ld is None else ld
        buf = np.empty((U, item_ld), np.int32)
        buf[:, :Cn] = items
        buf[:, Cn:] = (items[:, :1] + 7) % ROWS[1 - user_slot]
    d_u, d_i = torch.from_numpy(np.ascontiguousarray(user, np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    out = torch.full((U * Cn + guard,), -7.0, device="cuda")
    _lib.check(_lib.lib().rsx_predict_pair_rank(C.byref(m), user_slot, d_u.data_ptr(), d_i.data_ptr(), item_ld, out.data_ptr(), U, Cn,
                                                torch.cuda.current_stream().cuda_stream), "rsx_predict_pair_rank")
    got = out.cpu().numpy()
    assert np.all(got[U * Cn:] == -7.0), "the kernel wrote past prob[U * C]"
    return got[:U * Cn].reshape(U, Cn)


@pytest.mark.parametrize("D,layers", MODELS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_against_the_oracle_through_the_c_abi(D, layers):
    """1: max |prob - oracle| <= 1e-5 at every shape, with a shared list and with padded per-user lists, the user field in
    either slot; a guard after prob[U * C] keeps its bits."""
    from recsys_amd import _lib
    P = pair_params(D, layers)
    m, keep = device_pair_model(P, D, layers)
    assert _lib.lib().rsx_predict_pair_rank_supported(3, 200, D, len(layers), (C.c_int32 * 3)(*layers)) == 1
    worst = 0.0
    for user_slot in (1, 0):
        rng = np.random.default_rng(0)
        for U, Cn in SHAPES:
            user, items = draw_pairs(rng, U, Cn, user_slot)
            want = oracle_pair_prob(P, len(layers), user, items, user_slot)
            if (U, Cn) == (3, 37):
                assert want.std() >= 0.05, (D, float(want.std()))
            got = launch(m, user, items, user_slot, ld=Cn + 3)
            err = float(np.abs(got - want).max())
            # one shared list: every user against user 0's items
            shared = launch(m, user, items[0], user_slot)
            want_s = oracle_pair_prob(P, len(layers), user, np.tile(items[0], (U, 1)), user_slot)
            err_s = float(np.abs(shared - want_s).max())
            print("pair rank D=%d %s user_slot=%d U=%d C=%d: max |prob - oracle| = %.3g (item_ld = C + 3), %.3g (shared list)"
                  % (D, layers, user_slot, U, Cn, err, err_s))
            assert np.isfinite(got).all() and np.isfinite(shared).all()
            assert err <= 1e-5 and err_s <= 1e-5, (user_slot, U, Cn, err, err_s)
            worst = max(worst, err, err_s)
    assert worst <= 1e-5


def test_a_pairs_bits_are_its_own():
    """2: the same (user, item) pair alone, at position 37 of 200, in a shared and in a per-user list, as user 0 of 1 and as
    user 2 of 3, launched eagerly and replayed from a graph: one bit pattern."""
    from recsys_amd import _lib
    D, layers = 32, (200, 200, 200)
    P = pair_params(D, layers)
    m, keep = device_pair_model(P, D, layers)
    rng = np.random.default_rng(5)
    user, items = draw_pairs(rng, 3, 200)
    u, i = user[2], items[2, 37]
    alone = bits(launch(m, np.int32([u]), np.int32([[i]])))[0, 0]
    assert alone == bits(launch(m, np.int32([u]), np.int32([i])))[0, 0]                         # shared list of one
    assert alone == bits(launch(m, np.int32([u]), items[2]))[0, 37]                             # position 37 of 200, user 0 of 1
    assert alone == bits(launch(m, np.int32([u]), items[2:3], ld=203))[0, 37]                   # ... in a per-user list
    assert alone == bits(launch(m, user, items[2]))[2, 37]                                      # user 2 of 3, shared list
    assert alone == bits(launch(m, user, items, ld=200))[2, 37] == bits(launch(m, user, items, ld=211))[2, 37]
    other = items.copy()
    other[2, :37] = rng.integers(0, ROWS[0], 37)                                                # other neighbours in the tile
    other[:2] = rng.integers(0, ROWS[0], (2, 200))
    assert alone == bits(launch(m, user, other))[2, 37]
    assert alone == bits(launch(m, np.int32([u]), items[2, 30:41]))[0, 7]                       # another position in the tile
    # eager against a graph replay of the same launch
    d_u, d_i = torch.from_numpy(user).cuda(), torch.from_numpy(items).cuda()
    out = torch.zeros(3 * 200, device="cuda")
    L = _lib.lib()

    def go():
        _lib.check(L.rsx_predict_pair_rank(C.byref(m), 1, d_u.data_ptr(), d_i.data_ptr(), 200, out.data_ptr(), 3, 200,
                                           torch.cuda.current_stream().cuda_stream), "rsx_predict_pair_rank")
    go()
    torch.cuda.synchronize()
    eager = out.cpu().numpy().copy()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with _lib.capture_gc_guard(), torch.cuda.graph(g):
        go()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(eager))
        out.zero_()
    assert bits(eager.reshape(3, 200))[2, 37] == alone


@pytest.mark.parametrize("D,layers", [(32, (200, 200, 200)), (16, (64, 32))], ids=["32", "16"])
def test_16_bit_tables_give_the_fp32_bits_of_the_widened_table(D, layers):
    """3: a bfloat16 and a float16 table against the fp32 instantiation over the widened table, bit for bit."""
    from recsys_amd import serving
    P = pair_params(D, layers)
    rng = np.random.default_rng(9)
    user, items = draw_pairs(rng, 3, 37)
    for name, code in (("bfloat16", 1), ("float16", 2)):
        q = serving.quantize_rows(P["tables"], name)
        wide = serving.dequantize_rows(q, name)
        assert wide.dtype == np.float32 and not np.array_equal(wide, P["tables"])
        m16, keep16 = device_pair_model(P, D, layers, tables=q, table_dtype=code)
        m32, keep32 = device_pair_model(P, D, layers, tables=wide)
        a, b = launch(m16, user, items, ld=40), launch(m32, user, items, ld=40)
        assert np.array_equal(bits(a), bits(b)), name
        assert np.array_equal(bits(launch(m16, user, items[1])), bits(launch(m32, user, items[1]))), name
        assert a.std() >= 0.05


# ---- the Predictor ---------------------------------------------------------------------------------------------------------
def pair_bundle(tmp_path_factory, D, layers):
    """-> the bundle directory of an Estimator over the two small id columns holding pair_params(D, layers)."""
    from recsys_amd import deepfm
    from recsys_amd.estimator import ModeKeys
    from tests.parity_util import load_oracle_weights, make_estimator
    key = (D, tuple(layers))
    if key not in _BUNDLES:
        lin, emb = pair_columns(D)
        params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": D, "learning_rate": 1e-3,
                  "dropout": 0.5, "deep_layers": ",".join(map(str, layers)), "max_batch_size": 64}
        est = make_estimator(deepfm.model_fn, params)
        with torch.no_grad():
            est._call_model_fn({"ids": torch.zeros(1, 2, dtype=torch.int32, device="cuda")}, None, ModeKeys.PREDICT)
        load_oracle_weights(est, pair_params(D, layers))
        _BUNDLES[key] = est.export_savedmodel(str(tmp_path_factory.mktemp("pair_rank_export")))
        del est
    return _BUNDLES[key]


def raw_request(rng, U, Cn):
    """Raw int64 ids from a range far wider than the buckets: different ids collide in a bucket."""
    return rng.integers(0, 10 ** 6, U).astype(np.int64), rng.integers(0, 10 ** 6, (U, Cn)).astype(np.int64)


def _examples(u, it):
    from oracle import tfrecord
    return [tfrecord.encode_example({"u_id": [int(a)], "i_id": [int(b)]}) for a, b in zip(u, it)]


@pytest.mark.parametrize("D,layers,path", [(32, (200, 200, 200), "layers"), (16, (64, 32), "fused")], ids=["32-layers", "16-fused"])
def test_rank_items_against_predict_on_the_expansion(tmp_path_factory, D, layers, path):
    """4: within 2e-5 (both sit within 1e-5 of the same oracle) in every request form, four chunks included; `path`,
    `predict` and `predict_examples` of the same Predictor give the bits they gave before any ranking request."""
    from recsys_amd import serving
    d = pair_bundle(tmp_path_factory, D, layers)
    p = serving.Predictor.load(d, max_batch_size=512, max_candidates=256)
    assert p.manifest["feature_set"] == "uid_iid" and p.path == path and p.pair_path == "fused" and p._pair is None
    rng = np.random.default_rng(13)
    u, it = raw_request(rng, 3, 1000)
    ids0 = serving.expand_pair_request(p.layout, u, it[:, :50])
    ex = _examples(np.repeat(u, 50), it[:, :50].reshape(-1))
    before = (p.predict({"ids": ids0})["prob"], p.predict_examples(ex)["prob"])
    assert np.array_equal(bits(before[0]), bits(before[1])) and p._pair is None
    rows = serving.hash_pair_ids(p.layout, "i_id", it[0])
    assert len(np.unique(rows)) < len(np.unique(it[0]))                   # the request does hold colliding ids

    def check(uu, ii, shape):
        got = p.rank_items(uu, ii)["prob"]
        want = p.predict({"ids": serving.expand_pair_request(p.layout, uu, ii)})["prob"].reshape(shape)
        err = float(np.abs(got - want).max())
        print("rank_items D=%d %s: max |rank_items - predict(expansion)| = %.3g" % (D, shape, err))
        assert got.shape == shape and got.dtype == np.float32 and err <= 2e-5, (shape, err)
        return got
    check(int(u[0]), it[0, :37], (37,))                                   # a scalar user, one list
    check(u[:1], it[0, :37], (1, 37))                                     # [U] users, a shared list
    a = check(u, it[1, :200], (3, 200))
    b = check(u, np.tile(it[1, :200], (3, 1)), (3, 200))                  # [U, C]: the same list per user, the same bits
    assert np.array_equal(bits(a), bits(b))
    full = check(u, it, (3, 1000))                                        # four chunks of 256 / 256 / 256 / 232
    assert full.std() >= 0.05
    assert np.array_equal(bits(check(u[2:], it[2:, :300], (1, 300))), bits(full[2:, :300]))
    for _ in range(2):                                                    # the second and third request of a shape: graph replays
        assert np.array_equal(bits(p.rank_items(u, it)["prob"]), bits(full))
    assert "graph" in p._graphs[("pair_rank", 3, 256, 256)] and "graph" in p._graphs[("pair_rank", 3, 232, 232)]
    assert p.path == path and p._pair is not None
    after = (p.predict({"ids": ids0})["prob"], p.predict_examples(ex)["prob"])
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))


def test_one_launch_per_chunk(tmp_path_factory):
    """5: eager, rsx_dbg_launch_count advances by one rank launch per chunk, with top_k by one selection launch behind each;
    `predict` on the expansion takes more; with graphs the second request of a shape is captured and replays."""
    from recsys_amd import _lib, serving
    d = pair_bundle(tmp_path_factory, 32, (200, 200, 200))
    p = serving.Predictor.load(d, max_batch_size=256, max_candidates=256, use_hip_graph=False)
    L = _lib.lib()
    rng = np.random.default_rng(17)
    u, it = raw_request(rng, 3, 600)

    def count(f):
        f()
        n0 = L.rsx_dbg_launch_count()
        f()
        return L.rsx_dbg_launch_count() - n0
    for Cn, chunks in ((1, 1), (16, 1), (200, 1), (256, 1), (600, 3)):
        assert count(lambda: p.rank_items(int(u[0]), it[0, :Cn])) == chunks, Cn
        assert count(lambda: p.rank_items(u, it[:, :Cn])) == chunks, Cn
        assert count(lambda: p.rank_items(u, it[:, :Cn], top_k=10)) == 2 * chunks, Cn
    n = count(lambda: p.predict({"ids": serving.expand_pair_request(p.layout, u[:1], it[0, :200])}))
    print("C=200: rank_items 1 launch, predict on the expansion %d library launches" % n)
    assert n > 1
    g = serving.Predictor.load(d, max_batch_size=256, max_candidates=256, use_hip_graph=True)
    want = p.rank_items(u, it[:, :200])["prob"]
    for call in range(3):
        assert np.array_equal(bits(g.rank_items(u, it[:, :200])["prob"]), bits(want)), call
        assert ("graph" in g._graphs[("pair_rank", 3, 200, 200)]) == (call >= 1)
    assert g._n_graphs == 1


def test_top_k_on_the_device_against_the_host_definition(tmp_path_factory):
    """6: the same indices and probability bits as `topk_rows_host` on the full scores; colliding ids resolve by the lower
    index; a k beyond the device's takes the host path with the same answer."""
    from recsys_amd import serving
    d = pair_bundle(tmp_path_factory, 32, (200, 200, 200))
    p = serving.Predictor.load(d, max_batch_size=256, max_candidates=256)
    rng = np.random.default_rng(19)
    u, it = raw_request(rng, 3, 1000)
    it[:, 500:] = it[:, :500][:, ::-1]                                    # every id twice: equal scores at two positions
    for Cn in (37, 1000):
        full = p.rank_items(u, it[:, :Cn])["prob"]
        for k in (1, 10, 100):
            assert p.pair_topk_path_for(k) == "device"
            for _ in range(2):                                            # (eager, then the captured graph)
                got = p.rank_items(u, it[:, :Cn], top_k=k)
                want = serving.topk_rows_host(full, k)
                assert p.pair_topk_path == "device" and got["index"].shape == (3, min(k, Cn))
                assert np.array_equal(got["index"], want["index"]) and np.array_equal(bits(got["prob"]), bits(want["prob"])), (Cn, k)
            one = p.rank_items(int(u[1]), it[1, :Cn], top_k=k)
            assert np.array_equal(one["index"], want["index"][1]) and np.array_equal(bits(one["prob"]), bits(want["prob"][1]))
    top = p.rank_items(u, it, top_k=100)
    pairs = 0                                                             # position j and 999 - j hold the same id
    for r in range(3):
        order = top["index"][r].tolist()
        for j in order:
            if j < 999 - j and 999 - j in order:
                assert full[r, j] == full[r, 999 - j] and order.index(j) < order.index(999 - j), (r, j)
                pairs += 1
    assert pairs >= 100
    assert p.pair_topk_path_for(2000) == "host"
    got = p.rank_items(u, it, top_k=2000)
    want = serving.topk_rows_host(full, 2000)
    assert p.pair_topk_path == "host" and got["index"].shape == (3, 1000)
    assert np.array_equal(got["index"], want["index"]) and np.array_equal(bits(got["prob"]), bits(want["prob"]))


def test_recommend_items_against_the_host_definition(tmp_path_factory):
    """7: the device path against `recommend_items_host` over a 1 000-item catalogue in 300 buckets: items, indices, counts and
    probability bits, for every kind of `exclude`; 300 distinct exclusions take the host path with the same result."""
    from recsys_amd import _lib, serving
    d = pair_bundle(tmp_path_factory, 32, (200, 200, 200))
    p = serving.Predictor.load(d, max_batch_size=256, max_candidates=256)
    rng = np.random.default_rng(23)
    cat = rng.permutation(5000)[:1000].astype(np.int64)
    cat[3] = 0                                                            # item 0 is a real item
    cat = np.unique(cat)[rng.permutation(len(np.unique(cat)))]
    N = len(cat)
    with pytest.raises(_lib.RsxError, match=r"i_id\[5\] = .* repeats i_id\[2\]"):
        p.set_item_catalogue(np.concatenate([cat[:5], cat[2:3]]))
    with pytest.raises(_lib.RsxError, match=r"i_id\[1\] = -2 is negative"):
        p.set_item_catalogue([4, -2, 5])
    with pytest.raises(_lib.RsxError, match="set_item_catalogue"):
        p.recommend_items(1, 3)
    p.set_item_catalogue(cat)
    assert p.item_catalogue_size == N and len(np.unique(serving.hash_pair_ids(p.layout, "i_id", cat))) <= 300 < N
    users = rng.integers(0, 10 ** 6, 3).astype(np.int64)
    full = p.rank_items(users, cat)["prob"]

    def same(got, want):
        assert np.array_equal(got["index"], want["index"]) and np.array_equal(got["item"], want["item"])
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(bits(got["prob"]), bits(want["prob"]))
    pad = lambda rows: np.array([list(r) + [-1] * (max(map(len, rows)) - len(r)) for r in rows], np.int64)
    for k in (10, 100):
        assert p.recommend_items_path_for(k) == "device"
        for U in (1, 3):
            u = users[:U]
            per_user = pad([list(cat[rng.permutation(N)[:5 + 7 * r]]) + [0, 777777 + r] for r in range(U)])
            for exclude in (None, np.tile(cat[:40], (U, 1)), per_user, np.full((U, 3), 888888, np.int64), np.zeros((U, 1), np.int64)):
                for _ in range(2):                                        # (eager, then the captured graph)
                    got = p.recommend_items(u, k, exclude)
                    assert p.recommend_items_path == "device", (k, U)
                    same(got, serving.recommend_items_host(full[:U], cat, exclude, k))
            # every excluded entry is absent; an id that is not in the catalogue excluded nothing
            got = p.recommend_items(u, k, per_user)
            for r in range(U):
                assert not set(got["item"][r].tolist()) & set(per_user[r][per_user[r] >= 0].tolist())
            # the scalar form: arrays cut to count
            one = p.recommend_items(int(u[0]), k, per_user[0])
            want = serving.recommend_items_host(full[0], cat, per_user[0], k)
            same(one, want)
            assert one["count"] == k and one["prob"].shape == (k,)
    assert "graph" in p._graphs[("pair_recommend", 3, 100, 0)]
    # one user with 300 distinct exclusions: beyond rsx_topk_rows_excl's 256, the host path, the same result
    many = np.full((3, 300), -1, np.int64)
    many[1] = cat[rng.permutation(N)[:300]]
    many[0, :4] = cat[:4]
    got = p.recommend_items(users, 10, many)
    assert p.recommend_items_path == "host"
    same(got, serving.recommend_items_host(full, cat, many, 10))
    # count < top_k when the exclusions leave fewer entries (a small catalogue: kk = N)
    small = cat[:20]
    p.set_item_catalogue(small)
    ex = pad([list(small[:15]), list(small[:3]), []])
    got = p.recommend_items(users, 100, ex)
    assert p.recommend_items_path == "device" and got["count"].tolist() == [5, 17, 20] and got["prob"].shape == (3, 20)
    same(got, serving.recommend_items_host(p.rank_items(users, small)["prob"], small, ex, 100))
    assert np.isnan(got["prob"][0, 5:]).all() and (got["item"][0, 5:] == -1).all() and (got["index"][1, 17:] == -1).all()


def test_embedding_size_12_cannot_be_built(tmp_path_factory):
    """8, the premise: this package builds no model of embedding_size 12 at all -- rsx_gather_fm_fwd, the first launch of every
    Estimator forward, takes D in {4, 8, 16, 32, 64} and refuses anything else before any HIP call -- so there is no such
    bundle to rank with.  The embedding sizes outside rsx_predict_pair_rank's envelope that a bundle can have are 4 and 64;
    the C ABI's answer for D = 12 is in tests/test_pair_rank_cpu.py."""
    from recsys_amd import _lib
    with pytest.raises(_lib.RsxError, match="rsx_gather_fm_fwd failed: invalid argument"):
        pair_bundle(tmp_path_factory, 12, (32, 18))


@pytest.mark.parametrize("D,layers", [(64, (32, 18)), (4, (32, 18)), (8, (100, 50, 30, 20))], ids=["D64", "D4", "4-layers"])
def test_outside_the_envelope_answers_through_the_expansion(tmp_path_factory, D, layers):
    """8: the same API and the same order through `predict` on the expansion and the host selection."""
    from recsys_amd import serving
    d = pair_bundle(tmp_path_factory, D, layers)
    p = serving.Predictor.load(d, max_batch_size=256, max_candidates=256)
    assert p.path == "layers" and p.pair_path == "layers" and p.pair_topk_path_for(10) == "host" and p.recommend_items_path_for(10) == "host"
    rng = np.random.default_rng(29)
    u, it = raw_request(rng, 2, 300)
    got = p.rank_items(u, it)["prob"]
    want = p.predict({"ids": serving.expand_pair_request(p.layout, u, it)})["prob"].reshape(2, 300)
    assert np.array_equal(bits(got), bits(want))
    top = p.rank_items(u, it, top_k=10)
    ref = serving.topk_rows_host(want, 10)
    assert p.pair_topk_path == "host" and np.array_equal(top["index"], ref["index"]) and np.array_equal(bits(top["prob"]), bits(ref["prob"]))
    cat = np.unique(it[0])
    p.set_item_catalogue(cat)
    rec = p.recommend_items(u, 10, np.tile(cat[:5], (2, 1)))
    full = p.rank_items(u, cat)["prob"]
    ref = serving.recommend_items_host(full, cat, np.tile(cat[:5], (2, 1)), 10)
    assert p.recommend_items_path == "host" and p._pair is None
    assert np.array_equal(rec["item"], ref["item"]) and np.array_equal(bits(rec["prob"]), bits(ref["prob"]))


def test_other_bundles_raise_the_naming_error(tmp_path_factory, tmp_path):
    """8: a Criteo-style deepfm.py bundle and a din.py bundle."""
    from recsys_amd import _lib, deepfm, serving
    from recsys_amd.estimator import ModeKeys
    from tests.parity_util import make_estimator, small_columns
    from tests.test_gpu_din_rank import din_bundle
    lin, emb = small_columns([7, 50, 3], 16)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
              "dropout": 0.5, "deep_layers": "32,16", "max_batch_size": 64}
    est = make_estimator(deepfm.model_fn, params)
    with torch.no_grad():
        est._call_model_fn({"ids": torch.zeros(1, 3, dtype=torch.int32, device="cuda")}, None, ModeKeys.PREDICT)
    for d, script in ((est.export_savedmodel(str(tmp_path / "criteo")), "deepfm"), (din_bundle(tmp_path_factory, 32, 30)[0], "din")):
        p = serving.Predictor.load(d, max_batch_size=64)
        assert p.script == script and p.pair_path is None and p.pair_topk_path_for(5) is None
        for name, args in (("rank_items", (1, [1, 2])), ("set_item_catalogue", ([1, 2],)), ("recommend_items", (1, 3))):
            with pytest.raises(_lib.RsxError, match=r"%s: only deepfm\.py bundles.*this bundle is %s\.py" % (name, script)):
                getattr(p, name)(*args)


def test_script_train_export_rank(tmp_path):
    """9: deepfm.main --feature_set uid_iid: train a few steps, export, Predictor.load(export_path).rank_items against `predict`
    on the expansion."""
    from oracle import tfrecord
    from recsys_amd import deepfm, serving
    rng = np.random.default_rng(0)
    d = str(tmp_path) + "/"
    for k in range(2):
        n = 256
        u, i = rng.integers(1, 40, n), rng.integers(1, 25, n)
        lab = ((i % 3 == 0) ^ (rng.random(n) < 0.1)).astype(np.int64)
        blob = b"".join(tfrecord.frame(tfrecord.encode_example({"label": [int(lab[r])], "u_id": [int(u[r])], "i_id": [int(i[r])]}))
                        for r in range(n))
        open(d + "part-r-%05d" % k, "wb").write(blob)
    export_path = str(tmp_path / "export")
    common = ["--train_path", d, "--train_parts", "2", "--eval_parts", "1", "--batch_size", "64", "--model_dir",
              str(tmp_path / "model"), "--save_checkpoints_steps", "8", "--log_steps", "4", "--dropout", "0.1", "--learning_rate",
              "0.01", "--feature_set", "uid_iid", "--embedding_size", "8", "--export_path", export_path]
    res = deepfm.main(common + ["--task_type", "train", "--num_epochs", "2"])
    assert np.isfinite(res["loss"])
    deepfm.main(common + ["--task_type", "export"])
    p = serving.Predictor.load(export_path, max_candidates=64)
    assert p.pair_path == "fused" and p.global_step == res["global_step"]
    users, items = np.int64([3, 17, 39]), np.arange(0, 100, dtype=np.int64)
    got = p.rank_items(users, items)["prob"]
    want = p.predict({"ids": serving.expand_pair_request(p.layout, users, items)})["prob"].reshape(3, 100)
    err = float(np.abs(got - want).max())
    print("deepfm.main uid_iid: max |rank_items - predict(expansion)| = %.3g" % err)
    assert got.shape == (3, 100) and err <= 2e-5
    top = p.rank_items(users, items, top_k=5)
    assert np.array_equal(top["index"], serving.topk_rows_host(got, 5)["index"])
