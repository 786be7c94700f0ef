"""Item ranking for uid_iid deepfm.py bundles, the part that needs no device: the expansion that defines a request, the numpy
definition of `recommend_items`, every request validator, rsx_predict_pair_rank's envelope and its refusals (all of which
happen before any HIP call)."""
import ctypes as C

import numpy as np
import pytest

from oracle import hashing
from recsys_amd import _lib, serving
from recsys_amd.feature_columns import CriteoLayout
from tests.pair_util import ROWS, pair_columns, pair_params, oracle_pair_prob, draw_pairs

EINVAL, EUNSUPPORTED = -1, -3
P = C.c_void_p(0x1000)                                    # an aligned non-NULL address that is never dereferenced


@pytest.fixture(scope="module")
def L():
    from recsys_amd import build
    build.build(verbose=False)
    return _lib.lib()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _hash(key, rows):
    return hashing.fingerprint64(str(int(key)).encode()) % rows


def test_expand_pair_request_against_hand_hashed_ids(L):
    lay = CriteoLayout.from_columns(pair_columns(8)[1])
    assert [c.key for c in lay.columns] == ["i_id", "u_id"] and serving.pair_slots(lay) == (1, 0)
    u, it = np.int64([7, 123456789012, -3]), np.int64([[5, 0, 99999999999], [1, 2, 3], [300, 600, 5]])
    ids = serving.expand_pair_request(lay, u, it)
    assert ids.shape == (9, 2) and ids.dtype == np.int32
    for a in range(3):
        for c in range(3):
            assert ids[a * 3 + c].tolist() == [_hash(it[a, c], ROWS[0]), _hash(u[a], ROWS[1])], (a, c)
    # a shared list is the list repeated for every user; a scalar user is one user
    assert np.array_equal(serving.expand_pair_request(lay, u, it[0]), serving.expand_pair_request(lay, u, np.tile(it[0], (3, 1))))
    assert np.array_equal(serving.expand_pair_request(lay, 7, it[0]), ids[:3])
    # the one-field hash `rank_items` uses is that column of the expansion
    assert np.array_equal(serving.hash_pair_ids(lay, "i_id", it), ids[:, 0].reshape(3, 3))
    assert np.array_equal(serving.hash_pair_ids(lay, "u_id", u), ids[::3, 1])


def test_request_validators():
    ok_u, ok_i = np.int64([1, 2]), np.int64([[1, 2, 3], [4, 5, 6]])
    u, it, single = serving.check_pair_request(5, [1, 2, 3])
    assert single and u.tolist() == [5] and it.shape == (3,) and u.dtype == it.dtype == np.int64
    assert serving.check_pair_request(ok_u, ok_i)[2] is False and serving.check_pair_request(ok_u, ok_i[0])[1].shape == (3,)
    for bad_u, bad_i in ((1.5, ok_i[0]), (ok_u, ok_i.astype(np.float32)), (True, ok_i[0]), (ok_u[None], ok_i), (5, ok_i),
                         (np.int64([1, 2, 3]), ok_i), (ok_u, ok_i[:, :, None]), (ok_u, 3), (np.zeros(0, np.int64), ok_i[0]),
                         (ok_u, np.zeros((2, 0), np.int64))):
        with pytest.raises(_lib.RsxError, match="rank_items"):
            serving.check_pair_request(bad_u, bad_i)
    assert serving.check_item_catalogue([3, 0, 9]).tolist() == [3, 0, 9]
    with pytest.raises(_lib.RsxError, match=r"i_id\[2\] = -4 is negative"):
        serving.check_item_catalogue([3, 0, -4, -5])
    with pytest.raises(_lib.RsxError, match=r"i_id\[3\] = 7 repeats i_id\[1\]"):
        serving.check_item_catalogue([3, 7, 9, 7, 9])
    for bad in (np.int64([[1, 2]]), [], [1.0, 2.0], 5):
        with pytest.raises(_lib.RsxError, match="set_item_catalogue"):
            serving.check_item_catalogue(bad)
    assert serving.check_pair_exclude(None, 3, False).shape == (3, 0)
    assert serving.check_pair_exclude([4, -1], 1, True).tolist() == [[4, -1]] and serving.check_pair_exclude([], 1, True).shape == (1, 0)
    for ex, U, single in (([[1, 2]], 1, True), ([1, 2], 2, False), ([[1], [2], [3]], 2, False), ([0.5], 1, True)):
        with pytest.raises(_lib.RsxError, match="exclude"):
            serving.check_pair_exclude(ex, U, single)
    for bad in (0, -1, True, 2.5, None):
        with pytest.raises(_lib.RsxError, match="top_k"):
            serving.recommend_items_host(np.float32([0.5, 0.25]), np.int64([1, 2]), None, bad)


def test_exclusion_positions():
    cat = np.int64([50, 0, 7, 2 ** 40, 3])
    ex = np.int64([[7, -1, 0, 99], [2 ** 40, 2 ** 40, 3, -7]])
    assert serving.exclusion_positions(cat, ex).tolist() == [[3, 0, 2, 0], [4, 4, 5, 0]]
    assert serving.exclusion_positions(cat, np.zeros((2, 0), np.int64)).shape == (2, 0)


def test_recommend_items_host_on_hand_made_scores():
    cat = np.int64([10, 0, 30, 40, 2 ** 35, 60])
    prob = np.float32([[0.5, 0.9, 0.5, 0.1, 0.9, 0.3], [0.2, 0.2, 0.2, 0.2, 0.2, 0.2]])
    got = serving.recommend_items_host(prob, cat, None, 3)
    assert got["index"].tolist() == [[1, 4, 0], [0, 1, 2]] and got["count"].tolist() == [3, 3]       # ties: the lower position
    assert got["item"].tolist() == [[0, 2 ** 35, 10], [10, 0, 30]] and got["item"].dtype == np.int64
    assert np.array_equal(bits(got["prob"]), bits(np.float32([[0.9, 0.9, 0.5], [0.2, 0.2, 0.2]])))
    # exclusions: item 0 is real, negative entries are padding, an id outside the catalogue excludes nothing
    got = serving.recommend_items_host(prob, cat, np.int64([[0, -1, 77], [10, 30, 40]]), 3)
    assert got["index"].tolist() == [[4, 0, 2], [1, 4, 5]] and got["item"].tolist() == [[2 ** 35, 10, 30], [0, 2 ** 35, 60]]
    # short lists are padded with NaN / -1 / -1 and counted
    got = serving.recommend_items_host(prob, cat, np.int64([[10, 0, 30, 40, -1], [10, 0, 30, 40, 2 ** 35]]), 4)
    assert got["count"].tolist() == [2, 1] and got["index"].tolist() == [[4, 5, -1, -1], [5, -1, -1, -1]]
    assert got["item"].tolist() == [[2 ** 35, 60, -1, -1], [60, -1, -1, -1]] and np.isnan(got["prob"][0, 2:]).all()
    assert np.isnan(got["prob"][1, 1:]).all() and got["prob"].shape == (2, 4)
    # top_k beyond N: kk = N; the one-user form is cut to count
    one = serving.recommend_items_host(prob[0], cat, np.int64([40]), 100)
    assert one["count"] == 5 and one["index"].tolist() == [1, 4, 0, 2, 5] and one["prob"].shape == (5,)
    with pytest.raises(_lib.RsxError, match="recommend_items_host"):
        serving.recommend_items_host(prob, cat[:5], None, 3)
    with pytest.raises(_lib.RsxError, match="exclude"):
        serving.recommend_items_host(prob[0], cat, np.int64([[1]]), 3)


def test_weights_recipe_spreads_the_probabilities():
    """The checks of tests/test_gpu_pair_rank.py have teeth only while the oracle's probabilities spread."""
    rng = np.random.default_rng(0)
    user, items = draw_pairs(rng, 3, 37)
    for D, layers in ((32, (200, 200, 200)), (16, (64, 32)), (8, (32, 18))):
        std = float(oracle_pair_prob(pair_params(D, layers), len(layers), user, items).std())
        print("D=%d %s: std of the oracle's probabilities %.3f" % (D, layers, std))
        assert std >= 0.05, (D, std)


def test_supported_over_the_envelopes_edges(L):
    def sup(U, Cn, D, layers):
        return L.rsx_predict_pair_rank_supported(U, Cn, D, len(layers), (C.c_int32 * max(1, len(layers)))(*layers))
    for D in (8, 16, 32):
        for layers in ((200, 200, 200), (64, 32), (100,), (32, 18), (256,), (512, 256)):
            assert sup(3, 37, D, layers) == 1, (D, layers)
    assert sup(1, 1, 32, (200, 200, 200)) == 1 and sup(1, 2 ** 31 - 1, 32, (200,)) == 1 and sup(2 ** 15, 2 ** 15, 8, (4,)) == 1
    for D in (12, 0, 4, 64, -16):
        assert sup(3, 37, D, (64, 32)) == 0, D
    assert sup(3, 37, 16, ()) == 0 and sup(3, 37, 16, (64, 32, 16, 8)) == 0                       # L = 0 and L = 4
    assert sup(3, 37, 16, (64, 260)) == 0 and sup(3, 37, 16, (260,)) == 0                         # last width 260
    assert sup(3, 37, 16, (50, 32)) == 0 and sup(3, 37, 16, (64, 50, 32)) == 0                    # inner width 50
    assert sup(3, 37, 16, (64, 50)) == 1                                                          # (the last one may be)
    assert sup(2 ** 16, 2 ** 15, 16, (64, 32)) == 0 and sup(1, 2 ** 31 - 1, 16, (64, 32)) == 1    # U * C = 2^31
    assert sup(0, 5, 16, (64, 32)) == 0 and sup(5, 0, 16, (64, 32)) == 0
    assert L.rsx_predict_pair_rank_supported(3, 37, 16, 2, None) == 0
    assert sup(3, 37, 32, (20000, 64)) == 0                                                       # beyond the 160 KB of LDS


def _model(D=32, layers=(200, 200, 200), F=2):
    m = _lib.PredictModel()
    m.tables = m.w1 = m.row_off = m.wd = m.bd = m.c0 = m.wo = m.bo = P.value
    for l, n in enumerate(layers[:3]):
        m.W[l] = m.b[l] = m.gamma[l] = m.beta[l] = P.value
        m.widths[l] = n
    m.w1_field_mask, m.bn_eps, m.F, m.D, m.L = 3, 1e-3, F, D, len(layers)
    return m


def test_refusals_come_before_any_hip_call(L):
    """No device here: a call that got past its checks would fail in the launch instead of returning these codes."""
    def call(m, user_slot=1, user=P, item=P, ld=0, prob=P, U=3, Cn=37):
        return L.rsx_predict_pair_rank(C.byref(m) if m is not None else None, user_slot, user, item, ld, prob, U, Cn, None)
    ok = _model()
    assert call(None) == EINVAL
    for kw in (dict(user=None), dict(item=None), dict(prob=None), dict(U=0), dict(U=-1), dict(Cn=0), dict(user_slot=2),
               dict(user_slot=-1), dict(ld=36), dict(ld=-1), dict(ld=1)):
        assert call(ok, **kw) == EINVAL, kw
    assert call(_model(F=3)) == EINVAL and call(_model(F=1)) == EINVAL
    for name in ("tables", "row_off", "wo", "bo", "wd", "bd"):
        m = _model()
        setattr(m, name, None)
        assert call(m) == EINVAL, name
    for arr in ("W", "b"):
        m = _model()
        getattr(m, arr)[1] = None
        assert call(m) == EINVAL, arr
    m = _model()
    m.gamma[0] = None                                     # gamma without beta
    assert call(m) == EINVAL
    m = _model()
    m.tables = 0x1004                                     # not 16-byte aligned
    assert call(m) == EINVAL
    m = _model()
    m.table_dtype = 3
    assert call(m) == EINVAL
    m = _model()
    m.bn_eps = -1.0
    assert call(m) == EINVAL
    # outside the envelope: RSX_EUNSUPPORTED, also before any HIP call
    assert call(_model(D=12)) == EUNSUPPORTED and call(_model(D=64)) == EUNSUPPORTED
    assert call(_model(layers=())) == EUNSUPPORTED and call(_model(layers=(64, 32, 16, 8))) == EUNSUPPORTED
    assert call(_model(layers=(64, 260))) == EUNSUPPORTED and call(_model(layers=(50, 32))) == EUNSUPPORTED
    assert call(ok, U=2 ** 16, Cn=2 ** 15) == EUNSUPPORTED


def _bare(script, feature_set=None, **kw):
    p = object.__new__(serving.Predictor)
    p.script, p._item_cat, p._pair = script, None, None
    p.manifest = {"params": {"embedding_size": 16, "deep_layers": "64,32"}}
    if feature_set:
        p.manifest["feature_set"] = feature_set
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_predictor_refusals_name_the_bundle():
    for script, fs in (("din", "din"), ("deepfm", "criteo"), ("dcn", "criteo"), ("fm", None)):
        p = _bare(script, fs)
        for name, args in (("rank_items", (1, [1, 2])), ("set_item_catalogue", ([1, 2],)), ("recommend_items", (1, 3))):
            with pytest.raises(_lib.RsxError, match=r"%s: only deepfm\.py bundles.*this bundle is %s\.py" % (name, script)):
                getattr(p, name)(*args)
        assert p.pair_path is None and p.pair_topk_path_for(3) is None and p.recommend_items_path_for(3) is None
    p = _bare("deepfm", "uid_iid")
    with pytest.raises(_lib.RsxError, match="set_item_catalogue"):
        p.recommend_items(1, 3)
    with pytest.raises(_lib.RsxError, match="u_id must hold integers"):
        p.rank_items(1.5, [1, 2])
    with pytest.raises(_lib.RsxError, match="top_k"):
        p.pair_topk_path_for(0)
