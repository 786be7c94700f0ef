"""Candidate ranking of din.py bundles, the parts that need no device: the request expansion (the baseline every GPU test and
scripts/bench_serving_din.py compare against), the argument checking of `Predictor.rank_candidates`, and the host-side refusals
of rsx_predict_din_rank / rsx_predict_din_rank_supported (include/rsx.h), which all return before any HIP call."""
import ctypes as C

import numpy as np
import pytest

EINVAL, EUNSUPPORTED = -1, -3
FAKE = 0x1000                       # "some non-NULL, 16-byte aligned pointer": never read
P = C.c_void_p(FAKE)


@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_expand_rank_request_against_a_loop():
    from recsys_amd import serving
    rng = np.random.default_rng(0)
    U, Cn, Pq, P_ = 3, 5, 7, 10
    hi, hc = rng.integers(0, 50, (U, Pq)), rng.integers(0, 9, (U, Pq))
    ci, cc = rng.integers(0, 50, (U, Cn)), rng.integers(0, 9, (U, Cn))
    e = serving.expand_rank_request(hi, hc, ci, cc, hist_len=P_)
    assert {k: (v.shape, v.dtype) for k, v in e.items()} == {
        "i_id": ((U * Cn,), np.dtype(np.int32)), "i_cate": ((U * Cn,), np.dtype(np.int32)),
        "u_iid_seq": ((U * Cn, P_), np.dtype(np.int32)), "u_icat_seq": ((U * Cn, P_), np.dtype(np.int32))}
    for u in range(U):
        for c in range(Cn):
            r = u * Cn + c
            assert e["i_id"][r] == ci[u, c] and e["i_cate"][r] == cc[u, c]
            for p in range(P_):
                assert e["u_iid_seq"][r, p] == (hi[u, p] if p < Pq else 0)
                assert e["u_icat_seq"][r, p] == (hc[u, p] if p < Pq else 0)
    # one user given as 1-D arrays; no hist_len: the histories keep their length
    e1 = serving.expand_rank_request(hi[0], hc[0], ci[0], cc[0])
    assert e1["u_iid_seq"].shape == (Cn, Pq) and np.array_equal(e1["u_iid_seq"], np.repeat(hi[:1], Cn, 0))
    assert np.array_equal(e1["i_cate"], cc[0])
    from recsys_amd._lib import RsxError
    with pytest.raises(RsxError, match="length 7 does not fit hist_len 5"):
        serving.expand_rank_request(hi, hc, ci, cc, hist_len=5)
    with pytest.raises(RsxError):
        serving.expand_rank_request(hi[:2], hc[:2], ci, cc)


def test_rank_request_checking():
    from recsys_amd import serving
    from recsys_amd._lib import RsxError
    chk = lambda *a: serving.check_rank_request(*a, 30, 300, 20)
    h, c = np.arange(1, 11), np.arange(5)
    assert chk(h, h % 20, c, c) == (1, 5, 10, True)
    assert chk(h[None].astype(np.int64), h[None] % 20, c[None].astype(np.uint8), c[None].astype(np.int16)) == (1, 5, 10, False)
    assert chk(np.tile(h, (3, 1)), np.tile(h % 20, (3, 1)), np.tile(c, (3, 1)), np.tile(c, (3, 1))) == (3, 5, 10, False)
    assert chk(list(h), list(h % 20), list(c), list(c)) == (1, 5, 10, True)              # lists become numpy
    import torch
    assert chk(torch.from_numpy(h), torch.from_numpy(h % 20), torch.from_numpy(c), torch.from_numpy(c)) == (1, 5, 10, True)
    with pytest.raises(RsxError, match="length 31 does not fit this bundle's hist_len 30"):
        chk(np.ones(31, np.int32), np.ones(31, np.int32), c, c)
    with pytest.raises(RsxError, match="integers"):
        chk(h.astype(np.float32), h % 20, c, c)
    with pytest.raises(RsxError, match="expected histories"):
        chk(h, h[:-1] % 20, c, c)                                     # the two histories differ in length
    with pytest.raises(RsxError, match="expected histories"):
        chk(h, h % 20, c, c[:-1])
    with pytest.raises(RsxError, match="expected histories"):
        chk(h[None], h[None] % 20, c, c)                              # 2-D histories with 1-D candidates
    with pytest.raises(RsxError, match="2 histories for 3 rows"):
        chk(np.tile(h, (2, 1)), np.tile(h % 20, (2, 1)), np.tile(c, (3, 1)), np.tile(c, (3, 1)))
    with pytest.raises(RsxError, match="empty request"):
        chk(h, h % 20, c[:0], c[:0])
    with pytest.raises(RsxError, match=r"i_id holds ids outside \[0, 300\)"):
        chk(h, h % 20, c + 296, c)
    with pytest.raises(RsxError, match=r"u_icat_seq holds ids outside \[0, 20\)"):
        chk(h, h + 15, c, c)
    with pytest.raises(RsxError, match="u_iid_seq holds ids outside"):
        chk(h - 5, h % 20, c, c)
    with pytest.raises(RsxError, match="i_cate holds ids outside"):
        chk(torch.from_numpy(h), torch.from_numpy(h % 20), torch.from_numpy(c), torch.from_numpy(c + 16))


def test_only_din_bundles_rank_candidates():
    from recsys_amd import serving
    from recsys_amd._lib import RsxError
    for script in ("fm", "deepfm", "dcn", "xdeepfm"):
        p = object.__new__(serving.Predictor)            # (a loaded Predictor of that script; loading needs a device)
        p.script = script
        with pytest.raises(RsxError, match=r"only din.py bundles .* this bundle is %s.py" % script):
            p.rank_candidates(np.ones(3, np.int32), np.ones(3, np.int32), np.ones(2, np.int32), np.ones(2, np.int32))


def test_supported_envelope_corners(L):
    w = (C.c_int32 * 3)(100, 50, 20)
    sup = lambda U=1, Cn=200, Pn=100, K=32, n1=80, n2=40, Ln=3, wd=w: L.rsx_predict_din_rank_supported(U, Cn, Pn, K, n1, n2, Ln, wd)
    assert sup() == 1 and sup(K=16) == 1
    assert sup(Pn=1) == 1 and sup(Pn=128) == 1 and sup(Pn=129) == 0 and sup(Pn=0) == 0
    assert sup(Cn=1) == 1 and sup(Cn=0) == 0 and sup(U=0) == 0 and sup(U=7, Cn=4096) == 1
    assert sup(K=8) == 0 and sup(K=64) == 0 and sup(K=24) == 0
    assert sup(n1=64) == 0 and sup(n2=32) == 0 and sup(Ln=2) == 0 and sup(wd=None) == 0
    assert sup(wd=(C.c_int32 * 3)(100, 52, 20)) == 0 and sup(wd=(C.c_int32 * 3)(128, 50, 20)) == 0
    # U * C * P < 2^31
    assert sup(U=1, Cn=(1 << 31) // 128 - 1, Pn=128) == 1 and sup(U=1, Cn=(1 << 31) // 128, Pn=128) == 0
    assert sup(U=1 << 12, Cn=1 << 12, Pn=128) == 0 and sup(U=1 << 12, Cn=1 << 12, Pn=127) == 1


def _fake_model(K=32):
    from recsys_amd import _lib
    m = _lib.PredictDinModel()
    m.item_emb = m.cate_emb = m.item_bias = m.mlp_wout = m.mlp_bout = FAKE
    for a in range(2):
        for l in range(3):
            m.att_W[a][l] = m.att_b[a][l] = FAKE
    for l, (n, ld) in enumerate(((100, 100), (50, 52), (20, 20))):
        m.mlp_W[l] = m.mlp_b[l] = FAKE
        m.widths[l], m.ld[l] = n, ld
    m.K, m.n1, m.n2, m.L, m.bias_ld = K, 80, 40, 3, 4
    return m


def test_rank_entry_refuses_bad_arguments_before_any_device_call(L):
    call = lambda m, hi=P, hc=P, ci=P, cc=P, pr=P, U=1, Cn=8, Pn=30: \
        L.rsx_predict_din_rank(C.byref(m) if m is not None else None, hi, hc, ci, cc, pr, U, Cn, Pn, None)
    m = _fake_model()
    assert call(None) == EINVAL
    for kw in ("hi", "hc", "ci", "cc", "pr"):
        assert call(m, **{kw: None}) == EINVAL, kw
    assert call(m, Cn=0) == EINVAL and call(m, Pn=0) == EINVAL and call(m, U=0) == EINVAL and call(m, U=-1) == EINVAL
    for field in ("item_emb", "cate_emb", "item_bias", "mlp_wout", "mlp_bout"):
        bad = _fake_model()
        setattr(bad, field, None)
        assert call(bad) == EINVAL, field
    bad = _fake_model()
    bad.att_W[1][2] = None
    assert call(bad) == EINVAL
    bad = _fake_model()
    bad.mlp_b[1] = None
    assert call(bad) == EINVAL
    bad = _fake_model()
    bad.ld[1] = 48                                        # a row stride shorter than the layer
    assert call(bad) == EINVAL
    bad = _fake_model()
    bad.item_emb = FAKE + 4                               # rows are read 16 bytes at a time
    assert call(bad) == EINVAL
    bad = _fake_model()
    bad.bias_ld = 0
    assert call(bad) == EINVAL
    # outside the envelope
    assert call(_fake_model(K=8)) == EUNSUPPORTED
    assert call(m, Pn=129) == EUNSUPPORTED
    assert call(m, U=1 << 12, Cn=1 << 12, Pn=128) == EUNSUPPORTED
    bad = _fake_model()
    bad.n1 = 64
    assert call(bad) == EUNSUPPORTED
    bad = _fake_model()
    bad.widths[0], bad.ld[0] = 128, 128
    assert call(bad) == EUNSUPPORTED
