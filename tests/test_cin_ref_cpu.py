"""The conditions tests/test_gpu_cin_forms.py rests on, checked without a GPU: the case table of tests/cin_ref.py takes the forms it
records (read from rsx_cin_layer_plan, the launchers' own selection) and holds every form, the fp64 reference is the oracle's and
a torch autograd restatement's, both float32 restatements are inside a quarter of the bounds on every case, and the bounds have teeth."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import models
from tests import cin_ref as cr

OK, EUNSUPPORTED = 0, -3
TIGHT = dict(rtol=1e-12, atol=1e-12)


@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _plan(L, c, sweep=0):
    out = (C.c_int32 * 8)()
    assert L.rsx_cin_layer_plan(c.B, c.F, c.H, c.N, sweep, out) == OK, c.id
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the table
def test_every_case_takes_the_form_the_table_records(L):
    for c in cr.LAYER_CASES:
        p = _plan(L, c)
        assert cr.plan_key(p) == cr.plan_of(c), (c.id, p)
        if c.lds is not None:
            assert p[4] == c.lds, (c.id, p)
        assert (p[5] == 1) == (p[4] > 64 * 1024)
        # a sweep slice riding changes the weight-gradient configuration and nothing else
        s = _plan(L, c, 1)
        assert s[6] == 2 and s[:6] == p[:6] and s[7] == p[7], (c.id, s)
        if c.first:
            assert c.F == c.H


def test_the_table_holds_every_form_and_edge(L):
    forms = set()
    for c in cr.LAYER_CASES:
        p = _plan(L, c)
        forms.add(((p[1], p[2], p[3]), p[6], p[0]))
    assert forms == cr.FORMS_REQUIRED
    by = cr.LAYER
    # the untiled form at 7 and at 8 waves with one field part; the tiled one at its first HT; both sides of H = 48
    assert (_plan(L, by["fs1_7"])[7], _plan(L, by["fs1"])[7], _plan(L, by["t5_n2"])[7]) == (7, 8, 5)
    assert (_plan(L, by["h48"])[0], _plan(L, by["h49"])[0]) == (12, 32) and (_plan(L, by["h48"])[3], _plan(L, by["h49"])[3]) == (4, 2)
    assert [c.id for c in cr.LAYER_CASES if _plan(L, c)[5]] == ["lds82"]
    # the batch is ragged against 4 (forward workgroup, EB) and takes a second and a third trip of the weight gradients' loop
    assert {c.id for c in cr.LAYER_CASES if c.B % 4 == 0} == {"h48", "h49"}      # (the pair about H alone: one full workgroup)
    assert by["l2_c0"].B > 32 and by["c2"].B > 16 and by["b67"].B > 64 and by["l1_c3"].B > 32
    # the sweep cases: one whose configuration is 2 anyway, one where the slice changes it
    assert _plan(L, by[cr.SWEEP_SAME_CFG])[6] == 2 and _plan(L, by[cr.SWEEP_OTHER_CFG])[6] == 0
    # gradient modes and accumulate flags: each mode and each flag pair occurs, in both data-gradient kernels
    for tiled in (0, 1):
        vs = [cr.parse_variant(v) for c in cr.LAYER_CASES if c.tiled == tiled and not c.first for v in c.variants]
        assert {v[0] for v in vs} == {"d", "g", "b"} and {v[1:] for v in vs} == {(0, 0), (0, 1), (1, 0), (1, 1)}, tiled
    for c in cr.LAYER_CASES:
        if c.first:                      # one buffer: acc_dx0 = 1, with and without a prefill
            assert {cr.parse_variant(v)[2] for v in c.variants} == {1} and {cr.parse_variant(v)[1] for v in c.variants} == {0, 1}
    assert {c.tiled for c in cr.LAYER_CASES if c.own_out} == {0, 1} and any(c.first for c in cr.LAYER_CASES if c.own_out)
    h = cr.HEAD_CASES
    assert any(c.B > 128 for c in h) and any(c.B > 512 and c.nnum > 16 for c in h) and any(len(c.sizes) == cr.CIN_MAXL for c in h)
    assert any(n * 4 > 512 for c in h for n in c.sizes) and any(n % 16 for c in h if len(c.sizes) > 1 for n in c.sizes)
    assert any(c.nnum == 0 for c in h) and (1, (16,), 0) in {(c.B, c.sizes, c.nnum) for c in h}


def test_workspace_is_dpre_and_one_plane_of_partials_per_h_tile(L):
    for c in cr.LAYER_CASES:
        assert L.rsx_cin_bwd_workspace_floats(c.B, c.F, c.H, c.N) == c.B * c.N * 16 + (-(-c.H // 16)) * c.B * c.F * 16


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("cid", ["l1_c3", "c1", "fs2", "tiny", "one"])
def test_fp64_reference_is_the_oracles(cid):
    c, d = cr.LAYER[cid], cr.draw_layer(cid)
    X0, Xk, W, cc = (t.double().numpy() for t in (d.X0, d.Xk, d.W, d.c))
    pre, out = cr.fwd_of(cid)
    o = models.cin_layer_fwd(X0, Xk, W, cc)
    np.testing.assert_allclose(out, o, **TIGHT)
    for mode in "dgb":
        r = cr.bwd_of(cid, mode, mask=out > 0)
        dX0, dXk, dW, dc = models.cin_layer_bwd(X0, Xk, W, o, cr.grad_in(d, mode))
        for name, want in (("dX0", dX0), ("dXk", dXk), ("dW", dW), ("dc", dc)):
            np.testing.assert_allclose(r[name], want, err_msg=name, **TIGHT)


@pytest.mark.parametrize("cid", ["l1_c3", "c2", "fs1_7", "h49", "one"])
def test_fp64_reference_is_torch_autograds(cid):
    c, d = cr.LAYER[cid], cr.draw_layer(cid)
    X0 = d.X0.double().requires_grad_()
    Xk = X0 if c.first else d.Xk.double().requires_grad_()
    W, cc = d.W.double().requires_grad_(), d.c.double().requires_grad_()
    _, out = cr.layer_fwd_chain(X0, Xk, W, cc)
    pre_r, out_r = cr.fwd_of(cid)
    np.testing.assert_allclose(out.detach().numpy(), out_r, **TIGHT)
    out.backward(torch.from_numpy(cr.grad_in(d, "b")))
    r = cr.bwd_of(cid, "b", mask=out_r > 0)
    zero = (np.zeros_like(r["dXk"]), np.zeros_like(r["dX0"]))
    want = cr.expected(c, r, 0, 1, zero)
    got = {"dW": W.grad, "dc": cc.grad}
    got.update({"dX": X0.grad} if c.first else {"dXk": Xk.grad, "dX0": X0.grad})
    assert set(got) == set(want)
    for name in want:
        np.testing.assert_allclose(got[name].numpy(), want[name], err_msg=name, **TIGHT)


@pytest.mark.parametrize("cid", cr.HEAD_IDS)
def test_head_reference_is_torch_autograds(cid):
    c, d = cr.HEAD[cid], cr.draw_head(cid)
    W, b = d.Wout.double().requires_grad_(), d.bout.double().requires_grad_()
    y = torch.relu(torch.cat([m.double() for m in d.maps], 1).sum(-1) @ W + b)
    y_r = cr.head_fwd(d)
    np.testing.assert_allclose(y.detach().numpy(), y_r, **TIGHT)
    (y * d.gy.double()).sum().backward()
    r = cr.head_bwd(d, y=y_r)
    np.testing.assert_allclose(W.grad.numpy(), r["dWout"], **TIGHT)
    np.testing.assert_allclose(b.grad.numpy(), r["dbout"], **TIGHT)
    np.testing.assert_allclose((d.gy.double() * (y.detach() > 0)).numpy(), r["gs"], **TIGHT)
    if c.nnum:
        lx = d.logx.double().requires_grad_()
        w = torch.zeros(c.nnum, dtype=torch.float64, requires_grad=True)
        ((lx @ w) * d.g_lin.double()).sum().backward()
        np.testing.assert_allclose(w.grad.numpy(), r["dwnum"], **TIGHT)
    else:
        assert r["dwnum"] is None
    # the backward's y input holds a y that is exactly 0 and one below it wherever the batch has room
    if c.B >= 6:
        assert bool((d.y_bwd == 0).any()) and bool((d.y_bwd < 0).any()) and bool((d.y_bwd > 0).any())


def test_draws_are_a_function_of_the_case_alone():
    a, b = cr.draw_layer("tiny"), cr.draw_layer.__wrapped__("tiny")
    for k in ("X0", "Xk", "W", "c", "dout", "gs", "wout", "pre_k", "pre_0"):
        assert torch.equal(getattr(a, k), getattr(b, k))
    assert cr.draw_layer("l1_c3").Xk is cr.draw_layer("l1_c3").X0
    for cid in cr.LAYER_IDS:            # about half of the relus are open, and the pre-activation is of order 1
        out = cr.fwd_of(cid)[1]
        assert 0.3 <= float((out > 0).mean()) <= 0.7 and 1.0 <= float(out.max()) <= 10.0, cid


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("cid", cr.LAYER_IDS)
def test_float32_restatements_are_inside_a_quarter_of_the_bounds(cid):
    c, d = cr.LAYER[cid], cr.draw_layer(cid)
    ref = cr.fwd_of(cid)[1]
    bad = []
    for impl in ("einsum", "torch"):
        got = cr.fwd_of(cid, impl)[1]
        assert got.dtype == np.float32
        if cr.misses(got, ref, "out", cr.MARGIN):
            bad.append((impl, "out", cr.figure(got, ref)))
        for v in c.variants:
            mode, ak, a0 = cr.parse_variant(v)
            r = cr.bwd_cached(cid, mode)
            pre = cr.prefills(d, r)
            want, have = cr.expected(c, r, ak, a0, pre), cr.expected(c, cr.bwd_cached(cid, mode, impl), ak, a0, pre)
            for name in want:
                assert have[name].dtype == np.float32
                if cr.misses(have[name], want[name], name, cr.MARGIN):
                    bad.append((impl, v, name, cr.figure(have[name], want[name])))
    assert not bad, bad


@pytest.mark.parametrize("cid", cr.HEAD_IDS)
def test_head_float32_restatements_are_inside_a_quarter_of_the_bounds(cid):
    d = cr.draw_head(cid)
    y, r = cr.head_fwd(d), cr.head_bwd(d)
    bad = []
    for impl in ("einsum", "torch"):
        got = cr.head_fwd(d, impl)
        assert got.dtype == np.float32
        if cr.misses(got, y, "y", cr.MARGIN):
            bad.append((impl, "y", cr.figure(got, y)))
        g = cr.head_bwd(d, impl)
        for name in r:
            if r[name] is not None and cr.misses(g[name], r[name], name, cr.MARGIN):
                bad.append((impl, name, cr.figure(g[name], r[name])))
    assert not bad, bad


def test_bounds_are_no_looser_than_the_split_paths():
    """TOL / BTOL of tests/test_gpu_cin_split.py: 2e-6 forward, 3e-6 backward of the largest entry"""
    assert cr.RTOL + cr.A_FWD <= 2e-6 and cr.RTOL + cr.A_BWD <= 3e-6 and cr.MARGIN >= 4.0
    ref = torch.tensor([0.0, -1.0, 4.0], dtype=torch.float64)
    assert float(cr.bound(ref, "out").max()) <= 2e-6 * 4.0 and float(cr.bound(ref, "dW").max()) <= 3e-6 * 4.0
    assert cr.misses(torch.tensor([float("nan"), -1.0, 4.0]), ref, "out") == 1


# ------------------------------------------------------------------------------------------------ teeth
def _median_index(a):
    """index of the element of median magnitude among the non-zero ones"""
    flat = np.abs(a).reshape(-1)
    nz = np.flatnonzero(flat)
    return np.unravel_index(nz[np.argsort(flat[nz])[len(nz) // 2]], a.shape)


@pytest.mark.parametrize("cid", cr.LAYER_IDS)
def test_bounds_reject_a_wrong_layer(cid):
    c, d = cr.LAYER[cid], cr.draw_layer(cid)
    X0, Xk, W, cc = (t.double().numpy() for t in (d.X0, d.Xk, d.W, d.c))
    pre, out = cr.fwd_of(cid)
    # one (f, h) term of median size dropped from one output element (the largest: its relu is open)
    b, n, dd = np.unravel_index(np.argmax(out), out.shape)
    terms = X0[b, :, None, dd] * Xk[b, None, :, dd] * W.reshape(c.F, c.H, c.N)[:, :, n]
    f, h = _median_index(terms)
    w = out.copy()
    w[b, n, dd] = max(pre[b, n, dd] - terms[f, h] + cc[n], 0.0)
    assert cr.misses(w, out, "out") == 1, (f, h)
    # the bias added after the relu
    assert cr.misses(np.maximum(pre, 0) + cc[None, :, None], out, "out") > 0
    for v in c.variants:
        mode, ak, a0 = cr.parse_variant(v)
        r = cr.bwd_cached(cid, mode)
        pf = cr.prefills(d, r)
        want = cr.expected(c, r, ak, a0, pf)
        # one example (of median share) dropped from one dW element
        j, n = _median_index(r["dW"])
        f, h = divmod(int(j), c.H)
        share = (X0[:, f, :] * Xk[:, h, :] * r["dpre"][:, n, :]).sum(1)
        w = r["dW"].copy()
        w[j, n] -= share[_median_index(share)[0]]
        assert cr.misses(w, want["dW"], "dW") == 1, (v, j, n)
        # dc without one d-lane
        assert cr.misses(r["dc"] - r["dpre"][:, :, cr.D - 1].sum(0), want["dc"], "dc") > 0, v
        # the accumulate prefill ignored / the gradient not added onto it
        for name, acc, p in (("dXk", ak, pf[0]), ("dX0", a0, pf[1])):
            if not c.first and acc:
                assert cr.misses(r[name], want[name], name) > 0 and cr.misses(p, want[name], name) > 0, (v, name)
        if c.first:
            base = pf[1].astype(np.float64) if ak else 0.0
            # a gradient role of X0 missing
            assert cr.misses(base + r["dXk"], want["dX"], "dX") > 0 and cr.misses(base + r["dX0"], want["dX"], "dX") > 0, v
            if ak:
                assert cr.misses(r["dXk"] + r["dX0"], want["dX"], "dX") > 0, v


@pytest.mark.parametrize("cid", cr.HEAD_IDS)
def test_bounds_reject_a_wrong_head(cid):
    c, d = cr.HEAD[cid], cr.draw_head(cid)
    r = cr.head_bwd(d)
    ar = np.arange(c.B)
    # gs taken with y >= 0: the examples whose y is exactly 0 pass their gradient on
    if bool((d.y_bwd == 0).any()):
        w = cr.head_bwd(d, gate=lambda y: y >= 0)
        for name in ("gs", "dWout", "dbout"):
            assert cr.misses(w[name], r[name], name) > 0, name
    # ... and with no gate at all (y < 0)
    if bool((d.y_bwd < 0).any()):
        assert cr.misses(cr.head_bwd(d, gate=lambda y: y == y)["gs"], r["gs"], "gs") > 0
    # a strided loop without its second trip: examples >= 128 of dWout / dbout, examples >= 512 and column 16 of dwnum
    if c.B > 128:
        w = cr.head_bwd(d, keep=ar < 128)
        assert cr.misses(w["dWout"], r["dWout"], "dWout") > 0 and cr.misses(w["dbout"], r["dbout"], "dbout") > 0
    if c.B > 512 and c.nnum:
        assert cr.misses(cr.head_bwd(d, keep=ar < 512)["dwnum"], r["dwnum"], "dwnum") > 0
    if c.nnum > 16:
        w = r["dwnum"].copy()
        w[16:] = 0.0
        assert cr.misses(w, r["dwnum"], "dwnum") == c.nnum - 16
    # the forward: one layer's last column left out, the bias added after the relu
    y = cr.head_fwd(d)
    S = np.concatenate([m.double().numpy().sum(2) for m in d.maps], 1)
    Wd = d.Wout.double().numpy()
    live = y > 0
    w = y.copy()
    w[live] = (y - S[:, -1] * Wd[-1])[live]
    assert cr.misses(w, y, "y") > 0
    if bool((S @ Wd < 0).any()):        # (an example whose logit is positive without the bias cannot tell)
        assert cr.misses(np.maximum(S @ Wd, 0) + 0.1, y, "y") > 0
