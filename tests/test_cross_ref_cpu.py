"""The conditions tests/test_gpu_cross_forms.py rests on, checked without a GPU: the case table of tests/cross_ref.py takes the forms
its comments claim, the backward workspace holds every batch up to its capacity, the fp64 reference is the oracle's, the float32
restatement is inside the bounds, the bounds have teeth in every case, and the cross terms are not negligible in the drawn inputs."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import models
from tests import cross_ref as cr

BWD = cr.ids_of("bwd")
FWD = cr.ids_of("fwd") + cr.ids_of("gather")
EUNSUPPORTED = -3
P = C.c_void_p(0x1000)          # "some non-NULL pointer": never read, the call is refused before any HIP call


@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _ref(cid, terms="xz", dtype=torch.float64):
    return cr.run_ref(cr.draw(cid), terms, dtype=dtype)


# ------------------------------------------------------------------------------------------------ the table
def test_every_case_takes_the_form_its_comment_claims():
    for c in cr.CASES:
        if c.kind == "bwd":
            assert cr.bwd_form(c.B, c.dim, c.L) == (c.form, c.epw, c.RT, c.lds), c.id
        elif c.kind == "rider":
            f = cr.rider_form(c.B, c.dim, c.L, c.widths)
            assert f is not None and f[:4] == (c.ntd, c.epw, c.RT, c.lds), (c.id, f)
            # the separate-launch path of the same shape is cross_bwd4_k<3> with the SAME examples per wave and partials
            assert cr.bwd_form(c.B, c.dim, c.L) == ("bwd4", c.epw, c.RT, c.lds), c.id
        else:
            assert c.dim % 4 == 0 and c.dim <= cr.CROSS_MAX_DIM and c.L <= cr.CROSS_MAX_L
            assert c.kind == "fwd" or (c.dim == 16 * len(c.rows) and len(c.rows) <= 64)


def test_the_table_holds_every_form_and_edge():
    b = [cr.CASE[i] for i in BWD]
    assert {(c.form, c.epw) for c in b} == {("bwd4", 1), ("bwd4", 2), ("bwd4", 4), ("wave", 1), ("wave", 2), ("wave", 4)}
    assert {c.L for c in b if c.form == "bwd4"} == {1, 2, 3}                       # every instantiation of cross_bwd4_k
    # both sides of every examples-per-wave switch
    for form, edges, L_ in (("bwd4", (1024, 8192), 2), ("wave", (512, 2048), 4)):
        for e in edges:
            lo, hi = cr.bwd_form(e, 16, L_), cr.bwd_form(e + 1, 16, L_)
            assert lo[0] == hi[0] == form and hi[1] == 2 * lo[1]
    assert {1024, 1025, 8193} <= {c.B for c in b if c.form == "bwd4"} and {512, 513, 2049} <= {c.B for c in b if c.form == "wave"}
    # the LDS edges: exactly 80 KiB, the widest <3>, four bytes' worth of dim beyond it, the widest L = 8, and the refused one
    assert any(c.lds == cr.LDS_BWD4 for c in b if c.form == "bwd4")
    assert cr.bwd_form(9, 728, 3)[0] == "bwd4" and cr.bwd_form(9, 732, 3)[0] == "wave"
    assert cr.bwd_form(11, 960, 8)[0] == "wave" and cr.bwd_form(11, 960, 8)[3] <= cr.LDS_WAVE < cr.bwd_form(*cr.UNSUPPORTED)[3]
    assert cr.bwd_form(*cr.UNSUPPORTED)[0] == "unsupported"
    assert cr.bwd_form(70, 1024, 7)[0] == "wave"
    # lanes: one live lane, exactly one full vector, a second vector with one live lane, four full vectors
    assert {4, 256, 260, 1024, 624} <= {c.dim for c in cr.CASES if c.kind == "fwd"}
    assert any(c.defer for c in b if c.form == "bwd4") and any(c.defer for c in b if c.form == "wave")
    assert any(c.own_s for c in b if c.form == "bwd4") and any(c.own_s for c in b if c.form == "wave")
    r = [c for c in cr.CASES if c.kind == "rider"]
    assert {c.ntd for c in r} == {4, 8} and {c.epw for c in r} == {2, 4}
    assert any(c.widths[-2] == 128 for c in r) and any(c.lds == 81536 for c in r)
    assert any(cr.rider_form(c.B, c.dim, c.L, c.widths)[4] for c in r)             # a wide first layer accumulating onto dX
    assert cr.rider_form(4096, 732, 3, (64, 16)) is None and cr.rider_form(4096, 64, 3, (132, 64)) is None


def test_the_unsupported_shape_is_refused_before_any_launch(L):
    B, dim, Lc = cr.UNSUPPORTED
    assert L.rsx_cross_bwd_defer(P, P, P, P, P, None, None, P, 0, P, P, None, P, B, dim, Lc, None, None) == EUNSUPPORTED
    assert L.rsx_cross_bwd(P, P, P, P, P, None, None, P, 0, P, P, None, P, B, dim, Lc, None) == EUNSUPPORTED


@pytest.mark.parametrize("Lc", [3, 4])
def test_workspace_holds_every_batch_up_to_the_capacity(L, Lc):
    """For capacities 1..9000: the partials of EVERY batch b <= capacity, in either backward form, fit in
    rsx_cross_bwd_workspace_floats(capacity) -- through the running maximum of the per-batch need -- and the size is no more than that."""
    dim, n = 32, (2 * Lc + 1) * 32
    need = np.array([cr.partials_needed(b, Lc, dim) for b in range(1, 9001)])
    worst = np.maximum.accumulate(need)
    got = np.array([L.rsx_cross_bwd_workspace_floats(cap, dim, Lc) for cap in range(1, 9001)], dtype=np.int64)
    assert (got % n == 0).all()
    assert (got // n >= worst).all(), int(np.flatnonzero(got // n < worst)[0]) + 1
    assert (got // n == worst).all()
    assert need[1999] == 1000 and need[2999] == 750                                 # the example of the defect: 2000 needs more than 3000
    for dim_, L_, cap, batches in cr.CAPACITY_CASES:
        ws = L.rsx_cross_bwd_workspace_floats(cap, dim_, L_)
        for b in batches:
            assert cr.partials_needed(b, L_, dim_) * (2 * L_ + 1) * dim_ <= ws
    assert L.rsx_cross_bwd_workspace_floats(0, 32, 3) == 0


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("cid", ["b5x4x1", "b513x64x5", "b300x624x3", "g130x80x8"])
def test_fp64_reference_is_the_oracles(cid):
    d = cr.draw(cid)
    x0, W, Bc, wout, dxL, gz = (t.double().numpy() for t in (d.x0, d.W, d.Bc, d.wout, d.dxL, d.gz))
    xs, ss = models.cross_fwd(x0, W, Bc)
    r = _ref(cid, "xz")
    tol = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r.xL.numpy(), xs[-1], **tol)
    np.testing.assert_allclose(r.s.numpy(), np.stack(ss, 1), **tol)
    np.testing.assert_allclose(r.cz.numpy(), xs[-1] @ wout, **tol)
    for terms, g in (("x", dxL), ("z", gz[:, None] * wout[None, :]), ("xz", dxL + gz[:, None] * wout[None, :])):
        dX, dW, dB = models.cross_bwd(xs, ss, W, g)
        r = _ref(cid, terms)
        np.testing.assert_allclose(r.dX.numpy(), dX, **tol)
        np.testing.assert_allclose(r.dW.numpy(), dW, **tol)
        np.testing.assert_allclose(r.dB.numpy(), dB, **tol)
        if "z" in terms:
            np.testing.assert_allclose(r.dwout.numpy(), (gz[:, None] * xs[-1]).sum(0), **tol)
        else:
            assert r.dwout is None


def test_draws_are_a_function_of_the_case_alone():
    for cid in ("b5x4x1", "g9x16x2"):
        c = cr.CASE[cid]
        a, b = cr.draw(cid), cr.draw_shape(c.B, c.dim, c.L, c.seed, c.rows)
        for k in ("x0", "W", "Bc", "wout", "dxL", "gz", "pre"):
            assert torch.equal(getattr(a, k), getattr(b, k))
    d = cr.draw("b300x624x3")
    assert float(d.gz.abs().min()) >= 0.5e-2 and float(d.gz.abs().max()) <= 1.5e-2 and bool((d.gz < 0).any()) and bool((d.gz > 0).any())


@pytest.mark.parametrize("cid", [c.id for c in cr.CASES])
def test_cross_terms_are_not_negligible(cid):
    assert float(_ref(cid).s.abs().median()) >= 0.2


def _held(name, key, got, ref):
    """the float32 restatement: inside the default bounds, or listed with its figure and then within 4 x that figure"""
    if key in cr.RESTATEMENT_OUTSIDE:
        lim = 4.0 * cr.RESTATEMENT_OUTSIDE[key] * float(ref.abs().max())
        assert float((got.double() - ref).abs().max()) <= lim, (name, key)
    else:
        assert cr.misses(got, ref) == 0, (name, key, cr.figure(got, ref))


@pytest.mark.parametrize("cid", FWD + BWD)
def test_float32_restatement_is_inside_the_bounds(cid):
    c = cr.CASE[cid]
    r, f = _ref(cid), _ref(cid, "xz", torch.float32)
    for name in ("s", "xL", "cz"):
        _held(name, (cid, "fwd", name), getattr(f, name), getattr(r, name))
    if c.kind != "bwd":
        return
    for terms in cr.TERMS:
        tr_, tf = cr.tensors(_ref(cid, terms), terms), cr.tensors(_ref(cid, terms, torch.float32), terms)
        for name in tr_:
            _held(name, (cid, terms, name), tf[name], tr_[name])


# ------------------------------------------------------------------------------------------------ teeth
@pytest.mark.parametrize("cid", FWD + BWD)
def test_bounds_reject_a_layer_without_its_cross_term(cid):
    c, d, r = cr.CASE[cid], cr.draw(cid), _ref(cid)
    for l in range(c.L):
        w = cr.run_ref(d, "xz", drop_layer=l)
        assert cr.misses(w.xL, r.xL, (cid, "fwd", "xL")) > 0 and cr.misses(w.cz, r.cz, (cid, "fwd", "cz")) > 0, (cid, l)
        if l < c.L - 1:          # (the last layer's term reaches no later s)
            assert cr.misses(w.s, r.s, (cid, "fwd", "s")) > 0, (cid, l)
        if c.kind == "bwd":      # the backward of the same wrong function: dx0 lacks s_l * dx_{l+1}
            for terms in cr.TERMS:
                assert cr.misses(cr.run_ref(d, terms, drop_layer=l).dX, _ref(cid, terms).dX, (cid, terms, "dX")) > 0, (cid, l, terms)


@pytest.mark.parametrize("cid", BWD + cr.ids_of("rider"))
def test_bounds_reject_a_wrong_backward(cid):
    """(a rider case: its cross layers' share alone, gz only as the rider runs, with the drawn gz in the head gradient's place)"""
    c, d = cr.CASE[cid], cr.draw(cid)
    for terms in (cr.TERMS if c.kind == "bwd" else ("z",)):
        r = _ref(cid, terms)
        t = cr.tensors(r, terms)
        # one example left out of the batch sums: the first, the last (alone in its wave where the batch is ragged), one inside
        for b in sorted({0, c.B // 2, c.B - 1}):
            keep = torch.ones(c.B, dtype=torch.bool)
            keep[b] = False
            w = cr.tensors(cr.run_ref(d, terms, keep=keep), terms)
            for name in t:
                if name != "dX":
                    assert cr.misses(w[name], t[name], (cid, terms, name)) > 0, (cid, terms, name, b)
        if "z" in terms:         # dX without gz * wout: with dxL that is the "x" gradient; alone, nothing flows at all
            w = _ref(cid, "x").dX if "x" in terms else torch.zeros_like(r.dX)
            assert cr.misses(w, r.dX, (cid, terms, "dX")) > 0, (cid, terms)
            # ... and in EVERY example (gz is nowhere small): no row of dX survives the omission
            bad = ~((w - r.dX).abs() <= cr.bound(r.dX, (cid, terms, "dX")))
            assert bool(bad.any(1).all()), (cid, terms)
        # accumulate ignored: the gradient alone where prefill + gradient is expected
        pre = cr.prefill(d, r.dX)
        want = cr.tensors(r, terms, pre)["dX"]
        assert cr.misses(r.dX, want, (cid, terms, "dX")) > 0 and cr.misses(pre, want, (cid, terms, "dX")) > 0, (cid, terms)
