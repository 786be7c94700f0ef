"""The fp32 CIN layer kernels and the 'cin_net' head (csrc/cin.hip) against a plain fp64 restatement of xdeepfm/xdeepfm.py:145-182, in
every dispatch form -- tests/cin_ref.py holds the case tables (with the form each layer case was derived to take), the inputs, the
reference, two float32 restatements and the bounds; tests/test_cin_ref_cpu.py checks the tables, the reference and the bounds' teeth
without a GPU.

Every case calls the C ABI on buffers of the test's own: each output (out, dXk, dX0, dW, dc; y, gs, dWout, dbout, dwnum) between
sentinel blocks, the backward workspace (sized by rsx_cin_bwd_workspace_floats) with a sentinel block behind it, every output that
is not accumulated onto prefilled with NaN.  Before a launch the case asserts, through rsx_cin_layer_plan, that its shape takes the
form the table records.  The backward runs on the float32 rounding of the REFERENCE's out, so it is judged apart from the forward;
the `own_out` cases also on the kernel's own forward output (the reference then takes that output's relu mask).

Bounds: tests/cin_ref.py (2e-6 of max|reference| forward, 3e-6 backward).  Every comparison prints max|got - ref| / max|ref| next
to the same figure of the two float32 restatements (profiles/cin_fp64_errors.txt is one run's table)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cin_ref as cr

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats: 256 bytes, so the guarded views keep the float4 alignment
SENTINEL = -3.0e33
NAN = float("nan")
D = cr.D


def _L():
    from recsys_amd import _lib
    return _lib.lib()


def _check(rc, what):
    from recsys_amd import _lib
    _lib.check(rc, what)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Guarded:
    """n floats between two sentinel blocks (front=False: one block, behind), filled with `fill` (a number or an array)"""

    def __init__(self, n, fill=NAN, front=True):
        self.n, self.off = n, GUARD if front else 0
        self.whole = torch.full((self.off + n + GUARD,), SENTINEL, device="cuda")
        self.view = self.whole[self.off:self.off + n]
        if isinstance(fill, float):
            self.view.fill_(fill)
        else:
            self.view.copy_(torch.as_tensor(fill).reshape(-1))

    def intact(self):
        return bool((self.whole[:self.off] == SENTINEL).all()) and bool((self.whole[self.off + self.n:] == SENTINEL).all())


class _Report:
    """prints the error table of a case and gathers the misses, so that one run reports every tensor"""

    def __init__(self):
        self.bad = []

    def cmp(self, cid, tag, name, got, ref, ref_e, ref_t):
        fig = cr.figure(got, ref)
        print("CIN_ERR %-13s %-8s %-6s kernel %.3e  fp32-einsum %.3e  fp32-torch %.3e"
              % (cid, tag, name, fig, cr.figure(ref_e, ref), cr.figure(ref_t, ref)))
        n = cr.misses(got, ref, name)
        if n:
            self.bad.append("%s %s %s: %d elements outside, figure %.3e" % (cid, tag, name, n, fig))

    def note(self, ok, what):
        if not ok:
            self.bad.append(what)

    def done(self):
        for b in self.bad:
            print("CIN_FAIL " + b)
        assert not self.bad, "\n".join(self.bad)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ the layer
def _assert_plan(c, sweep=0):
    out = (C.c_int32 * 8)()
    assert _L().rsx_cin_layer_plan(c.B, c.F, c.H, c.N, sweep, out) == 0, c.id
    want = cr.plan_of(c)
    if sweep:
        want = want[:5] + (2,) + want[6:]
    assert cr.plan_key(tuple(out)) == want, (c.id, tuple(out))
    if c.lds is not None:
        assert out[4] == c.lds, (c.id, tuple(out))
    return tuple(out)


def _dev(c, d):
    v = {k: getattr(d, k).cuda() for k in ("X0", "W", "c", "dout", "gs", "wout")}
    v["Xk"] = v["X0"] if c.first else d.Xk.cuda()
    return v


def _forward(c, v, sweep=None):
    g = _Guarded(c.B * c.N * D)
    _check(_L().rsx_cin_layer_fwd(_p(v["X0"]), _p(v["Xk"]), _p(v["W"]), _p(v["c"]), _p(g.view), c.B, c.F, c.H, c.N, D,
                                  None if sweep is None else C.byref(sweep), _st()), "rsx_cin_layer_fwd")
    torch.cuda.synchronize()
    assert g.intact(), "out's neighbours were written"
    assert bool(torch.isfinite(g.view).all()), "out keeps a NaN of its prefill"
    return g.view.view(c.B, c.N, D)


def _backward(c, v, out, mode, ak, a0, pre, sweep=None):
    """one rsx_cin_layer_bwd on guarded buffers -> {name: tensor}; pre = (dXk, dX0) prefills of the accumulating outputs"""
    L_ = _L()
    B, F, H, N = c.B, c.F, c.H, c.N
    if c.first:
        assert a0 == 1
        gx = _Guarded(B * F * D, pre[1] if ak else NAN)
        gk = g0 = gx
    else:
        gk, g0 = _Guarded(B * H * D, pre[0] if ak else NAN), _Guarded(B * F * D, pre[1] if a0 else NAN)
    gW, gc = _Guarded(F * H * N), _Guarded(N)
    n_ws = int(L_.rsx_cin_bwd_workspace_floats(B, F, H, N))
    assert n_ws == B * N * D + (-(-H // 16)) * B * F * D
    ws = _Guarded(n_ws, front=False)
    _check(L_.rsx_cin_layer_bwd(_p(v["X0"]), _p(v["Xk"]), _p(v["W"]), _p(out), _p(v["dout"]) if mode in "db" else None,
                                _p(v["gs"]) if mode in "gb" else None, _p(v["wout"]) if mode in "gb" else None,
                                _p(gk.view), ak, _p(g0.view), a0, _p(gW.view), _p(gc.view), _p(ws.view), B, F, H, N, D,
                                None if sweep is None else C.byref(sweep), _st()), "rsx_cin_layer_bwd")
    torch.cuda.synchronize()
    assert gk.intact() and g0.intact(), "a data gradient's neighbours were written"
    assert gW.intact() and gc.intact(), "dW's or dc's neighbours were written"
    assert ws.intact(), "the workspace was overrun"
    res = {"dW": gW.view.view(F * H, N), "dc": gc.view}
    if c.first:
        res["dX"] = gk.view.view(B, F, D)
    else:
        res["dXk"], res["dX0"] = gk.view.view(B, H, D), g0.view.view(B, F, D)
    for name, t in res.items():
        assert bool(torch.isfinite(t).all()), "%s keeps a NaN of its prefill" % name
    return res


def _compare_bwd(rep, c, d, tag, got, mode, ak, a0, mask=None, names=None):
    refs = [cr.bwd_cached(c.id, mode, impl) if mask is None else cr.bwd_of(c.id, mode, impl, mask) for impl in ("ref", "einsum", "torch")]
    pre = cr.prefills(d, refs[0])
    want, want_e, want_t = (cr.expected(c, r, ak, a0, pre) for r in refs)
    assert set(got) == set(want)
    for name in (names or want):
        rep.cmp(c.id, tag, name, got[name], want[name], want_e[name], want_t[name])


@pytest.mark.parametrize("cid", cr.LAYER_IDS)
def test_cin_layer_matches_fp64(cid):
    c, d = cr.LAYER[cid], cr.draw_layer(cid)
    _assert_plan(c)
    v = _dev(c, d)
    rep = _Report()
    out_own = _forward(c, v)
    rep.cmp(cid, "fwd", "out", out_own, cr.fwd_of(cid)[1], cr.fwd_of(cid, "einsum")[1], cr.fwd_of(cid, "torch")[1])
    out32 = torch.from_numpy(cr.out32_of(cid)).cuda()
    for var in c.variants:
        mode, ak, a0 = cr.parse_variant(var)
        pre = cr.prefills(d, cr.bwd_cached(cid, mode))
        _compare_bwd(rep, c, d, var, _backward(c, v, out32, mode, ak, a0, pre), mode, ak, a0)
    if c.own_out:                       # as production runs: the relu mask is the kernel's own
        mode, ak, a0 = cr.parse_variant(c.variants[0])
        mask = (out_own > 0).cpu().numpy()
        pre = cr.prefills(d, cr.bwd_of(cid, mode, "ref", mask))
        _compare_bwd(rep, c, d, c.variants[0] + "/own", _backward(c, v, out_own, mode, ak, a0, pre), mode, ak, a0, mask=mask)
    rep.done()


# ------------------------------------------------------------------------------------------------ a sweep slice riding
class _Sweep:
    """optimizer state of cr.SWEEP_ROWS rows of 16 (a TABLE_TF1_COLD segment) and as many scalars (a VEC_COLD segment), about
    cr.SWEEP_TOUCHED of them touched, and the ONE slice that covers the whole untouched-row sweep (tests/test_gpu_adam_window.py)"""
    NAMES = ("tables", "m", "v", "w1", "m_w", "v_w")

    def __init__(self):
        from recsys_amd import _lib
        from recsys_amd.ops import AdamTF1
        R = cr.SWEEP_ROWS
        g = torch.Generator().manual_seed(20)
        self.init = [torch.randn(R, 16, generator=g), torch.randn(R, 16, generator=g) * 0.01, torch.rand(R, 16, generator=g) * 1e-4,
                     torch.randn(R, generator=g), torch.randn(R, generator=g) * 0.01, torch.rand(R, generator=g) * 1e-4]
        slot = torch.full((R + 4,), -1, dtype=torch.int32)
        idx = torch.randperm(R, generator=g)[:cr.SWEEP_TOUCHED]
        slot[idx] = torch.arange(cr.SWEEP_TOUCHED, dtype=torch.int32)
        self.touched = slot[:R] >= 0
        self.slot = slot.cuda()
        self.state = [t.clone().cuda() for t in self.init]
        t, m, v, w, mw, vw = self.state
        self.opt = AdamTF1(lr=1e-3, device="cuda")
        segs = [dict(kind=_lib.RSX_ADAM_TABLE_TF1_COLD, d=16, n=R, var=t, m=m, v=v, slot=self.slot),
                dict(kind=_lib.RSX_ADAM_VEC_COLD, n=R, var=w, m=mw, v=vw, slot=self.slot)]
        sl = self.opt.cold_slices(segs, [1.0])
        assert len(sl) == 1 and sl[0] is not None
        self.slice = sl[0]

    def assert_same_as(self, other, what):
        torch.cuda.synchronize()
        for name, a, b in zip(self.NAMES, self.state, other.state):
            assert _bits_equal(a, b), (what, name)

    def assert_swept(self):
        """the untouched rows moved, the touched ones did not"""
        for name, a, a0 in zip(self.NAMES, self.state, self.init):
            a = a.cpu()
            assert torch.equal(a[self.touched], a0[self.touched]), name
        assert not torch.equal(self.state[0].cpu()[~self.touched], self.init[0][~self.touched])
        assert not torch.equal(self.state[3].cpu()[~self.touched], self.init[3][~self.touched])


def _swept_alone():
    s = _Sweep()
    s.opt.run_slice(s.slice)
    torch.cuda.synchronize()
    s.assert_swept()
    return s


def test_cin_layer_carrying_a_sweep_slice_same_configuration():
    """cr.SWEEP_SAME_CFG: the plan says weight-gradient configuration 2 with or without a slice, so every output of the forward
    and of the backward is bit-identical to the run without one, and the swept state is rsx_adam_slice_run's of the same slice"""
    c, d = cr.LAYER[cr.SWEEP_SAME_CFG], cr.draw_layer(cr.SWEEP_SAME_CFG)
    assert _assert_plan(c)[6] == 2 and _assert_plan(c, sweep=1)[6] == 2
    v = _dev(c, d)
    alone = _swept_alone()
    out0 = _forward(c, v)
    sf = _Sweep()
    out1 = _forward(c, v, sweep=sf.slice)
    assert _bits_equal(out0, out1)
    sf.assert_same_as(alone, "forward")
    out32 = torch.from_numpy(cr.out32_of(c.id)).cuda()
    rep = _Report()
    for var in c.variants:
        mode, ak, a0 = cr.parse_variant(var)
        pre = cr.prefills(d, cr.bwd_cached(c.id, mode))
        g0 = _backward(c, v, out32, mode, ak, a0, pre)
        sb = _Sweep()
        g1 = _backward(c, v, out32, mode, ak, a0, pre, sweep=sb.slice)
        for name in g0:
            rep.note(_bits_equal(g0[name], g1[name]), "%s %s %s: not the bits of the run without a slice" % (c.id, var, name))
        sb.assert_same_as(alone, "backward " + var)
        _compare_bwd(rep, c, d, var + "/sw", g1, mode, ak, a0)
    rep.done()


def test_cin_layer_carrying_a_sweep_slice_other_configuration():
    """cr.SWEEP_OTHER_CFG: the slice turns weight-gradient configuration 0 into 2, another summation order -- dW and dc are held to
    the fp64 bounds (the direct check of the form the model-level test sees only through Adam), the data gradients (the same launch
    either way) to the bits of the run without a slice, the swept state to rsx_adam_slice_run's"""
    c, d = cr.LAYER[cr.SWEEP_OTHER_CFG], cr.draw_layer(cr.SWEEP_OTHER_CFG)
    assert _assert_plan(c)[6] == 0 and _assert_plan(c, sweep=1)[6] == 2
    v = _dev(c, d)
    alone = _swept_alone()
    out32 = torch.from_numpy(cr.out32_of(c.id)).cuda()
    rep = _Report()
    var = c.variants[0]
    mode, ak, a0 = cr.parse_variant(var)
    pre = cr.prefills(d, cr.bwd_cached(c.id, mode))
    g0 = _backward(c, v, out32, mode, ak, a0, pre)
    sb = _Sweep()
    g1 = _backward(c, v, out32, mode, ak, a0, pre, sweep=sb.slice)
    for name in ("dXk", "dX0"):
        rep.note(_bits_equal(g0[name], g1[name]), "%s %s %s: not the bits of the run without a slice" % (c.id, var, name))
    sb.assert_same_as(alone, "backward")
    _compare_bwd(rep, c, d, var + "/sw", g1, mode, ak, a0)
    rep.done()


# ------------------------------------------------------------------------------------------------ the head
def _head_args(c, maps):
    ptrs = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    sizes = (C.c_int32 * len(maps))(*c.sizes)
    return ptrs, sizes


@pytest.mark.parametrize("cid", cr.HEAD_IDS)
def test_cin_head_matches_fp64(cid):
    c, d = cr.HEAD[cid], cr.draw_head(cid)
    L_ = _L()
    maps = [m.cuda().contiguous() for m in d.maps]
    ptrs, sizes = _head_args(c, maps)
    Wout, bout, gy = d.Wout.cuda(), d.bout.cuda(), d.gy.cuda()
    tot, nl = sum(c.sizes), len(c.sizes)
    rep = _Report()
    gyv = _Guarded(c.B)
    _check(L_.rsx_cin_out_fwd(ptrs, sizes, nl, _p(Wout), _p(bout), _p(gyv.view), c.B, D, _st()), "rsx_cin_out_fwd")
    torch.cuda.synchronize()
    assert gyv.intact() and bool(torch.isfinite(gyv.view).all())
    rep.cmp(cid, "fwd", "y", gyv.view, cr.head_fwd(d), cr.head_fwd(d, "einsum"), cr.head_fwd(d, "torch"))
    # the backward, on a y that also holds exact zeros and negative entries
    y = torch.from_numpy(d.y_bwd).cuda()
    r, re_, rt = cr.head_bwd(d), cr.head_bwd(d, "einsum"), cr.head_bwd(d, "torch")
    logx, g_lin = d.logx.cuda().contiguous(), d.g_lin.cuda()
    for lin in (False, True):
        ggs, gW, gb = _Guarded(c.B), _Guarded(tot), _Guarded(1)
        gn = _Guarded(max(c.nnum, 1), NAN if (lin and c.nnum) else SENTINEL)
        if lin:
            rider = (_p(logx), _p(g_lin), _p(gn.view), c.nnum) if c.nnum else (None, None, None, 0)
            _check(L_.rsx_cin_out_bwd_lin(ptrs, sizes, nl, _p(y), _p(gy), _p(ggs.view), _p(gW.view), _p(gb.view), *rider, c.B, D, _st()),
                   "rsx_cin_out_bwd_lin")
        else:
            _check(L_.rsx_cin_out_bwd(ptrs, sizes, nl, _p(y), _p(gy), _p(ggs.view), _p(gW.view), _p(gb.view), c.B, D, _st()),
                   "rsx_cin_out_bwd")
        torch.cuda.synchronize()
        assert ggs.intact() and gW.intact() and gb.intact() and gn.intact(), "an output's neighbours were written"
        tag = "lin" if lin else "bwd"
        got = {"gs": ggs.view, "dWout": gW.view, "dbout": gb.view}
        if lin and c.nnum:
            got["dwnum"] = gn.view
        else:
            assert bool((gn.view == SENTINEL).all()), "dwnum was written without the rider"
        for name, t in got.items():
            assert bool(torch.isfinite(t).all()), "%s keeps a NaN of its prefill" % name
            rep.cmp(cid, tag, name, t, r[name], re_[name], rt[name])
        rep.note(bool((ggs.view[y <= 0] == 0).all()), "%s %s gs: an example with y <= 0 passes its gradient on" % (cid, tag))
    rep.done()
