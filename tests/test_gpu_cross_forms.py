"""The DCN cross layers (csrc/cross.hip, csrc/cross_device.h, gather_cross_fwd_k of csrc/embedding.hip, the cross rider of
tower_bwd_big_k in csrc/tower.hip) against a plain torch fp64 autograd restatement of dcn/dcn.py:132-142, in every dispatch form --
tests/cross_ref.py holds the case table (with the form each case was derived to take), the inputs and the reference;
tests/test_cross_ref_cpu.py checks the table, the reference and the bounds' teeth without a GPU.

The backward cases call rsx_cross_bwd / rsx_cross_bwd_defer on buffers of the test's own: dX between sentinel blocks, the workspace
(sized by rsx_cross_bwd_workspace_floats) with a sentinel block behind it, dW / dB / dwout prefilled with NaN (they are written, not
added to), dwout a sentinel block where gz is absent.  Each runs dxL only / gz only / both, with accumulate 0 (dX prefilled with NaN)
and 1 (expected = prefill + gradient), on the float32 rounding of the REFERENCE's s, so the backward is judged apart from the
forward; the `own_s` cases also on the kernel's own forward output, as production runs.

Bounds: tests/cross_ref.py (rtol 2e-5 + 2e-7 max|reference| per tensor).  Every comparison prints max|got - ref| / max|ref| next
to the same figure of a plain float32 torch restatement (profiles/cross_fp64_errors.txt is one run's table)."""
import ctypes as C

import pytest
import torch

from tests import cross_ref as cr
from tests import tower_ref as tr

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats: 256 bytes, so the guarded views keep the float4 alignment
SENTINEL = -3.0e33
NAN = float("nan")


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


def _guarded(n, fill, front=True):
    """(whole, view of n floats) with GUARD sentinel floats behind (and in front of) the view"""
    off = GUARD if front else 0
    whole = torch.full((off + n + GUARD,), SENTINEL, device="cuda")
    whole[off:off + n] = fill
    return whole, whole[off:off + n]


def _guards_intact(whole, n, front=True):
    off = GUARD if front else 0
    return bool((whole[:off] == SENTINEL).all()) and bool((whole[off + n:] == SENTINEL).all())


def _dev(d):
    return {k: getattr(d, k).cuda() for k in ("x0", "W", "Bc", "wout", "dxL", "gz")}


class _Report:
    """prints the error table of a case and gathers the misses, so that one run reports every tensor"""

    def __init__(self):
        self.bad = []

    def cmp(self, cid, tag, name, got, ref, ref32, key):
        print("CROSS_ERR %-18s %-10s %-6s kernel %.3e  fp32-torch %.3e" % (cid, tag, name, cr.figure(got, ref), cr.figure(ref32, ref)))
        n = cr.misses(got, ref, key)
        if n:
            self.bad.append("%s %s %s: %d elements outside, figure %.3e" % (cid, tag, name, n, cr.figure(got, ref)))

    def done(self):
        for b in self.bad:
            print("CROSS_FAIL " + b)
        assert not self.bad, "\n".join(self.bad)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("cid", cr.ids_of("fwd"))
def test_cross_fwd_matches_fp64(cid):
    c, d = cr.CASE[cid], cr.draw(cid)
    r, f = cr.run_ref(d), cr.run_ref(d, dtype=torch.float32)
    v = _dev(d)
    rep = _Report()
    for outs in cr.FWD_OUTS:
        s = torch.full((c.B, c.L), NAN, device="cuda")
        wx, xL = _guarded(c.B * c.dim, NAN)
        wz, cz = _guarded(c.B, NAN)
        want_x, want_z = "xL" in outs, "cz" in outs
        _check(_L().rsx_cross_fwd(_p(v["x0"]), _p(v["W"]), _p(v["Bc"]), _p(v["wout"]) if want_z else None, _p(s),
                                  _p(xL) if want_x else None, _p(cz) if want_z else None, c.B, c.dim, c.L, _st()), "rsx_cross_fwd")
        torch.cuda.synchronize()
        assert _guards_intact(wx, c.B * c.dim) and _guards_intact(wz, c.B)
        rep.cmp(cid, outs, "s", s, r.s, f.s, (cid, "fwd", "s"))
        if want_x:
            rep.cmp(cid, outs, "xL", xL, r.xL, f.xL, (cid, "fwd", "xL"))
        else:
            assert bool(torch.isnan(xL).all())
        if want_z:
            rep.cmp(cid, outs, "cz", cz, r.cz, f.cz, (cid, "fwd", "cz"))
        else:
            assert bool(torch.isnan(cz).all())
    rep.done()


@pytest.mark.parametrize("cid", cr.ids_of("gather"))
def test_gather_cross_fwd_matches_fp64(cid):
    """x0 = the gathered rows: E must be exactly them, s and cz the cross layers' of them"""
    c, d = cr.CASE[cid], cr.draw(cid)
    r, f = cr.run_ref(d), cr.run_ref(d, dtype=torch.float32)
    v = _dev(d)
    F = len(c.rows)
    tables, row_off, ids = d.tables.cuda(), d.row_off.cuda(), d.ids.cuda().contiguous()
    we, E = _guarded(c.B * c.dim, NAN)
    s = torch.full((c.B, c.L), NAN, device="cuda")
    wz, cz = _guarded(c.B, NAN)
    _check(_L().rsx_gather_cross_fwd(_p(tables), _p(row_off), _p(ids), _p(E), _p(v["W"]), _p(v["Bc"]), _p(v["wout"]), _p(s), _p(cz),
                                     c.B, F, 16, c.L, _st()), "rsx_gather_cross_fwd")
    torch.cuda.synchronize()
    assert _guards_intact(we, c.B * c.dim) and _guards_intact(wz, c.B)
    assert torch.equal(E.view(c.B, c.dim), v["x0"])
    rep = _Report()
    rep.cmp(cid, "gather", "s", s, r.s, f.s, (cid, "fwd", "s"))
    rep.cmp(cid, "gather", "cz", cz, r.cz, f.cz, (cid, "fwd", "cz"))
    rep.done()


# ------------------------------------------------------------------------------------------------ backward
def _backward(c, v, s, terms, pre, defer):
    """one rsx_cross_bwd (defer: rsx_cross_bwd_defer + rsx_cross_reduce_run) on guarded buffers -> {name: tensor}"""
    from recsys_amd import _lib
    L_ = _L()
    B, dim, Lc = c.B, c.dim, c.L
    wd, dX = _guarded(B * dim, NAN)
    if pre is not None:
        dX.copy_(pre.reshape(-1))
    n_ws = int(L_.rsx_cross_bwd_workspace_floats(B, dim, Lc))
    assert n_ws >= c.RT * (2 * Lc + 1) * dim
    ww, ws = _guarded(n_ws, NAN, front=False)
    dW, dB = torch.full((Lc, dim), NAN, device="cuda"), torch.full((Lc, dim), NAN, device="cuda")
    wo, dwo = _guarded(dim, NAN if "z" in terms else SENTINEL)
    args = (_p(v["x0"]), _p(v["W"]), _p(v["Bc"]), _p(s), _p(v["dxL"]) if "x" in terms else None, _p(v["gz"]) if "z" in terms else None,
            _p(v["wout"]) if "z" in terms else None, _p(dX), int(pre is not None), _p(dW), _p(dB), _p(dwo), _p(ws), B, dim, Lc)
    if defer:
        job = _lib.CrossReduceJob()
        _check(L_.rsx_cross_bwd_defer(*args, C.byref(job), _st()), "rsx_cross_bwd_defer")
        assert (job.RT, job.n) == (c.RT, (2 * Lc + 1) * dim) and job.RT * job.n <= n_ws
        _check(L_.rsx_cross_reduce_run(C.byref(job), _st()), "rsx_cross_reduce_run")
    else:
        _check(L_.rsx_cross_bwd(*args, _st()), "rsx_cross_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(wd, B * dim), "dX's neighbours were written"
    assert _guards_intact(ww, n_ws, front=False), "the workspace was overrun"
    assert _guards_intact(wo, dim)
    out = {"dX": dX.view(B, dim), "dW": dW, "dB": dB}
    if "z" in terms:
        out["dwout"] = dwo
    else:
        assert bool((dwo == SENTINEL).all()), "dwout was written without gz"
    return out


@pytest.mark.parametrize("cid", cr.ids_of("bwd"))
def test_cross_bwd_matches_fp64(cid):
    c, d = cr.CASE[cid], cr.draw(cid)
    assert cr.bwd_form(c.B, c.dim, c.L)[0] == c.form
    v = _dev(d)
    s_ref = cr.run_ref(d).s.to(torch.float32).cuda()
    runs = [("ref", s_ref, False)]
    if c.defer:
        runs.append(("defer", s_ref, True))
    if c.own_s:
        s_own = torch.empty(c.B, c.L, device="cuda")
        _check(_L().rsx_cross_fwd(_p(v["x0"]), _p(v["W"]), _p(v["Bc"]), None, _p(s_own), None, None, c.B, c.dim, c.L, _st()), "rsx_cross_fwd")
        runs.append(("own", s_own, False))
    rep = _Report()
    for terms in cr.TERMS:
        r, f = cr.run_ref(d, terms), cr.run_ref(d, terms, dtype=torch.float32)
        pre = cr.prefill(d, r.dX)
        for acc in (0, 1):
            want, want32 = cr.tensors(r, terms, pre if acc else None), cr.tensors(f, terms, pre if acc else None)
            got_ref = None
            for tag, s, defer in runs:
                got = _backward(c, v, s, terms, pre.cuda() if acc else None, defer)
                assert set(got) == set(want)
                for name in want:
                    rep.cmp(cid, "%s/%d/%s" % (terms, acc, tag), name, got[name], want[name], want32[name], (cid, terms, name))
                if tag == "ref":
                    got_ref = got
                elif tag == "defer":            # the deferred reduce is the same launch later: the same bits
                    for name in want:
                        assert torch.equal(got[name], got_ref[name]), (terms, acc, name)
    rep.done()


# ------------------------------------------------------------------------------------------------ capacity != batch
@pytest.mark.parametrize("dim,Lc,cap,batches", cr.CAPACITY_CASES)
def test_cross_layers_runs_any_batch_up_to_its_capacity(dim, Lc, cap, batches):
    """CrossLayers sizes its workspace once, for its capacity; a smaller batch may write MORE partials than the capacity does (2 000
    examples through the one-wave form: 1 000 partials; 3 000: 750).  The job's partials must fit the workspace, and the result must
    be the reference's."""
    from recsys_amd import _lib
    from recsys_amd.ops import CrossLayers
    op = CrossLayers(dim, Lc, cap)
    rep = _Report()
    for B in batches:
        cid = "cap%d/%dx%dx%d" % (cap, B, dim, Lc)
        d = cr.draw_shape(B, dim, Lc, 77000 + B)
        r, f = cr.run_ref(d), cr.run_ref(d, dtype=torch.float32)
        v = _dev(d)
        s, _, cz = op.forward(v["x0"], v["W"], v["Bc"], wout=v["wout"])
        dW, dB = torch.full((Lc, dim), NAN, device="cuda"), torch.full((Lc, dim), NAN, device="cuda")
        dwo, dX = torch.full((dim,), NAN, device="cuda"), torch.full((B, dim), NAN, device="cuda")
        job = op.backward(v["x0"], v["W"], v["Bc"], dW, dB, dX, False, dxL=v["dxL"], gz=v["gz"], wout=v["wout"], dwout=dwo,
                          defer_reduce=True)
        form = cr.bwd_form(B, dim, Lc)
        assert (job.RT, job.n) == (form[2], (2 * Lc + 1) * dim)
        assert job.RT * job.n <= op.ws.numel(), (job.RT, job.n, op.ws.numel())
        _check(_L().rsx_cross_reduce_run(C.byref(job), _st()), "rsx_cross_reduce_run")
        torch.cuda.synchronize()
        rep.cmp(cid, "xz/0/own", "s", s, r.s, f.s, None)
        rep.cmp(cid, "xz/0/own", "cz", cz, r.cz, f.cz, None)
        want, want32 = cr.tensors(r, "xz"), cr.tensors(f, "xz")
        for name, got in (("dX", dX), ("dW", dW), ("dB", dB), ("dwout", dwo)):
            rep.cmp(cid, "xz/0/own", name, got, want[name], want32[name], None)
    rep.done()


# ------------------------------------------------------------------------------------------------ the rider
def _rider_inputs(c):
    """the tower's case (tests/tower_ref.py, dcn head, out.W = [n_last tower weights | dim cross weights]) and the cross layers'
    inputs sharing x0 and wout with it"""
    tcase = tr.Case(c.id, c.B, c.dim, c.widths, c.rate, "dcn", 1, c.seed % (1 << 31), c.dim)
    d = dict(tr.draw(tcase, tcase.base_seed))
    dc = cr.draw(c.id)
    d["X"] = dc.x0                                                  # 0.5 N(0,1), as every cross case
    di = cr.Inputs()
    di.B, di.dim, di.L = c.B, c.dim, c.L
    di.x0, di.W, di.Bc = dc.x0, dc.W, dc.Bc
    di.wout = d["vals"]["out.W"].reshape(-1)[c.widths[-1]:].contiguous()      # N(0,1) / sqrt(n_last + dim)
    di.dxL, di.gz = None, None
    return tcase, d, di


def _rider_step(c, tcase, d, di, ride):
    """one dcn.py step of tower + cross layers wired as dcn._train_fused wires it; ride: the cross backward inside the tower's last
    backward launch, else the launch of its own adding onto the tower's dX afterwards -> every output as a copy"""
    from recsys_amd.ops import CrossLayers, DenseArena, FusedTower
    assert FusedTower.supports(tcase.k0, tcase.widths)
    shapes = dict(tr.param_shapes(tcase))
    shapes["cross.W"], shapes["cross.b"] = (c.L, c.dim), (c.L, c.dim)
    P = DenseArena(shapes, "cuda")
    vals = {k: v.numpy() for k, v in d["vals"].items()}
    vals["cross.W"], vals["cross.b"] = di.W.numpy(), di.Bc.numpy()
    P.load(vals)
    tw = FusedTower(P, "dnn", tcase.k0, list(tcase.widths), capacity=c.B, batch_norm=True)
    op = CrossLayers(c.dim, c.L, c.B)
    assert op.cross_ride_ok(tw, c.B)
    x0, y = d["X"].cuda(), d["y"].cuda()
    step = torch.tensor([tr.RNG_STEP], dtype=torch.int32, device="cuda")
    masks = None if d["masks"] is None else [m.cuda() for m in d["masks"]]
    nh = tcase.widths[-1]
    P.grad.zero_()
    oW, oG = P["out.W"].detach().view(-1), P["out.W"].grad.view(-1)
    s, _, cz = op.forward(x0, P["cross.W"], P["cross.b"], wout=oW[nh:])
    rider = op.rider_args(x0, P["cross.W"], P["cross.b"], P["cross.W"].grad, P["cross.b"].grad, oW[nh:], oG[nh:]) if ride else None
    loss, prob, dX, gs0, _ = tw.train_step(x0, y, tcase.rate, step, s0=cz, head=((oW[:nh], oG[:nh]), "out.b", None, None), relu0=False,
                                           relu2=False, replicas=1, masks=masks, seed=tr.HASH_SEED, cross_rider=rider)
    if ride:
        job = tw.cross_job_pending
        assert (job.RT, job.n) == (c.RT, (2 * c.L + 1) * c.dim) and job.RT * job.n <= op.ws.numel()
        _check(_L().rsx_cross_reduce_run(C.byref(job), _st()), "rsx_cross_reduce_run")
    else:
        op.backward(x0, P["cross.W"], P["cross.b"], P["cross.W"].grad, P["cross.b"].grad, dX, True, gz=gs0, wout=oW[nh:], dwout=oG[nh:])
    torch.cuda.synchronize()
    return dict(loss=loss.clone(), prob=prob.clone(), dX=dX.clone(), gs0=gs0.clone(), s=s.clone(), cz=cz.clone(),
                grads={k: P[k].grad.clone() for k in P.params}, a=[a[:c.B].clone() for a in tw.a])


@pytest.mark.parametrize("cid", cr.ids_of("rider"))
def test_cross_rider_matches_fp64_and_the_separate_launch(cid):
    c = cr.CASE[cid]
    assert cr.rider_form(c.B, c.dim, c.L, c.widths)[:3] == (c.ntd, c.epw, c.RT)
    tcase, d, di = _rider_inputs(c)
    nh = tcase.widths[-1]
    a, b = _rider_step(c, tcase, d, di, True), _rider_step(c, tcase, d, di, False)
    # the rider is the same arithmetic in another launch (include/rsx.h): every output, the tower's own gradients included, bit for
    # bit -- the two copies of the examples-per-wave rule (tower.hip p.xr_epw, cross.hip cross_epw4) disagreeing would show here
    for k in ("loss", "prob", "dX", "gs0", "s", "cz"):
        assert torch.equal(a[k], b[k]), k
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    for l in range(len(tcase.widths)):
        assert torch.equal(a["a"][l], b["a"][l]), l
    # against fp64, end to end: the tower with s0 = the reference's cz, the cross layers with gz = the reference's gs0
    def ref(dtype, gates=None):
        to = lambda t: t.to(dtype)
        _, _, cz = cr.forward(to(di.x0), to(di.W), to(di.Bc), to(di.wout))
        d2 = dict(d)
        d2["s0"] = cz
        r = tr.run_ref(tcase, d2, masks=d["masks"], dtype=dtype, device="cuda", gates=gates)
        if gates is None and sum(r.near):
            r = tr.run_ref(tcase, d2, masks=d["masks"], kernel_a=a["a"], dtype=dtype, device="cuda")
        rc = cr.run_ref(di, "z", dtype=dtype, gz=r.gs0.cpu())
        return r, rc
    r, rc = ref(torch.float64)
    assert r.head_near == 0
    for l, n in enumerate(tcase.widths):
        assert r.near[l] <= tr.GATE_CAP * c.B * n, (cid, l, r.near[l])
    f, fc = ref(torch.float32, gates=r.gates)
    rep = _Report()
    rep.cmp(cid, "rider", "dX", a["dX"], r.dX.cpu() + rc.dX, f.dX.cpu() + fc.dX, (cid, "rider", "dX"))
    rep.cmp(cid, "rider", "dW", a["grads"]["cross.W"], rc.dW, fc.dW, (cid, "rider", "dW"))
    rep.cmp(cid, "rider", "dB", a["grads"]["cross.b"], rc.dB, fc.dB, (cid, "rider", "dB"))
    rep.cmp(cid, "rider", "dwout", a["grads"]["out.W"].reshape(-1)[nh:], rc.dwout, fc.dwout, (cid, "rider", "dwout"))
    rep.done()
