"""The batch-norm-free tower (recsys_amd.ops.FusedTower(batch_norm=False): din.py's 'mlp_layer') against a plain torch fp64 autograd
restatement, in BOTH of its forms and every dispatch form of each:

  * launch per layer -- the gamma == nullptr / gamma_prev == nullptr branches of csrc/tower.hip (small and big forward, head, both
    backward kernels, the split and the deferred dW reduce), forced with RSX_FORMS=mlp_fuse=0 or taken because the widths are outside
    the one-launch envelope (tests/tower_ref.py NOBN_CASES, with the kernel each layer was derived to take);
  * one launch -- csrc/mlp_fused.hip (tests/tower_ref.py FUSED_CASES): depth, k-step parity of both tile loops, column tiles,
    the LDS sizes on both sides of 64 KB, batch sizes around the tile and around the reduce's loads in flight, and its deferred,
    riding and re-used-workspace forms bit for bit against the default.

Compared per case: loss, prob, dX, gs0, the gradient of EVERY dense variable (a wrong scale, which Adam's update would hide from
the model-level tests, fails here) and, launch per layer, every layer's relu output.  Tolerances and the borrowed-gate scheme:
tests/tower_check.py.  The one-launch form keeps its activations in LDS, so there is no kernel gate to borrow: its cases' seeds have
no pre-activation within TAU of zero at all (tests/test_tower_nobn_ref_cpu.py pins them).  Every comparison prints
max|got - ref| / max|ref| next to the same figure of a plain fp32 torch restatement (profiles/tower_nobn_fp64_errors.txt is one
run's table)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tower_check as tc
from tests import tower_ref as tr

pytestmark = pytest.mark.gpu

HEAD = ("mlp.Wout", "mlp.bout", None, None)

# Bounds wider than the defaults, per (case, tensor), as a multiple of max|reference|: 4 x the figure of the plain fp32 torch
# restatement for that tensor and case (profiles/tower_nobn_fp64_errors.txt, rounded down) -- the margin and the rule of
# tests/test_gpu_tower_bn.py's LOOSER, never taken from the kernels' own error.  None was needed: every tensor of every case is
# inside the default bound.
LOOSER = {}


def _tower(case, d, capacity=None):
    from recsys_amd.ops import DenseArena, FusedTower
    assert FusedTower.supports(case.k0, case.widths)
    P = DenseArena(tr.param_shapes(case), "cuda")
    P.load({k: v.numpy() for k, v in d["vals"].items()})
    tw = FusedTower(P, "mlp", case.k0, list(case.widths), capacity=capacity or case.B, batch_norm=False)
    dev = {k: d[k].cuda() for k in ("X", "s0", "y")}
    dev["step"] = torch.tensor([tr.RNG_STEP], dtype=torch.int32, device="cuda")
    return P, tw, dev


def _train(case, P, tw, dev, masks, B=None, **extra):
    """One train_step (on the first B rows) from a zeroed gradient arena -> every output as a copy."""
    B = case.B if B is None else B
    P.grad.zero_()
    m = None if masks is None else [t[:B].contiguous().cuda() for t in masks]
    fused = tw._mlp_fused_ok()
    loss, prob, dX, gs0, _ = tw.train_step(dev["X"][:B], dev["y"][:B], case.rate, dev["step"], s0=dev["s0"][:B] if case.s0 else None,
                                           head=HEAD, relu0=False, relu2=False, replicas=case.replicas, masks=m,
                                           seed=tr.HASH_SEED, **extra)
    torch.cuda.synchronize()
    return dict(loss=loss.clone(), prob=prob.clone(), dX=dX.clone(), gs0=gs0.clone(), grad=P.grad.clone(),
                grads={k: P[k].grad.clone() for k in P.params}, a=None if fused else [a[:B].clone() for a in tw.a])


def _check_train(case, d, out, masks, tag):
    return tc.check_train(case, d, out, masks, tag, label="TOWER_NOBN", looser=LOOSER)


def _assert_pad_units_have_zero_gradients(case, out):
    """din.py's stored units without a counterpart in the model (pre-activation exactly 0, gate 0): zero by VALUE."""
    l, n = case.pad
    nxt = f"mlp.W{l + 1}" if l + 1 < len(case.widths) else "mlp.Wout"
    for name, g in ((f"mlp.W{l}", out["grads"][f"mlp.W{l}"][:, n:]), (f"mlp.b{l}", out["grads"][f"mlp.b{l}"][n:]),
                    (nxt, out["grads"][nxt][n:])):
        assert g.numel() > 0 and bool((g == 0).all()), (case.id, name)


def _same(a, b, keys=("loss", "prob", "dX", "gs0", "grad")):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


# ============================================================================================= launch per layer
def _per_layer(monkeypatch, cid):
    case = tr.NOBN_CASE[cid]
    if cid != "fallback":          # (fallback: default forms -- rsx_mlp_nobn_supported has to say no by itself)
        monkeypatch.setenv("RSX_FORMS", "mlp_fuse=0")
    d = tr.draw(case, tr.case_seed(case))
    P, tw, dev = _tower(case, d)
    assert not tw._mlp_fused_ok()
    return case, d, P, tw, dev


@pytest.mark.parametrize("cid", [c.id for c in tr.NOBN_CASES])
def test_per_layer_train_step_matches_fp64(cid, monkeypatch):
    case, d, P, tw, dev = _per_layer(monkeypatch, cid)
    extra, big = {}, None
    if cid == "grouped":        # caller-owned outputs (din.py: gs0 is a slice of the scatter's first-order block): its neighbours stay
        big = torch.full((case.B + 16,), -7.5, device="cuda")
        bufs = (torch.full((case.B, case.k0), float("nan"), device="cuda"), big[8:8 + case.B], None)
        extra["outs"] = bufs
    out = _train(case, P, tw, dev, d["masks"], **extra)
    if big is not None:
        assert torch.equal(out["dX"], bufs[0]) and torch.equal(out["gs0"], bufs[1])
        assert bool((big[:8] == -7.5).all()) and bool((big[8 + case.B:] == -7.5).all())
    _check_train(case, d, out, d["masks"], cid)
    assert tw.dw_jobs_pending == [] and tw.mlp_reduce_job is None
    if cid == "b1":             # no batch statistics: one example has gradients like any other
        for k, g in out["grads"].items():
            assert float(g.abs().max()) > 0.0, k
        assert float(out["dX"].abs().max()) > 0.0 and float(out["gs0"].abs().max()) > 0.0
    if case.pad is not None:
        _assert_pad_units_have_zero_gradients(case, out)


@pytest.mark.parametrize("cid", tr.NOBN_HASH_CASES)
def test_per_layer_in_kernel_dropout_is_the_documented_hash(cid, monkeypatch):
    """masks=None: every kernel that evaluates the keep mask without batch-norm (small and big forward A-loads, the head, the
    d(input) epilogues and dW loads of both backward kernels) evaluates the documented hash: the step equals, bit for bit, the
    same step with the host's restatement of that hash injected."""
    case, d, P, tw, dev = _per_layer(monkeypatch, cid)
    a = _train(case, P, tw, dev, None)
    hm = tr.hash_masks(case.B, case.widths, case.rate)
    b = _train(case, P, tw, dev, hm)
    _same(a, b, ("loss", "prob", "dX", "grad") + (("gs0",) if case.s0 else ()))
    for l in range(len(case.widths)):
        assert torch.equal(a["a"][l], b["a"][l]), l
        assert not bool(hm[l].all())
    assert bool(torch.isfinite(a["grad"]).all()) and float(a["grad"].abs().max()) > 0.0
    if case.pad is not None:
        _assert_pad_units_have_zero_gradients(case, a)


@pytest.mark.parametrize("cid", tr.NOBN_INFER_CASES)
def test_per_layer_infer_matches_fp64_and_leaves_training_alone(cid, monkeypatch):
    """FusedTower.infer without batch-norm (no dropout, no statistics) against the fp64 EVAL forward; a train_step on the same
    tower afterwards still matches fp64."""
    case, d, P, tw, dev = _per_layer(monkeypatch, cid)
    prob, loss = tw.infer(dev["X"], dev["step"], labels=dev["y"], s0=dev["s0"] if case.s0 else None, head=HEAD, relu0=False,
                          relu2=False)
    torch.cuda.synchronize()
    with torch.no_grad():
        r = tr.run_ref(case, d, train=False, device="cuda")
        r32 = tr.run_ref(case, d, train=False, dtype=torch.float32, device="cuda")
    for name, got, ref, ref32 in (("loss", loss[0], r.loss, r32.loss), ("prob", prob, r.prob, r32.prob)):
        print("TOWER_NOBN_ERR %-14s %-12s kernel %.3e  fp32-torch %.3e" % (cid + "/infer", name, tc.figure(got, ref),
                                                                          tc.figure(ref32, ref)))
    bad = [b for b in (tc.close(LOOSER, cid + "/infer", "loss", loss[0], r.loss, rtol=1e-5, atol=0.0),
                       tc.close(LOOSER, cid + "/infer", "prob", prob, r.prob, rtol=1e-5, atol=1e-6)) if b is not None]
    assert not bad, "\n".join(bad)
    out = _train(case, P, tw, dev, d["masks"])
    _check_train(case, d, out, d["masks"], cid + "/after")


# ============================================================================================= one launch
def _fused(cid):
    case = tr.FUSED_CASE[cid]
    seed = tr.case_seed(case)
    assert seed == tr.FUSED_SEEDS[cid]
    d = tr.draw(case, seed)
    P, tw, dev = _tower(case, d)
    assert tw._mlp_fused_ok()
    return case, d, P, tw, dev


@pytest.mark.parametrize("cid", [c.id for c in tr.FUSED_CASES])
def test_fused_train_step_matches_fp64(cid):
    """Hash-dropout cases (FUSED_HASH) run with masks=None and are compared with the reference under hash_masks(..., layer0=0)."""
    case, d, P, tw, dev = _fused(cid)
    out = _train(case, P, tw, dev, None if cid in tr.FUSED_HASH else d["masks"])
    _check_train(case, d, out, tr.case_masks(case, d), cid)
    assert tw.mlp_reduce_job is None and tw.dw_jobs_pending == []
    if case.pad is not None:
        _assert_pad_units_have_zero_gradients(case, out)


@pytest.mark.parametrize("cid", ["f_l1", "f_112", "f_din", "f_din520"])
def test_fused_in_kernel_dropout_is_the_documented_hash(cid):
    case, d, P, tw, dev = _fused(cid)
    a = _train(case, P, tw, dev, None)
    hm = tr.hash_masks(case.B, case.widths, case.rate)
    keep = float(torch.cat([m.reshape(-1) for m in hm]).mean())
    assert abs(keep - (1.0 - case.rate)) < 0.05 + 1.0 / np.sqrt(case.B * sum(case.widths))
    b = _train(case, P, tw, dev, hm)
    _same(a, b, ("loss", "prob", "dX", "grad") + (("gs0",) if case.s0 else ()))
    assert bool(torch.isfinite(a["grad"]).all()) and float(a["grad"].abs().max()) > 0.0
    if case.pad is not None:
        _assert_pad_units_have_zero_gradients(case, a)


def mlp_step_struct(case, P, tw, dev, masks, defer):
    """The rsx_mlp_step of the case on the tower's buffers, as FusedTower.train_step fills it."""
    from recsys_amd import _lib
    B = case.B
    mk = tw._masks(B, case.rate, None if masks is None else [m.cuda() for m in masks])
    ms = _lib.MlpStep()
    ms.X, ms.B, ms.K0, ms.L = dev["X"].data_ptr(), B, case.k0, len(case.widths)
    for l, n in enumerate(case.widths):
        ms.W[l], ms.b[l] = P[f"mlp.W{l}"].data_ptr(), P[f"mlp.b{l}"].data_ptr()
        ms.dW[l], ms.db[l] = P[f"mlp.W{l}"].grad.data_ptr(), P[f"mlp.b{l}"].grad.data_ptr()
        ms.masks[l] = None if mk[l] is None else mk[l].data_ptr()
        ms.widths[l] = n
    ms.wout, ms.bout = P["mlp.Wout"].data_ptr(), P["mlp.bout"].data_ptr()
    ms.dwout, ms.dbout = P["mlp.Wout"].grad.data_ptr(), P["mlp.bout"].grad.data_ptr()
    ms.s0 = dev["s0"].data_ptr() if case.s0 else None
    ms.labels, ms.rng_step = dev["y"].data_ptr(), dev["step"].data_ptr()
    ms.prob, ms.dX, ms.gs0 = tw.prob.data_ptr(), tw.dX.data_ptr(), tw.gs0.data_ptr() if case.s0 else None
    ms.workspace, ms.loss = tw._mlp_ws.data_ptr(), tw.loss.data_ptr()
    ms.seed, ms.dropout_rate, ms.loss_scale = tr.HASH_SEED, case.rate, 1.0 / (B * case.replicas)
    ms.defer_reduce = 1 if defer else 0
    return ms


@pytest.mark.parametrize("cid", ["f_b1", "f_48", "f_din520", "f_din"])
def test_fused_deferred_reduce_equals_the_default(cid):
    """defer_reduce = 1 leaves every weight gradient and the loss alone until rsx_mlp_nobn_reduce, which then writes what the
    default form's second launch writes, bit for bit."""
    from recsys_amd import _lib
    from recsys_amd.ops import _stream
    L = _lib.lib()
    case, d, P, tw, dev = _fused(cid)
    masks = None if cid in tr.FUSED_HASH else d["masks"]
    want = _train(case, P, tw, dev, masks)
    P.grad.fill_(-3.25)
    tw.loss.fill_(-3.25)
    tw.dX.fill_(float("nan"))
    tw.prob.fill_(float("nan"))
    ms = mlp_step_struct(case, P, tw, dev, masks, defer=True)
    _lib.check(L.rsx_mlp_nobn_train_step(C.byref(ms), _stream()), "rsx_mlp_nobn_train_step")
    torch.cuda.synchronize()
    assert bool((P.grad == -3.25).all()) and float(tw.loss[0]) == -3.25
    assert torch.equal(tw.dX[:case.B], want["dX"]) and torch.equal(tw.prob[:case.B], want["prob"])
    _lib.check(L.rsx_mlp_nobn_reduce(C.byref(ms), _stream()), "rsx_mlp_nobn_reduce")
    torch.cuda.synchronize()
    assert torch.equal(tw.loss, want["loss"])
    for k in P.params:
        assert torch.equal(P[k].grad, want["grads"][k]), k


def tiny_pool_args(K=8, B=3, P=5, seed=5):
    """A small pooling-backward problem for a rider to ride in: (args of rsx_din_pool_bwd_pair[_ride] up to ld_dH, the tensors)."""
    g = torch.Generator().manual_seed(seed)
    t = {}
    for h in (0, 1):
        t[f"H{h}"] = torch.randn(B, P, K, generator=g).cuda()
        t[f"w{h}"] = torch.randn(B, P, generator=g).cuda()
        t[f"ids{h}"] = torch.randint(0, 4, (B, P), generator=g, dtype=torch.int32).cuda()
        t[f"dout{h}"] = torch.randn(B, K, generator=g).cuda()
        t[f"dH{h}"] = torch.zeros(B, P, K, device="cuda")
        t[f"dw{h}"] = torch.zeros(B, P, device="cuda")
    ptrs = [t[f"{n}{h}"].data_ptr() for h in (0, 1) for n in ("H", "w", "ids", "dout", "dH", "dw")]
    return ptrs + [0, B, P, K, K, K], t


@pytest.mark.parametrize("cid", ["f_b1", "f_din520", "f_max"])
def test_fused_reduce_as_a_rider_of_the_pooling_backward_equals_the_default(cid):
    """reduce_rider: the reduce as extra workgroups of rsx_din_pool_bwd_pair_ride (mlp_reduce_body<16> instead of <32>: another
    number of loads in flight, the same ascending workgroup order, the loss summed in fp64) -- bit for bit the default's
    gradients and loss, and the launch it rides in computes what the plain pair launch computes."""
    from recsys_amd import _lib
    from recsys_amd.ops import _stream
    L = _lib.lib()
    case, d, P, tw, dev = _fused(cid)
    masks = None if cid in tr.FUSED_HASH else d["masks"]
    want = _train(case, P, tw, dev, masks)
    got = _train(case, P, tw, dev, masks, reduce_rider=True)
    job = tw.mlp_reduce_job
    assert job is not None and job.e4_last > 0 and job.nwg == (case.B + 15) // 16
    assert not bool(got["grad"].any())                      # (zeroed by _train: nothing reduced yet)
    _same(got, want, ("prob", "dX") + (("gs0",) if case.s0 else ()))
    P.grad.fill_(-3.25)
    tw.loss.fill_(-3.25)
    args, t = tiny_pool_args()
    _lib.check(L.rsx_din_pool_bwd_pair(*args, _stream()), "rsx_din_pool_bwd_pair")
    torch.cuda.synchronize()
    pool_want = {k: t[k].clone() for k in ("dH0", "dw0", "dH1", "dw1")}
    assert bool((P.grad == -3.25).all())
    for k in pool_want:
        t[k].fill_(float("nan"))
    _lib.check(L.rsx_din_pool_bwd_pair_ride(*args, C.byref(job), _stream()), "rsx_din_pool_bwd_pair_ride")
    torch.cuda.synchronize()
    for k in pool_want:
        assert torch.equal(t[k], pool_want[k]), k
    assert torch.equal(tw.loss, want["loss"])
    for k in P.params:
        assert torch.equal(P[k].grad, want["grads"][k]), k


def test_fused_tower_reused_at_smaller_batches_equals_fresh_towers():
    """din.py's tower has the capacity of the full batch and meets smaller ones (an epoch's last batch): the partials of the
    larger batch's workgroups are still in the workspace and must not be summed.  Capacity 1024 at B = 1000 and then at B = 37
    against fresh towers of those capacities, bit for bit (hash dropout: element b * n + c does not depend on the batch)."""
    case = tr.FUSED_CASE["f_din"]._replace(id="cap1024", B=1024)
    d = tr.draw(case, case.base_seed)
    P, tw, dev = _tower(case, d)
    assert tw._mlp_fused_ok()
    full = _train(case, P, tw, dev, None)
    assert bool(torch.isfinite(full["grad"]).all())
    for B in (1000, 37):
        got = _train(case, P, tw, dev, None, B=B)
        P2, tw2, dev2 = _tower(case, d, capacity=B)
        assert tw2._mlp_fused_ok()
        want = _train(case, P2, tw2, dev2, None, B=B)
        _same(got, want)
        assert not torch.equal(got["grad"], full["grad"])
