"""The batch-norm tower (csrc/tower.hip through recsys_amd.ops.FusedTower: deepfm.py / dcn.py / xdeepfm.py's dense tower) against a
plain torch fp64 autograd restatement, in every dispatch form of rsx_tower_fwd_layer / rsx_tower_head /
rsx_tower_bwd_layer_defer -- tests/tower_ref.py holds the case table (with the kernel each layer was derived to take), the inputs
and the reference; tests/test_tower_ref_cpu.py checks the reference and the inputs' conditions without a GPU.

Compared per case: loss, prob, dX, gs0, gs1, the gradient of EVERY dense variable (so a wrong scale, which Adam's update would
hide from the model-level tests, fails here) and every layer's relu output.  Tolerances: the project's numbers for this comparison
(tests/test_gpu_mlp_fused.py) -- loss rtol 1e-5; prob rtol 1e-5 / atol 1e-6; gradients and activations rtol 1e-4 with
atol 2e-7 * max|reference| of that tensor (1e-7 absolute where the reference is exactly zero: B = 1).  Every comparison prints
max|got - ref| / max|ref| next to the same figure of a plain fp32 torch restatement of the step (profiles/tower_bn_fp64_errors.txt
is one run's table)."""
import numpy as np
import pytest
import torch

from tests import tower_check as tc
from tests import tower_ref as tr

pytestmark = pytest.mark.gpu


def _tower(case, d):
    from recsys_amd.ops import DenseArena, FusedTower
    assert FusedTower.supports(case.k0, case.widths)
    P = DenseArena(tr.param_shapes(case), "cuda")
    P.load({k: v.numpy() for k, v in d["vals"].items()})
    tw = FusedTower(P, "dnn", case.k0, list(case.widths), capacity=case.B, batch_norm=True)
    dev = {k: d[k].cuda() for k in ("X", "s0", "s1", "y")}
    dev["step"] = torch.tensor([tr.RNG_STEP], dtype=torch.int32, device="cuda")
    return P, tw, dev


def _head_kwargs(case, P, dev):
    n = case.widths[-1]
    if case.head == "deepfm":
        return dict(s0=dev["s0"], c0="b1", s1=dev["s1"], relu0=True, relu2=True)
    if case.head == "dcn":      # wd = the first n_last entries of a longer variable (dcn.py: out.W over [tower | cross])
        oW, oG = P["out.W"].detach().view(-1), P["out.W"].grad.view(-1)
        return dict(s0=dev["s0"], head=((oW[:n], oG[:n]), "out.b", None, None), relu0=False, relu2=False)
    return dict(s1=dev["s1"], relu0=False, relu2=True)


def _train(case, P, tw, dev, masks, **extra):
    """One train_step from a zeroed gradient arena -> every output as a copy."""
    P.grad.zero_()
    m = None if masks is None else [t.cuda() for t in masks]
    loss, prob, dX, gs0, gs1 = tw.train_step(dev["X"], dev["y"], case.rate, dev["step"], replicas=case.replicas, masks=m,
                                             seed=tr.HASH_SEED, **_head_kwargs(case, P, dev), **extra)
    torch.cuda.synchronize()
    return dict(loss=loss.clone(), prob=prob.clone(), dX=dX.clone(), gs0=gs0.clone(), gs1=gs1.clone(), grad=P.grad.clone(),
                grads={k: P[k].grad.clone() for k in P.params}, a=[a[:case.B].clone() for a in tw.a])


# Bounds wider than the defaults, per (case, tensor), as a multiple of max|reference|: 4 x the figure of the plain fp32 torch
# restatement for that tensor and case (profiles/tower_bn_fp64_errors.txt, rounded down) -- never taken from the kernels' own error.
# Each is a tensor of a B >= 1030 case with one to three elements, of thousands, that are small themselves (so rtol gives them
# nothing) while their fp32 rounding error is set by the large terms of a sum over the batch or over K: the kernels' figure for
# every one of them is within 1.05 x the fp32 restatement's.
LOOSER = {
    ("splitA", "a2"): 2.38e-6,            # fp32 torch 5.972e-07 (kernel 5.804e-07)
    ("splitA", "a3"): 3.27e-6,            # 8.190e-07 (7.541e-07)
    ("splitA", "dnn.W2"): 4.07e-6,        # 1.019e-06 (6.445e-07)
    ("splitA", "dnn.beta0"): 2.21e-6,     # 5.536e-07 (5.732e-07)
    ("splitB", "a2"): 2.34e-6,            # 5.868e-07 (5.814e-07)
    ("splitB", "dnn.W0"): 3.44e-6,        # 8.620e-07 (4.951e-07)
    ("splitB", "dnn.gamma0"): 2.33e-6,    # 5.829e-07 (5.978e-07)
    ("b4k", "dnn.W0"): 5.81e-6,           # 1.453e-06 (4.113e-07)
    ("b4k", "dnn.W3"): 5.07e-6,           # 1.269e-06 (5.553e-07)
}


def _close(cid, name, got, ref, rtol, atol_rel=None, atol=None):
    return tc.close(LOOSER, cid, name, got, ref, rtol, atol_rel=atol_rel, atol=atol)


def _check_train(case, d, out, masks, tag):
    """out (a train_step's outputs) against the fp64 restatement with the same masks (tests/tower_check.py: the scheme shared
    with the batch-norm-free tower's tests); prints the error table first."""
    return tc.check_train(case, d, out, masks, tag, label="TOWER_BN", looser=LOOSER)


def _case_inputs(cid):
    case = tr.CASE[cid]
    return case, tr.draw(case, tr.case_seed(case))


@pytest.mark.parametrize("cid", [c.id for c in tr.CASES])
def test_train_step_matches_fp64(cid):
    case, d = _case_inputs(cid)
    P, tw, dev = _tower(case, d)
    extra, bufs = {}, None
    if cid == "default":        # caller-owned output buffers (the data-parallel send block's views)
        bufs = (torch.full((case.B, case.k0), float("nan"), device="cuda"), torch.full((case.B,), float("nan"), device="cuda"),
                torch.full((case.B,), float("nan"), device="cuda"))
        extra["outs"] = bufs
    out = _train(case, P, tw, dev, d["masks"], **extra)
    if bufs is not None:
        assert torch.equal(out["dX"], bufs[0]) and torch.equal(out["gs0"], bufs[1]) and torch.equal(out["gs1"], bufs[2])
    _check_train(case, d, out, d["masks"], cid)
    if case.head == "dcn":      # the entries of out.W behind the tower's belong to someone else: untouched
        assert not bool(out["grads"]["out.W"].reshape(-1)[case.widths[-1]:].any())
    assert tw.dw_jobs_pending == []
    if cid == "b1":             # variance 0: BN output = beta, nothing flows back through the statistics
        for l in range(len(case.widths)):
            assert float(out["grads"][f"dnn.W{l}"].abs().max()) <= 1e-7 and float(out["grads"][f"dnn.b{l}"].abs().max()) <= 1e-7
        assert float(out["dX"].abs().max()) <= 1e-7


def test_layer_done_callback_reduces_every_layer_at_once_in_order():
    """layer_done: no deferred dW reduce although nl <= 4 -- both reduce kernels launched directly behind their layer -- and the
    calls come in the order L-1 .. 0."""
    case, d = _case_inputs("splitA")
    P, tw, dev = _tower(case, d)
    calls = []
    out = _train(case, P, tw, dev, d["masks"], layer_done=calls.append)
    assert calls == [3, 2, 1, 0]
    assert tw.dw_jobs_pending == []
    _check_train(case, d, out, d["masks"], "splitA/done")


@pytest.mark.parametrize("cid", tr.HASH_CASES)
def test_in_kernel_dropout_is_the_documented_hash(cid):
    """masks=None: every kernel that evaluates the keep mask (small and large forward A-loads, the head, the d(input) epilogues
    and dW loads of both backward kernels) must evaluate the documented hash of (seed, step, layer - 1, b * n + col): the step equals,
    bit for bit, the same step with the host's restatement of that hash injected."""
    case, d = _case_inputs(cid)
    P, tw, dev = _tower(case, d)
    a = _train(case, P, tw, dev, None)
    hm = tr.hash_masks(case.B, case.widths, case.rate)
    keep = float(torch.cat([m.reshape(-1) for m in hm]).mean())
    assert abs(keep - (1.0 - case.rate)) < 0.05 + 1.0 / np.sqrt(case.B * sum(case.widths))
    b = _train(case, P, tw, dev, hm)
    for k in ("loss", "prob", "dX", "gs0", "gs1", "grad"):
        assert torch.equal(a[k], b[k]), k
    for l in range(len(case.widths)):
        assert torch.equal(a["a"][l], b["a"][l]), l
    assert bool(torch.isfinite(a["grad"]).all()) and float(a["grad"].abs().max()) > 0.0
    for l in range(len(case.widths) - 1):      # (not the all-ones mask: the next layer's input depends on it)
        assert not bool(hm[l].all())


@pytest.mark.parametrize("cid", tr.INFER_CASES)
def test_infer_matches_fp64_and_leaves_training_alone(cid):
    """FusedTower.infer (BN with mean 0 / variance 1 through hand-encoded statistics rows, no dropout) against the fp64 EVAL forward;
    a train_step on the same tower afterwards still matches fp64: the eval rows do not leak into training."""
    case, d = _case_inputs(cid)
    P, tw, dev = _tower(case, d)
    kw = _head_kwargs(case, P, dev)
    prob, loss = tw.infer(dev["X"], dev["step"], labels=dev["y"], **kw)
    torch.cuda.synchronize()
    with torch.no_grad():
        r = tr.run_ref(case, d, train=False, device="cuda")
        r32 = tr.run_ref(case, d, train=False, dtype=torch.float32, device="cuda")
    for name, got, ref, ref32 in (("loss", loss[0], r.loss, r32.loss), ("prob", prob, r.prob, r32.prob)):
        print("TOWER_BN_ERR %-14s %-12s kernel %.3e  fp32-torch %.3e" % (cid + "/infer", name, tc.figure(got, ref), tc.figure(ref32, ref)))
    bad = [b for b in (_close(cid + "/infer", "loss", loss[0], r.loss, rtol=1e-5, atol=0.0),
                       _close(cid + "/infer", "prob", prob, r.prob, rtol=1e-5, atol=1e-6)) if b is not None]
    assert not bad, "\n".join(bad)
    out = _train(case, P, tw, dev, d["masks"])
    _check_train(case, d, out, d["masks"], cid + "/after")
