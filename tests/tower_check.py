"""The comparison of one tower train_step with its fp64 restatement, shared by tests/test_gpu_tower_bn.py (batch-norm) and
tests/test_gpu_tower_nobn.py (without): the tolerances, the borrowed-gate scheme and the printed error table.  Nothing here
touches the HIP library; tests/test_tower_nobn_ref_cpu.py runs it on the CPU against restatements with planted defects.

Tolerances (the project's numbers for this comparison, tests/test_gpu_mlp_fused.py): loss rtol 1e-5; prob rtol 1e-5 / atol 1e-6;
gradients and activations rtol 1e-4 with atol 2e-7 * max|reference| of that tensor (1e-7 absolute where the reference is exactly
zero).  A (case, tensor) may carry a wider atol in `looser`, as a multiple of max|reference|."""
import numpy as np
import torch

from tests import tower_ref as tr


def figure(got, ref):
    """max|got - ref| / max|ref| (the absolute error where the reference is exactly zero)"""
    m = float(ref.abs().max()) if ref.numel() else 0.0
    e = float((got.double() - ref.double()).abs().max()) if ref.numel() else 0.0
    return e / m if m > 0.0 else e


def close(looser, cid, name, got, ref, rtol, atol_rel=None, atol=None):
    """None, or the reason `got` misses `ref` (so that one run reports every tensor of a case)."""
    ref = ref.reshape(got.shape)
    m = float(ref.abs().max())
    if (cid, name) in looser:
        atol = looser[(cid, name)] * m
    elif atol is None:
        atol = atol_rel * m if m > 0.0 else 1e-7       # (reference exactly zero -- B = 1 with batch-norm: 1e-7 absolute)
    try:
        np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=rtol, atol=atol, err_msg=f"{cid} {name}")
    except AssertionError as e:
        return str(e)
    return None


def check_train(case, d, out, masks, tag, *, label, looser, device="cuda"):
    """out (a train_step's outputs: loss, prob, dX, gs0, gs1, grads {name} and, where the form leaves them in memory, a = the
    layers' relu outputs) against the fp64 restatement with the same masks; prints the error table (`label`_ERR lines) first.
    Pre-activations inside TAU take the kernel's gate (out["a"]), at most GATE_CAP of a layer; a form without `a` (the one-launch
    tower) must have none at all (the fused seed rule)."""
    use_s0, use_s1, _, _ = tr.head_flags(case)
    has_a = out.get("a") is not None
    r = tr.run_ref(case, d, masks=masks, device=device)
    assert r.head_near == 0                                             # (the seed rule, the CPU tests of the reference)
    if not has_a:
        assert sum(r.near) == 0, (case.id, r.near)
    elif sum(r.near):                                                   # pre-activations inside TAU: the kernel's gates there
        r = tr.run_ref(case, d, masks=masks, kernel_a=out["a"], device=device)
    for l, n in enumerate(case.widths):
        assert r.near[l] <= tr.GATE_CAP * case.B * n, (case.id, l, r.near[l])
    f32 = tr.run_ref(case, d, masks=masks, gates=r.gates, dtype=torch.float32, device=device)
    pairs = [("loss", out["loss"][0], r.loss, f32.loss), ("prob", out["prob"], r.prob, f32.prob), ("dX", out["dX"], r.dX, f32.dX)]
    if use_s0:
        pairs.append(("gs0", out["gs0"], r.gs0, f32.gs0))
    if use_s1:
        pairs.append(("gs1", out["gs1"], r.gs1, f32.gs1))
    if has_a:
        pairs += [(f"a{l}", out["a"][l], r.a[l], f32.a[l]) for l in range(len(case.widths))]
    pairs += [(k, out["grads"][k], r.grads[k], f32.grads[k]) for k in out["grads"]]
    for name, got, ref, ref32 in pairs:
        print("%s_ERR %-14s %-12s kernel %.3e  fp32-torch %.3e" % (label, tag, name, figure(got.reshape(ref.shape), ref),
                                                                   figure(ref32, ref)))
    cid = tag.split("/")[0]                                             # (the variants of a case run the same step: one bound)
    bad = [close(looser, cid, "loss", out["loss"][0], r.loss, rtol=1e-5, atol=0.0),
           close(looser, cid, "prob", out["prob"], r.prob, rtol=1e-5, atol=1e-6)]
    bad += [close(looser, cid, name, got, ref, rtol=1e-4, atol_rel=2e-7) for name, got, ref, _ in pairs[2:]]
    bad = [b for b in bad if b is not None]
    for b in bad:
        print("%s_FAIL %s: %s" % (label, tag, " ".join(b.split()[:40])))
    assert not bad, "\n".join(bad)
    assert set(out["grads"]) == set(r.grads)
    return r
