"""The fp64 reference of tests/test_gpu_tower_bn.py, checked without a GPU: every case's inputs satisfy the two conditions the
GPU comparison rests on (no head row on a relu kink for the case's seed, at most GATE_CAP of a layer's pre-activations within
TAU of zero), the restatement's gradients are the oracle's (oracle.models.tower_fwd / tower_bwd in float64), and the host
restatement of the dropout hash is the one tests/test_gpu_embedding.py states."""
import numpy as np
import pytest
import torch

from oracle import models
from tests import tower_ref as tr


@pytest.mark.parametrize("cid", [c.id for c in tr.CASES])
def test_case_inputs_satisfy_the_seed_rule_and_the_gate_cap(cid):
    case = tr.CASE[cid]
    seed = tr.case_seed(case)
    assert case.base_seed <= seed < case.base_seed + tr.SEED_TRIES
    d = tr.draw(case, seed)
    r = tr.run_ref(case, d, masks=d["masks"])
    assert r.head_near == 0
    for l, n in enumerate(case.widths):
        assert r.near[l] <= tr.GATE_CAP * case.B * n, (cid, l, r.near[l], case.B * n)
    for t in [r.loss, r.prob, r.dX] + list(r.grads.values()):
        assert bool(torch.isfinite(t).all())
    if d["masks"] is not None:
        keep = float(torch.cat([m.reshape(-1) for m in d["masks"]]).mean())
        assert abs(keep - (1.0 - case.rate)) < 0.1


def test_case_table_is_inside_the_fused_envelope_and_has_every_head_form_on_both_sides():
    for c in tr.CASES:       # (FusedTower.supports, restated: the GPU test would otherwise fail at construction)
        assert c.k0 % 4 == 0 and all(w % 4 == 0 for w in c.widths[:-1]) and c.widths[-1] <= 256, c.id
    for form in ("deepfm", "dcn", "nos0"):
        assert any(c.head == form and c.B <= 512 for c in tr.CASES) and any(c.head == form and c.B >= 1024 for c in tr.CASES)
    assert sum(c.replicas == 2 for c in tr.CASES) >= 2
    assert {c.rate for c in tr.CASES} == {0.0, 0.3, 0.5}
    assert all(tr.CASE[i].rate > 0.0 for i in tr.HASH_CASES)


@pytest.mark.parametrize("cid", ["tiny17", "edge512"])
def test_restatement_gradients_are_the_oracles(cid):
    """The sum head (z = s0 + h . wd + bd) by hand around oracle.models.tower_fwd / tower_bwd, all in float64."""
    case = tr.CASE[cid]
    d = tr.draw(case, tr.case_seed(case))
    r = tr.run_ref(case, d, masks=d["masks"])
    P = {k: v.double().numpy() for k, v in d["vals"].items()}
    masks = [m.double().numpy() for m in d["masks"]]
    nl, n_last = len(case.widths), case.widths[-1]
    h, caches = models.tower_fwd(d["X"].double().numpy(), P, "dnn", nl, True, case.rate, masks)
    wd = P["out.W"].reshape(-1)[:n_last]
    z = d["s0"].double().numpy() + h @ wd + P["out.b"]
    y = d["y"].double().numpy()
    dz = (1.0 / (1.0 + np.exp(-z)) - y) / (case.B * case.replicas)
    grads = {}
    dX = models.tower_bwd(np.outer(dz, wd), P, "dnn", caches, case.rate, grads)
    grads["out.W"] = np.concatenate([h.T @ dz, np.zeros(tr.DCN_TAIL)]).reshape(-1, 1)
    grads["out.b"] = dz.sum(keepdims=True)
    per = np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))
    np.testing.assert_allclose(float(r.loss), per.mean(), rtol=1e-12)
    np.testing.assert_allclose(r.prob.numpy(), 1.0 / (1.0 + np.exp(-z)), rtol=1e-12)
    np.testing.assert_allclose(r.dX.numpy(), dX, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(r.gs0.numpy(), dz, rtol=1e-12)
    assert set(grads) == set(r.grads)
    for k, g in grads.items():
        np.testing.assert_allclose(r.grads[k].numpy(), g.reshape(r.grads[k].shape), rtol=1e-9, atol=1e-15, err_msg=k)
    for l in range(nl):
        np.testing.assert_allclose(r.a[l].numpy(), caches[l][1], rtol=1e-9, atol=1e-13)     # (torch's and numpy's GEMM add in another order)


def test_borrowed_gates_replace_the_fp64_sign_only_inside_tau():
    case = tr.CASE["tiny17"]
    d = tr.draw(case, tr.case_seed(case))
    r = tr.run_ref(case, d, masks=d["masks"])
    lent = [torch.ones_like(a) for a in r.a]                 # a "kernel" that kept every element
    r2 = tr.run_ref(case, d, masks=d["masks"], kernel_a=lent)
    for l in range(len(case.widths)):
        assert r.near[l] == 0 and torch.equal(r.gates[l], r2.gates[l])
    assert torch.equal(r.dX, r2.dX)


def test_host_hash_is_the_documented_one():
    from tests.test_gpu_embedding import _hash32
    x = np.arange(0, 2 ** 32, 65537, dtype=np.uint64)
    assert np.array_equal(tr.hash32(x), _hash32(x))
    B, widths, rate, step, seed = 96, (32, 16), 0.5, 1, 0x5eed
    got = tr.hash_masks(B, widths, rate, step=step, seed=seed)
    for l, n in enumerate(widths):          # (the expression of test_tower_rng_dropout_is_the_documented_hash_and_consistent_fwd_bwd)
        key = _hash32(np.array([(seed ^ ((step * 0x9E3779B9) & 0xFFFFFFFF) ^ ((l * 0x85EBCA6B + 0x27220A95) & 0xFFFFFFFF))]))[0]
        h = _hash32(np.arange(B * n, dtype=np.uint64) ^ key)
        assert np.array_equal(got[l].numpy(), (h >= np.uint64(int(rate * 2 ** 32))).astype(np.float32).reshape(B, n))
