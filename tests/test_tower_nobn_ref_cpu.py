"""The references of tests/test_gpu_tower_nobn.py and tests/test_gpu_din_pool_forms.py, checked without a GPU:

  * every batch-norm-free case's inputs satisfy the rule its comparison rests on (launch per layer: at most GATE_CAP of a layer's
    pre-activations within TAU of zero; one launch: NONE, for the pinned seed, under the masks the test runs with);
  * the one-launch table covers what it claims (depth, k-step parity of both tile loops, column tiles, LDS on both sides of
    64 KB -- the kernel's layout arithmetic restated here and held against rsx_mlp_nobn_supported);
  * a plain fp32 restatement of each step PASSES the comparison helper with the stated tolerances, and the same restatement
    with ONE planted defect FAILS it -- which is how the GPU tests show they would notice a subtly wrong kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import din_pool_ref as pr
from tests import test_gpu_tower_nobn as tn
from tests import tower_check as tc
from tests import tower_ref as tr

ALL = tr.NOBN_CASES + tr.FUSED_CASES


def _inputs(case):
    d = tr.draw(case, tr.case_seed(case))
    return d, tr.case_masks(case, d)


def _as_out(case, f):
    """a restated step in the shape of a train_step's outputs"""
    return dict(loss=f.loss.reshape(1), prob=f.prob, dX=f.dX, gs0=f.gs0, grads=dict(f.grads), a=None if case.fused else list(f.a))


def _fp32_step(case, d, masks, **kw):
    """the stand-in kernel: the same step in fp32, with the gates of ITS OWN pre-activations"""
    return tr.run_ref(case, d, masks=masks, dtype=torch.float32, **kw)


def _check(case, d, out, masks):
    return tc.check_train(case, d, out, masks, case.id, label="TOWER_NOBN_CPU", looser=tn.LOOSER, device="cpu")


# ------------------------------------------------------------------------------------------------ the cases' conditions
@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_case_inputs_satisfy_their_seed_rule(case):
    seed = tr.case_seed(case)
    assert case.base_seed <= seed < case.base_seed + (tr.FUSED_SEED_TRIES if case.fused else tr.SEED_TRIES)
    d, masks = _inputs(case)
    r = tr.run_ref(case, d, masks=masks)
    assert r.head_near == 0
    if case.fused:
        assert seed == tr.FUSED_SEEDS[case.id] and sum(r.near) == 0, (case.id, seed, r.near)
    for l, n in enumerate(case.widths):
        assert r.near[l] <= tr.GATE_CAP * case.B * n, (case.id, l, r.near[l])
    for t in [r.loss, r.prob, r.dX] + list(r.grads.values()):
        assert bool(torch.isfinite(t).all())
    assert set(r.grads) == set(tr.param_shapes(case)) and not any("gamma" in k or "beta" in k for k in r.grads)
    assert (r.gs0 is not None) == bool(case.s0)
    if case.rate > 0.0:
        keep = float(torch.cat([m.reshape(-1) for m in masks]).mean())
        assert abs(keep - (1.0 - case.rate)) < 0.1
    if case.pad is not None:        # the pad units: pre-activation exactly 0, outside the near count, gradients exactly 0
        l, n = case.pad
        assert bool((r.pre[l][:, n:] == 0).all()) and bool((r.grads[f"mlp.W{l}"][:, n:] == 0).all())
        assert bool((r.grads[f"mlp.b{l}"][n:] == 0).all()) and bool((r.grads[f"mlp.W{l + 1}"][n:] == 0).all())


def test_restatement_without_bn_is_the_formula():
    """h = relu(h W + b) * mask / (1 - rate) per layer, z = s0 + h Wout + bout, by hand in numpy float64."""
    case = tr.NOBN_CASE["tiny17"]._replace(s0=True)
    d = tr.draw(case, case.base_seed)
    r = tr.run_ref(case, d, masks=d["masks"])
    v = {k: t.double().numpy() for k, t in d["vals"].items()}
    h = d["X"].double().numpy()
    for l in range(len(case.widths)):
        h = np.maximum(h @ v[f"mlp.W{l}"] + v[f"mlp.b{l}"], 0.0) * d["masks"][l].double().numpy() / (1.0 - case.rate)
    z = d["s0"].double().numpy() + (h @ v["mlp.Wout"]).reshape(-1) + v["mlp.bout"]
    y = d["y"].double().numpy()
    np.testing.assert_allclose(r.prob.numpy(), 1.0 / (1.0 + np.exp(-z)), rtol=1e-12)
    np.testing.assert_allclose(float(r.loss), (np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))).mean(), rtol=1e-12)
    dz = (1.0 / (1.0 + np.exp(-z)) - y) / (case.B * case.replicas)
    np.testing.assert_allclose(r.gs0.numpy(), dz, rtol=1e-12)
    np.testing.assert_allclose(r.grads["mlp.Wout"].numpy().reshape(-1), h.T @ dz, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(r.grads["mlp.bout"].numpy(), [dz.sum()], rtol=1e-12)
    # eval: no dropout, no moments
    e = tr.run_ref(case, d, train=False)
    h = d["X"].double().numpy()
    for l in range(len(case.widths)):
        h = np.maximum(h @ v[f"mlp.W{l}"] + v[f"mlp.b{l}"], 0.0)
    ze = d["s0"].double().numpy() + (h @ v["mlp.Wout"]).reshape(-1) + v["mlp.bout"]
    np.testing.assert_allclose(e.prob.numpy(), 1.0 / (1.0 + np.exp(-ze)), rtol=1e-12)


def lds_bytes(k0, widths):
    """mlp_lds_layout (csrc/mlp_fused.hip) restated: the weights [K to 16][N to 16, + 4], the biases and output weights, per
    layer boundary an activation tile (two behind the input) of 16 rows of (width + 1 to 16) + 8, two da tiles of 16 rows of
    (widest to 16) + 8, 32 floats per-row scalars."""
    up16 = lambda x: (x + 15) // 16 * 16
    off, K = 0, k0
    for n in widths:
        off += up16(K) * (up16(n) + 4)
        K = n
    off += sum((n + 3) // 4 * 4 for n in widths) + (widths[-1] + 3) // 4 * 4
    for l, wdt in enumerate((k0,) + tuple(widths)):
        off += (1 if l == 0 else 2) * 16 * (up16(wdt + 1) + 8)
    off += 2 * 16 * (up16(max((k0,) + tuple(widths))) + 8) + 32
    return 4 * ((off + 3) // 4 * 4)


def test_lds_layout_restated_and_held_against_supported():
    from recsys_amd import _lib
    L = _lib.lib()
    table = {(96, (100, 100, 20)): 172608, (112, (112, 112)): 164288, (112, (112, 112, 112)): 234112,
             (96, (100, 52, 20)): 137856, (112, (112, 64, 32)): 152640, (48, (48, 48)): 50880}
    for (k0, ws), want in table.items():
        assert lds_bytes(k0, ws) == want, (k0, ws)
    for k0, ws in list(table) + [(c.k0, c.widths) for c in ALL
                                    if len(c.widths) <= 3 and max((c.k0,) + c.widths) <= 112 and not any(w % 4 for w in (c.k0,) + c.widths)]:
        got = L.rsx_mlp_nobn_supported(k0, (C.c_int32 * len(ws))(*ws), len(ws))
        assert got == int(lds_bytes(k0, ws) <= 160 * 1024), (k0, ws)
    for c in tr.FUSED_CASES:
        assert lds_bytes(c.k0, c.widths) <= 160 * 1024, c.id
    assert lds_bytes(*(lambda c: (c.k0, c.widths))(tr.NOBN_CASE["fallback"])) > 160 * 1024


def test_fused_table_covers_what_it_claims():
    cs = tr.FUSED_CASES
    nks = lambda k: (k + 15) // 16
    assert {len(c.widths) for c in cs} == {1, 2, 3}
    fwd = {nks(k) for c in cs for k in (c.k0,) + c.widths[:-1]}
    bwd = {nks(n) for c in cs for n in c.widths}
    for s in (fwd, bwd):                       # the tail alone, odd and even counts behind the two-accumulator loop
        assert 1 in s and any(x % 2 == 1 and x > 1 for x in s) and any(x % 2 == 0 for x in s), s
    assert {16, 32, 48, 96, 112} <= {c.k0 for c in cs}
    assert {4, 20, 52, 100, 64, 112} <= {n for c in cs for n in c.widths}
    sizes = [lds_bytes(c.k0, c.widths) for c in cs]
    assert any(s <= 64 * 1024 for s in sizes) and any(64 * 1024 < s <= 160 * 1024 for s in sizes) and 152640 in sizes
    assert {1, 16, 17, 250, 520, 1030} <= {c.B for c in cs}
    assert {bool(c.s0) for c in cs} == {True, False} and {c.replicas for c in cs} == {1, 2} and {0.0, 0.5} <= {c.rate for c in cs}
    assert all(tr.FUSED_CASE[i].rate > 0.0 for i in tr.FUSED_HASH)
    assert any(c.pad == (1, 50) and c.id in tr.FUSED_HASH for c in cs) and any(c.pad == (1, 50) and c.id not in tr.FUSED_HASH for c in cs)


def test_per_layer_table_is_inside_the_tower_envelope_and_outside_the_one_launch_form_where_it_says():
    for c in tr.NOBN_CASES:
        assert c.k0 % 4 == 0 and all(w % 4 == 0 for w in c.widths[:-1]) and c.widths[-1] <= 256, c.id
    assert all(tr.NOBN_CASE[i].rate > 0.0 for i in tr.NOBN_HASH_CASES)
    fb = tr.NOBN_CASE["fallback"]
    assert len(fb.widths) <= 3 and max((fb.k0,) + fb.widths) <= 112       # (inside the WIDTH envelope: only the LDS says no)


# ------------------------------------------------------------------------------------------------ the comparison notices
@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_fp32_restatement_passes_the_comparison(case):
    d, masks = _inputs(case)
    _check(case, d, _as_out(case, _fp32_step(case, d, masks)), masks)


DEFECT_CASES = [tr.FUSED_CASE["f_l1"], tr.FUSED_CASE["f_din"], tr.NOBN_CASE["din1024"], tr.NOBN_CASE["splitB"]]


@pytest.mark.parametrize("case", DEFECT_CASES, ids=lambda c: c.id)
def test_gradients_scaled_by_the_batch_alone_fail(case):
    """1 / B instead of 1 / (B * replicas): Adam's normalisation hides it from the model-level parity tests."""
    assert case.replicas == 2
    d, masks = _inputs(case)
    out = _as_out(case, _fp32_step(case, d, masks))
    _check(case, d, out, masks)
    out["grads"] = {k: g * case.replicas for k, g in out["grads"].items()}
    out["dX"] = out["dX"] * case.replicas
    if case.s0:
        out["gs0"] = out["gs0"] * case.replicas
    with pytest.raises(AssertionError, match="Mismatched|Not equal"):
        _check(case, d, out, masks)
    # ... and a single tensor with the wrong scale is enough
    out2 = _as_out(case, _fp32_step(case, d, masks))
    out2["grads"]["mlp.b0"] = out2["grads"]["mlp.b0"] * case.replicas
    with pytest.raises(AssertionError, match="mlp.b0"):
        _check(case, d, out2, masks)


@pytest.mark.parametrize("case", DEFECT_CASES + [tr.FUSED_CASE["f_max"], tr.NOBN_CASE["b4k"]], ids=lambda c: c.id)
def test_one_flipped_gate_fails(case):
    """ONE element of one layer takes the other side of its relu in the backward pass (its pre-activation is far from the kink:
    no borrowed gate covers it)."""
    d, masks = _inputs(case)
    f = _fp32_step(case, d, masks)
    gates = [g.clone() for g in f.gates]
    l = len(case.widths) - 1
    live = gates[l] * (masks[l] if masks is not None else 1.0)
    b, c = divmod(int((f.pre[l].abs() * live).argmax()), case.widths[l])          # an open, kept unit
    assert float(f.pre[l][b, c]) > 100 * tr.TAU and gates[l][b, c] == 1
    gates[l][b, c] = 0.0
    g = _fp32_step(case, d, masks, gates=gates)
    out = _as_out(case, g)
    # (the forward of the defective step is the right one -- what a kernel with a wrong backward gate would leave behind)
    out["loss"], out["prob"] = f.loss.reshape(1), f.prob
    if out["a"] is not None:
        out["a"] = list(f.a)
    with pytest.raises(AssertionError, match="Mismatched|Not equal"):
        _check(case, d, out, masks)


@pytest.mark.parametrize("case", [tr.FUSED_CASE["f_112"], tr.FUSED_CASE["f_din520"], tr.NOBN_CASE["din1024"]], ids=lambda c: c.id)
def test_dropout_hash_indexed_with_the_wrong_width_fails(case):
    """element index b * N' + c with N' the PADDED width (a multiple of 16) instead of the layer's own -- the same for every
    layer whose width is a multiple of 16, another mask everywhere else."""
    d, _ = _inputs(case)
    right = tr.hash_masks(case.B, case.widths, case.rate)
    wrong = []
    for l, n in enumerate(case.widths):
        npad = (n + 15) // 16 * 16
        wrong.append(tr.hash_masks(case.B, (npad,), case.rate, layer0=l)[0][:, :n].contiguous())
    assert any(not torch.equal(a, b) for a, b in zip(right, wrong))
    _check(case, d, _as_out(case, _fp32_step(case, d, right)), right)
    with pytest.raises(AssertionError, match="Mismatched|Not equal"):
        _check(case, d, _as_out(case, _fp32_step(case, d, wrong)), right)


# ------------------------------------------------------------------------------------------------ the pooling reference
@pytest.mark.parametrize("K", pr.KS)
def test_pool_fp32_restatement_passes_and_planted_defects_fail(K):
    assert pr.rpw(K) * K == 256
    for i, (P, B) in enumerate(pr.shapes(K)):
        hs = pr.draw(K, P, B, 1000 * K + i)
        for t, h in enumerate(hs):
            ids = h["ids"]
            assert ids[0, 0] == 0 and np.isfinite(h["H"]).all()
            if B >= 2:
                assert (ids[1] <= 0).all()
            if B >= 3:
                assert ids[-1, -1] < 0
            pr.check_fwd(("fp32", K, P, B, t), pr.f32_fwd(h), h)
            for acc in (0, 1):
                dH, dw = pr.f32_bwd(h, acc)
                pr.check_bwd(("fp32", K, P, B, t, acc), dH, dw, h, acc)
            # the mask taken as ids != 0: negative ids count as history
            neg = ids < 0
            if neg.any():
                m = ids != 0
                if (np.abs(h["w"])[neg] > 0).any():
                    with pytest.raises(AssertionError):
                        pr.check_fwd(("ne0",), pr.f32_fwd(h, mask=m), h)
                for acc in (0, 1):
                    dH, dw = pr.f32_bwd(h, acc, mask=m)
                    with pytest.raises(AssertionError):
                        pr.check_bwd(("ne0",), dH, dw, h, acc)
            # one pooling position dropped (the last valid one of some example: a loop that ends one trip early)
            valid = np.argwhere(ids > 0)
            if len(valid):
                b, p = valid[-1]
                with pytest.raises(AssertionError):
                    pr.check_fwd(("drop",), pr.f32_fwd(h, drop=(b, p)), h)
                dH, dw = pr.f32_bwd(h, 0)
                dH[b, p] = 0.0
                with pytest.raises(AssertionError):
                    pr.check_bwd(("drop",), dH, dw, h, 0)
    assert any((pr.draw(K, P, B, 1000 * K + i)[0]["ids"] < 0).any() for i, (P, B) in enumerate(pr.shapes(K)))


def test_pool_shapes_are_the_ones_around_the_kernels_loop():
    for K in pr.KS:
        r = pr.rpw(K)
        assert set(pr.positions(K)) == {1, r - 1, r, r + 1, 4 * r - 1, 4 * r, 4 * r + 1, 9 * r + 3}
        assert len(pr.shapes(K)) == 8 * 5
