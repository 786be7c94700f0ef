"""The fp64 reference of tests/test_gpu_din_attn.py, checked without a GPU: the forward is the attention block of
oracle.models (the independent numpy restatement), the hand-written backward is torch autograd's of that forward, the host
restatement of the dropout hash with a layer offset is drop_device.h's formula, the case table reaches every dispatch form the
GPU test claims to cover, and the drawn history ids have the counts and the padding pattern the row-list tests rest on."""
import numpy as np
import pytest
import torch

from oracle import models
from tests import din_attn_ref as ar
from tests import tower_ref

SMALL = ar.Case("small", 5, 7, 16, 12, 8, 0.5, "masks", False, False, True, 11)


def test_forward_is_the_oracles_attention_block():
    d = ar.draw(SMALL)
    a1, a2, w = ar.forward_ref(d, d["masks"])
    B, P, K = SMALL.B, SMALL.P, SMALL.K
    table = np.concatenate([np.zeros((1, K)), d["H"].double().numpy()])          # row 1 + m = H[m]; id 0 is the padding id
    hist = 1 + np.arange(B * P).reshape(B, P)
    Pm = {"att.%s" % k: d[k].double().numpy() for k in ("W0", "b0", "W1", "b1", "b2")}
    Pm["att.W2"] = d["W2"].double().numpy().reshape(-1, 1)
    masks = [m.double().numpy() for m in d["masks"]]
    _, cache = models.din_attention_fwd(table, hist, d["q"].double().numpy(), Pm, "att", True, SMALL.rate, masks)
    for got, want in ((a1, cache[5]), (a2, cache[8]), (w, cache[11].reshape(-1))):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
    assert float(a1.min()) == 0.0 and float(a2.min()) == 0.0 and float(a1.max()) > 0.5      # (relu outputs, before dropout)


@pytest.mark.parametrize("variant", ["plain", "masks", "list", "acc"])
def test_backward_is_autograd_of_the_forward(variant):
    """backward_ref from the fp64 forward's own a1 / a2 against torch autograd of sum(w * dw) (row list: the padding positions'
    w multiplied by 0), 1e-10 relative to each tensor's largest entry."""
    case = SMALL._replace(rate=0.0, drop="none") if variant == "plain" else SMALL
    d = ar.draw(case)
    masks = d["masks"]
    ids = ar.draw_ids(case, "anywhere") if variant in ("list", "acc") else None
    acc = variant == "acc"
    names = ("H", "q", "W0", "b0", "W1", "b1", "W2", "b2")
    leaf = dict(d)
    leaf.update({k: d[k].double().requires_grad_() for k in names})
    a1, a2, w = ar.forward_ref(leaf, masks)
    weight = d["dw"].double() * ((ids.reshape(-1) > 0).double() if ids is not None else 1.0)
    (w * weight).sum().backward()
    r = ar.backward_ref(d, a1.detach(), a2.detach(), masks, ids=ids, accumulate_dH=acc, dq_add=acc)
    want = {k: leaf[k].grad for k in names}
    want["H"] = want["H"] + (d["dH0"].double() if acc else 0.0)
    want["q"] = want["q"] + (d["dq_add"].double() if acc else 0.0)
    for name, key in (("dH", "H"), ("dq", "q"), ("dW0", "W0"), ("db0", "b0"), ("dW1", "W1"), ("db1", "b1"), ("dW2", "W2"), ("db2", "b2")):
        m = float(want[key].abs().max())
        assert m > 0.0, name
        assert float((r[name] - want[key]).abs().max()) <= 1e-10 * m, name
    packed = torch.cat([want[k].reshape(-1) for k in ("W0", "b0", "W1", "b1", "W2", "b2")])
    assert r["grads"].numel() == ar.n_grads(case) and float((r["grads"] - packed).abs().max()) <= 1e-10 * float(packed.abs().max())
    for name, (o, shape) in ar.grad_slices(case).items():
        assert torch.equal(r["grads"][o:o + int(np.prod(shape))].reshape(shape), r[name]), name
    if ids is not None:       # positions that are padding get no gradient; an all-padding example's query neither
        pad = (ids.reshape(-1) == 0)
        base = d["dH0"].double() if acc else torch.zeros_like(r["dH"])
        assert torch.equal(r["dH"][pad], base[pad])
        b = case.B // 2
        assert torch.equal(r["dq"][b], d["dq_add"].double()[b] if acc else torch.zeros(case.K, dtype=torch.float64))


def _hash32(x):
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_hash_masks_with_a_layer_offset_are_the_documented_formula():
    """drop_device.h, scalar and in pure Python: key = hash32(seed ^ step * 0x9E3779B9 ^ (layer * 0x85EBCA6B + 0x27220A95)),
    element idx = m * N + n kept when hash32(idx ^ key) >= rate * 2^32; the attention block's layers are layer0 and layer0 + 1."""
    M, widths, rate, step, seed = 37, (12, 8), 0.5, ar.RNG_STEP, ar.HASH_SEED
    m3 = tower_ref.hash_masks(M, widths, rate, step=step, seed=seed, layer0=3)
    m0 = tower_ref.hash_masks(M, widths, rate, step=step, seed=seed)
    assert all(not torch.equal(a, b) for a, b in zip(m3, m0))
    assert torch.equal(m0[1], tower_ref.hash_masks(M, (widths[1],), rate, step=step, seed=seed, layer0=1)[0])
    thresh = int(rate * 2 ** 32)
    for l, n in enumerate(widths):
        key = _hash32((seed ^ ((step * 0x9E3779B9) & 0xFFFFFFFF) ^ (((3 + l) * 0x85EBCA6B + 0x27220A95) & 0xFFFFFFFF)) & 0xFFFFFFFF)
        for m, c in ((0, 0), (0, n - 1), (1, 0), (17, 3), (M - 1, n - 1), (M // 2, n // 2)):
            keep = 0.0 if _hash32((m * n + c) ^ key) < thresh else 1.0
            assert float(m3[l][m, c]) == keep, (l, m, c)
    assert 0.3 < float(m3[0].mean()) < 0.7
    case = ar.CASE["a_off"]
    hm = ar.masks_of(case, ar.draw(case))
    assert hm[0].shape == (case.B * case.P, case.N1) and hm[1].shape == (case.B * case.P, case.N2)
    assert torch.equal(hm[0], tower_ref.hash_masks(case.B * case.P, (case.N1,), case.rate, step=7, seed=0xD1A77, layer0=2)[0])


# Every dispatch form tests/test_gpu_din_attn.py is meant to run: a form nobody reaches fails HERE, not silently on the GPU.
REQUIRED_FORMS = [
    "fwd split<2>", "fwd split<1>", "fwd fp32<2>", "fwd fp32<1>",
    "bwd<2,true>", "bwd<1,true>", "bwd<2,false>", "bwd<1,false>",
    "W-staging vec4", "W-staging scalar",
    "fwd wrap split", "fwd wrap fp32",
    "bwd wrap K=16", "bwd wrap K=32",
    "per=1", "per=2", "per=9", "per=16",
]


def test_case_table_reaches_every_dispatch_form():
    reached = set()
    for c in ar.CASES:
        reached |= set(ar.forms(c))
    missing = [f for f in REQUIRED_FORMS if f not in reached]
    assert not missing, missing
    # the combinations the table's comments name
    f = {c.id: ar.forms(c) for c in ar.CASES}
    assert "bwd<2,true>" in f["w_off"] and "W-staging scalar" in f["w_off"] and "fwd split<2>" in f["w_off"]
    assert "fwd fp32<2>" in f["a_off"] and "bwd<2,false>" in f["a_off"]
    assert "G=17" in f["g17"] and "per=2" in f["g17"] and "G=130" in f["g130"] and "per=9" in f["g130"]
    assert "G=1" in f["one"] and "G=16" in f["w_off"] and "per=1" in f["w_off"]
    assert "bwd wrap K=16" in f["bwrap16"] and "per=16" in f["bwrap16"] and "fwd blocks 65 <= grid" in f["bwrap16"]
    assert "fwd wrap split" in f["wrap"] and "fwd wrap fp32" in f["wrap-a_off"] and "bwd wrap K=32" in f["wrap"]
    for cid in ("scaled", "scaled-k16", "w7636", "w7636-k16", "w44", "w6432", "w8048"):
        assert any(x.startswith("fwd split") for x in f[cid]), cid
    for cid in ("scaled-a_off", "scaled-k16-a_off", "w7838", "w7838-k16", "w75"):
        assert any(x.startswith("fwd fp32") for x in f[cid]) and any(x.endswith(",false>") for x in f[cid]), cid
    assert len({c.id for c in ar.CASES}) == len(ar.CASES)
    for cid in ar.LIST_CASES:
        assert ar.CASE[cid].drop == "masks" and ar.CASE[cid].rate == 0.5
    assert {ar.CASE[c].K for c in ar.LIST_CASES} == {16, 32}
    # a case and its offset twin share their inputs (and so their reference)
    assert ar.draw(ar.CASE["wrap"]) is ar.draw(ar.CASE["wrap-a_off"])
    # unit-scale pre-activations, as draw() promises (so that the bars mean what they mean for the tower)
    d = ar.draw(ar.CASE["g17"])
    a1, a2, w = ar.forward_ref(d)
    assert 0.3 < float(a1.std()) < 3.0 and 0.3 < float(a2.std()) < 3.0 and 0.3 < float(w.std()) < 3.0


@pytest.mark.parametrize("cid", ar.LIST_CASES)
def test_drawn_ids_have_the_counts_and_padding_the_row_list_tests_rest_on(cid):
    case = ar.CASE[cid]
    M = case.B * case.P
    count = {mode: int((ar.draw_ids(case, mode) > 0).sum()) for mode in ar.ID_MODES}
    assert count["zero"] == 0 and count["one"] == 1 and count["full"] == M
    assert 0.6 * M < count["anywhere"] < 0.9 * M
    ids = ar.draw_ids(case, "anywhere").numpy()
    assert (ids.max(1) == 0).sum() >= 1                                  # an all-padding example
    assert ids[0, 0] == 0                                                # row 0 is not in the list
    first_pad = (ids == 0).argmax(1)
    has_pad = (ids == 0).any(1)
    not_suffix = [b for b in range(case.B) if has_pad[b] and ids[b].max() > 0 and (ids[b, first_pad[b]:] > 0).any()]
    assert len(not_suffix) >= 1                                          # padding that is not a suffix
    assert count["anywhere"] % ar.BWD_ROWS != 0 and count["anywhere"] % 16 != 0      # a ragged last block and a ragged last wave
    one = ar.draw_ids(case, "one").numpy()
    assert one[0, 0] == 0 and one.reshape(-1).argmax() not in (0, M - 1)
