"""The compact form of the window sweep (rsx_adam_slice.window_compact, RSX_FORMS window_compact; csrc/adam_device.h): a
block's rows are classified first -- void (m and v all +0: nothing loaded further, nothing stored), idle (m all +0, v in
[+0, +inf]: v alone is multiplied and stored), live (everything else) -- and the full updates run on the live rows only,
compacted into full waves.  It has to be the one-pass form bit for bit: every comparison here is on int32 views of var, m
and v, against the one-pass form of the same launch and against k single-step sweeps."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
BLOCK_ROWS_D16 = 512          # ADAM_T * ADAM_U float4 per workgroup / (16 / 4) float4 per row
WAVE_ROWS_D16 = 16            # rows of one wave's 64 lanes
KINDS = ("void", "idle_ord", "idle_mixed0", "idle_denorm", "idle_edge", "idle_inf", "live_ord", "live_single_m",
         "live_single_m_v0", "live_m_negzero", "live_v_negzero", "live_v_nan")
VOID, IDLE, LIVE = ("void",), KINDS[1:6], KINDS[6:]


def _row(kind, D, rng):
    """(m, v) of one row of class `kind`."""
    m, v = np.zeros(D, F), np.zeros(D, F)
    ordinary_v = lambda: ((rng.random(D).astype(F) * F(1e-3)) ** 2 + F(1e-12)).astype(F)
    j = int(rng.integers(0, D))
    if kind == "idle_ord":
        v = ordinary_v()
    elif kind == "idle_mixed0":                       # some v of the row still +0
        v = ordinary_v()
        v[rng.random(D) < 0.5] = 0.0
        v[j] = F(1e-7)
    elif kind == "idle_denorm":
        v = (rng.integers(1, 1 << 23, D).astype(np.uint32)).view(F).copy()       # every denormal exponent pattern
        v[j] = F(1e-45)
    elif kind == "idle_edge":                         # around the packed square root's lower guard
        v = np.array([2.0 ** -87, 2.0 ** -86, 2.0 ** -85], F)[rng.integers(0, 3, D)]
    elif kind == "idle_inf":
        v = ordinary_v()
        v[j] = np.inf
        if rng.random() < 0.3:
            v[:] = np.inf
    elif kind == "live_ord":
        m = (rng.standard_normal(D) * 1e-4).astype(F) * (F(0.9) ** rng.integers(0, 700, D)).astype(F)
        v = ordinary_v()
    elif kind == "live_single_m":
        v = ordinary_v()
        m[j] = F(rng.choice([3e-5, -2e-3, 1e-45, -1e-39, 2.0 ** -81]))
    elif kind == "live_single_m_v0":                  # a single moment in a row of zeros
        m[j] = F(rng.choice([3e-5, -2e-3, 1e-45]))
    elif kind == "live_m_negzero":
        v = ordinary_v() if rng.random() < 0.7 else v
        m[j] = F(-0.0)
    elif kind == "live_v_negzero":
        v = ordinary_v() if rng.random() < 0.7 else v
        v[j] = F(-0.0)
    elif kind == "live_v_nan":
        v = ordinary_v()
        v[j] = np.nan
    else:
        assert kind == "void"
    return m, v


def _mix(rng, n, p_void, p_idle):
    """n class names: void / idle / live with the given shares, the sub-kinds uniform inside each."""
    u = rng.random(n)
    return [VOID[0] if x < p_void else IDLE[rng.integers(0, len(IDLE))] if x < p_void + p_idle
            else LIVE[rng.integers(0, len(LIVE))] for x in u]


@functools.lru_cache(maxsize=None)
def _state(layout, R, D, k):
    """Host state (var, m, v as [R, D] fp32), the k slot maps [k, R + 4] and each row's class, from a seed."""
    rng = np.random.default_rng([R, D, k, sorted(("interleave", "void_block", "live_block", "alternating")).index(layout)])
    rows_per_block = BLOCK_ROWS_D16 * 16 // D
    wave_rows = max(1, WAVE_ROWS_D16 * 16 // D)
    if layout == "interleave":
        kinds = _mix(rng, R, 0.34, 0.26)
    elif layout == "void_block":                      # the first workgroup's block holds nothing but void rows
        kinds = ["void"] * rows_per_block + _mix(rng, R - rows_per_block, 0.06, 0.40)
    elif layout == "live_block":                      # the second workgroup's block holds nothing but live rows
        kinds = _mix(rng, R, 0.56, 0.34)
        kinds[rows_per_block:2 * rows_per_block] = [LIVE[rng.integers(0, len(LIVE))] for _ in range(rows_per_block)]
        # and the first wave of the first block meets live rows only in its first batch (rows 0..15 and 64..79 at D = 16: the
        # wave takes the one-pass pipeline, its neighbours classify), void and idle ones in its later batches
        for r in list(range(0, wave_rows)) + list(range(4 * wave_rows, 5 * wave_rows)):
            kinds[r] = LIVE[rng.integers(0, len(LIVE))]
    else:                                             # strictly alternating: void, idle, live, void, ...
        kinds = [("void", IDLE[(i // 3) % len(IDLE)], LIVE[(i // 3) % len(LIVE)])[i % 3] for i in range(R)]
    m, v = (np.stack(x) for x in zip(*[_row(kd, D, rng) for kd in kinds]))
    var = (rng.standard_normal((R, D)) * 0.05).astype(F)
    pick = rng.random((R, D))
    var[pick < 0.10] = F(0.0)
    var[(pick >= 0.10) & (pick < 0.20)] = F(-0.0)
    var[(pick >= 0.20) & (pick < 0.30)] = F(1e-41)
    var[(pick >= 0.30) & (pick < 0.33)] = F(-3e-45)
    # slot maps: 2 % of the rows per step at random, and the first / last row of wave batches and of blocks
    edges = [0, wave_rows - 1, wave_rows, 2 * wave_rows - 1, rows_per_block - 1, rows_per_block, rows_per_block + wave_rows - 1,
             R - 1]
    if R > 2 * rows_per_block:
        edges += [2 * rows_per_block - 1, 2 * rows_per_block]
    edges = [e for e in edges if e < R]
    slots = np.full((k, R + 4), -1, np.int32)
    for i in range(k):
        idx = np.unique(np.concatenate([rng.choice(R, R // 50, replace=False), np.array(edges[i::k], np.int64)]))
        slots[i, idx] = np.arange(len(idx), dtype=np.int32)
    return var, m, v, slots, tuple(kinds)


def _assert_not_vacuous(state):
    """From the host arrays: every class is there in bulk among the rows no step touches, and touched rows of every class."""
    var, m, v, slots, kinds = state
    R = len(kinds)
    mb, vb = m.view(np.uint32), v.view(np.uint32)
    m0 = (mb == 0).all(1)
    void = m0 & (vb == 0).all(1)
    idle = m0 & ~void & (vb <= 0x7f800000).all(1)
    live = ~void & ~idle
    for name, mask in (("void", void), ("idle", idle), ("live", live)):     # the builder's labels are the bits' classes
        want = np.array([kd in {"void": VOID, "idle": IDLE, "live": LIVE}[name] for kd in kinds])
        assert np.array_equal(mask, want), name
    touched = (slots[:, :R] >= 0).any(0)
    n = int((~touched).sum())
    assert (void & ~touched).sum() >= 0.25 * n and (idle & ~touched).sum() >= 0.15 * n and (live & ~touched).sum() >= 0.25 * n, \
        ((void & ~touched).sum(), (idle & ~touched).sum(), (live & ~touched).sum(), n)
    assert (void & touched).any() and (idle & touched).any() and (live & touched).any()
    for kd in KINDS:
        assert any(x == kd and not t for x, t in zip(kinds, touched)), kd
    for bits in (0x00000000, 0x80000000):                                     # var: both zeros, denormals, ordinary values
        assert (var.view(np.uint32)[~touched] == bits).any()
    a = np.abs(var[~touched])
    assert ((a > 0) & (a < 2.0 ** -126)).any() and (a > 1e-3).any()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _sweep(state, form, hyper=None):
    """One window sweep over `state` ('compact' / 'one_pass'), or k single-step sweeps with the beta powers advanced by hand
    ('singles') -> (var, m, v) on the host."""
    from recsys_amd import _lib
    from recsys_amd.ops import AdamTF1
    hyper = hyper or {}
    var0, m0, v0, slots_h, _ = state
    R, D = var0.shape
    k = slots_h.shape[0]
    t, m, v = (torch.from_numpy(x.copy()).cuda() for x in (var0, m0, v0))
    slot_all = torch.from_numpy(slots_h).cuda()
    b1, b2 = hyper.get("b1", 0.9), hyper.get("b2", 0.999)
    opt = AdamTF1(lr=hyper.get("lr", 1e-3), beta1=b1, beta2=b2, eps=hyper.get("eps", 1e-8), device="cuda")
    if form in ("compact", "one_pass"):
        segs = [dict(kind=_lib.RSX_ADAM_TABLE_TF1_COLD, d=D, n=R, var=t, m=m, v=v, slot=slot_all[0],
                     slot_w=[slot_all[i] for i in range(1, k)])]
        for sl in opt.cold_slices(segs, [1.0, 2.0]):
            if sl is not None:
                sl.window_compact = int(form == "compact")
                opt.run_slice(sl)
    else:
        union = torch.where((slot_all[:, :R] >= 0).any(0), 0, -1).to(torch.int32)
        union = torch.cat([union, torch.full((4,), -1, dtype=torch.int32, device="cuda")])
        segs = [dict(kind=_lib.RSX_ADAM_TABLE_TF1_COLD, d=D, n=R, var=t, m=m, v=v, slot=union)]
        for _ in range(k):
            for sl in opt.cold_slices(segs, [1.0]):
                opt.run_slice(sl)
            st = opt.state.cpu().numpy().copy()          # COLD slices never advance the powers: do it as the step would
            st[0], st[1] = F(st[0] * F(b1)), F(st[1] * F(b2))
            opt.state.copy_(torch.from_numpy(st))
    torch.cuda.synchronize()
    return [x.cpu() for x in (t, m, v)]


def _assert_same_bits(a, b, state, what):
    for name, x, y in zip(("var", "m", "v"), a, b):
        diff = (_bits(x) != _bits(y)).any(1)
        rows = torch.nonzero(diff).flatten()[:4].tolist()
        assert not bool(diff.any()), (what, name, int(diff.sum()), [(r, state[4][r]) for r in rows])


@pytest.mark.parametrize("k", [2, 5, 8])
@pytest.mark.parametrize("layout", ["interleave", "void_block", "live_block", "alternating"])
def test_compact_sweep_is_the_bits_of_the_one_pass_form_and_of_k_single_sweeps(layout, k):
    """R = 1100 rows of 16: two full 512-row blocks and a tail block of 76, every class in every layout."""
    state = _state(layout, 1100, 16, k)
    _assert_not_vacuous(state)
    compact = _sweep(state, "compact")
    _assert_same_bits(compact, _sweep(state, "one_pass"), state, "one-pass form")
    _assert_same_bits(compact, _sweep(state, "singles"), state, "k single sweeps")
    # and the shortcuts did what they claim: void / idle rows kept var and m, void rows kept v, idle rows' v moved
    var0, m0, v0, slots, kinds = state
    cold = ~(slots[:, :1100] >= 0).any(0)
    still = cold & np.array([kd in VOID + IDLE for kd in kinds])
    assert np.array_equal(compact[0].numpy().view(np.int32)[still], var0.view(np.int32)[still])
    assert np.array_equal(compact[1].numpy().view(np.int32)[still], m0.view(np.int32)[still])
    moved = cold & np.array([kd == "idle_ord" for kd in kinds])
    assert (compact[2].numpy()[moved] < v0[moved]).all()


@pytest.mark.parametrize("hyper", [dict(eps=0.0), dict(lr=float("inf")), dict(b1=0.5)], ids=["eps0", "lr_inf", "b1_half"])
def test_compact_sweep_outside_and_inside_the_gate(hyper):
    """eps = 0 and lr = inf close the gate (0 / 0 and inf * 0: every row takes the full updates and gets the one-pass form's
    NaNs); b1 = 0.5 switches the packed chain off but keeps the shortcuts."""
    state = _state("interleave", 1100, 16, 8)
    _assert_same_bits(_sweep(state, "compact", hyper), _sweep(state, "one_pass", hyper), state, repr(hyper))


@pytest.mark.parametrize("D", [8, 32])
def test_compact_sweep_other_row_widths(D):
    state = _state("interleave", 700, D, 8)
    _assert_not_vacuous(state)
    _assert_same_bits(_sweep(state, "compact"), _sweep(state, "one_pass"), state, "D = %d" % D)


def test_deepfm_training_is_identical_in_both_forms(monkeypatch):
    """DeepFM, batch 32, embedding 16: 24 steps through train_resident in 8-step windows, 8 steps per graph, with
    RSX_FORMS window_compact = 1 and = 0: the loss, the dense arena and every table row."""
    from recsys_amd import deepfm, synthetic
    from recsys_amd.estimator import Estimator, PackedBatch, RunConfig
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    B = 32
    lin, emb = build_feature_columns(16, "indicator_all")
    layout = CriteoLayout.from_columns(emb)
    host = synthetic.criteo_id_batches(layout, 16, B, seed=2718)
    res = []
    for compact in ("1", "0"):
        monkeypatch.setenv("RSX_FORMS", "window_compact=" + compact)
        params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
                  "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": B, "overlap_adam": True, "adam_window": 8}
        est = Estimator(deepfm.model_fn, None, params, RunConfig(use_hip_graph=True, adam_mode="tf1_dense", device="cuda", seed=9,
                                                                 log_step_count_steps=10))
        feats = [PackedBatch({"ids": i}, y, device="cuda") for i, y, _ in host]
        with torch.no_grad():
            est._call_model_fn(feats[0].views()[0], None, "infer")
        assert est._window_len() == 8
        loss = est.train_resident(feats, 24, 8)
        assert est.global_step == 24
        torch.cuda.synchronize()
        a = est.store.embeddings["input_layer"]
        res.append({"loss": loss.clone(), "dense": est.store.dense.flat.clone(), "dense_m": est.store.dense.m.clone(),
                    "dense_v": est.store.dense.v.clone(), "tables": a.tables.clone(), "m": a.m_t.clone(), "v": a.v_t.clone(),
                    "w1": a.w1.clone(), "m_w": a.m_w.clone(), "v_w": a.v_w.clone()})
    for name in res[0]:
        assert torch.isfinite(res[0][name].float()).all(), name
        assert torch.equal(_bits(res[0][name].float()), _bits(res[1][name].float())), name
    # (the run is not vacuous either way: most rows of the tables are still void, the touched ones carry moments)
    m_rows = (res[0]["m"].view(-1, 16) != 0).any(1)
    assert 0 < int(m_rows.sum()) < m_rows.numel() // 2
