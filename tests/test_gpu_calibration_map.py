"""Isotonic calibration on the device: rsx_calibration_quantile_table and rsx_calibrate_apply (csrc/calibration_map.hip) against
metrics.quantile_table_host / isotonic_apply_host, whose definitions tests/test_calibration_map_cpu.py holds to Python integers
and fractions; RunConfig.calibration_fit / calibration_apply through the Estimator; the bundle's calibration.json through the
Predictor on every path.  Tables are compared as integers and probabilities as bit patterns: no tolerance anywhere."""
import ctypes as C
import importlib
import json
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch

from recsys_amd import metrics
from recsys_amd._lib import RsxError, check, lib

pytestmark = pytest.mark.gpu

ONE = 1 << 32
INVALID_BITS = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0xBF800000, 0x40000000, 0x3F800001,
                         0x80000001], np.uint32)            # NaNs with payloads, +-inf, -1, 2, 1 + ulp, -denormal
GARBAGE = 0x5A5A5A5A5A5A5A5A


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the table ------------------------------------------------------------------------------------------------------------------
def sorted_stream(y, p, batch=None, order=None):
    """An ExactAUC after result(): the keys sorted on the device."""
    if order is not None:
        y, p = y[order], p[order]
    ex = metrics.ExactAUC("cuda")
    step = batch or max(1, len(p))
    yd, pd = up(y), up(p)
    for i in range(0, len(p), step):
        ex.update(yd[i:i + step], pd[i:i + step])
    res = ex.result()
    return ex, res


def raw_table(ex, V, M):
    """The C entry itself over a table filled with garbage, one guard row behind it."""
    table = torch.full((3 * M + 3,), GARBAGE, dtype=torch.int64, device="cuda")
    check(lib().rsx_calibration_quantile_table(C.c_void_p(ex.keys.data_ptr()), V, M, C.c_void_p(table.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "quantile_table")
    t = table.cpu().numpy()
    assert t[3 * M:].tolist() == [GARBAGE] * 3                 # nothing behind the table
    return t[:3 * M].reshape(M, 3)


def check_tables(y, p, Ms=(2, 10, 1024), **kw):
    ex, res = sorted_stream(y, p, **kw)
    V = res["positives"] + res["negatives"]
    for M in Ms:
        want = metrics.quantile_table_host(y, p, M)
        got = ex.quantile_table(M)
        assert got.dtype == np.int64 and got.shape == (M, 3)
        assert np.array_equal(got, want), (len(p), M)
        assert np.array_equal(raw_table(ex, V, M), want), (len(p), M)      # every word written, garbage or not
        assert int(got[:, 0].sum()) == V and int(got[:, 1].sum()) == res["positives"]
    return ex


def stream(rng, n, ties=None):
    p = rng.random(n).astype(np.float32)
    if ties:
        p = (np.round(p * ties) / ties).astype(np.float32)
    y = (rng.random(n) < 0.1 + 0.8 * p).astype(np.float32)
    return y, p


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 1024, 4095, 4096, 4097, 65836])   # 255 / 1024: the 256-thread block sum,
def test_table_at_every_size_and_bin_count(n):                                           # partly and exactly 4 keys per thread
    rng = np.random.default_rng(3 * n)
    y, p = stream(rng, n)
    check_tables(y, p)                                         # M = 1024 > n for the small sizes: most bins empty
    y, p = stream(rng, n, ties=8)                              # tie groups straddle the quantile boundaries
    check_tables(y, p)


@pytest.mark.parametrize("n", [65, 4097, 65836])
def test_table_of_degenerate_score_sets(n):
    rng = np.random.default_rng(n)
    y = (rng.random(n) < 0.3).astype(np.float32)
    for value in (0.0, 1.0, 0.37):                             # all scores equal: one workgroup reads everything
        p = np.full(n, value, np.float32)
        ex = check_tables(y, p)
        t = ex.quantile_table(10)
        assert t[0].tolist() == [n, int(y.sum()), n * int(metrics.calibration_q_host(np.float32(value)))] and not t[1:].any()
    p = np.where(rng.random(n) < 0.4, np.float32(0.2), np.float32(0.9)).astype(np.float32)      # two distinct scores
    ex = check_tables(y, p)
    assert np.count_nonzero(ex.quantile_table(1024)[:, 0]) == 2


def test_table_with_invalid_probabilities_and_padding_behind_the_valid_keys():
    rng = np.random.default_rng(11)
    n = 4097
    y, p = stream(rng, n, ties=64)
    at = rng.choice(n, 10 * INVALID_BITS.size, replace=False)
    pb = bits(p).copy()
    pb[at] = np.tile(INVALID_BITS, 10)
    pb[:3] = [0x80000000, 0x00000000, 0x3F800000]              # -0.0 counts as +0.0
    p = pb.view(np.float32)
    ex, res = sorted_stream(y, p)
    assert res["invalid"] == at.size and ex.sorted_valid == n - at.size
    for M in (2, 10, 1024):
        assert np.array_equal(ex.quantile_table(M), metrics.quantile_table_host(y, p, M))


def test_table_does_not_depend_on_batches_or_order():
    rng = np.random.default_rng(12)
    n = 65836
    y, p = stream(rng, n, ties=4096)
    want = [metrics.quantile_table_host(y, p, M) for M in (10, 1024)]
    for kw in ({}, {"batch": 7 * 1024 + 7}, {"order": np.arange(n)[::-1].copy()}, {"order": rng.permutation(n), "batch": 9999}):
        ex, _ = sorted_stream(y, p, **kw)
        assert all(np.array_equal(ex.quantile_table(M), w) for M, w in zip((10, 1024), want))
    small_y, small_p = stream(rng, 300, ties=8)
    ex, _ = sorted_stream(small_y, small_p, batch=7)           # batches of 7
    assert np.array_equal(ex.quantile_table(10), metrics.quantile_table_host(small_y, small_p, 10))


def test_table_of_nothing_and_the_call_order():
    ex = metrics.ExactAUC("cuda", 8)
    with pytest.raises(RsxError, match="result"):
        ex.quantile_table(10)                                  # nothing sorted yet
    ex.result()
    assert not ex.quantile_table(10).any()                     # n_valid == 0
    assert not raw_table(ex, 0, 1024).any()
    ex.update(np.ones(4, np.float32), np.full(4, np.nan, np.float32))
    with pytest.raises(RsxError, match="result"):
        ex.quantile_table(10)                                  # an update since the sort
    ex.result()
    assert ex.sorted_valid == 0 and not ex.quantile_table(2).any()      # only invalid examples
    for M in (1, 1025):
        with pytest.raises(RsxError, match="n_bins"):
            ex.quantile_table(M)


# ---- the map ------------------------------------------------------------------------------------------------------------------
def knots(K, seed=0):
    rng = np.random.default_rng(seed + K)
    if K == 1024:                                              # a dense map: neighbouring knots a few ulps apart in places
        x = np.unique(np.concatenate([rng.random(900), 0.5 + rng.random(400) * 1e-4]).astype(np.float32))[:1024]
        assert x.size == 1024
    else:
        x = np.sort(rng.random(K).astype(np.float32) * np.float32(0.8) + np.float32(0.1))
    y = np.sort(rng.random(K).astype(np.float32))
    y[K // 2:K // 2 + 2] = y[K // 2]                           # a flat stretch
    return np.ascontiguousarray(x), np.ascontiguousarray(np.sort(y))


def inputs(x, n, seed=0):
    """n fp32 bit patterns: every knot and its two neighbours, 0, 1, -0.0, subnormals, the invalid patterns, then random ones."""
    rng = np.random.default_rng(seed + n)
    near = np.concatenate([x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2))]).astype(np.float32)
    special = np.concatenate([INVALID_BITS, np.array([0x00000000, 0x3F800000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000],
                                                     np.uint32), bits(near)])
    special = special[rng.permutation(special.size)]
    fill = bits(rng.random(max(n, 1)).astype(np.float32))
    return np.concatenate([special, fill])[:n].copy() if n >= 64 else np.concatenate([special[:n // 2], fill])[:n].copy()


def apply_device(cal, pb, in_off=0, out_off=0, in_place=False):
    """The launch over views that start `*_off` elements into their buffers; -> the output bits (guards checked)."""
    n = pb.size
    src = torch.full((n + 8,), -7.0, device="cuda")
    src[in_off:in_off + n] = up(pb.view(np.int32)).view(torch.float32)
    if in_place:
        dst, out_off = src, in_off
    else:
        dst = torch.full((n + 8,), -7.0, device="cuda")
    out = cal.apply(src[in_off:in_off + n], out=dst[out_off:out_off + n])
    assert out.data_ptr() == dst.data_ptr() + 4 * out_off
    got = dst.cpu().numpy()
    assert np.all(got[:out_off] == -7.0) and np.all(got[out_off + n:] == -7.0)      # nothing outside the view
    if not in_place:
        assert np.array_equal(src[in_off:in_off + n].cpu().numpy().view(np.uint32), pb)      # the input is not touched
    return got[out_off:out_off + n].view(np.uint32)


@pytest.mark.parametrize("K", [1, 2, 3, 1024])
def test_apply_bit_for_bit_at_every_size_and_alignment(K):
    x, y = knots(K)
    m = metrics.IsotonicMap(x, y)
    cal = metrics.Calibrator("cuda", m)
    for n in (1, 63, 64, 65, 257, 65836):
        pb = inputs(x, n)
        want = metrics.isotonic_apply_host(pb.view(np.float32), x, y).view(np.uint32)
        assert np.array_equal(apply_device(cal, pb), want), (K, n)
        assert np.array_equal(apply_device(cal, pb, in_place=True), want), (K, n, "in place")
        if n in (1, 65, 257, 65836):
            for io, oo in ((1, 1), (2, 2), (3, 3), (1, 0), (0, 3), (2, 1)):       # vector body with a head, and all-scalar
                assert np.array_equal(apply_device(cal, pb, io, oo), want), (K, n, io, oo)
            for io in (1, 2, 3):
                assert np.array_equal(apply_device(cal, pb, io, in_place=True), want), (K, n, io, "in place")
    # what must hold whatever the knots are
    pb = inputs(x, 65836)
    got = apply_device(cal, pb)
    u = np.where(pb == 0x80000000, 0, pb)
    bad = u > 0x3F800000
    assert bad.sum() >= INVALID_BITS.size - 1 and np.array_equal(got[bad], pb[bad])        # unchanged, NaN payloads included
    v = np.sort(u[~bad].view(np.float32))
    out = metrics.isotonic_apply_host(v, x, y)
    dev = apply_device(cal, bits(v)).view(np.float32)
    assert np.array_equal(bits(dev), bits(out)) and bool(np.all(dev[1:] >= dev[:-1]))      # sorted in, non-decreasing out
    assert dev[0] == y[0] and dev[-1] == y[-1]
    knots_out = apply_device(cal, bits(x)).view(np.float32)
    assert np.array_equal(bits(knots_out), bits(y))                                        # exact at every knot


def test_apply_numpy_tensors_and_a_graph_replay():
    x, y = knots(1024)
    cal = metrics.Calibrator("cuda", metrics.IsotonicMap(x, y))
    pb = inputs(x, 4099)
    p = pb.view(np.float32)
    want = metrics.isotonic_apply_host(p, x, y)
    got = cal.apply(p.reshape(-1, 1))                          # numpy in, numpy out, the shape kept
    assert isinstance(got, np.ndarray) and got.shape == (4099, 1) and np.array_equal(bits(got.reshape(-1)), bits(want))
    d = up(pb.view(np.int32)).view(torch.float32)
    fresh = cal.apply(d)                                       # a tensor in, a new tensor out
    assert fresh.data_ptr() != d.data_ptr() and np.array_equal(bits(fresh.cpu().numpy()), bits(want))
    assert cal.apply(d[:0]).numel() == 0                       # n == 0
    out = torch.zeros_like(d)
    eager = cal.apply(d, out=out).cpu().numpy().copy()
    out.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cal.apply(d, out=out)
    g.replay()
    assert np.array_equal(bits(out.cpu().numpy()), bits(eager))
    pb2 = inputs(x, 4099, seed=5)                              # a replay reads the new input
    d.copy_(up(pb2.view(np.int32)).view(torch.float32))
    g.replay()
    assert np.array_equal(bits(out.cpu().numpy()), bits(metrics.isotonic_apply_host(pb2.view(np.float32), x, y)))
    with pytest.raises(ValueError):
        cal.apply(d, out=out[:10])
    with pytest.raises(ValueError):
        cal.apply(d.double())


# ---- through the Estimator ----------------------------------------------------------------------------------------------------
def criteo_estimator(B, steps, model_dir=None, script="deepfm"):
    from recsys_amd import synthetic
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    mod = importlib.import_module("recsys_amd." + script)
    lin, emb = build_feature_columns(16, "indicator_all")
    layout = CriteoLayout.from_columns(emb)
    host_batches = synthetic.criteo_id_batches(layout, steps, B, seed=11)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-2,
              "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": B}

    def fn():
        for i, y, _ in host_batches:
            yield {"ids": i}, y.reshape(-1, 1)
    est = Estimator(mod.model_fn, model_dir, params, RunConfig(device="cuda", seed=3, log_step_count_steps=1000000))
    return est, fn, host_batches, layout


def lines(out, prefix):
    return [ln for ln in out.splitlines() if ln.startswith(prefix)]


def host_map(labels, prob, M):
    return metrics.isotonic_from_table(metrics.quantile_table_host(labels, prob, M))


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


@pytest.fixture(scope="module")
def fitted(tmp_path_factory):
    """The trained deepfm.py Estimator of the recipe (B = 64, 5 steps) in a model_dir, its predictions and labels."""
    B, steps = 64, 5
    model_dir = str(tmp_path_factory.mktemp("model"))
    est, fn, host_batches, layout = criteo_estimator(B, steps, model_dir)
    est.train(fn, steps=steps)
    prob = np.array([r["prob"] for r in est.predict(fn)], np.float32)
    labels = np.concatenate([y.reshape(-1) for _, y, _ in host_batches]).astype(np.float32)
    return {"est": est, "fn": fn, "steps": steps, "B": B, "prob": prob, "labels": labels, "model_dir": model_dir,
            "batches": host_batches, "layout": layout}


def test_estimator_fits_writes_and_applies_the_map(fitted, capsys):
    est, fn, steps, prob, labels = (fitted[k] for k in ("est", "fn", "steps", "prob", "labels"))
    capsys.readouterr()
    off = est.evaluate(fn, steps=steps)
    out = capsys.readouterr().out
    line_off = lines(out, "INFO:Saving dict")
    assert set(off) == {"AUC", "Accuracy", "loss", "global_step"} and len(line_off) == 1
    assert re.fullmatch(r"INFO:Saving dict for global step \d+: AUC = \S+, Accuracy = \S+, global_step = \d+, loss = \S+", line_off[0])
    assert not lines(out, "INFO:calibration map") and est.last_calibration_map is None
    assert not [f for f in os.listdir(fitted["model_dir"]) if f.startswith("calibration")]

    M = 16
    est.config.calibration_fit = M
    fit = est.evaluate(fn, steps=steps)
    out = capsys.readouterr().out
    x, y = host_map(labels, prob, M)
    cmap = est.last_calibration_map
    assert np.array_equal(bits(cmap.x), bits(x)) and np.array_equal(bits(cmap.y), bits(y))          # knot for knot, in bits
    assert set(fit) == set(off) | {"calibration_knots"} and fit["calibration_knots"] == x.size >= 2
    assert all(fit[k] == off[k] for k in off) and lines(out, "INFO:Saving dict") == line_off       # AUC_exact is not reported
    P = int((labels > 0.5).sum())
    assert (cmap.bins, cmap.examples, cmap.positives, cmap.global_step, cmap.script) == (M, labels.size, P, est.global_step, "deepfm")
    table = metrics.quantile_table_host(labels, prob, M)
    assert np.array_equal(cmap.table, table) and cmap.ece == metrics.calibration_from_table(table, 0)["ECE"]
    path = os.path.join(fitted["model_dir"], "calibration-%d.json" % est.global_step)
    assert lines(out, "INFO:calibration map") == ["INFO:calibration map: K = %d, V = %d, P = %d, path = %s"
                                                  % (x.size, labels.size, P, path)]
    assert not lines(out, "WARNING:")
    assert sorted(f for f in os.listdir(fitted["model_dir"]) if f.startswith("calibration")) == [os.path.basename(path)]
    assert metrics.IsotonicMap.load(path).to_json() == cmap.to_json()
    from recsys_amd import checkpoint
    assert checkpoint.latest(fitted["model_dir"]).endswith("model.ckpt-%d.pt" % est.global_step)    # the glob does not see it

    est.config.exact_auc = True                                # with exact_auc the statistic is reported as before
    both = est.evaluate(fn, steps=steps)
    assert both["AUC_exact"] == metrics.exact_auc_host(labels, prob)["AUC_exact"] and both["calibration_knots"] == x.size
    est.config.exact_auc = False

    N = 20
    est.config.calibration_fit, est.config.calibration_bins = 0, N
    capsys.readouterr()
    raw = est.evaluate(fn, steps=steps)
    line_raw = lines(capsys.readouterr().out, "INFO:Saving dict")
    est.config.calibration_apply = True
    for source in ("memory", "file"):
        if source == "file":
            est.last_calibration_map = None                    # the file of this step is found
        app = est.evaluate(fn, steps=steps)
        line_app = lines(capsys.readouterr().out, "INFO:Saving dict")
        mapped = metrics.isotonic_apply_host(prob, x, y)
        t2, invalid = metrics.calibration_bins_host(labels, mapped, N)
        want = metrics.calibration_from_table(t2, invalid)
        assert invalid == 0 and (app["ECE_cal"], app["MCE_cal"], app["PCOC_cal"]) == (want["ECE"], want["MCE"], want["PCOC"])
        assert set(app) == set(raw) | {"ECE_cal", "MCE_cal", "PCOC_cal"} and all(same(app[k], raw[k]) for k in raw)
        assert line_app == [line_raw[0] + ", ECE_cal = %.7g, PCOC_cal = %.7g" % (app["ECE_cal"], app["PCOC_cal"])]
    est.last_calibration_map = cmap
    est.config.calibration_apply, est.config.calibration_bins = False, 0
    again = est.evaluate(fn, steps=steps)                      # everything off again: today's keys and line
    assert again == off and lines(capsys.readouterr().out, "INFO:Saving dict") == line_off


def test_fit_is_refused_with_one_warning_and_no_file(tmp_path, capsys):
    B, steps = 64, 2
    est, fn, host_batches, _ = criteo_estimator(B, steps, str(tmp_path / "model"))
    est.train(fn, steps=steps)
    est.config.calibration_fit = 16
    real = est._infer_step

    def poisoned(features, labels_, mode):
        prob_, loss, lab = real(features, labels_, mode)
        prob_ = prob_.clone()
        prob_.reshape(-1)[3] = float("nan")
        return prob_, loss, lab
    est._infer_step = poisoned
    capsys.readouterr()
    bad = est.evaluate(fn, steps=steps)
    est._infer_step = real
    out = capsys.readouterr().out
    assert bad["calibration_knots"] == 0 and est.last_calibration_map is None
    assert len(lines(out, "WARNING:calibration_fit:")) == 1 and "%d of %d" % (steps, steps * B) in lines(out, "WARNING:")[0]
    assert not lines(out, "INFO:calibration map")

    def no_positives():
        for i, y, _ in host_batches:
            yield {"ids": i}, np.zeros_like(y).reshape(-1, 1)
    none = est.evaluate(no_positives, steps=steps)
    out = capsys.readouterr().out
    assert none["calibration_knots"] == 0 and len(lines(out, "WARNING:calibration_fit:")) == 1 and "0 positives" in out
    assert not [f for f in os.listdir(str(tmp_path / "model")) if f.startswith("calibration")]


def test_bad_settings_are_refused_before_any_batch(tmp_path):
    est, fn, _, _ = criteo_estimator(32, 1, str(tmp_path / "model"))
    est.train(fn, steps=1)
    read = []

    def watched():
        read.append(1)
        yield from fn()
    cfg = est.config
    cfg.calibration_apply = True
    with pytest.raises(RsxError, match="calibration_bins"):
        est.evaluate(watched, steps=1)
    cfg.calibration_bins = 20
    with pytest.raises(RsxError, match="no calibration map for global step %d" % est.global_step):
        est.evaluate(watched, steps=1)
    other = metrics.IsotonicMap([0.25, 0.5], [0.125, 0.75], global_step=est.global_step + 1, script="deepfm")
    est.last_calibration_map = other                           # a map of another step is not taken
    other.save(os.path.join(est.model_dir, "calibration-%d.json" % (est.global_step + 1)))
    with pytest.raises(RsxError, match="no calibration map"):
        est.evaluate(watched, steps=1)
    est.last_calibration_map = metrics.IsotonicMap([0.25, 0.5], [0.125, 0.75], global_step=est.global_step, script="deepfm")
    cfg.calibration_fit = 16
    with pytest.raises(RsxError, match="in-sample"):
        est.evaluate(watched, steps=1)
    cfg.calibration_apply = False
    for M in (1, 1025, -4):
        cfg.calibration_fit = M
        with pytest.raises(RsxError, match="calibration_fit"):
            est.evaluate(watched, steps=1)

    class TwoRanks:
        world, rank = 2, 0
    for fit, app in ((16, False), (0, True)):
        cfg.calibration_fit, cfg.calibration_apply = fit, app
        est.store.dp = TwoRanks()
        try:
            with pytest.raises(RsxError, match="data-parallel evaluation is not supported"):
                est.evaluate(watched, steps=1)
        finally:
            est.store.dp = None
    assert read == []
    res = est.evaluate(watched, steps=1)                       # the hand-made map of this step is applied
    assert read == [1] and "ECE_cal" in res


def test_din_fits_and_applies_through_its_own_pipeline(tmp_path, capsys):
    from recsys_amd import din, synthetic
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.input_pipeline import write_din_shard
    B, steps, P, M, N = 64, 4, 10, 16, 10
    b = synthetic.din_batch(np.random.default_rng(5), B * steps, P=P, n_item=500, n_cate=12)
    path = str(tmp_path / "valid2")
    write_din_shard(path, b)
    params = {"embedding_size": 16, "learning_rate": 1e-3, "dropout": 0.5, "max_batch_size": B, "hist_len": P,
              "n_item": 500, "n_cate": 12}

    def fn():
        return din.input_fn([path], B, 1, False, P)
    est = Estimator(din.model_fn, None, params, RunConfig(device="cuda", seed=3, log_step_count_steps=1000000,
                                                           calibration_fit=M))
    est.train(fn, steps=steps)
    fit = est.evaluate(fn, steps=steps)
    prob = np.array([r["prob"] for r in est.predict(fn)], np.float32)
    labels = b["label"].astype(np.float32)
    x, y = host_map(labels, prob, M)
    cmap = est.last_calibration_map
    assert np.array_equal(bits(cmap.x), bits(x)) and np.array_equal(bits(cmap.y), bits(y)) and cmap.script == "din"
    assert fit["calibration_knots"] == x.size
    assert "path = None" in lines(capsys.readouterr().out, "INFO:calibration map")[0]      # no model_dir: no file
    est.config.calibration_fit, est.config.calibration_apply, est.config.calibration_bins = 0, True, N
    app = est.evaluate(fn, steps=steps)
    want = metrics.calibration_from_table(metrics.calibration_bins_host(labels, metrics.isotonic_apply_host(prob, x, y), N)[0], 0)
    assert (app["ECE_cal"], app["MCE_cal"], app["PCOC_cal"]) == (want["ECE"], want["MCE"], want["PCOC"])


# ---- serving --------------------------------------------------------------------------------------------------------------------
def test_serving_deepfm_on_the_fused_and_the_device_parse_path(fitted, tmp_path):
    from recsys_amd import serving
    from tests import device_parse_util as U
    est, prob, labels = fitted["est"], fitted["prob"], fitted["labels"]
    before = est.last_calibration_map
    x, y = host_map(labels, prob, 16)
    est.last_calibration_map = metrics.IsotonicMap(x, y, bins=16, examples=labels.size, positives=int(labels.sum()),
                                                   global_step=est.global_step, script="deepfm")
    d = est.export_savedmodel(str(tmp_path / "auto"))
    d_off = est.export_savedmodel(str(tmp_path / "off"), calibration="off")
    assert sorted(os.listdir(d)) == ["calibration.json", "model.json", "variables.npz"]
    assert sorted(os.listdir(d_off)) == ["model.json", "variables.npz"]
    assert open(os.path.join(d, "model.json")).read() == open(os.path.join(d_off, "model.json")).read()
    cal = serving.Predictor.load(d, max_batch_size=256)
    raw = serving.Predictor.load(d, max_batch_size=256, calibrated=False)
    off = serving.Predictor.load(d_off, max_batch_size=256)
    assert cal.path == raw.path == off.path == "fused"
    assert (cal.calibrated, raw.calibrated, off.calibrated) == (True, False, False)
    assert cal.calibration.to_json() == est.last_calibration_map.to_json() == raw.calibration.to_json() and off.calibration is None
    with pytest.raises(RsxError, match="calibrated=True"):
        serving.Predictor.load(d_off, calibrated=True)
    assert serving.Predictor.load(d, max_batch_size=8, calibrated=True).calibrated
    ids = np.concatenate([i for i, _, _ in fitted["batches"]])
    for n in (1, 200, 300):                                    # 300: two chunks
        want_raw = raw.predict({"ids": ids[:n]})["prob"]
        assert np.array_equal(bits(off.predict({"ids": ids[:n]})["prob"]), bits(want_raw))
        want = metrics.isotonic_apply_host(want_raw, x, y)
        assert n == 1 or not np.array_equal(bits(want), bits(want_raw))
        for it in range(3):                                    # eager warm-up, capture + replay, replay
            got = cal.predict({"ids": ids[:n]})["prob"]
            assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (n, it)
    assert "graph" in cal._graphs[200]
    assert np.array_equal(bits(cal.calibrate(want_raw)), bits(want)) and np.array_equal(bits(raw.calibrate(want_raw)), bits(want))
    with pytest.raises(RsxError, match="calibration.json"):
        off.calibrate(want_raw)

    # the device parse: the apply launch sits behind the predict launch in the request's graph
    lay = U.layout()
    from recsys_amd.input_pipeline import criteo_parse_spec
    pool = U.canonical_corpus(lay, criteo_parse_spec(lay), n=300)[::2]
    on = serving.Predictor.load(d, max_batch_size=64, device_parse=True)
    host = serving.Predictor.load(d, max_batch_size=64, calibrated=False)
    assert on.parse_path == "device" and on.calibrated
    for n in (1, 100):
        want = metrics.isotonic_apply_host(host.predict_examples(pool[:n])["prob"], x, y)
        for it in range(3):
            assert np.array_equal(bits(on.predict_examples(pool[:n])["prob"]), bits(want)), (n, it)
        assert np.array_equal(bits(cal.predict_examples(pool[:n])["prob"]), bits(want))            # the host parse, calibrated
    assert "graph" in on._graphs[("examples", 64)]

    # a map of another step: not taken at export, refused at load
    est.last_calibration_map = metrics.IsotonicMap(x, y, global_step=est.global_step + 1, script="deepfm")
    mdir_map = os.path.join(fitted["model_dir"], "calibration-%d.json" % est.global_step)
    hidden = mdir_map + ".hidden"
    if os.path.exists(mdir_map):
        os.replace(mdir_map, hidden)                           # (the file an earlier test's fit left for this step)
    try:
        d_none = est.export_savedmodel(str(tmp_path / "other"))
        assert sorted(os.listdir(d_none)) == ["model.json", "variables.npz"]
        with pytest.raises(RsxError, match="require"):
            est.export_savedmodel(str(tmp_path / "other"), calibration="require")
        with pytest.raises(RsxError, match="calibration"):
            est.export_savedmodel(str(tmp_path / "other"), calibration="sometimes")
    finally:
        if os.path.exists(hidden):
            os.replace(hidden, mdir_map)
    wrong = str(tmp_path / "wrong")
    shutil.copytree(d, wrong)
    for change in ({"global_step": est.global_step + 1}, {"script": "fm"}):
        doc = dict(json.load(open(os.path.join(d, "calibration.json"))), **change)
        json.dump(doc, open(os.path.join(wrong, "calibration.json"), "w"))
        for flag in (None, False, True):
            with pytest.raises(RsxError, match="belongs to"):
                serving.Predictor.load(wrong, calibrated=flag)
    json.dump({"format": "x"}, open(os.path.join(wrong, "calibration.json"), "w"))
    with pytest.raises(RsxError, match="unknown format"):
        serving.Predictor.load(wrong)
    est.last_calibration_map = before


def tiny_model(kind):
    """A tiny model of `kind` with random variables (tests/test_gpu_device_parse.py's recipe) -> its Estimator."""
    from recsys_amd import serving
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.feature_columns import build_feature_columns
    mod = importlib.import_module("recsys_amd." + kind)
    if kind == "din":
        params = {"embedding_size": 32, "learning_rate": 1e-3, "dropout": 0.5, "max_batch_size": 64, "hist_len": 30,
                  "n_item": 300, "n_cate": 20}
    else:
        lin, emb = build_feature_columns(16, "numeric")
        params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
                  "dropout": 0.5, "deep_layers": "8,8", "max_batch_size": 64, "cross_layers": 3}
    est = Estimator(mod.model_fn, None, params, RunConfig(device="cuda", seed=5))
    serving._build_store(est, kind)
    return est


def map_over(raw, est, script):
    """A hand-made map whose knots lie among the model's own probabilities."""
    x = np.unique(np.quantile(raw, np.linspace(0.02, 0.98, 33)).astype(np.float32))
    y = np.sort((x.astype(np.float64) ** 2).astype(np.float32))
    return metrics.IsotonicMap(x, y, bins=33, examples=raw.size, positives=1, global_step=est.global_step, script=script)


def test_serving_dcn_on_the_layers_path(tmp_path):
    from recsys_amd import serving
    from recsys_amd.feature_columns import CriteoLayout
    from tests.parity_util import synth_ids
    est = tiny_model("dcn")
    layout = CriteoLayout.from_columns(est.params["embedding_feature_columns"])
    ids = synth_ids(np.random.default_rng(4), 150, layout.row_off)
    d_off = est.export_savedmodel(str(tmp_path / "off"), calibration="off")
    off = serving.Predictor.load(d_off, max_batch_size=64)
    want_raw = off.predict({"ids": ids})["prob"]
    est.last_calibration_map = cmap = map_over(want_raw, est, "dcn")
    assert cmap.knots >= 8
    d = est.export_savedmodel(str(tmp_path / "auto"), calibration="require")
    cal = serving.Predictor.load(d, max_batch_size=64)
    raw = serving.Predictor.load(d, max_batch_size=64, calibrated=False)
    assert cal.path == raw.path == "layers" and cal.calibrated and not raw.calibrated
    want = metrics.isotonic_apply_host(want_raw, cmap.x, cmap.y)
    assert not np.array_equal(bits(want), bits(want_raw))
    for it in range(3):                                        # 150 rows at 64 per chunk; the Estimator's graph replays
        assert np.array_equal(bits(cal.predict({"ids": ids})["prob"]), bits(want)), it
        assert np.array_equal(bits(raw.predict({"ids": ids})["prob"]), bits(want_raw)), it
    assert np.array_equal(bits(cal.predict({"ids": ids}, raw=True)["prob"]), bits(want_raw))


def test_serving_din_predict_is_mapped_and_ranking_stays_raw(tmp_path):
    from recsys_amd import serving
    est = tiny_model("din")
    rng = np.random.default_rng(6)
    n, P = 100, 30
    feats = {"i_id": rng.integers(1, 300, n).astype(np.int32), "i_cate": rng.integers(1, 20, n).astype(np.int32),
             "u_iid_seq": rng.integers(0, 300, (n, P)).astype(np.int32), "u_icat_seq": rng.integers(0, 20, (n, P)).astype(np.int32)}
    d_off = est.export_savedmodel(str(tmp_path / "off"), calibration="off")
    off = serving.Predictor.load(d_off, max_batch_size=64)
    want_raw = off.predict(feats)["prob"]
    est.last_calibration_map = cmap = map_over(want_raw, est, "din")
    d = est.export_savedmodel(str(tmp_path / "auto"))
    cal = serving.Predictor.load(d, max_batch_size=64)
    raw = serving.Predictor.load(d, max_batch_size=64, calibrated=False)
    assert cal.calibrated and cal.calibration.script == "din"
    want = metrics.isotonic_apply_host(want_raw, cmap.x, cmap.y)
    assert not np.array_equal(bits(want), bits(want_raw))
    for it in range(3):
        assert np.array_equal(bits(cal.predict(feats)["prob"]), bits(want)), it
    assert np.array_equal(bits(raw.predict(feats)["prob"]), bits(want_raw))
    hist = (feats["u_iid_seq"][0], feats["u_icat_seq"][0])
    ranked = [p.rank_candidates(hist[0], hist[1], feats["i_id"], feats["i_cate"])["prob"] for p in (cal, raw, off)]
    assert np.array_equal(bits(ranked[0]), bits(ranked[1])) and np.array_equal(bits(ranked[0]), bits(ranked[2]))      # raw scores
    assert np.array_equal(bits(cal.calibrate(ranked[0])), bits(metrics.isotonic_apply_host(ranked[0], cmap.x, cmap.y)))
    cal.rank_path = raw.rank_path = "layers"                   # the ranking that goes through predict(): raw all the same
    through = [p.rank_candidates(hist[0], hist[1], feats["i_id"], feats["i_cate"])["prob"] for p in (cal, raw)]
    assert np.array_equal(bits(through[0]), bits(through[1])) and through[0].shape == (n,)
