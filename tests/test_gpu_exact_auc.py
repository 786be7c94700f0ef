"""The exact ROC AUC on the device (rsx_auc_exact_append / rsx_auc_exact_finalize, csrc/auc_exact.hip; metrics.ExactAUC;
RunConfig.exact_auc) against metrics.exact_auc_host, whose definition tests/test_exact_auc_cpu.py holds to a pair count.
Integers are compared as integers: no tolerance anywhere."""
import math

import numpy as np
import pytest
import torch

from recsys_amd import metrics
from recsys_amd._lib import lib

pytestmark = pytest.mark.gpu

WORDS = ("u2", "positives", "negatives", "invalid")
INVALID = np.array([np.nan, np.inf, -np.inf, -1e-9, 1.0000001], np.float32)


def tile():
    return int(lib().rsx_auc_exact_tile())


def words(res):
    return tuple(res[k] for k in WORDS)


def device_words(y, p, batch=None, capacity=None):
    dev = torch.device("cuda")
    ex = metrics.ExactAUC(dev, capacity)
    yd, pd = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
    step = batch or max(1, len(p))
    for i in range(0, len(p), step):
        ex.update(yd[i:i + step], pd[i:i + step])
    return ex.result()


def check(y, p, **kw):
    got, want = device_words(y, p, **kw), metrics.exact_auc_host(y, p)
    assert words(got) == words(want)
    assert got["AUC_exact"] == want["AUC_exact"] or (math.isnan(got["AUC_exact"]) and math.isnan(want["AUC_exact"]))
    return got


def distinct_scores(rng, n):
    """n different fp32 values of [0, 1]: distinct bit patterns below 0x3F800000 (subnormals included), plus 0.0 and 1.0."""
    bits = (rng.choice(0x3F800000 - 2, size=n, replace=False) + 2).astype(np.uint32)
    bits[:min(n, 3)] = np.array([0x3F800000, 0, 1], np.uint32)[:min(n, 3)]
    return rng.permutation(bits).view(np.float32)


def labels_for(rng, p):
    return (rng.random(len(p)) < 0.2 + 0.6 * p).astype(np.float32)


def sizes():
    T = tile()
    return [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17, 70001, 300007]


@pytest.mark.parametrize("which", range(14))
@pytest.mark.parametrize("distinct", [None, 7])
def test_sizes_on_the_tile_edges(which, distinct):
    n = sizes()[which]
    rng = np.random.default_rng(17 * n + (distinct or 0))
    if distinct is None:
        p = distinct_scores(rng, n)
    else:                                                  # tie groups that cross tile and workgroup borders
        p = rng.random(distinct).astype(np.float32)[rng.integers(0, distinct, n)]
    check(labels_for(rng, p), p)


def test_more_tiles_than_workgroups():
    """Above 1024 tiles the launches' workgroups stride over the tiles and the one-workgroup tile scan carries from one round of
    1024 tiles into the next: the smallest size at which both happen."""
    n = 1024 * tile() + tile() + 5
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 0x3F800001, n).astype(np.uint32)
    heavy = rng.random(n) < 0.3                            # 30 % of the examples on 5 scores: groups longer than many tiles
    bits[heavy] = rng.integers(0, 0x3F800001, 5).astype(np.uint32)[rng.integers(0, 5, int(heavy.sum()))]
    p = bits.view(np.float32)
    check(labels_for(rng, p), p)


def test_all_scores_equal_is_exactly_one_half():
    n = 3 * tile() + 17
    rng = np.random.default_rng(2)
    y = (rng.random(n) < 0.3).astype(np.float32)
    got = check(y, np.full(n, 0.25, np.float32))
    assert got["u2"] == got["positives"] * got["negatives"] and got["AUC_exact"] == 0.5


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_one_class(label):
    n = tile() + 5
    p = distinct_scores(np.random.default_rng(3), n)
    got = check(np.full(n, label, np.float32), p)
    assert math.isnan(got["AUC_exact"]) and got["u2"] == 0


@pytest.mark.parametrize("shift", [0, 7, 15, 23])
def test_scores_that_differ_in_one_radix_digit(shift):
    """Bit patterns d << shift: all keys agree outside one (or two adjacent) 8-bit digits of the sort; shift 0 are subnormals."""
    rng = np.random.default_rng(shift)
    n = 2 * tile() + 3
    top = 128 if shift == 23 else 256                      # 127 << 23 = 1.0 is the largest valid pattern
    p = (rng.integers(0, top, n).astype(np.uint32) << np.uint32(shift)).view(np.float32)
    assert p.min() >= 0 and p.max() <= 1
    check((rng.random(n) < 0.4).astype(np.float32), p)


def test_invalid_scores_at_random_positions():
    rng = np.random.default_rng(5)
    n = 2 * tile() + 100
    p = distinct_scores(rng, n)
    at = rng.choice(n, 40 * INVALID.size, replace=False)
    p[at] = np.tile(INVALID, 40)
    p[rng.choice(np.setdiff1d(np.arange(n), at), 3, replace=False)] = np.float32(-0.0)
    y = labels_for(rng, np.nan_to_num(np.clip(p, 0, 1)))
    got = check(y, p)
    assert got["invalid"] == 40 * INVALID.size
    assert math.isnan(metrics.exact_auc_reported(got)) and not math.isnan(got["AUC_exact"])


def test_streaming_does_not_depend_on_batches_or_order(monkeypatch):
    rng = np.random.default_rng(6)
    n = 20000
    p = np.concatenate([distinct_scores(rng, n // 2), rng.random(50).astype(np.float32)[rng.integers(0, 50, n - n // 2)]])
    p = rng.permutation(p)
    y = labels_for(rng, p)
    want = words(metrics.exact_auc_host(y, p))
    for batch in (1, 256, 4096):                           # 20 000 = 4 * 4096 + 3616: an uneven last batch
        assert words(device_words(y, p, batch=batch, capacity=n)) == want
    perm = rng.permutation(n)
    assert words(device_words(y[perm], p[perm], batch=4096, capacity=n)) == want
    dev = torch.device("cuda")
    monkeypatch.setattr(metrics.ExactAUC, "GROW_FROM", 1000)
    ex = metrics.ExactAUC(dev)                             # a buffer that grows: 1000 -> 2000 -> ... -> 32000
    assert ex.keys.numel() == 1000
    yd, pd = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
    mid = None
    for i in range(0, n, 777):
        ex.update(yd[i:i + 777], pd[i:i + 777])
        if mid is None and i > n // 2:                     # result() in mid-stream reorders the keys and keeps the multiset
            mid = ex.result()
            assert words(mid) == words(metrics.exact_auc_host(y[:i + 777], p[:i + 777]))
    assert ex.keys.numel() >= n and mid is not None
    assert words(ex.result()) == want
    assert words(ex.result()) == want                      # and again, on keys that are already sorted
    with pytest.raises(metrics.RsxError):
        device_words(y, p, batch=4096, capacity=n - 1)


def test_numpy_inputs_and_empty_stream():
    rng = np.random.default_rng(7)
    p = rng.random(300).astype(np.float32)
    y = labels_for(rng, p)
    ex = metrics.ExactAUC("cuda")
    got = ex.result()
    assert words(got) == (0, 0, 0, 0) and math.isnan(got["AUC_exact"])
    ex.update(y.reshape(-1, 1), p.reshape(-1, 1))
    assert words(ex.result()) == words(metrics.exact_auc_host(y, p))


def test_estimator_reports_auc_exact(capsys):
    from recsys_amd import deepfm, synthetic
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    lin, emb = build_feature_columns(16, "indicator_all")
    layout = CriteoLayout.from_columns(emb)
    B, steps = 64, 5
    host = synthetic.criteo_id_batches(layout, steps, B, seed=11)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-2,
              "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": B}

    def fn():
        for i, y, _ in host:
            yield {"ids": i}, y.reshape(-1, 1)
    est = Estimator(deepfm.model_fn, None, params, RunConfig(device="cuda", seed=3, log_step_count_steps=1000000))
    est.train(fn, steps=steps)
    capsys.readouterr()
    off = est.evaluate(fn, steps=steps)
    line_off = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("INFO:Saving dict")]
    assert "AUC_exact" not in off and len(line_off) == 1 and "AUC_exact" not in line_off[0]
    est.config.exact_auc = True
    on = est.evaluate(fn, steps=steps)
    out_on = capsys.readouterr().out.splitlines()
    line_on = [ln for ln in out_on if ln.startswith("INFO:Saving dict")]
    assert set(on) == set(off) | {"AUC_exact"}
    for k in off:                                          # the other keys: bit for bit what the flag-off evaluate gives
        assert on[k] == off[k], k
    assert line_on == [line_off[0] + ", AUC_exact = %.7g" % on["AUC_exact"]]
    assert not any(ln.startswith("WARNING:") for ln in out_on)
    prob = np.array([r["prob"] for r in est.predict(fn)], np.float32)
    labels = np.concatenate([y.reshape(-1) for _, y, _ in host]).astype(np.float32)
    assert prob.shape == (steps * B,)
    want = metrics.exact_auc_host(labels, prob)
    assert want["invalid"] == 0 and on["AUC_exact"] == want["AUC_exact"]

    # a NaN among the probabilities: nan and ONE warning with the count
    real = est._infer_step

    def poisoned(features, labels_, mode):
        prob_, loss, lab = real(features, labels_, mode)
        prob_ = prob_.clone()
        prob_.reshape(-1)[3] = float("nan")
        return prob_, loss, lab
    est._infer_step = poisoned
    bad = est.evaluate(fn, steps=steps)
    est._infer_step = real
    warn = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("WARNING:")]
    assert math.isnan(bad["AUC_exact"]) and len(warn) == 1 and ("%d of %d" % (steps, steps * B)) in warn[0]
