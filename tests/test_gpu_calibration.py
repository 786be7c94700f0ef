"""The calibration tables on the device (rsx_calibration_update, csrc/calibration.hip; metrics.Calibration;
RunConfig.calibration_bins / calibration_key) against metrics.calibration_bins_host / calibration_groups_host, whose definitions
tests/test_calibration_cpu.py holds to struct / fractions arithmetic.  Tables, records and the invalid count are compared as
integers: no tolerance anywhere."""
import math

import numpy as np
import pytest
import torch

from recsys_amd import metrics

pytestmark = pytest.mark.gpu

ONE = 1 << 32
INVALID = np.array([np.nan, np.inf, -np.inf, -1e-9, 1.0000001], np.float32)
GRID_SPAN = 256 * 256                    # the launch's bound: 256 workgroups of 256 threads; above it they stride


def host_records(g, y, p, n_groups):
    table, invalid = metrics.calibration_groups_host(g, y, p, n_groups)
    live = np.flatnonzero(table[:, 0])
    return np.concatenate([live.reshape(-1, 1).astype(np.int64), table[live]], axis=1), invalid


def device(y, p, n_bins=None, g=None, n_groups=None, batch=None):
    dev = torch.device("cuda")
    cal = metrics.Calibration(dev, n_bins, n_groups)
    yd, pd = torch.from_numpy(np.ascontiguousarray(y)).to(dev), torch.from_numpy(np.ascontiguousarray(p)).to(dev)
    gd = None if g is None else torch.from_numpy(np.ascontiguousarray(g)).to(dev)
    step = batch or max(1, len(p))
    for i in range(0, len(p), step):
        cal.update(yd[i:i + step], pd[i:i + step], None if gd is None else gd[i:i + step])
    return cal.result(per_group=True)


def check_bins(y, p, n_bins, **kw):
    res = device(y, p, n_bins, **kw)
    table, invalid = metrics.calibration_bins_host(y, p, n_bins)
    assert res["table"].dtype == np.int64 and res["table"].shape == (n_bins, 3)
    assert np.array_equal(res["table"], table) and res["invalid"] == invalid
    want = metrics.calibration_from_table(table, invalid)
    for k in want:
        assert res[k] == want[k] or (math.isnan(res[k]) and math.isnan(want[k])), k
    return res


def check_groups(g, y, p, n_groups, **kw):
    res = device(y, p, None, g, n_groups, **kw)
    rec, invalid = host_records(g, y, p, n_groups)
    assert res["records"].dtype == np.int64 and res["records"].shape == rec.shape
    assert np.array_equal(res["records"], rec) and res["invalid"] == invalid
    want = metrics.group_calibration_from_table(rec[:, 1:], invalid)
    assert {k: res[k] for k in want if k != "GCE"} == {k: want[k] for k in want if k != "GCE"}
    assert res["GCE"] == want["GCE"] or (math.isnan(res["GCE"]) and math.isnan(want["GCE"]))
    assert "table" not in res and "ECE" not in res
    return res


def labels_for(rng, p):
    return (rng.random(len(p)) < 0.1 + 0.8 * np.nan_to_num(np.clip(p, 0, 1))).astype(np.float32)


def scores(rng, n):
    """Random probabilities with the ends of the range among them."""
    p = rng.random(n).astype(np.float32)
    p[rng.random(n) < 0.02] = np.float32(0.0)
    p[rng.random(n) < 0.02] = np.float32(1.0)
    return p


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, GRID_SPAN + 300])
def test_stream_sizes_at_every_bin_count(n):
    rng = np.random.default_rng(7 * n)
    p = scores(rng, n)
    y = labels_for(rng, p)
    for n_bins in (2, 10, 1024):
        res = check_bins(y, p, n_bins)
        assert res["examples"] == n
    g = rng.integers(0, 5, n).astype(np.int32)
    check_groups(g, y, p, 5)


def test_one_bin_takes_everything_and_the_largest_sums():
    rng = np.random.default_rng(1)
    n = GRID_SPAN + 4321
    p = (np.float32(0.5) + np.float32(0.09) * rng.random(n).astype(np.float32)).astype(np.float32)
    res = check_bins(labels_for(rng, p), p, 10)             # every example in bin 5: the heaviest LDS contention
    assert res["table"][5, 0] == n
    ones = np.ones(n, np.float32)
    res = check_bins(ones, ones, 1024)                      # every p = 1.0: the largest q_sum
    assert res["table"][1023].tolist() == [n, n, n * ONE] and res["ECE"] == 0.0 and res["PCOC"] == 1.0
    res = check_groups(np.full(n, 3, np.int32), ones, ones, 5)
    assert res["records"].tolist() == [[3, n, n, n * ONE]]


def edge_bits(N):
    """k / N as fp32 and its two neighbours for every k, inside [0, 1], as bit patterns."""
    mid = (np.arange(N + 1, dtype=np.float64) / N).astype(np.float32)
    v = np.concatenate([mid, np.nextafter(mid, np.float32(-1)), np.nextafter(mid, np.float32(2)), np.array([-0.0], np.float32)])
    v = v[(v >= 0) & (v <= 1)].astype(np.float32)
    return v.view(np.int32).copy()


@pytest.mark.parametrize("N", [2, 10, 1024])
def test_bin_edge_values_uploaded_as_bit_patterns(N):
    bits = edge_bits(N)
    p = bits.view(np.float32)
    y = (np.arange(p.size) % 3 == 0).astype(np.float32)
    dev = torch.device("cuda")
    cal = metrics.Calibration(dev, N)
    cal.update(torch.from_numpy(y).to(dev), torch.from_numpy(bits).to(dev).view(torch.float32))
    res = cal.result()
    table, invalid = metrics.calibration_bins_host(y, p, N)
    assert invalid == 0 == res["invalid"] and np.array_equal(res["table"], table)
    assert res["table"][0, 0] >= 2 and int(res["table"][:, 0].sum()) == p.size      # 0.0 and -0.0 both in bin 0


def test_invalid_probabilities_and_group_ids_at_random_positions():
    rng = np.random.default_rng(2)
    n, G = 3000, 200
    p = scores(rng, n)
    g = rng.integers(0, G, n).astype(np.int32)
    at = rng.choice(n, 40 * INVALID.size + 60, replace=False)
    p[at[:40 * INVALID.size]] = np.tile(INVALID, 40)
    y = labels_for(rng, p)
    res = check_bins(y, p, 10)
    assert res["invalid"] == 40 * INVALID.size and all(math.isnan(v) for v in metrics.calibration_reported(res).values())
    assert not math.isnan(res["ECE"])
    g[at[40 * INVALID.size:]] = np.tile(np.array([G, G + 1, -1, -2 ** 31, 2 ** 31 - 1, 1 << 20], np.int64), 10).astype(np.int32)
    res = check_groups(g, y, p, G)
    assert res["invalid"] == 40 * INVALID.size + 60 and math.isnan(metrics.group_calibration_reported(res)["GCE"])
    wide = g.astype(np.int64)
    wide[at[-3:]] = [1 << 40, -(1 << 35), (1 << 32) + 5]     # ids int32 cannot hold: invalid, not wrapped
    rec, invalid = host_records(wide, y, p, G)
    cal = metrics.Calibration("cuda", None, G)
    cal.update(y, p, torch.from_numpy(wide).cuda())
    got = cal.result(per_group=True)
    assert got["invalid"] == invalid == 40 * INVALID.size + 60 and np.array_equal(got["records"], rec)


@pytest.mark.parametrize("n_groups", [1, 5])
def test_a_strided_group_column_is_read_in_place(n_groups):
    rng = np.random.default_rng(3 + n_groups)
    n, F, slot = 1000, 7, 3
    ids = rng.integers(0, n_groups, (n, F)).astype(np.int32)
    ids[:, [0, 1, 2, 4, 5, 6]] = -7                          # the neighbours of the column are all invalid ids
    p = scores(rng, n)
    y = labels_for(rng, p)
    dev = torch.device("cuda")
    col = torch.from_numpy(ids).to(dev)[:, slot]
    assert col.stride(0) == F and not col.is_contiguous()
    cal = metrics.Calibration(dev, None, n_groups)
    tensor, stride = metrics.group_column_on_device(col, dev)
    assert stride == F and tensor.data_ptr() == col.data_ptr()          # the view itself is what the launch reads
    cal.update(torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev), col)
    res = cal.result(per_group=True)
    rec, invalid = host_records(ids[:, slot], y, p, n_groups)
    assert invalid == 0 == res["invalid"] and np.array_equal(res["records"], rec) and res["GCE_groups"] == n_groups


def test_many_groups_and_one_hot_group():
    rng = np.random.default_rng(5)
    n = G = 70000
    p = scores(rng, n)
    y = labels_for(rng, p)
    res = check_groups(rng.permutation(G).astype(np.int32), y, p, G)       # one example per group
    assert res["GCE_groups"] == G
    res = check_groups(rng.integers(0, G, n).astype(np.int32), y, p, G)    # ~1 per group, some empty, some shared
    assert G // 2 < res["GCE_groups"] < G
    res = check_groups(np.full(n, G - 1, np.int32), y, p, G)               # every example on one row's three words
    assert res["GCE_groups"] == 1 and res["records"][0, 0] == G - 1 and res["records"][0, 1] == n


def test_tables_do_not_depend_on_batches_or_order():
    rng = np.random.default_rng(6)
    n, G, N = 1500, 40, 20
    p = scores(rng, n)
    p[::131] = np.float32(np.nan)
    y = labels_for(rng, p)
    g = rng.integers(0, G, n).astype(np.int32)
    table, invalid = metrics.calibration_bins_host(y, p, N)
    rec, _ = host_records(g, y, p, G)
    for order, batch in ((slice(None), None), (slice(None), 7), (slice(None, None, -1), 7), (slice(None, None, -1), None)):
        res = device(y[order], p[order], N, g[order], G, batch=batch)
        assert np.array_equal(res["table"], table) and np.array_equal(res["records"], rec) and res["invalid"] == invalid


def test_numpy_inputs_an_empty_update_and_updates_after_result():
    rng = np.random.default_rng(8)
    n, G, N = 900, 6, 10
    p = scores(rng, n)
    y = labels_for(rng, p)
    g = rng.integers(0, G, n).astype(np.int64)
    cal = metrics.Calibration("cuda", N, G)
    empty = cal.result(per_group=True)
    assert empty["examples"] == 0 and not empty["table"].any() and empty["records"].shape == (0, 4)
    assert math.isnan(empty["ECE"]) and math.isnan(empty["GCE"]) and empty["GCE_groups"] == 0
    cal.update(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64))
    assert not cal.result()["table"].any()
    cal.update(y[:500].reshape(-1, 1), p[:500].reshape(-1, 1), g[:500].reshape(-1, 1))     # numpy, int64, [B, 1]
    mid = cal.result(loss=0.5, per_group=True)
    table, _ = metrics.calibration_bins_host(y[:500], p[:500], N)
    assert np.array_equal(mid["table"], table) and np.array_equal(mid["records"], host_records(g[:500], y[:500], p[:500], G)[0])
    assert mid["NE"] == metrics.calibration_from_table(table, 0, loss=0.5)["NE"] and not math.isnan(mid["NE"])
    cal.update(y[500:], p[500:], g[500:])
    end = cal.result(per_group=True)
    assert np.array_equal(end["table"], metrics.calibration_bins_host(y, p, N)[0])
    assert np.array_equal(end["records"], host_records(g, y, p, G)[0])
    assert np.array_equal(mid["table"], table)                             # an earlier result is a copy
    with pytest.raises(ValueError):
        cal.update(y, p)                                                   # a group table needs the ids
    for bad in ((None, None), (1, None), (1025, None), (None, 0), (None, (1 << 22) + 1)):
        with pytest.raises(metrics.RsxError):
            metrics.Calibration("cuda", *bad)


def test_both_tables_in_one_launch_equal_the_two_taken_separately():
    rng = np.random.default_rng(9)
    n, G, N = GRID_SPAN + 1000, 300, 20
    p = scores(rng, n)
    p[rng.choice(n, 50, replace=False)] = np.float32(np.nan)
    y = labels_for(rng, p)
    g = rng.integers(0, G, n).astype(np.int32)
    both = device(y, p, N, g, G, batch=30000)
    bins = device(y, p, N, batch=30000)
    groups = device(y, p, None, g, G, batch=30000)
    assert np.array_equal(both["table"], bins["table"]) and np.array_equal(both["records"], groups["records"])
    assert both["invalid"] == bins["invalid"] == groups["invalid"] == 50
    assert both["ECE"] == bins["ECE"] and both["GCE"] == groups["GCE"] and both["examples"] == n - 50
    assert np.array_equal(both["table"], metrics.calibration_bins_host(y, p, N)[0])


# ---- through the Estimator ----------------------------------------------------------------------------------------------------
def criteo_estimator(B, steps):
    from recsys_amd import deepfm, synthetic
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    lin, emb = build_feature_columns(16, "indicator_all")
    layout = CriteoLayout.from_columns(emb)
    host_batches = synthetic.criteo_id_batches(layout, steps, B, seed=11)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-2,
              "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": B}

    def fn():
        for i, y, _ in host_batches:
            yield {"ids": i}, y.reshape(-1, 1)
    est = Estimator(deepfm.model_fn, None, params, RunConfig(device="cuda", seed=3, log_step_count_steps=1000000))
    return est, fn, host_batches, layout


def saving_lines(out):
    return [ln for ln in out.splitlines() if ln.startswith("INFO:Saving dict")]


def entropy(c):
    return -(c * math.log(c) + (1.0 - c) * math.log(1.0 - c))


def test_estimator_reports_the_calibration_figures(capsys):
    B, steps, N = 64, 5, 20
    est, fn, host_batches, layout = criteo_estimator(B, steps)
    key = "_c30"                                           # 10 buckets
    slot = [c.key for c in layout.columns].index(key)
    G = int(layout.columns[slot].rows)
    assert G == 10
    est.train(fn, steps=steps)
    capsys.readouterr()
    off = est.evaluate(fn, steps=steps)
    line_off = saving_lines(capsys.readouterr().out)
    assert set(off) == {"AUC", "Accuracy", "loss", "global_step"} and len(line_off) == 1
    assert not any(w in line_off[0] for w in ("ECE", "PCOC", "NE =", "GCE")) and est.last_calibration is None

    prob = np.array([r["prob"] for r in est.predict(fn)], np.float32)
    labels = np.concatenate([y.reshape(-1) for _, y, _ in host_batches]).astype(np.float32)
    groups = np.concatenate([i[:, slot] for i, _, _ in host_batches])
    table, invalid = metrics.calibration_bins_host(labels, prob, N)
    gtable, ginvalid = metrics.calibration_groups_host(groups, labels, prob, G)
    assert invalid == 0 == ginvalid
    want = metrics.calibration_from_table(table, 0, loss=off["loss"])
    gwant = metrics.group_calibration_from_table(gtable, 0)
    assert 0.0 < want["CTR"] < 1.0 and gwant["GCE_groups"] >= 2

    est.config.calibration_bins = N
    bins = est.evaluate(fn, steps=steps)
    out = capsys.readouterr().out
    assert set(bins) == set(off) | {"ECE", "MCE", "PCOC", "NE"}
    for k in off:                                          # the other keys: bit for bit what the flags-off evaluate gives
        assert bins[k] == off[k], k
    assert saving_lines(out) == [line_off[0] + ", ECE = %.7g, PCOC = %.7g, NE = %.7g" % (bins["ECE"], bins["PCOC"], bins["NE"])]
    assert not any(ln.startswith("WARNING:") for ln in out.splitlines())
    assert (bins["ECE"], bins["MCE"], bins["PCOC"]) == (want["ECE"], want["MCE"], want["PCOC"])
    assert bins["NE"] == bins["loss"] / entropy(int(table[:, 1].sum()) / int(table[:, 0].sum()))
    assert np.array_equal(est.last_calibration["table"], table) and "records" not in est.last_calibration

    est.config.calibration_key = key
    on = est.evaluate(fn, steps=steps)
    out = capsys.readouterr().out
    assert set(on) == set(off) | {"ECE", "MCE", "PCOC", "NE", "GCE", "GCE_groups"}
    assert all(isinstance(v, (int, float)) for v in on.values())          # the result dict stays scalar-only
    for k in bins:
        assert on[k] == bins[k], k
    assert (on["GCE"], on["GCE_groups"]) == (gwant["GCE"], gwant["GCE_groups"])
    assert saving_lines(out) == [line_off[0] + ", ECE = %.7g, PCOC = %.7g, NE = %.7g, GCE = %.7g"
                                 % (on["ECE"], on["PCOC"], on["NE"], on["GCE"])]
    live = np.flatnonzero(gtable[:, 0])
    assert np.array_equal(est.last_calibration["records"], np.concatenate([live.reshape(-1, 1), gtable[live]], axis=1))
    assert np.array_equal(est.last_calibration["table"], table)

    # the key alone, behind both AUC additions: the suffixes keep their order
    est.config.calibration_bins, est.config.exact_auc, est.config.group_auc_key = 0, True, key
    alone = est.evaluate(fn, steps=steps)
    assert set(alone) == set(off) | {"AUC_exact", "GAUC", "GAUC_groups", "GAUC_skipped_examples", "GCE", "GCE_groups"}
    assert alone["GCE"] == on["GCE"]
    assert saving_lines(capsys.readouterr().out) == [line_off[0] + ", AUC_exact = %.7g, GAUC = %.7g, GCE = %.7g"
                                                     % (alone["AUC_exact"], alone["GAUC"], alone["GCE"])]
    est.config.calibration_bins, est.config.exact_auc, est.config.group_auc_key = N, False, None

    # a NaN among the probabilities: nan figures and ONE warning with the count
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
    assert all(math.isnan(bad[k]) for k in ("ECE", "MCE", "PCOC", "NE", "GCE")) and bad["loss"] == off["loss"]
    assert len(warn) == 1 and warn[0].startswith("WARNING:calibration: %d of %d " % (steps, steps * B))
    assert est.last_calibration["invalid"] == steps and not math.isnan(est.last_calibration["ECE"])


def test_bad_settings_and_a_second_rank_are_refused_before_any_batch():
    est, fn, _, _ = criteo_estimator(32, 1)
    read = []

    def watched():
        read.append(1)
        yield from fn()
    est.config.calibration_key = "u_id"
    with pytest.raises(metrics.RsxError, match="_c14"):    # the message names the allowed keys
        est.evaluate(watched, steps=1)
    est.config.calibration_key = None
    for n_bins in (1, 1025, -3):
        est.config.calibration_bins = n_bins
        with pytest.raises(metrics.RsxError, match="n_bins"):
            est.evaluate(watched, steps=1)
    est.config.calibration_bins = 20

    class TwoRanks:
        world, rank = 2, 0
    est.store.dp = TwoRanks()
    try:
        with pytest.raises(metrics.RsxError, match="data-parallel evaluation is not supported"):
            est.evaluate(watched, steps=1)
    finally:
        est.store.dp = None
    assert read == []
    est.evaluate(watched, steps=1)
    assert read == [1]


def test_estimator_reports_the_calibration_of_din_categories(capsys, tmp_path):
    """din.py's own input pipeline (a TFRecord shard through din.input_fn) with calibration_key = i_cate."""
    from recsys_amd import din, synthetic
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.input_pipeline import write_din_shard
    B, steps, P, N = 64, 4, 10, 10
    b = synthetic.din_batch(np.random.default_rng(5), B * steps, P=P, n_item=500, n_cate=12)
    path = str(tmp_path / "valid2")
    write_din_shard(path, b)
    params = {"embedding_size": 16, "learning_rate": 1e-3, "dropout": 0.5, "max_batch_size": B, "hist_len": P,
              "n_item": 500, "n_cate": 12}

    def fn():
        return din.input_fn([path], B, 1, False, P)
    est = Estimator(din.model_fn, None, params, RunConfig(device="cuda", seed=3, log_step_count_steps=1000000))
    est.train(fn, steps=steps)
    capsys.readouterr()
    off = est.evaluate(fn, steps=steps)
    line_off = saving_lines(capsys.readouterr().out)
    est.config.calibration_bins, est.config.calibration_key = N, "i_cate"
    on = est.evaluate(fn, steps=steps)
    line = saving_lines(capsys.readouterr().out)
    assert set(on) == set(off) | {"ECE", "MCE", "PCOC", "NE", "GCE", "GCE_groups"} and all(on[k] == off[k] for k in off)
    prob = np.array([r["prob"] for r in est.predict(fn)], np.float32)
    labels, groups = b["label"].astype(np.float32), b["i_cate"]
    assert prob.shape == labels.shape
    table, invalid = metrics.calibration_bins_host(labels, prob, N)
    gtable, ginvalid = metrics.calibration_groups_host(groups, labels, prob, 13)      # 13 rows with the dummy
    assert invalid == 0 == ginvalid
    want = metrics.calibration_from_table(table, 0, loss=on["loss"])
    gwant = metrics.group_calibration_from_table(gtable, 0)
    assert gwant["GCE_groups"] >= 2
    assert (on["ECE"], on["MCE"], on["PCOC"], on["NE"]) == (want["ECE"], want["MCE"], want["PCOC"], want["NE"])
    assert on["NE"] == on["loss"] / entropy(int(table[:, 1].sum()) / int(table[:, 0].sum()))
    assert (on["GCE"], on["GCE_groups"]) == (gwant["GCE"], gwant["GCE_groups"])
    assert line == [line_off[0] + ", ECE = %.7g, PCOC = %.7g, NE = %.7g, GCE = %.7g" % (on["ECE"], on["PCOC"], on["NE"], on["GCE"])]
    est.config.calibration_key = "u_id"
    with pytest.raises(metrics.RsxError, match="i_id, i_cate"):
        est.evaluate(fn, steps=steps)
