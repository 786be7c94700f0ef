"""GAUC on the device (rsx_auc_group_append / _finalize / _records, csrc/auc_group.hip; metrics.GroupAUC;
RunConfig.group_auc_key) against metrics.group_auc_records_host, whose definition tests/test_group_auc_cpu.py holds to a pair
count.  Header words and records are compared as integers: no tolerance anywhere."""
import math

import numpy as np
import pytest
import torch

from recsys_amd import metrics
from recsys_amd._lib import lib

pytestmark = pytest.mark.gpu

INVALID = np.array([np.nan, np.inf, -np.inf, -1e-9, 1.0000001], np.float32)


def tile():
    return int(lib().rsx_auc_exact_tile())


def host(g, y, p, bits):
    """(header, records of the mixed groups) of the definition in numpy."""
    rec, invalid = metrics.group_auc_records_host(g, y, p, bits)
    mixed = (rec[:, 1] > 0) & (rec[:, 2] > 0)
    return metrics.group_auc_header_host(rec, invalid), rec[mixed]


def device(g, y, p, bits, batch=None, capacity=None):
    dev = torch.device("cuda")
    ga = metrics.GroupAUC(dev, bits, capacity)
    gd = torch.from_numpy(np.ascontiguousarray(g)).to(dev)
    yd, pd = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
    step = batch or max(1, len(p))
    for i in range(0, len(p), step):
        ga.update(gd[i:i + step], yd[i:i + step], pd[i:i + step])
    res = ga.result(per_group=True)
    return ga.header, res["records"], res


def check(g, y, p, bits, **kw):
    hdr, rec, res = device(g, y, p, bits, **kw)
    want_hdr, want_rec = host(g, y, p, bits)
    assert hdr == want_hdr
    assert rec.shape == want_rec.shape and np.array_equal(rec, want_rec)
    want = metrics.group_auc_host(g, y, p, bits)
    assert {k: v for k, v in res.items() if k != "records"}.keys() == want.keys()
    assert all(res[k] == want[k] or (k == "GAUC" and math.isnan(res[k]) and math.isnan(want[k])) for k in want)
    return hdr, rec, res


def labels_for(rng, p):
    return (rng.random(len(p)) < 0.2 + 0.6 * p).astype(np.float32)


def scores(rng, n, distinct=None):
    if distinct is None:
        return rng.random(n).astype(np.float32)
    return rng.random(distinct).astype(np.float32)[rng.integers(0, distinct, n)]


def sizes():
    T = tile()
    return [1, 63, 64, 65, T - 1, T, T + 1, 2 * T, 3 * T + 17]


@pytest.mark.parametrize("which", range(9))
@pytest.mark.parametrize("distinct", [None, 7])
def test_sizes_on_the_tile_edges(which, distinct):
    n = sizes()[which]
    rng = np.random.default_rng(23 * n + (distinct or 0))
    g = rng.integers(0, max(2, n // 40), n).astype(np.int32)            # ~40 examples per group: groups cross every tile edge
    p = scores(rng, n, distinct)
    hdr, _, _ = check(g, labels_for(rng, p), p, 10)
    assert hdr[0] == n


def from_runs(rng, runs, distinct=None):
    """A stream whose SORTED order has the given (group id, length) runs, fed shuffled."""
    g = np.concatenate([np.full(m, gid, np.int32) for gid, m in runs])
    p = scores(rng, g.size, distinct)
    y = labels_for(rng, p)
    perm = rng.permutation(g.size)
    return g[perm], y[perm], p[perm]


def test_group_boundary_exactly_on_a_tile_edge():
    T = tile()
    rng = np.random.default_rng(31)
    g, y, p = from_runs(rng, [(0, T - 100), (1, 100), (2, T), (3, 50)])   # boundaries at T - 100, T, 2 T
    check(g, y, p, 2)


@pytest.mark.parametrize("distinct", [None, 5])
def test_one_group_spans_three_tiles_between_small_groups(distinct):
    T = tile()
    rng = np.random.default_rng(32)
    runs = [(i, 9) for i in range(20)] + [(40, 3 * T + 11)] + [(50 + i, 7) for i in range(20)]
    g, y, p = from_runs(rng, runs, distinct)                           # distinct = 5: score ties that cross tile edges in one group
    _, rec, _ = check(g, y, p, 7)
    assert 40 in rec[:, 0].tolist()


def test_equal_scores_on_both_sides_of_a_group_boundary_are_no_tie():
    """All scores equal: inside a group every pair is a tie (U2_g == P_g N_g); across a boundary, on a tile edge or not, none."""
    T = tile()
    rng = np.random.default_rng(33)
    g, y, _ = from_runs(rng, [(3, T - 1), (4, 1), (5, T), (6, T // 2), (9, 5)])
    _, rec, res = check(g, y, np.full(g.size, 0.5, np.float32), 4)
    assert len(rec) >= 3 and np.array_equal(rec[:, 3], rec[:, 1] * rec[:, 2]) and res["GAUC"] == 0.5


@pytest.mark.parametrize("bits", [1, 8, 9, 19, 31])
def test_pass_counts_with_the_highest_id_present(bits):
    """4 + ceil(bits / 8) passes: 5, 5, 6, 7, 8 -- both parities; at 8 bits the top id's digit is the padding key's 0xFF."""
    rng = np.random.default_rng(bits)
    n = 2 * tile() + 77
    top = (1 << bits) - 1
    pool = np.unique(np.concatenate([[0, top, top - 1 if top > 1 else 0], rng.integers(0, top + 1, 60)])).astype(np.int64)
    g = pool[rng.integers(0, pool.size, n)]
    g[:5] = top
    p = scores(rng, n, 50)
    p[rng.choice(n, 9, replace=False)] = np.float32(np.nan)            # padding keys, to be sorted behind the top id
    y = labels_for(rng, np.nan_to_num(p))
    hdr, rec, _ = check(g.astype(np.int32), y, p, bits)
    assert hdr[1] == 9 and (bits == 1 or int(rec[-1, 0]) == top)


def test_more_tiles_than_workgroups():
    """Above 1024 tiles the launches' workgroups stride over the tiles and the one-workgroup tile scans carry from one round of
    1024 tiles into the next: the smallest size at which both happen.  One group is longer than the 1024-tile round."""
    n = 1024 * tile() + tile() + 5
    rng = np.random.default_rng(8)
    g = rng.integers(0, 3000, n).astype(np.int32)
    g[rng.random(n) < 0.3] = 1500
    p = scores(rng, n)
    p[rng.random(n) < 0.3] = np.float32(0.375)
    check(g, labels_for(rng, p), p, 12)


def test_one_group_equals_exact_auc():
    rng = np.random.default_rng(9)
    n = 2 * tile() + 100
    p = scores(rng, n, 300)
    y = labels_for(rng, p)
    hdr, rec, res = check(np.full(n, 77, np.int32), y, p, 7)
    dev = torch.device("cuda")
    ex = metrics.ExactAUC(dev)
    ex.update(torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev))
    e = ex.result()
    assert rec.tolist() == [[77, e["positives"], e["negatives"], e["u2"]]] and res["GAUC"] == e["AUC_exact"]
    assert hdr[2:5] == [1, 1, 0]


def test_only_one_class_groups():
    rng = np.random.default_rng(10)
    n = tile() + 300
    g = rng.integers(0, 64, n).astype(np.int32)
    hdr, rec, res = check(g, (g % 2).astype(np.float32), scores(rng, n), 6)
    assert len(rec) == 0 and math.isnan(res["GAUC"]) and hdr[3] == 0 and hdr[4] == n == res["skipped_examples"]


def test_invalid_probabilities_and_ids_at_random_positions():
    rng = np.random.default_rng(11)
    n = 2 * tile() + 100
    g = rng.integers(0, 200, n).astype(np.int32)
    p = scores(rng, n)
    at = rng.choice(n, 40 * INVALID.size + 60, replace=False)
    p[at[:40 * INVALID.size]] = np.tile(INVALID, 40)
    g[at[40 * INVALID.size:]] = np.tile(np.array([256, 257, -1, -2 ** 31, 2 ** 31 - 1, 1 << 20], np.int64), 10).astype(np.int32)
    y = labels_for(rng, np.nan_to_num(np.clip(p, 0, 1)))
    hdr, _, res = check(g, y, p, 8)
    assert hdr[1] == res["invalid"] == 40 * INVALID.size + 60
    assert math.isnan(metrics.group_auc_reported(res)) and not math.isnan(res["GAUC"])


def test_streaming_does_not_depend_on_batches_or_order(monkeypatch):
    rng = np.random.default_rng(12)
    n = 20000
    g = rng.integers(0, 500, n).astype(np.int32)
    p = scores(rng, n, 400)
    y = labels_for(rng, p)
    want_hdr, want_rec = host(g, y, p, 9)
    for batch in (1000, 4096):                             # 20 000 = 4 * 4096 + 3616: an uneven last batch
        hdr, rec, _ = device(g, y, p, 9, batch=batch, capacity=n)
        assert hdr == want_hdr and np.array_equal(rec, want_rec)
    perm = rng.permutation(n)
    hdr, rec, _ = device(g[perm], y[perm], p[perm], 9, batch=777, capacity=n)
    assert hdr == want_hdr and np.array_equal(rec, want_rec)
    dev = torch.device("cuda")
    monkeypatch.setattr(metrics.GroupAUC, "GROW_FROM", 1000)
    ga = metrics.GroupAUC(dev, 9)                          # a buffer that grows: 1000 -> 2000 -> ... -> 32000
    gd, yd, pd = (torch.from_numpy(a).to(dev) for a in (g, y, p))
    for i in range(0, n, 3000):
        ga.update(gd[i:i + 3000], yd[i:i + 3000], pd[i:i + 3000])
        if i == 9000:                                      # result() in mid-stream reorders the keys and keeps the multiset
            mid = ga.result(per_group=True)
            mid_hdr, mid_rec = host(g[:12000], y[:12000], p[:12000], 9)
            assert ga.header == mid_hdr and np.array_equal(mid["records"], mid_rec)
    assert ga.keys.numel() >= n
    for _ in range(2):                                     # and again, on keys that are already sorted
        res = ga.result(per_group=True)
        assert ga.header == want_hdr and np.array_equal(res["records"], want_rec)
    with pytest.raises(metrics.RsxError):
        device(g, y, p, 9, batch=4096, capacity=n - 1)


def test_numpy_inputs_empty_stream_and_strided_column():
    rng = np.random.default_rng(13)
    n, F, slot = 700, 5, 3
    ids = rng.integers(0, 30, (n, F)).astype(np.int32)
    p = scores(rng, n, 40)
    y = labels_for(rng, p)
    want_hdr, want_rec = host(ids[:, slot], y, p, 5)
    ga = metrics.GroupAUC("cuda", 5)
    res = ga.result(per_group=True)
    assert ga.header == [0] * 8 and math.isnan(res["GAUC"]) and res["records"].shape == (0, 4)
    ga.update(ids[:, slot].astype(np.int64).reshape(-1, 1), y.reshape(-1, 1), p.reshape(-1, 1))   # numpy, int64, [B, 1]
    res = ga.result(per_group=True)
    assert ga.header == want_hdr and np.array_equal(res["records"], want_rec)
    dev = torch.device("cuda")
    ids_d = torch.from_numpy(ids).to(dev)
    col = ids_d[:, slot]
    assert col.stride(0) == F and not col.is_contiguous()
    gb = metrics.GroupAUC(dev, 5)
    tensor, stride = metrics.group_column_on_device(col, dev)
    assert stride == F and tensor.data_ptr() == col.data_ptr()         # the view itself is what the launch reads
    gb.update(col, torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev))
    res = gb.result(per_group=True)
    assert gb.header == want_hdr and np.array_equal(res["records"], want_rec)


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


def test_estimator_reports_gauc_for_a_criteo_column(capsys):
    B, steps = 64, 5
    est, fn, host_batches, layout = criteo_estimator(B, steps)
    key = "_c30"                                           # 10 buckets: the groups hold both classes
    slot = [c.key for c in layout.columns].index(key)
    assert layout.columns[slot].rows == 10
    est.train(fn, steps=steps)
    capsys.readouterr()
    off = est.evaluate(fn, steps=steps)
    line_off = saving_lines(capsys.readouterr().out)
    assert set(off) == {"AUC", "Accuracy", "loss", "global_step"} and len(line_off) == 1 and "GAUC" not in line_off[0]
    est.config.group_auc_key = key
    on = est.evaluate(fn, steps=steps)
    out_on = capsys.readouterr().out
    assert set(on) == set(off) | {"GAUC", "GAUC_groups", "GAUC_skipped_examples"}
    for k in off:                                          # the other keys: bit for bit what the key-off evaluate gives
        assert on[k] == off[k], k
    assert saving_lines(out_on) == [line_off[0] + ", GAUC = %.7g" % on["GAUC"]]
    assert not any(ln.startswith("WARNING:") for ln in out_on.splitlines())
    prob = np.array([r["prob"] for r in est.predict(fn)], np.float32)
    labels = np.concatenate([y.reshape(-1) for _, y, _ in host_batches]).astype(np.float32)
    groups = np.concatenate([i[:, slot] for i, _, _ in host_batches])
    want = metrics.group_auc_host(groups, labels, prob, 4)
    assert want["invalid"] == 0 and want["mixed_groups"] >= 2
    assert on["GAUC"] == want["GAUC"] and on["GAUC_groups"] == want["mixed_groups"]
    assert on["GAUC_skipped_examples"] == want["skipped_examples"]
    # both opt-in metrics at once: independent objects, each its own number
    est.config.exact_auc = True
    both = est.evaluate(fn, steps=steps)
    assert both["GAUC"] == on["GAUC"] and both["AUC_exact"] == metrics.exact_auc_host(labels, prob)["AUC_exact"]
    assert saving_lines(capsys.readouterr().out)[0].endswith(", AUC_exact = %.7g, GAUC = %.7g" % (both["AUC_exact"], both["GAUC"]))
    est.config.exact_auc = False

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
    assert math.isnan(bad["GAUC"]) and len(warn) == 1 and ("%d examples" % steps) in warn[0]


def test_unknown_key_and_second_rank_are_refused_before_any_batch():
    est, fn, _, _ = criteo_estimator(32, 1)
    read = []

    def watched():
        read.append(1)
        yield from fn()
    est.config.group_auc_key = "u_id"
    with pytest.raises(metrics.RsxError, match="_c14"):    # the message names the allowed keys
        est.evaluate(watched, steps=1)
    est.config.group_auc_key = "_c14"

    class TwoRanks:
        world, rank = 2, 0
    est.store.dp = TwoRanks()
    try:
        with pytest.raises(metrics.RsxError, match="data-parallel evaluation is not supported"):
            est.evaluate(watched, steps=1)
    finally:
        est.store.dp = None
    assert read == []


def test_estimator_reports_gauc_for_din_categories(capsys, tmp_path):
    """din.py's own input pipeline (a TFRecord shard through din.input_fn) with group_auc_key = i_cate."""
    from recsys_amd import din, synthetic
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.input_pipeline import write_din_shard
    B, steps, P = 64, 4, 10
    b = synthetic.din_batch(np.random.default_rng(5), B * steps, P=P, n_item=500, n_cate=12)
    path = str(tmp_path / "valid2")
    write_din_shard(path, b)
    params = {"embedding_size": 16, "learning_rate": 1e-3, "dropout": 0.5, "max_batch_size": B, "hist_len": P,
              "n_item": 500, "n_cate": 12}

    def fn():
        return din.input_fn([path], B, 1, False, P)
    est = Estimator(din.model_fn, None, params, RunConfig(device="cuda", seed=3, log_step_count_steps=1000000,
                                                          group_auc_key="i_cate"))
    est.train(fn, steps=steps)
    capsys.readouterr()
    on = est.evaluate(fn, steps=steps)
    line = saving_lines(capsys.readouterr().out)
    prob = np.array([r["prob"] for r in est.predict(fn)], np.float32)
    labels, groups = b["label"].astype(np.float32), b["i_cate"]
    assert prob.shape == labels.shape
    want = metrics.group_auc_host(groups, labels, prob, 4)              # 13 rows with the dummy: 4 bits
    assert want["invalid"] == 0 and want["mixed_groups"] >= 2
    assert on["GAUC"] == want["GAUC"] and on["GAUC_groups"] == want["mixed_groups"]
    assert len(line) == 1 and line[0].endswith(", GAUC = %.7g" % on["GAUC"])
    est.config.group_auc_key = "u_id"
    with pytest.raises(metrics.RsxError, match="i_id, i_cate"):
        est.evaluate(fn, steps=steps)
