"""Time per serving request of an exported deepfm.py model (Criteo-39, d = 16, DNN 100-100) on the two paths that can answer
it, in ONE process, their timed regions alternating, `--repeats` rounds per request size; medians and the spread are reported.

  A  the parent path: Estimator._infer_step(PREDICT) with HIP graphs on (what Estimator.predict_examples does): the captured
     graph of gather + two tower-forward launches + head.
  B  serving.Predictor, fused path: the captured graph of ONE rsx_predict_fm_tower launch (csrc/predict.hip).

    python scripts/bench_serving.py [--sizes 1,16,200,256,4096] [--replays 3000] [--repeats 3]
        device time per request: hipEvents around `--replays` graph replays over resident request batches, after every
        size of both contenders has been warmed up and captured; then predict_examples end to end at --e2e_rows rows from
        serialized Examples (host parse + H2D + launch + D2H), wall clock around a synchronise.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/bench_serving.py --profile-run 200
        eager requests of both paths for a kernel trace of its own (kernel names in the trace; no timing printed);
    python scripts/bench_serving.py --kernel-stats DIR/.../NAME_kernel_stats.csv --profile-run 200
        kernel time of predict_fm_tower_k against the sum of A's four kernels per request, and the kernel's achieved rates.

    python scripts/bench_serving.py --layer-probe
        where the kernel's time goes: rsx_predict_fm_tower through the C ABI on random weights with 0 to 3 layers of several
        widths, 20 launches back to back per graph replay, device time per launch at 16 and 4096 rows.

    python scripts/bench_serving.py --model dcn [the same options]
        the dcn.py leg (Criteo-39, d = 16, DNN 100-100, 3 cross layers), both contenders loaded from ONE exported bundle:
        A  serving.Predictor as it loads by default: the layers path, HIP graphs on (the rebuilt Estimator's captured graph
           of gather + cross forward + two tower-forward launches + head);
        B  serving.Predictor.load(..., one_launch=True): the captured graph of ONE rsx_predict_dcn launch
           (csrc/predict_dcn.hip).

    python scripts/bench_serving.py --table_dtype bfloat16|float16 [--model dcn] [the same options]
        16-bit embedding tables (--export_table_dtype): ONE model exported twice,
        A  the float32 bundle on the fused path (dcn: one_launch=True),
        B  the same model exported with the 16-bit dtype, its table on the device in 16 bits;
        device time per request over graph replays as above, torch.cuda.memory_allocated after each load, and max / mean
        |prob_B - prob_A| on each request batch (an UNTRAINED, randomly initialised model: not an accuracy figure).
        With --profile-run / --kernel-stats: the kernel-trace time of every instantiation of the kernel; a request reads
        B x 39 x 32 B of 16-bit rows (64 B of fp32 rows) + the dense weights once.

    python scripts/bench_serving.py --device_parse [--parse_sizes 1,16,200,4096] [--e2e_calls 300] [--repeats 3]
        `predict_examples` end to end (wall clock, host to host, around a synchronise) of ONE exported deepfm.py bundle,
        A  serving.Predictor as it loads by default: the request parsed on the host (rsx_criteo_parse_h), ids shipped, one launch;
        B  serving.Predictor.load(..., device_parse=True): the request's bytes shipped, rsx_criteo_parse_examples + the predict
           launch in one graph (csrc/parse_examples.hip),
        alternating within every repeat at every request size, with the method of the predict_examples_rows line; the
        probabilities must be equal bit for bit.  Then a one-off split of A at 200 rows: the host parse alone, and everything
        else (predict() on the parsed ids).

Roofline terms (named for what they are): bytes the request needs = B x 39 rows x 64 B + the dense weights once; FLOPs =
2 x B x (624 x 100 + 100 x 100 + 100) (dcn: 2 x B x (624 x 100 + 100 x 100 + 100 + 624) + 3 x B x 5 x 624 for the cross
layers); over the kernel time.  At these sizes the kernel is latency-bound: the figure to watch is time per request."""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A_KERNELS = ("gather_fm", "tower_fwd", "tower_head")        # the four launches of Estimator deepfm inference
B_KERNEL = "predict_fm_tower_k"
A_KERNELS_DCN = ("gather_fm", "cross_fwd", "tower_fwd", "tower_head")   # the launches of Estimator dcn inference
B_KERNEL_DCN = "predict_dcn_k"
DCN_CROSS_LAYERS = 3


def build(dev, max_batch, export_dir):
    """-> (Estimator with HIP graphs on, Predictor on the fused path, layout) over the same variables."""
    import torch
    from recsys_amd import deepfm, serving
    from recsys_amd.estimator import Estimator, ModeKeys, RunConfig
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    lin, emb = build_feature_columns(16, "indicator_all")
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
              "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": max_batch}
    est = Estimator(deepfm.model_fn, None, params, RunConfig(device=str(dev), seed=1234, use_hip_graph=True))
    layout = CriteoLayout.from_columns(emb)
    with torch.no_grad():
        est._call_model_fn({"ids": torch.zeros(1, layout.F, dtype=torch.int32, device=dev)}, None, ModeKeys.PREDICT)
        g = torch.Generator(device="cpu").manual_seed(7)          # a served model is a trained one: no all-zero biases
        for k, p in est.store.dense.params.items():
            if k.split(".")[-1][0] in "bg":
                p.add_((torch.rand(p.shape, generator=g) * 0.2 - 0.1).to(dev))
    pred = serving.Predictor.load(est.export_savedmodel(export_dir), device=str(dev), max_batch_size=max_batch)
    assert pred.path == "fused", pred.path
    torch.cuda.synchronize()
    return est, pred, layout


class LayersContender:
    """The layers-path Predictor in the place of the Estimator of the deepfm leg: the calls the timing code makes."""

    def __init__(self, pred):
        self.pred, self.config = pred, pred._est.config
        self._graphs = pred._est._graphs

    def _infer_step(self, features, labels, mode):
        return self.pred._est._infer_step(features, labels, mode)

    def _call_model_fn(self, features, labels, mode):
        return self.pred._est._call_model_fn(features, labels, mode)

    def predict_examples(self, serialized):
        return self.pred.predict_examples(serialized)


def build_dcn(dev, max_batch, export_dir):
    """-> (the default Predictor of a dcn.py bundle = layers path with HIP graphs on, the one_launch Predictor, layout)."""
    import torch
    from recsys_amd import dcn, serving
    from recsys_amd.estimator import Estimator, ModeKeys, RunConfig
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    lin, emb = build_feature_columns(16, "numeric")
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
              "dropout": 0.5, "deep_layers": "100,100", "cross_layers": DCN_CROSS_LAYERS, "max_batch_size": 64}
    est = Estimator(dcn.model_fn, None, params, RunConfig(device=str(dev), seed=1234, use_hip_graph=False))
    layout = CriteoLayout.from_columns(emb)
    with torch.no_grad():
        est._call_model_fn({"ids": torch.zeros(1, layout.F, dtype=torch.int32, device=dev)}, None, ModeKeys.PREDICT)
        g = torch.Generator(device="cpu").manual_seed(7)          # a served model is a trained one: no all-zero biases
        for k, p in est.store.dense.params.items():
            if k.startswith("dnn.") and k.split(".")[-1][0] in "bg" or k == "out.b":
                p.add_((torch.rand(p.shape, generator=g) * 0.2 - 0.1).to(dev))
    d = est.export_savedmodel(export_dir)
    del est
    pa = serving.Predictor.load(d, device=str(dev), max_batch_size=max_batch)
    pb = serving.Predictor.load(d, device=str(dev), max_batch_size=max_batch, one_launch=True)
    assert pa.path == "layers" and pb.path == "fused", (pa.path, pb.path)
    torch.cuda.synchronize()
    return LayersContender(pa), pb, layout


def build_table_dtype(dev, max_batch, export_dir, model, dtype):
    """-> (Predictor of the float32 bundle, Predictor of the `dtype` bundle of the same model, layout, device bytes of each
    load): both on the fused path."""
    import torch
    from recsys_amd import dcn, deepfm, serving
    from recsys_amd.estimator import Estimator, ModeKeys, RunConfig
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    lin, emb = build_feature_columns(16, "numeric" if model == "dcn" else "indicator_all")
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
              "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": 64}
    if model == "dcn":
        params["cross_layers"] = DCN_CROSS_LAYERS
    est = Estimator((dcn if model == "dcn" else deepfm).model_fn, None, params,
                    RunConfig(device=str(dev), seed=1234, use_hip_graph=False))
    layout = CriteoLayout.from_columns(emb)
    with torch.no_grad():
        est._call_model_fn({"ids": torch.zeros(1, layout.F, dtype=torch.int32, device=dev)}, None, ModeKeys.PREDICT)
        g = torch.Generator(device="cpu").manual_seed(7)          # a served model is a trained one: no all-zero biases
        for k, p in est.store.dense.params.items():
            if k.split(".")[-1][0] in "bg":
                p.add_((torch.rand(p.shape, generator=g) * 0.2 - 0.1).to(dev))
    da = est.export_savedmodel(os.path.join(export_dir, "float32"))
    db = est.export_savedmodel(os.path.join(export_dir, dtype), table_dtype=dtype)
    del est
    kw = {"one_launch": True} if model == "dcn" else {}
    preds, mem = [], []
    for d in (da, db):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        preds.append(serving.Predictor.load(d, device=str(dev), max_batch_size=max_batch, **kw))
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated() - before)
        assert preds[-1].path == "fused", preds[-1].path
    assert preds[0].table_dtype == "float32" and preds[1].table_dtype == dtype
    return preds[0], preds[1], layout, mem


def capture_predictors(pa, pb, ids):
    """Warm up and capture the request size on both Predictors -> (A's graph, B's graph, max and mean |prob_B - prob_A|)."""
    for _ in range(3):                           # eager warm-up, capture + replay, replay
        a, b = pa.predict({"ids": ids})["prob"], pb.predict({"ids": ids})["prob"]
    B = ids.shape[0]
    assert "graph" in pa._graphs[B] and "graph" in pb._graphs[B]
    d = np.abs(b.astype(np.float64) - a.astype(np.float64))
    return pa._graphs[B]["graph"], pb._graphs[B]["graph"], float(d.max()), float(d.mean())


def table_dtype_stats(a, b_kernel, dense_floats):
    """--kernel-stats of a --table_dtype --profile-run trace: every instantiation of the kernel (its last template argument
    is the table dtype: 0 float32, 1 bfloat16, 2 float16) with the bytes a request needs over its time."""
    import re
    out = []
    for name, (calls, _, avg) in sorted(kernel_stats(a.kernel_stats).items()):
        m = re.search(b_kernel + r"<([\d, ]+)>", name)
        if not m:
            continue
        td = int(m.group(1).split(",")[-1])
        nbytes = a.profile_run * 39 * (64 if td == 0 else 32) + 4 * dense_floats
        rec = {"model": a.model, "kernel": b_kernel + "<" + m.group(1) + ">", "table_dtype": ("float32", "bfloat16", "float16")[td],
               "batch_size": a.profile_run, "calls": calls, "kernel_us_per_request": round(avg / 1e3, 3), "request_bytes": nbytes,
               "achieved_GBps": round(nbytes / avg, 1)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def run_table_dtype(a, dev, sizes):
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        pa, pb, layout, mem = build_table_dtype(dev, max(sizes), tmp, a.model, a.table_dtype)
    if a.profile_run:
        pa.use_hip_graph = pb.use_hip_graph = False                 # eager: every launch appears in the trace under its name
        ids = torch.from_numpy(request_ids(layout, a.profile_run, 11)).to(dev)
        for pr in (pa, pb):
            for _ in range(a.profile_requests):
                pr.predict({"ids": ids})
        torch.cuda.synchronize()
        return None
    out = [{"model": a.model, "A_table_dtype": "float32", "B_table_dtype": a.table_dtype,
            "A_load_device_bytes": mem[0], "B_load_device_bytes": mem[1], "A_table_bytes": pa._tables.numel() * pa._tables.element_size(),
            "B_table_bytes": pb._tables.numel() * pb._tables.element_size(),
            "note": "prob_diff figures: an UNTRAINED, randomly initialised model -- what rounding the tables does to its "
                    "probabilities, not an accuracy figure of a trained one"}]
    print(json.dumps(out[0]), flush=True)
    graphs = {B: capture_predictors(pa, pb, request_ids(layout, B, 100 + B)) for B in sizes}     # every size, before any timing
    for B in sizes:
        ga, gb, dmax, dmean = graphs[B]
        for g in (ga, gb):
            time_replays(g, 200)
        ta, tb = [], []
        for _ in range(a.repeats):                 # the contenders alternate within every round
            ta.append(time_replays(ga, a.replays))
            tb.append(time_replays(gb, a.replays))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        rec = {"model": a.model, "table_dtype": a.table_dtype, "batch_size": B, "A_float32_us": round(ma, 3), "B_16bit_us": round(mb, 3),
               "B_minus_A_us": round(mb - ma, 3), "A_repeats_us": [round(x, 3) for x in ta], "B_repeats_us": [round(x, 3) for x in tb],
               "A_spread_us": round(max(ta) - min(ta), 3), "B_spread_us": round(max(tb) - min(tb), 3),
               "max_abs_prob_diff": dmax, "mean_abs_prob_diff": dmean}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def run_device_parse(a, dev):
    import torch
    from recsys_amd import serving
    sizes = [int(x) for x in a.parse_sizes.split(",")]
    with tempfile.TemporaryDirectory() as tmp:
        est, host, layout = build(dev, max(sizes), os.path.join(tmp, "export"))
        del est
        devp = serving.Predictor.load(host.bundle_dir, device=str(dev), max_batch_size=max(sizes), device_parse=True)
    assert host.parse_path == "host" and devp.parse_path == "device"

    def wall(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()                                   # (ends in a device-to-host copy: synchronises)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e6

    out = []
    for n in sizes:
        reqs = serialized_requests(n)
        for _ in range(3):                         # eager warm-up, capture + replay, replay
            pa, pb = host.predict_examples(reqs)["prob"], devp.predict_examples(reqs)["prob"]
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), n
        calls = max(20, min(a.e2e_calls, 100000 // n))
        ta, tb = [], []
        for _ in range(a.repeats):                 # the contenders alternate within every repeat
            ta.append(wall(lambda: host.predict_examples(reqs), calls))
            tb.append(wall(lambda: devp.predict_examples(reqs), calls))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        rec = {"predict_examples_rows": n, "request_bytes": sum(map(len, reqs)), "calls": calls, "A_host_parse_us": round(ma, 1),
               "B_device_parse_us": round(mb, 1), "B_over_A": round(mb / ma, 4), "A_repeats_us": [round(x, 1) for x in ta],
               "B_repeats_us": [round(x, 1) for x in tb], "A_spread_us": round(max(ta) - min(ta), 1),
               "B_spread_us": round(max(tb) - min(tb), 1), "bit_identical": True}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    reqs = serialized_requests(200)                # the split of the host path: the parse alone, and everything else
    feats = host._parse(reqs)
    host.predict(feats)
    tp, tr, tt = [], [], []
    for _ in range(a.repeats):
        tp.append(wall(lambda: host._parse(reqs), a.e2e_calls))
        tr.append(wall(lambda: host.predict(feats), a.e2e_calls))
        tt.append(wall(lambda: host.predict_examples(reqs), a.e2e_calls))
    rec = {"host_path_split_rows": 200, "parse_alone_us": round(float(np.median(tp)), 1),
           "everything_else_us": round(float(np.median(tr)), 1), "predict_examples_us": round(float(np.median(tt)), 1),
           "parse_repeats_us": [round(x, 1) for x in tp], "else_repeats_us": [round(x, 1) for x in tr],
           "total_repeats_us": [round(x, 1) for x in tt]}
    out.append(rec)
    print(json.dumps(rec), flush=True)
    return out


def request_ids(layout, B, seed):
    from recsys_amd import synthetic
    return synthetic.criteo_id_batches(layout, 1, B, seed=seed)[0][0]


def capture_both(est, pred, ids):
    """Warm up and capture the request size on both paths -> (A's graph, B's graph); both hold `ids` in their static inputs."""
    import torch
    from recsys_amd.estimator import ModeKeys
    B = ids.shape[0]
    with torch.no_grad():
        for _ in range(3):                       # eager warm-up, capture + replay, replay
            pa = est._infer_step({"ids": ids}, None, ModeKeys.PREDICT)[0].reshape(-1).float().cpu().numpy()
            pb = pred.predict({"ids": ids})["prob"]
    err = float(np.abs(pa - pb).max())
    assert err <= 2e-5, (B, err)                 # (faster and different is not faster)
    ga = [g for k, g in est._graphs.items() if k[0] == "infer" and g.graph is not None and g.static.views()[0]["ids"].shape[0] == B]
    assert len(ga) == 1 and "graph" in pred._graphs[B]
    return ga[0].graph, pred._graphs[B]["graph"], err


def time_replays(graph, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per request


def serialized_requests(n, seed=5):
    """n serialized tf.train.Examples as a client sends them (deepfm/grpc_client.py:50-76)."""
    from oracle import tfrecord
    from recsys_amd import synthetic
    from recsys_amd.input_pipeline import write_criteo_shard
    label, cont, cat = synthetic.criteo_raw_batch(np.random.default_rng(seed), n)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "requests")
        write_criteo_shard(path, label, cont, cat)
        return list(tfrecord.unframe(open(path, "rb").read()))


def algorithmic(B, dense_floats, model="deepfm"):
    flops = 2 * B * (624 * 100 + 100 * 100 + 100)
    if model == "dcn":          # + the head's cross part, + per cross layer a 624-long dot (2) and s * x0 + x + b (3) per element
        flops += 2 * B * 624 + DCN_CROSS_LAYERS * B * 5 * 624
    return {"bytes": B * 39 * 64 + 4 * dense_floats, "flops": flops}


def kernel_stats(path):
    rows = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            rows[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]), float(row["AverageNs"]))
    return rows


def layer_probe():
    """Device time per rsx_predict_fm_tower launch by number and width of layers (Criteo-39 shapes, random weights)."""
    import ctypes as C
    import torch
    from recsys_amd import _lib
    L = _lib.lib()
    F, R, dev = 39, 1086810, "cuda"
    g = torch.Generator().manual_seed(0)
    tables, w1 = (torch.randn(R, 16, generator=g) * 0.25).to(dev), torch.randn(R, generator=g).to(dev)
    row_off = (torch.arange(F, dtype=torch.int32) * (R // F)).to(dev)
    rnd = lambda *shape: (torch.randn(*shape, generator=g) * 0.05).to(dev)
    out = []
    for layers in ((), (100,), (100, 100), (100, 100, 100), (64,), (128,), (256,)):
        m, keep, K = _lib.PredictModel(), [], F * 16
        m.tables, m.w1, m.row_off = tables.data_ptr(), w1.data_ptr(), row_off.data_ptr()
        for l, n in enumerate(layers):
            ts = [rnd(K, n), rnd(n), rnd(n), rnd(n)]
            keep += ts
            m.W[l], m.b[l], m.gamma[l], m.beta[l] = [t.data_ptr() for t in ts]
            m.widths[l], K = n, n
        ts = [rnd(max(K, 4)), rnd(1), rnd(1), rnd(3), rnd(1)]
        keep += ts
        m.wd, m.bd, m.c0, m.wo, m.bo = [t.data_ptr() for t in ts]
        m.w1_field_mask, m.bn_eps, m.F, m.D, m.L = (1 << F) - 1, 1e-3, F, 16, len(layers)
        for B in (16, 4096):
            ids = torch.randint(0, R // F, (B, F), generator=g, dtype=torch.int32).to(dev)
            prob = torch.empty(B, device=dev)
            launch = lambda: _lib.check(L.rsx_predict_fm_tower(C.byref(m), ids.data_ptr(), prob.data_ptr(), B,
                                                               torch.cuda.current_stream().cuda_stream), "rsx_predict_fm_tower")
            for _ in range(3):
                launch()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(20):
                    launch()
            time_replays(graph, 20)
            rec = {"layer_probe": list(layers), "batch_size": B, "us_per_launch": round(time_replays(graph, 200) / 20, 2)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--layer-probe", dest="layer_probe", action="store_true")
    p.add_argument("--model", choices=("deepfm", "dcn"), default="deepfm")
    p.add_argument("--sizes", default="1,16,200,256,4096")
    p.add_argument("--replays", type=int, default=3000)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--e2e_rows", type=int, default=200)
    p.add_argument("--e2e_calls", type=int, default=300)
    p.add_argument("--profile-run", dest="profile_run", type=int, default=0, help="request size of a rocprofv3 run")
    p.add_argument("--profile-requests", dest="profile_requests", type=int, default=200)
    p.add_argument("--kernel-stats", dest="kernel_stats", default=None)
    p.add_argument("--table_dtype", choices=("bfloat16", "float16"), default=None,
                   help="A = the float32 bundle, B = the same model exported with this table dtype, both on the fused path")
    p.add_argument("--device_parse", action="store_true",
                   help="predict_examples end to end: A = the host parse, B = Predictor.load(..., device_parse=True)")
    p.add_argument("--parse_sizes", default="1,16,200,4096")
    a = p.parse_args()
    dense_floats = 624 * 100 + 100 * 100 + 6 * 100 + 100 + 1 + 3 + 1 + 1
    a_kernels, b_kernel = A_KERNELS, B_KERNEL
    if a.model == "dcn":
        dense_floats = 624 * 100 + 100 * 100 + 6 * 100 + 2 * DCN_CROSS_LAYERS * 624 + 100 + 624 + 1
        a_kernels, b_kernel = A_KERNELS_DCN, B_KERNEL_DCN
    if a.kernel_stats and a.table_dtype:
        return table_dtype_stats(a, b_kernel, dense_floats)
    if a.kernel_stats:                            # no GPU needed: the trace's own numbers
        B, n = a.profile_run, a.profile_requests
        st = kernel_stats(a.kernel_stats)
        a_ns = sum(t for name, (c, t, _) in st.items() if any(k in name for k in a_kernels))
        a_calls = sum(c for name, (c, t, _) in st.items() if any(k in name for k in a_kernels))
        b = [(c, t, avg) for name, (c, t, avg) in st.items() if b_kernel in name]
        alg = algorithmic(B, dense_floats, a.model)
        rec = {"model": a.model, "batch_size": B, "A_kernels_per_request": round(a_calls / n, 2), "A_kernel_us_per_request": round(a_ns / n / 1e3, 3),
               "B_kernel_us_per_request": round(b[0][2] / 1e3, 3), "B_calls": b[0][0], "request_bytes": alg["bytes"],
               "request_flops": alg["flops"], "B_achieved_GBps": round(alg["bytes"] / b[0][2], 1),
               "B_achieved_GFLOPs": round(alg["flops"] / b[0][2], 1)}
        print(json.dumps(rec), flush=True)
        return rec
    from recsys_amd import build as _b
    _b.build(verbose=False)
    if a.layer_probe:
        return layer_probe()
    dev = torch.device("cuda")
    sizes = [int(s) for s in a.sizes.split(",")] if not a.profile_run else [a.profile_run]
    if a.table_dtype:
        return run_table_dtype(a, dev, sizes)
    if a.device_parse:
        return run_device_parse(a, dev)
    with tempfile.TemporaryDirectory() as tmp:
        est, pred, layout = (build_dcn if a.model == "dcn" else build)(dev, max(sizes + [a.e2e_rows]), os.path.join(tmp, "export"))
    if a.profile_run:
        from recsys_amd.estimator import ModeKeys
        est.config.use_hip_graph = pred.use_hip_graph = False       # eager: every launch appears in the trace under its name
        ids = torch.from_numpy(request_ids(layout, a.profile_run, 11)).to(dev)
        with torch.no_grad():
            for _ in range(a.profile_requests):
                est._call_model_fn({"ids": ids}, None, ModeKeys.PREDICT)
            for _ in range(a.profile_requests):
                pred.predict({"ids": ids})
        torch.cuda.synchronize()
        return None
    out = []
    graphs = {B: capture_both(est, pred, request_ids(layout, B, 100 + B)) for B in sizes}     # every size, before any timing
    for B in sizes:
        ga, gb, err = graphs[B]
        for g in (ga, gb):
            time_replays(g, 200)
        ta, tb = [], []
        for _ in range(a.repeats):                 # the contenders alternate within every round
            ta.append(time_replays(ga, a.replays))
            tb.append(time_replays(gb, a.replays))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        alg = algorithmic(B, dense_floats, a.model)
        rec = {"model": a.model, "batch_size": B, "A_estimator_us": round(ma, 3), "B_predictor_us": round(mb, 3), "B_over_A": round(mb / ma, 4),
               "A_repeats_us": [round(x, 3) for x in ta], "B_repeats_us": [round(x, 3) for x in tb],
               "A_spread": round((max(ta) - min(ta)) / ma, 4), "B_spread": round((max(tb) - min(tb)) / mb, 4),
               "max_abs_prob_diff": err, "request_bytes": alg["bytes"], "request_flops": alg["flops"]}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    if a.e2e_rows:
        reqs = serialized_requests(a.e2e_rows)
        for _ in range(3):
            pa = est.predict_examples(reqs)["prob"]
            pb = pred.predict_examples(reqs)["prob"]
        assert float(np.abs(pa - pb).max()) <= 2e-5
        ta, tb = [], []
        for _ in range(a.repeats):
            for fn, dst in ((est.predict_examples, ta), (pred.predict_examples, tb)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.e2e_calls):
                    fn(reqs)                       # (ends in a device-to-host copy of prob: synchronises)
                torch.cuda.synchronize()
                dst.append((time.perf_counter() - t0) / a.e2e_calls * 1e6)
        rec = {"model": a.model, "predict_examples_rows": a.e2e_rows, "A_estimator_us": round(float(np.median(ta)), 1),
               "B_predictor_us": round(float(np.median(tb)), 1), "A_repeats_us": [round(x, 1) for x in ta],
               "B_repeats_us": [round(x, 1) for x in tb]}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


if __name__ == "__main__":
    main()
