"""Time per candidate-ranking request of an exported din.py model at the reference's sizes (K = 32, hist_len = 100, 63 002
items, 802 categories, histories of synthetic.din_batch): ONE user history against C candidates, on the two ways the package
can answer it, in ONE process, their timed regions alternating, `--repeats` rounds per C; medians and the spread are reported.

  A  what a caller had before `rank_candidates`: serving.expand_rank_request on the host (the history copied C times) and
     Predictor.predict on the `layers` path with HIP graphs on -- five row lookups, attention and pooling forward twice
     each, the concat, three tower-forward launches and the head, captured as one graph per request size.
  B  Predictor.rank_candidates: the captured graph of ONE rsx_predict_din_rank launch (csrc/predict_din.hip).

    python scripts/bench_serving_din.py [--sizes 1,16,200,1000,4096] [--replays 2000] [--repeats 3]
        device time per request: hipEvents around graph replays over resident inputs (every C of both contenders warmed up
        and captured before any timing; the replay count is cut for the slow sizes so that a timed region stays ~0.5 s);
        wall time per request: host arrays in, host probabilities out (A: expansion + copies + graph; B: copies + graph),
        around a synchronise.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/bench_serving_din.py --profile-run 200
        eager requests of both paths for a kernel trace of its own (no timing printed);
    python scripts/bench_serving_din.py --kernel-stats DIR/.../NAME_kernel_stats.csv --profile-run 200
        the kernel's time against the sum of A's kernels per request (every other kernel the trace holds at least once per
        request, the runtime's buffer copies left out), and its achieved FLOP/s against the fp32 MFMA peak.

  --top_k K  the request that ends in the K best candidates, C = 200 / 4096 / 63001 (the whole catalogue, 16 chunks at the default
     max_candidates of 4096) unless --sizes says otherwise, the same protocol (one process, the contenders alternating,
     medians and spread of --repeats rounds):
       A  rank_candidates(...)["prob"] (a blocking copy of every chunk's probabilities), then the fastest host selection with
          the order of serving.topk_rows_host: np.partition for the K-th value, a stable sort of the survivors;
       B  rank_candidates(..., top_k=K): rsx_topk_rows (csrc/topk.hip) behind every chunk's rank launch, one copy of K pairs.
     wall time host to host; device time = hipEvents around replays of the request's captured chunk graphs (B: with the
     state's zeroing in front) over the static buffers as one request of that size left them: the request's own history, the
     candidates of its last chunk.  With --profile-run C: eager B requests for a kernel trace of its own, and --kernel-stats
     prints the selection launch's time next to the rank launch's.

  --recommend  the request `recommend` was built for: the K best (--top_k, default 100) items of the whole 63 001-item catalogue
     that the user has not seen, U = 1 and U = 16 users, the same protocol:
       A  rank_candidates(history, catalogue, top_k=K + valid history length) with the catalogue passed from the host, then the
          seen items dropped and the rest cut to K in numpy;
       B  set_catalogue once, then recommend(history, K): rsx_predict_din_rank_shared over the resident catalogue and
          rsx_topk_rows_excl (csrc/topk_excl.hip), the whole request ONE captured graph, one copy back.
     Both must return the same items (asserted).  Device time = hipEvents around replays (A: the state's zeroing and the 16 chunk
     graphs; B: its one graph); wall time = host arrays in, host result out.

FLOPs of a request, from shapes: 2 x C x valid positions x (K x 80 + 80 x 40 + 40) per attention (the folded first layer), both
attentions; the user-side and candidate-side terms and the tower are not counted."""
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

B_KERNEL = "predict_din_rank_k"
K, P = 32, 100
PEAK_F32_MFMA = 157.3e12                         # 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz (v_mfma_f32_16x16x4_f32)


def build(dev, max_c, export_dir):
    """-> Predictor of a din.py bundle at the reference's sizes (both contenders answer from its variables)."""
    import torch
    from recsys_amd import din, serving
    from recsys_amd.estimator import Estimator, ModeKeys, RunConfig
    params = {"embedding_size": K, "learning_rate": 1e-3, "dropout": 0.5, "max_batch_size": 64, "hist_len": P}
    est = Estimator(din.model_fn, None, params, RunConfig(device=str(dev), seed=1234))
    z1, zP = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, P, dtype=torch.int32, device=dev)
    with torch.no_grad():
        est._call_model_fn({"i_id": z1, "i_cate": z1.clone(), "u_iid_seq": zP, "u_icat_seq": zP.clone()}, None, ModeKeys.PREDICT)
        g = torch.Generator(device="cpu").manual_seed(7)          # a served model is a trained one: no all-zero biases
        for k, p in est.store.dense.params.items():
            if k.split(".")[-1][0] == "b":
                p.add_((torch.rand(p.shape, generator=g) * 0.2 - 0.1).to(dev))
        est.store.embeddings["i_item"].table[:, 0].add_((torch.randn(din.N_ITEM, generator=g) * 0.3).to(dev))
    d = est.export_savedmodel(export_dir)
    del est
    pred = serving.Predictor.load(d, device=str(dev), max_batch_size=max_c, max_candidates=max_c)
    assert pred.path == "layers" and pred.rank_path == "fused", (pred.path, pred.rank_path)
    torch.cuda.synchronize()
    return pred


def request(C, seed):
    """One user's history (synthetic.din_batch: ragged, zero padded to P) and C candidates."""
    from recsys_amd import synthetic
    rng = np.random.default_rng(seed)
    h = synthetic.din_batch(rng, 1, P)
    c = synthetic.din_batch(rng, C, 1)
    return (h["u_iid_seq"][0].astype(np.int32), h["u_icat_seq"][0].astype(np.int32), c["i_id"].astype(np.int32),
            c["i_cate"].astype(np.int32))


def answer_a(pred, req):
    from recsys_amd import serving
    return pred.predict(serving.expand_rank_request(*req, hist_len=P))["prob"]


def answer_b(pred, req):
    return pred.rank_candidates(*req)["prob"]


def capture_both(pred, req):
    """Warm up and capture the request size on both paths -> (A's graph, B's graph, max |A - B|)."""
    C = len(req[2])
    for _ in range(3):                           # eager warm-up, capture + replay, replay
        pa, pb = answer_a(pred, req), answer_b(pred, req)
    err = float(np.abs(pa - pb).max())
    assert err <= 2e-5, (C, err)                 # (faster and different is not faster)
    ga = [g for k, g in pred._est._graphs.items() if k[0] == "infer" and g.graph is not None
          and g.static.views()[0]["i_id"].shape[0] == C]
    assert len(ga) == 1 and "graph" in pred._graphs[("rank", 1, C)]
    return ga[0].graph, pred._graphs[("rank", 1, C)]["graph"], err


def host_select(prob, k):
    """The k best of prob [C] in the order of serving.topk_rows_host (no NaN among probabilities): np.partition for the k-th
    value, every entry >= it in index order, a stable sort of those survivors (ties keep the lower index)."""
    C = len(prob)
    kk = min(k, C)
    thr = np.partition(prob, C - kk)[C - kk]
    cand = np.flatnonzero(prob >= thr)
    order = cand[np.argsort(-prob[cand], kind="stable")][:kk]
    return {"prob": prob[order], "index": order.astype(np.int32)}


def host_select_argpartition(prob, k):
    """The same answer from np.argpartition.  Its k picks are right except inside the tie group of the k-th value, where it may
    take any members: those are replaced by the group's lowest indices, then the picks go through the same stable sort."""
    C = len(prob)
    kk = min(k, C)
    pick = np.argpartition(-prob, kk - 1)[:kk] if kk < C else np.arange(C)
    thr = prob[pick].min()
    above = pick[prob[pick] > thr]
    cand = np.sort(np.concatenate([above, np.flatnonzero(prob == thr)[:kk - len(above)]]))
    order = cand[np.argsort(-prob[cand], kind="stable")]
    return {"prob": prob[order], "index": order.astype(np.int32)}


def topk_a(pred, req, k):
    return host_select(pred.rank_candidates(*req)["prob"], k)


def topk_b(pred, req, k):
    return pred.rank_candidates(*req, top_k=k)


def time_request_graphs(pred, graphs, n, zero_state):
    """us per request of replaying the captured graphs of a request's chunks (over the resident inputs of the last chunk)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    state = pred._rank["topk"]["state"] if zero_state else None
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        if state is not None:
            state.zero_()
        for g in graphs:
            g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def bench_topk(pred, sizes, k, a):
    out = []
    reqs = {C: request(C, 100 + C) for C in sizes}
    graphs = {}
    for C in sizes:                                        # every size warmed up and captured before any timing
        for _ in range(3):
            ra, rb = topk_a(pred, reqs[C], k), topk_b(pred, reqs[C], k)
        assert pred.topk_path == "device"
        assert np.array_equal(ra["index"], rb["index"]) and np.array_equal(ra["prob"].view(np.uint32), rb["prob"].view(np.uint32)), C
        ns = [min(pred.max_candidates, C - s) for s in range(0, C, pred.max_candidates)]
        graphs[C] = ([pred._graphs[("rank", 1, n)]["graph"] for n in ns], [pred._graphs[("rank_topk", 1, n, k)]["graph"] for n in ns])
    for C in sizes:
        ga, gb = graphs[C]
        # the replays run over whatever the static buffers hold: make that THIS request (its history decides the rank kernel's
        # time; the candidates are those of its last chunk), once for each contender's timed region below
        topk_a(pred, reqs[C], k)
        topk_b(pred, reqs[C], k)
        nrep = max(20, min(a.replays, int(5e5 / max(time_request_graphs(pred, gb, 10, True), 1.0))))
        nw = max(10, min(a.wall_calls, nrep))
        ta, tb, wa, wb = [], [], [], []
        for _ in range(a.repeats):                         # the contenders alternate within every round
            ta.append(time_request_graphs(pred, ga, nrep, False))
            tb.append(time_request_graphs(pred, gb, nrep, True))
        for _ in range(a.repeats):
            wa.append(time_wall(lambda p, r: topk_a(p, r, k), pred, reqs[C], nw))
            wb.append(time_wall(lambda p, r: topk_b(p, r, k), pred, reqs[C], nw))
        prob = pred.rank_candidates(*reqs[C])["prob"]
        sel_us = {}
        for fn in (host_select, host_select_argpartition):  # A uses the first; the second is the form the other way round
            assert np.array_equal(fn(prob, k)["index"], host_select(prob, k)["index"])
            t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(50):
                    fn(prob, k)
                t.append((time.perf_counter() - t0) / 50 * 1e6)
            sel_us[fn.__name__] = round(float(np.median(t)), 1)
        med = lambda x: float(np.median(x))
        spread = lambda x: max(x) - min(x)
        rec = {"candidates": C, "top_k": k, "chunks": len(ga),
               "A_device_us": round(med(ta), 3), "B_device_us": round(med(tb), 3), "device_B_minus_A_us": round(med(tb) - med(ta), 3),
               "A_device_repeats_us": [round(x, 3) for x in ta], "B_device_repeats_us": [round(x, 3) for x in tb],
               "A_wall_us": round(med(wa), 1), "B_wall_us": round(med(wb), 1), "wall_B_over_A": round(med(wb) / med(wa), 4),
               "A_wall_repeats_us": [round(x, 1) for x in wa], "B_wall_repeats_us": [round(x, 1) for x in wb],
               "wall_accepted": bool(med(wa) - med(wb) > max(spread(wa), spread(wb))),
               "A_host_selection_us": sel_us["host_select"], "argpartition_selection_us": sel_us["host_select_argpartition"],
               "history_valid_positions": int((reqs[C][0] > 0).sum()), "replays": nrep, "wall_calls": nw}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def recommend_request(U, seed):
    """U users' histories (synthetic.din_batch) and the whole catalogue: every item 1 .. N_ITEM - 1 once, a fixed category each."""
    from recsys_amd import din, synthetic
    rng = np.random.default_rng(seed)
    h = synthetic.din_batch(rng, U, P)
    items = np.arange(1, din.N_ITEM, dtype=np.int32)
    cates = rng.integers(1, din.N_CATE, len(items)).astype(np.int32)
    return h["u_iid_seq"].astype(np.int32), h["u_icat_seq"].astype(np.int32), items, cates


def recommend_a(pred, req, k):
    """What a caller does without `recommend`: the catalogue passed from the host, top_k over-fetched by the longest valid
    history, then the seen items dropped and the rest cut to k in numpy -> items [U, k]."""
    hi, hc, ci, cc = req
    over = k + int((hi > 0).sum(1).max())
    out = pred.rank_candidates(hi, hc, ci, cc, top_k=over)
    items = np.take_along_axis(ci, out["index"].astype(np.int64), 1)
    res = np.empty((len(hi), k), np.int32)
    for u in range(len(hi)):
        res[u] = items[u][~np.isin(items[u], hi[u][hi[u] > 0])][:k]
    return res


def recommend_b(pred, req, k):
    return pred.recommend(req[0], req[1], k)["item"]


def bench_recommend(pred, k, a):
    """A against B for U = 1 and U = 16 users over the whole catalogue, alternating, medians and spread of --repeats rounds."""
    import torch
    out = []
    for U in (1, 16):
        hi, hc, items, cates = recommend_request(U, 300 + U)
        pred.set_catalogue(items, cates)
        req = (hi, hc, np.tile(items, (U, 1)), np.tile(cates, (U, 1)))     # A ships [U, N] candidates with every request
        for _ in range(3):                                     # eager, capture, replay -- before any timing
            ra, rb = recommend_a(pred, req, k), recommend_b(pred, req, k)
        assert pred.topk_path == "device" and pred.recommend_path == "device"
        assert np.array_equal(ra, rb), U                        # the same items in the same order
        N, over = len(items), k + int((hi > 0).sum(1).max())
        ns = [min(pred.max_candidates, N - s) for s in range(0, N, pred.max_candidates)]
        ga = [pred._graphs[("rank_topk", U, n, over)]["graph"] for n in ns]
        gb = [g["graph"] for key, g in pred._graphs.items() if key[0] == "recommend" and key[1:3] == (U, k)]
        assert len(gb) == 1
        nrep = max(10, min(a.replays, int(5e5 / max(time_request_graphs(pred, gb, 5, False), 1.0))))
        nw = max(5, min(a.wall_calls, nrep))
        ta, tb, wa, wb = [], [], [], []
        for _ in range(a.repeats):                             # the contenders alternate within every round
            recommend_a(pred, req, k)                           # (the static buffers hold this request on A's side)
            ta.append(time_request_graphs(pred, ga, nrep, True))
            tb.append(time_request_graphs(pred, gb, nrep, False))
        for _ in range(a.repeats):
            wa.append(time_wall(lambda p, r: recommend_a(p, r, k), pred, req, nw))
            wb.append(time_wall(lambda p, r: recommend_b(p, r, k), pred, req, nw))
        med = lambda x: float(np.median(x))
        spread = lambda x: max(x) - min(x)
        rec = {"users": U, "catalogue": N, "top_k": k, "A_top_k": over, "chunks": len(ns), "A_graphs": len(ga), "B_graphs": 1,
               "A_device_us": round(med(ta), 3), "B_device_us": round(med(tb), 3), "device_B_minus_A_us": round(med(tb) - med(ta), 3),
               "A_device_repeats_us": [round(x, 3) for x in ta], "B_device_repeats_us": [round(x, 3) for x in tb],
               "device_accepted": bool(med(ta) - med(tb) > max(spread(ta), spread(tb))),
               "A_wall_us": round(med(wa), 1), "B_wall_us": round(med(wb), 1), "wall_B_over_A": round(med(wb) / med(wa), 4),
               "A_wall_repeats_us": [round(x, 1) for x in wa], "B_wall_repeats_us": [round(x, 1) for x in wb],
               "wall_accepted": bool(med(wa) - med(wb) > max(spread(wa), spread(wb))),
               "A_request_bytes_host_to_device": int(8 * U * N + 8 * U * P), "B_request_bytes_host_to_device": int(8 * U * P + 4 * U * 128),
               "history_valid_positions_max": over - k, "replays": nrep, "wall_calls": nw}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    return out


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


def time_wall(fn, pred, req, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn(pred, req)                             # (ends in a device-to-host copy of prob: synchronises)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def flops(C, valid):
    return 2 * 2 * C * valid * (K * 80 + 80 * 40 + 40)


def kernel_stats(path):
    rows = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            rows[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]), float(row["AverageNs"]))
    return rows


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="1,16,200,1000,4096")
    p.add_argument("--replays", type=int, default=2000)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--wall_calls", type=int, default=200)
    p.add_argument("--profile-run", dest="profile_run", type=int, default=0, help="C of a rocprofv3 run")
    p.add_argument("--profile-requests", dest="profile_requests", type=int, default=200)
    p.add_argument("--kernel-stats", dest="kernel_stats", default=None)
    p.add_argument("--top_k", type=int, default=0, help="compare the top-k request: host selection against rank_candidates(top_k=K)")
    p.add_argument("--max_candidates", type=int, default=4096, help="--top_k / --recommend: candidates per rank launch")
    p.add_argument("--recommend", action="store_true",
                   help="compare the whole-catalogue request without seen items: over-fetch + numpy filter against Predictor.recommend")
    a = p.parse_args()
    if a.kernel_stats and a.top_k:                # the selection launch next to the rank launch, from the trace
        st = kernel_stats(a.kernel_stats)
        rec = {"candidates": a.profile_run, "top_k": a.top_k}
        for tag, kern in (("topk", "topk_rows_k"), ("rank", B_KERNEL)):
            c = [(c, avg) for name, (c, t, avg) in st.items() if kern in name]
            if not c or not sum(x[0] for x in c):
                sys.exit("%s holds no launch of %s: was the trace taken with --top_k %d --profile-run C on a Predictor whose "
                         "topk_path is \"device\"?" % (a.kernel_stats, kern, a.top_k))
            rec[tag + "_calls"], rec[tag + "_kernel_us"] = sum(x[0] for x in c), round(sum(x[0] * x[1] for x in c) / sum(x[0] for x in c) / 1e3, 3)
        print(json.dumps(rec), flush=True)
        return rec
    if a.kernel_stats:                            # no GPU needed: the trace's own numbers
        C, n = a.profile_run, a.profile_requests
        st = kernel_stats(a.kernel_stats)
        b = [(c, t, avg) for name, (c, t, avg) in st.items() if B_KERNEL in name]
        # A's kernels: everything else the trace holds at least once per request (the Estimator's and the Predictor's variable
        # set-up add one or two calls each: per request = calls // requests, at the kernel's average time); the runtime's
        # buffer copies serve both contenders and are left out
        a_k = {name: (c // n, c // n * avg) for name, (c, t, avg) in st.items()
               if B_KERNEL not in name and "copyBuffer" not in name and c >= n}
        req = request(C, 100 + C)
        valid = int((req[0] > 0).sum())
        fl = flops(C, valid)
        rec = {"candidates": C, "A_kernels_per_request": sum(c for c, _ in a_k.values()),
               "A_kernel_us_per_request": round(sum(t for _, t in a_k.values()) / 1e3, 3),
               "B_kernel_us_per_request": round(b[0][2] / 1e3, 3), "B_calls": b[0][0], "valid_positions": valid,
               "request_flops": fl, "B_achieved_TFLOPs": round(fl / b[0][2] / 1e3, 3),
               "B_share_of_fp32_mfma_peak": round(fl / (b[0][2] * 1e-9) / PEAK_F32_MFMA, 4),
               "A_kernels": {name[:48]: c for name, (c, _) in sorted(a_k.items())}}
        print(json.dumps(rec), flush=True)
        return rec
    from recsys_amd import build as _b
    _b.build(verbose=False)
    dev = torch.device("cuda")
    if a.top_k and a.sizes == p.get_default("sizes"):
        a.sizes = "200,4096,63001"
    sizes = [int(s) for s in a.sizes.split(",")] if not a.profile_run else [a.profile_run]
    with tempfile.TemporaryDirectory() as tmp:
        pred = build(dev, a.max_candidates if a.top_k or a.recommend else max(sizes), os.path.join(tmp, "export"))
    if a.recommend:
        return bench_recommend(pred, a.top_k or 100, a)
    if a.top_k and a.profile_run:
        pred.use_hip_graph = False                                      # eager: the launches appear in the trace under their names
        req = request(a.profile_run, 100 + a.profile_run)
        for _ in range(a.profile_requests):
            topk_b(pred, req, a.top_k)
        torch.cuda.synchronize()
        return None
    if a.top_k:
        return bench_topk(pred, sizes, a.top_k, a)
    if a.profile_run:
        pred.use_hip_graph = pred._est.config.use_hip_graph = False     # eager: every launch appears in the trace under its name
        req = request(a.profile_run, 100 + a.profile_run)
        for _ in range(a.profile_requests):
            answer_a(pred, req)
        for _ in range(a.profile_requests):
            answer_b(pred, req)
        torch.cuda.synchronize()
        return None
    out = []
    reqs = {C: request(C, 100 + C) for C in sizes}
    graphs = {C: capture_both(pred, reqs[C]) for C in sizes}            # every size, before any timing
    for C in sizes:
        ga, gb, err = graphs[C]
        na = max(20, min(a.replays, int(5e5 / max(time_replays(ga, 20), 1.0))))
        nb = max(20, min(a.replays, int(5e5 / max(time_replays(gb, 20), 1.0))))
        ta, tb, wa, wb = [], [], [], []
        for _ in range(a.repeats):                 # the contenders alternate within every round
            ta.append(time_replays(ga, na))
            tb.append(time_replays(gb, nb))
        nw = max(10, min(a.wall_calls, na))
        for fn in (answer_a, answer_b):
            time_wall(fn, pred, reqs[C], 5)
        for _ in range(a.repeats):
            wa.append(time_wall(answer_a, pred, reqs[C], nw))
            wb.append(time_wall(answer_b, pred, reqs[C], nw))
        med = lambda x: float(np.median(x))
        spread = lambda x: max(x) - min(x)
        valid = int((reqs[C][0] > 0).sum())
        rec = {"candidates": C, "valid_positions": valid,
               "A_device_us": round(med(ta), 3), "B_device_us": round(med(tb), 3), "device_B_over_A": round(med(tb) / med(ta), 4),
               "A_device_repeats_us": [round(x, 3) for x in ta], "B_device_repeats_us": [round(x, 3) for x in tb],
               "device_accepted": bool(med(ta) - med(tb) > max(spread(ta), spread(tb))),
               "A_wall_us": round(med(wa), 1), "B_wall_us": round(med(wb), 1), "wall_B_over_A": round(med(wb) / med(wa), 4),
               "A_wall_repeats_us": [round(x, 1) for x in wa], "B_wall_repeats_us": [round(x, 1) for x in wb],
               "wall_accepted": bool(med(wa) - med(wb) > max(spread(wa), spread(wb))),
               "max_abs_prob_diff": err, "replays": [na, nb], "wall_calls": nw, "request_flops": flops(C, valid),
               "B_TFLOPs_at_device_time": round(flops(C, valid) / med(tb) / 1e6, 3)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


if __name__ == "__main__":
    main()
