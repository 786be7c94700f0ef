"""Time per item-ranking request of an exported deepfm.py model AS COMMITTED (--feature_set uid_iid) at the reference's shape:
embedding_size 32, deep_layers 200,200,200, tables of 500 000 (u_id) + 100 000 (i_id) rows.  The two ways the package can
answer a request run in ONE process, their timed regions alternating, `--repeats` rounds each; medians and the spread
(max - min over the rounds) are reported, one JSON line per case.

  rank       U users x C items (default C = 1 / 16 / 200 / 1000 / 4096 for one user, and 4096 for 16 users, per-user lists):
       A  Predictor.predict(serving.expand_pair_request(...)): every pair hashed on the host (2 U C hashes), 8 U C bytes shipped,
          the rebuilt Estimator's inference graph (path == "layers": D = 32 is outside rsx_predict_fm_tower's envelope);
       B  Predictor.rank_items(u_id, i_id): U + U C hashes, 4 (U + U C) bytes, ONE launch of rsx_predict_pair_rank per chunk.
  recommend  the --top_k (100) best of a 100 000-item catalogue without 50 excluded ids per user, U = 1 and U = 16:
       A  rank_items over the catalogue passed from the host (25 chunks, every chunk's probabilities copied back), then
          serving.recommend_items_host;
       B  set_item_catalogue once, then recommend_items: per chunk rsx_predict_pair_rank over the resident rows and
          rsx_topk_rows_excl, the whole request ONE captured graph, one copy back.  Both must return the same items (asserted).

Device time: hipEvents around replays of the request's captured graphs over resident inputs (every case of both contenders
warmed up and captured before any timing).  Wall time: host arrays in, host result out, around a synchronise.

    python scripts/bench_serving_pairs.py [--sizes 1,16,200,1000,4096] [--repeats 5] > profiles/serving_pair_rank.txt
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, LAYERS = 32, "200,200,200"


def build(dev, max_rows, max_c, export_dir):
    """-> Predictor of a uid_iid deepfm.py bundle at the reference's shape (both contenders answer from its variables)."""
    import torch
    from recsys_amd import deepfm, serving
    from recsys_amd.estimator import Estimator, ModeKeys, RunConfig
    from recsys_amd.feature_columns import build_model_columns
    lin, emb = build_model_columns(D)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": D, "learning_rate": 1e-3,
              "dropout": 0.5, "deep_layers": LAYERS, "max_batch_size": 64}
    est = Estimator(deepfm.model_fn, None, params, RunConfig(device=str(dev), seed=1234))
    with torch.no_grad():
        est._call_model_fn({"ids": torch.zeros(1, 2, dtype=torch.int32, device=dev)}, None, ModeKeys.PREDICT)
        g = torch.Generator(device="cpu").manual_seed(7)          # a served model is a trained one: no all-zero biases
        for k, p in est.store.dense.params.items():
            if k.split(".")[-1][0] == "b":
                p.add_((torch.rand(p.shape, generator=g) * 0.2 - 0.1).to(dev))
    d = est.export_savedmodel(export_dir)
    del est
    pred = serving.Predictor.load(d, device=str(dev), max_batch_size=max_rows, max_candidates=max_c)
    assert pred.path == "layers" and pred.pair_path == "fused", (pred.path, pred.pair_path)
    torch.cuda.synchronize()
    return pred


def answer_a(pred, req):
    from recsys_amd import serving
    return pred.predict({"ids": serving.expand_pair_request(pred.layout, *req)})["prob"].reshape(req[1].shape)


def answer_b(pred, req):
    return pred.rank_items(*req)["prob"]


def replay_us(graphs, n, before=None):
    """us per request of replaying the captured graphs of one request over the resident inputs."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        if before is not None:
            before()
        for g in graphs:
            g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def wall_us(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()                                      # (ends in a device-to-host copy: synchronises)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def infer_graphs(pred, rows):
    """The Estimator's captured inference graphs of a request of `rows` examples, chunk by chunk."""
    out = []
    for s in range(0, rows, pred.max_batch_size):
        n = min(pred.max_batch_size, rows - s)
        g = [g for k, g in pred._est._graphs.items() if k[0] == "infer" and g.graph is not None
             and g.static.views()[0]["ids"].shape[0] == n]
        assert len(g) == 1, (rows, n, len(g))
        out.append(g[0].graph)
    return out


def pair_graphs(pred, U, C, ld_of):
    ns = [min(pred.max_candidates, C - s) for s in range(0, C, pred.max_candidates)]
    return [pred._graphs[("pair_rank", U, n, ld_of(n))]["graph"] for n in ns]


def compare(ta, tb, wa, wb, extra):
    med = lambda x: float(np.median(x))
    spread = lambda x: max(x) - min(x)
    rec = dict(extra)
    rec.update({"A_device_us": round(med(ta), 3), "B_device_us": round(med(tb), 3), "device_A_over_B": round(med(ta) / med(tb), 3),
                "A_device_spread_us": round(spread(ta), 3), "B_device_spread_us": round(spread(tb), 3),
                "device_B_wins": bool(med(ta) - med(tb) > max(spread(ta), spread(tb))),
                "device_B_loses": bool(med(tb) - med(ta) > max(spread(ta), spread(tb))),
                "A_wall_us": round(med(wa), 1), "B_wall_us": round(med(wb), 1), "wall_A_over_B": round(med(wa) / med(wb), 3),
                "A_wall_spread_us": round(spread(wa), 1), "B_wall_spread_us": round(spread(wb), 1),
                "wall_B_wins": bool(med(wa) - med(wb) > max(spread(wa), spread(wb))),
                "wall_B_loses": bool(med(wb) - med(wa) > max(spread(wa), spread(wb))),
                "A_device_repeats_us": [round(x, 3) for x in ta], "B_device_repeats_us": [round(x, 3) for x in tb],
                "A_wall_repeats_us": [round(x, 1) for x in wa], "B_wall_repeats_us": [round(x, 1) for x in wb]})
    print(json.dumps(rec), flush=True)
    return rec


def reps_for(us, a):
    """Replays of a timed region of about 0.3 s, at least 10 and at most --replays."""
    return max(10, min(a.replays, int(3e5 / max(us, 1.0))))


def bench_rank(pred, cases, a):
    rng = np.random.default_rng(100)
    reqs, graphs = {}, {}
    for U, C in cases:                            # every case warmed up and captured on both paths before any timing
        u = rng.integers(0, 10 ** 7, U).astype(np.int64)
        it = rng.integers(0, 10 ** 7, (U, C)).astype(np.int64)
        req = reqs[(U, C)] = (int(u[0]), it[0]) if U == 1 else (u, it)
        for _ in range(3):
            pa, pb = answer_a(pred, req), answer_b(pred, req)
        err = float(np.abs(pa - pb).max())
        assert err <= 2e-5, (U, C, err)           # (faster and different is not faster)
        graphs[(U, C)] = (infer_graphs(pred, U * C), pair_graphs(pred, U, C, (lambda n: 0) if U == 1 else (lambda n: n)), err)
    out = []
    for U, C in cases:
        req = reqs[(U, C)]
        ga, gb, err = graphs[(U, C)]
        answer_a(pred, req), answer_b(pred, req)  # the static buffers hold THIS request on both sides
        na, nb = reps_for(replay_us(ga, 10), a), reps_for(replay_us(gb, 10), a)
        ta, tb, wa, wb = [], [], [], []
        for _ in range(a.repeats):                # the contenders alternate within every round
            ta.append(replay_us(ga, na))
            tb.append(replay_us(gb, nb))
        nw = max(5, min(a.wall_calls, int(3e5 / max(wall_us(lambda: answer_a(pred, req), 3), 1.0))))
        wall_us(lambda: answer_a(pred, req), nw), wall_us(lambda: answer_b(pred, req), nw)      # one untimed round each
        for _ in range(a.repeats):
            wa.append(wall_us(lambda: answer_a(pred, req), nw))
            wb.append(wall_us(lambda: answer_b(pred, req), nw))
        out.append(compare(ta, tb, wa, wb, {"case": "rank", "users": U, "items": C, "A_graphs": len(ga), "B_graphs": len(gb),
                                            "max_abs_prob_diff": err, "replays": [na, nb], "wall_calls": nw,
                                            "A_request_bytes_host_to_device": 8 * U * C, "B_request_bytes_host_to_device": 4 * (U + U * C)}))
    return out


def bench_recommend(pred, N, k, a):
    from recsys_amd import serving
    rng = np.random.default_rng(200)
    cat = rng.permutation(10 ** 7)[:N].astype(np.int64)
    pred.set_item_catalogue(cat)
    out = []
    for U in (1, 16):
        u = rng.integers(0, 10 ** 7, U).astype(np.int64)
        excl = cat[rng.integers(0, N, (U, 50))]

        def rec_a():
            return serving.recommend_items_host(pred.rank_items(u, cat)["prob"], cat, excl, k)

        def rec_b():
            return pred.recommend_items(u, k, excl)
        for _ in range(3):                        # eager, capture, replay -- before any timing
            ra, rb = rec_a(), rec_b()
        assert pred.recommend_items_path == "device"
        assert np.array_equal(ra["item"], rb["item"]) and np.array_equal(ra["prob"].view(np.uint32), rb["prob"].view(np.uint32)), U
        ga = pair_graphs(pred, U, N, lambda n: 0)
        gb = [g["graph"] for key, g in pred._graphs.items() if key[0] == "pair_recommend" and key[1:3] == (U, k)]
        assert len(gb) == 1
        na, nb = reps_for(replay_us(ga, 3), a), reps_for(replay_us(gb, 3), a)
        ta, tb, wa, wb = [], [], [], []
        for _ in range(a.repeats):
            ta.append(replay_us(ga, na))
            tb.append(replay_us(gb, nb))
        nw = max(3, min(a.wall_calls, int(3e5 / max(wall_us(rec_a, 2), 1.0))))
        wall_us(rec_a, nw), wall_us(rec_b, nw)                                                  # one untimed round each
        for _ in range(a.repeats):
            wa.append(wall_us(rec_a, nw))
            wb.append(wall_us(rec_b, nw))
        out.append(compare(ta, tb, wa, wb, {"case": "recommend", "users": U, "catalogue": N, "top_k": k, "excluded_per_user": 50,
                                            "A_graphs": len(ga), "B_graphs": 1, "replays": [na, nb], "wall_calls": nw,
                                            "A_device_note": "A's device time leaves out its host selection and its copies",
                                            "A_request_bytes_host_to_device": 4 * (U + N), "B_request_bytes_host_to_device": 4 * (U + 64 * U),
                                            "A_result_bytes_device_to_host": 4 * U * N, "B_result_bytes_device_to_host": 4 * (2 * U * k + 2 * U)}))
    return out


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="1,16,200,1000,4096", help="items per request of one user")
    p.add_argument("--many", default="16x4096", help="one more rank case, UxC with per-user lists ('' for none)")
    p.add_argument("--catalogue", type=int, default=100000)
    p.add_argument("--top_k", type=int, default=100)
    p.add_argument("--max_candidates", type=int, default=4096)
    p.add_argument("--replays", type=int, default=2000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--wall_calls", type=int, default=200)
    p.add_argument("--skip", default="", help="'rank' or 'recommend'")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_serving_pairs.py measures on a GPU and there is none: not measured")
    from recsys_amd import build as _b
    _b.build(verbose=False)
    cases = [(1, int(s)) for s in a.sizes.split(",") if s]
    if a.many:
        cases.append(tuple(int(x) for x in a.many.split("x")))
    rows = max(U * C for U, C in cases)
    with tempfile.TemporaryDirectory() as tmp:
        pred = build(torch.device("cuda"), rows, a.max_candidates, os.path.join(tmp, "export"))
    print(json.dumps({"model": "deepfm.py uid_iid", "embedding_size": D, "deep_layers": LAYERS, "table_rows": [500000, 100000],
                      "max_batch_size": rows, "max_candidates": a.max_candidates, "repeats": a.repeats,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    out = []
    if a.skip != "rank":
        out += bench_rank(pred, cases, a)
    if a.skip != "recommend":
        out += bench_recommend(pred, a.catalogue, a.top_k, a)
    return out


if __name__ == "__main__":
    main()
