"""Time per request of `recommend_two_stage` against `recommend` of the same commit, for an exported din.py model at the
reference's sizes (K = 32, hist_len = 100, the whole 63 001-item catalogue, histories of synthetic.din_batch), n = 32 neighbours
per item, top_k = 100, U = 1 and 16 users, in ONE process, the timed regions alternating, `--repeats` rounds; medians and spread.

  A  `recommend`: ONE captured graph -- per chunk rsx_predict_din_rank_shared over the resident catalogue and
     rsx_topk_rows_excl: every catalogue entry is scored for every user.
  B  `recommend_two_stage`: ONE captured graph -- rsx_din_retrieve_candidates, rsx_predict_din_rank over the users' candidate
     lists [U, cap], rsx_topk_rows_counted, the gather of the catalogue positions: at most hist_len (n + 1) entries are scored.

`build_neighbours` is timed once (wall time around a synchronise: the upload of the unit rows, per block of queries and per
chunk rsx_rows_dot and rsx_topk_rows_excl, the table's copy to the host).  Wall time of a request = host arrays in, host answer
out; device time = replays of the request's captured graph.  There is no threshold: every ratio is reported whichever way it
falls, and "faster" only beyond the larger spread.
The two lists DIFFER by design; overlap@k = |A's items and B's items| / k is printed beside the times.  On synthetic weights
the overlap says nothing about quality: the embeddings are random, so "neighbours" are arbitrary.  Quality is what
`retrieve_candidates` together with held-out items measures on a real model (the candidate recall of the retrieval stage).

    python scripts/bench_two_stage.py [--users 1,16] [--repeats 5] [--out profiles/serving_din_two_stage.txt]
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

TOP_K, N_NBR = 100, 32


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--users", default="1,16")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--replays", type=int, default=200)
    p.add_argument("--wall_calls", type=int, default=10)
    p.add_argument("--max_candidates", type=int, default=4096)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_din_two_stage.txt"))
    a = p.parse_args()
    from recsys_amd import build as _b
    from scripts.bench_serving_din import build, recommend_request, time_request_graphs, time_wall, K, P
    _b.build(verbose=False)
    with tempfile.TemporaryDirectory() as tmp:
        pred = build(torch.device("cuda"), a.max_candidates, os.path.join(tmp, "export"))
    lines = ["# scripts/bench_two_stage.py --users %s --repeats %d --replays %d --wall_calls %d --max_candidates %d"
             % (a.users, a.repeats, a.replays, a.wall_calls, a.max_candidates),
             "# A: recommend (the whole catalogue); B: recommend_two_stage (n = %d neighbours); top_k %d; medians of the repeats, the"
             " arms alternating.  overlap_at_k on synthetic weights says nothing about quality." % (N_NBR, TOP_K)]
    med = lambda x: float(np.median(x))
    spread = lambda x: max(x) - min(x)
    call = {"A": lambda q, r: q.recommend(r[0], r[1], TOP_K), "B": lambda q, r: q.recommend_two_stage(r[0], r[1], TOP_K)}
    built = False
    for U in (int(x) for x in a.users.split(",")):
        hi, hc, items, cates = recommend_request(U, 300 + U)
        N = len(items)
        if not built:
            pred.set_catalogue(items, cates)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pred.build_neighbours(N_NBR)
            torch.cuda.synchronize()
            rec = {"case": "build_neighbours", "catalogue": N, "K": K, "n_neighbours": N_NBR, "path": pred.neighbours_path,
                   "wall_s": round(time.perf_counter() - t0, 3), "multiply_adds": N * N * K,
                   "table_bytes": N * N_NBR * 8 + N * 4, "unit_rows_bytes": N * K * 4, "buffer_bytes": pred.neighbours_buffer_bytes()}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            built = True
        req = (hi, hc)
        for _ in range(3):                                               # eager, capture, replay -- before any timing
            got = {x: call[x](pred, req) for x in "AB"}
        assert pred.recommend_path == "device" and pred.two_stage_path == "device"
        cap = pred._two_stage_cap(P)
        graphs = {"A": [g["graph"] for key, g in pred._graphs.items() if key[0] == "recommend" and key[1:3] == (U, TOP_K)],
                  "B": [g["graph"] for key, g in pred._graphs.items() if key[0] == "two_stage" and key[1:3] == (U, TOP_K)]}
        assert len(graphs["A"]) == 1 and len(graphs["B"]) == 1
        nrep = max(10, min(a.replays, int(5e5 / max(time_request_graphs(pred, graphs["A"], 5, False), 1.0))))
        nw = max(3, min(a.wall_calls, 64 // U))
        wall, device = {x: [] for x in "AB"}, {x: [] for x in "AB"}
        for _ in range(a.repeats):                                       # the contenders alternate within every round
            for x in "AB":
                call[x](pred, req)                                       # (the static buffers hold this arm's request)
                device[x].append(time_request_graphs(pred, graphs[x], nrep, False))
        for _ in range(a.repeats):
            for x in "AB":
                wall[x].append(time_wall(call[x], pred, req, nw))
        n_cand = pred.retrieve_candidates(hi, hc)["count"]
        overlap = [len(np.intersect1d(got["A"]["item"][u][:got["A"]["count"][u]], got["B"]["item"][u][:got["B"]["count"][u]])) / TOP_K
                   for u in range(U)]
        rec = {"case": "request", "users": U, "catalogue": N, "top_k": TOP_K, "history": P, "n_neighbours": N_NBR, "cap": cap,
               "candidates_min": int(n_cand.min()), "candidates_mean": round(float(n_cand.mean()), 1), "candidates_max": int(n_cand.max()),
               "B_count_min": int(np.min(got["B"]["count"])), "overlap_at_k_mean": round(float(np.mean(overlap)), 3)}
        for x in "AB":
            rec.update({x + "_wall_us": round(med(wall[x]), 1), x + "_wall_spread_us": round(spread(wall[x]), 1),
                        x + "_device_us": round(med(device[x]), 2), x + "_device_spread_us": round(spread(device[x]), 2),
                        x + "_wall_repeats_us": [round(v, 1) for v in wall[x]], x + "_device_repeats_us": [round(v, 2) for v in device[x]]})
        for name, t in (("wall", wall), ("device", device)):
            d, s = med(t["A"]) - med(t["B"]), max(spread(t["A"]), spread(t["B"]))
            rec[name + "_A_vs_B"] = "B faster" if d > s else ("A faster" if -d > s else "inside the spread")
            rec[name + "_A_over_B"] = round(med(t["A"]) / med(t["B"]), 2)
        rec.update({"replays": nrep, "wall_calls": nw})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
