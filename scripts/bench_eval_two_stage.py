"""Time per offline evaluation request of the TWO-STAGE list of an exported din.py model at the reference's sizes (K = 32,
hist_len = 100, the whole 63 001-item catalogue, histories of synthetic.din_batch, n = 32 neighbours per item): U users with T
held-out items each -> whether the retrieval stage kept every held-out item and the rank of the kept ones among the user's
candidates, on the two paths of `Predictor.evaluate_two_stage`, in ONE process, their timed regions alternating, `--repeats`
rounds per (U, T); medians and the spread are reported.

  A  the method's own host path (the same Predictor with the device path switched off for the call): retrieve_candidates_host
     on the host table, rank_candidates on the padded candidate lists (a blocking copy of every block's [U, width]
     probabilities), then numpy.
  B  the device path: per block of 16 users ONE captured graph -- rsx_din_retrieve_candidates, rsx_predict_din_rank over
     [U, cap], rsx_rank_count_lists (csrc/rank_count_lists.hip) -- and one copy of 12 bytes per (user, target slot) plus n_cand.

Both must return the same integers and probability bits (asserted).  Wall time = host arrays in, host answer out, around a
synchronise.  There is no threshold: the ratio is reported whichever way it falls.
Then, from the ONE table built, CandRecall and candidates_mean for n_neighbours = 8 / 16 / 32 (`n_neighbours=m` narrows the
table, nothing is rebuilt).  On synthetic weights these say nothing about quality: the embeddings are random, so
"neighbours" are arbitrary and held-out items are drawn at random; the lines show the call and what it costs, not a model.

    python scripts/bench_eval_two_stage.py [--users 1,16,256] [--targets 1,10] [--repeats 5] [--out profiles/serving_din_eval_two_stage.txt]
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

BLOCK, N_NBR = 16, 32


def evaluate(pred, req, device=True, m=None):
    hi, hc, held = req
    if device:
        return pred.evaluate_two_stage(hi, hc, held, ks=(10,), user_block=BLOCK, n_neighbours=m)
    pred._evaluate_two_stage_on_device = lambda T, cap: False            # arm A: this call takes the method's host path
    try:
        return pred.evaluate_two_stage(hi, hc, held, ks=(10,), user_block=BLOCK, n_neighbours=m)
    finally:
        del pred._evaluate_two_stage_on_device


def time_wall(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--users", default="1,16,256")
    p.add_argument("--targets", default="1,10")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--max_candidates", type=int, default=4096)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_din_eval_two_stage.txt"))
    a = p.parse_args()
    from recsys_amd import build as _b, serving
    from scripts.bench_eval_recommend import request
    from scripts.bench_serving_din import build, P
    _b.build(verbose=False)
    with tempfile.TemporaryDirectory() as tmp:
        pred = build(torch.device("cuda"), a.max_candidates, os.path.join(tmp, "export"))
    lines = ["# scripts/bench_eval_two_stage.py --users %s --targets %s --repeats %d --max_candidates %d"
             % (a.users, a.targets, a.repeats, a.max_candidates),
             "# A: evaluate_two_stage on its host path; B: evaluate_two_stage on its device path; n = %d neighbours; wall time host to"
             " host, medians of the repeats, the contenders alternating.  CandRecall on synthetic weights says nothing about quality."
             % N_NBR]
    med = lambda x: float(np.median(x))
    spread = lambda x: max(x) - min(x)

    def same(x, y):
        return (all(np.array_equal(x[k], y[k]) for k in ("rank", "retrieved", "target_index", "n_candidates"))
                and np.array_equal(x["target_prob"].view(np.uint32), y["target_prob"].view(np.uint32)))
    built = False
    for U in (int(x) for x in a.users.split(",")):
        for T in (int(x) for x in a.targets.split(",")):
            hi, hc, items, cates, held = request(U, T, 700 + U + T)
            if not built:                  # (the first request's catalogue serves them all: the items are the same every time)
                pred.set_catalogue(items, cates)
                pred.build_neighbours(N_NBR)
                built = True
            req = (hi, hc, held)
            assert pred.evaluate_two_stage_path_for(T) == "device"
            for _ in range(3):                                       # eager, capture, replay -- before any timing
                ra, rb = evaluate(pred, req, False), evaluate(pred, req, True)
            assert pred.evaluate_two_stage_path == "device" and same(ra, rb), (U, T)
            n = max(1, min(20, 64 // U))
            wa, wb = [], []
            for _ in range(a.repeats):                               # the contenders alternate within every round
                wa.append(time_wall(lambda: evaluate(pred, req, False), n))
                wb.append(time_wall(lambda: evaluate(pred, req, True), n))
            Tc = pred._target_capacity(T)
            cap = pred._two_stage_cap(P)
            rec = {"case": "request", "users": U, "targets": T, "catalogue": len(items), "history": P, "n_neighbours": N_NBR, "cap": cap,
                   "user_block": BLOCK, "A_wall_us": round(med(wa), 1), "B_wall_us": round(med(wb), 1),
                   "wall_B_over_A": round(med(wb) / med(wa), 4), "A_wall_repeats_us": [round(x, 1) for x in wa],
                   "B_wall_repeats_us": [round(x, 1) for x in wb], "A_wall_spread_us": round(spread(wa), 1),
                   "B_wall_spread_us": round(spread(wb), 1),
                   "A_vs_B": ("B faster" if med(wa) - med(wb) > max(spread(wa), spread(wb)) else
                              "A faster" if med(wb) - med(wa) > max(spread(wa), spread(wb)) else "inside the spread"),
                   "A_bytes_device_to_host": int(4 * sum(max(1, int(rb["n_candidates"][b:b + BLOCK].max())) * len(rb["n_candidates"][b:b + BLOCK])
                                                         for b in range(0, U, BLOCK))),
                   "B_bytes_device_to_host": int(sum(12 * (min(U, b + BLOCK) - b) * Tc + 4 * (min(U, b + BLOCK) - b) for b in range(0, U, BLOCK))),
                   "target_capacity": Tc, "candidates_mean": rb["candidates_mean"], "CandRecall": rb["CandRecall"],
                   "calls_per_region": n}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    # the sweep over n_neighbours from the one table: the largest request above, nothing rebuilt
    for m in (8, 16, 32):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = evaluate(pred, req, True, m)
        wall = time.perf_counter() - t0
        rec = {"case": "n_neighbours", "n_neighbours": m, "built": N_NBR, "users": len(req[0]), "targets": req[2].shape[1],
               "cap": serving.candidate_capacity(len(items), P, m), "CandRecall": out["CandRecall"],
               "CandRecall_users": out["CandRecall_users"], "candidates_mean": out["candidates_mean"], "HR@10": out["HR@10"],
               "first_call_wall_s": round(wall, 4), "neighbours_buffer_bytes": pred.neighbours_buffer_bytes(),
               "note": "synthetic weights: says nothing about quality"}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
