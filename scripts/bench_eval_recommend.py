"""Time per offline ranking-evaluation request of an exported din.py model at the reference's sizes (K = 32, hist_len = 100, the
whole 63 001-item catalogue, histories of synthetic.din_batch): U users with T held-out items each -> the rank of every held-out
item among the catalogue entries the user has not seen, on the two ways the package can answer it, in ONE process, their timed
regions alternating, `--repeats` rounds per (U, T); medians and the spread are reported.

  A  the host path, made only of what the package had before `evaluate_recommend`'s kernel: rank_candidates(history, the whole
     catalogue) per block of 16 users (a blocking copy of every chunk's [U, n] probabilities), then serving.target_ranks_host.
  B  Predictor.evaluate_recommend on its device path: per block of 16 users ONE captured graph -- the targets' scores, then
     rsx_predict_din_rank_shared and rsx_rank_count_rows (csrc/rank_count.hip) over every chunk -- and one copy of 8 bytes per
     (user, target slot).

Both must return the same ranks (asserted).  Wall time = host arrays in, host ranks out, around a synchronise.  There is no
threshold: the ratio is reported whichever way it falls.

    python scripts/bench_eval_recommend.py [--users 1,16,256] [--targets 1,10] [--repeats 5] [--out profiles/serving_din_eval_recommend.txt]
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

BLOCK = 16


def request(U, T, seed):
    """U histories, the whole catalogue (every item once, a fixed category each) and T held-out items per user: distinct
    catalogue items the user's history does not hold."""
    from scripts.bench_serving_din import recommend_request
    hi, hc, items, cates = recommend_request(U, seed)
    rng = np.random.default_rng(seed + 1)
    held = np.zeros((U, T), np.int64)
    for u in range(U):
        pool = rng.permutation(items)[:T + 128]
        held[u] = pool[~np.isin(pool, hi[u])][:T]
    return hi, hc, items, cates, held


def ranks_a(pred, req):
    from recsys_amd import serving
    hi, hc, items, cates, held = req
    out = np.empty(held.shape, np.int32)
    for b in range(0, len(hi), BLOCK):
        e = min(len(hi), b + BLOCK)
        prob = pred.rank_candidates(hi[b:e], hc[b:e], np.tile(items, (e - b, 1)), np.tile(cates, (e - b, 1)))["prob"]
        out[b:e] = serving.target_ranks_host(prob, items, hi[b:e], held[b:e])
    return out


def ranks_b(pred, req):
    return pred.evaluate_recommend(req[0], req[1], req[4], ks=(10,), user_block=BLOCK)["rank"]


def time_wall(fn, pred, req, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn(pred, req)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--users", default="1,16,256")
    p.add_argument("--targets", default="1,10")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--max_candidates", type=int, default=4096)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_din_eval_recommend.txt"))
    a = p.parse_args()
    from recsys_amd import build as _b
    from scripts.bench_serving_din import build, P
    _b.build(verbose=False)
    with tempfile.TemporaryDirectory() as tmp:
        pred = build(torch.device("cuda"), a.max_candidates, os.path.join(tmp, "export"))
    lines = ["# scripts/bench_eval_recommend.py --users %s --targets %s --repeats %d --max_candidates %d"
             % (a.users, a.targets, a.repeats, a.max_candidates),
             "# A: rank_candidates over the catalogue + target_ranks_host; B: evaluate_recommend (device path); wall time host to host,"
             " medians of the repeats, the contenders alternating"]
    for U in (int(x) for x in a.users.split(",")):
        for T in (int(x) for x in a.targets.split(",")):
            req = request(U, T, 500 + U + T)
            pred.set_catalogue(req[2], req[3])
            for _ in range(3):                                       # eager, capture, replay -- before any timing
                ra, rb = ranks_a(pred, req), ranks_b(pred, req)
            assert pred.evaluate_recommend_path == "device"
            assert np.array_equal(ra, rb) and (ra >= 0).all(), (U, T)
            N = len(req[2])
            n = max(1, min(20, 64 // U))
            wa, wb = [], []
            for _ in range(a.repeats):                               # the contenders alternate within every round
                wa.append(time_wall(ranks_a, pred, req, n))
                wb.append(time_wall(ranks_b, pred, req, n))
            med = lambda x: float(np.median(x))
            spread = lambda x: max(x) - min(x)
            Tc = pred._target_capacity(T)
            rec = {"users": U, "targets": T, "catalogue": N, "history": P, "chunks": -(-N // pred.max_candidates), "user_block": BLOCK,
                   "A_wall_us": round(med(wa), 1), "B_wall_us": round(med(wb), 1), "wall_B_over_A": round(med(wb) / med(wa), 4),
                   "A_wall_repeats_us": [round(x, 1) for x in wa], "B_wall_repeats_us": [round(x, 1) for x in wb],
                   "B_wins_beyond_spread": bool(med(wa) - med(wb) > max(spread(wa), spread(wb))),
                   "A_bytes_device_to_host": int(4 * U * N), "B_bytes_device_to_host": int(8 * U * Tc), "target_capacity": Tc,
                   "median_rank": float(np.median(ra)), "calls_per_region": n}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
