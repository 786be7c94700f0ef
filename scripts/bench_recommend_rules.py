"""Time per `recommend` request WITH category rules of an exported din.py model at the reference's sizes (K = 32, hist_len = 100,
the whole 63 001-item catalogue with 801 categories, histories of synthetic.din_batch), top_k = 100, U = 1 and 16 users, on the
ways the package can answer it, in ONE process, their timed regions alternating, `--repeats` rounds; medians and the spread.

  A  the host path of the same request (Predictor.rules_on_device = False): rank_candidates(history, the whole catalogue) -- a
     blocking copy of every chunk's [U, n] probabilities -- then serving.recommend_host with the rules.
  B  the device path: ONE captured graph -- per chunk rsx_predict_din_rank_shared and rsx_topk_rows_rules (csrc/topk_rules.hip)
     -- the histories, the exclusion ids and the bitmap shipped, one copy of k pairs back.
  C  the plain device `recommend` at the same k (rsx_topk_rows_excl): what the rules kernel costs on top of it.

Rules: max_per_category = 2 ("m2"), and the same with a 10-category deny list per user ("m2_deny10").  A and B must return the
same bits (asserted).  One skewed case for B against C: half of the catalogue in ONE category, m = 2 -- the same-address case
of the threshold rounds.  Wall time = host arrays in, host answer out, around a synchronise; device time = replays of the
request's captured graphs.  There is no threshold: every ratio is reported whichever way it falls, and "wins" only beyond the
larger spread.

    python scripts/bench_recommend_rules.py [--users 1,16] [--repeats 5] [--out profiles/serving_din_recommend_rules.txt]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOP_K, M = 100, 2


def rules_of(name, U, seed):
    from recsys_amd import din
    if name == "m2":
        return {"max_per_category": M}
    rng = np.random.default_rng(seed)
    return {"max_per_category": M, "exclude_categories": np.stack([rng.permutation(np.arange(1, din.N_CATE))[:10] for _ in range(U)])}


def answer(pred, req, rules, on_device):
    pred.rules_on_device = on_device
    return pred.recommend(req[0], req[1], TOP_K, **rules)


def same(a, b):
    return (np.array_equal(a["index"], b["index"]) and np.array_equal(a["count"], b["count"])
            and np.array_equal(a["prob"].view(np.uint32), b["prob"].view(np.uint32)))


def graphs_of(pred, kind, pick):
    return [g["graph"] for key, g in pred._graphs.items() if key[0] == kind and pick(key)]


def measure(pred, req, rules, a, arms):
    """arms: names out of "A", "B", "C" -> {arm: (wall repeats, device repeats)} with the regions alternating."""
    from scripts.bench_serving_din import time_request_graphs, time_wall
    U = len(req[0])
    call = {"A": lambda p, r: answer(p, r, rules, False), "B": lambda p, r: answer(p, r, rules, True),
            "C": lambda p, r: p.recommend(r[0], r[1], TOP_K)}
    for _ in range(3):                                               # eager, capture, replay -- before any timing
        got = {x: call[x](pred, req) for x in arms}
    if "A" in arms:
        assert pred.recommend_path_for(TOP_K, M, rules=True) == "device" and same(got["A"], got["B"]), "A and B differ"
    m, bitmap = rules["max_per_category"], "exclude_categories" in rules
    N = pred.catalogue_size
    ns = sorted({min(pred.max_candidates, N - s) for s in range(0, N, pred.max_candidates)})
    graphs = {"A": [g for n in ns for g in graphs_of(pred, "rank", lambda k: k[1:] == (U, n))
                    for _ in range(sum(1 for s in range(0, N, pred.max_candidates) if min(pred.max_candidates, N - s) == n))],
              "B": graphs_of(pred, "recommend", lambda k: len(k) == 6 and k[1:3] == (U, TOP_K) and k[4:] == (bitmap, m)),
              "C": graphs_of(pred, "recommend", lambda k: len(k) == 4 and k[1:3] == (U, TOP_K))}
    assert len(graphs["B"]) == 1 and len(graphs["C"]) == 1
    nrep = max(10, min(a.replays, int(5e5 / max(time_request_graphs(pred, graphs["B"], 5, False), 1.0))))
    nw = max(3, min(a.wall_calls, 64 // U))
    wall, device = {x: [] for x in arms}, {x: [] for x in arms}
    for _ in range(a.repeats):                                       # the contenders alternate within every round
        for x in arms:
            call[x](pred, req)                                       # (the static buffers hold this arm's request)
            device[x].append(time_request_graphs(pred, graphs[x], nrep, False))
    for _ in range(a.repeats):
        for x in arms:
            wall[x].append(time_wall(call[x], pred, req, nw))
    return wall, device, got, nrep, nw


def record(wall, device, arms):
    med = lambda x: float(np.median(x))
    spread = lambda x: max(x) - min(x)
    rec = {}
    for x in arms:
        rec.update({x + "_wall_us": round(med(wall[x]), 1), x + "_wall_spread_us": round(spread(wall[x]), 1),
                    x + "_device_us": round(med(device[x]), 2), x + "_device_spread_us": round(spread(device[x]), 2),
                    x + "_wall_repeats_us": [round(v, 1) for v in wall[x]], x + "_device_repeats_us": [round(v, 2) for v in device[x]]})
    def verdict(p, q, t):
        d, s = med(t[p]) - med(t[q]), max(spread(t[p]), spread(t[q]))
        return "%s faster" % q if d > s else ("%s faster" % p if -d > s else "inside the spread")
    for p, q in (("A", "B"), ("C", "B")):
        if p in arms and q in arms:
            rec["wall_%s_vs_%s" % (p, q)], rec["device_%s_vs_%s" % (p, q)] = verdict(p, q, wall), verdict(p, q, device)
    return rec


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--users", default="1,16")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--replays", type=int, default=200)
    p.add_argument("--wall_calls", type=int, default=10)
    p.add_argument("--max_candidates", type=int, default=4096)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_din_recommend_rules.txt"))
    a = p.parse_args()
    from recsys_amd import build as _b, din
    from scripts.bench_serving_din import build, recommend_request, P
    _b.build(verbose=False)
    with tempfile.TemporaryDirectory() as tmp:
        pred = build(torch.device("cuda"), a.max_candidates, os.path.join(tmp, "export"))
    W = (din.N_CATE + 31) // 32
    lines = ["# scripts/bench_recommend_rules.py --users %s --repeats %d --replays %d --wall_calls %d --max_candidates %d"
             % (a.users, a.repeats, a.replays, a.wall_calls, a.max_candidates),
             "# A: host path (rank_candidates over the catalogue + recommend_host with the rules); B: device path (rsx_topk_rows_rules);"
             " C: plain device recommend (rsx_topk_rows_excl); top_k %d, m %d; medians of the repeats, the arms alternating" % (TOP_K, M)]
    for U in (int(x) for x in a.users.split(",")):
        hi, hc, items, cates = recommend_request(U, 300 + U)
        N = len(items)
        for name in ("m2", "m2_deny10"):
            pred.set_catalogue(items, cates)
            rules = rules_of(name, U, 700 + U)
            wall, device, got, nrep, nw = measure(pred, (hi, hc), rules, a, ("A", "B", "C"))
            E = pred._excl_capacity(P)
            rec = {"case": name, "users": U, "catalogue": N, "categories": int(din.N_CATE), "top_k": TOP_K, "history": P,
                   "chunks": -(-N // pred.max_candidates), **record(wall, device, ("A", "B", "C")),
                   "count_min": int(np.min(got["B"]["count"])), "plain_count_min": int(np.min(got["C"]["count"])),
                   "A_bytes_shipped_per_user": 8 * P + 8 * N, "A_bytes_returned_per_user": 4 * N,
                   "B_bytes_shipped_per_user": 8 * P + 4 * E + (4 * W if "exclude_categories" in rules else 0),
                   "B_bytes_returned_per_user": 8 * TOP_K + 8,
                   "C_bytes_shipped_per_user": 8 * P + 4 * E, "C_bytes_returned_per_user": 8 * TOP_K + 8,
                   "replays": nrep, "wall_calls": nw}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        # the skewed catalogue: half of the entries in ONE category
        skew = cates.copy()
        skew[np.random.default_rng(900 + U).random(N) < 0.5] = 1
        pred.set_catalogue(items, skew)
        wall, device, got, nrep, nw = measure(pred, (hi, hc), {"max_per_category": M}, a, ("B", "C"))
        rec = {"case": "m2_half_in_one_category", "users": U, "catalogue": N, "top_k": TOP_K, **record(wall, device, ("B", "C")),
               "count_min": int(np.min(got["B"]["count"])), "replays": nrep, "wall_calls": nw}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
