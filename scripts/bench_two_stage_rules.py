"""Time per `recommend_two_stage` request WITH category rules of an exported din.py model at the reference's sizes (K = 32,
hist_len = 100, the whole 63 001-item catalogue with 801 categories, histories of synthetic.din_batch), n = 32 neighbours per
item, top_k = 100, U = 1 and 16 users, on the ways the package can answer it, in ONE process, the timed regions alternating,
`--repeats` rounds; medians and the spread.

  A  the host path of the same request (Predictor.rules_on_device = False): serving.retrieve_candidates_host with the lists,
     rank_candidates over the padded lists, the greedy walk.  Wall time only: its device work is one rank launch among host
     loops, and the graph it replays changes with the longest list.
  B  the device path: ONE captured graph -- rsx_din_retrieve_candidates[_rules], rsx_predict_din_rank over [U, cap],
     rsx_topk_rows_counted or rsx_topk_lists_capped, the gather -- histories, exclusion ids and the bitmap shipped, one copy back.
  C  the plain device `recommend_two_stage` at the same k: what the rules cost on top of it.
  D  the device `recommend` with the same rules over the whole catalogue (rsx_topk_rows_rules): what a caller who needs rules
     uses today.  Its list differs from B's by design (B never leaves the candidate set).

Rules: a 10-category deny list per user ("deny10"), max_per_category = 2 ("m2"), and both ("m2_deny10").  A and B must return
the same bits (asserted).  The candidates per user before and after the filter are recorded: the rank launch runs over
[U, cap] whatever the counts are, so a filter shortens the lists, not the launch.  Wall time = host arrays in, host answer
out, around a synchronise; device time = replays of the request's captured graph.  There is no threshold: every ratio is
reported whichever way it falls, and "faster" only beyond the larger spread.

    python scripts/bench_two_stage_rules.py [--users 1,16] [--repeats 5] [--out profiles/serving_din_two_stage_rules.txt]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOP_K, M, N_NBR = 100, 2, 32
ARMS = ("A", "B", "C", "D")


def rules_of(name, U, seed):
    from recsys_amd import din
    rules = {}
    if "m2" in name:
        rules["max_per_category"] = M
    if "deny10" in name:
        rng = np.random.default_rng(seed)
        rules["exclude_categories"] = np.stack([rng.permutation(np.arange(1, din.N_CATE))[:10] for _ in range(U)])
    return rules


def same(a, b):
    return (np.array_equal(a["index"], b["index"]) and np.array_equal(a["count"], b["count"])
            and np.array_equal(a["prob"].view(np.uint32), b["prob"].view(np.uint32)))


def two_stage(pred, req, rules, on_device):
    pred.rules_on_device = on_device
    try:
        return pred.recommend_two_stage(req[0], req[1], TOP_K, **rules)
    finally:
        pred.rules_on_device = True


def measure(pred, req, rules, a):
    """-> (wall, device: {arm: repeats}, got: {arm: answer}, nrep, nw) with the regions alternating; A has no device time."""
    from scripts.bench_serving_din import time_request_graphs, time_wall
    U = len(req[0])
    call = {"A": lambda p, r: two_stage(p, r, rules, False), "B": lambda p, r: two_stage(p, r, rules, True),
            "C": lambda p, r: p.recommend_two_stage(r[0], r[1], TOP_K), "D": lambda p, r: p.recommend(r[0], r[1], TOP_K, **rules)}
    for _ in range(3):                                               # eager, capture, replay -- before any timing
        got = {x: call[x](pred, req) for x in ARMS}
        assert pred.recommend_path == "device"
    assert pred.two_stage_path_for(TOP_K, None, rules.get("max_per_category"), rules=True) == "device"
    assert same(got["A"], got["B"]), "A and B differ"
    how = ("exclude_categories" in rules, rules.get("max_per_category", 0))
    pick = lambda kind, n, tail: [g["graph"] for key, g in pred._graphs.items()
                                  if key[0] == kind and len(key) == n and key[1:3] == (U, TOP_K) and key[n - 2:] == tail]
    graphs = {"B": pick("two_stage", 8, how), "D": pick("recommend", 6, how),
              "C": [g["graph"] for key, g in pred._graphs.items() if key[0] == "two_stage" and len(key) == 6 and key[1:3] == (U, TOP_K)]}
    assert all(len(graphs[x]) == 1 for x in "BCD"), {x: len(v) for x, v in graphs.items()}
    nrep = max(10, min(a.replays, int(5e5 / max(time_request_graphs(pred, graphs["D"], 5, False), 1.0))))
    nw = max(3, min(a.wall_calls, 64 // U))
    wall, device = {x: [] for x in ARMS}, {x: [] for x in "BCD"}
    for _ in range(a.repeats):                                       # the contenders alternate within every round
        for x in "BCD":
            call[x](pred, req)                                       # (the static buffers hold this arm's request)
            device[x].append(time_request_graphs(pred, graphs[x], nrep, False))
    for _ in range(a.repeats):
        for x in ARMS:
            wall[x].append(time_wall(call[x], pred, req, nw))
    return wall, device, got, nrep, nw


def record(wall, device):
    med = lambda x: float(np.median(x))
    spread = lambda x: max(x) - min(x)
    rec = {}
    for x in ARMS:
        rec.update({x + "_wall_us": round(med(wall[x]), 1), x + "_wall_spread_us": round(spread(wall[x]), 1),
                    x + "_wall_repeats_us": [round(v, 1) for v in wall[x]]})
        if x in device:
            rec.update({x + "_device_us": round(med(device[x]), 2), x + "_device_spread_us": round(spread(device[x]), 2),
                        x + "_device_repeats_us": [round(v, 2) for v in device[x]]})

    def verdict(p, q, t):
        d, s = med(t[p]) - med(t[q]), max(spread(t[p]), spread(t[q]))
        return "%s faster" % q if d > s else ("%s faster" % p if -d > s else "inside the spread")
    for p, q in (("A", "B"), ("C", "B"), ("D", "B")):
        rec["wall_%s_vs_%s" % (p, q)], rec["wall_%s_over_%s" % (p, q)] = verdict(p, q, wall), round(med(wall[p]) / med(wall[q]), 2)
        if p in device:
            rec["device_%s_vs_%s" % (p, q)] = verdict(p, q, device)
            rec["device_%s_over_%s" % (p, q)] = round(med(device[p]) / med(device[q]), 2)
    return rec


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--users", default="1,16")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--replays", type=int, default=200)
    p.add_argument("--wall_calls", type=int, default=10)
    p.add_argument("--max_candidates", type=int, default=4096)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_din_two_stage_rules.txt"))
    a = p.parse_args()
    from recsys_amd import build as _b, din
    from scripts.bench_serving_din import build, recommend_request, P
    _b.build(verbose=False)
    with tempfile.TemporaryDirectory() as tmp:
        pred = build(torch.device("cuda"), a.max_candidates, os.path.join(tmp, "export"))
    lines = ["# scripts/bench_two_stage_rules.py --users %s --repeats %d --replays %d --wall_calls %d --max_candidates %d"
             % (a.users, a.repeats, a.replays, a.wall_calls, a.max_candidates),
             "# A: host path of the rule request (wall only); B: device path of the rule request; C: plain device recommend_two_stage;"
             " D: device recommend with the same rules over the whole catalogue; n = %d neighbours, top_k %d, m %d; medians of the"
             " repeats, the arms alternating" % (N_NBR, TOP_K, M)]
    built = False
    for U in (int(x) for x in a.users.split(",")):
        hi, hc, items, cates = recommend_request(U, 300 + U)
        N = len(items)
        if not built:
            pred.set_catalogue(items, cates)
            pred.build_neighbours(N_NBR)
            built = True
        for name in ("deny10", "m2", "m2_deny10"):
            rules = rules_of(name, U, 700 + U)
            wall, device, got, nrep, nw = measure(pred, (hi, hc), rules, a)
            filters = {k: v for k, v in rules.items() if k != "max_per_category"}
            before = pred.retrieve_candidates(hi, hc)["count"]
            after = pred.retrieve_candidates(hi, hc, **filters)["count"]
            rec = {"case": name, "users": U, "catalogue": N, "categories": int(din.N_CATE), "top_k": TOP_K, "history": P,
                   "n_neighbours": N_NBR, "cap": pred._two_stage_cap(P), **record(wall, device),
                   "candidates_mean": round(float(before.mean()), 1), "candidates_min": int(before.min()),
                   "candidates_after_filter_mean": round(float(after.mean()), 1), "candidates_after_filter_min": int(after.min()),
                   "B_count_min": int(np.min(got["B"]["count"])), "C_count_min": int(np.min(got["C"]["count"])),
                   "D_count_min": int(np.min(got["D"]["count"])), "replays": nrep, "wall_calls": nw}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
