"""GPU box: what RunConfig.group_auc_key costs (metrics.GroupAUC, csrc/auc_group.hip).

Leg 1  Estimator.evaluate(steps=200) of deepfm.py at batch 256 and 4096 with the key off and on (`_c16`: 100 000 buckets, 17 id
       bits, 7 sort passes), alternating in ONE process, 5 rounds each: median and spread of the wall time (evaluate ends in
       device->host copies, so the host clock sees the device work), and the key's cost against the key-off evaluate.  A third
       arm of the same alternation has exact_auc on instead of the key: the other opt-in metric, one append launch per batch too.
Leg 2  rsx_auc_group_finalize + rsx_auc_group_records alone, by device events, at n = 51 200, 819 200 and 16 777 216 keys over
       100 000 groups (unsorted before every repetition: the restore copy is outside the events), beside rsx_auc_exact_finalize
       at the same n in the same run.  The device's header and records are checked against metrics.group_auc_records_host at
       every size, in every run.

`--out FILE` also writes the report there (profiles/eval_group_auc.txt is such a run)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recsys_amd import deepfm, metrics, synthetic
from recsys_amd._lib import check, lib
from recsys_amd.estimator import Estimator, RunConfig
from recsys_amd.feature_columns import CriteoLayout, build_feature_columns

KEY, GROUPS, BITS = "_c16", 100000, 17
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def leg_evaluate(rounds, steps):
    lin, emb = build_feature_columns(16, "indicator_all")
    layout = CriteoLayout.from_columns(emb)
    assert {c.key: c.rows for c in layout.columns}[KEY] == GROUPS
    say("leg 1: Estimator.evaluate(steps=%d), deepfm.py, group_auc_key off / %s / exact_auc instead, alternating, %d rounds, wall time in ms"
        % (steps, KEY, rounds))
    for B in (256, 4096):
        host = synthetic.criteo_id_batches(layout, 32, B, seed=5)
        params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
                  "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": B}
        est = Estimator(deepfm.model_fn, None, params, RunConfig(device="cuda", seed=1, log_step_count_steps=1000000))

        def fn(n):
            def gen():
                for s in range(n):
                    i, y, _ = host[s % 32]
                    yield {"ids": i}, y.reshape(-1, 1)
            return gen
        est.train(fn(40), steps=40)
        arms = {"off": (None, False), "key": (KEY, False), "exact": (None, True)}
        times = {a: [] for a in arms}
        res = {}
        for r in range(rounds + 1):               # round 0 warms every form up
            for arm, (key, exact) in arms.items():
                est.config.group_auc_key, est.config.exact_auc = key, exact
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[arm] = est.evaluate(fn(steps), steps=steps)
                dt = time.perf_counter() - t0
                if r:
                    times[arm].append(dt * 1e3)
        est.config.group_auc_key, est.config.exact_auc = None, False
        med = {a: statistics.median(t) for a, t in times.items()}
        say("  batch %4d  off: median %8.3f (min %8.3f max %8.3f)   key on: median %8.3f (min %8.3f max %8.3f)   "
            "exact_auc on instead: median %8.3f (min %8.3f max %8.3f)   the key costs %+.3f ms = %+.2f %% of the key-off evaluate, "
            "%+.3f ms against exact_auc   AUC %.7f GAUC %.7f over %d mixed groups, %d examples skipped"
            % (B, med["off"], min(times["off"]), max(times["off"]), med["key"], min(times["key"]), max(times["key"]),
               med["exact"], min(times["exact"]), max(times["exact"]), med["key"] - med["off"],
               100.0 * (med["key"] - med["off"]) / med["off"], med["key"] - med["exact"], res["key"]["AUC"], res["key"]["GAUC"],
               res["key"]["GAUC_groups"], res["key"]["GAUC_skipped_examples"]))


def timed(reps, restore, launch):
    us = []
    for r in range(reps + 2):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        if r >= 2:
            us.append(a.elapsed_time(b) * 1e3)
    return statistics.median(us), min(us), max(us)


def leg_finalize(reps):
    dev = torch.device("cuda")
    say("leg 2: rsx_auc_group_finalize + rsx_auc_group_records alone (%d groups, %d id bits: %d sort passes over 64-bit keys) beside "
        "rsx_auc_exact_finalize (4 passes over 32-bit keys), device events, %d repetitions on unsorted keys"
        % (GROUPS, BITS, 4 + (BITS + 7) // 8, reps))
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    L = lib()
    for n in (51200, 819200, 16777216):
        p = torch.sigmoid(torch.randn(n, device=dev, generator=gen) - 1.1)        # logit-normal scores, about 27 % positives
        y = (torch.rand(n, device=dev, generator=gen) < p).to(torch.float32)
        g = torch.randint(0, GROUPS, (n,), device=dev, generator=gen, dtype=torch.int32)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        ga = metrics.GroupAUC(dev, BITS, n)
        ga.update(g, y, p)
        pristine = ga.keys.clone()
        first = ga.result(per_group=True)
        hdr, mixed = list(ga.header), int(ga.header[3])
        rec_h, invalid = metrics.group_auc_records_host(g.cpu().numpy(), y.cpu().numpy(), p.cpu().numpy(), BITS)
        want_hdr = metrics.group_auc_header_host(rec_h, invalid)
        assert hdr == want_hdr, (hdr, want_hdr)
        assert np.array_equal(first["records"], rec_h[(rec_h[:, 1] > 0) & (rec_h[:, 2] > 0)])
        rec = torch.zeros((max(1, mixed), 4), dtype=torch.int64, device=dev)

        def group_launch():
            check(L.rsx_auc_group_finalize(C.c_void_p(ga.keys.data_ptr()), n, BITS, C.c_void_p(ga.workspace.data_ptr()),
                                           int(ga.workspace.numel()), C.c_void_p(ga.out.data_ptr()), stream))
            check(L.rsx_auc_group_records(C.c_void_p(ga.keys.data_ptr()), n, C.c_void_p(ga.workspace.data_ptr()),
                                          C.c_void_p(ga.out.data_ptr()), C.c_void_p(rec.data_ptr()), mixed, stream))
        g_med, g_min, g_max = timed(reps, lambda: ga.keys.copy_(pristine), group_launch)
        assert np.array_equal(rec[:mixed].cpu().numpy().view(np.uint64), first["records"])
        assert [int(v) for v in ga.out.cpu().numpy()[:8]] == hdr

        ex = metrics.ExactAUC(dev, n)
        ex.update(y, p)
        pristine32 = ex.keys.clone()
        e_first = ex.result()

        def exact_launch():
            check(L.rsx_auc_exact_finalize(C.c_void_p(ex.keys.data_ptr()), n, C.c_void_p(ex.workspace.data_ptr()),
                                           int(ex.workspace.numel()), C.c_void_p(ex.out.data_ptr()), stream))
        e_med, e_min, e_max = timed(reps, lambda: ex.keys.copy_(pristine32), exact_launch)
        assert ex.result() == e_first
        assert (hdr[5], hdr[6]) == (e_first["positives"], e_first["negatives"])
        say("  n %9d  group: median %10.1f us (min %10.1f max %10.1f)   exact: median %10.1f us (min %10.1f max %10.1f)   "
            "group / exact = %.2f   %8.1f keys/us   %d groups, %d mixed, GAUC %.7f   workspace %d B + keys %d B + records %d B"
            % (n, g_med, g_min, g_max, e_med, e_min, e_max, g_med / e_med, n / g_med, hdr[2], mixed, first["GAUC"],
               int(L.rsx_auc_group_workspace_bytes(n, BITS)), 8 * n, 32 * mixed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_group_auc.py measures on the GPU; none found")
    say("device: %s" % torch.cuda.get_device_name(0))
    leg_evaluate(a.rounds, a.steps)
    leg_finalize(a.reps)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
