"""GPU box: what RunConfig.exact_auc costs (metrics.ExactAUC, csrc/auc_exact.hip).

Leg 1  Estimator.evaluate(steps=200) of deepfm.py at batch 256 and 4096 with the flag off and on, alternating in ONE process,
       5 rounds each: median and spread of the wall time (evaluate ends in a device->host copy, so the host clock sees the
       device work), and the flag's cost against the flag-off evaluate of the same commit.
Leg 2  rsx_auc_exact_finalize alone, by device events, at n = 51 200, 819 200 and 16 777 216 keys (unsorted before every
       repetition: the restore copy is outside the events).  The bytes its passes move are computed from n below; bytes / time
       over the HBM peak is the share of the BANDWIDTH bound (the sort does no arithmetic worth counting).

`--out FILE` also writes the report there (profiles/eval_exact_auc.txt is such a run)."""
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

HBM_PEAK = 8.0e12           # B/s, MI355X specification (a float4 copy reaches about 6.3e12)
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def finalize_bytes(n):
    """Bytes the launches of rsx_auc_exact_finalize read and write, from n (csrc/auc_exact.hip)."""
    tile, bins, passes = int(lib().rsx_auc_exact_tile()), 256, 4
    nt = (n + tile - 1) // tile
    hist = 4 * bins * nt
    per_pass = 4 * n + hist                 # histogram: reads the keys, writes the tile counts
    per_pass += 2 * hist                    # scan: in place
    per_pass += 4 * n + hist + 4 * n        # scatter: reads keys and offsets, writes keys
    reduce_ = (4 * n + 8 * nt) + 16 * nt + (4 * n + 8 * nt)      # counts, tile scan, u2
    return passes * per_pass + reduce_


def leg_evaluate(rounds, steps):
    lin, emb = build_feature_columns(16, "indicator_all")
    layout = CriteoLayout.from_columns(emb)
    say("leg 1: Estimator.evaluate(steps=%d), deepfm.py, flag off / on alternating, %d rounds, wall time in ms" % (steps, rounds))
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
        times = {False: [], True: []}
        res = {}
        for r in range(rounds + 1):               # round 0 warms both forms up
            for flag in (False, True):
                est.config.exact_auc = flag
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[flag] = est.evaluate(fn(steps), steps=steps)
                dt = time.perf_counter() - t0
                if r:
                    times[flag].append(dt * 1e3)
        off, on = statistics.median(times[False]), statistics.median(times[True])
        say("  batch %4d  off: median %8.3f (min %8.3f max %8.3f)   on: median %8.3f (min %8.3f max %8.3f)   "
            "flag costs %+.3f ms = %+.2f %% of the flag-off evaluate   AUC %.7f AUC_exact %.7f"
            % (B, off, min(times[False]), max(times[False]), on, min(times[True]), max(times[True]), on - off,
               100.0 * (on - off) / off, res[True]["AUC"], res[True]["AUC_exact"]))


def leg_finalize(reps):
    dev = torch.device("cuda")
    say("leg 2: rsx_auc_exact_finalize alone, device events, %d repetitions on unsorted keys; share = bytes / time / %.1f TB/s "
        "(the bandwidth bound)" % (reps, HBM_PEAK / 1e12))
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for n in (51200, 819200, 16777216):
        p = torch.sigmoid(torch.randn(n, device=dev, generator=gen) - 1.1)        # logit-normal scores, about 27 % positives
        y = (torch.rand(n, device=dev, generator=gen) < p).to(torch.float32)
        ex = metrics.ExactAUC(dev, n)
        ex.update(y, p)
        first = ex.result()
        pristine = torch.empty_like(ex.keys)
        ex.count = 0
        ex.out.zero_()
        ex.update(y, p)
        pristine.copy_(ex.keys)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        us = []
        for r in range(reps + 2):
            ex.keys.copy_(pristine)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            check(lib().rsx_auc_exact_finalize(C.c_void_p(ex.keys.data_ptr()), n, C.c_void_p(ex.workspace.data_ptr()),
                                               int(ex.workspace.numel()), C.c_void_p(ex.out.data_ptr()), stream))
            b.record()
            b.synchronize()
            if r >= 2:
                us.append(a.elapsed_time(b) * 1e3)
        again = ex.result()
        assert again == first, (first, again)
        if n <= 1 << 20:                           # the host statement of the same numbers (a 16.8 M-key numpy sort is left out)
            want = metrics.exact_auc_host(y.cpu().numpy(), p.cpu().numpy())
            assert want == first, (want, first)
        med, nbytes = statistics.median(us), finalize_bytes(n)
        say("  n %9d  median %10.1f us (min %10.1f max %10.1f)   %8.1f keys/us   %12d B moved -> %7.1f GB/s = %5.2f %% of the "
            "HBM peak (bandwidth-bound share)   workspace %d B + keys %d B"
            % (n, med, min(us), max(us), n / med, nbytes, nbytes / med / 1e3, 100.0 * nbytes / (med * 1e-6) / HBM_PEAK,
               int(lib().rsx_auc_exact_workspace_bytes(n)), 4 * n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_exact_auc.py measures on the GPU; none found")
    say("device: %s" % torch.cuda.get_device_name(0))
    leg_evaluate(a.rounds, a.steps)
    leg_finalize(a.reps)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
