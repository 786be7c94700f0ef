"""GPU box: what RunConfig.calibration_bins / calibration_key cost (metrics.Calibration, csrc/calibration.hip).

Leg 1  Estimator.evaluate(steps=200) of deepfm.py at batch 256 and 4096 with the settings off, with calibration_bins = 20, and with
       calibration_bins = 20 + calibration_key = `_c16` (100 000 buckets), alternating in ONE process, 5 rounds each: median and
       spread of the wall time (evaluate ends in device->host copies, so the host clock sees the device work) and each arm's cost
       against the settings-off arm of the same run.
Leg 2  rsx_calibration_update alone, by device events around 50 back-to-back launches replayed as one captured graph (one launch
       is shorter than an event pair resolves, and the host cannot issue them as fast), at 256, 4096 and 1 048 576 examples: the bin table alone, both tables with ids spread over 100 000 groups, and
       both tables with EVERY example in one group -- what one hot id costs while the group table takes one atomic per example and
       word.  The device's tables are checked against metrics.calibration_bins_host / calibration_groups_host at every size.

`--out FILE` also writes the report there (profiles/eval_calibration.txt is such a run)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recsys_amd import deepfm, metrics, synthetic
from recsys_amd._lib import capture_gc_guard
from recsys_amd.estimator import Estimator, RunConfig
from recsys_amd.feature_columns import CriteoLayout, build_feature_columns

KEY, GROUPS, BINS = "_c16", 100000, 20
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def leg_evaluate(rounds, steps):
    lin, emb = build_feature_columns(16, "indicator_all")
    layout = CriteoLayout.from_columns(emb)
    assert {c.key: c.rows for c in layout.columns}[KEY] == GROUPS
    say("leg 1: Estimator.evaluate(steps=%d), deepfm.py, calibration off / calibration_bins=%d / calibration_bins=%d + "
        "calibration_key=%s, alternating, %d rounds, wall time in ms" % (steps, BINS, BINS, KEY, rounds))
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
        arms = {"off": (0, None), "bins": (BINS, None), "both": (BINS, KEY)}
        times = {a: [] for a in arms}
        res = {}
        for r in range(rounds + 1):               # round 0 warms every form up
            for arm, (bins, key) in arms.items():
                est.config.calibration_bins, est.config.calibration_key = bins, key
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[arm] = est.evaluate(fn(steps), steps=steps)
                dt = time.perf_counter() - t0
                if r:
                    times[arm].append(dt * 1e3)
        est.config.calibration_bins, est.config.calibration_key = 0, None
        assert all(res[a][k] == res["off"][k] for a in arms for k in res["off"])
        med = {a: statistics.median(t) for a, t in times.items()}
        say("  batch %4d  off: median %8.3f (min %8.3f max %8.3f)   bins: median %8.3f (min %8.3f max %8.3f)   "
            "bins + key: median %8.3f (min %8.3f max %8.3f)   bins cost %+.3f ms = %+.2f %%, bins + key %+.3f ms = %+.2f %% of the "
            "settings-off evaluate   ECE %.7f PCOC %.7f NE %.7f GCE %.7f over %d groups"
            % (B, med["off"], min(times["off"]), max(times["off"]), med["bins"], min(times["bins"]), max(times["bins"]),
               med["both"], min(times["both"]), max(times["both"]), med["bins"] - med["off"],
               100.0 * (med["bins"] - med["off"]) / med["off"], med["both"] - med["off"],
               100.0 * (med["both"] - med["off"]) / med["off"], res["both"]["ECE"], res["both"]["PCOC"], res["both"]["NE"],
               res["both"]["GCE"], res["both"]["GCE_groups"]))


def per_launch_us(reps, burst, launch):
    """The burst is captured into one graph (a chain of `burst` kernel nodes), so the events see the device, not the host's
    launch rate."""
    graph = torch.cuda.CUDAGraph()
    with capture_gc_guard(), torch.cuda.graph(graph):
        for _ in range(burst):
            launch()
    us = []
    for r in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        if r >= 2:
            us.append(a.elapsed_time(b) * 1e3 / burst)
    return statistics.median(us), min(us), max(us)


def leg_update(reps, burst):
    dev = torch.device("cuda")
    say("leg 2: rsx_calibration_update alone, device events around a captured graph of %d back-to-back launches, %d repetitions, us per launch; "
        "%d bins, %d groups" % (burst, reps, BINS, GROUPS))
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for n in (256, 4096, 1 << 20):
        p = torch.sigmoid(torch.randn(n, device=dev, generator=gen) - 1.1)        # logit-normal scores, about 27 % positives
        y = (torch.rand(n, device=dev, generator=gen) < p).to(torch.float32)
        spread = torch.randint(0, GROUPS, (n,), device=dev, generator=gen, dtype=torch.int32)
        hot = torch.full((n,), 4242, device=dev, dtype=torch.int32)
        yh, ph = y.cpu().numpy(), p.cpu().numpy()
        want_bins, _ = metrics.calibration_bins_host(yh, ph, BINS)
        out = {}
        for name, n_groups, g in (("bins", None, None), ("bins + spread ids", GROUPS, spread), ("bins + one hot id", GROUPS, hot)):
            cal = metrics.Calibration(dev, BINS, n_groups)
            cal.update(y, p, g)
            first = cal.result(per_group=True)
            assert np.array_equal(first["table"], want_bins)
            if g is not None:
                want, _ = metrics.calibration_groups_host(g.cpu().numpy(), yh, ph, GROUPS)
                live = np.flatnonzero(want[:, 0])
                assert np.array_equal(first["records"], np.concatenate([live.reshape(-1, 1), want[live]], axis=1))
            out[name] = per_launch_us(reps, burst, lambda: cal.update(y, p, g))
            launches = 1 + (reps + 2) * burst
            assert np.array_equal(cal.result()["table"], launches * want_bins)     # every launch of the burst added the batch
        say("  n %8d  " % n + "   ".join("%s: median %9.2f (min %9.2f max %9.2f)" % ((k,) + v) for k, v in out.items())
            + "   one hot id / spread ids = %.2f   %.1f examples/us with spread ids"
            % (out["bins + one hot id"][0] / out["bins + spread ids"][0], n / out["bins + spread ids"][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibration.py measures on the GPU; none found")
    say("device: %s" % torch.cuda.get_device_name(0))
    leg_evaluate(a.rounds, a.steps)
    leg_update(a.reps, a.burst)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
