"""GPU box: what isotonic calibration costs (csrc/calibration_map.hip; metrics.ExactAUC.quantile_table / Calibrator;
RunConfig.calibration_fit / calibration_apply; serving.Predictor(calibrated=...)).  Nothing here is a bar: the numbers say what the
feature's price is.

Leg 1  Serving.  Predictor.predict on a deepfm.py bundle (fused path) that carries a map, loaded with calibrated=False and True:
       device time per request (events around `--replays` replays of the request size's captured graph, the request resident)
       and wall time host to host (predict() from numpy ids to numpy prob), the two arms alternating in ONE process, median of
       `--rounds` rounds with min and max, at 1, 16, 200 and 4096 rows.  The comparison is the uncalibrated arm of the same run.
Leg 2  rsx_calibrate_apply alone: device events around 50 back-to-back launches replayed as one captured graph (as
       scripts/bench_calibration.py times its launch), n = 256, 4096 and 1 048 576, K = 16 and 1024 knots; at the last size the
       rate at 8 bytes per element against the HBM rate (8.0 TB/s specified, 6.29 TB/s measured for a float4 copy).
Leg 3  The fit.  ExactAUC.result() alone and result() + quantile_table(M), wall time (both end in a device->host copy),
       alternating, at 51 200, 819 200 and 16 777 216 keys, M = 64 and 1024; the all-scores-equal case (one workgroup reads every
       key) once at 819 200 keys.  The device's table is checked against metrics.quantile_table_host where the host can afford it.
Leg 4  Estimator.evaluate(steps=200) of deepfm.py at batch 256 and 4096: settings off, calibration_fit = 256, calibration_bins =
       20 alone, and calibration_apply + calibration_bins = 20, alternating, wall time.

`--out FILE` also writes the report there (profiles/serving_calibrated.txt is such a run)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recsys_amd import deepfm, metrics, serving, synthetic
from recsys_amd._lib import capture_gc_guard
from recsys_amd.estimator import Estimator, RunConfig
from recsys_amd.feature_columns import CriteoLayout, build_feature_columns

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def mmm(v):
    return "median %9.3f (min %9.3f max %9.3f)" % (statistics.median(v), min(v), max(v))


def trained(B, steps=40):
    lin, emb = build_feature_columns(16, "indicator_all")
    layout = CriteoLayout.from_columns(emb)
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
    est.train(fn(steps), steps=steps)
    return est, fn, host, layout


def leg_serving(rounds, replays, calls):
    est, fn, host, layout = trained(4096)
    est.config.calibration_fit = 256
    est.evaluate(fn(32), steps=32)
    est.config.calibration_fit = 0
    cmap = est.last_calibration_map
    say("leg 1: Predictor.predict, deepfm.py bundle on the fused path, a map of %d knots (fitted from %d examples at M = 256); "
        "calibrated off / on alternating, %d rounds; device time: events around %d replays of the request's graph; wall time: "
        "%d predict() calls host to host; us per request" % (cmap.knots, cmap.examples, rounds, replays, calls))
    with tempfile.TemporaryDirectory() as tmp:
        d = est.export_savedmodel(os.path.join(tmp, "export"), calibration="require")
        arms = {"off": serving.Predictor.load(d, max_batch_size=4096, calibrated=False),
                "on": serving.Predictor.load(d, max_batch_size=4096, calibrated=True)}
    assert arms["on"].path == "fused" and arms["on"].calibrated and not arms["off"].calibrated
    for n in (1, 16, 200, 4096):
        ids = np.ascontiguousarray(host[3][0][:n])
        out = {}
        for a, p in arms.items():
            for _ in range(3):                   # eager warm-up, capture, replay
                out[a] = p.predict({"ids": ids})["prob"]
            assert "graph" in p._graphs[n]
        assert np.array_equal(out["on"].view(np.uint32), metrics.isotonic_apply_host(out["off"], cmap.x, cmap.y).view(np.uint32))
        dev_us, wall_us = {a: [] for a in arms}, {a: [] for a in arms}
        for r in range(rounds + 1):              # round 0 is not counted
            for a, p in arms.items():
                g = p._graphs[n]["graph"]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(replays):
                    g.replay()
                e1.record()
                e1.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    p.predict({"ids": ids})
                dt = time.perf_counter() - t0
                if r:
                    dev_us[a].append(e0.elapsed_time(e1) * 1e3 / replays)
                    wall_us[a].append(dt * 1e6 / calls)
        md = {a: statistics.median(v) for a, v in dev_us.items()}
        mw = {a: statistics.median(v) for a, v in wall_us.items()}
        say("  rows %4d  device  off: %s   on: %s   on - off %+.3f us = %+.2f %%" % (n, mmm(dev_us["off"]), mmm(dev_us["on"]),
                                                                                   md["on"] - md["off"], 100 * (md["on"] - md["off"]) / md["off"]))
        say("             wall    off: %s   on: %s   on - off %+.3f us = %+.2f %%" % (mmm(wall_us["off"]), mmm(wall_us["on"]),
                                                                                   mw["on"] - mw["off"], 100 * (mw["on"] - mw["off"]) / mw["off"]))


def per_launch_us(reps, burst, launch):
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
    return us


def leg_apply(reps, burst):
    dev = torch.device("cuda")
    say("leg 2: rsx_calibrate_apply alone (out of place), device events around a captured graph of %d back-to-back launches, %d "
        "repetitions, us per launch" % (burst, reps))
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    rng = np.random.default_rng(3)
    for n in (256, 4096, 1 << 20):
        p = torch.sigmoid(torch.randn(n, device=dev, generator=gen) - 1.1)
        out = torch.empty_like(p)
        parts = []
        for K in (16, 1024):
            x = np.unique(rng.random(4 * K).astype(np.float32))[:K]
            y = np.sort(rng.random(K).astype(np.float32))
            cal = metrics.Calibrator(dev, metrics.IsotonicMap(x, y))
            cal.apply(p, out=out)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), metrics.isotonic_apply_host(p.cpu().numpy(), x, y).view(np.uint32))
            us = per_launch_us(reps, burst, lambda: cal.apply(p, out=out))
            rate = 8.0 * n / (statistics.median(us) * 1e-6)
            parts.append("K %4d: %s" % (K, mmm(us)) + ("   %.2f TB/s at 8 B per element = %.1f %% of the specified, %.1f %% of the "
                                                       "copy-measured HBM rate (8 MB: the data stays in the last-level cache)"
                                                       % (rate / 1e12, 100 * rate / HBM_SPEC, 100 * rate / HBM_COPY) if n == 1 << 20 else ""))
        say("  n %8d  " % n + "   ".join(parts))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def leg_fit(rounds):
    dev = torch.device("cuda")
    say("leg 3: the fit: ExactAUC.result() alone and result() + quantile_table(M), alternating, %d rounds, wall time in ms" % rounds)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)

    def run(name, p, y, check):
        ex = metrics.ExactAUC(dev, p.numel())
        ex.update(y, p)
        t = {"result": [], 64: [], 1024: []}
        for r in range(rounds + 1):
            dt, _ = timed(ex.result)
            if r:
                t["result"].append(dt)
            for M in (64, 1024):
                dt, table = timed(lambda: (ex.result(), ex.quantile_table(M))[1])
                if r:
                    t[M].append(dt)
                elif check:
                    assert np.array_equal(table, metrics.quantile_table_host(y.cpu().numpy(), p.cpu().numpy(), M))
                assert int(table[:, 0].sum()) == p.numel()
        m = {k: statistics.median(v) for k, v in t.items()}
        say("  %-28s result(): %s   + table M = 64: %s (%+.3f ms = %+.2f %%)   + table M = 1024: %s (%+.3f ms = %+.2f %%)"
            % (name, mmm(t["result"]), mmm(t[64]), m[64] - m["result"], 100 * (m[64] - m["result"]) / m["result"],
               mmm(t[1024]), m[1024] - m["result"], 100 * (m[1024] - m["result"]) / m["result"]))
    for n in (51200, 819200, 1 << 24):
        p = torch.sigmoid(torch.randn(n, device=dev, generator=gen) - 1.1)
        y = (torch.rand(n, device=dev, generator=gen) < p).to(torch.float32)
        run("%d keys" % n, p, y, n <= 819200)
    n = 819200
    y = (torch.rand(n, device=dev, generator=gen) < 0.3).to(torch.float32)
    run("%d keys, all scores equal" % n, torch.full((n,), 0.37, device=dev), y, True)


def leg_evaluate(rounds, steps):
    say("leg 4: Estimator.evaluate(steps=%d), deepfm.py: settings off / calibration_fit=256 / calibration_bins=20 / "
        "calibration_apply + calibration_bins=20, alternating, %d rounds, wall time in ms" % (steps, rounds))
    arms = {"off": (0, 0, False), "fit": (256, 0, False), "bins": (0, 20, False), "apply": (0, 20, True)}
    for B in (256, 4096):
        est, fn, _, _ = trained(B)
        times, res = {a: [] for a in arms}, {}
        for r in range(rounds + 1):               # round 0 warms every form up (and fits the map the apply arm loads)
            for arm, (fit, bins, app) in arms.items():
                est.config.calibration_fit, est.config.calibration_bins, est.config.calibration_apply = fit, bins, app
                dt, res[arm] = timed(lambda: est.evaluate(fn(steps), steps=steps))
                if r:
                    times[arm].append(dt)
        est.config.calibration_fit, est.config.calibration_bins, est.config.calibration_apply = 0, 0, False
        assert all(res[a][k] == res["off"][k] for a in arms for k in res["off"])
        med = {a: statistics.median(t) for a, t in times.items()}
        say("  batch %4d  " % B + "   ".join("%s: %s" % (a, mmm(times[a])) for a in arms))
        say("              fit %+.3f ms = %+.2f %% of the settings-off evaluate (K = %d);  apply + bins %+.3f ms = %+.2f %%, of which "
            "bins alone %+.3f ms;  ECE %.7f -> ECE_cal %.7f, PCOC %.7f -> PCOC_cal %.7f (in-sample here: the map was fitted on "
            "these batches)"
            % (med["fit"] - med["off"], 100 * (med["fit"] - med["off"]) / med["off"], res["fit"]["calibration_knots"],
               med["apply"] - med["off"], 100 * (med["apply"] - med["off"]) / med["off"], med["bins"] - med["off"],
               res["apply"]["ECE"], res["apply"]["ECE_cal"], res["apply"]["PCOC"], res["apply"]["PCOC_cal"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--replays", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--legs", default="1,2,3,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibration_map.py measures on the GPU; none found")
    say("device: %s" % torch.cuda.get_device_name(0))
    legs = set(a.legs.split(","))
    if "1" in legs:
        leg_serving(a.rounds, a.replays, a.calls)
    if "2" in legs:
        leg_apply(a.reps, a.burst)
    if "3" in legs:
        leg_fit(a.rounds)
    if "4" in legs:
        leg_evaluate(a.rounds, a.steps)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
