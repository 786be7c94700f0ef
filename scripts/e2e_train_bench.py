#!/usr/bin/env python
"""The whole product path end to end on the GPU box: TFRecord shards on disk -> C++ reader (framing, CRC-32C, Example parse,
FarmHash / bucketize, batching) -> Estimator.train (optimizer windows, one H2D copy per batch, HIP graphs) for deepfm.py and
fm.py at batch 256.  Prints examples/s of `Estimator.train` itself, input pipeline included.
usage: python scripts/e2e_train_bench.py [n_records=600000]
       python scripts/e2e_train_bench.py [n_records] --device_parse [--steps S] [--configs deepfm,fm,dcn] [--chunk C]
--device_parse: an A/B of `criteo_input_fn(device_parse=True)` (csrc/parse_records.hip; raw shard bytes to the GPU) against the
default host parse, ALTERNATING in one process, three runs each: median and spread of `Estimator.train` examples/s, of the input
pipeline alone, and the bytes shipped per example -- for deepfm.py and fm.py at batch 256 and dcn.py at batch 4096."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recsys_amd import dcn, deepfm, fm, synthetic
from recsys_amd import input_pipeline as ip
from recsys_amd.estimator import Estimator, RunConfig
from recsys_amd.feature_columns import CriteoLayout, build_feature_columns


def _opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _write_shards(d, n):
    rng = np.random.default_rng(0)
    files = []
    for k in range(4):
        label, cont, cat = synthetic.criteo_raw_batch(rng, n // 4)
        p = os.path.join(d, "part-r-%05d" % k)
        ip.write_criteo_shard(p, label, cont, cat)
        files.append(p)
    return files


def device_parse_ab(n):
    """See the module docstring."""
    steps_opt, chunk = _opt("--steps", 0), _opt("--chunk", 8)
    want = _opt("--configs", "deepfm,fm,dcn").split(",")
    configs = [c for c in (("deepfm", deepfm.model_fn, 256, "indicator_all", None), ("fm", fm.model_fn, 256, "indicator_all", None),
                           ("dcn", dcn.model_fn, 4096, "numeric", 3)) if c[0] in want]
    with tempfile.TemporaryDirectory() as d:
        files = _write_shards(d, n)
        shard_bytes = sum(os.path.getsize(f) for f in files)
        print("cores=%d  records=%d  shard bytes per record=%.1f  parse_chunk_batches=%d" % (os.cpu_count(), n, shard_bytes / n, chunk),
              flush=True)
        for name, mfn, bs, linear, cross in configs:
            lin, emb = build_feature_columns(16, linear)
            layout = CriteoLayout.from_columns(emb)
            params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
                      "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": bs, "cross_layers": cross}
            est = Estimator(mfn, None, params, RunConfig(device="cuda", seed=1, log_step_count_steps=1000000))

            def fn(flag):
                return lambda: ip.criteo_input_fn(files, bs, num_epochs=-1, need_shuffle=True, layout=layout, shuffle_buffer=100,
                                                  num_parallel=min(32, os.cpu_count()), device_parse=flag, parse_chunk_batches=chunk)
            steps = steps_opt or max(64, 2 * ((n // bs) // 8 * 8))
            for flag in (False, True):                     # build, warm-up, graph captures of both input signatures
                est.train(fn(flag), steps=min(steps, 96))
            torch.cuda.synchronize()
            train, alone, shipped = {False: [], True: []}, {False: [], True: []}, []
            for rep in range(3):
                for flag in (False, True):
                    t0 = time.time()
                    est.train(fn(flag), steps=steps)
                    torch.cuda.synchronize()
                    train[flag].append(steps * bs / (time.time() - t0) / 1e6)
            for rep in range(3):
                for flag in (False, True):
                    before = dict(ip.device_parse_stats)
                    it = iter(fn(flag)())
                    t0 = time.time()
                    for _ in range(steps):
                        x = next(it)
                    if flag:
                        torch.cuda.synchronize()
                    alone[flag].append(steps * bs / (time.time() - t0) / 1e6)
                    it.close()
                    del x
                    if flag:
                        after = ip.device_parse_stats
                        shipped.append((after["bytes"] - before["bytes"]) / max(1, after["records"] - before["records"]))
            for flag in (False, True):
                t, a = sorted(train[flag]), sorted(alone[flag])
                print("%-7s bs=%-5d device_parse=%-5s Estimator.train %.3f M examples/s (median of 3; %.3f .. %.3f)   input pipeline "
                      "alone %.3f M examples/s (%.3f .. %.3f)   bytes shipped per example %s"
                      % (name, bs, flag, t[1], t[0], t[2], a[1], a[0], a[2],
                         "%.1f" % sorted(shipped)[1] if flag else "%d (packed batch)" % ((bs * 4 + bs * 52 + bs * layout.F * 4) // bs)), flush=True)
            del est
            torch.cuda.empty_cache()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 600000
    if "--device_parse" in sys.argv:
        return device_parse_ab(n)
    bs = 256
    lin, emb = build_feature_columns(16, "indicator_all")
    layout = CriteoLayout.from_columns(emb)
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.default_rng(0)
        files = []
        for k in range(4):
            label, cont, cat = synthetic.criteo_raw_batch(rng, n // 4)
            p = os.path.join(d, "part-r-%05d" % k)
            ip.write_criteo_shard(p, label, cont, cat)
            files.append(p)
        print("cores=%d  records=%d  batch=%d" % (os.cpu_count(), n, bs), flush=True)
        for name, mfn in (("deepfm", deepfm.model_fn), ("fm", fm.model_fn)):
            params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
                      "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": bs}
            est = Estimator(mfn, None, params, RunConfig(device="cuda", seed=1, log_step_count_steps=1000000))
            fn = lambda: ip.criteo_input_fn(files, bs, num_epochs=-1, need_shuffle=True, layout=layout,
                                            num_parallel=min(32, os.cpu_count()))
            est.train(fn, steps=300)                       # build, warm-up, graph captures
            torch.cuda.synchronize()
            # every Estimator.train call starts its input pipeline afresh (reader threads, mmap, and the 1 000-batch shuffle
            # buffer has to fill before the first batch comes out): timed separately, and the runs are long enough to amortise it
            t0 = time.time()
            it = iter(fn())
            next(it)
            t_start = time.time() - t0
            it.close()
            print("%-7s input pipeline start-up (threads + shuffle buffer of 1000 batches) until the first batch: %.1f ms" % (name, t_start * 1e3), flush=True)
            steps = 4 * ((n // bs) // 8 * 8)
            for rep in range(3):
                t0 = time.time()
                est.train(fn, steps=steps)
                torch.cuda.synchronize()
                dt = time.time() - t0
                print("%-7s Estimator.train over TFRecord shards: %d steps in %.2f s = %.3f M examples/s (%.1f us per step; %.1f without the start-up)"
                      % (name, steps, dt, steps * bs / dt / 1e6, dt / steps * 1e6, (dt - t_start) / steps * 1e6), flush=True)
            # the same input pipeline alone (no training): what the host side can deliver
            t0 = time.time()
            it = iter(fn())
            for _ in range(steps):
                next(it)
            dt = time.time() - t0
            it.close()
            print("        input pipeline alone: %.3f M examples/s (%.1f us per batch)" % (steps * bs / dt / 1e6, dt / steps * 1e6), flush=True)


if __name__ == "__main__":
    main()
