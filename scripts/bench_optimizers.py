"""Step time of the TF-1 optimizers on the headline configurations: Adam (adam_mode tf1_dense and lazy_rows) against
Adagrad and FTRL (csrc/sparse_opt.hip), HBM-resident synthetic batches through Estimator.train_resident as bench.py times
them.  The variants of one configuration live in one process and their timed regions alternate, `--repeats` rounds; the
median region per variant is reported.

    python scripts/bench_optimizers.py [--configs deepfm:256,dcn:4096,fm:65536] [--steps 20] [--repeats 3]
    python scripts/bench_optimizers.py --kernel-stats <rocprofv3 *_kernel_stats.csv> ...   (achieved bandwidth of the launch)

Algorithmic bytes of one rsx_sparse_opt_multi launch: every updated element reads and writes var and the accumulator
(Adagrad: + the gradient read = 20 B) or var, linear and the accumulator (FTRL: 28 B); the elements are the step's unique
table rows x D plus the dense elements (the dense arena and the touched elements of the first-order vector)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {
    "adam_tf1_dense": dict(optimizer="adam", adam_mode="tf1_dense"),
    "adam_lazy_rows": dict(optimizer="adam", adam_mode="lazy_rows"),
    "adagrad": dict(optimizer="adagrad"),
    "ftrl": dict(optimizer="ftrl"),
}
BYTES_PER_ELEMENT = {"adagrad": 20, "ftrl": 28}


def build(model, B, variant, dev):
    import torch
    from recsys_amd import dcn, deepfm, fm, synthetic
    from recsys_amd.estimator import Estimator, PackedBatch, RunConfig
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    linear = {"deepfm": "indicator_all", "fm": "indicator_all", "dcn": "numeric"}[model]
    lin, emb = build_feature_columns(16, linear)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
              "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": B, "cross_layers": 3}
    mfn = {"deepfm": deepfm.model_fn, "fm": fm.model_fn, "dcn": dcn.model_fn}[model]
    est = Estimator(mfn, None, params, RunConfig(device=str(dev), seed=1234, **VARIANTS[variant]))
    layout = CriteoLayout.from_columns(emb)
    host = synthetic.criteo_id_batches(layout, 16, B, seed=synthetic.SEED)
    feats = [PackedBatch({"ids": i}, y, device=dev) for i, y, _ in host]
    torch.cuda.synchronize()
    return est, feats


def algorithmic_bytes(est, variant):
    """Bytes one rsx_sparse_opt_multi launch must move for the LAST step's batch (see the module docstring)."""
    if variant not in BYTES_PER_ELEMENT:
        return None
    st = est.store
    elems = st.dense.n
    for a in st.embeddings.values():
        u = int(a.nuniq.sum().item())
        elems += u * a.D + (u if a.with_w1 else 0)
    return elems * BYTES_PER_ELEMENT[variant]


def kernel_avg_ns(path, name="sparse_opt_k"):
    with open(path) as f:
        for row in csv.DictReader(f):
            if name in row.get("Name", ""):
                return float(row["AverageNs"])
    return None


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="deepfm:256,dcn:4096,fm:65536")
    p.add_argument("--variants", default=",".join(VARIANTS))
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--steps_per_graph", type=int, default=8)
    p.add_argument("--kernel-stats", dest="kernel_stats", default=None)
    a = p.parse_args()
    from recsys_amd import build as _b
    _b.build(verbose=False)
    dev = torch.device("cuda")
    variants = a.variants.split(",")
    out = []
    for cfg in a.configs.split(","):
        model, B = cfg.split(":")
        B = int(B)
        ests = {v: build(model, B, v, dev) for v in variants}
        for v, (est, feats) in ests.items():
            est.train_resident(feats, a.warmup, a.steps_per_graph)
            est.prepare_resident(feats, a.steps, a.steps_per_graph)
        dts = {v: [] for v in variants}
        for _ in range(a.repeats):
            for v, (est, feats) in ests.items():          # the variants alternate within every round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                est.train_resident(feats, a.steps, a.steps_per_graph)
                torch.cuda.synchronize()
                dts[v].append((time.perf_counter() - t0) / a.steps * 1e3)
        lazy = float(np.median(dts["adam_lazy_rows"])) if "adam_lazy_rows" in dts else None
        for v in variants:
            ms = float(np.median(dts[v]))
            rec = {"model": model, "batch_size": B, "variant": v, "ms_per_step": round(ms, 5),
                   "repeats_ms": [round(x, 5) for x in dts[v]]}
            if lazy:
                rec["vs_adam_lazy_rows"] = round(ms / lazy - 1.0, 4)
            nb = algorithmic_bytes(ests[v][0], v)
            if nb is not None:
                rec["sparse_opt_bytes_per_step"] = nb
                if a.kernel_stats:
                    ns = kernel_avg_ns(a.kernel_stats)
                    if ns:
                        rec["sparse_opt_kernel_us"] = round(ns / 1e3, 3)
                        rec["sparse_opt_GBps"] = round(nb / ns, 1)
            out.append(rec)
            print(json.dumps(rec), flush=True)
        del ests
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
