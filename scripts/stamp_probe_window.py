#!/usr/bin/env python
"""Phase stamps (100 MHz wall clock) of the stand-alone window sweep (adam_window_k), -DRSX_STAMPS build
(scripts/build_stamps.sh): when does the last block of the first-order vector leave, when the last table block?

    python scripts/stamp_probe_window.py [--void 0.85] [--idle 0.0] [--k 8] [--form 1]

DeepFM-size state as in scripts/window_compact_time.py (the same mix for the tables' rows and the vector's elements),
the segment list in the step's order (vector first); state restored before every launch; us since workgroup 0's entry."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["RSX_LIB_PATH"] = os.path.join(ROOT, "scripts", "_build", os.environ.get("RSX_STAMP_LIB", "librsx_stamps.so"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from recsys_amd.ops import AdamTF1, EmbeddingArena  # noqa: E402
from scripts.kernel_roofline_util import criteo_row_off, synth_ids  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--idle", type=float, default=0.0)
p.add_argument("--void", type=float, default=0.85)
p.add_argument("--k", type=int, default=8)
p.add_argument("--form", type=int, default=1)
args = p.parse_args()

dbg = C.CDLL(os.environ["RSX_LIB_PATH"])
row_off = criteo_row_off()
a = EmbeddingArena(row_off, 16, 256, "cuda", with_w1=True, w1_field_mask=(1 << 39) - 1)
g = torch.Generator(device="cuda").manual_seed(1)
with torch.no_grad():
    a.tables.normal_(generator=g); a.w1.normal_(generator=g)
    a.m_t.normal_(generator=g).mul_(0.01); a.v_t.uniform_(generator=g).mul_(1e-4).add_(1e-12)
    a.m_w.normal_(generator=g).mul_(0.01); a.v_w.uniform_(generator=g).mul_(1e-4).add_(1e-12)
    u = torch.rand(a.m_t.shape[0], device="cuda", generator=g)
    a.m_t[u < args.idle + args.void] = 0.0; a.m_w[u < args.idle + args.void] = 0.0
    a.v_t[u < args.void] = 0.0; a.v_w[u < args.void] = 0.0
state = [a.m_t, a.v_t, a.tables, a.m_w, a.v_w, a.w1]
state0 = [x.clone() for x in state]
rng = np.random.default_rng(0)
a.sort_window([torch.from_numpy(synth_ids(rng, 256, row_off)).cuda() for _ in range(args.k)])
opt = AdamTF1(device="cuda")
cold, _ = a.adam_split_segments(window_k=args.k)
sl = opt.cold_slices(cold[::-1], [1.0])[0]
sl.window_compact = args.form
n_blk = sl.blk_hi - sl.blk_lo
acc, reps = np.zeros(3), 0
for s in range(40):
    for x, x0 in zip(state, state0):
        x.copy_(x0)
    torch.cuda.synchronize()
    assert dbg.rsx_dbg_stamps_adam_zero() == 0
    opt.run_slice(sl)
    torch.cuda.synchronize()
    if s >= 10:
        buf = (C.c_ulonglong * 64)()
        assert dbg.rsx_dbg_stamps_adam(buf) == 0
        t = np.array(list(buf)[:3], np.float64)
        acc += (t - t[0]) * 0.01
        reps += 1
acc /= reps
print("window sweep, k = %d, form %s, %d workgroups, rows: %.0f %% idle, %.0f %% void: us since workgroup 0's entry (mean of %d "
      "launches): last exit of a first-order-vector block %.2f, last exit of a table block %.2f"
      % (args.k, "compact" if args.form else "one_pass", n_blk, 100 * args.idle, 100 * args.void, reps, acc[1], acc[2]))
