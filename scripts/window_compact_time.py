"""GPU box: the window sweep alone (k = 8, DeepFM-size state), its two forms (rsx_adam_slice.window_compact) alternating in one
process, HIP events around 20 captured launches.

    python scripts/window_compact_time.py [--idle 0.0] [--void 0.0] [--rounds 6] [--no_w1]

--idle / --void: share of the table rows whose m is all +0 with v > 0 (idle) / with v = +0 too (void), hash-scattered; the
rest are live (m, v from a seed).  0 / 0 is the all-live state a long run approaches.  The first-order vector's elements get
the same mix.  --no_w1: an arena without the first-order vector, so the sweep holds the tables' blocks only (what the
vector's blocks cost the launch is the difference)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from recsys_amd.ops import AdamTF1, EmbeddingArena
from kernel_roofline_util import criteo_row_off, synth_ids

p = argparse.ArgumentParser()
p.add_argument("--idle", type=float, default=0.0)
p.add_argument("--void", type=float, default=0.0)
p.add_argument("--rounds", type=int, default=6)
p.add_argument("--k", type=int, default=8)
p.add_argument("--no_w1", action="store_true")
args = p.parse_args()

row_off = criteo_row_off()
w1 = not args.no_w1
a = EmbeddingArena(row_off, 16, 256, "cuda", with_w1=w1, w1_field_mask=(1 << 39) - 1)
g = torch.Generator(device="cuda").manual_seed(1)
with torch.no_grad():
    a.tables.normal_(generator=g)
    a.m_t.normal_(generator=g).mul_(0.01); a.v_t.uniform_(generator=g).mul_(1e-4).add_(1e-12)
    u = torch.rand(a.m_t.shape[0], device="cuda", generator=g)
    a.m_t[u < args.idle + args.void] = 0.0
    a.v_t[u < args.void] = 0.0
    if w1:
        a.w1.normal_(generator=g)
        a.m_w.normal_(generator=g).mul_(0.01); a.v_w.uniform_(generator=g).mul_(1e-4).add_(1e-12)
        a.m_w[u < args.idle + args.void] = 0.0
        a.v_w[u < args.void] = 0.0
state = [a.m_t, a.v_t, a.tables] + ([a.m_w, a.v_w, a.w1] if w1 else [])
state0 = [x.clone() for x in state]
rng = np.random.default_rng(0)
a.sort_window([torch.from_numpy(synth_ids(rng, 256, row_off)).cuda() for _ in range(args.k)])
opt = AdamTF1(device="cuda")
cold, _ = a.adam_split_segments(window_k=args.k)
graphs = {}
for form in (0, 1):
    sl = opt.cold_slices(cold[::-1], [1.0])[0]
    sl.window_compact = form
    opt.run_slice(sl)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(20):
            opt.run_slice(sl)
    graphs[form] = (gr, sl)


def timed(form):
    # the same state for every measurement: 20 launches decay m by 0.9^160, and denormal moments take the IEEE path
    for x, x0 in zip(state, state0):
        x.copy_(x0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    graphs[form][0].replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / 20

print("window sweep alone%s, k = %d, rows: %.0f %% idle, %.0f %% void, rest live; us per launch (20 captured launches)"
      % ("" if w1 else " (tables only, --no_w1)", args.k, 100 * args.idle, 100 * args.void))
for _ in range(6):                        # (clocks and caches settle over the first ~100 launches)
    for form in (0, 1):
        timed(form)
res = {0: [], 1: []}
for r in range(args.rounds):
    for form in (0, 0, 1, 1):             # each form twice in a row: the second against the first is its own spread
        res[form].append(timed(form))
    print("round %d: one_pass %.1f %.1f   compact %.1f %.1f" % (r, res[0][-2], res[0][-1], res[1][-2], res[1][-1]))
for form, name in ((0, "one_pass"), (1, "compact")):
    x = np.array(res[form])
    print("%-8s median %.1f  min %.1f  max %.1f  (spread %.1f)" % (name, np.median(x), x.min(), x.max(), x.max() - x.min()))
