"""What the fused TRAIN steps of fm.py, deepfm.py, dcn.py and xdeepfm.py share: how a step schedules its dedup sort, its
untouched-row optimizer sweep, its gradient exchange and its optimizer launch.  Three phases around the model's own forward /
head / backward launches:

  configure()                            set-up, once per store: optimizer windows, the data-parallel send block, sweep shares
  begin() sort_ids() sort_now() split_update() local_sums()
                                         ids phase, inside the (captured) forward half; the model calls them in ITS launch order
  finish()                               optimizer phase, the step's train_op

The models differ in data only: their arenas ([arena], or [a1, a2] where a2 shares a1's sort), the column widths of their send
block, the sweep shares of their carrier launches, and where their own first launch sits between these calls.  din.py's
DinFused keeps a step of its own (its ids phase runs on a side stream over SparseTable views).
"""
import os
from dataclasses import dataclass
from typing import Any

from . import _lib
from . import layers as L
from .dist import window_global_ids
from .ops import EmbeddingArena, FusedTower


def dp_unique_wanted(store, params):
    """The data-parallel sparse exchange of this run: unique-row lists (round 5; the default from two ranks on) need the split
    TF-1 update (the optimizer launch that owns the touched rows); RSX_DP_EXCHANGE=examples: the pre-dedup per-example block of
    rounds 1-4 -- also the default at world 1 (RSX_FORCE_DIST), where there is nothing to merge and the rank-local dedup +
    segment-sum are pure overhead (through RCCL at world 1: deepfm.py 0.0790 ms against 0.0875)."""
    world = store.dp.world if store.dp is not None else 1
    default = "unique" if world > 1 else "examples"
    return os.environ.get("RSX_DP_EXCHANGE", default) == "unique" and store.adam_mode == "tf1_dense" and \
        bool(params.get("overlap_adam", True)) and params.get("dp_send_block", True)


def tower_specs(shapes, init, d, layers):
    """Adds the tower's variables dnn.{W,b,gamma,beta}{i} (glorot-uniform kernels, zero biases, BN gamma 1 / beta 0: Appendix
    A-7) for an input of width d; -> the last layer's width.  (Insertion order = the dense arena's layout and the order the
    initialisers draw from the generator.)"""
    for i, n in enumerate(layers):
        shapes[f"dnn.W{i}"], shapes[f"dnn.b{i}"] = (d, n), (n,)
        init[f"dnn.W{i}"] = lambda t, g, fi=d, fo=n: L.glorot_uniform_(t, fi, fo, g)
        init[f"dnn.b{i}"] = lambda t, g: t.zero_()
        shapes[f"dnn.gamma{i}"], init[f"dnn.gamma{i}"] = (n,), lambda t, g: t.fill_(1.0)
        shapes[f"dnn.beta{i}"], init[f"dnn.beta{i}"] = (n,), lambda t, g: t.zero_()
        d = n
    return d


def fused_tower(store, params, k0, layers, capacity):
    """The FusedTower over store.dense's dnn.* variables, or None (params tower='torch', or widths the kernels do not cover)."""
    if params.get("tower", "hip") != "hip":
        return None
    if not FusedTower.supports(k0, layers):
        print("INFO:deep_layers=%s is outside the fused tower's envelope (widths multiple of 4, last <= 256): using the "
              "autograd tower (tower='torch')" % params["deep_layers"], flush=True)
        return None
    return FusedTower(store.dense, "dnn", k0, layers, capacity, store.device)


def replica_args(dp):
    """FusedTower.train_step's replicas / seed: the loss is a mean over the global batch, replicas draw independent dropout
    patterns."""
    return dict(replicas=dp.world if dp is not None else 1, seed=0x5eed + (7919 * dp.rank if dp is not None else 0))


def configure(store, params, arenas, capacity, example_cols, unique_cols, windows, send_block, default_sweep_weights=None):
    """Set-up of a store whose TRAIN step is a fused one.  capacity: the GLOBAL batch the arenas were built for.
    windows: the step has the split TF-1 update optimizer windows need; send_block: data parallel, exchange through the
    persistent send block with these per-unit float counts -- example_cols (per example: dX of every arena, S, gy2, gy1) or
    unique_cols (per packed unique row: G of every arena, gw1).  default_sweep_weights (None: the model cuts its own): the
    share of the untouched-row sweep carried by each launch, for store.sweep_weights."""
    dp, a0 = store.dp, arenas[0]
    world = dp.world if dp is not None else 1
    want_ux = dp is not None and send_block and dp_unique_wanted(store, params) and \
        EmbeddingArena.unique_exchange_ok(a0.row_off_np, world)
    # optimizer windows (include/rsx.h rsx_adam_window): up to 8 consecutive steps share ONE sweep over the untouched rows
    # (capacity = the GLOBAL batch under data parallelism; the window's sorts are the ranks' LOCAL ones under the unique-list
    # exchange, so only the local batch has to fit the one-launch multi-sort -- dcn.py at 8 x 4 096 keeps its windows)
    if windows and (capacity // world if want_ux else capacity) <= 16384:
        store.window_k = _lib.default_adam_window(capacity, want_ux)
        store.window_dp = True
    store.graph_safe_dp = True      # the fused step issues its collectives outside autograd
    store.dp_block = False
    store.dp_unique = False
    if dp is not None and send_block:
        # zero-copy gradient exchange: the dense gradient arena and the rank's block of the sparse exchange live inside ONE
        # persistent send buffer (no pack launch before the all-gather).
        # Round 5 (default; RSX_DP_EXCHANGE=examples keeps the round-1..4 exchange of the pre-dedup per-example block): every
        # rank de-duplicates and sums ITS batch, the ranks exchange unique (row, sum) lists (EmbeddingArena.enable_unique_exchange,
        # csrc/uniq_exchange.hip) -- the send block is [dense | G [capT, D] (of every table set: one dedup serves all) | gw1 [capT]]
        if want_ux:
            ux = a0.enable_unique_exchange(world, capacity // world)
            for a in arenas[1:]:
                a.ux = ux
            dp.make_send_block(store.dense, ux.capT, unique_cols)
            store.dp_unique = True
        else:
            dp.make_send_block(store.dense, capacity // world, example_cols)
        store.dp_block = True
    if default_sweep_weights is not None:
        env = os.environ.get("RSX_SWEEP_WEIGHTS")
        store.sweep_weights = params.get("sweep_weights") or ([float(x) for x in env.split(",")] if env else
                                                              default_sweep_weights)


@dataclass
class Plan:
    """One fused TRAIN step: what the model's launches and finish() read of the ids phase."""
    store: Any
    arenas: list
    ids: Any                    # the rank's batch
    ids_sort: Any               # the batch the optimizer sees (data parallel, per-example exchange: the all-gathered ids)
    split: bool                 # exact TF-1 Adam as untouched-row sweep + touched rows (adam_mode tf1_dense, overlap_adam)
    wk: int                     # optimizer window (estimator.Window, rsx_adam_window): this step is position wpos of wk
    wpos: int                   # consecutive steps whose batches (wfeat) are known
    wfeat: Any
    ux: bool                    # data parallel: exchange of per-rank unique-row lists (round 5)
    zc: bool                    # data parallel: per-example gradient block, written in place into the send block
    job: Any = None             # the step's dedup sort while no launch has taken it (EmbeddingArena.sort_job)
    sweeps: Any = None          # slices of the untouched-row sweep for the model's carrier launches, in launch order
    last_sweep: Any = None      # the slice the optimizer launch carries
    hot: bool = False           # the step ends in ONE launch: scatter + touched-row Adam + dense Adam


def begin(store, arenas, ids, split, presort=True):
    """Opens the step.  Data parallel: the optimizer sees the GLOBAL batch (TF concatenates the replicas' IndexedSlices), so the
    dedup sort runs over the all-gathered ids -- a 40 KB collective issued FIRST (ids depend on nothing of this step), so that
    every launch from the gather to the last backward layer is one graph segment.  presort=False: the model exchanges ids
    with its gradients and sorts in train_op (it calls neither sort_ids nor split_update)."""
    dp = store.dp
    wk, wpos, wfeat = store.window_of_step()
    if wk > 1 and not split:
        raise _lib.RsxError("optimizer windows need the split TF-1 update (adam_mode=tf1_dense, overlap_adam)")
    ux = dp is not None and store.dp_unique
    zc = dp is not None and store.dp_block and not ux
    gather_ids = dp is not None and wk == 1 and not ux and presort
    ids_sort = dp.all_gather_id_list([ids], prefetchable=True)[0] if gather_ids else ids
    for a in arenas:
        a.select(wpos)
    return Plan(store, arenas, ids, ids_sort, split, wk, wpos, wfeat, ux, zc)


def sort_ids(plan):
    """The dedup of the step's (position 0: the window's) ids.  A single step's sort is left in plan.job for a launch of the
    model to carry (sort_rides) or for sort_now()."""
    a0, dp, wk = plan.arenas[0], plan.store.dp, plan.wk
    if plan.ux:
        # ids phase of the unique-list exchange: the rank's OWN dedup sorts (the window's wk batches in one launch) -> key
        # blocks -> ONE all-gather -> the global lists / slot maps / src of all wk positions (rsx_uniq_merge): 3 launches
        # and a collective per WINDOW, no global sort
        if plan.wpos == 0:
            idl = [f["ids"] for f in plan.wfeat] if wk > 1 else [plan.ids]
            a0.ux_merge(dp.all_gather_keys(a0.ux_sort_pack(idl), a0, idl), wk)
        n = a0.ux.max_unique
    elif wk > 1:
        if plan.wpos == 0:
            a0.sort_window(window_global_ids(dp, plan.wfeat))   # data-parallel: ONE all-gather for the ids of all wk local batches
        n = plan.ids.shape[0] * (dp.world if dp is not None else 1)
    else:
        plan.job = a0.sort_job(plan.ids_sort)
        n = plan.ids_sort.shape[0]
    for a in plan.arenas:
        a.last_B = n


def sort_rides(plan):
    """May another launch carry the step's sort as extra workgroups?  Larger sorts are faster with 1024 threads of their own
    (a 256-thread carrier workgroup sorts 4096 keys in 55 us, the 1024-thread kernel in 26 us).  (A side HIP stream was
    measured instead: inside a graph the fork/join across HW queues costs ~10 us each way, more than it hides.)"""
    return plan.job is not None and plan.ids_sort.shape[0] <= int(_lib.form("sort_ride_max"))


def sort_now(plan):
    """The sort no launch carries, as a launch of its own."""
    if plan.job is not None:
        plan.arenas[0].field_sort(plan.ids_sort)
        plan.job = None


def split_update(plan, weights, n_carriers):
    """Exact TF-1 Adam, split: the sort runs first (its slot map says which rows this step touches); the HBM-bound sweep over
    the UNtouched rows (old state only) then rides along in the model's launches as extra workgroups, filling the CUs the
    latency-bound tower leaves idle; touched rows + dense follow the scatter.  weights: the sweep's share per carrier launch,
    n_carriers of the model's own and optionally one more for the optimizer launch (table blocks only: each arena's
    first-order vector goes first).
    Optimizer window: ONE sweep for the whole window at position 0, as a launch of its own: k updates per row in registers make
    the slices ALU-heavy, and as riders they inherit their carrier's occupancy (measured, DeepFM bs 256: carried 164 us per
    4-step window, stand-alone 73 us = 18 us per step against 53-60 us for a one-step sweep); later positions run none."""
    if not plan.split:
        return
    plan.hot = True
    opt = plan.store.opt
    if plan.wk > 1:
        if plan.wpos == 0:
            opt.window_sweep([s for a in plan.arenas for s in a.adam_split_segments(window_k=plan.wk)[0][::-1]])
        return
    sl = opt.cold_slices([s for a in plan.arenas for s in a.adam_split_segments()[0][::-1]], weights)
    plan.last_sweep = sl[-1] if len(sl) == n_carriers + 1 else None
    plan.sweeps = sl[:n_carriers]


def local_sums(plan, grads):
    """Unique-list exchange, end of the forward half: the rank's own sorted segment-sums (what a single replica's scatter does),
    written as its block of the send buffer.  grads: per arena (S, dX, gy1, gy2)."""
    if not plan.ux:
        return
    a0 = plan.arenas[0]
    views = plan.store.dp.send_views(a0.ux.capT)
    gw1 = views[len(plan.arenas)] if len(views) > len(plan.arenas) else None
    for a, g, G in zip(plan.arenas, grads, views):
        a.ux_segsum_local(plan.ids.shape[0], *g, G, gw1 if a is a0 else None, plan.wpos)


def finish(plan, grads, riders=None, dense_segs=None, pending=None):
    """The step's train_op: gradient exchange + optimizer launch.  grads: per arena (S, dX, gy1, gy2), as for segsum_adam.
    riders: launches whose results only the optimizer reads (ops.make_scatter_riders); dense_segs: replaces the dense arena's
    segments on a single replica; pending: RSX_DP_OVERLAP's per-layer all-reduces of the dense arena, awaited here."""
    store, arenas, dp = plan.store, plan.arenas, plan.store.dp
    a0, B, window = arenas[0], plan.ids.shape[0], (plan.wk, plan.wpos)
    second = (arenas[1], grads[1][1]) if len(arenas) > 1 else None
    blocks = None
    for a in arenas:
        a.select(plan.wpos)
    if pending is not None:
        dp.wait_all(pending)
    if plan.ux:
        # ONE collective [dense | G | gw1], then the touched-row Adam off the merged lists: N looked-up rows per global
        # unique row, summed in rank order
        parts, blocks, dense_segs = dp.gather_send_block(a0.ux.capT, fold_dense=True, dense_done=pending is not None)
        gw10 = parts[len(arenas)] if len(parts) > len(arenas) else None
        a0.ux_merged_adam(parts[0], gw10, blocks[1], store.opt, dense_segs or store.dense.adam_segments(), plan.last_sweep,
                          second=second and (second[0], parts[1]), window=window)
        return
    if plan.zc:
        # ONE collective straight from the send block (dense arena + per-example block, in configure()'s example_cols order)
        parts, blocks, dense_segs = dp.gather_send_block(B, fold_dense=plan.hot, dense_done=pending is not None)
        parts = iter(parts)
        dXs = [next(parts) if g[1] is not None else None for g in grads]
        S, gy2, gy1 = (next(parts) if grads[0][i] is not None else None for i in (0, 3, 2))
        grads = [(S, dXs[0], gy1, gy2)] + [(None, dX, None, None) for dX in dXs[1:]]
        second = second and (second[0], dXs[1])
        B *= dp.world
    elif dp is not None:
        # ONE collective: per-example gradient block + dense arena (summed in rank order); the scatter then reads every
        # rank's block in place from the gathered buffer
        assert second is None
        S, dX, gy1, gy2 = grads[0]
        dX, S, gy1, gy2, blocks = dp.gather_example_grads(dX, S, gy1, gy2, dense=store.dense.grad, blocked=True)
        grads = [(S, dX, gy1, gy2)]
        B *= dp.world
    if plan.hot:        # scatter + touched-row Adam + dense Adam in ONE launch; advances the beta powers
        a0.segsum_adam(B, *grads[0], store.opt, dense_segs or store.dense.adam_segments(), plan.last_sweep, blocks=blocks,
                       second=second, window=window, riders=riders)
    else:
        for a, g in zip(arenas, grads):
            a.segsum(B, *g, blocks=blocks)
        store.apply_gradients()
