"""Estimator-shaped surface of the reference scripts on PyTorch-ROCm.

Mirrors what fm/fm.py:173-224 (and its four twins) use from `tensorflow_estimator`:
`Estimator(model_fn, model_dir, params, config)`, `.train/.evaluate/.predict`,
`train_and_evaluate(est, TrainSpec, EvalSpec)`, `RunConfig`, `EstimatorSpec`, `ModeKeys`.

Differences that are deliberate (MI355X-first):
  * model_fn runs eagerly on `cuda`; its variables live in the Estimator's `VariableStore`
    (flat HBM arenas) instead of a TF graph.
  * TRAIN mode returns `train_op` as a closure (backward + one fused Adam launch).  The Estimator
    captures `model_fn + train_op` ONCE per batch shape into a HIP graph and replays it per step,
    which removes the Python/launch overhead that dominates at batch 256.
  * MirroredStrategy (fm/fm.py:184-194) becomes one process per GPU + RCCL (recsys_amd.dist).
"""
import collections
import os
import queue
import threading
import time
from dataclasses import dataclass
from typing import Any, Callable, Dict, Optional

import numpy as np
import torch

from . import _lib
from . import metrics as _metrics
from .ops import SPARSE_OPTIMIZERS, AdamTF1, DenseArena, EmbeddingArena


class ModeKeys:
    TRAIN = "train"
    EVAL = "eval"
    PREDICT = "infer"


@dataclass
class EstimatorSpec:
    mode: str
    predictions: Optional[Dict[str, torch.Tensor]] = None
    loss: Optional[torch.Tensor] = None
    train_op: Optional[Callable[[], None]] = None
    eval_metric_ops: Optional[Dict[str, Any]] = None
    export_outputs: Optional[Dict[str, Any]] = None


@dataclass
class RunConfig:
    """estimator.RunConfig fields the scripts set (fm/fm.py:187-194)."""
    save_checkpoints_steps: Optional[int] = None
    keep_checkpoint_max: int = 5
    log_step_count_steps: int = 100
    save_summary_steps: int = 200
    train_distribute: Any = None
    eval_distribute: Any = None
    use_hip_graph: bool = True
    device: str = "cuda"
    seed: int = 0
    adam_mode: str = "tf1_dense"    # 'tf1_dense' (reference semantics) | 'lazy_rows' (NOT TF semantics)
    # 'adam' (tf.train.AdamOptimizer, adam_mode above) | 'adagrad' | 'ftrl' (tf.train.AdagradOptimizer / FtrlOptimizer:
    # ops.AdagradTF1 / FtrlTF1, sparse on the tables' unique rows); optimizer_hparams: their TF argument names
    # (initial_accumulator_value, learning_rate_power, l1_/l2_/l2_shrinkage_regularization_strength), TF's defaults
    optimizer: str = "adam"
    optimizer_hparams: Optional[Dict[str, float]] = None
    # evaluate() also reports "AUC_exact", the exact tie-aware rank statistic (metrics.ExactAUC: a device-wide key sort, one more
    # device->host copy per evaluate).  Off: every result dictionary and log line as before.  Single replica only
    exact_auc: bool = False
    # evaluate() also reports "GAUC" (+ "GAUC_groups", "GAUC_skipped_examples"): the exact AUC of every group's examples, weighted
    # by the group's examples (the DIN paper's per-user AUC; metrics.GroupAUC).  The key of an embedding column of the layout
    # (Criteo scripts, --feature_set uid_iid: e.g. "u_id") or "i_id" / "i_cate" (din.py); None: everything as before.  Single replica
    group_auc_key: Optional[str] = None
    # evaluate() also reports "ECE", "MCE", "PCOC" and "NE" from a reliability table of this many equal-width bins (0: off; 2..1024)
    # and, with calibration_key (group_auc_key's names), "GCE" and "GCE_groups" from one (count, positives, sum of p) row per id of
    # that column -- metrics.Calibration: one more launch per batch, one more device->host copy.  Both off: everything as before.
    # Single replica
    calibration_bins: int = 0
    calibration_key: Optional[str] = None
    # calibration_fit = M (2..1024; 0: off): evaluate() fits an isotonic map (metrics.IsotonicMap) from an equal-mass table of M
    # bins over this call's sorted (score, label) keys, keeps it in Estimator.last_calibration_map, writes
    # <model_dir>/calibration-<global_step>.json and reports "calibration_knots".  calibration_apply (needs calibration_bins, and a
    # map of the current global_step): evaluate() also reports "ECE_cal", "MCE_cal" and "PCOC_cal", the figures of the mapped
    # probabilities (one more launch of rsx_calibrate_apply and of the bin table per batch).  Never both in one call: the figures
    # would be in-sample.  Both off: everything as before.  Single replica
    calibration_fit: int = 0
    calibration_apply: bool = False


@dataclass
class TrainSpec:
    input_fn: Callable
    max_steps: Optional[int] = None


@dataclass
class EvalSpec:
    input_fn: Callable
    steps: Optional[int] = 100
    start_delay_secs: int = 120
    throttle_secs: int = 600


class PackedBatch:
    """(features, labels) of one batch packed into ONE contiguous byte buffer, so a training step needs a single
    host->device (or device->device) copy into the HIP graph's static input buffer instead of one per tensor."""

    _flat_layouts = {}      # (key of a FlatFeatures batch) -> (layout, nbytes): batches of one stream share them

    def __init__(self, features, labels, device=None, pin=False):
        dev_flat = getattr(features, "dev_flat", None)
        if isinstance(dev_flat, torch.Tensor) and dev_flat.is_cuda and device is None and not pin:
            # the device-parse stream wrote the batch on the device in this packing (input_pipeline.DeviceFeatures): adopt its
            # buffer.  It was allocated on the producer's stream: tell the allocator which stream reads it from here on.
            ids = features.get("ids")
            if len(features) == 1 and isinstance(ids, torch.Tensor) and isinstance(labels, torch.Tensor) and \
                    ids.dtype == torch.int32 and labels.dtype == torch.float32 and labels.data_ptr() == dev_flat.data_ptr():
                o_ids = (labels.numel() * 4 + 15) & ~15
                nb_ids = ids.numel() * 4
                if ids.data_ptr() == dev_flat.data_ptr() + o_ids and dev_flat.numel() == (o_ids + nb_ids + 15) & ~15 and \
                        ids.is_contiguous() and labels.is_contiguous():
                    self.layout = [("__label__", labels.dtype, tuple(labels.shape), 0, labels.numel() * 4),
                                   ("ids", ids.dtype, tuple(ids.shape), o_ids, nb_ids)]
                    self.nbytes = dev_flat.numel()
                    self.flat = dev_flat
                    dev_flat.record_stream(torch.cuda.current_stream(dev_flat.device))
                    return
        flat_np = getattr(features, "flat", None)
        if flat_np is not None and device is None and not pin:
            # the input pipeline's reader already assembled the batch in this packing (input_pipeline.FlatFeatures): O(1)
            pkey = features.pack_key
            hit = PackedBatch._flat_layouts.get(pkey)
            if hit is not None and hit[1] == flat_np.nbytes and labels.shape[0] == hit[0][0][2][0] and \
                    labels.__array_interface__["data"][0] == flat_np.__array_interface__["data"][0]:
                self.layout, self.nbytes = hit
                self.flat = torch.from_numpy(flat_np)
                return
        items = [("__label__", labels)] + sorted(features.items())
        self.layout, off = [], 0
        arrs = []
        for k, v in items:
            t = torch.as_tensor(v).contiguous()
            nb = t.numel() * t.element_size()
            self.layout.append((k, t.dtype, tuple(t.shape), off, nb))
            arrs.append(t)
            off = (off + nb + 15) & ~15
        self.nbytes = off
        flat = self._adopt(items) if (device is None and not pin) else None
        if flat is not None and flat_np is not None and flat.data_ptr() == flat_np.ctypes.data and off == flat_np.nbytes:
            PackedBatch._flat_layouts[pkey] = (self.layout, self.nbytes)      # the next batch of this stream skips all of this
        if flat is None:
            # plain memcpy through numpy views (torch's CPU copy_ of > 32 KB wakes its thread pool: ~0.4 ms per part when the
            # pool is asleep, which it is between two batches)
            buf = np.zeros(off, np.uint8)
            for (k, dt, sh, o, nb), t in zip(self.layout, arrs):
                if nb:
                    buf[o:o + nb] = t.cpu().reshape(-1).view(torch.uint8).numpy()
            flat = torch.from_numpy(buf)
        if pin and torch.cuda.is_available():
            flat = flat.pin_memory()
        self.flat = flat if device is None else flat.to(device)

    def _adopt(self, items):
        """Zero-copy: the input pipeline's C++ reader assembles every batch in ONE flat host buffer laid out exactly like
        this packing (input_pipeline._criteo_batches: label | cont_log | ids, 16-byte aligned parts); when the arrays handed
        in are views of such a buffer at the packing's own offsets, wrap it instead of copying 40 KB per step."""
        arrays = [v for _, v in items]
        if not all(isinstance(v, np.ndarray) for v in arrays):
            return None
        root = arrays[0]
        while isinstance(root.base, np.ndarray):
            root = root.base
        if root.dtype != np.uint8 or root.ndim != 1 or not root.flags["C_CONTIGUOUS"]:
            return None
        p0 = arrays[0].ctypes.data
        off0 = p0 - root.ctypes.data
        if off0 < 0 or off0 + self.nbytes > root.nbytes or (p0 & 15):
            return None
        for (k, dt, sh, o, nb), v in zip(self.layout, arrays):
            if not v.flags["C_CONTIGUOUS"] or (nb and v.ctypes.data - p0 != o):
                return None
        return torch.from_numpy(root[off0:off0 + self.nbytes])

    def key(self):
        return tuple((k, str(dt), sh) for k, dt, sh, _, _ in self.layout)

    def over(self, flat):
        """This batch's packing over another buffer."""
        o = PackedBatch.__new__(PackedBatch)
        o.layout, o.nbytes, o.flat = self.layout, self.nbytes, flat
        return o

    def to(self, device):
        return self.over(self.flat.to(device, non_blocking=True))

    def clone(self):
        return self.over(self.flat.clone())

    def views(self):
        feats, labels = {}, None
        for k, dt, sh, o, nb in self.layout:
            v = self.flat[o:o + nb].view(dt).view(sh)
            if k == "__label__":
                labels = v
            else:
                feats[k] = v
        return feats, labels


class LazyMeanLoss:
    """A TRAIN step's mean loss that nobody has asked for yet: the per-example terms sit in a device buffer (column `col` of
    `terms` [n, stride], written by the step's kernels) and are summed when the value is read -- float(), .item(), .tensor().
    The Estimator only touches a step's loss at log lines, so a step that would need a launch of its own just to reduce 256
    numbers (fm.py's fused forward + head, csrc/embedding.hip gather_fm_head_k) does not pay for it."""

    def __init__(self, terms, col, n):
        self.terms, self.col, self.n = terms, int(col), int(n)       # n = examples (the rows may be pre-added groups)

    def detach(self):
        return self

    def tensor(self):
        return (self.terms[:, self.col].double().sum() / self.n).to(torch.float32)

    def clone(self):
        return self.tensor()

    def reshape(self, *shape):
        return self.tensor().reshape(*shape)

    def item(self):
        return float(self.tensor().item())

    def __float__(self):
        return self.item()

    def __format__(self, spec):
        return format(float(self), spec)


class VariableStore:
    """The variables of one model: named embedding arenas + one flat dense arena + the optimizer."""

    def __init__(self, device, seed, adam_mode, optimizer="adam", optimizer_hparams=None):
        if optimizer != "adam" and optimizer not in SPARSE_OPTIMIZERS:
            raise ValueError("optimizer must be one of adam, %s; got %r" % (", ".join(sorted(SPARSE_OPTIMIZERS)), optimizer))
        self.device = torch.device(device)
        self.embeddings: Dict[str, EmbeddingArena] = {}
        self.dense: Optional[DenseArena] = None
        self.opt: Optional[AdamTF1] = None
        self.built = False
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(seed)
        # The one predicate of the model code: every fused-Adam branch (the split TF-1 sweep, optimizer windows, the cold-sweep
        # slices, the segment-sum fused with Adam) tests adam_mode == "tf1_dense".  Under another optimizer it is "off", so
        # none of them runs and the steps end in segsum + apply_gradients (rsx_sparse_opt_multi).
        self.optimizer = optimizer
        self.optimizer_hparams = dict(optimizer_hparams or {})
        self.adam_mode = adam_mode if optimizer == "adam" else "off"
        self.extra_segments = []     # model-specific optimizer segments (e.g. DIN tables)
        self.dp = None               # recsys_amd.dist.DataParallel when training data-parallel
        self.graph_safe_dp = False   # set by model code whose DP collectives run outside autograd (segmentable)
        self.dp_unique = False       # data parallel: the sparse exchange carries per-rank unique-row lists (dist.py, round 5)
        # Optimizer window (include/rsx.h rsx_adam_window): window_k = the longest run of consecutive TRAIN steps the
        # model's fused step can treat as one window (set by model code; 1 = every step on its own); `window` =
        # (k, position, [features of the k batches]) while the Estimator runs a step that belongs to one.
        self.window_k = 1
        self.window = None
        self.window_dp = False       # set by model code whose fused step supports optimizer windows under data parallelism
        self.window_broken = False   # an exception interrupted a window (Estimator._train_window): the variables are poisoned

    def window_of_step(self):
        """-> (k, position, features of the window's batches) of the TRAIN step being built; (1, 0, None) without a window."""
        return self.window if self.window is not None else (1, 0, None)

    def build(self, embeddings: Dict[str, EmbeddingArena], dense_shapes, dense_init, lr, storage_shapes=None):
        self.embeddings = embeddings
        self.dense = DenseArena(dense_shapes, self.device, storage_shapes)
        with torch.no_grad():
            for k, fn in dense_init.items():
                t = torch.empty(tuple(dense_shapes[k]))
                fn(t, self.gen)
                self.dense[k].copy_(t)
        if self.optimizer == "adam":
            self.opt = AdamTF1(lr=lr, device=self.device)
        else:
            if self.dp is not None:
                raise _lib.RsxError("optimizer=%r: data-parallel training supports optimizer='adam' only" % self.optimizer)
            if self.extra_segments:
                raise _lib.RsxError("optimizer=%r: this model's variables have no sparse-optimizer segments" % self.optimizer)
            self.opt = SPARSE_OPTIMIZERS[self.optimizer](lr=lr, device=self.device, **self.optimizer_hparams)
            acc0 = self.opt.initial_accumulator_value
            with torch.no_grad():           # every accumulator slot starts at initial_accumulator_value (TF's slot init)
                for a in embeddings.values():
                    a.v_t.fill_(acc0)
                    if a.with_w1:
                        a.v_w.fill_(acc0)
                self.dense.v.fill_(acc0)
        self.built = True

    def adam_segments(self):
        lazy = self.adam_mode == "lazy_rows"
        segs = []
        for a in self.embeddings.values():
            segs += a.adam_segments(lazy)
        segs += self.extra_segments
        segs += self.dense.adam_segments()
        return segs

    def sort_ids_for_backward(self, arena, ids):
        """Dedup stage of the sparse gradient (ids only).  Data-parallel: over the all-gathered global batch.  (The fused
        TRAIN steps do not call this: their sort rides in the first tower launch.)"""
        if self.dp is not None:
            ids = self.dp.all_gather_rows(ids)
        arena.field_sort(ids)

    def minimize(self, loss):
        """optimizer.minimize(loss) (fm/fm.py:162-163) incl. MirroredStrategy's 1/N loss scaling and
        cross-replica gradient sum (Appendix A-12)."""
        if self.dp is not None:
            (loss / self.dp.world).backward()
            self.dp.all_reduce_sum(self.dense.grad)
        else:
            loss.backward()
        self.apply_gradients()

    def sparse_opt_segments(self):
        segs = []
        for a in self.embeddings.values():
            segs += a.sparse_opt_segments()
        return segs + self.dense.adam_segments()

    def apply_gradients(self):
        if self.optimizer != "adam":
            self.opt.step(self.sparse_opt_segments())
            return
        self.opt.step(self.adam_segments())

    # -- checkpoint -------------------------------------------------------
    def state_dict(self):
        sd = {"opt_state": self.opt.state.cpu(), "dense": {k: getattr(self.dense, k).cpu() for k in ("flat", "m", "v")}}
        if self.optimizer != "adam":        # (no tag: Adam -- what every checkpoint written before the tag existed holds)
            sd["optimizer"] = {"name": self.optimizer, "hparams": dict(self.opt.hparams)}
        for name, a in self.embeddings.items():
            sd["emb." + name] = {k: getattr(a, k).cpu() for k in ("tables", "m_t", "v_t", "w1", "m_w", "v_w", "table", "m", "v")
                                 if getattr(a, k, None) is not None}
        return sd

    def load_state_dict(self, sd):
        tag = sd.get("optimizer") or {"name": "adam"}
        if tag["name"] != self.optimizer:
            raise _lib.RsxError("checkpoint was written by optimizer=%r (%s); this run uses optimizer=%r -- the slots do not carry "
                                "over" % (tag["name"], tag.get("hparams", {}), self.optimizer))
        with torch.no_grad():
            self.opt.state[:4].copy_(sd["opt_state"][:4])      # (beta powers, ticket, step; the arrival counters stay zero)
            for k in ("flat", "m", "v"):
                getattr(self.dense, k).copy_(sd["dense"][k])
            for name, a in self.embeddings.items():
                for k, v in sd["emb." + name].items():
                    getattr(a, k).copy_(v)


_CURRENT_STORE = []


def get_variable_store() -> VariableStore:
    """What tf.get_variable's implicit graph is to the reference: the calling Estimator's store."""
    if not _CURRENT_STORE:
        raise RuntimeError("model_fn must be called by an Estimator (no active VariableStore)")
    return _CURRENT_STORE[-1]


# -- the records of Estimator._graphs (key[0] names the kind) ---------------------------------------------------------------
class StepGraph:
    """One step over static inputs ("packed", "infer" and the dict-input keys): `warm` eager runs, then the batch is cloned into
    static inputs and captured, afterwards every batch is loaded into them and the graph replayed.  load(static, *batch);
    eager(*batch) -> the step's result; capture(*batch) -> (static inputs holding the batch, replayable, static outputs)."""
    __slots__ = ("warm", "static", "graph", "out", "_load", "_eager", "_capture")

    def __init__(self, warm, load, eager, capture):
        self.warm, self.static, self.graph, self.out = warm, None, None, None     # warm: eager runs still to do
        self._load, self._eager, self._capture = load, eager, capture

    def run(self, *batch):
        if self.graph is not None:
            self._load(self.static, *batch)
            self.graph.replay()
            return self.out
        if self.warm > 0:                 # eager (lazy initialisation, allocator warm-up)
            self.warm -= 1
            return self._eager(*batch)
        self.static, self.graph, self.out = self._capture(*batch)
        self.graph.replay()               # capture executes nothing: the static inputs already hold this batch, so replay once
        return self.out


class StagingRing:
    """Pinned staging buffers of one size that take turns (Estimator._h2d), each with the event of the copy that last read it."""
    __slots__ = ("bufs", "np", "evs", "used", "i")

    def __init__(self, nbytes, R):
        self.bufs = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(R)]
        self.np = [b.numpy() for b in self.bufs]
        self.evs = [torch.cuda.Event() for _ in range(R)]
        self.used, self.i = [False] * R, 0

    def copy(self, dst, src):
        i = self.i
        self.i = (i + 1) % len(self.bufs)
        if self.used[i]:
            self.evs[i].synchronize()          # the copy that last read this staging buffer has run (long ago)
        np.copyto(self.np[i], src.numpy())     # (a plain memcpy: torch's CPU copy_ of > 32 KB wakes its thread pool, ~0.4 ms)
        dst.copy_(self.bufs[i], non_blocking=True)
        self.evs[i].record()
        self.used[i] = True


class StagedWindow:
    """One captured instance of a streaming window (Estimator._train_window_packed): its static inputs (slices of ONE device
    allocation), for host batches the pinned staging buffer the graph's first node fetches them from, the graph and the static
    loss of every step.  `free` / `done`: the launch that last used the instance has been issued / has run on the GPU."""
    __slots__ = ("all", "stride", "static", "pin", "pin_np", "graph", "losses", "done", "free")

    def __init__(self, dev, host):
        self.stride = stride = (dev[0].nbytes + 255) & ~255
        self.done, self.free = torch.cuda.Event(), threading.Event()
        self.free.set()
        self.all = torch.empty(len(dev) * stride, dtype=torch.uint8, device=dev[0].flat.device)
        self.static = []
        for i, pb in enumerate(dev):
            self.static.append(pb.over(self.all[i * stride:i * stride + pb.nbytes]))
            self.static[i].flat.copy_(pb.flat)
        self.pin = self.pin_np = self.graph = self.losses = None
        if host:
            self.pin = torch.empty(len(dev) * stride, dtype=torch.uint8).pin_memory()
            self.pin_np = self.pin.numpy()
            self.pin.copy_(self.all)    # (the staging buffer starts as this window's batches: the graph's first node reads it)
            torch.cuda.synchronize()

    def fetch(self):
        """The captured window's first node: staging buffer -> static inputs.  The kernel reads the pinned buffer through the
        device's mapping of host memory, right after plain host stores: that needs coherent (fine-grained) pinned allocations,
        torch's default.  RSX_WINDOW_STAGE=memcpy (automatic under HIP_HOST_COHERENT=0) makes the node a hipMemcpyAsync
        instead (0.0696 vs 0.0680 ms per DeepFM step)."""
        if _lib.form("window_stage") == "memcpy" or os.environ.get("HIP_HOST_COHERENT", "1") == "0":
            self.all.copy_(self.pin, non_blocking=True)
        else:
            _lib.check(_lib.lib().rsx_copy_bytes(self.all.data_ptr(), self.pin.data_ptr(), self.all.numel(),
                                                 torch.cuda.current_stream().cuda_stream), "rsx_copy_bytes")

    def stage(self, pbs):
        """Host half of a window (the training thread): the staging buffer <- the window's batches."""
        self.free.wait()                   # the launch that last used this instance has been issued (and `done` recorded)
        self.free.clear()
        self.done.synchronize()            # ... and the GPU has finished it (two windows ago): its first node read the buffer
        stride, pin = self.stride, self.pin_np
        for i, pb in enumerate(pbs):       # (plain memcpys: torch's CPU copy_ of > 32 KB wakes its thread pool, ~0.4 ms)
            np.copyto(pin[i * stride:i * stride + pb.nbytes], pb.flat.numpy())

    def launch(self):
        """Device half of a window (the launch thread, or in line): ONE graph replay -- staged batches in, all steps -> loss of
        the last step."""
        self.graph.replay()
        self.done.record()
        self.free.set()
        return self.losses[-1]


class WindowSets:
    """The "packedwin" entry of one window signature: `warm` eager windows still to run, then the StagedWindow instances that
    take turns (sets[0] is the next one; the deque is rotated when it is taken)."""
    __slots__ = ("warm", "sets")

    def __init__(self):
        self.warm, self.sets = 1, collections.deque()


class ResidentPlan:
    """The graphs of train_resident over ONE list of resident batches, which they read in place: the plan keeps the batches
    alive, and a list that differs in any batch has a plan of its own.  `graphs`: (first, count) -> (graph, static loss of its
    last step), the groups, heads and tails of resident_schedule.  Data parallel with eager collectives ("resident-dp"):
    `steps` = one (segmented step, loss) per batch, `graphs`: first -> (segmented window of K steps, losses)."""
    __slots__ = ("batches", "spg", "warm", "loss", "graphs", "steps", "K")

    def __init__(self, batches, spg):
        self.batches, self.spg, self.graphs, self.steps, self.K = tuple(batches), spg, {}, None, 0
        self.warm, self.loss = 2, None         # eager warm-up steps still to run; the loss of the last step run


def resident_schedule(start, steps, n, spg):
    """`steps` steps over n resident batches in order, from batch start % n, in graphs of spg steps -> [(first, count, kind)]:
    a "head" up to the next group boundary (first call: the two eager warm-up steps leave the stream at batch 2), the full
    "group"s, then ONE "tail" holding the remaining (< spg) steps."""
    sched, pos, left = [], start % n, steps
    if pos % spg and left > 0:
        cnt = min(spg - pos % spg, left)
        sched.append((pos, cnt, "head"))
        pos, left = (pos + cnt) % n, left - cnt
    while left >= spg:
        if spg < left < spg + spg // 2 and pos + left <= n:
            # a full group + a short tail (20 steps at 16 per graph): ONE graph for both -- a graph launch costs ~9 us of
            # start-up and ~8 us at its end on this stack
            sched.append((pos, left, "tail"))
            return sched
        sched.append((pos, spg, "group"))
        pos, left = (pos + spg) % n, left - spg
    if left:
        sched.append((pos, left, "tail"))
    return sched


def window_lengths(count, K):
    """The optimizer windows (<= K steps each) of a graph of `count` steps, as EVEN as possible, longest first (20 steps: 7 + 7
    + 6 rather than 8 + 8 + 4: a window's ONE sweep costs 57 us + ~3 us per step, so short windows are the dear ones)."""
    out = []
    for nwin in range(-(-count // K), 0, -1):
        out.append(-(-count // nwin))
        count -= out[-1]
    return out


class Estimator:
    MAX_INFER_GRAPHS = 32      # EVAL / PREDICT input signatures that get a captured graph (and an entry in _graphs) at most

    def __init__(self, model_fn, model_dir=None, params=None, config: Optional[RunConfig] = None):
        self._n_infer_graphs = 0
        self.last_calibration = None      # the latest evaluate()'s full metrics.Calibration result (table, records), if asked for
        self.last_calibration_map = None  # the metrics.IsotonicMap the latest evaluate() with calibration_fit fitted (table, ece)
        self.model_fn = model_fn
        self.model_dir = model_dir
        self.params = dict(params or {})
        self.config = config or RunConfig()
        self.store = VariableStore(self.config.device, self.config.seed, self.config.adam_mode, self.config.optimizer,
                                   self.config.optimizer_hparams)
        if self.config.optimizer != "adam" and int(self.params.get("adam_window", 0) or 0) > 1:
            raise _lib.RsxError("adam_window=%d: optimizer windows exist for optimizer='adam' only (got optimizer=%r)"
                                % (int(self.params["adam_window"]), self.config.optimizer))
        self._graphs = {}
        self._ring = {}        # pinned staging buffers for host batches (see _h2d)
        # captured instances of a streaming window that take turns (_train_window_packed): window w + 1 is staged into the
        # other instance while window w is queued or running (3 measured the same as 2: the stream is GPU-bound)
        self._window_sets = max(2, int(_lib.form("window_sets")))
        self._restored = False
        self._log_t = None
        self.dist = None       # recsys_amd.dist.DataParallel, set by attach_distributed()

    # -- plumbing ----------------------------------------------------------------------------
    def _call_model_fn(self, features, labels, mode):
        _CURRENT_STORE.append(self.store)
        try:
            return self.model_fn(features, labels, mode, self.params)
        finally:
            _CURRENT_STORE.pop()

    def _to_device(self, x):
        dev = self.store.device
        if isinstance(x, dict):
            return {k: self._to_device(v) for k, v in x.items()}
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        if isinstance(x, torch.Tensor):
            return x.to(dev, non_blocking=True)
        return x

    def _train_eager(self, features, labels):
        spec = self._call_model_fn(features, labels, ModeKeys.TRAIN)
        spec.train_op()
        # detach: a live loss would keep this step's autograd graph (and its AccumulateGrad nodes, bound to
        # this stream) alive into the next step, which breaks HIP-graph capture on the capture stream
        return spec.loss.detach()

    def _train_window(self, batches):
        """len(batches) consecutive TRAIN steps as ONE optimizer window: the model's fused step sorts the ids of all of
        them at the first step and sweeps the untouched rows of the optimizer state once for the whole window.  After the
        last step the variables equal those of len(batches) single steps bit for bit; between two steps of a window they
        are not a state any single-step run passes through, so nothing else (evaluate, checkpoint) may run in between.
        -> the loss of every step."""
        k = len(batches)
        feats = [f for f, _ in batches]
        losses = []
        for pos, (f, l) in enumerate(batches):
            self.store.window = (k, pos, feats) if k > 1 else None
            try:
                losses.append(self._train_eager(f, l))
            except BaseException:
                if k > 1:
                    # the rows no step of the window touches are already k steps ahead, the touched ones and global_step only
                    # `pos`: not a state any run passes through.  Poison the store: evaluate / predict / checkpoint refuse.
                    self.store.window_broken = True
                raise
            finally:
                self.store.window = None
        return losses

    def _check_consistent(self, what):
        if self.store.window_broken:
            raise _lib.RsxError("Estimator.%s: an optimizer window was interrupted by an exception; the variables are between two "
                           "window boundaries (untouched rows ahead of the touched ones).  Restore from a checkpoint." % what)

    def _window_len(self):
        """Steps per optimizer window: what the model supports (store.window_k), RSX_ADAM_WINDOW overrides (1 = off)."""
        if not self.store.built or (self.store.dp is not None and not self.store.window_dp):
            return 1
        k = int(os.environ.get("RSX_ADAM_WINDOW", self.params.get("adam_window", self.store.window_k)))
        return max(1, min(k, self.store.window_k))

    def _dp_capture(self):
        from .dist import dp_capture
        return dp_capture(self.store.dp)

    def _use_graph(self):
        """HIP graphs are on unless the step has data-parallel collectives issued from inside autograd's backward
        (worker thread: the capture cannot be segmented there); RSX_DP_CAPTURE=1 captures the collectives too."""
        if not self.config.use_hip_graph:
            return False
        return self.store.dp is None or self.store.graph_safe_dp or self._dp_capture()

    def _capture(self, fn, segment=True):
        """-> (replayable, fn's result).  Data-parallel steps become graph segments with eager RCCL calls between
        them (dist.SegmentedGraph); single-process steps one HIP graph, and so does an fn without collectives (segment=False)."""
        torch.cuda.synchronize()
        if segment and self.store.dp is not None and not self._dp_capture():
            from .dist import SegmentedGraph
            seg = SegmentedGraph()
            return seg, seg.capture(fn)
        graph = torch.cuda.CUDAGraph()
        # (data parallel with captured collectives: "thread_local" lets ProcessGroupNCCL's watchdog thread poll its events
        # while THIS thread captures -- see dist.SegmentedGraph._begin)
        kw = {"capture_error_mode": "thread_local"} if self.store.dp is not None else {}
        with _lib.capture_gc_guard(), torch.cuda.graph(graph, **kw):
            out = fn()
        return graph, out

    def _capture_step(self, features, labels):
        """The TRAIN step over static input tensors -> (replayable, static loss).  Data-parallel steps whose train_op is
        plain kernel calls (store.graph_safe_dp): only model_fn is captured; train_op -- pack, the gradient all-gather, 2-3
        launches -- is re-issued eagerly on every replay.  A graph launch costs ~9 us of start-up and ~8 us before the next
        un-captured operation begins (measured through RCCL at world 1): a graph around so few launches loses more than it saves."""
        if self.store.dp is not None and self.store.graph_safe_dp and not self._dp_capture() and \
                _lib.form("dp_eager_tail") == "1":
            seg, spec = self._capture(lambda: self._call_model_fn(features, labels, ModeKeys.TRAIN))
            seg.items.append(spec.train_op)      # re-executed (eagerly) by every replay, after the captured segments
            return seg, spec.loss.detach()
        return self._capture(lambda: self._train_eager(features, labels))

    def _shape_key(self, features, labels):
        return tuple(sorted((k, tuple(v.shape), str(v.dtype)) for k, v in features.items())) + (tuple(labels.shape),)

    def _train_step(self, features, labels=None):
        """One global step; captured into a HIP graph per input signature after 2 eager warm-up steps.
        `features` may be a PackedBatch (then one copy feeds the graph's static input buffer)."""
        if isinstance(features, PackedBatch):
            return self._train_step_packed(features)
        if not self._use_graph():
            return self._train_eager(features, labels)
        key = self._shape_key(features, labels)
        g = self._graphs.get(key)
        if g is None:
            def load(static, features, labels):          # one copy per tensor
                for k, v in features.items():
                    static[0][k].copy_(v, non_blocking=True)
                static[1].copy_(labels, non_blocking=True)

            def capture(features, labels):
                static = {k: v.clone() for k, v in features.items()}, labels.clone()
                return (static,) + self._capture_step(*static)

            g = self._graphs[key] = StepGraph(2, load, self._train_eager, capture)
        return g.run(features, labels)

    def _on_device(self, pb):
        return pb if pb.flat.device == self.store.device else pb.to(self.store.device)

    def _h2d(self, static, pb):
        """One batch -> the graph's static input buffer, ONE copy.  A pageable host batch (what an input pipeline hands over)
        goes through a ring of pinned staging buffers first: the H2D copy of pageable memory is synchronous -- the host would
        wait for the GPU to finish the previous window before it could even start packing the next one (measured end to end
        over TFRecord shards: 185 us per DeepFM step against 70 us of GPU time)."""
        src = pb.flat
        if src.device.type == "cpu" and not src.is_pinned() and torch.cuda.is_available():
            ring = self._ring.get(pb.nbytes)
            if ring is None:
                ring = self._ring[pb.nbytes] = StagingRing(pb.nbytes, 4 * max(2, self.store.window_k))
            ring.copy(static.flat, src)
            return
        static.flat.copy_(src, non_blocking=True)

    def _train_step_packed(self, pb):
        if not self._use_graph():
            if pb.flat.device != self.store.device:      # (in line: this is the eager step's timed path)
                pb = pb.to(self.store.device)
            return self._train_eager(*pb.views())
        key = ("packed",) + pb.key()
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = self._packed_step(2, self._train_eager, self._capture_step)
        return g.run(pb)

    def _packed_step(self, warm, eager, capture):
        """A StepGraph over ONE packed static buffer, loaded by ONE copy per batch, host or device (_h2d).  eager(features, labels)
        runs a batch as it is; capture(features, labels) -> (replayable, static outputs) over the views of the static buffer."""
        def clone_and_capture(pb):
            static = self._on_device(pb).clone()
            return (static,) + capture(*static.views())

        return StepGraph(warm, self._h2d, lambda pb: eager(*self._on_device(pb).views()), clone_and_capture)

    def train_resident(self, batches, steps, steps_per_graph=8):
        """Train `steps` steps over a list of HBM-resident PackedBatch objects (cycled in order).  Groups of
        `steps_per_graph` consecutive batches are captured into ONE HIP graph each that reads the resident
        buffers directly: no per-step input copy and one graph launch per group ("capture launch-bound inner
        loops in hipGraphs").  An input pipeline refills the buffers in place between replays."""
        n = len(batches)
        if self._use_graph() and self.store.dp is not None and not self._dp_capture():
            # data-parallel with eager collectives: one segmented step per RESIDENT batch, reading its buffer in place
            # (no per-step input copy); steps cannot be grouped because the collectives sit between the segments
            key = ("resident-dp",) + tuple(map(id, batches))
            g = self._graphs.get(key)
            done = 0
            if g is None:
                for s in range(min(2, steps)):
                    self._train_eager(*batches[s % n].views())
                done = min(2, steps)
                g = ResidentPlan(batches, 0)
                g.steps = [self._capture_step(*b.views()) for b in batches]
                # optimizer windows (model code that supports them under data parallelism sets store.window_dp): K consecutive
                # resident batches as ONE segmented capture -- the ids of all K batches are all-gathered at its start
                K = self._window_len()
                if K > 1 and n % K == 0:
                    for i in range(0, n, K):
                        g.graphs[i] = self._capture(
                            lambda i=i: self._train_window([batches[i + j].views() for j in range(K)]))
                    g.K = K
                self._graphs[key] = g
            loss = None
            s = done
            K = g.K
            while s < steps:
                if K and (s % n) % K == 0 and steps - s >= K:
                    seg, losses = g.graphs[s % n]
                    seg.replay()
                    loss = losses[-1]
                    s += K
                    continue
                seg, loss = g.steps[s % n]
                # RSX_DP_PREFETCH=1: the next batch's ids all-gather is issued underneath this step (not after the last one:
                # nothing would consume it before the buffers may be refilled).  Off by default: through RCCL at world 1 the
                # async launch + stream hand-over costs 7 us more than it hides; whether real xGMI latency reverses that can
                # only be measured on a multi-GPU node.
                nxt = g.steps[(s + 1) % n][0] if (s + 1 < steps and _lib.form("dp_prefetch") == "1") else None
                seg.replay(nxt)
                s += 1
            return loss if loss is not None else g.steps[0][1]
        g = self._resident_plan(batches, steps_per_graph)
        if g is None:
            for s in range(steps):
                loss = self._train_step(batches[s % n])
            return loss
        done = 0
        while g.warm > 0 and done < steps:                     # eager warm-up (allocator, lazy init), first call only
            g.loss = self._train_eager(*batches[done % n].views())
            g.warm -= 1
            done += 1
        # Every graph is captured before anything is replayed, and a caller that times this function calls prepare_resident()
        # first, so no capture ever falls inside a timed region.
        for graph, loss in self._resident_schedule(g, done, steps - done):
            graph.replay()
            g.loss = loss
        return g.loss

    def _resident_plan(self, batches, spg):
        """-> the ResidentPlan of exactly these batches in this order, None where train_resident runs them step by step.  (The
        key holds every batch's id and the plan every batch, so equal ids are the same live objects.)
        Data parallel with captured collectives (dist.dp_capture, the default over RCCL) plans like a single process: they sit
        in the groups' graphs like any other launch."""
        dp_eager = self.store.dp is not None and not self._dp_capture()
        if not self._use_graph() or spg <= 1 or len(batches) % spg != 0 or dp_eager:
            return None
        key = ("resident", spg) + tuple(map(id, batches))
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = ResidentPlan(batches, spg)
        return g

    def _resident_schedule(self, g, start, steps):
        """-> the (graph, static loss of its last step) of every entry of resident_schedule, captured where the plan does not
        hold it yet.  Optimizer windows never cross a graph: the resident batches ARE the look-ahead."""
        def steps_of(first, count):
            for w in window_lengths(count, self._window_len()):
                loss = self._train_window([g.batches[first + j].views() for j in range(w)])[-1]
                first += w
            return loss

        sched = []
        for first, count, _ in resident_schedule(start, steps, len(g.batches), g.spg):
            if (first, count) not in g.graphs:
                g.graphs[(first, count)] = self._capture(lambda: steps_of(first, count))
            sched.append(g.graphs[(first, count)])
        return sched

    def prepare_resident(self, batches, steps, steps_per_graph=8):
        """Capture every HIP graph train_resident(batches, steps, steps_per_graph) will replay, so that a timed region
        afterwards is pure replay.  Capturing itself executes nothing -- but when the resident graphs are still cold this runs
        the TWO eager warm-up training steps first (lazy initialisation, allocator warm-up): real optimizer steps."""
        g = self._resident_plan(batches, steps_per_graph)
        if g is None:
            return
        if g.warm > 0:
            self.train_resident(batches, 2, steps_per_graph)       # the two eager warm-up steps
        self._resident_schedule(g, 0, steps)

    def _maybe_restore(self):
        if self._restored or not self.model_dir or not self.store.built:
            return
        self._restored = True
        from . import checkpoint
        checkpoint.restore_latest(self.model_dir, self.store)

    @property
    def global_step(self):
        return self.store.opt.global_step if self.store.built else 0

    # -- public API --------------------------------------------------------------------------
    def _train_window_packed(self, pbs, launcher=None):
        """One optimizer window over len(pbs) host (or device) batches -> loss of the last step: ONE graph replay.
        Host batches are memcpy'ed into one pinned staging buffer, and the captured window's FIRST NODE is a kernel that
        fetches that buffer into the window's static inputs (slices of one device allocation; csrc/embedding.hip
        rsx_copy_bytes), so that a window is one hipGraphLaunch (22-45 us of host time) and nothing else on the stream.
        Measured before it (ms per DeepFM step, bench.py --host_input, unprofiled): one hipMemcpyAsync per batch on a copy
        stream + two events per window 0.0786, one copy per window on the copy stream 0.0749, the same copy in line 0.0696,
        the kernel node 0.0680 (resident batches: 0.0655).  Two captured instances of the window (each with its own inputs
        and staging buffer) take turns, so that window w + 1 is staged while window w is queued or running.
        launcher (Estimator.train, opt-in): the replay is handed to the launch thread; -> None (the loss is the launch's)."""
        host = all(pb.flat.device.type == "cpu" for pb in pbs)
        key = ("packedwin", len(pbs), host) + pbs[0].key()
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = WindowSets()
        if len(g.sets) == self._window_sets:
            st = g.sets[0]
            g.sets.rotate(-1)
            if host:
                st.stage(pbs)
                if launcher is not None:
                    launcher.submit(st.launch)
                    return None
                return st.launch()
            if launcher is not None:
                launcher.drain()
            for sb, pb in zip(st.static, pbs):             # device-resident batches: one D2D copy each, in stream order
                self._h2d(sb, pb)
            st.graph.replay()
            return st.losses[-1]
        if launcher is not None:
            launcher.drain()
        dev =[self._on_device(pb) for pb in pbs]
        if g.warm > 0:
            g.warm -= 1
            return self._train_window([pb.views() for pb in dev])[-1]
        st = StagedWindow(dev, host)

        def window():
            if host:                    # first node: the staged batches, fetched from pinned host memory
                st.fetch()
            return self._train_window([sb.views() for sb in st.static])

        st.graph, st.losses = self._capture(window)
        st.graph.replay()               # capture executes nothing: the inputs already hold this window's batches
        st.done.record(torch.cuda.current_stream())
        g.sets.append(st)
        return st.losses[-1]

    def train(self, input_fn, steps=None, max_steps=None):
        self._check_consistent("train")       # (a poisoned store must be restored from a checkpoint, not trained on)
        it = iter(input_fn())
        if self._use_graph() and _lib.form("input_thread") != "0":      # (measured: no gain next to the launch thread)
            depth = max(16, 2 * self._window_len())
            # (an iterator that outlives this call keeps its thread and whatever the thread has pulled ahead)
            it = it.threaded(depth) if isinstance(it, _Resumable) else _InputThread(it, depth)
        # optional thread that issues the staged windows (single replica, HIP graphs on).  Off by default: a window launch
        # costs the training thread 22-45 us per 8 steps (scripts/graph_launch_cost.py) and the stream is GPU-bound without
        # it; with a slow input pipeline it takes the launch off the fetching thread (e2e A/B: within the box-to-box noise)
        launcher = None
        if self._use_graph() and self.store.dp is None and _lib.form("launch_thread") != "0":
            launcher = _LaunchThread(self.config.device)
        try:
            self._train_loop(it, steps, max_steps, launcher)
        finally:
            if launcher is not None:
                launcher.close()
            _close_iter(it)
        return self

    def _train_loop(self, it, steps, max_steps, launcher):
        done = 0
        cfg = self.config
        self._log_t, log_step0 = time.time(), None
        held = []                # batches pulled ahead that did not go into the last window
        gs_host = None           # the global step, tracked on the host after one device read
        exhausted = False
        while True:
            if steps is not None and done >= steps:
                break
            if max_steps is not None and self.store.built:
                if gs_host is None:
                    gs_host = self.global_step
                if gs_host >= max_steps:
                    break
            # How many steps the next optimizer window may hold (look-ahead over the input pipeline, which runs ahead of
            # the device anyway): never across the end of training, a log line or a checkpoint -- between the steps of a
            # window the variables are not a state the step-by-step run passes through.
            room = self._window_len() if self._use_graph() else 1
            if steps is not None:
                room = min(room, steps - done)
            if max_steps is not None and gs_host is not None:
                room = min(room, max_steps - gs_host)
            for every in (cfg.log_step_count_steps, cfg.save_checkpoints_steps if self.model_dir else 0):
                if every:
                    room = min(room, every - done % every)
            while len(held) < room and not exhausted:
                try:
                    held.append(next(it))
                except StopIteration:
                    exhausted = True
            if not held:
                break
            features, labels = held[0]
            if not self.store.built:          # variables are created by the first model_fn call
                self._call_model_fn(self._to_device(features), self._to_device(labels), ModeKeys.PREDICT)
                self._maybe_restore()
                room = 1
            # one packed host buffer per batch -> one H2D copy each -> the HIP graph's static inputs
            win = [PackedBatch(*held[0])]
            while len(win) < room and len(win) < len(held):
                pb = PackedBatch(*held[len(win)])
                if pb.key() != win[0].key():   # e.g. the last, smaller batch of an epoch: a step of its own
                    break
                win.append(pb)
            if len(win) == 1:
                if launcher is not None:
                    launcher.drain()
                loss = self._train_step(win[0])
            else:                              # (one graph per window length: the full one, and the shorter ones that
                loss = self._train_window_packed(win, launcher)     # end at a log line / checkpoint / the end of training)
            features, labels = held[len(win) - 1]
            del held[:len(win)]
            done += len(win)
            if gs_host is not None:
                gs_host += len(win)
            gs = None
            if done % cfg.log_step_count_steps == 0 or (cfg.save_checkpoints_steps and done % cfg.save_checkpoints_steps == 0):
                if launcher is not None and loss is None:
                    loss = launcher.drain()
                gs = self.global_step
            if gs is not None and done % cfg.log_step_count_steps == 0:
                now = time.time()
                world = 1
                if self.store.dp is not None:
                    # every TRAIN step returns its REPLICA's mean loss (only the gradients carry MirroredStrategy's 1/N): the
                    # mean over replicas is the mean loss of the global batch, which is what gets logged
                    world = self.store.dp.world
                    loss = self.store.dp.all_reduce_sum(loss.detach().clone().reshape(1)) / world
                if self._is_chief():
                    if log_step0 is not None:
                        rate = (gs - log_step0) / max(now - self._log_t, 1e-9)
                        print("INFO:global_step/sec: %.4g  (examples/sec: %.6g)" % (rate, rate * labels.shape[0] * world), flush=True)
                    print("INFO:loss = %.7g, step = %d" % (float(loss), gs), flush=True)
                self._log_t, log_step0 = now, gs
            if gs is not None and cfg.save_checkpoints_steps and self.model_dir and \
                    done % cfg.save_checkpoints_steps == 0:
                self._save_checkpoint(gs)
        if launcher is not None:
            launcher.drain()
        if self.model_dir and self.store.built and done:
            self._save_checkpoint(self.global_step)

    def _infer_step(self, features, labels, mode):
        """One EVAL / PREDICT forward over a host (or device) batch -> (prob, loss or None, labels on the device).  With HIP
        graphs on, the forward is captured once per input signature over static input buffers (ONE packed copy per batch,
        one graph launch): evaluate() was 283 us per batch of eager launches against a 70 us TRAIN step.
        self._infer_features: the features of this batch on the device, valid until the next call."""
        has_lab = labels is not None
        if not self.store.built:          # variables are created by the first model_fn call
            self._call_model_fn(self._to_device(features), self._to_device(labels) if has_lab else None, ModeKeys.PREDICT)
        self._maybe_restore()

        def forward(f, l):                # the eager forward over device tensors -> (prob, loss, labels, features)
            spec = self._call_model_fn(f, l if mode == ModeKeys.EVAL else None, mode)
            return spec.predictions["prob"], spec.loss, (l if has_lab else None), f

        if not self._use_graph():
            out = forward(self._to_device(features), self._to_device(labels) if has_lab else None)
        else:
            pb = PackedBatch(features, labels if has_lab else np.zeros(0, np.float32))
            key = ("infer", mode, has_lab) + pb.key()
            g = self._graphs.get(key)
            if g is None and self._n_infer_graphs < self.MAX_INFER_GRAPHS:
                # the first batch of a signature runs eagerly, the second is captured (one graph also under data parallelism:
                # the forward has no collectives)
                g = self._graphs[key] = self._packed_step(
                    1, forward, lambda f, l: self._capture(lambda: forward(f, l), segment=False))
                self._n_infer_graphs += 1
            # (no record: a serving loop with ever-new request sizes -- stop capturing and remembering signatures, stay eager)
            out = g.run(pb) if g is not None else forward(*self._on_device(pb).views())
        self._infer_features = out[3]
        return out[:3]

    def evaluate(self, input_fn, steps=None):
        """Estimator.evaluate (fm/fm.py:216-221): AUC-200 / Accuracy / mean batch loss accumulated ON DEVICE by one
        launch per batch (metrics.EvalMetrics); the host synchronises once, when the counters are read back.
        Data-parallel: every rank evaluates its own shard of the eval stream and the integer counters are summed.
        The opt-in settings of RunConfig -- exact_auc, group_auc_key, calibration_bins / calibration_key, calibration_fit /
        calibration_apply -- are one object each (_ExactKeys, _GroupAUCSetting, _CalibrationSetting, _CalibrationMapSetting below;
        their docstrings say what each adds): built in that order before the first batch is read, which is where a bad setting
        or a second rank is refused; updated in that order behind EvalMetrics.update on the same stream; reported in that order."""
        self._check_consistent("evaluate")
        settings = self._eval_settings(steps)
        met = _metrics.EvalMetrics(self.store.device)
        n = 0
        it = input_fn()
        try:
            with torch.no_grad():
                for features, labels in it:
                    if steps is not None and n >= steps:
                        break
                    prob, loss, lab = self._infer_step(features, labels, ModeKeys.EVAL)
                    met.update(lab, prob, loss)
                    if settings:
                        # the device copy of the batch that _infer_step just used (the graph's static buffer or the eager
                        # copy): a group column is read in place, behind the forward on the same stream
                        on_device = getattr(self, "_infer_features", None) or features
                        for s in settings:
                            s.update(lab, prob, on_device)
                    n += 1
        finally:
            _close_iter(it)
        if self.store.dp is not None:
            met.all_reduce(self.store.dp)
        res = met.result()
        res = {"AUC": res["AUC"], "Accuracy": res["Accuracy"], "loss": res["loss"], "global_step": self.global_step}
        line = ("INFO:Saving dict for global step %d: AUC = %.7g, Accuracy = %.7g, global_step = %d, loss = %.7g"
                % (res["global_step"], res["AUC"], res["Accuracy"], res["global_step"], res["loss"]))
        for s in settings:
            line += s.report(res)
        if self._is_chief():
            print(line, flush=True)
        for s in settings:
            s.finish(res)
        return res

    def _eval_settings(self, steps):
        """RunConfig -> evaluate()'s opt-in settings, in update and report order."""
        cfg = self.config
        exact, fit = bool(getattr(cfg, "exact_auc", False)), int(getattr(cfg, "calibration_fit", 0) or 0)
        gkey, ckey = getattr(cfg, "group_auc_key", None), getattr(cfg, "calibration_key", None)
        bins, apply = int(getattr(cfg, "calibration_bins", 0) or 0), bool(getattr(cfg, "calibration_apply", False))
        keys = _ExactKeys(self, steps, reported=exact) if exact or fit else None
        return [s for s in (keys,
                            _GroupAUCSetting(self, steps, gkey) if gkey else None,
                            _CalibrationSetting(self, bins, ckey) if bins or ckey else None,
                            _CalibrationMapSetting(self, keys, fit, apply, bins) if fit or apply else None) if s is not None]

    def _script_name(self):
        return self.model_fn.__module__.rsplit(".", 1)[-1]

    def _calibration_path(self, step):
        return os.path.join(self.model_dir, "calibration-%d.json" % int(step)) if self.model_dir else None

    def _calibration_step(self):
        """The global_step the next evaluate() / export runs at, known without reading a batch: the restored variables', or the
        latest checkpoint's while the variables are not built yet."""
        if self.store.built:
            self._maybe_restore()
            return int(self.global_step)
        from . import checkpoint
        import re
        p = checkpoint.latest(self.model_dir) if self.model_dir else None
        return int(re.search(r"model\.ckpt-(\d+)\.pt$", p).group(1)) if p else 0

    def calibration_map_for_step(self, step=None):
        """The metrics.IsotonicMap of `step` (default: the current one): last_calibration_map when it is of that step, else
        <model_dir>/calibration-<step>.json, else None.  A map of another step or another script is never taken."""
        step = self._calibration_step() if step is None else int(step)
        m = self.last_calibration_map
        if m is not None and m.global_step == step and m.script == self._script_name():
            return m
        path = self._calibration_path(step)
        if path and os.path.isfile(path):
            m = _metrics.IsotonicMap.load(path)
            if m.global_step == step and m.script == self._script_name():
                return m
        return None

    def _fit_calibration_map(self, ex, xr, bins):
        """calibration_fit's tail: the equal-mass table of ex's sorted keys -> the map, last_calibration_map, the file.
        -> the number of knots (0: refused)."""
        V, P = xr["positives"] + xr["negatives"], xr["positives"]
        if xr["invalid"] or P == 0 or xr["negatives"] == 0:
            if self._is_chief():
                why = ("%d of %d probabilities are outside [0, 1] or not finite" % (xr["invalid"], xr["invalid"] + V)
                       if xr["invalid"] else "the %d examples hold %d positives and %d negatives" % (V, P, xr["negatives"]))
                print("WARNING:calibration_fit: no map is fitted: %s" % why, flush=True)
            return 0
        table = ex.quantile_table(bins)
        x, y = _metrics.isotonic_from_table(table)
        m = _metrics.IsotonicMap(x, y, bins=bins, examples=V, positives=P, global_step=self.global_step,
                                 script=self._script_name(), table=table, ece=_metrics.calibration_from_table(table, 0)["ECE"])
        self.last_calibration_map = m
        path = self._calibration_path(m.global_step)
        if path and self._is_chief():
            os.makedirs(self.model_dir, exist_ok=True)
            m.save(path)
        if self._is_chief():
            print("INFO:calibration map: K = %d, V = %d, P = %d, path = %s" % (m.knots, V, P, path), flush=True)
        return m.knots

    def _group_column(self, key, setting):
        """The key of RunConfig.group_auc_key / calibration_key -> (features -> the batch's group ids, the column's row count;
        GAUC's group_bits are the bits of row count - 1).
        Criteo scripts and --feature_set uid_iid: the key of an embedding column of the layout; the group is the column's
        table-local id, ids[:, slot] of the batch as it is (host or device, no copy here).  din.py: i_id / i_cate."""
        cols = self.params.get("embedding_feature_columns")
        if cols is not None:
            from .feature_columns import CriteoLayout
            layout = CriteoLayout.from_columns(cols)
            rows = {c.key: (slot, int(c.rows)) for slot, c in enumerate(layout.columns)}
            allowed = [c.key for c in layout.columns]
        else:
            from . import din
            rows = {"i_id": ("i_id", int(self.params.get("n_item", din.N_ITEM)) + 1),
                    "i_cate": ("i_cate", int(self.params.get("n_cate", din.N_CATE)) + 1)}
            allowed = list(rows)
        if key not in rows:
            raise _metrics.RsxError("%s %r is not a feature of this model; allowed: %s" % (setting, key, ", ".join(allowed)))
        where, n_rows = rows[key]
        if cols is not None:
            return (lambda features: features["ids"][:, where]), n_rows
        return (lambda features: features[where]), n_rows

    def _is_chief(self):
        return self.store.dp is None or getattr(self.store.dp, "rank", 0) == 0

    def _save_checkpoint(self, step):
        """Replicas are bit-identical by construction: rank 0 writes, everybody waits (MirroredStrategy: the chief saves)."""
        from . import checkpoint
        self._check_consistent("checkpoint")
        if self._is_chief():
            checkpoint.save(self.model_dir, self.store, step, self.config.keep_checkpoint_max)
        if self.store.dp is not None:
            self.store.dp.barrier()

    def predict(self, input_fn):
        self._check_consistent("predict")
        it = input_fn()
        try:
            with torch.no_grad():
                for features, labels in it:
                    prob, _, _ = self._infer_step(features, labels, ModeKeys.PREDICT)
                    prob = prob.reshape(-1).cpu().numpy()
                    for p in prob:
                        yield {"prob": p}
        finally:
            _close_iter(it)        # the caller usually breaks out after a few results (fm/fm.py:216-219)


    def predict_examples(self, serialized, parse_fn=None, batch_size=4096):
        """Inference entry that takes what a serving client sends: a list of serialized `tf.train.Example` byte strings
        (deepfm/grpc_client.py:50-76 builds exactly these; the reference's exported SavedModel parses them with the
        script's feature_description, deepfm/deepfm.py:213-233) -> {'prob': float32 [n]}.
        parse_fn(list[bytes]) -> (features, labels); default: the Criteo parse spec of the params' embedding columns, or
        the DIN spec (din/din.py:44-57) when the params hold no feature columns."""
        from . import input_pipeline as ip
        self._check_consistent("predict_examples")
        if parse_fn is None:
            cols = self.params.get("embedding_feature_columns")
            if cols is not None:
                from .feature_columns import CriteoLayout
                layout = CriteoLayout.from_columns(cols)
                parse_fn = lambda ex: ip.parse_criteo_examples(ex, layout)          # noqa: E731
            else:
                P = int(self.params.get("hist_len", 100))
                parse_fn = lambda ex: ip.parse_din_examples(ex, P)                  # noqa: E731
        serialized = list(serialized)
        out = []
        with torch.no_grad():
            for s in range(0, len(serialized), batch_size):
                features, labels = parse_fn(serialized[s:s + batch_size])
                prob, _, _ = self._infer_step(features, labels, ModeKeys.PREDICT)
                out.append(prob.reshape(-1).float().cpu().numpy())
        return {"prob": np.concatenate(out) if out else np.zeros(0, np.float32)}


    def export_savedmodel(self, export_dir_base, table_dtype="float32", calibration="auto"):
        """Estimator.export_savedmodel (deepfm/deepfm.py:220-234): the latest checkpoint of model_dir as a serving bundle
        `<export_dir_base>/<unix seconds>/` = model.json + variables.npz (recsys_amd.serving: the variables in fp32, no
        optimizer slots or state), written under a temporary name and renamed when complete.  -> the directory (the chief's
        under data parallelism; None on the other ranks).  serving.Predictor.load() serves it.
        table_dtype "bfloat16" / "float16" (--export_table_dtype): the embedding tables are rounded to that dtype and stored
        in it (a format_version 2 bundle); opt-in, it changes the probabilities.
        calibration (--export_calibration): "auto" puts calibration.json (the metrics.IsotonicMap of the exported global_step:
        last_calibration_map, else <model_dir>/calibration-<step>.json) beside the two files when there is one; "off" never;
        "require" raises when there is none.  A map of another step is never taken."""
        from . import serving
        return serving.export_estimator(self, export_dir_base, table_dtype=table_dtype, calibration=calibration)


class _LaunchThread:
    """Issues the staged windows of Estimator.train (ONE graph replay each) in order, on a thread of its own (opt-in,
    RSX_LAUNCH_THREAD=1): torch releases the GIL inside replay(), so the training thread fetches and stages window w + 1
    meanwhile.  (It was written when a rocprofv3 --hip-runtime-trace showed hipGraphLaunch holding its caller for 499 us per
    window -- which turned out to be the profiler's own interception of the graph's 58 dispatches; unprofiled the launch
    costs 22-45 us, and the stream is GPU-bound either way.)"""

    def __init__(self, device):
        self._q = queue.Queue(maxsize=1)
        self._err = None
        self.last = None
        self._dev = torch.cuda.current_device() if torch.device(device).type == "cuda" else None
        self._t = threading.Thread(target=self._run, name="rsx-launch", daemon=True)
        self._t.start()

    def _run(self):
        while True:
            fn = self._q.get()
            try:
                if fn is None:
                    return
                if self._err is None:
                    if self._dev is not None and torch.cuda.current_device() != self._dev:
                        torch.cuda.set_device(self._dev)
                    self.last = fn()
            except BaseException as e:             # surfaces at the next submit / drain
                self._err = e
            finally:
                self._q.task_done()

    def _check(self):
        if not self._t.is_alive():
            raise RuntimeError("rsx-launch thread is gone") from self._err

    def submit(self, fn):
        if self._err is not None:
            self.drain()
        while True:
            self._check()
            try:
                self._q.put(fn, timeout=1.0)
                return
            except queue.Full:
                continue

    def drain(self):
        """Everything submitted has been issued to the stream -> result of the last launch."""
        with self._q.all_tasks_done:
            while self._q.unfinished_tasks:
                self._check()
                self._q.all_tasks_done.wait(timeout=1.0)
        if self._err is not None:
            e, self._err = self._err, None
            raise e
        return self.last

    def close(self):
        try:
            self.drain()
        except BaseException:
            pass
        if self._t.is_alive():
            self._q.put(None)
            self._t.join(timeout=5.0)
        self._err = None


class _InputThread:
    """Pulls batches from an input iterator on a thread of its own, a bounded number ahead of the consumer (opt-in,
    RSX_INPUT_THREAD=1).  The reader's `next` is a C call that releases the GIL, but the generator code around it and the
    training thread's own Python share the GIL: end to end it measured within the noise of the default (the C++ reader already
    runs `prefetch` batches ahead on its own threads), so it stays a knob for input_fns that do real Python work per batch."""

    _END = object()

    def __init__(self, it, depth):
        self._it = it
        self._q = queue.Queue(maxsize=max(2, int(depth)))
        self._stop = False
        self._t = threading.Thread(target=self._run, name="rsx-input", daemon=True)
        self._t.start()

    def _run(self):
        try:
            for item in self._it:
                if self._stop:
                    break
                while not self._stop:
                    try:
                        self._q.put((item, None), timeout=0.05)
                        break
                    except queue.Full:
                        continue
                if self._stop:
                    break
            item = (self._END, None)
        except BaseException as e:                 # surfaces in the consumer
            item = (self._END, e)
        _close_iter(self._it)                      # (by the thread that runs the generator)
        while not self._stop:
            try:
                self._q.put(item, timeout=0.05)
                return
            except queue.Full:
                continue

    def __iter__(self):
        return self

    def __next__(self):
        item, extra = self._q.get()
        if item is self._END:
            self._q.put((item, extra))             # (stay exhausted)
            if extra is not None:
                raise extra
            raise StopIteration
        return item

    def close(self):
        self._stop = True
        try:
            while True:
                self._q.get_nowait()
        except queue.Empty:
            pass
        self._t.join(timeout=5.0)


def _close_iter(it):
    """Stop a prefetching input iterator whose consumer leaves early (evaluate(steps=...), predict's caller breaking
    out): generators get close(), which runs their `finally` and stops the producer thread."""
    close = getattr(it, "close", None)
    if close is not None:
        close()


def _world(est):
    return 1 if est.store.dp is None else est.store.dp.world


class _EvalSetting:
    """One opt-in setting of Estimator.evaluate().  The constructor refuses what the setting cannot do before the first batch is
    read.  update(lab, prob, features): the batch's launches, behind EvalMetrics.update on the same stream, no synchronisation
    (features: the device copy of the batch).  report(res): adds the result keys, prints the setting's WARNING line on the chief
    and returns its part of the "INFO:Saving dict" line.  finish(res): what comes behind that line."""

    def update(self, lab, prob, features):
        pass

    def report(self, res):
        return ""

    def finish(self, res):
        pass


def _first_batch_capacity(steps, prob):
    """The key buffers are sized by the first batch: steps batches of its size, growable when steps is None."""
    return None if steps is None else max(1, int(steps) * int(prob.numel()))


class _ExactKeys(_EvalSetting):
    """RunConfig.exact_auc: "AUC_exact" (metrics.ExactAUC: one more launch per batch, one sort and one more device->host copy at
    the end; nan, with a WARNING line, when a probability was outside [0, 1]); single replica only.  calibration_fit reduces the
    same sorted keys, so with either setting ONE ExactAUC is kept; without exact_auc nothing is reported."""

    def __init__(self, est, steps, reported):
        if reported:
            _metrics.check_single_replica("exact_auc", _world(est))
        self.est, self.steps, self.reported, self.acc, self.counts = est, steps, reported, None, None

    def update(self, lab, prob, features):
        if self.acc is None:
            self.acc = _metrics.ExactAUC(self.est.store.device, _first_batch_capacity(self.steps, prob))
        self.acc.update(lab, prob)

    def report(self, res):
        self.acc = self.acc or _metrics.ExactAUC(self.est.store.device, 1)
        xr = self.counts = self.acc.result()
        if not self.reported:
            return ""
        res["AUC_exact"] = _metrics.exact_auc_reported(xr)
        if xr["invalid"] and self.est._is_chief():
            print("WARNING:exact_auc: %d of %d probabilities are outside [0, 1] or not finite; AUC_exact is nan"
                  % (xr["invalid"], xr["invalid"] + xr["positives"] + xr["negatives"]), flush=True)
        return ", AUC_exact = %.7g" % res["AUC_exact"]


class _GroupAUCSetting(_EvalSetting):
    """RunConfig.group_auc_key: "GAUC", "GAUC_groups" and "GAUC_skipped_examples" (metrics.GroupAUC: one more launch per batch;
    at the end one sort, the header's copy, one records launch and the records' copy); single replica only.  An unknown key is
    refused by Estimator._group_column."""

    def __init__(self, est, steps, key):
        _metrics.check_single_replica("group_auc_key", _world(est))
        self.group_of, n_rows = est._group_column(key, "group_auc_key")
        self.bits = min(31, max(1, (n_rows - 1).bit_length()))
        self.est, self.steps, self.key, self.acc = est, steps, key, None

    def update(self, lab, prob, features):
        if self.acc is None:
            self.acc = _metrics.GroupAUC(self.est.store.device, self.bits, _first_batch_capacity(self.steps, prob))
        self.acc.update(self.group_of(features), lab, prob)

    def report(self, res):
        gr = (self.acc or _metrics.GroupAUC(self.est.store.device, self.bits, 1)).result()
        res["GAUC"] = _metrics.group_auc_reported(gr)
        res["GAUC_groups"] = gr["mixed_groups"]
        res["GAUC_skipped_examples"] = gr["skipped_examples"]
        if gr["invalid"] and self.est._is_chief():
            print("WARNING:group_auc_key %s: %d examples have a probability outside [0, 1] or not finite, or an id outside "
                  "[0, 2^%d); GAUC is nan" % (self.key, gr["invalid"], self.bits), flush=True)
        return ", GAUC = %.7g" % res["GAUC"]


class _CalibrationSetting(_EvalSetting):
    """RunConfig.calibration_bins: "ECE", "MCE", "PCOC" and "NE" (NE from this call's loss); RunConfig.calibration_key: "GCE" and
    "GCE_groups" (metrics.Calibration: one more launch per batch for both, one more device->host copy at the end; nan, with a
    WARNING line, when an example was invalid); the full result stays in Estimator.last_calibration; single replica only."""

    def __init__(self, est, bins, key):
        _metrics.check_single_replica("calibration", _world(est))
        self.group_of, self.n_groups = est._group_column(key, "calibration_key") if key else (None, None)
        self.acc = _metrics.Calibration(est.store.device, bins or None, self.n_groups)
        self.est, self.bins, self.key = est, bins, key

    def update(self, lab, prob, features):
        self.acc.update(lab, prob, self.group_of(features) if self.key else None)

    def report(self, res):
        cr = self.est.last_calibration = self.acc.result(loss=res["loss"], per_group=True)
        line = ""
        if self.bins:
            res.update({k: v for k, v in _metrics.calibration_reported(cr).items() if k in ("ECE", "MCE", "PCOC", "NE")})
            line += ", ECE = %.7g, PCOC = %.7g, NE = %.7g" % (res["ECE"], res["PCOC"], res["NE"])
        if self.key:
            res["GCE"] = _metrics.group_calibration_reported(cr)["GCE"]
            res["GCE_groups"] = cr["GCE_groups"]
            line += ", GCE = %.7g" % res["GCE"]
        if cr["invalid"] and self.est._is_chief():
            print("WARNING:calibration: %d of %d examples have a probability outside [0, 1] or not finite%s; the calibration "
                  "figures are nan" % (cr["invalid"], cr["invalid"] + cr["examples"],
                                       ", or a %s id outside [0, %d)" % (self.key, self.n_groups) if self.key else ""), flush=True)
        return line


class _CalibrationMapSetting(_EvalSetting):
    """RunConfig.calibration_fit = M: behind the INFO line, an isotonic map fitted from the keys _ExactKeys has sorted (ONE launch
    of rsx_calibration_quantile_table and a copy of 24 M bytes, then metrics.isotonic_from_table on the host):
    Estimator.last_calibration_map, <model_dir>/calibration-<global_step>.json (the chief writes it, temporary name and rename),
    "calibration_knots" in the result (0 when the fit is refused: an invalid example, or no positive or no negative -- one
    WARNING line, no file).  RunConfig.calibration_apply: every batch's prob is mapped through the map of the current
    global_step into a second buffer (rsx_calibrate_apply, same stream) and a second bin table gives "ECE_cal", "MCE_cal" and
    "PCOC_cal"; every other key keeps its raw value.  Refused: a second rank, both settings together (in-sample figures), M
    outside 2..1024, calibration_apply without calibration_bins or without a map of this step.  A logloss / NE of the mapped
    probabilities is out of scope.
    The fit depends on `keys` (the _ExactKeys of this evaluate()): keys.report() must have run, reported or not -- it sorts the
    keys and leaves the counts that finish() reads -- which evaluate() guarantees by reporting every setting before any finish()."""

    def __init__(self, est, keys, fit, apply, bins):
        _metrics.check_single_replica("calibration map", _world(est))
        if fit and apply:
            raise _metrics.RsxError("calibration_fit and calibration_apply in one evaluate() would report in-sample figures: "
                                    "fit on one evaluation, apply in another")
        if fit:
            _metrics.check_bins(fit, "calibration_fit %d is outside %d..%d")
        self.est, self.keys, self.fit, self.map, self.buf = est, keys, fit, None, None
        if apply:
            if not bins:
                raise _metrics.RsxError("calibration_apply needs calibration_bins: ECE_cal is a figure of that table")
            step = est._calibration_step()
            m = est.calibration_map_for_step(step)
            if m is None:
                raise _metrics.RsxError("calibration_apply: no calibration map for global step %d (neither last_calibration_map "
                                        "nor %s); run evaluate() with calibration_fit first"
                                        % (step, est._calibration_path(step) or "a model_dir"))
            self.map = _metrics.Calibrator(est.store.device, m)
            self.acc = _metrics.Calibration(est.store.device, bins)

    def update(self, lab, prob, features):
        if self.map is None:
            return
        # into a buffer of its own (prob may be the graph's static output), the same stream
        p1 = prob if prob.dtype == torch.float32 and prob.is_contiguous() else prob.to(torch.float32).contiguous()
        if self.buf is None or self.buf.numel() != p1.numel():              # (the last batch of a stream may be a partial one)
            self.buf = torch.empty(p1.numel(), dtype=torch.float32, device=p1.device)
        self.acc.update(lab, self.map.apply(p1, out=self.buf))

    def report(self, res):
        if self.map is None:
            return ""
        rep = _metrics.calibration_reported(self.acc.result())
        res.update({"ECE_cal": rep["ECE"], "MCE_cal": rep["MCE"], "PCOC_cal": rep["PCOC"]})
        return ", ECE_cal = %.7g, PCOC_cal = %.7g" % (res["ECE_cal"], res["PCOC_cal"])

    def finish(self, res):
        if self.fit:
            res["calibration_knots"] = self.est._fit_calibration_map(self.keys.acc, self.keys.counts, self.fit)


def train_and_evaluate(estimator: Estimator, train_spec: TrainSpec, eval_spec: EvalSpec, eval_every_steps=None):
    """estimator.train_and_evaluate (fm/fm.py:222): train until the input is exhausted / max_steps, evaluating
    at every checkpoint (the TF loop evaluates whenever a new checkpoint appears, throttled)."""
    every = eval_every_steps or estimator.config.save_checkpoints_steps
    res = None
    if not every:
        estimator.train(train_spec.input_fn, max_steps=train_spec.max_steps)
        return estimator.evaluate(eval_spec.input_fn, steps=eval_spec.steps)
    it_fn = _Resumable(train_spec.input_fn)
    while not it_fn.exhausted:
        estimator.train(it_fn, steps=every, max_steps=train_spec.max_steps)
        res = estimator.evaluate(eval_spec.input_fn, steps=eval_spec.steps)
        if train_spec.max_steps is not None and estimator.global_step >= train_spec.max_steps:
            break
    return res


class _Resumable:
    """Keeps one iterator alive across successive Estimator.train(steps=...) calls."""

    def __init__(self, input_fn):
        self.it = None
        self.input_fn = input_fn
        self.exhausted = False

    def __call__(self):
        if self.it is None:
            self.it = iter(self.input_fn())
        return self

    def __iter__(self):
        return self

    def threaded(self, depth):
        """Move the underlying iterator behind an input thread (once): batches pulled ahead stay queued between calls."""
        if not isinstance(self.it, _InputThread):
            self.it = _InputThread(self.it, depth)
        return self

    def __next__(self):
        try:
            return next(self.it)
        except StopIteration:
            self.exhausted = True
            raise
