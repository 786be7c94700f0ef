"""Streaming eval metrics on device: tf.metrics.auc (200 thresholds, trapezoidal
ROC), tf.metrics.accuracy(labels, tf.round(pred)) and the Estimator's mean of the batch losses, as the
eval_metric_ops of fm/fm.py:150-153 and Estimator.evaluate(steps=200) fm/fm.py:221 produce them.

One HIP launch per eval batch (`rsx_eval_metrics_update`, csrc/metrics.hip) accumulates everything in a 406-word
device buffer; the host reads it back ONCE in `result()` -- evaluate() never synchronises per batch.  Data-parallel
evaluation sums the integer counters of all ranks before the finalisation (`all_reduce`).

Opt-in beside it (RunConfig.exact_auc): `ExactAUC`, the exact tie-aware rank statistic (sklearn's roc_auc_score, which the
reference's serving client reports, deepfm/grpc_client.py:84) from a device-wide key sort (csrc/auc_exact.hip); `exact_auc_host`
states its definition in numpy.  And beside that (RunConfig.group_auc_key): `GroupAUC`, the same statistic per group, weighted by the
group's examples -- the DIN paper's GAUC (csrc/auc_group.hip); `group_auc_records_host` is its definition in numpy and
`group_auc_from_records` the one place that divides.  Those three are rank statistics; whether a probability of 0.03 means 3 % is
what `Calibration` answers (RunConfig.calibration_bins / calibration_key): a reliability table and a per-group table of (count,
positives, fixed-point sum of p), one launch per batch (csrc/calibration.hip); `calibration_bins_host` / `calibration_groups_host`
are their definitions in numpy and `calibration_from_table` (ECE, MCE, PCOC, NE) / `group_calibration_from_table` (GCE) divide.
What to do about a miscalibrated model is isotonic regression (RunConfig.calibration_fit / calibration_apply,
csrc/calibration_map.hip): `ExactAUC.quantile_table` reduces the sorted keys to an equal-mass table, `isotonic_from_table` fits the
knots from it in Python integers, `IsotonicMap` carries them (JSON, fp32 bit patterns) and `Calibrator` applies them on the device;
`quantile_table_host` / `isotonic_apply_host` are the definitions in numpy."""
import ctypes as C

import numpy as np
import torch

from ._lib import RsxError, check, lib


def auc_thresholds(num_thresholds=200):
    """TF metrics_impl.py: kepsilon = 1e-7; thresholds = [0 - eps] + [(i+1)/(n-1) for i in range(n-2)] + [1 + eps],
    Python doubles handed to a float32 constant."""
    n, eps = num_thresholds, 1e-7
    return np.array([0.0 - eps] + [(i + 1) * 1.0 / (n - 1) for i in range(n - 2)] + [1.0 + eps], np.float32)


class EvalMetrics:
    """AUC + Accuracy + mean loss of one evaluate() call."""

    def __init__(self, device, num_thresholds=200):
        self.T = num_thresholds
        self.device = torch.device(device)
        self.th = torch.from_numpy(auc_thresholds(num_thresholds)).to(self.device)
        words = lib().rsx_eval_metrics_state_words(self.T)
        self.state = torch.zeros(words, dtype=torch.int64, device=self.device)

    def update(self, labels, prob, batch_loss=None):
        """labels / prob: device tensors of B elements (any shape); batch_loss: device scalar or None."""
        y = labels.reshape(-1).to(torch.float32).contiguous()
        p = prob.reshape(-1).to(torch.float32).contiguous()
        if y.numel() != p.numel():
            raise ValueError("labels and predictions differ in size")
        bl = None if batch_loss is None else batch_loss.detach().reshape(-1)[:1].to(torch.float32).contiguous()
        check(lib().rsx_eval_metrics_update(C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()),
                                            C.c_void_p(self.th.data_ptr()), self.T,
                                            C.c_void_p(bl.data_ptr() if bl is not None else None),
                                            C.c_void_p(self.state.data_ptr()), int(p.numel()),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rsx_eval_metrics_update")

    def all_reduce(self, dp):
        """Sum the counters of every rank (data-parallel evaluation over disjoint shards)."""
        T = self.T
        loss = self.state[2 * T + 5:2 * T + 6].view(torch.float64).clone()
        ints = self.state.clone()
        ints[2 * T + 5] = 0
        dp.all_reduce_sum(ints)
        dp.all_reduce_sum(loss)
        self.state.copy_(ints)
        self.state[2 * T + 5:2 * T + 6] = loss.view(torch.int64)

    def result(self):
        """-> {'AUC', 'Accuracy', 'loss', 'examples'}; ONE device->host copy."""
        T = self.T
        s = self.state.cpu().numpy()
        return finalize(s[:T + 1], s[T + 1:2 * T + 2], int(s[2 * T + 2]), int(s[2 * T + 3]), int(s[2 * T + 4]),
                        float(s[2 * T + 5:2 * T + 6].view(np.float64)[0]))


def finalize(hist_pos, hist_neg, correct, examples, batches, loss_sum):
    """Counters -> metric values with TF's fp32 formulas: tpr = (tp + 1e-6) / (tp + fn + 1e-6),
    fpr = fp / (fp + tn + 1e-6), AUC = sum((fpr[i] - fpr[i+1]) * (tpr[i] + tpr[i+1]) / 2)."""
    T = len(hist_pos) - 1
    # tp[i] = #(label & pred > t_i) = examples that exceed MORE than i thresholds
    tp = (hist_pos[::-1].cumsum()[::-1])[1:].astype(np.float32)
    fp = (hist_neg[::-1].cumsum()[::-1])[1:].astype(np.float32)
    fn = np.float32(hist_pos.sum()) - tp
    tn = np.float32(hist_neg.sum()) - fp
    assert tp.shape[0] == T
    e = np.float32(1e-6)
    tpr = (tp + e) / (tp + fn + e)
    fpr = fp / (fp + tn + e)
    auc = float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / np.float32(2.0), dtype=np.float32))
    return {"AUC": auc, "Accuracy": correct / max(examples, 1), "loss": loss_sum / max(batches, 1), "examples": examples}


# ---- what the opt-in metrics share: the example rule, the settings' checks, the inputs of an update ---------------------------
CALIBRATION_MIN_BINS, CALIBRATION_MAX_BINS = 2, 1024       # rsx_calibration_max_bins()


def example_bits_host(labels, prob):
    """The example rule of csrc/eval_device.h, in numpy: u = the fp32 pattern of p as an integer (never passed through
    arithmetic), -0.0 as +0.0; valid when u <= 0x3F800000 (0 <= p <= 1); positive when label > 0.5.
    -> (positive bool [n] (None when labels is None), u uint32 [n], valid bool [n]), flat."""
    p = np.ascontiguousarray(np.asarray(prob, np.float32).reshape(-1))
    pos = None
    if labels is not None:
        y = np.ascontiguousarray(np.asarray(labels, np.float32).reshape(-1))
        if y.size != p.size:
            raise ValueError("labels and predictions differ in size")
        pos = y > np.float32(0.5)
    u = p.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return pos, u, u <= 0x3F800000


def check_bins(n_bins, refusal=None):
    """n_bins as an int in 2..1024.  Outside: ValueError (the host definitions), or RsxError(refusal % (n_bins, 2, 1024)) where
    a device class or evaluate() names its own text."""
    n_bins = int(n_bins)
    if not CALIBRATION_MIN_BINS <= n_bins <= CALIBRATION_MAX_BINS:
        if refusal is None:
            raise ValueError("n_bins must be in 2..1024")
        raise RsxError(refusal % (n_bins, CALIBRATION_MIN_BINS, CALIBRATION_MAX_BINS))
    return n_bins


def check_single_replica(setting, world):
    """exact_auc, group_auc_key, the calibration tables and the calibration map are single-replica evaluations: the ranks' keys
    would have to be sorted together (the tables summed).  setting: "exact_auc", "group_auc_key", "calibration" or
    "calibration map", the prefix of the refusal."""
    if int(world) > 1:
        what = "tables would have to be summed" if setting == "calibration" else "keys would have to be sorted"
        raise RsxError("%s: data-parallel evaluation is not supported (the ranks' %s together); evaluate on one replica"
                       % (setting, what))


def floats_on_device(x, device):
    """-> B fp32 values, contiguous on the device.  A contiguous float32 device tensor is passed through as it is (evaluate()'s
    tensors: at batch 256 the host's work per batch is the cost); numpy arrays and other tensors are converted and flattened."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous():
        return x
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
    return x.to(device).reshape(-1).to(torch.float32).contiguous()


def _group_ids_int32(groups):
    """Group ids of any integer dtype as int32, an id that int32 cannot hold as -1 (invalid for every group_bits)."""
    g = np.asarray(groups).reshape(-1)
    if g.dtype == np.int32:
        return np.ascontiguousarray(g)
    g = g.astype(np.int64)
    return np.where((g < 0) | (g > 0x7FFFFFFF), -1, g).astype(np.int32)


def group_column_on_device(g, device):
    """-> (int32 device tensor, element stride): a 1-D int32 device tensor is taken as it is, strided or not (ids[:, slot])."""
    if isinstance(g, torch.Tensor):
        if g.is_cuda and g.dtype == torch.int32 and g.dim() == 1 and (g.numel() <= 1 or g.stride(0) >= 1):
            return g, max(1, int(g.stride(0)))
        g = g.reshape(-1)
        if g.dtype != torch.int32:
            g = g.to(torch.int64)
            g = torch.where((g < 0) | (g > 0x7FFFFFFF), torch.full_like(g, -1), g).to(torch.int32)
    else:
        g = torch.from_numpy(_group_ids_int32(g))
    return g.to(device).contiguous(), 1


class _KeyBuffer:
    """What ExactAUC and GroupAUC share: the device key buffer -- capacity (examples) fixed when given (an update past it
    raises), otherwise grown by doubling from GROW_FROM up to max_keys, with a device copy and no synchronisation --, `count`,
    the output words and the workspace of result()."""
    GROW_FROM = 1 << 16

    def __init__(self, device, name, key_dtype, max_keys, capacity, out_words):
        self.device, self.name = torch.device(device), name
        self.fixed = capacity is not None
        self.max_keys = int(max_keys)
        cap = max(1, int(capacity)) if self.fixed else self.GROW_FROM
        if cap > self.max_keys:
            raise RsxError("%s: capacity %d is above the %d keys one sort takes" % (name, cap, self.max_keys))
        self.keys = torch.empty(cap, dtype=key_dtype, device=self.device)
        self.count = 0
        self.out = torch.zeros(out_words, dtype=torch.int64, device=self.device)
        self.workspace = None

    def _room_for(self, n):
        """Room for n more keys behind the `count` that are held -> the new count (the caller stores it after its launch)."""
        need = self.count + n
        if need > self.keys.numel():
            if self.fixed or need > self.max_keys:
                raise RsxError("%s: %d examples do not fit the key buffer of %d"
                               % (self.name, need, self.keys.numel() if self.fixed else self.max_keys))
            grown = torch.empty(min(self.max_keys, max(2 * self.keys.numel(), need)), dtype=self.keys.dtype, device=self.device)
            grown[:self.count].copy_(self.keys[:self.count])
            self.keys = grown
        return need

    def _workspace_of(self, need):
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.workspace


# ---- exact, tie-aware ROC AUC (include/rsx.h rsx_auc_exact_*) -----------------------------------------------------------------
EXACT_AUC_PAD = 0xFFFFFFFF


def exact_auc_keys_host(labels, prob):
    """The 32-bit keys of rsx_auc_exact_append: (u << 1) | positive for a valid example (example_bits_host), else the padding
    key."""
    pos, u, valid = example_bits_host(labels, prob)
    return np.where(valid, (u << np.uint32(1)) | pos.astype(np.uint32), np.uint32(EXACT_AUC_PAD)).astype(np.uint32)


def sorted_valid_keys_host(labels, prob):
    """-> (the valid keys of exact_auc_keys_host, sorted; the head of every score group, bool; the number of invalid examples)"""
    keys = exact_auc_keys_host(labels, prob)
    ks = np.sort(keys[keys != EXACT_AUC_PAD])
    head = np.ones(ks.size, bool)
    head[1:] = (ks[1:] >> 1) != (ks[:-1] >> 1)
    return ks, head, int(keys.size - ks.size)


def exact_auc_from_counts(u2, positives, negatives, invalid):
    """The five-entry result from the four integers: AUC_exact = U2 / (2 P N) from Python integers (correctly rounded), nan
    when P N == 0."""
    u2, P, N = int(u2), int(positives), int(negatives)
    auc = u2 / (2 * P * N) if P * N else float("nan")
    return {"AUC_exact": auc, "u2": u2, "positives": P, "negatives": N, "invalid": int(invalid)}


def exact_auc_host(labels, prob):
    """The documented definition, in numpy (what serving.topk_rows_host is for top-k): sort the valid keys; c[i] = negatives in
    front of position i, h[i] = c at the head of i's score group; U2 = sum over positives of (c + h) =
    sum over positives of (2 #{negatives with a smaller score} + #{negatives with the same score}).
    -> {"AUC_exact", "u2", "positives", "negatives", "invalid"}"""
    ks, head, invalid = sorted_valid_keys_host(labels, prob)
    neg = (ks & 1) == 0
    c = np.cumsum(neg, dtype=np.int64) - neg                         # exclusive
    h = np.maximum.accumulate(np.where(head, c, 0)) if ks.size else c
    u2 = int(np.sum((c + h)[~neg], dtype=np.int64))
    return exact_auc_from_counts(u2, int((~neg).sum()), int(neg.sum()), invalid)


def exact_auc_reported(res):
    """What evaluate() reports as "AUC_exact": the statistic of a stream without invalid examples, nan otherwise (a model that
    emits a NaN or a probability outside [0, 1] has no AUC worth a number; the count goes into a WARNING line)."""
    return float("nan") if res["invalid"] else res["AUC_exact"]


class ExactAUC(_KeyBuffer):
    """Exact ROC AUC of one evaluate() call: one append launch per batch into a device key buffer, one sort + reduction and
    ONE device->host copy in `result()`.  capacity: _KeyBuffer's rules.  Memory: 4 B per key +
    rsx_auc_exact_workspace_bytes(n) = 4 n + 1032 ceil(n / 4096) + 4096 B while result() runs."""

    def __init__(self, device, capacity=None):
        # out: [0..3] finalize's {U2, P, N, invalid}; [4] the invalid examples the append launches counted
        super().__init__(device, "exact_auc", torch.int32, lib().rsx_auc_exact_max_keys(), capacity, 5)
        self.sorted_valid = None          # V = P + N of the latest result() while the buffer still holds its sorted keys

    def update(self, labels, prob):
        """labels / prob: device tensors or numpy arrays of B elements (any shape).  No host synchronisation."""
        y, p = floats_on_device(labels, self.device), floats_on_device(prob, self.device)
        n = int(p.numel())
        if y.numel() != n:
            raise ValueError("labels and predictions differ in size")
        if n == 0:
            return
        need = self._room_for(n)
        check(lib().rsx_auc_exact_append(C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()), n,
                                         C.c_void_p(self.keys.data_ptr() + 4 * self.count),
                                         C.c_void_p(self.out.data_ptr() + 8 * 4),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rsx_auc_exact_append")
        self.count = need
        self.sorted_valid = None

    def result(self):
        """-> {"AUC_exact", "u2", "positives", "negatives", "invalid"}; one finalize, ONE device->host copy.  The key buffer keeps
        its multiset (sorted), so updates may continue afterwards."""
        ws = self._workspace_of(int(lib().rsx_auc_exact_workspace_bytes(self.count)))
        check(lib().rsx_auc_exact_finalize(C.c_void_p(self.keys.data_ptr()), self.count, C.c_void_p(ws.data_ptr()),
                                           int(ws.numel()), C.c_void_p(self.out.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rsx_auc_exact_finalize")
        s = [int(v) for v in self.out.cpu().numpy()]
        if s[3] != s[4] or s[1] + s[2] + s[3] != self.count:
            raise RsxError("exact_auc: the sorted keys hold %d positives, %d negatives and %d invalid examples of %d; the append "
                           "launches counted %d invalid" % (s[1], s[2], s[3], self.count, s[4]))
        self.sorted_valid = s[1] + s[2]
        return exact_auc_from_counts(s[0], s[1], s[2], s[3])

    def quantile_table(self, n_bins):
        """The equal-mass, tie-aware table of the examples result() has sorted (quantile_table_host's, integer for integer):
        int64 [n_bins, 3] = (count, positives, q_sum).  Call it after result() and before the next update(); ONE launch
        (rsx_calibration_quantile_table, no workspace) and ONE device->host copy of 24 n_bins bytes."""
        n_bins = check_bins(n_bins, "quantile_table: n_bins %d is outside %d..%d")
        if self.sorted_valid is None:
            raise RsxError("quantile_table: call result() first (it sorts the keys), and again after any further update()")
        table = torch.empty(3 * n_bins, dtype=torch.int64, device=self.device)
        check(lib().rsx_calibration_quantile_table(C.c_void_p(self.keys.data_ptr()), self.sorted_valid, n_bins,
                                                   C.c_void_p(table.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "rsx_calibration_quantile_table")
        return table.cpu().numpy().reshape(n_bins, 3)


# ---- GAUC: the exact AUC per group, weighted by the group's examples (include/rsx.h rsx_auc_group_*) ---------------------------
GROUP_AUC_PAD = 0xFFFFFFFFFFFFFFFF
# the 8 words of rsx_auc_group_finalize's header (the last one is zero)
GROUP_AUC_HEADER = ("valid", "invalid", "groups", "mixed_groups", "skipped_examples", "positives", "negatives")


def group_auc_keys_host(groups, labels, prob, group_bits=31):
    """The 64-bit keys of rsx_auc_group_append: (uint64(g) << 32) | k32 with k32 = exact_auc_keys_host's key, for a valid k32 and
    0 <= g < 2^group_bits; the padding key otherwise."""
    if not 1 <= int(group_bits) <= 31:
        raise ValueError("group_bits must be in 1..31")
    k32 = exact_auc_keys_host(labels, prob)
    g = _group_ids_int32(groups).astype(np.int64)
    if g.size != k32.size:
        raise ValueError("groups and predictions differ in size")
    valid = (k32 != EXACT_AUC_PAD) & (g >= 0) & (g < (1 << int(group_bits)))
    key = (np.where(valid, g, 0).astype(np.uint64) << np.uint64(32)) | k32.astype(np.uint64)
    return np.where(valid, key, np.uint64(GROUP_AUC_PAD)).astype(np.uint64)


def group_auc_records_host(groups, labels, prob, group_bits=31):
    """The documented definition, in numpy: sort the valid keys; c[i] = negatives in front of position i (globally), h[i] = c at
    the head of i's score group, b[i] = c at the head of i's group; a positive adds (c - b) + (h - b) = 2 #{the group's smaller
    negatives} + #{the group's equal negatives} to its group's U2.
    -> (records uint64 [G, 4] = (g, P_g, N_g, U2_g) of ALL groups in ascending g, the number of invalid examples)"""
    keys = group_auc_keys_host(groups, labels, prob, group_bits)
    ks = np.sort(keys[keys != np.uint64(GROUP_AUC_PAD)])
    invalid = int(keys.size - ks.size)
    if ks.size == 0:
        return np.zeros((0, 4), np.uint64), invalid
    neg = (ks & np.uint64(1)) == 0
    c = np.cumsum(neg, dtype=np.int64) - neg                          # exclusive
    score, grp = ks >> np.uint64(1), ks >> np.uint64(32)
    shead, ghead = np.ones(ks.size, bool), np.ones(ks.size, bool)
    shead[1:] = score[1:] != score[:-1]
    ghead[1:] = grp[1:] != grp[:-1]
    h = np.maximum.accumulate(np.where(shead, c, 0))
    b = np.maximum.accumulate(np.where(ghead, c, 0))
    con = np.where(neg, 0, (c - b) + (h - b)).astype(np.int64)
    starts = np.flatnonzero(ghead)
    u2 = np.add.reduceat(con, starts)
    n_neg = np.add.reduceat(neg.astype(np.int64), starts)
    n_all = np.diff(np.append(starts, ks.size))
    rec = np.stack([grp[starts].astype(np.int64), n_all - n_neg, n_neg, u2], axis=1)
    return rec.astype(np.uint64), invalid


def group_auc_header_host(records, invalid):
    """The 8 header words rsx_auc_group_finalize gives for a stream with these records (of all its groups)."""
    rec = np.asarray(records, np.uint64).reshape(-1, 4)
    P, N = [int(v) for v in rec[:, 1]], [int(v) for v in rec[:, 2]]
    mixed = [p > 0 and n > 0 for p, n in zip(P, N)]
    skipped = sum(p + n for p, n, m in zip(P, N, mixed) if not m)
    return [sum(P) + sum(N), int(invalid), len(P), sum(mixed), skipped, sum(P), sum(N), 0]


def group_auc_from_records(records, header):
    """THE place that divides.  records: uint64 [G, 4] = (g, P_g, N_g, U2_g) (one-class groups among them are passed over);
    header: the 8 words of rsx_auc_group_finalize / group_auc_header_host.  Per mixed group the float64 U2 / (2 P N), correctly
    rounded (from Python integers where a term reaches 2^53 and a float64 would not hold it), weighted by n_g = P_g + N_g; both
    sums by math.fsum, so equal integers give an equal float.
    -> {"GAUC" (nan when no group is mixed), "groups", "mixed_groups", "skipped_examples", "invalid"}"""
    import math
    rec = np.asarray(records, np.uint64).reshape(-1, 4)
    hdr = [int(v) for v in header]
    P, N, U = rec[:, 1], rec[:, 2], rec[:, 3]
    mixed = (P > 0) & (N > 0)
    P, N, U = P[mixed], N[mixed], U[mixed]
    if int(P.size) != hdr[3]:
        raise RsxError("group_auc: %d mixed groups among the records, %d in the header" % (int(P.size), hdr[3]))
    gauc = float("nan")
    if P.size:
        den = np.uint64(2) * P * N                                    # P, N <= 2^27
        auc = np.empty(P.size, np.float64)
        exact = (U < np.uint64(1 << 53)) & (den < np.uint64(1 << 53))
        auc[exact] = U[exact].astype(np.float64) / den[exact].astype(np.float64)
        for i in np.flatnonzero(~exact):
            auc[i] = int(U[i]) / int(den[i])
        w = (P + N).astype(np.float64)
        gauc = math.fsum(w * auc) / math.fsum(w)
    return {"GAUC": gauc, "groups": hdr[2], "mixed_groups": hdr[3], "skipped_examples": hdr[4], "invalid": hdr[1]}


def group_auc_host(groups, labels, prob, group_bits=31):
    """group_auc_from_records of group_auc_records_host: GAUC as evaluate() computes it, in numpy."""
    rec, invalid = group_auc_records_host(groups, labels, prob, group_bits)
    return group_auc_from_records(rec, group_auc_header_host(rec, invalid))


def group_auc_reported(res):
    """What evaluate() reports as "GAUC": nan when any example was invalid (as exact_auc_reported)."""
    return float("nan") if res["invalid"] else res["GAUC"]


class GroupAUC(_KeyBuffer):
    """GAUC of one evaluate() call: one append launch per batch into a device buffer of 64-bit keys; `result()` does one finalize
    (sort + segmented reduction), one device->host copy of the header, one records launch and one copy of the records.  capacity:
    _KeyBuffer's rules.  group_bits: ids are valid in [0, 2^group_bits).
    Memory: 8 B per key + rsx_auc_group_workspace_bytes(n, group_bits) = round_up(8 n, 256) + round_up(1044 ceil(n / 4096) + 8192,
    256) + 16 ceil(n / 4096) B of workspace while result() runs + 32 B per mixed group for the records."""

    def __init__(self, device, group_bits, capacity=None):
        self.group_bits = int(group_bits)
        if not 1 <= self.group_bits <= 31:
            raise RsxError("group_auc: group_bits %d is outside 1..31" % self.group_bits)
        # out: [0..7] finalize's header; [8] the invalid examples the append launches counted
        super().__init__(device, "group_auc", torch.int64, lib().rsx_auc_group_max_keys(), capacity, 9)
        self.header = None                # the latest result()'s header, as Python integers

    def update(self, groups, labels, prob):
        """groups / labels / prob: device tensors or numpy arrays of B elements; groups may be a strided column view
        (ids[:, slot]).  No host synchronisation."""
        y, p = floats_on_device(labels, self.device), floats_on_device(prob, self.device)
        g, stride = group_column_on_device(groups, self.device)
        n = int(p.numel())
        if y.numel() != n or g.numel() != n:
            raise ValueError("groups, labels and predictions differ in size")
        if n == 0:
            return
        need = self._room_for(n)
        check(lib().rsx_auc_group_append(C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(g.data_ptr()), stride, n,
                                         self.group_bits, C.c_void_p(self.keys.data_ptr() + 8 * self.count),
                                         C.c_void_p(self.out.data_ptr() + 8 * 8),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rsx_auc_group_append")
        self.count = need

    def result(self, per_group=False):
        """-> {"GAUC", "groups", "mixed_groups", "skipped_examples", "invalid"}, plus "records" (uint64 [mixed_groups, 4] =
        (g, P_g, N_g, U2_g), ascending g) when per_group.  The key buffer keeps its multiset (sorted), so updates may continue."""
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ws = self._workspace_of(int(lib().rsx_auc_group_workspace_bytes(self.count, self.group_bits)))
        check(lib().rsx_auc_group_finalize(C.c_void_p(self.keys.data_ptr()), self.count, self.group_bits,
                                           C.c_void_p(ws.data_ptr()), int(ws.numel()),
                                           C.c_void_p(self.out.data_ptr()), stream), "rsx_auc_group_finalize")
        s = [int(v) for v in self.out.cpu().numpy()]
        if s[1] != s[8] or s[0] + s[1] != self.count or s[5] + s[6] != s[0] or s[3] > s[2]:
            raise RsxError("group_auc: the sorted keys hold %d positives, %d negatives and %d invalid examples of %d; the append "
                           "launches counted %d invalid" % (s[5], s[6], s[1], self.count, s[8]))
        rec = torch.zeros((s[3], 4), dtype=torch.int64, device=self.device)
        if s[3]:
            check(lib().rsx_auc_group_records(C.c_void_p(self.keys.data_ptr()), self.count, C.c_void_p(ws.data_ptr()),
                                              C.c_void_p(self.out.data_ptr()), C.c_void_p(rec.data_ptr()), s[3], stream),
                  "rsx_auc_group_records")
        rec = rec.cpu().numpy().view(np.uint64)
        self.header = s[:8]
        res = group_auc_from_records(rec, self.header)
        if per_group:
            res["records"] = rec
        return res


# ---- calibration: reliability bins, ECE / MCE / PCOC / NE and the same per group (include/rsx.h rsx_calibration_*) -------------
CALIBRATION_Q_ONE = 1 << 32             # the fixed-point 1.0 of q
_NAN = float("nan")


def calibration_bin_host(prob, n_bins):
    """The bin of every VALID fp32 probability: min(N - 1, int32(p * float32(N))) -- one fp32 multiply, rounded to nearest, then
    truncated.  The arithmetic is the definition: a p one ulp below k / N may land in bin k."""
    p = np.asarray(prob, np.float32)
    return np.minimum(np.int32(int(n_bins) - 1), (p * np.float32(int(n_bins))).astype(np.int32))


def calibration_q_host(prob):
    """The fixed-point form of every VALID fp32 probability: uint64(float64(p) * 2**32) -- the product is exact in fp64 and the
    conversion truncates; q(1.0) = 2**32.  A 64-bit sum of q is good for 2^31 examples."""
    return (np.asarray(prob, np.float32).astype(np.float64) * float(CALIBRATION_Q_ONE)).astype(np.uint64)


def _calibration_rows(index, rows, pos, q):
    table = np.zeros((rows, 3), np.int64)
    np.add.at(table[:, 0], index, 1)
    np.add.at(table[:, 1], index, pos.astype(np.int64))
    np.add.at(table[:, 2], index, q.astype(np.int64))
    return table


def calibration_bins_host(labels, prob, n_bins):
    """The documented definition of the bin table, in numpy.  An example is valid when 0 <= p <= 1 (exact_auc_keys_host's bit
    test, -0.0 as +0.0) and positive when y > 0.5: example_bits_host.
    -> (table int64 [n_bins, 3] = (count, positives, q_sum) per bin, the number of invalid examples).  The q sums are 64-bit
    integers, good for 2^31 examples."""
    n_bins = check_bins(n_bins)
    pos, u, valid = example_bits_host(labels, prob)
    pos, p = pos[valid], u[valid].view(np.float32)
    return _calibration_rows(calibration_bin_host(p, n_bins), n_bins, pos, calibration_q_host(p)), int(valid.size - valid.sum())


def calibration_groups_host(groups, labels, prob, n_groups):
    """The documented definition of the group table, in numpy: an example is valid when its probability is (as above) and its
    group id (any integer dtype, normalised by _group_ids_int32) lies in [0, n_groups).
    -> (table int64 [n_groups, 3] = (count, positives, q_sum) per group, the number of invalid examples)"""
    n_groups = int(n_groups)
    if n_groups < 1:
        raise ValueError("n_groups must be positive")
    pos, u, valid = example_bits_host(labels, prob)
    g = _group_ids_int32(groups).astype(np.int64)
    if g.size != u.size:
        raise ValueError("groups and predictions differ in size")
    valid = valid & (g >= 0) & (g < n_groups)
    pos, p, g = pos[valid], u[valid].view(np.float32), g[valid]
    return _calibration_rows(g, n_groups, pos, calibration_q_host(p)), int(valid.size - valid.sum())


def _calibration_rows_as_ints(table):
    t = np.asarray(table).reshape(-1, 3)
    return [int(v) for v in t[:, 0]], [int(v) for v in t[:, 1]], [int(v) for v in t[:, 2]]


def _exact_sum(a):
    """The sum of non-negative int64 values as a Python integer, whatever its size: the 32-bit halves are summed apart."""
    a = np.asarray(a, np.int64)
    return (int((a >> 32).sum(dtype=np.int64)) << 32) + int((a & 0xFFFFFFFF).sum(dtype=np.int64))


def calibration_from_table(table, invalid, loss=None):
    """THE place that divides, and it divides Python integers (each quotient correctly rounded).  table: [N, 3] = (count,
    positives, q_sum) per bin.  With n = sum(count), P = sum(positives), S = sum(q_sum), d_b = |q_sum_b - positives_b 2^32|:
    ECE = sum_b d_b / (n 2^32); MCE = max over non-empty bins of d_b / (count_b 2^32); PCOC = S / (P 2^32) (nan when P == 0);
    CTR = P / n; mean_prob = S / (n 2^32); NE = loss / H(CTR), H(c) = -(c ln c + (1 - c) ln(1 - c)) in Python floats (nan when
    loss is None or CTR is 0 or 1).  Everything is nan when n == 0.
    -> {"ECE", "MCE", "PCOC", "NE", "CTR", "mean_prob", "examples", "invalid"}"""
    import math
    cnt, pos, qs = _calibration_rows_as_ints(table)
    n, P, S, one = sum(cnt), sum(pos), sum(qs), CALIBRATION_Q_ONE
    res = {"ECE": _NAN, "MCE": _NAN, "PCOC": _NAN, "NE": _NAN, "CTR": _NAN, "mean_prob": _NAN, "examples": n,
           "invalid": int(invalid)}
    if n == 0:
        return res
    d = [abs(q - p * one) for p, q in zip(pos, qs)]
    res["ECE"] = sum(d) / (n * one)
    res["MCE"] = max(db / (c * one) for db, c in zip(d, cnt) if c)
    res["PCOC"] = S / (P * one) if P else _NAN
    res["CTR"] = ctr = P / n
    res["mean_prob"] = S / (n * one)
    if loss is not None and 0 < P < n:
        res["NE"] = float(loss) / -(ctr * math.log(ctr) + (1.0 - ctr) * math.log(1.0 - ctr))
    return res


def group_calibration_from_table(table, invalid):
    """The group table's figures, from Python integers: GCE = sum_g |q_sum_g - positives_g 2^32| / (n 2^32), the example-weighted
    absolute calibration error of the groups (nan when n == 0); GCE_groups = the non-empty groups.
    -> {"GCE", "GCE_groups", "examples", "invalid"}"""
    t = np.asarray(table).reshape(-1, 3).astype(np.int64)
    n, one = _exact_sum(t[:, 0]), CALIBRATION_Q_ONE
    if t.size and int(t[:, 1].max()) >= 1 << 31:                     # positives_g 2^32 would leave int64: Python integers
        d = sum(abs(int(q) - int(p) * one) for p, q in zip(t[:, 1], t[:, 2]))
    else:                                 # per group in int64, the sum over the groups exactly (it may pass 2^63)
        d = _exact_sum(np.abs(t[:, 2] - (t[:, 1] << 32)))
    return {"GCE": d / (n * one) if n else _NAN, "GCE_groups": int(np.count_nonzero(t[:, 0])), "examples": n,
            "invalid": int(invalid)}


CALIBRATION_FIGURES = ("ECE", "MCE", "PCOC", "NE", "CTR", "mean_prob")


def calibration_reported(res):
    """What evaluate() reports: the figures of a stream without invalid examples, nan for every figure otherwise (as
    exact_auc_reported).  -> {"ECE", "MCE", "PCOC", "NE", "CTR", "mean_prob"}"""
    return {k: (_NAN if res["invalid"] else res[k]) for k in CALIBRATION_FIGURES}


def group_calibration_reported(res):
    """-> {"GCE"}: nan when any example was invalid."""
    return {"GCE": _NAN if res["invalid"] else res["GCE"]}


class Calibration:
    """The calibration tables of one evaluate() call: one launch per batch (rsx_calibration_update, csrc/calibration.hip) adds
    the batch to a bin table (n_bins in 2..rsx_calibration_max_bins()) and / or a group table (n_groups in
    1..rsx_calibration_max_groups()); `result()` does ONE device->host copy.  Device state: 8 + 24 n_bins + 24 n_groups bytes,
    zeroed once here; no workspace.  An example is invalid, for both tables, when its probability is outside [0, 1] or, with a
    group table, its id outside [0, n_groups)."""

    def __init__(self, device, n_bins=None, n_groups=None):
        self.device = torch.device(device)
        self.n_groups = 0 if n_groups is None else int(n_groups)
        if n_bins is None and n_groups is None:
            raise RsxError("calibration: give n_bins, n_groups or both")
        self.n_bins = 0 if n_bins is None else check_bins(n_bins, "calibration: n_bins %d is outside %d..%d")
        if n_groups is not None and not 1 <= self.n_groups <= int(lib().rsx_calibration_max_groups()):
            raise RsxError("calibration: n_groups %d is outside 1..%d (the group table is 24 bytes per group)"
                           % (self.n_groups, int(lib().rsx_calibration_max_groups())))
        # [0] invalid examples; [1 .. 1 + 3 n_bins) the bin table; then the group table
        self.state = torch.zeros(1 + 3 * self.n_bins + 3 * self.n_groups, dtype=torch.int64, device=self.device)

    def update(self, labels, prob, groups=None):
        """labels / prob / groups: device tensors or numpy arrays of B elements (any shape); groups (needed with a group table,
        not read without one) may be a strided column view (ids[:, slot]), which is passed through in place.  No host
        synchronisation."""
        y, p = floats_on_device(labels, self.device), floats_on_device(prob, self.device)
        n = int(p.numel())
        if y.numel() != n:
            raise ValueError("labels and predictions differ in size")
        g, stride = None, 1
        if self.n_groups:
            if groups is None:
                raise ValueError("calibration: this object has a group table; update() needs the group ids")
            g, stride = group_column_on_device(groups, self.device)
            if g.numel() != n:
                raise ValueError("groups, labels and predictions differ in size")
        if n == 0:
            return
        base = self.state.data_ptr()
        check(lib().rsx_calibration_update(C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()),
                                           C.c_void_p(g.data_ptr() if g is not None else None), stride, n, self.n_bins,
                                           self.n_groups, C.c_void_p(base + 8 if self.n_bins else None),
                                           C.c_void_p(base + 8 + 24 * self.n_bins if self.n_groups else None), C.c_void_p(base),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rsx_calibration_update")

    def result(self, loss=None, per_group=False):
        """ONE device->host copy of the state.  With a bin table: calibration_from_table's dict (NE from `loss`) and "table", the
        int64 [n_bins, 3] array; with a group table: group_calibration_from_table's keys and, when per_group, "records": int64
        [G', 4] rows (g, count, positives, q_sum) of the non-empty groups in ascending g.  Updates may continue afterwards."""
        s = self.state.cpu().numpy()
        invalid, res = int(s[0]), {}
        if self.n_groups:
            gt = s[1 + 3 * self.n_bins:].reshape(self.n_groups, 3)
            live = np.flatnonzero(gt[:, 0])
            rec = np.concatenate([live.astype(np.int64).reshape(-1, 1), gt[live]], axis=1)
            res.update(group_calibration_from_table(rec[:, 1:], invalid))
            if per_group:
                res["records"] = rec
        if self.n_bins:
            table = s[1:1 + 3 * self.n_bins].reshape(self.n_bins, 3).copy()
            bins = calibration_from_table(table, invalid, loss)
            if self.n_groups and bins["examples"] != res["examples"]:
                raise RsxError("calibration: the bin table holds %d examples, the group table %d"
                               % (bins["examples"], res["examples"]))
            res.update(bins)
            res["table"] = table
        return res


# ---- isotonic calibration: equal-mass table, the fit and the map (include/rsx.h rsx_calibration_quantile_table, --------------
# ---- rsx_calibrate_apply) ---------------------------------------------------------------------------------------------------
ISOTONIC_MAX_KNOTS = 1024
ISOTONIC_FORMAT = "recsys_amd.isotonic_map.v1"


def quantile_table_host(labels, prob, n_bins):
    """The documented definition of the equal-mass, tie-aware table, in numpy.  ks = the sorted valid keys of
    exact_auc_keys_host, V of them; h(i) = the position of the first key with i's score; bin b(i) = (h(i) * M) // V in 64-bit
    integers.  All examples of one score share a bin, bins ascend with the score and may be empty.
    -> table int64 [n_bins, 3] = (count, positives, q_sum), calibration_bins_host's row and q."""
    M = check_bins(n_bins)
    ks, head, _ = sorted_valid_keys_host(labels, prob)
    V = int(ks.size)
    if V == 0:
        return np.zeros((M, 3), np.int64)
    score = ks >> np.uint32(1)
    h = np.maximum.accumulate(np.where(head, np.arange(V, dtype=np.int64), 0))
    b = (h * M) // V
    p = np.ascontiguousarray(score.astype(np.uint32)).view(np.float32)
    return _calibration_rows(b, M, (ks & np.uint32(1)) != 0, calibration_q_host(p))


def _isotonic_knot(block):
    c, s, q = block
    return float(np.float32(q / (c << 32))), float(np.float32(s / c))


def isotonic_from_table(table):
    """THE place that divides: the isotonic fit of a (count, positives, q_sum) table, over Python integers.  The non-empty rows,
    in order, are pushed as blocks (C, S, Q); while the last two violate STRICTLY -- S_prev C_last > S_last C_prev -- they are
    replaced by their sum (pool-adjacent-violators on a stack; equal means stay apart).  Knots x = float32(Q / (C << 32)),
    y = float32(S / C), true division of integers and then the rounding to fp32.  Two neighbours whose x are equal in fp32 are
    pooled and the knots taken again, until x ascends strictly.
    -> (x, y) float32 [K], 1 <= K <= rows, x strictly increasing, y non-decreasing.  An empty table raises ValueError."""
    cnt, pos, qs = _calibration_rows_as_ints(table)
    blocks = []
    for c, s, q in zip(cnt, pos, qs):
        if c == 0:
            continue
        blocks.append((c, s, q))
        while len(blocks) > 1 and blocks[-2][1] * blocks[-1][0] > blocks[-1][1] * blocks[-2][0]:
            (c1, s1, q1), (c0, s0, q0) = blocks.pop(), blocks.pop()
            blocks.append((c0 + c1, s0 + s1, q0 + q1))
    if not blocks:
        raise ValueError("isotonic_from_table: the table holds no example")
    while True:
        knots = [_isotonic_knot(b) for b in blocks]
        clash = next((j for j in range(len(knots) - 1) if knots[j][0] >= knots[j + 1][0]), None)
        if clash is None:
            break
        (c0, s0, q0), (c1, s1, q1) = blocks[clash], blocks[clash + 1]
        blocks[clash:clash + 2] = [(c0 + c1, s0 + s1, q0 + q1)]
    return np.array([k[0] for k in knots], np.float32), np.array([k[1] for k in knots], np.float32)


def _check_knots(x, y):
    """x, y as float32 [K] after IsotonicMap's checks (ValueError otherwise)."""
    x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
    y = np.ascontiguousarray(np.asarray(y, np.float32).reshape(-1))
    if x.size != y.size:
        raise ValueError("isotonic map: x has %d knots, y has %d" % (x.size, y.size))
    if not 1 <= x.size <= ISOTONIC_MAX_KNOTS:
        raise ValueError("isotonic map: %d knots are outside 1..%d" % (x.size, ISOTONIC_MAX_KNOTS))
    for name, v in (("x", x), ("y", y)):
        if not bool(np.all((v >= 0) & (v <= 1))):          # a NaN fails both comparisons
            raise ValueError("isotonic map: %s has a value outside [0, 1]" % name)
    if not bool(np.all(x[1:] > x[:-1])):
        raise ValueError("isotonic map: x is not strictly increasing")
    if not bool(np.all(y[1:] >= y[:-1])):
        raise ValueError("isotonic map: y decreases")
    return x, y


def isotonic_apply_host(p, x, y):
    """The documented definition of the map, in numpy fp32 -- bit for bit what rsx_calibrate_apply computes.  A p outside
    [0, 1] by example_bits_host's bit test is returned unchanged, bit for bit (-0.0 counts as +0.0); p <= x[0] -> y[0];
    p >= x[K-1] -> y[K-1]; otherwise with j the largest index with x[j] <= p:
    t = (p - x[j]) / (x[j+1] - x[j]); o = y[j] + t * (y[j+1] - y[j]); out = o if o < y[j+1] else y[j+1] -- every operation one
    fp32 operation rounded to nearest.  x must ascend strictly (not checked here).  -> float32, p's shape."""
    p = np.ascontiguousarray(np.asarray(p, np.float32))
    x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
    y = np.ascontiguousarray(np.asarray(y, np.float32).reshape(-1))
    K = int(x.size)
    if K < 1 or y.size != K:
        raise ValueError("isotonic map: x and y need the same number of knots, at least one")
    bits = p.reshape(-1).view(np.uint32)
    _, u, valid = example_bits_host(None, p)
    v = u[valid].view(np.float32)
    r = np.full(v.shape, y[0], np.float32)
    if K > 1:
        j = np.clip(np.searchsorted(x, v, side="right") - 1, 0, K - 2)
        x0, y0, y1 = x[j], y[j], y[j + 1]
        t = (v - x0) / (x[j + 1] - x0)
        o = y0 + t * (y1 - y0)
        r = np.where(o < y1, o, y1).astype(np.float32)
        r = np.where(v <= x[0], y[0], np.where(v >= x[K - 1], y[K - 1], r)).astype(np.float32)
    out = bits.copy()
    out[valid] = r.view(np.uint32)
    return out.view(np.float32).reshape(p.shape)


def _f32_bits(a):
    return [int(v) for v in np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)]


class IsotonicMap:
    """A fitted isotonic map: knots x (strictly increasing) and y (non-decreasing), float32 [K], 1 <= K <= 1024, all in [0, 1];
    bins = the M it was fitted with, examples = V, positives = P, global_step / script = the model it belongs to.  In memory only:
    table (the equal-mass table, int64 [M, 3]) and ece (its ECE by calibration_from_table) when evaluate() fitted it."""

    def __init__(self, x, y, bins=0, examples=0, positives=0, global_step=0, script="", table=None, ece=None):
        self.x, self.y = _check_knots(x, y)
        self.bins, self.examples, self.positives = int(bins), int(examples), int(positives)
        self.global_step, self.script = int(global_step), str(script)
        self.table, self.ece = table, ece

    @property
    def knots(self):
        return int(self.x.size)

    def to_json(self):
        """-> a dict for json.dump: the knots as fp32 bit patterns (x_bits / y_bits, what from_json reads) beside readable
        floats (x / y, never read back)."""
        return {"format": ISOTONIC_FORMAT, "script": self.script, "global_step": self.global_step, "bins": self.bins,
                "examples": self.examples, "positives": self.positives, "knots": self.knots,
                "x_bits": _f32_bits(self.x), "y_bits": _f32_bits(self.y),
                "x": [float(v) for v in self.x], "y": [float(v) for v in self.y]}

    @classmethod
    def from_json(cls, doc):
        """The map of to_json()'s dict (or its JSON text).  ValueError for: an unknown format, x and y of unequal length, K
        outside 1..1024, an x that does not increase strictly, a y that decreases, a value outside [0, 1]."""
        import json
        if isinstance(doc, (str, bytes)):
            doc = json.loads(doc)
        if not isinstance(doc, dict) or doc.get("format") != ISOTONIC_FORMAT:
            raise ValueError("isotonic map: unknown format %r" % (doc.get("format") if isinstance(doc, dict) else type(doc),))
        try:
            xb, yb = [int(v) for v in doc["x_bits"]], [int(v) for v in doc["y_bits"]]
        except (KeyError, TypeError) as e:
            raise ValueError("isotonic map: x_bits / y_bits are missing or not integers (%s)" % e)
        if len(xb) != len(yb):
            raise ValueError("isotonic map: x has %d knots, y has %d" % (len(xb), len(yb)))
        if any(not 0 <= v <= 0xFFFFFFFF for v in xb + yb):
            raise ValueError("isotonic map: a bit pattern is outside 32 bits")
        x, y = np.array(xb, np.uint32).view(np.float32), np.array(yb, np.uint32).view(np.float32)
        return cls(x, y, doc.get("bins", 0), doc.get("examples", 0), doc.get("positives", 0), doc.get("global_step", 0),
                   doc.get("script", ""))

    def save(self, path):
        """to_json() to `path`, written under a temporary name and renamed."""
        import json
        import os
        tmp = "%s.tmp.%d" % (path, os.getpid())
        with open(tmp, "w") as f:
            json.dump(self.to_json(), f)
            f.write("\n")
        os.replace(tmp, path)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls.from_json(f.read())

    def apply_host(self, p):
        return isotonic_apply_host(p, self.x, self.y)


class Calibrator:
    """An IsotonicMap held on the device (8 bytes per knot).  `apply` is ONE launch of rsx_calibrate_apply on the current stream;
    nothing is allocated when `out` is given, so the call can be captured into a graph."""

    def __init__(self, device, map):
        self.device = torch.device(device)
        self.map = map
        self.x = torch.from_numpy(map.x.copy()).to(self.device)
        self.y = torch.from_numpy(map.y.copy()).to(self.device)

    def apply(self, prob, out=None):
        """prob: a float32 device tensor (contiguous, any shape) or a numpy array.  -> the mapped probabilities: `out` (a device
        tensor of the same size; it may be `prob` itself) or a new tensor for a tensor, a numpy array for a numpy array."""
        host = not isinstance(prob, torch.Tensor)
        if host:
            shape = np.asarray(prob).shape
            prob = torch.from_numpy(np.ascontiguousarray(np.asarray(prob, np.float32)).reshape(-1).copy()).to(self.device)
        if not (prob.is_cuda and prob.dtype == torch.float32 and prob.is_contiguous()):
            raise ValueError("calibrate: prob must be a contiguous float32 device tensor (or a numpy array)")
        if out is None:
            out = torch.empty_like(prob)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                  and out.numel() == prob.numel()):
            raise ValueError("calibrate: out must be a contiguous float32 device tensor of prob's size")
        if prob.numel():                  # (an empty tensor has no address to pass)
            check(lib().rsx_calibrate_apply(C.c_void_p(self.x.data_ptr()), C.c_void_p(self.y.data_ptr()), int(self.x.numel()),
                                            C.c_void_p(prob.data_ptr()), C.c_void_p(out.data_ptr()), int(prob.numel()),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rsx_calibrate_apply")
        return out.cpu().numpy().reshape(shape) if host else out
