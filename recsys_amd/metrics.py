"""Streaming eval metrics on device: tf.metrics.auc (200 thresholds, trapezoidal
ROC), tf.metrics.accuracy(labels, tf.round(pred)) and the Estimator's mean of the batch losses, as the
eval_metric_ops of fm/fm.py:150-153 and Estimator.evaluate(steps=200) fm/fm.py:221 produce them.

One HIP launch per eval batch (`rsx_eval_metrics_update`, csrc/metrics.hip) accumulates everything in a 406-word
device buffer; the host reads it back ONCE in `result()` -- evaluate() never synchronises per batch.  Data-parallel
evaluation sums the integer counters of all ranks before the finalisation (`all_reduce`).

Opt-in beside it (RunConfig.exact_auc): `ExactAUC`, the exact tie-aware rank statistic (sklearn's roc_auc_score, which the
reference's serving client reports, deepfm/grpc_client.py:84) from a device-wide key sort (csrc/auc_exact.hip); `exact_auc_host`
states its definition in numpy."""
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


# ---- exact, tie-aware ROC AUC (include/rsx.h rsx_auc_exact_*) -----------------------------------------------------------------
EXACT_AUC_PAD = 0xFFFFFFFF


def exact_auc_keys_host(labels, prob):
    """The 32-bit keys of rsx_auc_exact_append: (bits(p) << 1) | (label > 0.5) for 0 <= p <= 1 (-0.0 as +0.0), else the padding
    key.  The fp32 pattern is taken as an integer, never passed through arithmetic."""
    y = np.ascontiguousarray(np.asarray(labels, np.float32).reshape(-1))
    p = np.ascontiguousarray(np.asarray(prob, np.float32).reshape(-1))
    if y.size != p.size:
        raise ValueError("labels and predictions differ in size")
    u = p.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    valid = u <= 0x3F800000
    pos = (y > np.float32(0.5)).astype(np.uint32)
    return np.where(valid, (u << np.uint32(1)) | pos, np.uint32(EXACT_AUC_PAD)).astype(np.uint32)


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
    keys = exact_auc_keys_host(labels, prob)
    ks = np.sort(keys[keys != EXACT_AUC_PAD])
    invalid = int(keys.size - ks.size)
    neg = (ks & 1) == 0
    c = np.cumsum(neg, dtype=np.int64) - neg                         # exclusive
    score = ks >> 1
    head = np.ones(ks.size, bool)
    head[1:] = score[1:] != score[:-1]
    h = np.maximum.accumulate(np.where(head, c, 0)) if ks.size else c
    u2 = int(np.sum((c + h)[~neg], dtype=np.int64))
    return exact_auc_from_counts(u2, int((~neg).sum()), int(neg.sum()), invalid)


def exact_auc_reported(res):
    """What evaluate() reports as "AUC_exact": the statistic of a stream without invalid examples, nan otherwise (a model that
    emits a NaN or a probability outside [0, 1] has no AUC worth a number; the count goes into a WARNING line)."""
    return float("nan") if res["invalid"] else res["AUC_exact"]


def check_exact_auc_world(world):
    """exact_auc is a single-replica evaluation: the ranks' keys would have to be sorted together."""
    if int(world) > 1:
        raise RsxError("exact_auc: data-parallel evaluation is not supported (the ranks' keys would have to be sorted together); "
                       "evaluate on one replica")


class ExactAUC:
    """Exact ROC AUC of one evaluate() call: one append launch per batch into a device key buffer, one sort + reduction and
    ONE device->host copy in `result()`.  capacity (examples): fixed when given (an update past it raises); otherwise the buffer
    grows by doubling, with a device copy and no synchronisation.  Memory: 4 B per key + rsx_auc_exact_workspace_bytes(n) =
    4 n + 1032 ceil(n / 4096) + 4096 B while result() runs."""
    GROW_FROM = 1 << 16

    def __init__(self, device, capacity=None):
        self.device = torch.device(device)
        self.fixed = capacity is not None
        self.max_keys = int(lib().rsx_auc_exact_max_keys())
        cap = max(1, int(capacity)) if self.fixed else self.GROW_FROM
        if cap > self.max_keys:
            raise RsxError("exact_auc: capacity %d is above the %d keys one sort takes" % (cap, self.max_keys))
        self.keys = torch.empty(cap, dtype=torch.int32, device=self.device)
        self.count = 0
        # [0..3] finalize's {U2, P, N, invalid}; [4] the invalid examples the append launches counted
        self.out = torch.zeros(5, dtype=torch.int64, device=self.device)
        self.workspace = None

    def _as_device(self, x):
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
        return x.to(self.device).reshape(-1).to(torch.float32).contiguous()

    def update(self, labels, prob):
        """labels / prob: device tensors or numpy arrays of B elements (any shape).  No host synchronisation."""
        y, p = self._as_device(labels), self._as_device(prob)
        n = int(p.numel())
        if y.numel() != n:
            raise ValueError("labels and predictions differ in size")
        if n == 0:
            return
        need = self.count + n
        if need > self.keys.numel():
            if self.fixed or need > self.max_keys:
                raise RsxError("exact_auc: %d examples do not fit the key buffer of %d"
                               % (need, self.keys.numel() if self.fixed else self.max_keys))
            grown = torch.empty(min(self.max_keys, max(2 * self.keys.numel(), need)), dtype=torch.int32, device=self.device)
            grown[:self.count].copy_(self.keys[:self.count])
            self.keys = grown
        check(lib().rsx_auc_exact_append(C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()), n,
                                         C.c_void_p(self.keys.data_ptr() + 4 * self.count),
                                         C.c_void_p(self.out.data_ptr() + 8 * 4),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rsx_auc_exact_append")
        self.count = need

    def result(self):
        """-> {"AUC_exact", "u2", "positives", "negatives", "invalid"}; one finalize, ONE device->host copy.  The key buffer keeps
        its multiset (sorted), so updates may continue afterwards."""
        need = int(lib().rsx_auc_exact_workspace_bytes(self.count))
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        check(lib().rsx_auc_exact_finalize(C.c_void_p(self.keys.data_ptr()), self.count, C.c_void_p(self.workspace.data_ptr()),
                                           int(self.workspace.numel()), C.c_void_p(self.out.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rsx_auc_exact_finalize")
        s = [int(v) for v in self.out.cpu().numpy()]
        if s[3] != s[4] or s[1] + s[2] + s[3] != self.count:
            raise RsxError("exact_auc: the sorted keys hold %d positives, %d negatives and %d invalid examples of %d; the append "
                           "launches counted %d invalid" % (s[1], s[2], s[3], self.count, s[4]))
        return exact_auc_from_counts(s[0], s[1], s[2], s[3])
