"""Factorization Machine on the Criteo 39-field pipeline -- MI355X-native mirror of `fm/fm.py`
(model_fn :115-170, build_feature_columns :47-97, flags :16-37; BASELINE config 1, the plumbing model).

logits = dense([relu(first_order), fm_second_order], 1).  The whole model is the fused embedding kernels
(gather + first-order + FM forward, sorted segment-sum backward) plus a 2->1 dense head.
"""
import ctypes as C

import torch

from . import _lib
from . import fused_step
from . import layers as L
from .deepfm import build_variables as _build
from .deepfm import define_flags, input_fn, make_params, run_main  # noqa: F401
from .estimator import EstimatorSpec, ModeKeys, get_variable_store
from .ops import _ptr, _stream, gather_fm


def model_fn(features, labels, mode, params):
    """fm/fm.py:115-170."""
    store = get_variable_store()
    ids = features["ids"]
    if not store.built:
        cap = max(int(params.get("max_batch_size", 0)), ids.shape[0])
        _build(store, params, capacity=cap, with_dnn=False)
        store.dp_block = False
        if params.get("fused", True):
            # data-parallel send block: [S | gy2 | gy1] per example, or [G | gw1] per packed unique row
            a0 = store.embeddings["input_layer"]
            fused_step.configure(store, params, [a0], cap * (store.dp.world if store.dp is not None else 1), [a0.D, 1, 1],
                                 [a0.D, 1], windows=store.adam_mode == "tf1_dense", send_block=True)
    arena, P = store.embeddings["input_layer"], store.dense
    training = mode == ModeKeys.TRAIN
    if training and store.adam_mode == "tf1_dense" and params.get("fused", True) and (store.dp is None or store.dp_block):
        return _train_fused(store, arena, ids, labels)
    if not training and store.adam_mode == "tf1_dense" and params.get("fused", True) and params.get("fused_infer", True) \
            and not torch.is_grad_enabled():
        # EVAL / PREDICT: gather + the FM head kernel of the TRAIN step (its gradients go to scratch)
        B = ids.shape[0]
        dev = ids.device
        _, _, y1p, y2 = arena.gather(ids, fm=True, first_order=True)
        lab = torch.zeros(B, device=dev) if (labels is None or mode == ModeKeys.PREDICT) else labels.reshape(-1).to(torch.float32)
        prob, loss = torch.empty(B, device=dev), torch.empty(1, device=dev)
        scr = torch.empty(2 * B + 4, device=dev)
        _lib.check(_lib.lib().rsx_fm_head(_ptr(y1p), _ptr(y2), _ptr(P["b1"]), _ptr(P["out.W"].detach().view(-1)), _ptr(P["out.b"]),
                                          _ptr(lab), _ptr(prob), _ptr(scr[:B]), _ptr(scr[B:2 * B]), _ptr(scr[2 * B:2 * B + 2]),
                                          _ptr(scr[2 * B + 2:2 * B + 3]), _ptr(scr[2 * B + 3:]), _ptr(loss), 1.0 / B, B, None,
                                          _stream()), "rsx_fm_head")
        predictions = {"prob": prob}
        if mode == ModeKeys.PREDICT:
            return EstimatorSpec(mode, predictions=predictions, export_outputs={"serving_default": predictions})
        return EstimatorSpec(mode, predictions=predictions, loss=loss[0], eval_metric_ops={"AUC": None, "Accuracy": None})
    if training:
        store.sort_ids_for_backward(arena, ids)
    _, y1p, y2 = gather_fm(arena, ids, fm=True, first_order=True, dp=store.dp if training else None)
    y_1d = torch.relu(y1p + P["b1"])                                               # 'linear_net' (:120-121)
    logits = L.dense(torch.stack([y_1d, y2], -1), P["out.W"], P["out.b"])          # (:131-132)  [B,1]
    pred = torch.sigmoid(logits)
    predictions = {"prob": pred}
    if mode == ModeKeys.PREDICT:
        return EstimatorSpec(mode, predictions=predictions, export_outputs={"serving_default": predictions})
    loss = L.sigmoid_ce_mean(logits, labels)
    if mode == ModeKeys.EVAL:
        return EstimatorSpec(mode, predictions=predictions, loss=loss, eval_metric_ops={"AUC": None, "Accuracy": None})
    return EstimatorSpec(mode, predictions=predictions, loss=loss, train_op=lambda: store.minimize(loss))


def _train_fused(store, arena, ids, labels):
    """TRAIN step as 4 launches, no autograd: dedup sort -> gather (+ first order + FM) -> FM head with its backward,
    carrying most of the untouched-row Adam sweep as extra workgroups -> segment-sum fused with the touched-row and dense
    Adam (+ the rest of the sweep).  The exact split of the TF-1 update and the scheduling around these launches:
    fused_step.py."""
    P, dp = store.dense, store.dp
    B = ids.shape[0]
    dev = ids.device
    with torch.no_grad():
        # (this path is the split TF-1 update by construction: model_fn takes it under adam_mode tf1_dense only)
        plan = fused_step.begin(store, [arena], ids, split=True)
        fused_step.sort_ids(plan)
        fused_step.sort_now(plan)
        # 70 % of the untouched-row sweep rides in the head launch, 30 % (table blocks only: the first-order vector goes
        # first) in the scatter + touched-row Adam launch (measured: 76.4 -> 72.2 us per step)
        fused_step.split_update(plan, [0.7, 0.3], 1)
        ux = plan.ux
        sweep = plan.sweeps[0] if plan.sweeps is not None else None
        Sv, gy2v, gy1v = dp.send_views(B) if (dp is not None and not ux) else (None,) * 3
        prob = torch.empty(B, device=dev)
        gy1, gy2 = (gy1v, gy2v) if (dp is not None and not ux) else (torch.empty(B, device=dev) for _ in range(2))
        oW, oG = P["out.W"].detach().view(-1), P["out.W"].grad.view(-1)
        world = dp.world if dp is not None else 1
        lab = labels.reshape(-1).to(torch.float32)
        # round 4: forward AND head in ONE launch (rsx_gather_fm_head: 3.25 -> 2.25 launches per step).  Every example leaves its
        # contribution to the four dense gradients as a row of `terms` in the dense arena's layout; the optimizer launch adds
        # the rows in example order (an RSX_ADAM_DENSE segment with B = batch "replicas"), the loss is read from the terms when
        # somebody asks (estimator.LazyMeanLoss).  Single replica, windows on (no sweep slice to carry); RSX_FM_FUSE=0: two launches.
        terms_on = dp is None and _lib.form("fm_fuse") != "0" and P.n + 1 <= 64
        fuse = terms_on and sweep is None
        terms, loss = None, None
        if terms_on:
            stride = (P.n + 1 + 3) & ~3
            terms = torch.empty((B + 15) // 16, stride, device=dev)      # rows of 16 examples, pre-added in example order
            from .estimator import LazyMeanLoss
            loss = LazyMeanLoss(terms, P.n, B)
        if fuse:
            S = torch.empty(B, arena.D, device=dev)
            _lib.check(_lib.lib().rsx_gather_fm_head(
                _ptr(arena.tables), _ptr(arena.w1), _ptr(arena.row_off), _ptr(ids), _ptr(S), arena.w1_mask, _ptr(P["b1"]), _ptr(oW),
                _ptr(P["out.b"]), _ptr(lab), _ptr(prob), _ptr(gy1), _ptr(gy2), _ptr(terms), stride, P.n, P.offsets["b1"],
                P.offsets["out.W"], P.offsets["out.b"], 1.0 / (B * world), B, arena.F, arena.D, _stream()), "rsx_gather_fm_head")
        else:
            # two launches: a sweep slice rides in the head launch (every step on its own), or data parallel.  Single replica:
            # the head leaves the same per-example terms as the fused launch, so both schedules train the same bits.
            E, S, y1p, y2 = arena.gather(ids, fm=True, first_order=True, S_out=Sv)
            if terms is None:
                loss = torch.empty(1, device=dev)
            _lib.check(_lib.lib().rsx_fm_head_terms(
                _ptr(y1p), _ptr(y2), _ptr(P["b1"]), _ptr(oW), _ptr(P["out.b"]), _ptr(lab), _ptr(prob), _ptr(gy1), _ptr(gy2),
                _ptr(oG), _ptr(P["out.b"].grad), _ptr(P["b1"].grad), _ptr(loss) if terms is None else None, _ptr(terms),
                stride if terms is not None else 0, P.n, P.offsets["b1"], P.offsets["out.W"], P.offsets["out.b"],
                1.0 / (B * world), B, None if sweep is None else C.byref(sweep), _stream()), "rsx_fm_head_terms")

        grads = [(S, None, gy1, gy2)]
        fused_step.local_sums(plan, grads)

    def train_op():
        with torch.no_grad():
            dense_segs = None
            if terms is not None:       # the head's dense gradients: the examples' rows, summed in example order by the launch
                dense_segs = [dict(kind=_lib.RSX_ADAM_DENSE, n=P.n, var=P.flat, m=P.m, v=P.v, g=terms, B=terms.shape[0],
                                   stride=terms.shape[1], zero_grad=0)]
            fused_step.finish(plan, grads, dense_segs=dense_segs)

    return EstimatorSpec(ModeKeys.TRAIN, predictions={"prob": prob}, loss=loss if terms is not None else loss[0],
                         train_op=train_op)


def main(argv=None):
    FLAGS = define_flags().parse_args(argv)
    FLAGS._argv = argv
    return run_main(model_fn, FLAGS, make_params)


if __name__ == "__main__":
    main()
