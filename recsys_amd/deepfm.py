"""DeepFM on the Criteo 39-field pipeline -- MI355X-native mirror of the reference's
`deepfm/deepfm.py:model_fn` (:73-150) married to `fm/fm.py:build_feature_columns` (:47-97), i.e. the
README's "DeepFM on Criteo, d=16, DNN 100-100, bs=256" (BASELINE config 2).

Same surface as the script: FLAGS-compatible argparse names, `input_fn`, `model_fn(features, labels,
mode, params)`, `main`.  The embedding gather + first-order + FM term, the row-wise gradient scatter
and the TF-1 Adam sweep are librsx.so kernels; the 624-100-100-1 tower is rocBLAS via torch.
"""
import argparse
import os

import torch

from . import _lib
from . import fused_step
from . import layers as L
from .dist import dp_overlap_enabled as dist_overlap_enabled, overlap_ranges as dist_overlap_ranges
from .estimator import Estimator, EstimatorSpec, EvalSpec, ModeKeys, RunConfig, TrainSpec, get_variable_store, \
    train_and_evaluate
from .feature_columns import CAT_FEATURE, CONT_FEATURE, CriteoLayout, build_feature_columns
from .ops import EmbeddingArena, gather_fm


def _dense_specs(F, D, layers, n_inputs_out, with_dnn=True):
    """Variable shapes + initialisers (glorot-uniform kernels, zero biases, BN gamma 1 / beta 0: Appendix A-7)."""
    shapes, init = {}, {}
    zeros = lambda t, g: t.zero_()

    def add_dense(name_w, name_b, fi, fo):
        shapes[name_w], shapes[name_b] = (fi, fo), (fo,)
        init[name_w] = lambda t, g, fi=fi, fo=fo: L.glorot_uniform_(t, fi, fo, g)
        init[name_b] = zeros

    shapes["b1"], init["b1"] = (1,), zeros
    if with_dnn:
        add_dense("dnn.Wout", "dnn.bout", fused_step.tower_specs(shapes, init, F * D, layers), 1)
    add_dense("out.W", "out.b", n_inputs_out, 1)
    return shapes, init


def build_variables(store, params, capacity, with_dnn=True):
    """Creates what TF creates lazily inside input_layer / tf.layers.* on the first model_fn call."""
    layout = CriteoLayout.from_columns(params["embedding_feature_columns"])
    D = params["embedding_size"]
    lin_keys = {c.key for c in params["linear_feature_columns"] if c.kind.endswith("indicator")}
    if store.dp is not None:
        capacity *= store.dp.world                              # the sort/scatter workspace holds the global batch
    arena = EmbeddingArena(layout.row_off, D, capacity, store.device, with_w1=True,
                           w1_field_mask=layout.field_mask(lin_keys))
    with torch.no_grad():
        t = torch.empty(arena.R, D)
        L.trunc_normal_(t, 1.0 / D ** 0.5, store.gen)          # embedding_column initializer (A-4)
        arena.tables.copy_(t)
        w = torch.empty(arena.R)
        L.glorot_uniform_(w, arena.R, 1, store.gen)             # tf.layers.dense kernel [R,1]
        arena.w1.copy_(w)
    layers = list(map(int, params["deep_layers"].split(","))) if with_dnn else []
    shapes, init = _dense_specs(layout.F, D, layers, 3 if with_dnn else 2, with_dnn)
    store.build({"input_layer": arena}, shapes, init, params["learning_rate"])
    store.layout = layout
    store.tower = fused_step.fused_tower(store, params, layout.F * D, layers, capacity) if with_dnn else None
    if store.tower is not None:
        # send block: [dX | S | gy2 | gy1] per example, or [G | gw1] per packed unique row.
        # share of the untouched-row Adam sweep carried by [fwd_0.., head, bwd_{L-1}..bwd_0, scatter] (measured: the
        # latency-bound scatter + touched-row Adam launch hides a quarter of the sweep; r02 grid over the shares with the faster
        # head kernel: [0,0,2,3,3,2] 93.2 us, [0,0,1,3.5,3.5,2.5] 91.4 us per step)
        fused_step.configure(store, params, [arena], capacity, [layout.F * D, D, 1, 1], [D, 1],
                             windows=store.adam_mode == "tf1_dense" and bool(params.get("overlap_adam", True)),
                             send_block=params.get("dp_send_block", True),
                             default_sweep_weights=[0.0] * len(layers) + [1.0] + [3.5] * len(layers) + [2.5])


def model_fn(features, labels, mode, params):
    """deepfm/deepfm.py:73-150.  features['ids']: int32 [B,39] table-local ids in slot order
    (recsys_amd.input_pipeline produces them; hashing/bucketizing is the input_layer's host half)."""
    store = get_variable_store()
    ids = features["ids"]
    if not store.built:
        build_variables(store, params, capacity=max(int(params.get("max_batch_size", 0)), ids.shape[0]))
    arena, P = store.embeddings["input_layer"], store.dense
    training = mode == ModeKeys.TRAIN
    n_layers = len(params["deep_layers"].split(","))
    masks = params.get("_dropout_masks")

    if training and getattr(store, "tower", None) is not None:
        return _train_fused(store, arena, ids, labels, params, masks)
    if not training and getattr(store, "tower", None) is not None and params.get("fused_infer", True) \
            and not torch.is_grad_enabled() and ids.shape[0] <= store.tower.cap:
        # EVAL / PREDICT through the TRAIN step's kernels (gather + 2 tower launches + head: 4 launches instead of ~70
        # framework ones; BN in inference form, dropout off -- FusedTower.infer)
        E, _, y1p, y2 = arena.gather(ids, fm=True, first_order=True)
        lab = None if (labels is None or mode == ModeKeys.PREDICT) else labels.reshape(-1).to(torch.float32)
        prob, loss = store.tower.infer(E, store.opt.state.view(torch.int32)[3:4], lab, s0=y1p, c0="b1", s1=y2)
        predictions = {"prob": prob}
        if mode == ModeKeys.PREDICT:
            return EstimatorSpec(mode, predictions=predictions, export_outputs={"serving_default": predictions})
        return EstimatorSpec(mode, predictions=predictions, loss=loss[0], eval_metric_ops={"AUC": None, "Accuracy": None})
    if training:
        store.sort_ids_for_backward(arena, ids)                # dedup for the sparse gradient (ids only)
    E, y1p, y2 = gather_fm(arena, ids, fm=True, first_order=True, dp=store.dp if training else None)
    y_1d = torch.relu(y1p + P["b1"])                           # 'first-order' (:90-91)
    dnn_net = L.tower(E, P, "dnn", n_layers, training, params["dropout"], masks)    # 'dnn' (:100-107)
    y_dnn = L.dense(dnn_net, P["dnn.Wout"], P["dnn.bout"], relu=True)              # (:108)
    logits = torch.cat([y_1d[:, None], y2[:, None], y_dnn], -1)                     # (:110)
    logits = L.dense(logits, P["out.W"], P["out.b"]).reshape(-1)                    # (:111-112)
    pred = torch.sigmoid(logits)
    predictions = {"prob": pred}
    if mode == ModeKeys.PREDICT:
        return EstimatorSpec(mode, predictions=predictions, export_outputs={"serving_default": predictions})
    loss = L.sigmoid_ce_mean(logits, labels)
    if mode == ModeKeys.EVAL:
        return EstimatorSpec(mode, predictions=predictions, loss=loss, eval_metric_ops={"AUC": None, "Accuracy": None})

    def train_op():                                            # AdamOptimizer.minimize (:142-143)
        store.minimize(loss)

    return EstimatorSpec(mode, predictions=predictions, loss=loss, train_op=train_op)


def _train_fused(store, arena, ids, labels, params, masks):
    """TRAIN step with no autograd, 7 launches: gather_fm -> tower forward x2 (the first carries the dedup sort) -> head +
    loss (+ a slice of the untouched-row Adam sweep) -> tower backward x2 (+ sweep slices) -> [train_op:] sorted
    segment-sum fused with the touched-row and dense-variable Adam.  Data-parallel: two all-gathers (ids; gradient block
    + dense arena) around the same launches.  The scheduling around these launches is fused_step's."""
    dp = store.dp
    with torch.no_grad():
        overlap = store.adam_mode == "tf1_dense" and bool(params.get("overlap_adam", True))
        plan = fused_step.begin(store, [arena], ids, split=overlap)
        fused_step.sort_ids(plan)
        ux, zc = plan.ux, plan.zc
        nl = len(store.tower.widths)
        if ux:      # (the unique-list exchange runs a window's sweep with its ids phase)
            fused_step.split_update(plan, store.sweep_weights, 2 * nl + 1)
        dXv, Sv, gy2v, gy1v = dp.send_views(ids.shape[0]) if zc else (None,) * 4
        # RSX_SORT_IN_GATHER=1: the sort rides in the GATHER launch (the step's first) instead, so that both tower-forward
        # launches may carry sweep slices too.  Measured (r02, MI355X): the same 93.4 us with the forward shares at 0, and
        # 106-108 us with any share given to the forward launches ([1,1,1,3,3,2.5] ...): a forward launch is a pure chain of
        # dependent L2 accesses and stretches by more than the slice it hides.  So the default stays the r01 form.
        rides = fused_step.sort_rides(plan)
        in_gather = rides and overlap and _lib.form("sort_in_gather") == "1"
        # round 4: the gather itself rides in the first tower-forward launch (E tiles gathered straight into LDS as the MFMA
        # A operand, rsx_gather_tower_fwd0): one launch less on the step's dependent chain
        fuse_gather = not in_gather and store.tower.fused_gather_ok(arena, ids.shape[0])
        if fuse_gather:
            E, S, y1p, y2 = arena.gather_outputs(ids.shape[0], fm=True, first_order=True, S_out=Sv)
        else:
            E, S, y1p, y2 = arena.gather(ids, fm=True, first_order=True, S_out=Sv, sort_job=plan.job if in_gather else None)
        if in_gather:
            plan.job = None
        elif not rides:
            fused_step.sort_now(plan)
        if not ux:
            fused_step.split_update(plan, store.sweep_weights, 2 * nl + 1)
        assert plan.job is None or plan.sweeps is None or plan.sweeps[0] is None, \
            "a forward launch that carries the sort cannot carry a sweep slice"
        # RSX_DP_OVERLAP=1 (opt-in): the dense arena is all-reduced per tower layer from inside backward, on RCCL's stream
        pending, layer_done = None, None
        if zc and dist_overlap_enabled():
            per_layer, rest = dist_overlap_ranges(
                store.dense, [[f"dnn.{v}{l}" for v in ("W", "b", "gamma", "beta")] for l in range(nl)])
            g = store.dense.grad
            pending = []

            def layer_done(l):
                for lo, hi in ([per_layer[l]] + (rest if l == nl - 1 else [])):
                    pending.append(dp.all_reduce_async(g[lo:hi]))
        loss, prob, dX, gy1, gy2 = store.tower.train_step(
            E, labels.reshape(-1).to(torch.float32), params["dropout"], store.opt.state.view(torch.int32)[3:4],
            s0=y1p, c0="b1", s1=y2, masks=masks, **fused_step.replica_args(dp),
            sort_job=plan.job, sweeps=plan.sweeps, sort_in_fwd=overlap, outs=(dXv, gy1v, gy2v) if zc else None,
            layer_done=layer_done, gather=(arena, ids, S, y1p, y2) if fuse_gather else None)
        grads = [(S, dX, gy1, gy2)]
        fused_step.local_sums(plan, grads)

    def train_op():
        with torch.no_grad():
            fused_step.finish(plan, grads, pending=pending)

    return EstimatorSpec(ModeKeys.TRAIN, predictions={"prob": prob}, loss=loss[0], train_op=train_op)


# ---- driver (deepfm/deepfm.py:153-234 + fm/fm.py flags) -----------------------------------------
def define_flags(p=None):
    p = p or argparse.ArgumentParser()
    p.add_argument("--embedding_size", type=int, default=16)
    p.add_argument("--learning_rate", type=float, default=0.001)
    p.add_argument("--dropout", type=float, default=0.5)
    p.add_argument("--task_type", default="train", help="{train, infer, eval, export}")
    p.add_argument("--export_path", default="./export/",
                   help="--task_type export: the latest checkpoint of --model_dir goes to <export_path>/<unix seconds>/")
    p.add_argument("--export_table_dtype", default="float32", choices=("float32", "bfloat16", "float16"),
                   help="--task_type export: how the bundle stores the embedding tables.  A 16-bit dtype rounds them (to nearest "
                        "even), halves the bundle and the tables a fused-path Predictor keeps on the device, and moves the "
                        "probabilities by 1e-4 to 1e-2; first-order weights and dense tensors stay float32")
    p.add_argument("--num_epochs", type=int, default=10)
    p.add_argument("--deep_layers", default="100,100")
    p.add_argument("--train_path", default="/home/wangrc/criteo_data/train/")
    p.add_argument("--train_parts", type=int, default=150)
    p.add_argument("--eval_parts", type=int, default=5)
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--log_steps", type=int, default=100)
    p.add_argument("--save_checkpoints_steps", type=int, default=1000)
    p.add_argument("--num_parallel", type=int, default=8)
    p.add_argument("--mirror", type=lambda s: s.lower() in ("1", "true", "yes"), default=True)
    p.add_argument("--model_dir", default="./model/")
    p.add_argument("--adam_mode", default="tf1_dense")
    p.add_argument("--adam_window", type=int, default=0,
                   help="steps per optimizer window (include/rsx.h rsx_adam_window; bit-identical to single steps): 0 = the "
                        "model's default (8 up to batch 1024, 4 above), 1 = every step on its own")
    # tf.train.AdagradOptimizer / FtrlOptimizer in place of AdamOptimizer (their TF argument names and defaults)
    p.add_argument("--optimizer", default="adam", choices=["adam", "adagrad", "ftrl"])
    p.add_argument("--initial_accumulator_value", type=float, default=0.1)
    p.add_argument("--learning_rate_power", type=float, default=-0.5, help="ftrl")
    p.add_argument("--l1_regularization_strength", type=float, default=0.0, help="ftrl")
    p.add_argument("--l2_regularization_strength", type=float, default=0.0, help="ftrl")
    p.add_argument("--l2_shrinkage_regularization_strength", type=float, default=0.0, help="ftrl")
    p.add_argument("--device_parse", type=lambda s: s.lower() in ("1", "true", "yes"), default=False,
                   help="parse the TFRecord shards on the GPU (input_pipeline.criteo_input_fn(device_parse=True)): the host ships "
                        "raw shard bytes; same batches, same bits.  Single-replica fm.py / deepfm.py / dcn.py with the Criteo "
                        "feature set only")
    p.add_argument("--exact_auc", type=lambda s: s.lower() in ("1", "true", "yes"), default=False,
                   help="evaluate() also reports AUC_exact, the exact tie-aware ROC AUC (sklearn's roc_auc_score, "
                        "deepfm/grpc_client.py:84) from a key sort on the GPU; the 200-threshold AUC stays as it is.  Single "
                        "replica only")
    p.add_argument("--group_auc_key", default=None,
                   help="evaluate() also reports GAUC, the exact AUC of every group's examples weighted by the group's examples "
                        "(the DIN paper's per-user AUC): the source key of an embedding column, e.g. u_id with --feature_set "
                        "uid_iid or _c14 with the Criteo set.  Single replica only")
    p.add_argument("--calibration_bins", type=int, default=0,
                   help="evaluate() also reports ECE, MCE, PCOC (predicted over observed CTR) and NE (normalized entropy) from a "
                        "reliability table of this many equal-width bins (2..1024), binned on the GPU; 0: off.  Single replica "
                        "only")
    p.add_argument("--calibration_key", default=None,
                   help="evaluate() also reports GCE, the example-weighted |mean prediction - observed CTR| of every id of this "
                        "column (--group_auc_key's names, e.g. _c16).  Single replica only")
    p.add_argument("--calibration_fit", type=int, default=0,
                   help="evaluate() also fits an isotonic calibration map from an equal-mass table of this many bins (2..1024) over "
                        "the evaluation's sorted scores, reduced on the GPU, and writes <model_dir>/calibration-<global_step>.json; "
                        "0: off.  Single replica only")
    p.add_argument("--calibration_apply", type=lambda s: s.lower() in ("1", "true", "yes"), default=False,
                   help="evaluate() also reports ECE_cal, MCE_cal and PCOC_cal: the figures of the probabilities mapped through the "
                        "calibration map of the current global step (needs --calibration_bins; never together with "
                        "--calibration_fit).  Single replica only")
    p.add_argument("--export_calibration", default="auto", choices=("auto", "off", "require"),
                   help="--task_type export: auto puts the calibration map of the exported global step into the bundle "
                        "(calibration.json) when there is one, off never does, require fails when there is none")
    p.add_argument("--feature_set", default="criteo", choices=["criteo", "uid_iid"],
                   help="criteo: the 39-field pipeline of fm.py (BASELINE configs); uid_iid: deepfm.py as committed "
                        "(int64 u_id / i_id hashed into 500000 / 100000 buckets, int64 label)")
    return p


def input_fn(filenames, batch_size, num_epochs=-1, need_shuffle=False, num_parallel=8, layout=None, shard=None,
             shard_tail=False, device_parse=False):
    if device_parse:                   # refused before anything is opened: see input_pipeline.check_device_parse
        from .input_pipeline import check_device_parse
        check_device_parse(layout=layout, world=1 if shard is None else shard[1])
    if layout is not None and layout.columns[0].key in ("i_id", "u_id"):     # --feature_set uid_iid (the script as committed)
        from .input_pipeline import uid_iid_input_fn
        assert shard is None or shard[1] == 1, "--feature_set uid_iid: single replica only"
        return uid_iid_input_fn(filenames, batch_size, num_epochs, need_shuffle, layout)
    from .input_pipeline import criteo_input_fn
    return criteo_input_fn(filenames, batch_size, num_epochs, need_shuffle, num_parallel, layout, shard=shard,
                           shard_tail=shard_tail, device_parse=device_parse)


def make_params(FLAGS, linear="indicator_all"):
    if getattr(FLAGS, "feature_set", "criteo") == "uid_iid":
        # deepfm/deepfm.py AS COMMITTED (:28-51): two int64 id features u_id / i_id, hashed as decimal strings
        from .feature_columns import build_model_columns
        lin, emb = build_model_columns(FLAGS.embedding_size)
    else:
        lin, emb = build_feature_columns(FLAGS.embedding_size, linear)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": FLAGS.embedding_size,
              "learning_rate": FLAGS.learning_rate, "dropout": FLAGS.dropout, "deep_layers": FLAGS.deep_layers,
              "max_batch_size": FLAGS.batch_size}
    if getattr(FLAGS, "adam_window", 0):
        params["adam_window"] = FLAGS.adam_window
    return params


def optimizer_config(FLAGS):
    """(optimizer, optimizer_hparams) of RunConfig from the --optimizer flags."""
    opt = getattr(FLAGS, "optimizer", "adam")
    if opt == "adam":
        return opt, None
    hp = {"initial_accumulator_value": FLAGS.initial_accumulator_value}
    if opt == "ftrl":
        hp.update(learning_rate_power=FLAGS.learning_rate_power, l1_regularization_strength=FLAGS.l1_regularization_strength,
                  l2_regularization_strength=FLAGS.l2_regularization_strength,
                  l2_shrinkage_regularization_strength=FLAGS.l2_shrinkage_regularization_strength)
    return opt, hp


def run_main(model_fn, FLAGS, make_params_fn):
    """The `main(_)` driver shared by the Criteo scripts (fm/fm.py:173-224, deepfm/deepfm.py:153-234, ...).
    --task_type export writes the serving bundle of the latest checkpoint (Estimator.export_savedmodel) and returns its
    directory.  The reference's deepfm.py exports after EVERY task because its `main` falls through to the export lines
    (deepfm/deepfm.py:220-234); here a model is exported only when asked."""
    optimizer, optimizer_hparams = optimizer_config(FLAGS)
    device_parse = bool(getattr(FLAGS, "device_parse", False))
    if device_parse:                   # what the device parse does not serve ends here, before anything is built or spawned
        import sys
        from .input_pipeline import check_device_parse
        module = model_fn.__module__
        if module == "__main__":
            spec = getattr(sys.modules["__main__"], "__spec__", None)
            module = spec.name if spec is not None else module
        check_device_parse(model=module)
        if getattr(FLAGS, "feature_set", "criteo") != "criteo":
            check_device_parse(layout=CriteoLayout.from_columns(make_params_fn(FLAGS)["embedding_feature_columns"]))
        if FLAGS.mirror and optimizer == "adam":
            from . import dist
            world = int(os.environ.get("WORLD_SIZE", "0") or 0) or dist.local_replica_count()
            check_device_parse(world=max(1, world))
    if optimizer != "adam" and FLAGS.mirror:
        # data-parallel training exists for the Adam step only (VariableStore.build refuses a data-parallel store)
        print("INFO:--optimizer %s: one replica in this process (data-parallel training supports --optimizer adam only)"
              % optimizer, flush=True)
        FLAGS.mirror = False
    if FLAGS.mirror:
        # MirroredStrategy() = every GPU of the host (fm/fm.py:184-186): on a multi-GPU box this process becomes the launcher
        from . import dist
        rc = dist.maybe_spawn_mirror(FLAGS, model_fn.__module__, getattr(FLAGS, "_argv", None))
        if rc is not None:
            if rc != 0:
                raise SystemExit(rc)
            return None
    files = [FLAGS.train_path + "part-r-{:0>5}".format(i) for i in range(FLAGS.train_parts)]
    train_files, eval_files = files[:-FLAGS.eval_parts], files[-FLAGS.eval_parts:]
    params = make_params_fn(FLAGS)
    config = RunConfig(save_checkpoints_steps=FLAGS.save_checkpoints_steps, keep_checkpoint_max=5,
                       log_step_count_steps=FLAGS.log_steps, adam_mode=FLAGS.adam_mode, optimizer=optimizer,
                       optimizer_hparams=optimizer_hparams, exact_auc=bool(getattr(FLAGS, "exact_auc", False)),
                       group_auc_key=getattr(FLAGS, "group_auc_key", None) or None,
                       calibration_bins=int(getattr(FLAGS, "calibration_bins", 0) or 0),
                       calibration_key=getattr(FLAGS, "calibration_key", None) or None,
                       calibration_fit=int(getattr(FLAGS, "calibration_fit", 0) or 0),
                       calibration_apply=bool(getattr(FLAGS, "calibration_apply", False)))
    est = Estimator(model_fn, FLAGS.model_dir, params, config)
    shard = None
    if FLAGS.mirror:
        from . import dist
        dp = dist.attach_if_distributed(est)
        if dp is not None:
            # MirroredStrategy (fm/fm.py:184-194): ONE batch stream, successive batches go to successive replicas -- rank r
            # trains on batches r, r+N, ... (disjoint records, same step count on every rank: csrc/tfrecord_reader.cpp)
            # and evaluates its own share of the eval stream; the metric counters are summed in Estimator.evaluate.
            shard = (dp.rank, dp.world)
    layout = CriteoLayout.from_columns(params["embedding_feature_columns"])
    if FLAGS.task_type == "train":
        tr = TrainSpec(lambda: input_fn(train_files, FLAGS.batch_size, FLAGS.num_epochs, True, FLAGS.num_parallel, layout, shard,
                                        device_parse=device_parse))
        ev = EvalSpec(lambda: input_fn(eval_files, FLAGS.batch_size, 1, False, FLAGS.num_parallel, layout, shard, True,
                                       device_parse=device_parse), steps=200)
        return train_and_evaluate(est, tr, ev)
    if FLAGS.task_type == "eval":
        return est.evaluate(lambda: input_fn(eval_files, FLAGS.batch_size, 1, False, FLAGS.num_parallel, layout, shard, True,
                                             device_parse=device_parse), steps=200)
    if FLAGS.task_type == "infer":
        out = []
        for i, p in enumerate(est.predict(lambda: input_fn(eval_files, FLAGS.batch_size, 1, False, FLAGS.num_parallel, layout,
                                                           device_parse=device_parse))):
            if est._is_chief():
                print(p)
            out.append(p)
            if i >= 9:
                break
        return out
    if FLAGS.task_type == "export":
        return est.export_savedmodel(FLAGS.export_path, table_dtype=FLAGS.export_table_dtype,
                                     calibration=getattr(FLAGS, "export_calibration", "auto"))
    raise SystemExit("unknown --task_type %r" % FLAGS.task_type)


def main(argv=None):
    FLAGS = define_flags().parse_args(argv)
    FLAGS._argv = argv
    return run_main(model_fn, FLAGS, make_params)


if __name__ == "__main__":
    main()
