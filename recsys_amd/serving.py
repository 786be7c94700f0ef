"""From a trained model to a served prediction: the export bundle and its `Predictor`.

The reference exports a SavedModel whose serving signature parses serialized `tf.train.Example`s and returns
`{"prob": ...}` (deepfm/deepfm.py:220-234); deepfm/grpc_client.py sends it 200 serialized Examples per request.  Here:

  bundle      `<export_dir_base>/<unix seconds>/` = `model.json` (settings only: the script, the columns, the layer sizes, the
              batch-norm epsilon, name / shape / dtype of every tensor) + `variables.npz` (the variables in fp32: tables,
              first-order weights, the dense arena's named tensors; no optimizer slots, no optimizer state), written under a
              temporary name and renamed when complete (`Estimator.export_savedmodel`, `--task_type export`).
              `--export_table_dtype bfloat16 | float16` (opt-in) stores the embedding tables rounded to that dtype: a
              format_version 2 bundle with a top-level "table_dtype"; bfloat16 rows are uint16 bit patterns whose tensor entry
              carries "encoding": "bfloat16".  First-order weights, din.py's bias table and the dense tensors stay fp32.  A
              float32 export is format_version 1, byte for byte what it was before the option existed.
  Predictor   loads a bundle and answers `predict_examples(list of serialized Examples)` / `predict(features)`.
              `Predictor.load(..., device_parse=True)` (opt-in; Criteo bundles on the fused path, `parse_path` == "device"):
              predict_examples ships the request's BYTES and rsx_criteo_parse_examples (csrc/parse_examples.hip) turns them
              into the ids on the device, two launches per request in one graph; the ids -- so the probabilities -- are the
              host parse's bit for bit, and whatever the device declines is parsed on the host as before.
              path == "fused":  fm.py / deepfm.py bundles inside the kernel's envelope -- the variables live on the device once
                                and a batch is ONE launch of rsx_predict_fm_tower (csrc/predict.hip), captured per request size
                                into a HIP graph over static input buffers.
                                dcn.py bundles loaded with `Predictor.load(..., one_launch=True)` inside rsx_predict_dcn's
                                envelope (csrc/predict_dcn.hip) -- the same buffers, graphs and chunking, ONE launch of that
                                kernel per batch.  Opt-in: it agrees with the Estimator to 2e-5, not bit for bit.
                                A 16-bit bundle's table goes to the device as stored (R x 16 x 2 bytes) and the kernel widens
                                a row as it loads it: bit-identical to an fp32 bundle holding the rounded values.
              path == "layers": dcn.py (the default) / xdeepfm.py / din.py bundles, and fm / deepfm / dcn shapes outside the
                                envelope -- the script's Estimator rebuilt from the manifest (model_dir=None) with the
                                bundle's variables, answering through Estimator._infer_step (the TRAIN kernels' inference
                                form), bit-identical to the Estimator the bundle came from.  A 16-bit bundle's tables are
                                widened to fp32 on the host first: it answers like an fp32 bundle holding the rounded values,
                                and saves no device memory here.
  calibration a bundle may carry one more file, `calibration.json`: the isotonic map (metrics.IsotonicMap: fp32 knots as bit
              patterns) fitted by `evaluate()` with RunConfig.calibration_fit at the exported global_step
              (`export_savedmodel(..., calibration="auto" | "off" | "require")`, `--export_calibration`).  The manifest and
              format_version do not change and read_bundle reads only its two files: old readers and old bundles are untouched.
              `Predictor.load(..., calibrated=None)` applies the map iff the bundle carries one (False: raw; True: it must):
              `predict` / `predict_examples` then return the mapped probabilities on every path -- one more launch of
              rsx_calibrate_apply (csrc/calibration_map.hip) behind the predict launch, inside the request size's graph on the
              fused and device-parse paths, an eager launch into a buffer of the Predictor's own on the layers path.
              `Predictor.calibrate(prob)` maps any array.  Out of scope: the din.py request kinds (`rank_candidates`,
              `recommend*`, `evaluate_*`) select on and return RAW scores -- the map is monotone, so the order stands, and the
              caller may pass the returned prob through `Predictor.calibrate`.
"""
import ctypes as C
import importlib
import json
import os
import re
import shutil
import time

import numpy as np

from . import _lib
from .feature_columns import Column, CriteoLayout
from .layers import BN_EPS
# what din.py bundles answer beside `predict` lives in serving_din.py; its names stay reachable as serving.X
from .serving_din import (  # noqa: F401
    EXCL_MAX, NBR_MAX, RANK_MAX_T, RANK_MISSING, RANK_PAD, RETRIEVED_MISSING, RETRIEVED_PAD, RULES_MAX_M, TOPK_MAX_K, DinRanking,
    _exclusion_ids, _list_place, _one_user, _target_positions, candidate_capacity, catalogue_first_positions, category_bitmap,
    check_catalogue, check_category_list, check_held_out, check_ks, check_max_per_category, check_n_neighbours, check_neighbours,
    check_rank_request, check_top_k, expand_rank_request, item_neighbours_host, narrow_neighbours_host, ranking_metrics,
    recommend_host, recommend_two_stage_host, retrieve_candidates_host, rows_dot_host, target_ranks_host, topk_rows_host,
    two_stage_metrics, two_stage_ranks_host, unit_rows_host)
# ... and what uid_iid deepfm.py bundles answer beside it in serving_pairs.py
from .serving_pairs import (  # noqa: F401
    PairRanking, check_item_catalogue, check_pair_exclude, check_pair_request, exclusion_positions, expand_pair_request,
    hash_pair_ids, pair_slots, recommend_items_host)

FORMAT_VERSION = 1                    # float32 tables; 16-bit tables (`table_dtype`, `encoding`) make a bundle version 2
FORMAT_VERSION_16BIT = 2
TABLE_DTYPES = ("float32", "bfloat16", "float16")
SCRIPTS = ("fm", "deepfm", "xdeepfm", "dcn", "din")
MANIFEST, VARIABLES = "model.json", "variables.npz"
CALIBRATION = "calibration.json"      # optional: the isotonic map of the exported global_step (metrics.IsotonicMap.to_json)
CALIBRATION_MODES = ("auto", "off", "require")
# model_fn parameters that shape the network (what a Predictor needs to rebuild it without the training flags)
_NETWORK_PARAMS = ("embedding_size", "deep_layers", "cross_layers", "cin_bf16", "cin_split", "hist_len", "n_item", "n_cate",
                   "tower", "force_generic")
SIGNATURE = {"serving_default": {"inputs": "examples", "outputs": ["prob"]}}


# ---- 16-bit embedding rows: plain numpy, no device ---------------------------------------------------------------------------
def is_embedding_rows(name, shape, embedding_size):
    """An embedding-row tensor: `emb.<arena>.tables` / `emb.<arena>.table` whose last dimension is the model's embedding_size
    (not the first-order vector `w1`, not din.py's 4-wide bias table, no dense tensor)."""
    return (name.startswith("emb.") and name.rsplit(".", 1)[-1] in ("tables", "table") and len(shape) >= 1
            and int(shape[-1]) == int(embedding_size))


def quantize_rows(a, dtype, name="tensor"):
    """fp32 array -> its stored form in `dtype`, rounded to nearest even: "float32" the array itself, "float16" a numpy
    float16 array, "bfloat16" the bit patterns as uint16 (numpy has no bfloat16).  Refuses (RsxError naming `name`) a value
    that is not finite and a finite one that rounds to infinity (float16 beyond 65504, bfloat16 just below the fp32 maximum)."""
    if dtype not in TABLE_DTYPES:
        raise _lib.RsxError("table dtype %r is none of %s" % (dtype, ", ".join(TABLE_DTYPES)))
    a = np.ascontiguousarray(a, np.float32)
    if dtype == "float32":
        return a
    if not np.isfinite(a).all():
        raise _lib.RsxError("tensor %r holds values that are not finite: it cannot be stored as %s" % (name, dtype))
    if dtype == "float16":
        with np.errstate(over="ignore"):
            out = a.astype(np.float16)
        over = ~np.isfinite(out)
    else:
        u = a.view(np.uint32)
        out = ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
        over = (out & np.uint16(0x7fff)) == np.uint16(0x7f80)
    if over.any():
        raise _lib.RsxError("tensor %r holds finite values (largest magnitude %g) that round to infinity in %s"
                            % (name, float(np.abs(a).max()), dtype))
    return out


def dequantize_rows(a, encoding=None):
    """The stored form back to fp32, exactly: encoding "bfloat16" takes uint16 bit patterns, otherwise the array's own dtype
    (float16 or float32) says what it is."""
    a = np.asarray(a)
    if encoding == "bfloat16":
        if a.dtype != np.uint16:
            raise _lib.RsxError("bfloat16 rows are stored as uint16 bit patterns, not %s" % a.dtype)
        return (a.astype(np.uint32) << np.uint32(16)).view(np.float32)
    if encoding not in (None, "float16", "float32") or a.dtype not in (np.float16, np.float32):
        raise _lib.RsxError("cannot widen rows of dtype %s with encoding %r" % (a.dtype, encoding))
    return a.astype(np.float32)


def quantize_tensors(tensors, embedding_size, table_dtype):
    """{name: fp32 array} -> the same with every embedding-row tensor in its stored 16-bit form (the rest untouched)."""
    return {k: quantize_rows(v, table_dtype, k) if is_embedding_rows(k, v.shape, embedding_size) else v
            for k, v in tensors.items()}


def widen_tensors(manifest, arrays):
    """A bundle's arrays as read -> every tensor fp32 (what the layers path loads); a version 1 bundle's arrays unchanged."""
    enc = {t["name"]: t.get("encoding") for t in manifest["tensors"]}
    return {k: v if v.dtype == np.float32 else dequantize_rows(v, enc.get(k)) for k, v in arrays.items()}


# ---- manifest ------------------------------------------------------------------------------------------------------------
def _column_json(c):
    return {"name": c.name, "key": c.key, "kind": c.kind, "rows": int(c.rows), "dimension": int(c.dimension),
            "boundaries": None if c.boundaries is None else [float(x) for x in c.boundaries], "log_shift": float(c.log_shift)}


def _column_from_json(d):
    return Column(d["name"], d["key"], d["kind"], int(d["rows"]), int(d["dimension"]), d["boundaries"], float(d["log_shift"]))


def linear_mode(linear_columns):
    """build_feature_columns' `linear` argument that yields these linear columns ('custom' for hand-made ones)."""
    kinds = {c.kind for c in linear_columns}
    if kinds <= {"bucketized_indicator", "hash_indicator"}:
        return "indicator_all"
    if kinds == {"numeric", "hash_indicator"}:
        return "numeric+indicator"
    if kinds == {"numeric"}:
        return "numeric"
    return "custom"


def _check_export(script, table_dtype, module=None):
    """What an export refuses about its table dtype and its script (`module`: the model_fn's module the script name came from)."""
    if table_dtype not in TABLE_DTYPES:
        raise _lib.RsxError("export: table dtype %r is none of %s" % (table_dtype, ", ".join(TABLE_DTYPES)))
    if script not in SCRIPTS:
        if module is not None:
            raise _lib.RsxError("export: model_fn of module %r is none of the scripts %s" % (module, ", ".join(SCRIPTS)))
        raise _lib.RsxError("export: unknown script %r (known: %s)" % (script, ", ".join(SCRIPTS)))


def make_manifest(script, params, global_step, tensors, table_dtype="float32"):
    """The settings of one exported model.  tensors: {name: numpy array} as stored -- only names, shapes and dtypes go in
    here.  A 16-bit table_dtype makes a format_version 2 manifest (see the module docstring); "float32" adds no key."""
    _check_export(script, table_dtype)
    emb = params.get("embedding_feature_columns")
    lin = params.get("linear_feature_columns") or []
    if script == "din":
        feature_set = "din"
    else:
        if emb is None:
            raise _lib.RsxError("export: the params of %s.py hold no embedding_feature_columns" % script)
        feature_set = "uid_iid" if {c.key for c in emb} <= {"u_id", "i_id"} else "criteo"
    m = {"format_version": FORMAT_VERSION, "script": script, "global_step": int(global_step), "feature_set": feature_set,
         "linear_mode": linear_mode(lin) if script != "din" else None, "batch_norm_epsilon": BN_EPS,
         "params": {k: params[k] for k in _NETWORK_PARAMS if k in params},
         "embedding_columns": [_column_json(c) for c in (emb or [])],
         "linear_columns": [_column_json(c) for c in lin],
         "signature": SIGNATURE,
         "tensors": [{"name": k, "shape": [int(d) for d in v.shape], "dtype": str(v.dtype)} for k, v in tensors.items()]}
    if table_dtype != "float32":
        m["format_version"], m["table_dtype"] = FORMAT_VERSION_16BIT, table_dtype
        if table_dtype == "bfloat16":
            for t in m["tensors"]:
                if is_embedding_rows(t["name"], t["shape"], params["embedding_size"]):
                    t["encoding"] = "bfloat16"
    return m


def layout_from_manifest(manifest):
    """The CriteoLayout (slot order, row offsets, host transform) of a bundle's embedding columns."""
    return CriteoLayout.from_columns([_column_from_json(d) for d in manifest["embedding_columns"]])


def params_from_manifest(manifest, max_batch_size):
    """model_fn params that rebuild the bundle's network for inference."""
    p = dict(manifest["params"])
    p.update(learning_rate=0.0, dropout=0.0, max_batch_size=int(max_batch_size))
    if manifest["script"] != "din":
        p["embedding_feature_columns"] = [_column_from_json(d) for d in manifest["embedding_columns"]]
        p["linear_feature_columns"] = [_column_from_json(d) for d in manifest["linear_columns"]]
    return p


# ---- bundle writer / reader ----------------------------------------------------------------------------------------------
def write_bundle(export_dir_base, manifest, tensors, extra_files=None):
    """-> `<export_dir_base>/<unix seconds>`, holding model.json and variables.npz.  The bundle is assembled in a temporary
    directory of the same parent and renamed when complete: a reader never sees half a bundle.  (A second export within the
    same second takes the next free second, as tf.estimator's export does.)
    extra_files: {file name: text} written beside the two (calibration.json); the manifest does not list them."""
    for name in (extra_files or {}):
        if name in (MANIFEST, VARIABLES) or os.path.basename(name) != name or not name:
            raise _lib.RsxError("export: %r is no name for an extra bundle file" % name)
    base = os.path.abspath(export_dir_base)
    os.makedirs(base, exist_ok=True)
    for k, v in tensors.items():
        if not isinstance(v, np.ndarray) or v.dtype.hasobject:
            raise _lib.RsxError("export: tensor %r is not a plain numpy array" % k)
    tmp = os.path.join(base, "temp-%d-%d" % (os.getpid(), time.monotonic_ns()))
    os.makedirs(tmp)
    try:
        with open(os.path.join(tmp, VARIABLES), "wb") as f:
            np.savez(f, **tensors)
        with open(os.path.join(tmp, MANIFEST), "w") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)
            f.write("\n")
        for name, text in (extra_files or {}).items():
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        ts = int(time.time())
        while True:
            final = os.path.join(base, "%d" % ts)
            try:
                os.rename(tmp, final)          # (fails when `final` exists and is not empty)
                return final
            except OSError:
                if not os.path.exists(final):
                    raise
                ts += 1
    finally:
        if os.path.isdir(tmp):
            shutil.rmtree(tmp, ignore_errors=True)


def latest_bundle(path):
    """`path` itself when it is a bundle, else its newest `<unix seconds>` child that is one."""
    if os.path.isfile(os.path.join(path, MANIFEST)):
        return path
    best = None
    if os.path.isdir(path):
        for name in os.listdir(path):
            if re.fullmatch(r"\d+", name) and os.path.isfile(os.path.join(path, name, MANIFEST)):
                if best is None or int(name) > int(best):
                    best = name
    if best is None:
        raise _lib.RsxError("no exported model under %r (run the script with --task_type export)" % path)
    return os.path.join(path, best)


def read_bundle(bundle_dir):
    """-> (manifest, {name: numpy array as stored}).  Refuses (RsxError naming the cause): an unknown format_version, a tensor
    the manifest lists and the archive lacks or the reverse, a shape or dtype that disagrees with the manifest; a version 2
    manifest whose table_dtype is no 16-bit dtype, a uint16 tensor without an encoding, an encoding on a tensor that is no
    embedding-row tensor, an embedding-row tensor stored in another dtype than table_dtype, and a version 1 manifest that
    carries `table_dtype` or an `encoding`."""
    mp = os.path.join(bundle_dir, MANIFEST)
    try:
        with open(mp) as f:
            manifest = json.load(f)
    except (OSError, ValueError) as e:
        raise _lib.RsxError("bundle %r: cannot read %s (%s)" % (bundle_dir, MANIFEST, e)) from e
    ver = manifest.get("format_version") if isinstance(manifest, dict) else None
    if ver not in (FORMAT_VERSION, FORMAT_VERSION_16BIT) or isinstance(ver, bool):
        raise _lib.RsxError("bundle %r: format_version %r is not supported (this reader knows %d and %d)"
                            % (bundle_dir, ver, FORMAT_VERSION, FORMAT_VERSION_16BIT))
    table_dtype = manifest.get("table_dtype")
    if ver == FORMAT_VERSION_16BIT and table_dtype not in TABLE_DTYPES[1:]:
        raise _lib.RsxError("bundle %r: a format_version %d manifest needs a table_dtype of %s, not %r"
                            % (bundle_dir, ver, " or ".join(TABLE_DTYPES[1:]), table_dtype))
    if ver == FORMAT_VERSION and "table_dtype" in manifest:
        raise _lib.RsxError("bundle %r: a format_version %d manifest cannot carry table_dtype (%r)" % (bundle_dir, ver, table_dtype))
    if manifest.get("script") not in SCRIPTS:
        raise _lib.RsxError("bundle %r: unknown script %r" % (bundle_dir, manifest.get("script")))
    try:
        with np.load(os.path.join(bundle_dir, VARIABLES), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
    except (OSError, ValueError) as e:
        raise _lib.RsxError("bundle %r: cannot read %s (%s)" % (bundle_dir, VARIABLES, e)) from e
    listed = {t["name"]: t for t in manifest["tensors"]}
    missing = sorted(set(listed) - set(arrays))
    if missing:
        raise _lib.RsxError("bundle %r: %s lacks the tensors %s listed in %s" % (bundle_dir, VARIABLES, missing, MANIFEST))
    extra = sorted(set(arrays) - set(listed))
    if extra:
        raise _lib.RsxError("bundle %r: %s holds the tensors %s that %s does not list" % (bundle_dir, VARIABLES, extra, MANIFEST))
    for k, t in listed.items():
        if list(arrays[k].shape) != list(t["shape"]):
            raise _lib.RsxError("bundle %r: tensor %r has shape %s, %s says %s"
                                % (bundle_dir, k, list(arrays[k].shape), MANIFEST, list(t["shape"])))
        if str(arrays[k].dtype) != t["dtype"]:
            raise _lib.RsxError("bundle %r: tensor %r has dtype %s, %s says %s" % (bundle_dir, k, arrays[k].dtype, MANIFEST, t["dtype"]))
    D = (manifest.get("params") or {}).get("embedding_size")
    stored = {"bfloat16": ("uint16", "bfloat16"), "float16": ("float16", None)}.get(table_dtype)      # (dtype, encoding)
    for k, t in listed.items():
        enc = t.get("encoding")
        rows = D is not None and is_embedding_rows(k, t["shape"], D)
        if "encoding" in t and ver == FORMAT_VERSION:
            raise _lib.RsxError("bundle %r: tensor %r carries an encoding (%r) in a format_version %d manifest" % (bundle_dir, k, enc, ver))
        if "encoding" in t and not rows:
            raise _lib.RsxError("bundle %r: tensor %r carries an encoding (%r) but is no embedding-row tensor" % (bundle_dir, k, enc))
        if t["dtype"] == "uint16" and enc is None:
            raise _lib.RsxError("bundle %r: tensor %r is uint16 without an encoding" % (bundle_dir, k))
        if rows and stored is not None and (t["dtype"], enc) != stored:
            raise _lib.RsxError("bundle %r: embedding-row tensor %r is stored as %s (encoding %r), the bundle's table_dtype is %s"
                                % (bundle_dir, k, t["dtype"], enc, table_dtype))
    return manifest, arrays


# ---- Estimator side --------------------------------------------------------------------------------------------------------
_TABLE_ATTRS = ("tables", "w1", "table")      # what an EmbeddingArena / SparseTable holds besides optimizer slots


def _store_tensors(store):
    """(bundle name, tensor) of every variable of a built VariableStore: `emb.<arena>.<tables|w1|table>`, then
    `dense.<variable>`."""
    for name, a in store.embeddings.items():
        for attr in _TABLE_ATTRS:
            t = getattr(a, attr, None)
            if t is not None:
                yield "emb.%s.%s" % (name, attr), t
    for k, p in store.dense.params.items():
        yield "dense." + k, p


def store_variables(store):
    """{name: fp32 numpy array} of a built VariableStore."""
    return {k: t.detach().float().cpu().contiguous().numpy().copy() for k, t in _store_tensors(store)}


def load_store_variables(store, arrays):
    """The reverse: a bundle's tensors into a built VariableStore of the same model."""
    import torch
    want = set(store_variables_names(store))
    if want != set(arrays):
        raise _lib.RsxError("bundle and model disagree on the variables: only in the bundle %s, only in the model %s"
                            % (sorted(set(arrays) - want), sorted(want - set(arrays))))
    with torch.no_grad():
        for k, t in _store_tensors(store):
            if tuple(arrays[k].shape) != tuple(t.shape):
                raise _lib.RsxError("bundle tensor %s has shape %s, the model's is %s" % (k, tuple(arrays[k].shape), tuple(t.shape)))
            t.copy_(torch.from_numpy(arrays[k]))


def store_variables_names(store):
    return [k for k, _ in _store_tensors(store)]


def export_estimator(est, export_dir_base, table_dtype="float32", calibration="auto"):
    """Estimator.export_savedmodel's body: the latest checkpoint of est.model_dir as a bundle -> its directory.  table_dtype
    "bfloat16" / "float16": every embedding-row tensor is rounded to it (`quantize_rows`) and stored in it.
    calibration: "auto" adds calibration.json when est has a map of the exported global_step (last_calibration_map, else
    <model_dir>/calibration-<step>.json), "off" never, "require" raises when there is none; a map of another step is never taken."""
    from . import checkpoint
    script = est.model_fn.__module__.rsplit(".", 1)[-1]
    _check_export(script, table_dtype, module=est.model_fn.__module__)
    if calibration not in CALIBRATION_MODES:
        raise _lib.RsxError("export: calibration %r is none of %s" % (calibration, ", ".join(CALIBRATION_MODES)))
    # With a model_dir the bundle is its latest checkpoint (restored now unless this Estimator already runs from it); an
    # Estimator without one (model_dir=None: tests, notebooks) exports the variables it holds.
    if est.model_dir:
        if checkpoint.latest(est.model_dir) is None:
            raise _lib.RsxError("export: no checkpoint in model_dir %r -- train first (--task_type train), then export"
                                % est.model_dir)
    elif not est.store.built:
        raise _lib.RsxError("export: this Estimator has neither a model_dir nor variables -- nothing to export")
    if not est.store.built:
        _build_store(est, script)
    est._maybe_restore()
    est._check_consistent("export_savedmodel")
    out = None
    if est._is_chief():                   # replicas are bit-identical: the chief writes (the rule of _save_checkpoint)
        tensors = store_variables(est.store)
        if table_dtype != "float32":
            tensors = quantize_tensors(tensors, est.params["embedding_size"], table_dtype)
        extra = None
        if calibration != "off":
            cmap = est.calibration_map_for_step(est.global_step)
            if cmap is None and calibration == "require":
                raise _lib.RsxError("export: calibration=\"require\" and there is no calibration map for global step %d (neither "
                                    "last_calibration_map nor %s)"
                                    % (est.global_step, est._calibration_path(est.global_step) or "a model_dir"))
            if cmap is not None:
                extra = {CALIBRATION: json.dumps(cmap.to_json()) + "\n"}
        out = write_bundle(export_dir_base, make_manifest(script, est.params, est.global_step, tensors, table_dtype), tensors,
                           extra)
        print("INFO:Model exported.", flush=True)
    if est.store.dp is not None:
        est.store.dp.barrier()
    return out


def _dummy_features(script, params, layout=None):
    """One all-zero request row: what the first model_fn call needs to create the variables."""
    if script == "din":
        P = int(params.get("hist_len", 100))
        z1, zP = np.zeros(1, np.int32), np.zeros((1, P), np.int32)
        return {"i_id": z1, "i_cate": z1.copy(), "u_iid_seq": zP, "u_icat_seq": zP.copy()}
    f = {"ids": np.zeros((1, layout.F), np.int32)}
    if script == "xdeepfm":
        f["cont_log"] = np.zeros((1, 13), np.float32)
    return f


def _build_store(est, script):
    """Creates the Estimator's variables (the first model_fn call does) without a batch of data."""
    import torch
    from .estimator import ModeKeys
    layout = None if script == "din" else CriteoLayout.from_columns(est.params["embedding_feature_columns"])
    with torch.no_grad():
        est._call_model_fn(est._to_device(_dummy_features(script, est.params, layout)), None, ModeKeys.PREDICT)


# ---- Predictor ---------------------------------------------------------------------------------------------------------------
class Predictor(DinRanking, PairRanking):
    """An exported model ready to answer requests.  See the module docstring for the two paths.  `table_dtype` is the
    bundle's ("float32" for a version 1 bundle): on the fused path the device holds the table in that dtype; on the layers
    path a 16-bit table is widened to fp32 on the host (the rounded values, no memory saved, `rank_candidates` unchanged).
    What din.py bundles answer beside `predict` is inherited from `DinRanking` (serving_din.py; its docstring has those requests),
    what uid_iid deepfm.py bundles answer -- `rank_items`, `set_item_catalogue`, `recommend_items` -- from `PairRanking`
    (serving_pairs.py)."""

    MAX_GRAPHS = 32            # request sizes that get a captured graph at most (Estimator.MAX_INFER_GRAPHS' twin)

    def __init__(self):
        raise TypeError("use Predictor.load(export_dir)")

    @classmethod
    def load(cls, export_dir, device="cuda", max_batch_size=4096, use_hip_graph=True, max_candidates=None, one_launch=False,
             device_parse=False, parse_row_bytes=2048, calibrated=None):
        """export_dir: a bundle, or the --export_path that holds bundles (the newest is taken).  max_candidates (din.py bundles;
        default max_batch_size): the candidates per user one `rank_candidates` launch takes, longer requests are cut along C.
        one_launch (dcn.py bundles; the other scripts ignore it): answer through rsx_predict_dcn, path == "fused", instead of
        the rebuilt Estimator.  Off by default: the one-launch forward sums in another order than the Estimator's kernels, so
        it agrees with them to 2e-5, not bit for bit.
        device_parse (Criteo bundles on the fused path; everything else ignores it, `parse_path` says which): predict_examples
        ships the request's bytes and a launch of rsx_criteo_parse_examples (csrc/parse_examples.hip) writes the ids in front of
        the predict launch, both in the graph of the request size.  The ids are the host parser's bit for bit; a chunk with an
        example the device declines (malformed, a missing numeric, a record above 8 KB) or with more bytes than the staging
        buffer holds is parsed on the host exactly as without the flag.  Off by default.
        parse_row_bytes: the staging buffers (one pinned, one on the device) hold max_batch_size * parse_row_bytes request
        bytes; a Criteo request row is about 0.9 KB (39 entries, 8-byte categorical values), 2048 leaves room for two.
        calibrated: None applies the bundle's calibration.json iff it carries one, False serves raw probabilities, True raises
        when there is none.  A map whose global_step or script disagrees with the manifest is refused (whatever `calibrated`
        says).  `calibration` holds the metrics.IsotonicMap or None, `calibrated` says whether predict / predict_examples map."""
        import torch
        self = object.__new__(cls)
        self.bundle_dir = latest_bundle(export_dir)
        self.manifest, arrays = read_bundle(self.bundle_dir)
        m = self.manifest
        self.script, self.global_step = m["script"], int(m["global_step"])
        self.calibration = self._read_calibration()
        if calibrated and self.calibration is None:
            raise _lib.RsxError("Predictor: calibrated=True and bundle %r carries no %s" % (self.bundle_dir, CALIBRATION))
        self.calibrated = self.calibration is not None and (calibrated is None or bool(calibrated))
        self._cal = self._cal_buf = None    # metrics.Calibrator; the layers path's output buffer
        self.table_dtype = m.get("table_dtype", "float32")
        self.signature = SIGNATURE
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.RsxError("Predictor: device %r -- there is no CPU path (the forward is HIP kernels)" % device)
        self.max_batch_size = int(max_batch_size)
        if self.max_batch_size < 1:
            raise _lib.RsxError("Predictor: max_batch_size must be at least 1")
        self.use_hip_graph = bool(use_hip_graph)
        self.layout = None if self.script == "din" else layout_from_manifest(m)
        self._graphs, self._n_graphs = {}, 0
        self._est = None
        self.one_launch = bool(one_launch)
        if self.script in ("fm", "deepfm") and self._fused_setup(arrays):
            self.path = "fused"
        elif self.script == "dcn" and self.one_launch and self._fused_dcn_setup(arrays):
            self.path = "fused"
        else:
            self.path = "layers"
            self._layers_setup(arrays)
        if self.calibration is not None:
            from .metrics import Calibrator
            self._cal = Calibrator(self.device, self.calibration)
            if self.calibrated and self.path == "layers":
                self._cal_buf = torch.empty(self.max_batch_size, dtype=torch.float32, device=self.device)
        self.max_candidates = self.max_batch_size if max_candidates is None else int(max_candidates)
        if self.max_candidates < 1:
            raise _lib.RsxError("Predictor: max_candidates must be at least 1")
        self.parse_path, self._dp = "host", None
        if device_parse:
            self._device_parse_setup(int(parse_row_bytes))
        self.rank_path = None
        self.topk_path = None               # where the latest `rank_candidates(top_k=k)` selected (before any: a small k)
        self._rank = None
        self.catalogue_size = None          # N of the latest `set_catalogue` (din.py bundles)
        self.recommend_path = None          # where the latest `recommend` selected
        self.rules_on_device = True         # False: a `recommend` / `recommend_two_stage` with a category rule takes the host path
        self.evaluate_recommend_path = None # where the latest `evaluate_recommend` ranked
        self._cat = None
        self._nbr = None                    # `build_neighbours`' table (din.py bundles)
        self.neighbours_path = None         # where the latest `build_neighbours` built it
        self.two_stage_path = None          # where the latest `recommend_two_stage` ran
        self.evaluate_two_stage_path = None # where the latest `evaluate_two_stage` ranked
        self._pair = None                   # PairRanking's model and buffers: made by the first ranking request
        self._item_cat = None               # `set_item_catalogue`'s ids (uid_iid deepfm.py bundles)
        self.item_catalogue_size = None
        self.pair_topk_path = None          # where the latest `rank_items(top_k=k)` selected
        self.recommend_items_path = None    # where the latest `recommend_items` selected
        if self.script == "din":
            self.rank_path = "fused" if self._rank_supported() else "layers"
            self.topk_path = "device" if self.rank_path == "fused" else "host"
        return self

    def _read_calibration(self):
        """The bundle's calibration.json as a metrics.IsotonicMap, None when the bundle has none."""
        from .metrics import IsotonicMap
        path = os.path.join(self.bundle_dir, CALIBRATION)
        if not os.path.isfile(path):
            return None
        try:
            cmap = IsotonicMap.load(path)
        except (OSError, ValueError) as e:
            raise _lib.RsxError("bundle %r: cannot read %s (%s)" % (self.bundle_dir, CALIBRATION, e)) from e
        if cmap.global_step != self.global_step or cmap.script != self.script:
            raise _lib.RsxError("bundle %r: %s belongs to %s.py at global step %d, the model is %s.py at global step %d"
                                % (self.bundle_dir, CALIBRATION, cmap.script, cmap.global_step, self.script, self.global_step))
        return cmap

    def calibrate(self, prob):
        """The bundle's map applied to any array of probabilities (numpy -> numpy, device tensor -> device tensor); what the
        din.py request kinds, which return raw scores, leave to the caller."""
        if self._cal is None:
            raise _lib.RsxError("Predictor: bundle %r carries no %s" % (self.bundle_dir, CALIBRATION))
        return self._cal.apply(prob)

    # -- the one-launch path ----------------------------------------------------------------------------------------------
    def _fused_variables(self, arrays, need):
        """The variables of a one-launch model on the device, once: the tables and every dense tensor of `need` in ONE flat
        buffer (16-byte aligned parts), the row offsets, and the request buffers -> the dense tensors' address by name.
        The table goes up in its stored form: fp32, float16, or bfloat16 bit patterns (the model struct's table_dtype)."""
        import torch
        if set(need) != set(arrays):
            raise _lib.RsxError("bundle %r: a %s bundle holds the tensors %s, not %s"
                                % (self.bundle_dir, self.script, sorted(need), sorted(arrays)))
        dev, lay = self.device, self.layout
        tables = arrays["emb.input_layer.tables"]
        self._tables = torch.from_numpy(tables.view(np.int16) if tables.dtype == np.uint16 else tables).to(dev)
        dense = [k for k in need if k.startswith("dense.")]
        offs, n = {}, 0
        for k in dense:
            offs[k] = n
            n = (n + arrays[k].size + 3) & ~3
        flat = np.zeros(n, np.float32)
        for k in dense:
            flat[offs[k]:offs[k] + arrays[k].size] = arrays[k].reshape(-1)
        self._dense = torch.from_numpy(flat).to(dev)
        self._row_off = torch.from_numpy(lay.row_off[:-1].astype(np.int32)).to(dev)
        # request buffers: ids and prob of one chunk (the static inputs / outputs of the captured graphs are slices of them)
        self._ids = torch.zeros(self.max_batch_size, lay.F, dtype=torch.int32, device=dev)
        self._prob = torch.zeros(self.max_batch_size, dtype=torch.float32, device=dev)
        return lambda k: self._dense.data_ptr() + 4 * offs[k]

    def _tower_widths(self):
        """The manifest's `deep_layers` (fm.py: no tower) -> (widths, their array for the C ABI; None when the model structs
        cannot hold them)."""
        deep = "" if self.script == "fm" else str(self.manifest["params"].get("deep_layers", ""))
        widths = [int(w) for w in deep.split(",") if w]
        fits = len(widths) <= _lib.PREDICT_MAX_LAYERS
        return widths, (C.c_int32 * _lib.PREDICT_MAX_LAYERS)(*widths) if fits else None

    @staticmethod
    def _tower_need(widths):
        return ["dense.dnn.%s%d" % (v, l) for l in range(len(widths)) for v in ("W", "b", "gamma", "beta")]

    def _fill_tower(self, pm, ptr, widths, D):
        """What rsx_predict_model and rsx_predict_dcn_model spell alike: the table, the tower's layers, the sizes."""
        pm.tables, pm.row_off = self._tables.data_ptr(), self._row_off.data_ptr()
        for l in range(len(widths)):
            pm.W[l], pm.b[l] = ptr("dense.dnn.W%d" % l), ptr("dense.dnn.b%d" % l)
            pm.gamma[l], pm.beta[l] = ptr("dense.dnn.gamma%d" % l), ptr("dense.dnn.beta%d" % l)
            pm.widths[l] = widths[l]
        pm.wo, pm.bo = ptr("dense.out.W"), ptr("dense.out.b")
        pm.bn_eps = float(self.manifest["batch_norm_epsilon"])
        pm.F, pm.D, pm.L = self.layout.F, D, len(widths)
        pm.table_dtype = _lib.TABLE_DTYPES[self.table_dtype]

    def _fused_setup(self, arrays):
        import torch
        m, lay = self.manifest, self.layout
        D = int(m["params"]["embedding_size"])
        widths, wa = self._tower_widths()
        if wa is None or not _lib.lib().rsx_predict_fm_tower_supported(self.max_batch_size, lay.F, D, len(widths), wa):
            return False
        need = ["emb.input_layer.tables", "emb.input_layer.w1", "dense.b1", "dense.out.W", "dense.out.b"] + self._tower_need(widths)
        if widths:
            need += ["dense.dnn.Wout", "dense.dnn.bout"]
        ptr = self._fused_variables(arrays, need)
        self._w1 = torch.from_numpy(arrays["emb.input_layer.w1"]).to(self.device)      # the first-order vector
        lin_keys = {c["key"] for c in m["linear_columns"] if c["kind"].endswith("indicator")}
        pm = _lib.PredictModel()
        self._fill_tower(pm, ptr, widths, D)
        pm.w1, pm.c0 = self._w1.data_ptr(), ptr("dense.b1")
        if widths:
            pm.wd, pm.bd = ptr("dense.dnn.Wout"), ptr("dense.dnn.bout")
        pm.w1_field_mask = lay.field_mask(lin_keys)
        self._model, self._kernel = pm, "rsx_predict_fm_tower"
        return True

    def _fused_dcn_setup(self, arrays):
        """dcn.py with one_launch=True: tables + ONE flat buffer of the dense tensors, no Estimator; False outside
        rsx_predict_dcn's envelope."""
        m, lay = self.manifest, self.layout
        widths, wa = self._tower_widths()
        Lc = int(m["params"].get("cross_layers", 0))
        D = int(m["params"]["embedding_size"])
        if wa is None or not _lib.lib().rsx_predict_dcn_supported(self.max_batch_size, lay.F, D, len(widths), wa, Lc):
            return False
        need = ["emb.input_layer.tables", "dense.cross.W", "dense.cross.b", "dense.out.W", "dense.out.b"] + self._tower_need(widths)
        ptr = self._fused_variables(arrays, need)
        pm = _lib.PredictDcnModel()
        self._fill_tower(pm, ptr, widths, D)
        pm.cross_W, pm.cross_b, pm.Lc = ptr("dense.cross.W"), ptr("dense.cross.b"), Lc
        self._model, self._kernel = pm, "rsx_predict_dcn"
        return True

    def _launch(self, n):
        import torch
        fn = getattr(_lib.lib(), self._kernel)          # rsx_predict_fm_tower / rsx_predict_dcn: the same call shape
        _lib.check(fn(C.byref(self._model), self._ids.data_ptr(), self._prob.data_ptr(), int(n),
                      torch.cuda.current_stream().cuda_stream), self._kernel)
        if self.calibrated:               # behind the predict launch, in place in the Predictor's own buffer (and in its graph)
            self._cal.apply(self._prob[:n], out=self._prob[:n])

    def _run(self, key, launch):
        """`launch()` eagerly, or as the captured graph of `key`: warm-up on the first request, capture on the second."""
        import torch
        g = self._graphs.get(key) if self.use_hip_graph else None
        if g is None and self.use_hip_graph and self._n_graphs < self.MAX_GRAPHS:
            g = self._graphs[key] = {"warm": 0}
            self._n_graphs += 1
        if g is None:                       # graphs off, or a serving loop with ever-new request sizes: eager
            launch()
        elif "graph" in g:
            g["graph"].replay()
        elif g["warm"] < 1:                 # first request of this size: eager
            g["warm"] += 1
            launch()
        else:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with _lib.capture_gc_guard(), torch.cuda.graph(graph):
                launch()
            g["graph"] = graph
            graph.replay()                  # capture executes nothing

    def _drop_graphs(self, *kinds):
        """Forgets the captured graphs of these key kinds (their static buffers are about to be replaced)."""
        for k in [k for k in self._graphs if isinstance(k, tuple) and k[0] in kinds]:
            del self._graphs[k]
            self._n_graphs -= 1

    def _fused_chunk(self, ids):
        """ids: int32 [n, F] (host or device), n <= max_batch_size -> prob [n] (a view of the Predictor's output buffer,
        valid until the next call)."""
        n = int(ids.shape[0])
        self._ids[:n].copy_(ids, non_blocking=True)
        self._run(n, lambda: self._launch(n))
        return self._prob[:n]

    # -- the device parse (device_parse=True) --------------------------------------------------------------------------------
    def _device_parse_setup(self, row_bytes):
        """Inside the envelope (a Criteo fm.py / deepfm.py / one_launch dcn.py bundle on the fused path, F <= 64, boundaries
        that give thresholds): the spec on the device and the two staging buffers, parse_path = "device".  Outside: nothing,
        the host parse stays."""
        import torch
        from . import input_pipeline as ip
        if self.path != "fused" or self.manifest["feature_set"] != "criteo" or row_bytes < 1:
            return
        lay, B = self.layout, self.max_batch_size
        if not _lib.lib().rsx_criteo_parse_examples_supported(B, lay.F):
            return
        try:
            a = ip.criteo_parse_spec(lay)
        except _lib.RsxError:               # boundaries without thresholds (unsorted, not finite): the host parse
            return
        dev = self.device
        keep = {k: torch.from_numpy(a[k]).to(dev) for k in ("slot_src", "slot_rows", "thr", "thr_off", "shift")}
        sp = _lib.ParseSpec()
        for k, t in keep.items():
            setattr(sp, k, t.data_ptr())
        sp.F, sp.null_hash = lay.F, a["null_hash"]
        # one staging buffer: int32 offs[n + 1] | (16-byte aligned) the request's bytes | >= 64 bytes of slack
        cap = B * row_bytes
        size = (self._dp_bytes_at(B) + cap + 64 + 15) & ~15
        pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
        # prob [n] | status int32 [n] come back in ONE copy: the output buffer doubles, the status words follow the n probs
        self._prob = torch.zeros(2 * B, dtype=torch.float32, device=dev)
        self._dp = {"spec": sp, "keep": keep, "cap": cap, "size": size, "pinned": pinned, "host": pinned.numpy(),
                    "stage": torch.zeros(size, dtype=torch.uint8, device=dev)}
        self.parse_path = "device"

    @staticmethod
    def _dp_bytes_at(n):
        """Where the request bytes of an n-row request start in the staging buffer."""
        return (4 * (n + 1) + 15) & ~15

    def _parse_launch(self, n):
        import torch
        d = self._dp
        at = self._dp_bytes_at(n)
        base = d["stage"].data_ptr()
        _lib.check(_lib.lib().rsx_criteo_parse_examples(base + at, (d["size"] - at) & ~3, base, int(n), C.byref(d["spec"]),
                                                       self._ids.data_ptr(), self._prob.data_ptr() + 4 * n,
                                                       torch.cuda.current_stream().cuda_stream), "rsx_criteo_parse_examples")
        self._launch(n)

    def _device_parse_chunk(self, chunk):
        """One chunk of serialized Examples -> prob [n] numpy, or None when the chunk has to be parsed on the host (more
        bytes than the staging buffer holds, or an example the device declined)."""
        d, n = self._dp, len(chunk)
        lens = np.fromiter((len(x) for x in chunk), np.int64, n)
        total = int(lens.sum())
        if total > d["cap"]:
            return None
        at = self._dp_bytes_at(n)
        offs = d["host"][:4 * (n + 1)].view(np.int32)
        offs[0] = 0
        np.cumsum(lens, out=offs[1:])
        d["host"][at:at + total] = np.frombuffer(b"".join(chunk), np.uint8)
        used = (at + total + 3) & ~3
        d["stage"][:used].copy_(d["pinned"][:used], non_blocking=True)       # the ONE H2D copy: offs and the bytes in use
        self._run(("examples", n), lambda: self._parse_launch(n))
        out = self._prob[:2 * n].cpu().numpy()                               # prob | status in one D2H copy
        if out[n:].view(np.int32).any():
            return None
        return out[:n]

    # -- the Estimator path -----------------------------------------------------------------------------------------------
    def _layers_setup(self, arrays):
        import torch
        from .estimator import Estimator, RunConfig
        mod = importlib.import_module("recsys_amd." + self.script)
        params = params_from_manifest(self.manifest, self.max_batch_size)
        est = Estimator(mod.model_fn, None, params, RunConfig(use_hip_graph=self.use_hip_graph, device=str(self.device)))
        _build_store(est, self.script)
        load_store_variables(est.store, widen_tensors(self.manifest, arrays))      # (16-bit tables: fp32 on the host first)
        torch.cuda.synchronize()
        self._est = est

    # -- public ------------------------------------------------------------------------------------------------------------
    def _parse(self, serialized):
        from . import input_pipeline as ip
        if self.script == "din":
            return ip.parse_din_examples(serialized, int(self.manifest["params"].get("hist_len", 100)))[0]
        if self.manifest["feature_set"] == "uid_iid":
            return {"ids": parse_uid_iid_examples(serialized, self.layout)}
        return ip.parse_criteo_examples(serialized, self.layout)[0]

    def predict(self, features, raw=False):
        """One parsed batch ({'ids': int32 [B, F]}, + 'cont_log' for xdeepfm.py; din.py: its four id arrays), host or device
        -> {'prob': float32 numpy [B]}: the mapped probabilities when `calibrated`.  raw=True (layers path; what rank_candidates
        asks for): the model's own probabilities whatever `calibrated` says."""
        import torch
        from .estimator import ModeKeys
        if raw and self.calibrated and self.path == "fused":
            raise _lib.RsxError("Predictor: raw=True on the fused path of a calibrated Predictor (the map is part of the request's "
                                "graph); load with calibrated=False")
        B = int(next(iter(features.values())).shape[0])
        out = np.empty(B, np.float32)
        with torch.no_grad():
            for s in range(0, B, self.max_batch_size):
                e = min(B, s + self.max_batch_size)
                if self.path == "fused":
                    ids = features["ids"][s:e]
                    if isinstance(ids, np.ndarray):
                        ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32))
                    prob = self._fused_chunk(ids.to(torch.int32))
                else:
                    part = {k: v[s:e] for k, v in features.items()}
                    prob, _, _ = self._est._infer_step(part, None, ModeKeys.PREDICT)
                    if self.calibrated and not raw:     # never into the Estimator's static graph buffer
                        prob = self._cal.apply(prob.reshape(-1).float().contiguous(), out=self._cal_buf[:e - s])
                out[s:e] = prob.reshape(-1).float().cpu().numpy()
        return {"prob": out}

    def predict_examples(self, serialized):
        """What deepfm/grpc_client.py sends: a list of serialized tf.train.Example byte strings -> {'prob': float32 [n]}."""
        serialized = list(serialized)
        if not serialized:
            return {"prob": np.zeros(0, np.float32)}
        import torch
        out = []
        for s in range(0, len(serialized), self.max_batch_size):
            chunk = serialized[s:s + self.max_batch_size]
            prob = None
            if self._dp is not None:
                with torch.no_grad():
                    prob = self._device_parse_chunk(chunk)
            if prob is None:                # the host parse: no device parse, a chunk over the byte budget, a declined example
                prob = self.predict(self._parse(chunk))["prob"]
            out.append(prob)
        return {"prob": np.concatenate(out)}


def parse_uid_iid_examples(serialized, layout):
    """deepfm/deepfm.py:28-33 AS COMMITTED applied to in-memory serialized Examples (no label needed): -> ids int32 [n, 2]."""
    from .input_pipeline import _p, _pack_serialized
    if not len(serialized):
        raise ValueError("no examples")
    buf, offs, lens = _pack_serialized(serialized)
    n = len(serialized)
    names = (C.c_char_p * 2)(b"u_id", b"i_id")
    out = np.empty((2, n), np.int64)
    _lib.check(_lib.lib().rsx_int64_features_parse_h(_p(buf), _p(offs), _p(lens), n, names, 2, _p(out), 1),
               "rsx_int64_features_parse_h")
    return layout.transform_int64({"u_id": out[0], "i_id": out[1]})
