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
              din.py bundles also answer `rank_candidates(u_iid_seq, u_icat_seq, i_id, i_cate)`: ONE user history against C
              candidate items (or U histories against C candidates each) -> prob [C] / [U, C].
              rank_path == "fused":  ONE launch of rsx_predict_din_rank (csrc/predict_din.hip) over the variables where the
                                rebuilt Estimator's store keeps them; the history is shipped and fetched once, not C times.
              rank_path == "layers": outside that kernel's envelope -- the request expanded on the host to the training-shaped
                                batch (`expand_rank_request`) and answered through `predict`.
              `rank_candidates(..., top_k=k)` returns the k best candidates only, {"prob", "index"} in the order of
              `topk_rows_host`.  topk_path_for(k) == "device" (rank_path == "fused", k <= 1024): rsx_topk_rows (csrc/topk.hip) behind
              every chunk's rank launch keeps the running list on the device, one copy of k pairs ends the request;
              "host": the probabilities as without top_k, then `topk_rows_host`.  The same bits either way.  (`topk_path`
              records where the latest such request selected.)
              `set_catalogue(i_id, i_cate)` keeps the servable items on the device; `recommend(u_iid_seq, u_icat_seq, top_k)`
              then returns the top_k best catalogue entries the user has NOT seen (and that `exclude` does not name),
              {"prob", "item", "index", "count"}; `recommend_host` is the definition.  recommend_path_for(k) == "device":
              per chunk rsx_predict_din_rank_shared (one candidate list for all users) and rsx_topk_rows_excl
              (csrc/topk_excl.hip), the whole request ONE graph, only histories and exclusion ids shipped; "host":
              `rank_candidates` over the catalogue, then `recommend_host`.  The same bits either way.
              `recommend(..., categories=, exclude_categories=, max_per_category=m)` adds category rules: only / never these
              categories, at most m entries of one category.  On the device rsx_topk_rows_rules (csrc/topk_rules.hip) takes
              rsx_topk_rows_excl's place, a bitmap [U, ceil(n_cate / 32)] travels with the exclusion ids, still ONE graph and
              one copy back; `rules_on_device = False` sends such requests to the host path.  The same bits either way.
              `evaluate_recommend(u_iid_seq, u_icat_seq, held_out, ks)` scores that list offline: the exact 0-based rank of every
              held-out item among the eligible catalogue entries (`target_ranks_host` is the definition) and HR / Recall / NDCG @k
              and MRR from the ranks (`ranking_metrics`).  evaluate_recommend_path_for(T) == "device": per block of users ONE
              graph -- the targets' scores, then per chunk rsx_predict_din_rank_shared and rsx_rank_count_rows
              (csrc/rank_count.hip) -- and 8 bytes per (user, slot) copied back; "host": `rank_candidates` over the catalogue,
              then `target_ranks_host`.  The same integers and probability bits either way.
              `build_neighbours(n)` keeps, per catalogue position, the n most similar other entries by cosine similarity of
              the item embedding rows (rsx_rows_dot, csrc/rows_dot.hip, + rsx_topk_rows_excl; `item_neighbours_host` is the
              definition; `similar_items` reads the rows).  `recommend_two_stage(u_iid_seq, u_icat_seq, top_k)` then scores
              only the neighbours of the history's items: two_stage_path_for(k) == "device": ONE graph --
              rsx_din_retrieve_candidates (csrc/retrieve.hip), rsx_predict_din_rank over the users' candidate lists,
              rsx_topk_rows_counted (csrc/topk_counted.hip), a gather of the positions -- and one copy back; "host":
              `retrieve_candidates_host`, `rank_candidates`, `topk_rows_host`.  The same bits either way;
              `recommend_two_stage_host` is the definition.  No back-fill: a list can be shorter than top_k and differs from
              `recommend`'s by design.
              `evaluate_two_stage(u_iid_seq, u_icat_seq, held_out, ks, n_neighbours=m)` scores that list offline: whether the
              retrieval stage kept each held-out item and the exact rank of the kept ones among the user's candidates
              (`two_stage_ranks_host` is the definition; `two_stage_metrics` adds CandRecall and the mean candidate count to
              `ranking_metrics`), for the first m neighbours of the table already built.
              evaluate_two_stage_path_for(T, hist_len, m) == "device": per block of users ONE graph --
              rsx_din_retrieve_candidates, rsx_predict_din_rank, rsx_rank_count_lists (csrc/rank_count_lists.hip) -- and 12
              bytes per (user, slot) copied back; "host": `retrieve_candidates_host`, `rank_candidates`, numpy.  The same
              integers and probability bits either way.
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

FORMAT_VERSION = 1                    # float32 tables; 16-bit tables (`table_dtype`, `encoding`) make a bundle version 2
FORMAT_VERSION_16BIT = 2
TABLE_DTYPES = ("float32", "bfloat16", "float16")
SCRIPTS = ("fm", "deepfm", "xdeepfm", "dcn", "din")
MANIFEST, VARIABLES = "model.json", "variables.npz"
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
def write_bundle(export_dir_base, manifest, tensors):
    """-> `<export_dir_base>/<unix seconds>`, holding model.json and variables.npz.  The bundle is assembled in a temporary
    directory of the same parent and renamed when complete: a reader never sees half a bundle.  (A second export within the
    same second takes the next free second, as tf.estimator's export does.)"""
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


def export_estimator(est, export_dir_base, table_dtype="float32"):
    """Estimator.export_savedmodel's body: the latest checkpoint of est.model_dir as a bundle -> its directory.  table_dtype
    "bfloat16" / "float16": every embedding-row tensor is rounded to it (`quantize_rows`) and stored in it."""
    from . import checkpoint
    script = est.model_fn.__module__.rsplit(".", 1)[-1]
    _check_export(script, table_dtype, module=est.model_fn.__module__)
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
        out = write_bundle(export_dir_base, make_manifest(script, est.params, est.global_step, tensors, table_dtype), tensors)
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


# ---- candidate ranking requests (din.py): pure numpy, no device ----------------------------------------------------------
def expand_rank_request(u_iid_seq, u_icat_seq, i_id, i_cate, hist_len=None):
    """The training-shaped batch that asks `predict` the question of `rank_candidates`: example u * C + c is (candidate c of
    user u, user u's history).  Histories [P'] / [U, P'], candidates [C] / [U, C]; hist_len pads the histories with zeros to
    that length.  -> {'i_id' [U * C], 'i_cate' [U * C], 'u_iid_seq' [U * C, P], 'u_icat_seq' [U * C, P]}, all int32."""
    hi, hc = np.atleast_2d(np.asarray(u_iid_seq)), np.atleast_2d(np.asarray(u_icat_seq))
    ci, cc = np.atleast_2d(np.asarray(i_id)), np.atleast_2d(np.asarray(i_cate))
    U, C = ci.shape
    if hi.shape != hc.shape or ci.shape != cc.shape or hi.shape[0] != U:
        raise _lib.RsxError("expand_rank_request: histories %s / %s and candidates %s / %s do not describe U users"
                            % (hi.shape, hc.shape, ci.shape, cc.shape))
    P = hi.shape[1] if hist_len is None else int(hist_len)
    if hi.shape[1] > P:
        raise _lib.RsxError("expand_rank_request: a history of length %d does not fit hist_len %d" % (hi.shape[1], P))
    out = {"i_id": ci.reshape(-1).astype(np.int32), "i_cate": cc.reshape(-1).astype(np.int32)}
    for k, h in (("u_iid_seq", hi), ("u_icat_seq", hc)):
        e = np.zeros((U, C, P), np.int32)
        e[:, :, :h.shape[1]] = h[:, None, :]
        out[k] = e.reshape(U * C, P)
    return out


def _is_int_array(x):
    dt = getattr(x, "dtype", None)
    if dt is None:
        return False
    if isinstance(x, np.ndarray):
        return np.issubdtype(dt, np.integer)
    return (not dt.is_floating_point) and (not dt.is_complex) and str(dt) != "torch.bool"


def check_rank_request(u_iid_seq, u_icat_seq, i_id, i_cate, hist_len, n_item, n_cate):
    """Argument checking of `Predictor.rank_candidates` (no device needed).  Accepts numpy arrays or torch tensors of any
    integer dtype (lists become numpy).  -> (U, C, P', single): `single` when the request was one user's 1-D arrays.
    Refuses (RsxError): non-integer inputs, shapes that are not [P'] + [C] or [U, P'] + [U, C], an empty request, a history
    longer than the bundle's hist_len (both lengths named), and -- for HOST inputs only, device inputs are trusted as in
    `predict` -- ids outside [0, n_item) / [0, n_cate)."""
    arrs = []
    for name, x in (("u_iid_seq", u_iid_seq), ("u_icat_seq", u_icat_seq), ("i_id", i_id), ("i_cate", i_cate)):
        if not hasattr(x, "shape") or not hasattr(x, "dtype"):
            x = np.asarray(x)
        if not _is_int_array(x):
            raise _lib.RsxError("rank_candidates: %s must hold integers, not %s" % (name, x.dtype))
        arrs.append(x)
    hi, hc, ci, cc = arrs
    nd = len(ci.shape)
    if nd not in (1, 2) or len(hi.shape) != nd or tuple(hi.shape) != tuple(hc.shape) or tuple(ci.shape) != tuple(cc.shape):
        raise _lib.RsxError("rank_candidates: expected histories [P] with candidates [C], or [U, P] with [U, C]; got u_iid_seq %s, "
                            "u_icat_seq %s, i_id %s, i_cate %s" % (tuple(hi.shape), tuple(hc.shape), tuple(ci.shape), tuple(cc.shape)))
    U = 1 if nd == 1 else int(ci.shape[0])
    C, Pq = int(ci.shape[-1]), int(hi.shape[-1])
    if nd == 2 and int(hi.shape[0]) != U:
        raise _lib.RsxError("rank_candidates: %d histories for %d rows of candidates" % (int(hi.shape[0]), U))
    if U < 1 or C < 1:
        raise _lib.RsxError("rank_candidates: an empty request (U = %d users, C = %d candidates)" % (U, C))
    if Pq > int(hist_len):
        raise _lib.RsxError("rank_candidates: a history of length %d does not fit this bundle's hist_len %d" % (Pq, int(hist_len)))
    for name, x, hi_ in (("u_iid_seq", hi, n_item), ("u_icat_seq", hc, n_cate), ("i_id", ci, n_item), ("i_cate", cc, n_cate)):
        if not getattr(x, "is_cuda", False) and int(np.prod(tuple(x.shape))) and (int(x.min()) < 0 or int(x.max()) >= int(hi_)):
            raise _lib.RsxError("rank_candidates: %s holds ids outside [0, %d) (min %d, max %d)" % (name, int(hi_), int(x.min()), int(x.max())))
    return U, C, Pq, nd == 1


TOPK_MAX_K = 1024                     # include/rsx.h rsx_topk_rows: the largest k selected on the device


def check_top_k(top_k):
    """`rank_candidates`' top_k argument -> int; RsxError unless it is an integer (Python or numpy, no bool) >= 1."""
    if isinstance(top_k, (bool, np.bool_)) or not isinstance(top_k, (int, np.integer)) or int(top_k) < 1:
        raise _lib.RsxError("rank_candidates: top_k must be an integer >= 1, not %r" % (top_k,))
    return int(top_k)


def topk_rows_host(prob, k):
    """The k best entries of every row of `prob` ([C] or [U, C], float32) in the order of rsx_topk_rows (include/rsx.h): a
    higher value first, equal values (-0.0 == +0.0) by the lower index, every NaN after every number and NaNs by index --
    np.lexsort((index, -value)).  -> {'prob': float32 [k'] / [U, k'] (the input's bits), 'index': int32, same shape},
    k' = min(k, C).  Pure numpy: the host form of `rank_candidates(top_k=k)` and the checker of the device form."""
    k = check_top_k(k)
    a = np.asarray(prob, np.float32)
    if a.ndim not in (1, 2) or a.shape[-1] < 1:
        raise _lib.RsxError("topk_rows_host: expected scores [C] or [U, C] with C >= 1, got %s" % (a.shape,))
    rows = np.atleast_2d(a)
    kk = min(k, rows.shape[1])
    index = np.broadcast_to(np.arange(rows.shape[1], dtype=np.int64), rows.shape)
    order = np.lexsort((index, -rows), axis=-1)[:, :kk]
    out = {"prob": np.take_along_axis(rows, order, 1), "index": order.astype(np.int32)}
    return out if a.ndim == 2 else {key: v[0] for key, v in out.items()}


# ---- recommendation over a resident catalogue (din.py): pure numpy, no device -------------------------------------------------
EXCL_MAX = 256                        # include/rsx.h rsx_topk_rows_excl: the longest exclusion list of a user on the device


def check_catalogue(i_id, i_cate, n_item, n_cate):
    """Argument checking of `Predictor.set_catalogue` (no device needed): two 1-D integer arrays of equal length N >= 1 (numpy
    or torch, any integer dtype; lists become numpy) with ids inside [0, n_item) / [0, n_cate) -> (i_id, i_cate) as int32
    numpy.  Duplicates and item id 0 are allowed: a position is what identifies an entry."""
    out = []
    for name, x in (("i_id", i_id), ("i_cate", i_cate)):
        if not hasattr(x, "shape") or not hasattr(x, "dtype"):
            x = np.asarray(x)
        if not _is_int_array(x):
            raise _lib.RsxError("set_catalogue: %s must hold integers, not %s" % (name, x.dtype))
        if not isinstance(x, np.ndarray):
            x = x.detach().cpu().numpy()
        out.append(x)
    ci, cc = out
    if ci.ndim != 1 or cc.ndim != 1 or ci.shape != cc.shape:
        raise _lib.RsxError("set_catalogue: expected two 1-D arrays of equal length, got i_id %s and i_cate %s" % (ci.shape, cc.shape))
    if ci.shape[0] < 1:
        raise _lib.RsxError("set_catalogue: an empty catalogue")
    for name, x, hi in (("i_id", ci, n_item), ("i_cate", cc, n_cate)):
        if int(x.min()) < 0 or int(x.max()) >= int(hi):
            raise _lib.RsxError("set_catalogue: %s holds ids outside [0, %d) (min %d, max %d)" % (name, int(hi), int(x.min()), int(x.max())))
    return np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(cc, np.int32)


def _exclusion_ids(hist_item, exclude, U, exclude_seen):
    """-> int64 [U, E'']: the ids a request names for exclusion, user by user (the history when exclude_seen, then `exclude`);
    RsxError when `exclude` does not have the histories' leading shape."""
    parts = []
    h = hist_item.detach().cpu().numpy() if hasattr(hist_item, "detach") else np.asarray(hist_item)
    single = h.ndim == 1
    if exclude_seen:
        parts.append(h.reshape(U, -1).astype(np.int64))
    if exclude is not None:
        e = exclude.detach().cpu().numpy() if hasattr(exclude, "detach") else np.asarray(exclude)
        if e.size and not np.issubdtype(e.dtype, np.integer):
            raise _lib.RsxError("recommend: exclude must hold integers, not %s" % e.dtype)
        if e.ndim != h.ndim or (not single and e.shape[0] != U):
            raise _lib.RsxError("recommend: exclude %s does not match the histories %s: [E] for one user, [U, E] for U users"
                                % (tuple(e.shape), tuple(h.shape)))
        parts.append(e.reshape(U, -1).astype(np.int64))
    return np.concatenate(parts, 1) if parts else np.zeros((U, 0), np.int64)


RULES_MAX_M = 16                      # include/rsx.h rsx_topk_rows_rules: the largest per-category cap applied on the device


def check_max_per_category(max_per_category):
    """`recommend`'s max_per_category -> None (no cap) or int; RsxError unless it is None or an integer (no bool) >= 1."""
    m = max_per_category
    if m is None:
        return None
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or int(m) < 1:
        raise _lib.RsxError("recommend: max_per_category must be None or an integer >= 1, not %r" % (m,))
    return int(m)


def check_category_list(x, name, U, single, n_cate=None):
    """`recommend`'s categories / exclude_categories -> None or int64 [U, G'].  The shape convention of `exclude`: [G'] for the
    one-user form, [U, G'] for U users; negative ids are padding, 0 is a category.  RsxError for non-integers, another shape,
    and -- when n_cate is given -- ids >= n_cate."""
    if x is None:
        return None
    c = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    if (c.size and not np.issubdtype(c.dtype, np.integer)) or c.dtype == np.bool_:
        raise _lib.RsxError("recommend: %s must hold integers, not %s" % (name, c.dtype))
    if c.ndim != (1 if single else 2) or (not single and c.shape[0] != U):
        raise _lib.RsxError("recommend: %s %s does not match the histories: [G] for one user, [U, G] for U = %d users"
                            % (name, tuple(c.shape), U))
    c = c.reshape(U, -1).astype(np.int64)
    if n_cate is not None and c.size and int(c.max()) >= int(n_cate):
        raise _lib.RsxError("recommend: %s holds ids outside [0, %d) (max %d); negative ids are padding" % (name, int(n_cate), int(c.max())))
    return c


def category_bitmap(categories, exclude_categories, n_cate):
    """The two checked lists (`check_category_list`: int64 [U, G'] or None, at least one given) folded into the bitmap
    rsx_topk_rows_rules takes: uint32 [U, ceil(n_cate / 32)], bit g of row u set when category g is allowed for user u."""
    U = (categories if categories is not None else exclude_categories).shape[0]
    ok = np.zeros((U, 32 * ((int(n_cate) + 31) // 32)), bool)
    for u in range(U):
        if categories is None:
            ok[u, :int(n_cate)] = True
        else:
            ok[u, categories[u][categories[u] >= 0]] = True
        if exclude_categories is not None:
            ok[u, exclude_categories[u][exclude_categories[u] >= 0]] = False
    return np.packbits(ok.reshape(U, -1, 32), axis=-1, bitorder="little").view(np.uint32).reshape(U, -1)


def recommend_host(prob, cat_item, hist_item, exclude, top_k, exclude_seen=True, cat_cate=None, categories=None,
                   exclude_categories=None, max_per_category=None, n_cate=None):
    """The definition of `Predictor.recommend`, in numpy.  prob: float32 [N] (one user) or [U, N], the scores of the N catalogue
    entries; cat_item: int [N], their item ids; hist_item: [P'] / [U, P']; exclude: None or [E'] / [U, E'].  An entry is
    EXCLUDED for user u when its item id equals a positive id of hist_item[u] (if exclude_seen) or of exclude[u]; ids <= 0 are
    padding.  The eligible entries, with their catalogue positions, in the order of `topk_rows_host` (higher score first, equal
    ones by the lower position, NaN last), the first top_k of them ->
    {'prob': float32 [U, kk], 'item': int32 [U, kk], 'index': int32 [U, kk], 'count': int32 [U]}, kk = min(top_k, N),
    count[u] = min(top_k, eligible entries of u); entries at and beyond count[u] are NaN / -1 / -1.  The one-user form returns
    the three arrays cut to count, and count as an int.
    CATEGORY RULES (all off by default; any of them needs cat_cate: int [N], the category of every catalogue entry -- what
    `set_catalogue` was given, not a table lookup).  categories / exclude_categories: [G'] / [U, G'] like `exclude`, negative
    ids padding, 0 a real category, ids >= n_cate refused when n_cate is given.  An entry is ALLOWED when its category is in
    categories[u] (if given; an empty list allows nothing) and not in exclude_categories[u] (if given); the eligible entries are
    the allowed ones that are not excluded.  max_per_category = m (an integer >= 1): walk the eligible entries in the order
    above and keep an entry only when fewer than m kept entries of its category precede it; stop at top_k.  The cap counts
    entries -- an item id at two positions counts twice -- and count[u] can stay below top_k while eligible entries remain."""
    k = check_top_k(top_k)
    a = np.asarray(prob, np.float32)
    cat = np.asarray(cat_item)
    if a.ndim not in (1, 2) or cat.ndim != 1 or a.shape[-1] != cat.shape[0] or cat.shape[0] < 1:
        raise _lib.RsxError("recommend_host: expected scores [N] or [U, N] over a catalogue [N], N >= 1; got %s and %s" % (a.shape, cat.shape))
    rows = np.atleast_2d(a)
    U, N = rows.shape
    ids = _exclusion_ids(hist_item, exclude, U, exclude_seen)
    m = check_max_per_category(max_per_category)
    only = check_category_list(categories, "categories", U, a.ndim == 1, n_cate)
    deny = check_category_list(exclude_categories, "exclude_categories", U, a.ndim == 1, n_cate)
    rules = m is not None or only is not None or deny is not None
    if rules:
        cc = None if cat_cate is None else np.asarray(cat_cate)
        if cc is None or cc.shape != cat.shape or not np.issubdtype(cc.dtype, np.integer):
            raise _lib.RsxError("recommend_host: a category rule needs cat_cate, integers [N] like cat_item; got %s"
                                % (None if cc is None else (cc.dtype, cc.shape),))
    kk = min(k, N)
    out = {"prob": np.full((U, kk), np.nan, np.float32), "item": np.full((U, kk), -1, np.int32),
           "index": np.full((U, kk), -1, np.int32), "count": np.zeros(U, np.int32)}
    for u in range(U):
        gone = np.isin(cat, ids[u][ids[u] > 0])
        if only is not None:
            gone |= ~np.isin(cc, only[u][only[u] >= 0])
        if deny is not None:
            gone |= np.isin(cc, deny[u][deny[u] >= 0])
        pos = np.flatnonzero(~gone)
        order = pos[np.lexsort((pos, -rows[u, pos]))]
        if m is None:
            order = order[:kk]
        else:                                                          # the cap: the plain greedy walk
            taken, keep = {}, []
            for p in order:
                g = int(cc[p])
                if taken.get(g, 0) < m:
                    taken[g] = taken.get(g, 0) + 1
                    keep.append(p)
                    if len(keep) == kk:
                        break
            order = np.asarray(keep, order.dtype)
        c = len(order)
        out["prob"][u, :c], out["item"][u, :c], out["index"][u, :c], out["count"][u] = rows[u, order], cat[order], order, c
    return out if a.ndim == 2 else _one_user(out)


def _one_user(out):
    c = int(out["count"][0])
    return {"prob": out["prob"][0, :c], "item": out["item"][0, :c], "index": out["index"][0, :c], "count": c}


# ---- offline ranking metrics over the catalogue (din.py): pure numpy, no device -------------------------------------------
RANK_MISSING = -1                     # a held-out id that is not in the catalogue, or whose entry is itself excluded
RANK_PAD = -2                         # a padding slot of held_out (id <= 0)
RANK_MAX_T = 32                       # include/rsx.h rsx_rank_count_rows: the most targets of a user on the device


def catalogue_first_positions(cat_item):
    """cat_item int [N] -> (the distinct ids ascending, int64; the LOWEST catalogue position of each, int64): the index that
    resolves a held-out id to its target entry."""
    ids, first = np.unique(np.asarray(cat_item).astype(np.int64), return_index=True)
    return ids, first.astype(np.int64)


def check_held_out(held_out, U, single, what="target_ranks_host"):
    """held_out: integers, [T] for the one-user form and [U, T] otherwise, T >= 1; no positive id twice in a row -> int64
    [U, T].  RsxError otherwise."""
    h = held_out.detach().cpu().numpy() if hasattr(held_out, "detach") else np.asarray(held_out)
    if not np.issubdtype(h.dtype, np.integer):
        raise _lib.RsxError("%s: held_out must hold integers, not %s" % (what, h.dtype))
    if h.ndim != (1 if single else 2) or (not single and h.shape[0] != U) or h.shape[-1] < 1:
        raise _lib.RsxError("%s: held_out %s does not match the request: [T] for one user, [U, T] for U = %d users, T >= 1"
                            % (what, tuple(h.shape), U))
    h = h.reshape(U, -1).astype(np.int64)
    for u in range(U):
        pos = h[u][h[u] > 0]
        if len(np.unique(pos)) != len(pos):
            raise _lib.RsxError("%s: held_out names an item twice for user %d" % (what, u))
    return h


def _target_positions(index, held):
    """held int64 [U, T] -> int64 [U, T]: the target entry's catalogue position, RANK_MISSING for an id the catalogue does not
    hold, RANK_PAD for padding.  index: `catalogue_first_positions`."""
    ids, first = index
    at = np.minimum(np.searchsorted(ids, held), len(ids) - 1)
    pos = np.where(ids[at] == held, first[at], RANK_MISSING)
    return np.where(held > 0, pos, RANK_PAD)


def target_ranks_host(prob, cat_item, hist_item, held_out, exclude=None, exclude_seen=True):
    """The definition of `Predictor.evaluate_recommend`'s ranks, in numpy.  prob: float32 [N] (one user) or [U, N], the scores
    of the N catalogue entries; cat_item: int [N]; hist_item: [P'] / [U, P']; held_out: int [T] / [U, T], ids <= 0 are padding;
    exclude: None or [E'] / [U, E'].  For every non-padding id the TARGET ENTRY is the lowest catalogue position that holds it,
    and its rank is the number of ELIGIBLE entries that come before the target entry in `recommend_host`'s order (a higher
    score first, equal scores -- -0.0 == +0.0 -- by the lower position, every NaN after every number): 0-based, the index at
    which that position stands in recommend_host(..., top_k=N)['index'].  Eligibility is recommend_host's: an entry is excluded
    when its item id is a positive id of the history (if exclude_seen) or of `exclude`.  The user's other held-out items stay
    eligible and compete.  -> int32 [U, T] ([T] for one user): the rank, RANK_MISSING (-1) for an id that is not in the
    catalogue or whose entry is excluded, RANK_PAD (-2) for padding.  The same positive id twice in a row: RsxError.
    Written by counting, not by sorting: entry j precedes the target p when score[j] > score[p], or they are equal and j < p;
    when score[p] is a NaN, every number precedes it and so do the NaNs at lower positions."""
    a = np.asarray(prob, np.float32)
    cat = np.asarray(cat_item)
    if a.ndim not in (1, 2) or cat.ndim != 1 or a.shape[-1] != cat.shape[0] or cat.shape[0] < 1:
        raise _lib.RsxError("target_ranks_host: expected scores [N] or [U, N] over a catalogue [N], N >= 1; got %s and %s" % (a.shape, cat.shape))
    rows = np.atleast_2d(a)
    U, N = rows.shape
    held = check_held_out(held_out, U, a.ndim == 1)
    ids = _exclusion_ids(hist_item, exclude, U, exclude_seen)
    pos = _target_positions(catalogue_first_positions(cat), held)
    where = np.arange(N)
    out = np.where(pos >= 0, RANK_MISSING, pos).astype(np.int32)
    for u in range(U):
        eligible = ~np.isin(cat, ids[u][ids[u] > 0])
        s, nan = rows[u], np.isnan(rows[u])
        for t in np.flatnonzero(pos[u] >= 0):
            p = int(pos[u, t])
            if not eligible[p]:
                continue
            before = ~nan | (where < p) if nan[p] else (s > s[p]) | ((s == s[p]) & (where < p))
            out[u, t] = np.count_nonzero(before & eligible)
    return out if a.ndim == 2 else out[0]


def check_ks(ks):
    """`ranking_metrics`' ks -> a list of ints; RsxError unless every one is an integer (no bool) >= 1."""
    try:
        ks = list(ks)
    except TypeError:
        raise _lib.RsxError("ranking_metrics: ks must be an iterable of integers >= 1, not %r" % (ks,))
    for k in ks:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or int(k) < 1:
            raise _lib.RsxError("ranking_metrics: ks must hold integers >= 1, not %r" % (k,))
    return [int(k) for k in ks]


def ranking_metrics(rank, ks, per_user=False):
    """rank: int [U, T] (or [T], one user) from `target_ranks_host` / `evaluate_recommend`; ks: integers >= 1.  In float64, per
    user first, then the mean over the users with at least one non-padding slot (NaN when there is none).  With n_u the
    non-padding slots of user u (RANK_MISSING slots count: they are misses) and hits_k the slots with 0 <= rank < k:
      'HR@k'      hits_k > 0
      'Recall@k'  hits_k / min(k, n_u)
      'NDCG@k'    sum over the hits of 1 / log2(rank + 2), over the sum for i < min(k, n_u) of 1 / log2(i + 2) (binary relevance)
      'MRR'       1 / (1 + the lowest non-negative rank), 0 without one
    and 'users' (those users) and 'missing' (the RANK_MISSING slots).  per_user=True adds the per-user float64 [U] arrays under
    the same keys suffixed '_user' (NaN for a user without a slot)."""
    ks = check_ks(ks)
    r = np.asarray(rank)
    if r.ndim not in (1, 2) or not np.issubdtype(r.dtype, np.integer) or r.size < 1 or int(r.min()) < RANK_PAD:
        raise _lib.RsxError("ranking_metrics: rank must be integers >= %d of shape [T] or [U, T], T >= 1, got %s %s" % (RANK_PAD, r.dtype, r.shape))
    r = np.atleast_2d(r).astype(np.int64)
    n_u = np.count_nonzero(r != RANK_PAD, axis=1)
    users = n_u > 0
    found = r >= 0
    gain = np.where(found, 1.0 / np.log2(np.where(found, r, 0) + 2.0), 0.0)
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(r.shape[1]) + 2.0))])     # ideal[m]: m hits at ranks 0 .. m - 1
    per = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in ks:
            hit = found & (r < k)
            m = np.minimum(k, n_u)
            per["HR@%d" % k] = np.where(users, (hit.sum(1) > 0).astype(np.float64), np.nan)
            per["Recall@%d" % k] = np.where(users, hit.sum(1) / m.astype(np.float64), np.nan)
            per["NDCG@%d" % k] = np.where(users, np.where(hit, gain, 0.0).sum(1) / ideal[m], np.nan)
        best = np.where(found, r, np.iinfo(np.int64).max).min(1)
        per["MRR"] = np.where(users, np.where(found.any(1), 1.0 / (1.0 + np.where(found.any(1), best, 0)), 0.0), np.nan)
    out = {"users": int(users.sum()), "missing": int(np.count_nonzero(r == RANK_MISSING))}
    for key, v in per.items():
        out[key] = float(v[users].mean()) if users.any() else float("nan")
        if per_user:
            out[key + "_user"] = v
    return out


# ---- two-stage recommendation: item neighbours and candidate retrieval (din.py): pure numpy, no device -------------------------
NBR_MAX = 64                          # include/rsx.h rsx_din_retrieve_candidates: the most neighbours kept per catalogue entry


def check_n_neighbours(n_neighbours):
    """`build_neighbours`' argument -> int; RsxError unless it is an integer (no bool) in [1, 64]."""
    n = n_neighbours
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= NBR_MAX:
        raise _lib.RsxError("build_neighbours: n_neighbours must be an integer in [1, %d], not %r" % (NBR_MAX, n))
    return int(n)


def unit_rows_host(E):
    """E: float [N, K] embedding rows -> float32 [N, K]: every row divided by its float64 norm and rounded to float32; a
    zero-norm row stays all +0.0.  RsxError for a non-finite entry.  This is what `build_neighbours` uploads: the device
    never normalises."""
    e = np.asarray(E, np.float64)
    if e.ndim != 2 or e.shape[0] < 1 or e.shape[1] < 1:
        raise _lib.RsxError("unit_rows_host: expected embedding rows [N, K], got %s" % (e.shape,))
    if not np.isfinite(e).all():
        raise _lib.RsxError("unit_rows_host: a non-finite embedding (row %d)" % int(np.flatnonzero(~np.isfinite(e).all(1))[0]))
    norm = np.sqrt((e * e).sum(1))
    out = np.zeros(e.shape, np.float32)
    nz = norm > 0
    out[nz] = (e[nz] / norm[nz, None]).astype(np.float32)
    return out


def rows_dot_host(A, q_rows, first, n):
    """The arithmetic of rsx_rows_dot (include/rsx.h) in numpy: A float32 [N, K], q_rows int [Q] ->
    float32 [Q, n], out[q, j] = dot(A[q_rows[q]], A[first + j]) as `s = +0.0f; for d in 0 .. K - 1: s = s + a[d] * b[d]`,
    strictly ascending in d, every product and every sum rounded to float32, no fused multiply-add."""
    A = np.asarray(A, np.float32)
    q = np.asarray(q_rows, np.int64).reshape(-1)
    first, n = int(first), int(n)
    if A.ndim != 2 or first < 0 or n < 1 or first + n > A.shape[0] or (q.size and (q.min() < 0 or q.max() >= A.shape[0])):
        raise _lib.RsxError("rows_dot_host: rows [%d, %d) or the query rows are outside A %s" % (first, first + n, A.shape))
    a, b = A[q], A[first:first + n]
    s = np.zeros((len(q), n), np.float32)
    for d in range(A.shape[1]):
        s = s + a[:, d, None] * b[None, :, d]                          # (two float32 ufuncs: a rounded product, a rounded sum)
    return s


def item_neighbours_host(unit, cat_item, n, block=512):
    """The definition of `build_neighbours`' table.  unit: float32 [N, K] (`unit_rows_host` of the catalogue entries' item
    embeddings); cat_item: int [N]; n in [1, 64].  For position i with cat_item[i] > 0: the n best positions j by
    `rows_dot_host` similarity in the ORDER of rsx_topk_rows (higher similarity first, equal ones by the lower position), every
    j with cat_item[j] == cat_item[i] left out -- i itself and the duplicates of its item.  A position with item id 0 (history
    padding, never a seed) gets an empty row; it may still be another entry's neighbour.
    -> (nbr_pos int32 [N, n], nbr_sim float32 [N, n], nbr_count int32 [N]), -1 / NaN beyond the count."""
    n = check_n_neighbours(n)
    unit = np.asarray(unit, np.float32)
    cat = np.asarray(cat_item).astype(np.int64)
    N = cat.shape[0]
    if unit.ndim != 2 or unit.shape[0] != N or cat.ndim != 1:
        raise _lib.RsxError("item_neighbours_host: unit rows %s do not match the catalogue %s" % (unit.shape, cat.shape))
    pos = np.full((N, n), -1, np.int32)
    sim = np.full((N, n), np.nan, np.float32)
    count = np.zeros(N, np.int32)
    cols = np.arange(N, dtype=np.int64)
    for s in range(0, N, block):
        rows = np.arange(s, min(N, s + block))
        score = rows_dot_host(unit, rows, 0, N)
        for r, i in enumerate(rows):
            if cat[i] <= 0:
                continue
            ok = cols[cat != cat[i]]
            order = ok[np.lexsort((ok, -score[r, ok]))][:n]
            c = len(order)
            pos[i, :c], sim[i, :c], count[i] = order, score[r, order], c
    return pos, sim, count


def check_neighbours(nbr_pos, nbr_count, N):
    pos, cnt = np.asarray(nbr_pos), np.asarray(nbr_count)
    if pos.ndim != 2 or cnt.shape != (pos.shape[0],) or pos.shape[0] != N:
        raise _lib.RsxError("neighbour table %s / %s does not match the catalogue [%d]" % (pos.shape, cnt.shape, N))
    return pos, cnt


def retrieve_candidates_host(nbr_pos, nbr_count, cat_item, hist_item, exclude=None, exclude_seen=True):
    """The definition of `Predictor.retrieve_candidates`, in numpy.  nbr_pos [N, n] / nbr_count [N]: `item_neighbours_host`'s
    table; cat_item int [N]; hist_item [P'] / [U, P']; exclude None or [E'] / [U, E'].  Per user: the SEEDS are the positive
    history ids that occur in the catalogue, each resolved to its lowest position (`catalogue_first_positions`); the candidates
    are the union of the seeds' neighbour rows -- with exclude_seen=False joined by every position whose item id is a seed id
    -- without every position whose item id is a positive id of the exclusion list (`_exclusion_ids`: the history when
    exclude_seen, then `exclude`; the list `recommend` uses).  -> a list of U int32 arrays: the sorted distinct positions."""
    cat = np.asarray(cat_item).astype(np.int64)
    N = cat.shape[0]
    pos, cnt = check_neighbours(nbr_pos, nbr_count, N)
    h = hist_item.detach().cpu().numpy() if hasattr(hist_item, "detach") else np.asarray(hist_item)
    if h.ndim not in (1, 2):
        raise _lib.RsxError("retrieve_candidates_host: expected histories [P] or [U, P], got %s" % (h.shape,))
    U = 1 if h.ndim == 1 else h.shape[0]
    ids = _exclusion_ids(h, exclude, U, exclude_seen)
    index = catalogue_first_positions(cat)
    hist = h.reshape(U, -1).astype(np.int64)
    out = []
    for u in range(U):
        at = _target_positions(index, hist[u][None, :])[0] if hist.shape[1] else np.zeros(0, np.int64)
        at = at[at >= 0]                                               # (padding and ids the catalogue does not hold are < 0)
        mark = np.zeros(N, bool)
        for a in at:
            mark[pos[a, :cnt[a]]] = True
        if not exclude_seen:
            mark |= np.isin(cat, cat[at])
        mark &= ~np.isin(cat, ids[u][ids[u] > 0])
        out.append(np.flatnonzero(mark).astype(np.int32))
    return out


def recommend_two_stage_host(prob, nbr_pos, nbr_count, cat_item, hist_item, exclude, top_k, exclude_seen=True):
    """The definition of `Predictor.recommend_two_stage`, in numpy.  prob: float32 [N] (one user) or [U, N], the scores of ALL
    catalogue entries (`rank_candidates` over the whole catalogue).  `recommend_host`'s order (higher score first, equal ones
    by the lower position, NaN last) restricted to the positions `retrieve_candidates_host` gives ->
    `recommend_host`'s dictionary, kk = min(top_k, N), count[u] = min(top_k, candidates of u): it can stay below top_k and can
    be 0 -- nothing is filled in from the rest of the catalogue."""
    k = check_top_k(top_k)
    a = np.asarray(prob, np.float32)
    cat = np.asarray(cat_item)
    if a.ndim not in (1, 2) or cat.ndim != 1 or a.shape[-1] != cat.shape[0] or cat.shape[0] < 1:
        raise _lib.RsxError("recommend_two_stage_host: expected scores [N] or [U, N] over a catalogue [N], N >= 1; got %s and %s"
                            % (a.shape, cat.shape))
    rows = np.atleast_2d(a)
    U, N = rows.shape
    cands = retrieve_candidates_host(nbr_pos, nbr_count, cat, hist_item, exclude, exclude_seen)
    if len(cands) != U:
        raise _lib.RsxError("recommend_two_stage_host: %d histories for %d rows of scores" % (len(cands), U))
    kk = min(k, N)
    out = {"prob": np.full((U, kk), np.nan, np.float32), "item": np.full((U, kk), -1, np.int32),
           "index": np.full((U, kk), -1, np.int32), "count": np.zeros(U, np.int32)}
    for u, pos in enumerate(cands):
        pos = pos.astype(np.int64)
        order = pos[np.lexsort((pos, -rows[u, pos]))][:kk]
        c = len(order)
        out["prob"][u, :c], out["item"][u, :c], out["index"][u, :c], out["count"][u] = rows[u, order], cat[order], order, c
    return out if a.ndim == 2 else _one_user(out)


def candidate_capacity(N, hist_len, n_neighbours):
    """Columns of a user's candidate list: min(N, hist_len * (n + 1)) -- every seed, its n neighbours -- rounded up to 64."""
    c = max(1, min(int(N), int(hist_len) * (int(n_neighbours) + 1)))
    return (c + 63) // 64 * 64


# ---- offline evaluation of the two-stage list (din.py): pure numpy, no device -------------------------------------------------
RETRIEVED_PAD, RETRIEVED_MISSING = -2, -1     # `retrieved` of a padding slot / of an id outside the catalogue or excluded


def _list_place(s, c):
    """The number of entries of the float32 list s that precede entry c in `recommend_host`'s order, by counting: j precedes c
    when s[j] > s[c], or they are equal (-0.0 == +0.0) and j < c; when s[c] is a NaN, every number and the NaNs before c."""
    where = np.arange(len(s))
    if np.isnan(s[c]):
        return int(np.count_nonzero(~np.isnan(s) | (where < c)))
    return int(np.count_nonzero((s > s[c]) | ((s == s[c]) & (where < c))))


def two_stage_ranks_host(prob, nbr_pos, nbr_count, cat_item, hist_item, held_out, exclude=None, exclude_seen=True):
    """The definition of `Predictor.evaluate_two_stage`'s ranks, in numpy.  prob: float32 [N] (one user) or [U, N], the scores of
    ALL catalogue entries, as for `recommend_two_stage_host`; held_out: int [T] / [U, T] (`check_held_out`).  Per user the
    candidates are `retrieve_candidates_host(...)`.  For a held-out id h > 0:
      - h is not in the catalogue, or is a positive id of the exclusion list (`_exclusion_ids`): rank = RANK_MISSING,
        retrieved = -1;
      - else no candidate position holds h: rank = RANK_MISSING, retrieved = 0 -- a miss of the retrieval stage is a miss of
        the list;
      - else the TARGET ENTRY is the lowest CANDIDATE position that holds h -- not the lowest catalogue position: a duplicate
        entry can be a neighbour where the first copy is not, all copies score the same bits, and the lowest candidate copy is
        the one the list shows first -- rank = the number of candidates that precede it in `recommend_host`'s order (a higher
        score first, equal scores -- -0.0 == +0.0 -- by the lower position, every NaN after every number): the index at which
        that position stands in recommend_two_stage_host(..., top_k=N)['index']; retrieved = 1.
    Padding (h <= 0): rank = RANK_PAD, retrieved = -2.
    -> {'rank': int32 [U, T], 'retrieved': int8 [U, T], 'target_index': int32 [U, T] (the target entry's catalogue position,
    -1 where retrieved != 1), 'target_prob': float32 [U, T] (NaN where retrieved != 1), 'n_candidates': int32 [U]}; the
    one-user form drops the leading axis and n_candidates is an int.  Written by counting, as `target_ranks_host` is."""
    a = np.asarray(prob, np.float32)
    cat = np.asarray(cat_item)
    if a.ndim not in (1, 2) or cat.ndim != 1 or a.shape[-1] != cat.shape[0] or cat.shape[0] < 1:
        raise _lib.RsxError("two_stage_ranks_host: expected scores [N] or [U, N] over a catalogue [N], N >= 1; got %s and %s"
                            % (a.shape, cat.shape))
    rows = np.atleast_2d(a)
    U, N = rows.shape
    held = check_held_out(held_out, U, a.ndim == 1, "two_stage_ranks_host")
    cands = retrieve_candidates_host(nbr_pos, nbr_count, cat, hist_item, exclude, exclude_seen)
    if len(cands) != U:
        raise _lib.RsxError("two_stage_ranks_host: %d histories for %d rows of scores" % (len(cands), U))
    ids = _exclusion_ids(hist_item, exclude, U, exclude_seen)
    cat = cat.astype(np.int64)
    T = held.shape[1]
    out = {"rank": np.full((U, T), RANK_PAD, np.int32), "retrieved": np.full((U, T), RETRIEVED_PAD, np.int8),
           "target_index": np.full((U, T), -1, np.int32), "target_prob": np.full((U, T), np.nan, np.float32),
           "n_candidates": np.asarray([len(x) for x in cands], np.int32)}
    for u in range(U):
        pos = cands[u].astype(np.int64)
        s, cid = rows[u, pos], cat[pos]
        known = np.isin(held[u], cat) & ~np.isin(held[u], ids[u][ids[u] > 0])
        for t in np.flatnonzero(held[u] > 0):
            at = np.flatnonzero(cid == held[u, t])
            if not known[t] or not len(at):
                out["rank"][u, t], out["retrieved"][u, t] = RANK_MISSING, 0 if known[t] else RETRIEVED_MISSING
                continue
            c = int(at[0])
            out["rank"][u, t], out["retrieved"][u, t] = _list_place(s, c), 1
            out["target_index"][u, t], out["target_prob"][u, t] = pos[c], s[c]
    if a.ndim == 2:
        return out
    return {key: (int(v[0]) if key == "n_candidates" else v[0]) for key, v in out.items()}


def two_stage_metrics(rank, retrieved, n_candidates, ks, per_user=False):
    """`ranking_metrics(rank, ks, per_user)` unchanged, plus what the retrieval stage kept.  retrieved: int [U, T] / [T] like
    rank (`two_stage_ranks_host`: 1 retrieved, 0 eligible and not retrieved, -1 not in the catalogue or excluded, -2 padding);
    n_candidates: int [U] (or an int, one user).  In float64:
      'CandRecall'        per user the slots with retrieved == 1 over the slots with retrieved >= 0, then the mean over the
                          users with at least one such slot; NaN when no user has one
      'CandRecall_users'  the number of those users
      'candidates_mean'   the mean of n_candidates
    per_user=True adds 'CandRecall_user', float64 [U], NaN for a user without an eligible slot."""
    out = ranking_metrics(rank, ks, per_user)
    g = np.asarray(retrieved)
    if g.shape != np.asarray(rank).shape or not np.issubdtype(g.dtype, np.integer) or int(g.min()) < RETRIEVED_PAD or int(g.max()) > 1:
        raise _lib.RsxError("two_stage_metrics: retrieved must be integers in [%d, 1] of rank's shape %s, got %s %s"
                            % (RETRIEVED_PAD, np.asarray(rank).shape, g.dtype, g.shape))
    g = np.atleast_2d(g)
    nc = np.atleast_1d(np.asarray(n_candidates))
    if nc.shape != (g.shape[0],) or not np.issubdtype(nc.dtype, np.integer) or int(nc.min()) < 0:
        raise _lib.RsxError("two_stage_metrics: n_candidates must be %d non-negative integers, got %s %s" % (g.shape[0], nc.dtype, nc.shape))
    eligible, kept = np.count_nonzero(g >= 0, axis=1), np.count_nonzero(g == 1, axis=1)
    users = eligible > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.where(users, kept / eligible.astype(np.float64), np.nan)
    out["CandRecall"] = float(per[users].mean()) if users.any() else float("nan")
    out["CandRecall_users"] = int(users.sum())
    out["candidates_mean"] = float(nc.astype(np.float64).mean())
    if per_user:
        out["CandRecall_user"] = per
    return out


def narrow_neighbours_host(nbr_pos, nbr_count, m):
    """The first m neighbours of every row of a table built with n >= m: (nbr_pos[:, :m], minimum(nbr_count, m)).  The rows are
    ordered best first, so this is `item_neighbours_host(..., m)`'s table bit for bit.  RsxError unless m is an integer (no
    bool) in [1, n]."""
    pos, cnt = np.asarray(nbr_pos), np.asarray(nbr_count)
    if pos.ndim != 2 or cnt.shape != (pos.shape[0],):
        raise _lib.RsxError("narrow_neighbours_host: neighbour table %s / %s is not [N, n] with [N]" % (pos.shape, cnt.shape))
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= pos.shape[1]:
        raise _lib.RsxError("n_neighbours must be an integer in [1, %d] (the table built), not %r" % (pos.shape[1], m))
    return np.ascontiguousarray(pos[:, :int(m)]), np.minimum(cnt, int(m)).astype(cnt.dtype)


# ---- Predictor ---------------------------------------------------------------------------------------------------------------
class Predictor:
    """An exported model ready to answer requests.  See the module docstring for the two paths.  `table_dtype` is the
    bundle's ("float32" for a version 1 bundle): on the fused path the device holds the table in that dtype; on the layers
    path a 16-bit table is widened to fp32 on the host (the rounded values, no memory saved, `rank_candidates` unchanged)."""

    MAX_GRAPHS = 32            # request sizes that get a captured graph at most (Estimator.MAX_INFER_GRAPHS' twin)

    def __init__(self):
        raise TypeError("use Predictor.load(export_dir)")

    @classmethod
    def load(cls, export_dir, device="cuda", max_batch_size=4096, use_hip_graph=True, max_candidates=None, one_launch=False,
             device_parse=False, parse_row_bytes=2048):
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
        bytes; a Criteo request row is about 0.9 KB (39 entries, 8-byte categorical values), 2048 leaves room for two."""
        import torch
        self = object.__new__(cls)
        self.bundle_dir = latest_bundle(export_dir)
        self.manifest, arrays = read_bundle(self.bundle_dir)
        m = self.manifest
        self.script, self.global_step = m["script"], int(m["global_step"])
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
        self.rules_on_device = True         # False: a `recommend` with a category rule takes the host path
        self.evaluate_recommend_path = None # where the latest `evaluate_recommend` ranked
        self._cat = None
        self._nbr = None                    # `build_neighbours`' table (din.py bundles)
        self.neighbours_path = None         # where the latest `build_neighbours` built it
        self.two_stage_path = None          # where the latest `recommend_two_stage` ran
        self.evaluate_two_stage_path = None # where the latest `evaluate_two_stage` ranked
        if self.script == "din":
            self.rank_path = "fused" if self._rank_supported() else "layers"
            self.topk_path = "device" if self.rank_path == "fused" else "host"
        return self

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

    # -- candidate ranking (din.py) ---------------------------------------------------------------------------------------
    def _din_sizes(self):
        from . import din
        pr = self.manifest["params"]
        return (int(pr.get("hist_len", 100)), int(pr.get("n_item", din.N_ITEM)), int(pr.get("n_cate", din.N_CATE)),
                int(pr["embedding_size"]))

    def _rank_supported(self):
        from . import din
        P, _, _, K = self._din_sizes()
        wa = (C.c_int32 * _lib.PREDICT_MAX_LAYERS)(*din.MLP_LAYERS)
        n1, n2 = din.ATTENTION_LAYERS
        return bool(_lib.lib().rsx_predict_din_rank_supported(1, self.max_candidates, P, K, n1, n2, len(din.MLP_LAYERS), wa))

    def _rank_setup(self, U):
        """The model (pointers into the Estimator's store: nothing is copied) and the static request buffers for U users."""
        import torch
        from . import din
        P, _, _, K = self._din_sizes()
        st = self._est.store
        r = self._rank
        if r is None:
            item, cate, bias = (st.embeddings[k].table for k in ("i_id", "i_cate", "i_item"))
            pm = _lib.PredictDinModel()
            pm.item_emb, pm.cate_emb, pm.item_bias = item.data_ptr(), cate.data_ptr(), bias.data_ptr()
            pm.bias_ld = int(bias.stride(0))
            for a, pre in enumerate(("att_i", "att_c")):
                for l in range(3):
                    pm.att_W[a][l] = st.dense["%s.W%d" % (pre, l)].data_ptr()
                    pm.att_b[a][l] = st.dense["%s.b%d" % (pre, l)].data_ptr()
            for l, n in enumerate(din.MLP_LAYERS):
                pm.mlp_W[l], pm.mlp_b[l] = st.dense["mlp.W%d" % l].data_ptr(), st.dense["mlp.b%d" % l].data_ptr()
                pm.widths[l], pm.ld[l] = n, int(st.dense.storage["mlp.W%d" % l][1])
            pm.mlp_wout, pm.mlp_bout = st.dense["mlp.Wout"].data_ptr(), st.dense["mlp.bout"].data_ptr()
            pm.K, pm.n1, pm.n2, pm.L = K, din.ATTENTION_LAYERS[0], din.ATTENTION_LAYERS[1], len(din.MLP_LAYERS)
            r = self._rank = {"model": pm, "U": 0}
        if U > r["U"]:
            # request buffers of one chunk: the histories [U, P], the candidates and their probabilities [U, max_candidates]
            # (a request of fewer users or candidates uses leading parts of them; graphs captured over smaller buffers go)
            dev, i32 = self.device, torch.int32
            self._drop_graphs("rank", "rank_topk", "recommend", "eval_recommend", "two_stage", "eval_two_stage")
            r.pop("ts", None)
            r.pop("ets", None)
            r.pop("topk", None)
            r.pop("rec", None)
            r.pop("eval", None)
            r["hist"] = [torch.zeros(U * P, dtype=i32, device=dev) for _ in range(2)]
            r["cand"] = [torch.zeros(U * self.max_candidates, dtype=i32, device=dev) for _ in range(2)]
            r["prob"] = torch.zeros(U * self.max_candidates, dtype=torch.float32, device=dev)
            r["U"] = U
        return r

    def _drop_graphs(self, *kinds):
        """Forgets the captured graphs of these key kinds (their static buffers are about to be replaced)."""
        for k in [k for k in self._graphs if isinstance(k, tuple) and k[0] in kinds]:
            del self._graphs[k]
            self._n_graphs -= 1

    def rank_buffer_bytes(self, U=1, top_k=None):
        """Bytes of the static request buffers `rank_candidates` holds for U users; with top_k, those of a request that
        selects on the device included (out_val and out_idx [U, k], state [U, 2])."""
        P = self._din_sizes()[0]
        n = 4 * (2 * U * P + 3 * U * self.max_candidates)
        if top_k is not None and self._topk_on_device(check_top_k(top_k)):
            n += 4 * (2 * U * int(top_k) + 2 * U)
        return n

    # -- top-k of a ranking request, selected on the device (csrc/topk.hip) ---------------------------------------------------
    def _topk_on_device(self, k):
        return self.rank_path == "fused" and k <= TOPK_MAX_K and bool(_lib.lib().rsx_topk_rows_supported(1, k))

    def topk_path_for(self, top_k):
        """Where `rank_candidates(..., top_k=top_k)` selects on this Predictor: "device" or "host" (None for a bundle that
        ranks no candidates).  A pure function of the bundle and k; `topk_path` only records what the latest request took."""
        if self.script != "din":
            return None
        return "device" if self._topk_on_device(check_top_k(top_k)) else "host"

    def _topk_setup(self, U, k):
        """The static buffers of the selection beside the rank buffers: one flat buffer that holds out_val [U, k] and, behind
        it, out_idx [U, k] of the request at hand (so both come back in ONE copy), and state [U, 2].  Reallocated like the
        rank buffers: when a request needs more than they hold (the graphs captured over the smaller ones go)."""
        import torch
        r = self._rank
        t = r.get("topk")
        if t is None or r["U"] * k > t["pairs"]:
            self._drop_graphs("rank_topk")
            t = r["topk"] = {"pairs": r["U"] * k,
                             "buf": torch.zeros(2 * r["U"] * k, dtype=torch.float32, device=self.device),
                             "state": torch.zeros(2 * r["U"], dtype=torch.int32, device=self.device)}
        return t

    def _rank_topk_launch(self, U, n, k):
        """The rank launch of one chunk, then the selection over its probabilities: one launch, or -- when n + k is beyond
        rsx_topk_rows' envelope (n + k > 16 384) -- one per slice of the chunk, the chunk halved until a slice fits (the running
        list carries over; n = 16 000 with k = 1 024: two slices of 8 000, three launches for the chunk)."""
        import torch
        self._rank_launch(U, n)
        r = self._rank
        t, L = r["topk"], _lib.lib()
        step = n
        while not L.rsx_topk_rows_supported(step, k):
            step = (step + 1) // 2
        for s in range(0, n, step):
            _lib.check(L.rsx_topk_rows(r["prob"].data_ptr() + 4 * s, int(n), int(U), min(step, n - s), int(k), t["buf"].data_ptr(),
                                       t["buf"].data_ptr() + 4 * U * k, t["state"].data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "rsx_topk_rows")

    def _rank_topk_device(self, U, Cn, P, Pq, k, u_iid_seq, u_icat_seq, i_id, i_cate):
        """-> (prob [U, k'], index [U, k']): per chunk the rank launch and the selection in one graph, nothing fetched until
        the request's last chunk is in."""
        import torch
        kk = min(k, Cn)
        with torch.no_grad():
            r = self._rank_setup(U)
            t = self._topk_setup(U, k)
            self._rank_histories(r, U, P, Pq, u_iid_seq, u_icat_seq)
            t["state"].zero_()
            ci, cc = self._dev32(i_id, U), self._dev32(i_cate, U)
            for s in range(0, Cn, self.max_candidates):
                e = min(Cn, s + self.max_candidates)
                n = e - s
                r["cand"][0][:U * n].view(U, n).copy_(ci[:, s:e], non_blocking=True)
                r["cand"][1][:U * n].view(U, n).copy_(cc[:, s:e], non_blocking=True)
                self._run(("rank_topk", U, n, k), lambda: self._rank_topk_launch(U, n, k))
            h = t["buf"][:2 * U * k].cpu().numpy()                     # the ONE device-to-host copy of the request
        return (np.ascontiguousarray(h[:U * k].reshape(U, k)[:, :kk]),
                np.ascontiguousarray(h[U * k:].view(np.int32).reshape(U, k)[:, :kk]))

    def _rank_launch(self, U, n):
        import torch
        r, P = self._rank, self._din_sizes()[0]
        _lib.check(_lib.lib().rsx_predict_din_rank(C.byref(r["model"]), r["hist"][0].data_ptr(), r["hist"][1].data_ptr(),
                                                   r["cand"][0].data_ptr(), r["cand"][1].data_ptr(), r["prob"].data_ptr(),
                                                   int(U), int(n), P, torch.cuda.current_stream().cuda_stream),
                   "rsx_predict_din_rank")

    def _rank_chunk(self, U, ci, cc):
        """ci, cc: int32 [U, n] (host or device), n <= max_candidates; the histories are in place -> prob [U, n] (a view of
        the output buffer, valid until the next call).  Graphs: the rule of _fused_chunk, keyed by the request shape."""
        r = self._rank
        n = int(ci.shape[1])
        r["cand"][0][:U * n].view(U, n).copy_(ci, non_blocking=True)
        r["cand"][1][:U * n].view(U, n).copy_(cc, non_blocking=True)
        self._run(("rank", U, n), lambda: self._rank_launch(U, n))
        return r["prob"][:U * n].view(U, n)

    @staticmethod
    def _dev32(x, rows):
        import torch
        if isinstance(x, torch.Tensor):
            return x.reshape(rows, -1).to(torch.int32)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(rows, -1), np.int32))

    def _rank_histories(self, r, U, P, Pq, u_iid_seq, u_icat_seq):
        """The request's histories into the static buffers, zero padded to the bundle's hist_len."""
        for buf, x in zip(r["hist"], (u_iid_seq, u_icat_seq)):
            hv = buf[:U * P].view(U, P)
            if Pq:
                hv[:, :Pq].copy_(self._dev32(x, U), non_blocking=True)
            if Pq < P:
                hv[:, Pq:].zero_()

    def rank_candidates(self, u_iid_seq, u_icat_seq, i_id, i_cate, top_k=None):
        """din.py bundles: score C candidate items against ONE user's behaviour history -- histories [P'], candidates [C] ->
        {'prob': float32 numpy [C]} -- or U users with C candidates each: histories [U, P'], candidates [U, C] -> prob [U, C].
        P' <= the bundle's hist_len (shorter histories are zero padded).  numpy or torch, host or device, any integer dtype.
        top_k=k (an integer >= 1): only the k' = min(k, C) best candidates of every user -> {'prob': float32 [k'] / [U, k'],
        'index': int32, same shape: positions on the request's candidate axis}, in the order of `topk_rows_host` (higher
        probability first, equal ones by the lower position).  `topk_path_for(k)` says where a request with that k selects
        (ask it before the call; `topk_path` records where the LATEST such request did):
        "device" (rank_path == "fused" and k <= 1024): rsx_topk_rows behind every chunk's rank launch, in the chunk's graph,
        the running list on the device and ONE copy of k' pairs at the end of the request; "host": the probabilities as
        without top_k, then `topk_rows_host`.  Both give the same bits."""
        import torch
        if getattr(self, "script", None) != "din":
            raise _lib.RsxError("rank_candidates: only din.py bundles rank candidates against a history; this bundle is %s.py"
                                % getattr(self, "script", None))
        P, n_item, n_cate, _ = self._din_sizes()
        U, Cn, Pq, single = check_rank_request(u_iid_seq, u_icat_seq, i_id, i_cate, P, n_item, n_cate)
        if top_k is not None:
            k = check_top_k(top_k)
            if self._topk_on_device(k):
                self.topk_path = "device"
                prob, index = self._rank_topk_device(U, Cn, P, Pq, k, u_iid_seq, u_icat_seq, i_id, i_cate)
                out = {"prob": prob, "index": index}
            else:
                self.topk_path = "host"
                out = topk_rows_host(self.rank_candidates(u_iid_seq, u_icat_seq, i_id, i_cate)["prob"].reshape(U, Cn), k)
            return {key: v[0] for key, v in out.items()} if single else out
        shape = (Cn,) if single else (U, Cn)
        if self.rank_path != "fused":
            host = [x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
                    for x in (u_iid_seq, u_icat_seq, i_id, i_cate)]
            return {"prob": self.predict(expand_rank_request(*host, hist_len=P))["prob"].reshape(shape)}

        out = np.empty((U, Cn), np.float32)
        with torch.no_grad():
            r = self._rank_setup(U)
            self._rank_histories(r, U, P, Pq, u_iid_seq, u_icat_seq)
            ci, cc = self._dev32(i_id, U), self._dev32(i_cate, U)
            for s in range(0, Cn, self.max_candidates):
                e = min(Cn, s + self.max_candidates)
                out[:, s:e] = self._rank_chunk(U, ci[:, s:e], cc[:, s:e]).cpu().numpy()
        return {"prob": out.reshape(shape)}

    # -- recommendation over a resident catalogue (din.py; csrc/topk_excl.hip) -----------------------------------------------
    def _need_din(self, what):
        if getattr(self, "script", None) != "din":
            raise _lib.RsxError("%s: only din.py bundles rank a catalogue against a history; this bundle is %s.py"
                                % (what, getattr(self, "script", None)))

    def set_catalogue(self, i_id, i_cate):
        """din.py bundles: the servable items and their categories, two 1-D integer arrays of equal length N >= 1 (numpy or
        torch; `check_catalogue` refuses anything else and ids outside the tables).  Uploaded once as int32, a host copy is
        kept; `catalogue_size` reports N.  A second call replaces the catalogue and drops the graphs captured over the old one
        and `build_neighbours`' table, which names positions of the old catalogue."""
        import torch
        self._need_din("set_catalogue")
        _, n_item, n_cate, _ = self._din_sizes()
        ci, cc = check_catalogue(i_id, i_cate, n_item, n_cate)
        self._drop_graphs("recommend", "eval_recommend", "two_stage", "eval_two_stage")
        self._nbr, self.neighbours_path = None, None                   # the neighbour table names positions of the old catalogue
        self._cat = {"host": (ci, cc), "dev": [torch.from_numpy(x).to(self.device) for x in (ci, cc)],
                     "first": catalogue_first_positions(ci)}       # id -> its lowest position (evaluate_recommend)
        self.catalogue_size = int(ci.shape[0])

    def _recommend_on_device(self, k):
        return self.rank_path == "fused" and k <= TOPK_MAX_K and bool(_lib.lib().rsx_topk_rows_excl_supported(1, k, 0))

    def _rules_on_device(self, k, m):
        """A request with a category rule (m: the cap, None or 0 for none): today's conditions, the switch, m <= 16 and
        rsx_topk_rows_rules' envelope for this bundle's n_cate."""
        m = int(m or 0)
        return (self.rules_on_device and self._recommend_on_device(k) and m <= RULES_MAX_M
                and bool(_lib.lib().rsx_topk_rows_rules_supported(1, k, 0, self._din_sizes()[2], m)))

    def recommend_path_for(self, top_k, max_per_category=None, rules=False):
        """Where `recommend(..., top_k=top_k)` runs on this Predictor: "device" or "host" (None for a bundle that ranks no
        candidates).  A pure function of the bundle and k; a request that names more than 256 distinct positive ids for one
        user still takes the host path, and `recommend_path` records what the latest request took.  With max_per_category or
        rules=True (a request that names categories / exclude_categories) the answer is that of a request with a category
        rule: "device" needs `rules_on_device`, a cap of at most 16 and rsx_topk_rows_rules' envelope as well."""
        if self.script != "din":
            return None
        k, m = check_top_k(top_k), check_max_per_category(max_per_category)
        if m is not None or rules:
            return "device" if self._rules_on_device(k, m) else "host"
        return "device" if self._recommend_on_device(k) else "host"

    def recommend_buffer_bytes(self, U=1, top_k=100, rules=False):
        """Bytes of the static buffers a `recommend` request of U users holds: the rank buffers, the catalogue (two int32 [N]),
        and on the device path out_val / out_idx [U, k] with state [U, 2] behind them and the exclusion ids [U, 256]; with
        rules=True also the category bitmap [U, ceil(n_cate / 32)] that a request with a category rule holds."""
        n = self.rank_buffer_bytes(U) + 8 * int(self.catalogue_size or 0)
        if self._recommend_on_device(check_top_k(top_k)):
            n += 4 * (2 * U * int(top_k) + 2 * U) + 4 * U * EXCL_MAX
            if rules:
                n += 4 * U * ((self._din_sizes()[2] + 31) // 32)
        return n

    def _rec_setup(self, U, k, rules=False):
        """The static buffers of a device `recommend` beside the rank buffers: ONE flat buffer that holds out_val [U, k], behind
        it out_idx [U, k] and state [U, 2] of the request at hand (so the answer and `filled` come back in one copy), and the
        exclusion ids [U, 256].  Reallocated like the selection's buffers: when a request needs more than they hold.  The
        category bitmap [U, ceil(n_cate / 32)] joins them with the first request that names a category rule."""
        import torch
        r = self._rank
        t = r.get("rec")
        if t is None or r["U"] * k > t["pairs"]:
            self._drop_graphs("recommend")
            t = r["rec"] = {"pairs": r["U"] * k,
                            "buf": torch.zeros(2 * r["U"] * k + 2 * r["U"], dtype=torch.float32, device=self.device),
                            "excl": torch.zeros(r["U"] * EXCL_MAX, dtype=torch.int32, device=self.device)}
        if rules and "allow" not in t:
            t["allow"] = torch.zeros(r["U"] * ((self._din_sizes()[2] + 31) // 32), dtype=torch.int32, device=self.device)
        return t

    def _recommend_launch(self, U, k, E, rules=None):
        """The whole request, one chain: the state's zeroing, then for every chunk of max_candidates catalogue entries the
        shared rank launch and the filtered selection (sliced as `_rank_topk_launch` slices it beyond n + k = 16 384).  Every
        address is fixed -- the catalogue's slices included -- so `_run` captures it as ONE graph per (U, k, E).
        rules = (bitmap present, m) for a request with a category rule: rsx_topk_rows_rules in rsx_topk_rows_excl's place,
        sliced by its own envelope, with the resident categories from position 0 and the bitmap buffer (or no bitmap)."""
        import torch
        r, t, L = self._rank, self._rank["rec"], _lib.lib()
        cat_i, cat_c = (x.data_ptr() for x in self._cat["dev"])
        N, mc, P = self.catalogue_size, self.max_candidates, self._din_sizes()[0]
        val = t["buf"].data_ptr()
        idx, state = val + 4 * U * k, val + 8 * U * k
        t["buf"][2 * U * k:2 * U * k + 2 * U].zero_()
        stream = torch.cuda.current_stream().cuda_stream
        for s in range(0, N, mc):
            n = min(mc, N - s)
            _lib.check(L.rsx_predict_din_rank_shared(C.byref(r["model"]), r["hist"][0].data_ptr(), r["hist"][1].data_ptr(),
                                                     cat_i + 4 * s, cat_c + 4 * s, r["prob"].data_ptr(), int(U), int(n), P, stream),
                       "rsx_predict_din_rank_shared")
            step = n
            if rules is not None:
                bitmap, m = rules
                G = self._din_sizes()[2]
                while not L.rsx_topk_rows_rules_supported(step, k, E, G, m):
                    step = (step + 1) // 2
                for s2 in range(0, n, step):
                    _lib.check(L.rsx_topk_rows_rules(r["prob"].data_ptr() + 4 * s2, int(n), cat_i + 4 * (s + s2), t["excl"].data_ptr(),
                                                     int(E), cat_c, G, t["allow"].data_ptr() if bitmap else None, int(m), int(U),
                                                     min(step, n - s2), int(k), val, idx, state, stream), "rsx_topk_rows_rules")
                continue
            while not L.rsx_topk_rows_excl_supported(step, k, E):
                step = (step + 1) // 2
            for s2 in range(0, n, step):
                _lib.check(L.rsx_topk_rows_excl(r["prob"].data_ptr() + 4 * s2, int(n), cat_i + 4 * (s + s2), t["excl"].data_ptr(),
                                                int(E), int(U), min(step, n - s2), int(k), val, idx, state, stream),
                           "rsx_topk_rows_excl")

    def _recommend_device(self, U, k, P, Pq, u_iid_seq, u_icat_seq, ids, rules=None):
        """ids: int32 [U, E] host, E one of the exclusion capacities -> the answer of `recommend_host` for U users.
        rules: None, or (bitmap: uint32 [U, W] host or None, m: the cap or 0) of a request with a category rule; its graph is
        keyed by (U, k, E, bitmap present, m)."""
        import torch
        E = int(ids.shape[1])
        kk = min(k, self.catalogue_size)
        with torch.no_grad():
            r = self._rank_setup(U)
            t = self._rec_setup(U, k, rules is not None)
            self._rank_histories(r, U, P, Pq, u_iid_seq, u_icat_seq)
            if E:
                t["excl"][:U * E].view(U, E).copy_(torch.from_numpy(ids), non_blocking=True)
            if rules is None:
                self._run(("recommend", U, k, E), lambda: self._recommend_launch(U, k, E))
            else:
                bitmap, m = rules
                if bitmap is not None:
                    W = bitmap.shape[1]
                    t["allow"][:U * W].view(U, W).copy_(torch.from_numpy(bitmap.view(np.int32)), non_blocking=True)
                how = (bitmap is not None, int(m))
                self._run(("recommend", U, k, E) + how, lambda: self._recommend_launch(U, k, E, how))
            h = t["buf"][:2 * U * k + 2 * U].cpu().numpy()           # the ONE device-to-host copy: pairs and `filled`
        count = h[2 * U * k:].view(np.int32).reshape(U, 2)[:, 0].copy()
        prob = np.ascontiguousarray(h[:U * k].reshape(U, k)[:, :kk])
        index = np.ascontiguousarray(h[U * k:2 * U * k].view(np.int32).reshape(U, k)[:, :kk])
        pad = np.arange(kk)[None, :] >= count[:, None]               # entries past `filled` are unspecified on the device
        prob[pad], index[pad] = np.nan, 0
        item = self._cat["host"][0][index]
        item[pad], index[pad] = -1, -1
        return {"prob": prob, "item": item, "index": index, "count": count}

    @staticmethod
    def _excl_capacity(cols):
        """Columns of the exclusion buffer a request of `cols` ids per user uses (a graph is keyed by it)."""
        return 0 if cols == 0 else next(c for c in (32, 64, 128, EXCL_MAX) if cols <= c)

    @classmethod
    def _device_exclusion(cls, ids):
        """ids: int64 [U, E''] (`_exclusion_ids`) -> int32 [U, capacity], the list the device takes (padding and ids no int32
        catalogue can hold as 0), or None when a user names more than 256 distinct positive ids."""
        U = ids.shape[0]
        ids = np.where((ids > 0) & (ids < 2 ** 31), ids, 0)
        if ids.shape[1] > EXCL_MAX:                                  # more columns than the kernel takes: the distinct ids may fit
            rows = [np.unique(x[x > 0]) for x in ids]
            if max(len(x) for x in rows) > EXCL_MAX:
                return None
            ids = np.zeros((U, max(len(x) for x in rows)), np.int64)
            for u, x in enumerate(rows):
                ids[u, :len(x)] = x
        padded = np.zeros((U, cls._excl_capacity(ids.shape[1])), np.int32)
        padded[:, :ids.shape[1]] = ids
        return padded

    def recommend(self, u_iid_seq, u_icat_seq, top_k, exclude_seen=True, exclude=None, categories=None, exclude_categories=None,
                  max_per_category=None):
        """din.py bundles, after `set_catalogue`: the top_k best catalogue entries for ONE user's history ([P']) or for U users
        ([U, P']), every entry scored exactly as `rank_candidates` scores it, without the entries whose item id is a positive
        id of the user's history (exclude_seen) or of `exclude` ([E'] / [U, E']: blocked, already bought; ids <= 0 are padding).
        -> {'prob': float32 [U, kk], 'item': int32 [U, kk] (the catalogue's i_id), 'index': int32 [U, kk] (the catalogue
        position), 'count': int32 [U]}, kk = min(top_k, N), count[u] = min(top_k, eligible entries); entries at and beyond
        count[u] are NaN / -1 / -1.  One user: the arrays cut to count, count an int.  `recommend_host` is the definition.
        `recommend_path_for(k)` says where a request selects: "device" (rank_path == "fused", k <= 1024, at most 256 distinct
        positive exclusion ids per user): only the histories and the exclusion ids are shipped, the whole request -- per chunk
        rsx_predict_din_rank_shared over the resident catalogue and rsx_topk_rows_excl -- is ONE captured graph per
        (U, k, exclusion capacity), one copy brings the answer back; "host": `rank_candidates` over the catalogue, then
        `recommend_host`.  Both give the same bits.
        CATEGORY RULES (`recommend_host` defines them; a request without one is exactly the request above): categories /
        exclude_categories ([G'] / [U, G'] like `exclude`; negative ids padding, ids >= n_cate refused) keep only / drop the
        entries of those categories -- the category of an entry is what `set_catalogue` was given -- and max_per_category = m
        keeps at most m entries of one category in the list, so count[u] can stay below top_k.
        `recommend_path_for(k, m, rules=True)` says where such a request runs: "device" (the conditions above,
        `rules_on_device`, m <= 16 and rsx_topk_rows_rules' envelope): the lists are folded into a bitmap [U, ceil(n_cate / 32)]
        that is shipped with the exclusion ids, rsx_topk_rows_rules takes rsx_topk_rows_excl's place launch for launch, and
        the request is ONE captured graph per (U, k, exclusion capacity, bitmap present, m); "host": `rank_candidates` over the
        catalogue, then `recommend_host`.  Both give the same bits."""
        import torch
        self._need_din("recommend")
        if self._cat is None:
            raise _lib.RsxError("recommend: no catalogue set -- call set_catalogue(i_id, i_cate) first")
        k = check_top_k(top_k)
        P, n_item, n_cate, _ = self._din_sizes()
        shape = tuple(u_iid_seq.shape) if hasattr(u_iid_seq, "shape") else np.shape(u_iid_seq)
        one = np.zeros((shape[0], 1) if len(shape) == 2 else 1, np.int32)      # a stand-in candidate: the histories' checks
        U, _, Pq, single = check_rank_request(u_iid_seq, u_icat_seq, one, one, P, n_item, n_cate)
        ids = _exclusion_ids(u_iid_seq, exclude, U, exclude_seen)
        m = check_max_per_category(max_per_category)
        only = check_category_list(categories, "categories", U, single, n_cate)
        deny = check_category_list(exclude_categories, "exclude_categories", U, single, n_cate)
        rules = None
        if m is not None or only is not None or deny is not None:
            rules = (category_bitmap(only, deny, n_cate) if only is not None or deny is not None else None, m or 0)
            on_device = self._rules_on_device(k, m)
        else:
            on_device = self._recommend_on_device(k)
        padded = self._device_exclusion(ids) if on_device else None
        if padded is not None:
            self.recommend_path = "device"
            out = self._recommend_device(U, k, P, Pq, u_iid_seq, u_icat_seq, padded, rules)
        else:
            self.recommend_path = "host"
            ci, cc = self._cat["host"]
            cand = (ci, cc) if single else tuple(np.broadcast_to(x, (U, len(x))) for x in (ci, cc))
            prob = self.rank_candidates(u_iid_seq, u_icat_seq, *cand)["prob"]
            if rules is None:
                return recommend_host(prob, ci, u_iid_seq, exclude, k, exclude_seen)
            return recommend_host(prob, ci, u_iid_seq, exclude, k, exclude_seen, cat_cate=cc, categories=categories,
                                  exclude_categories=exclude_categories, max_per_category=m, n_cate=n_cate)
        return _one_user(out) if single else out

    # -- two-stage recommendation: item neighbours, candidates on the device (din.py; csrc/rows_dot.hip, retrieve.hip) ---------
    def _need_catalogue(self, what):
        self._need_din(what)
        if self._cat is None:
            raise _lib.RsxError("%s: no catalogue set -- call set_catalogue(i_id, i_cate) first" % what)

    def _need_neighbours(self, what):
        self._need_catalogue(what)
        if self._nbr is None:
            raise _lib.RsxError("%s: no neighbour table -- call build_neighbours() after set_catalogue" % what)
        return self._nbr

    def _neighbours_on_device(self, n):
        P, _, _, K = self._din_sizes()
        L = _lib.lib()
        return (self.rank_path == "fused" and bool(L.rsx_rows_dot_supported(K)) and bool(L.rsx_topk_rows_excl_supported(1, n, 1))
                and bool(L.rsx_din_retrieve_candidates_supported(self.catalogue_size, P, n, 0)))

    def _build_neighbours_device(self, unit, n):
        """The build chain: the state's zeroing, then per block of max_candidates query positions and per chunk of catalogue
        rows rsx_rows_dot and rsx_topk_rows_excl -- cand_id = the chunk's item ids, excl [Q, 1] = each query's own id, k = n --
        so the running list carries absolute catalogue positions.  -> (pos int32 [N, n], sim float32 [N, n], count int32 [N])
        on the device, padded like `item_neighbours_host`'s."""
        import torch
        L, dev = _lib.lib(), self.device
        N, K = unit.shape
        cat_i = self._cat["dev"][0]
        unit_d = torch.from_numpy(np.ascontiguousarray(unit)).to(dev)
        chunk = min(N, self.max_candidates)
        while not L.rsx_topk_rows_excl_supported(chunk, n, 1):
            chunk = (chunk + 1) // 2
        QB = min(N, self.max_candidates)
        scores = torch.empty(QB * chunk, dtype=torch.float32, device=dev)
        q_rows = torch.arange(N, dtype=torch.int32, device=dev)
        sim = torch.zeros(N * n, dtype=torch.float32, device=dev)
        pos = torch.zeros(N * n, dtype=torch.int32, device=dev)
        state = torch.zeros(2 * N, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        for q0 in range(0, N, QB):
            Q = min(QB, N - q0)
            for s in range(0, N, chunk):
                m = min(chunk, N - s)
                _lib.check(L.rsx_rows_dot(unit_d.data_ptr(), int(N), int(K), q_rows.data_ptr() + 4 * q0, int(Q), int(s), int(m),
                                          scores.data_ptr(), int(m), stream), "rsx_rows_dot")
                _lib.check(L.rsx_topk_rows_excl(scores.data_ptr(), int(m), cat_i.data_ptr() + 4 * s, cat_i.data_ptr() + 4 * q0, 1,
                                                int(Q), int(m), int(n), sim.data_ptr() + 4 * q0 * n, pos.data_ptr() + 4 * q0 * n,
                                                state.data_ptr() + 8 * q0, stream), "rsx_topk_rows_excl")
        count = torch.where(cat_i > 0, state.view(N, 2)[:, 0], torch.zeros_like(cat_i))
        pad = torch.arange(n, device=dev)[None, :] >= count[:, None]     # entries past `filled` are unspecified on the device
        pos, sim = pos.view(N, n), sim.view(N, n)
        pos[pad], sim[pad] = -1, float("nan")
        torch.cuda.synchronize()
        return pos, sim, count.contiguous()

    def build_neighbours(self, n_neighbours=32):
        """din.py bundles, after `set_catalogue`: builds and keeps, for every catalogue position, the n most similar OTHER
        catalogue entries by cosine similarity of the bundle's item embedding rows (`item_neighbours_host` is the definition:
        entries of the same item id are left out, a position with item id 0 gets an empty row).  1 <= n <= 64.
        The rows are normalised on the host (`unit_rows_host`, float64 norms) and uploaded once, N K 4 bytes, released when the
        build ends.  `neighbours_path` == "device" (rank_path == "fused" and the kernels' envelopes hold): per block of query
        positions and per chunk of the catalogue rsx_rows_dot and rsx_topk_rows_excl, the table never leaves the device;
        "host": `item_neighbours_host`.  Both give the same bits.  The table is N n 8 + N 4 bytes (`neighbours_buffer_bytes`
        adds the id -> first position index, n_item 4 bytes); `set_catalogue` drops it."""
        import torch
        self._need_catalogue("build_neighbours")
        n = check_n_neighbours(n_neighbours)
        P, n_item, _, K = self._din_sizes()
        ci, _ = self._cat["host"]
        emb = self._est.store.embeddings["i_id"].table.detach()[:, :K].float().cpu().numpy()
        unit = unit_rows_host(emb[ci])
        self._drop_graphs("two_stage", "eval_two_stage")
        self._nbr = None                                               # (with it go `evaluate_two_stage`'s narrowed copies)
        ids, first = self._cat["first"]
        first_pos = np.full(n_item, -1, np.int32)
        first_pos[ids] = first
        if self._neighbours_on_device(n):
            self.neighbours_path = "device"
            with torch.no_grad():
                pos, sim, count = self._build_neighbours_device(unit, n)
            host = (pos.cpu().numpy(), sim.cpu().numpy(), count.cpu().numpy())
        else:
            self.neighbours_path = "host"
            host = item_neighbours_host(unit, ci, n)
            pos = sim = count = None
            if self.rank_path == "fused":
                pos, sim, count = (torch.from_numpy(x).to(self.device) for x in host)
        self._nbr = {"n": n, "host": host, "first_host": first_pos}
        if pos is not None:
            self._nbr["dev"] = (pos, sim, count)
            self._nbr["first"] = torch.from_numpy(first_pos).to(self.device)

    def neighbours_buffer_bytes(self):
        """Device bytes of the neighbour table and the id -> first position index (0 before `build_neighbours`, or when the
        table lives on the host only), plus N m 4 + N 4 for every narrowed copy `evaluate_two_stage(n_neighbours=m)` keeps."""
        if self._nbr is None or "dev" not in self._nbr:
            return 0
        N, n = self.catalogue_size, self._nbr["n"]
        narrowed = sum(N * m * 4 + N * 4 for m, e in self._nbr.get("narrow", {}).items() if "dev" in e)
        return N * n * 8 + N * 4 + 4 * self._din_sizes()[1] + narrowed

    def similar_items(self, item_ids, top_k):
        """After `build_neighbours(n)`: for every id of item_ids ([Q] integers) the kk = min(top_k, n) best neighbours of the
        LOWEST catalogue position that holds it -- rows of the table -> {'item': int32 [Q, kk], 'index': int32 [Q, kk] (catalogue
        positions), 'sim': float32 [Q, kk] (cosine similarity), 'count': int32 [Q]}.  An id the catalogue does not hold (and
        item id 0) has count 0; entries at and beyond the count are -1 / -1 / NaN.  top_k > n is refused."""
        nb = self._need_neighbours("similar_items")
        k = check_top_k(top_k)
        if k > nb["n"]:
            raise _lib.RsxError("similar_items: top_k %d exceeds the %d neighbours the table keeps" % (k, nb["n"]))
        q = item_ids.detach().cpu().numpy() if hasattr(item_ids, "detach") else np.asarray(item_ids)
        if q.ndim != 1 or (q.size and not np.issubdtype(q.dtype, np.integer)):
            raise _lib.RsxError("similar_items: item_ids must be a 1-D array of integers, got %s %s" % (q.dtype, q.shape))
        pos, sim, count = nb["host"]
        ci = self._cat["host"][0]
        at = _target_positions(self._cat["first"], q.astype(np.int64)[None, :])[0]
        ok = at >= 0
        row = np.where(ok, at, 0)
        index = np.where(ok[:, None], pos[row, :k], -1).astype(np.int32)
        cnt = np.where(ok, np.minimum(count[row], k), 0).astype(np.int32)
        s = np.where(index >= 0, sim[row, :k], np.float32(np.nan)).astype(np.float32)
        item = np.where(index >= 0, ci[np.maximum(index, 0)], -1).astype(np.int32)
        return {"item": item, "index": index, "sim": s, "count": cnt}

    def _two_stage_cap(self, Pq):
        return candidate_capacity(self.catalogue_size, Pq, self._nbr["n"])

    def _retrieve_on_device(self, cap):
        nb = self._nbr
        return (nb is not None and "dev" in nb and self.rank_path == "fused" and cap <= self.max_candidates
                and bool(_lib.lib().rsx_din_retrieve_candidates_supported(self.catalogue_size, self._din_sizes()[0], nb["n"], 0)))

    def _two_stage_on_device(self, k, cap):
        return self._retrieve_on_device(cap) and k <= TOPK_MAX_K and bool(_lib.lib().rsx_topk_rows_supported(cap, k))

    def two_stage_path_for(self, top_k, hist_len=None):
        """Where `recommend_two_stage(..., top_k=top_k)` runs for histories of hist_len positions (default: the bundle's):
        "device" or "host" (None for a bundle that ranks no candidates).  "device" needs `build_neighbours`' table on the
        device, rank_path == "fused", k <= 1024 and a candidate capacity -- min(N, hist_len (n + 1)) rounded up to 64 -- of at
        most max_candidates.  A request that names more than 256 distinct positive exclusion ids for one user still takes the
        host path; `two_stage_path` records what the latest request took."""
        if self.script != "din":
            return None
        k = check_top_k(top_k)
        if self._nbr is None:
            return "host"
        return "device" if self._two_stage_on_device(k, self._two_stage_cap(self._din_sizes()[0] if hist_len is None else hist_len)) else "host"

    def _ts_setup(self, U, k):
        """The static buffers of a device two-stage request beside the rank buffers: cand_pos [U, max_candidates], n_cand [U],
        the exclusion ids [U, 256], and ONE flat buffer that holds out_val [U, k], behind it the catalogue positions [U, k] and
        state [U, 2] (so the answer and `filled` come back in one copy) and, last, out_idx [U, k], which stays on the device."""
        import torch
        r = self._rank
        t = r.get("ts")
        if t is None:
            self._drop_graphs("two_stage")
            i32 = torch.int32
            t = r["ts"] = {"pairs": 0, "buf": None,
                           "pos": torch.zeros(r["U"] * self.max_candidates, dtype=i32, device=self.device),
                           "n_cand": torch.zeros(r["U"], dtype=i32, device=self.device),
                           "excl": torch.zeros(r["U"] * EXCL_MAX, dtype=i32, device=self.device)}
        if k and (t["buf"] is None or r["U"] * k > t["pairs"]):
            self._drop_graphs("two_stage")
            t["pairs"] = r["U"] * k
            t["buf"] = torch.zeros(3 * r["U"] * k + 2 * r["U"], dtype=torch.float32, device=self.device)
        return t

    def _two_stage_launch(self, U, k, E, cap, seeds):
        """The whole request, one chain: the state's zeroing, rsx_din_retrieve_candidates (the candidates' ids straight into
        the rank launch's candidate buffers), rsx_predict_din_rank over [U, cap], rsx_topk_rows_counted, and the gather that
        turns the selected columns into catalogue positions.  Every address is fixed, so `_run` captures it as ONE graph per
        (U, k, E, cap, seeds).  k = 0: the retrieval alone (`retrieve_candidates`)."""
        import torch
        r, t, nb, L = self._rank, self._rank["ts"], self._nbr, _lib.lib()
        cat_i, cat_c = (x.data_ptr() for x in self._cat["dev"])
        P, n_item = self._din_sizes()[:2]
        pos, _, count = nb["dev"]
        stream = torch.cuda.current_stream().cuda_stream
        if k:
            t["buf"][2 * U * k:2 * U * k + 2 * U].zero_()
        _lib.check(L.rsx_din_retrieve_candidates(r["hist"][0].data_ptr(), P, nb["first"].data_ptr(), n_item, pos.data_ptr(),
                                                 count.data_ptr(), nb["n"], cat_i, cat_c, self.catalogue_size,
                                                 t["excl"].data_ptr(), int(E), int(seeds), t["pos"].data_ptr(),
                                                 r["cand"][0].data_ptr(), r["cand"][1].data_ptr(), t["n_cand"].data_ptr(),
                                                 int(cap), int(U), stream), "rsx_din_retrieve_candidates")
        if not k:
            return
        self._rank_launch(U, cap)
        val = t["buf"].data_ptr()
        state, idx = val + 8 * U * k, val + 8 * U * k + 8 * U
        _lib.check(L.rsx_topk_rows_counted(r["prob"].data_ptr(), int(cap), t["n_cand"].data_ptr(), int(U), int(cap), int(k), val,
                                           idx, state, stream), "rsx_topk_rows_counted")
        ints = t["buf"].view(torch.int32)
        col = ints[2 * U * k + 2 * U:3 * U * k + 2 * U].view(U, k).clamp(0, cap - 1).long()     # (past `filled`: unspecified)
        torch.gather(t["pos"][:U * cap].view(U, cap), 1, col, out=ints[U * k:2 * U * k].view(U, k))

    def _two_stage_device(self, U, k, P, Pq, cap, u_iid_seq, u_icat_seq, ids, seeds):
        """ids: int32 [U, E] host, E one of the exclusion capacities.  k = 0 -> (cand_pos [U, cap], n_cand [U]); otherwise the
        answer of `recommend_two_stage_host` for U users."""
        import torch
        E = int(ids.shape[1])
        with torch.no_grad():
            r = self._rank_setup(U)
            t = self._ts_setup(U, k)
            self._rank_histories(r, U, P, Pq, u_iid_seq, u_icat_seq)
            if E:
                t["excl"][:U * E].view(U, E).copy_(torch.from_numpy(ids), non_blocking=True)
            self._run(("two_stage", U, k, E, cap, bool(seeds)), lambda: self._two_stage_launch(U, k, E, cap, seeds))
            if not k:
                return t["pos"][:U * cap].view(U, cap).cpu().numpy(), t["n_cand"][:U].cpu().numpy()
            h = t["buf"][:2 * U * k + 2 * U].cpu().numpy()           # the ONE device-to-host copy: pairs and `filled`
        kk = min(k, self.catalogue_size)
        count = h[2 * U * k:].view(np.int32).reshape(U, 2)[:, 0].copy()
        prob = np.ascontiguousarray(h[:U * k].reshape(U, k)[:, :kk])
        index = np.ascontiguousarray(h[U * k:2 * U * k].view(np.int32).reshape(U, k)[:, :kk])
        pad = np.arange(kk)[None, :] >= count[:, None]
        prob[pad], index[pad] = np.nan, 0
        item = self._cat["host"][0][np.maximum(index, 0)]
        item[pad], index[pad] = -1, -1
        return {"prob": prob, "item": item, "index": index, "count": count}

    def _two_stage_request(self, what, u_iid_seq, u_icat_seq, exclude_seen, exclude):
        self._need_neighbours(what)
        P, n_item, n_cate, _ = self._din_sizes()
        shape = tuple(u_iid_seq.shape) if hasattr(u_iid_seq, "shape") else np.shape(u_iid_seq)
        one = np.zeros((shape[0], 1) if len(shape) == 2 else 1, np.int32)      # a stand-in candidate: the histories' checks
        U, _, Pq, single = check_rank_request(u_iid_seq, u_icat_seq, one, one, P, n_item, n_cate)
        ids = _exclusion_ids(u_iid_seq, exclude, U, exclude_seen)
        return U, P, Pq, single, ids, self._two_stage_cap(Pq)

    def retrieve_candidates(self, u_iid_seq, u_icat_seq, exclude_seen=True, exclude=None):
        """After `build_neighbours`: the catalogue positions stage two of `recommend_two_stage` would score for these histories
        ([P'] or [U, P']) -- `retrieve_candidates_host` is the definition -> {'index': int32 [U, cap], ascending, -1 beyond the
        count; 'count': int32 [U]}, cap = min(N, P' (n + 1)) rounded up to 64.  One user: index cut to count, count an int.
        With held-out items this measures the candidate recall of the retrieval stage."""
        U, P, Pq, single, ids, cap = self._two_stage_request("retrieve_candidates", u_iid_seq, u_icat_seq, exclude_seen, exclude)
        padded = self._device_exclusion(ids) if self._retrieve_on_device(cap) else None
        if padded is not None:
            index, count = self._two_stage_device(U, 0, P, Pq, cap, u_iid_seq, u_icat_seq, padded, not exclude_seen)
        else:
            pos, _, cnt = self._nbr["host"]
            rows = retrieve_candidates_host(pos, cnt, self._cat["host"][0], u_iid_seq, exclude, exclude_seen)
            index = np.full((U, cap), -1, np.int32)
            count = np.zeros(U, np.int32)
            for u, x in enumerate(rows):
                index[u, :len(x)], count[u] = x, len(x)
        if single:
            return {"index": index[0, :int(count[0])], "count": int(count[0])}
        return {"index": index, "count": count}

    def recommend_two_stage(self, u_iid_seq, u_icat_seq, top_k, exclude_seen=True, exclude=None):
        """din.py bundles, after `set_catalogue` and `build_neighbours`: `recommend` over a RETRIEVED candidate set instead of
        the whole catalogue.  Stage one takes the neighbour rows of the history's items (`retrieve_candidates`), stage two scores
        those candidates exactly as `rank_candidates` scores them and returns the top_k best -- `recommend`'s result dictionary
        and one-user / U-user forms; `recommend_two_stage_host` is the definition.  count[u] = min(top_k, candidates of u): it
        can stay below top_k and can be 0 (an empty history, a history the catalogue does not hold).  There is NO back-fill
        from the rest of the catalogue, and the list differs from `recommend`'s by design: an entry outside the candidate set
        is never returned, however well it would score.  Category rules are not offered here.
        `two_stage_path_for(k)` says where a request runs: "device": only the histories and the exclusion ids are shipped and
        the whole request -- rsx_din_retrieve_candidates, rsx_predict_din_rank over [U, cap], rsx_topk_rows_counted, the
        gather of the catalogue positions -- is ONE captured graph per (U, k, exclusion capacity, cap), one copy brings the
        answer back; "host": `retrieve_candidates_host`, `rank_candidates` on the padded lists, `topk_rows_host` over each
        list's valid part.  Both give the same bits."""
        k = check_top_k(top_k)
        U, P, Pq, single, ids, cap = self._two_stage_request("recommend_two_stage", u_iid_seq, u_icat_seq, exclude_seen, exclude)
        padded = self._device_exclusion(ids) if self._two_stage_on_device(k, cap) else None
        if padded is not None:
            self.two_stage_path = "device"
            out = self._two_stage_device(U, k, P, Pq, cap, u_iid_seq, u_icat_seq, padded, not exclude_seen)
        else:
            self.two_stage_path = "host"
            pos, _, cnt = self._nbr["host"]
            ci, cc = self._cat["host"]
            N = self.catalogue_size
            rows = retrieve_candidates_host(pos, cnt, ci, u_iid_seq, exclude, exclude_seen)
            width = max(1, max(len(x) for x in rows))
            li, lc = np.zeros((U, width), np.int32), np.zeros((U, width), np.int32)     # padded with (item 0, category 0)
            for u, x in enumerate(rows):
                li[u, :len(x)], lc[u, :len(x)] = ci[x], cc[x]
            hi = u_iid_seq.reshape(U, -1) if hasattr(u_iid_seq, "reshape") else np.asarray(u_iid_seq).reshape(U, -1)
            hc = u_icat_seq.reshape(U, -1) if hasattr(u_icat_seq, "reshape") else np.asarray(u_icat_seq).reshape(U, -1)
            prob = self.rank_candidates(hi, hc, li, lc)["prob"].reshape(U, width)
            kk = min(k, N)
            out = {"prob": np.full((U, kk), np.nan, np.float32), "item": np.full((U, kk), -1, np.int32),
                   "index": np.full((U, kk), -1, np.int32), "count": np.zeros(U, np.int32)}
            for u, x in enumerate(rows):
                if len(x):
                    best = topk_rows_host(prob[u, :len(x)], kk)
                    c = len(best["index"])
                    at = x[best["index"]]
                    out["prob"][u, :c], out["item"][u, :c], out["index"][u, :c], out["count"][u] = best["prob"], ci[at], at, c
        return _one_user(out) if single else out

    # -- offline ranking metrics over the resident catalogue (din.py; csrc/rank_count.hip) -----------------------------------
    def _evaluate_on_device(self, T):
        return self.rank_path == "fused" and T <= RANK_MAX_T and bool(_lib.lib().rsx_rank_count_rows_supported(1, T, 0))

    def evaluate_recommend_path_for(self, T):
        """Where `evaluate_recommend` ranks T held-out items per user on this Predictor: "device" or "host" (None for a bundle
        that ranks no candidates).  A pure function of the bundle and T; a request that names more than 256 distinct positive
        exclusion ids for one user still takes the host path, and `evaluate_recommend_path` records what the latest took."""
        if self.script != "din":
            return None
        if isinstance(T, (bool, np.bool_)) or not isinstance(T, (int, np.integer)) or int(T) < 1:
            raise _lib.RsxError("evaluate_recommend: T must be an integer >= 1, not %r" % (T,))
        return "device" if self._evaluate_on_device(int(T)) else "host"

    @staticmethod
    def _target_capacity(T):
        """Columns of the target buffers a request of T held-out items per user uses (a graph is keyed by it; the capacities
        are the forms rsx_rank_count_rows is compiled in)."""
        return next(c for c in (1, 8, RANK_MAX_T) if T <= c)

    def _eval_setup(self):
        """The static buffers of a device `evaluate_recommend` beside the rank buffers, for the users the rank buffers hold and
        32 targets each: ONE flat buffer with count [U, T] and, behind it, tgt_score [U, T] of the block at hand (so both come
        back in one copy); one with the targets' item ids, categories and positions, three [U, T] (one copy up); the exclusion
        ids [U, 256]."""
        import torch
        r = self._rank
        t = r.get("eval")
        if t is None:
            n = r["U"] * RANK_MAX_T
            t = r["eval"] = {"buf": torch.zeros(2 * n, dtype=torch.float32, device=self.device),
                             "tgt": torch.zeros(3 * n, dtype=torch.int32, device=self.device),
                             "excl": torch.zeros(r["U"] * EXCL_MAX, dtype=torch.int32, device=self.device)}
        return t

    def _eval_launch(self, U, T, E):
        """One block of users, one chain: count's zeroing, the targets' own scores (one rsx_predict_din_rank launch over
        [U, T] pairs), then for every chunk of max_candidates catalogue entries the shared rank launch and the count of the
        entries that precede each target.  Every address is fixed, so `_run` captures it as ONE graph per (U, T, E)."""
        import torch
        r, t, L = self._rank, self._rank["eval"], _lib.lib()
        cat_i, cat_c = (x.data_ptr() for x in self._cat["dev"])
        N, mc, P = self.catalogue_size, self.max_candidates, self._din_sizes()[0]
        count = t["buf"].data_ptr()
        score = count + 4 * U * T
        item = t["tgt"].data_ptr()
        cate, pos = item + 4 * U * T, item + 8 * U * T
        hist_i, hist_c = r["hist"][0].data_ptr(), r["hist"][1].data_ptr()
        t["buf"][:U * T].zero_()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(L.rsx_predict_din_rank(C.byref(r["model"]), hist_i, hist_c, item, cate, score, int(U), int(T), P, stream),
                   "rsx_predict_din_rank")
        for s in range(0, N, mc):
            n = min(mc, N - s)
            _lib.check(L.rsx_predict_din_rank_shared(C.byref(r["model"]), hist_i, hist_c, cat_i + 4 * s, cat_c + 4 * s,
                                                     r["prob"].data_ptr(), int(U), int(n), P, stream), "rsx_predict_din_rank_shared")
            _lib.check(L.rsx_rank_count_rows(r["prob"].data_ptr(), int(n), cat_i + 4 * s, int(s), t["excl"].data_ptr(), int(E),
                                             score, pos, int(T), count, int(U), int(n), stream), "rsx_rank_count_rows")

    def _eval_device_block(self, hi, hc, P, Pq, excl, tgt):
        """hi, hc: int32 [U, P'] tensors; excl: int32 [U, E] host; tgt: int32 [3, U, T] host (item, category, position; T a
        target capacity) -> (count int32 [U, T], tgt_score float32 [U, T]) of one block of users."""
        import torch
        _, U, T = tgt.shape
        E = int(excl.shape[1])
        with torch.no_grad():
            r = self._rank
            t = self._eval_setup()
            self._rank_histories(r, U, P, Pq, hi, hc)
            if E:
                t["excl"][:U * E].view(U, E).copy_(torch.from_numpy(excl), non_blocking=True)
            t["tgt"][:3 * U * T].copy_(torch.from_numpy(tgt.reshape(-1)), non_blocking=True)
            self._run(("eval_recommend", U, T, E), lambda: self._eval_launch(U, T, E))
            h = t["buf"][:2 * U * T].cpu().numpy()                   # the ONE device-to-host copy of the block
        return h[:U * T].view(np.int32).reshape(U, T).copy(), h[U * T:].reshape(U, T).copy()

    def evaluate_recommend(self, u_iid_seq, u_icat_seq, held_out, ks=(10, 50, 100), exclude_seen=True, exclude=None,
                           user_block=16, per_user=False):
        """din.py bundles, after `set_catalogue`: where do each user's held-out items land in the list `recommend` would return
        over the WHOLE catalogue?  Histories [P'] / [U, P'] and `exclude` as in `recommend`; held_out: integer item ids [T] /
        [U, T], ids <= 0 are padding, no positive id twice for a user.  `target_ranks_host` is the definition of the ranks,
        `ranking_metrics` of the metrics -> ranking_metrics(rank, ks, per_user) plus 'rank' (int32 [U, T] / [T]: 0-based,
        RANK_MISSING = -1 for an id that is not in the catalogue or is itself excluded, RANK_PAD = -2 for padding) and
        'target_prob' (float32, same shape: the target entry's probability, NaN where the rank is negative).
        `evaluate_recommend_path_for(T)` says where a request ranks.  "device" (rank_path == "fused", T <= 32, at most 256
        distinct positive exclusion ids per user): the host resolves every held-out id to its catalogue position and
        eligibility and ships the histories, the exclusion ids and the targets; per block of at most `user_block` users ONE
        captured graph per (users, target capacity, exclusion capacity) zeroes the counts, scores the targets
        (rsx_predict_din_rank) and runs rsx_predict_din_rank_shared and rsx_rank_count_rows over every catalogue chunk; ONE
        copy of 8 bytes per (user, slot) comes back.  "host": `rank_candidates` over the catalogue per block of users, then
        `target_ranks_host`.  Both give the same integers and the same probability bits, whatever user_block and
        max_candidates are."""
        import torch
        self._need_din("evaluate_recommend")
        if self._cat is None:
            raise _lib.RsxError("evaluate_recommend: no catalogue set -- call set_catalogue(i_id, i_cate) first")
        ks = check_ks(ks)
        if isinstance(user_block, (bool, np.bool_)) or not isinstance(user_block, (int, np.integer)) or int(user_block) < 1:
            raise _lib.RsxError("evaluate_recommend: user_block must be an integer >= 1, not %r" % (user_block,))
        user_block = int(user_block)
        P, n_item, n_cate, _ = self._din_sizes()
        shape = tuple(u_iid_seq.shape) if hasattr(u_iid_seq, "shape") else np.shape(u_iid_seq)
        one = np.zeros((shape[0], 1) if len(shape) == 2 else 1, np.int32)      # a stand-in candidate: the histories' checks
        U, _, Pq, single = check_rank_request(u_iid_seq, u_icat_seq, one, one, P, n_item, n_cate)
        held = check_held_out(held_out, U, single, "evaluate_recommend")
        T = held.shape[1]
        ids = _exclusion_ids(u_iid_seq, exclude, U, exclude_seen)
        ci, cc = self._cat["host"]
        N = self.catalogue_size
        hi, hc = (self._dev32(x, U) if Pq else torch.zeros((U, 0), dtype=torch.int32) for x in (u_iid_seq, u_icat_seq))
        rank = np.empty((U, T), np.int32)
        tprob = np.full((U, T), np.nan, np.float32)
        excl = self._device_exclusion(ids) if self._evaluate_on_device(T) else None
        if excl is not None:
            self.evaluate_recommend_path = "device"
            pos = _target_positions(self._cat["first"], held)
            for u in range(U):                                       # a target whose entry is excluded has no rank
                x = ids[u][ids[u] > 0]
                if len(x):
                    pos[u][(pos[u] >= 0) & np.isin(held[u], x)] = RANK_MISSING
            ok = pos >= 0
            Tc = self._target_capacity(T)
            tgt = np.zeros((3, U, Tc), np.int32)                    # slots without a target: id 0, an ordinary row
            tgt[2] = -1
            at = np.where(ok, pos, 0)
            tgt[0, :, :T], tgt[1, :, :T], tgt[2, :, :T] = np.where(ok, ci[at], 0), np.where(ok, cc[at], 0), np.where(ok, pos, -1)
            self._rank_setup(min(U, user_block))
            for b in range(0, U, user_block):
                e = min(U, b + user_block)
                count, score = self._eval_device_block(hi[b:e], hc[b:e], P, Pq, excl[b:e], np.ascontiguousarray(tgt[:, b:e]))
                rank[b:e] = np.where(ok[b:e], count[:, :T], pos[b:e])
                tprob[b:e][ok[b:e]] = score[:, :T][ok[b:e]]
        else:
            self.evaluate_recommend_path = "host"
            hist_np = hi.cpu().numpy()
            for b in range(0, U, user_block):
                e = min(U, b + user_block)
                cand = tuple(np.tile(x, (e - b, 1)) for x in (ci, cc))
                prob = self.rank_candidates(hi[b:e], hc[b:e], *cand)["prob"]
                rank[b:e] = target_ranks_host(prob, ci, hist_np[b:e], held[b:e], ids[b:e], False)      # (ids: history included)
                pos = _target_positions(self._cat["first"], held[b:e])
                ok = rank[b:e] >= 0
                tprob[b:e][ok] = np.take_along_axis(prob, np.where(ok, pos, 0), 1)[ok]
        out = ranking_metrics(rank, ks, per_user)
        out["rank"], out["target_prob"] = (rank[0], tprob[0]) if single else (rank, tprob)
        return out

    # -- offline evaluation of the two-stage list (din.py; csrc/rank_count_lists.hip) ----------------------------------------
    def _eval_neighbours(self, n_neighbours):
        """`evaluate_two_stage`'s n_neighbours -> m: None is the built n; RsxError unless an integer (no bool) in [1, built n]."""
        n = self._nbr["n"]
        m = n if n_neighbours is None else n_neighbours
        if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= n:
            raise _lib.RsxError("evaluate_two_stage: n_neighbours must be None or an integer in [1, %d] (the table built), not %r"
                                % (n, n_neighbours))
        return int(m)

    def _narrowed_neighbours(self, m):
        """The table of the first m neighbours: `build_neighbours`' own for m == the built n, otherwise a contiguous copy kept
        per m inside the table's record -- host (`narrow_neighbours_host`) and, when the table is on the device, pos[:, :m] and
        count.clamp(max=m) there.  Whatever replaces the table (`set_catalogue`, `build_neighbours`) drops the copies with it."""
        nb = self._nbr
        if m == nb["n"]:
            return nb
        kept = nb.setdefault("narrow", {})
        if m not in kept:                                            # (pos, sim, count) like the table's own; sim is not kept
            pos, _, cnt = nb["host"]
            hp, hc = narrow_neighbours_host(pos, cnt, m)
            e = kept[m] = {"n": m, "host": (hp, None, hc)}
            if "dev" in nb:
                e["dev"] = (nb["dev"][0][:, :m].contiguous(), None, nb["dev"][2].clamp(max=m).contiguous())
        return kept[m]

    def _evaluate_two_stage_on_device(self, T, cap):
        return self._retrieve_on_device(cap) and T <= RANK_MAX_T and bool(_lib.lib().rsx_rank_count_lists_supported(cap, T))

    def evaluate_two_stage_path_for(self, T, hist_len=None, n_neighbours=None):
        """Where `evaluate_two_stage` ranks T held-out items per user for histories of hist_len positions (default: the
        bundle's) over the first n_neighbours of the table (default: all): "device" or "host" (None for a bundle that ranks no
        candidates).  "device" needs `build_neighbours`' table on the device, rank_path == "fused", T <= 32 and a candidate
        capacity of at most max_candidates.  A request that names more than 256 distinct positive exclusion ids for one user
        still takes the host path; `evaluate_two_stage_path` records what the latest request took."""
        if self.script != "din":
            return None
        if isinstance(T, (bool, np.bool_)) or not isinstance(T, (int, np.integer)) or int(T) < 1:
            raise _lib.RsxError("evaluate_two_stage: T must be an integer >= 1, not %r" % (T,))
        if self._nbr is None:
            return "host"
        m = self._eval_neighbours(n_neighbours)
        cap = candidate_capacity(self.catalogue_size, self._din_sizes()[0] if hist_len is None else hist_len, m)
        return "device" if self._evaluate_two_stage_on_device(int(T), cap) else "host"

    def _ets_setup(self):
        """The static buffers of a device `evaluate_two_stage` beside the rank buffers and the two-stage ones (cand_pos and the
        exclusion ids are `_ts_setup`'s), for the users the rank buffers hold and 32 targets each: the eligible targets' item
        ids [U, T], and ONE flat buffer with count, position and score, three [U, T], and behind them n_cand [U] of the block
        at hand -- so everything comes back in one copy."""
        import torch
        r = self._rank
        self._ts_setup(r["U"], 0)
        t = r.get("ets")
        if t is None:
            n = r["U"] * RANK_MAX_T
            t = r["ets"] = {"tgt": torch.zeros(n, dtype=torch.int32, device=self.device),
                            "out": torch.zeros(3 * n + r["U"], dtype=torch.float32, device=self.device)}
        return t

    def _eval_two_stage_launch(self, U, T, E, cap, seeds, nb):
        """One block of users, one chain: rsx_din_retrieve_candidates (the candidates' ids straight into the rank launch's
        candidate buffers, as in `_two_stage_launch`; n_cand into the answer's buffer), rsx_predict_din_rank over [U, cap],
        rsx_rank_count_lists.  The last writes every output slot, so nothing is zeroed.  Every address is fixed, so `_run`
        captures it as ONE graph per (U, T, E, cap, seeds, m)."""
        import torch
        r, ts, t, L = self._rank, self._rank["ts"], self._rank["ets"], _lib.lib()
        cat_i, cat_c = (x.data_ptr() for x in self._cat["dev"])
        P, n_item = self._din_sizes()[:2]
        pos, _, count = nb["dev"]
        out = t["out"].data_ptr()
        n_cand = out + 12 * U * T
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(L.rsx_din_retrieve_candidates(r["hist"][0].data_ptr(), P, self._nbr["first"].data_ptr(), n_item, pos.data_ptr(),
                                                 count.data_ptr(), nb["n"], cat_i, cat_c, self.catalogue_size,
                                                 ts["excl"].data_ptr(), int(E), int(seeds), ts["pos"].data_ptr(),
                                                 r["cand"][0].data_ptr(), r["cand"][1].data_ptr(), n_cand,
                                                 int(cap), int(U), stream), "rsx_din_retrieve_candidates")
        self._rank_launch(U, cap)
        _lib.check(L.rsx_rank_count_lists(r["prob"].data_ptr(), int(cap), r["cand"][0].data_ptr(), ts["pos"].data_ptr(), n_cand,
                                          t["tgt"].data_ptr(), int(T), out, out + 4 * U * T, out + 8 * U * T, int(U), int(cap),
                                          stream), "rsx_rank_count_lists")

    def _eval_two_stage_block(self, hi, hc, P, Pq, excl, tgt, cap, seeds, nb):
        """hi, hc: int32 [U, P'] tensors; excl: int32 [U, E] host; tgt: int32 [U, T] host (T a target capacity; 0 where the slot
        has no eligible target) -> (count int32 [U, T], position int32 [U, T], score float32 [U, T], n_cand int32 [U])."""
        import torch
        U, T = tgt.shape
        E = int(excl.shape[1])
        with torch.no_grad():
            r = self._rank
            t = self._ets_setup()
            self._rank_histories(r, U, P, Pq, hi, hc)
            if E:
                r["ts"]["excl"][:U * E].view(U, E).copy_(torch.from_numpy(excl), non_blocking=True)
            t["tgt"][:U * T].copy_(torch.from_numpy(tgt.reshape(-1)), non_blocking=True)
            self._run(("eval_two_stage", U, T, E, cap, bool(seeds), nb["n"]),
                      lambda: self._eval_two_stage_launch(U, T, E, cap, seeds, nb))
            h = t["out"][:3 * U * T + U].cpu().numpy()               # the ONE device-to-host copy of the block
        ints = h.view(np.int32)
        return (ints[:U * T].reshape(U, T).copy(), ints[U * T:2 * U * T].reshape(U, T).copy(),
                h[2 * U * T:3 * U * T].reshape(U, T).copy(), ints[3 * U * T:].copy())

    def evaluate_two_stage(self, u_iid_seq, u_icat_seq, held_out, ks=(10, 50, 100), exclude_seen=True, exclude=None,
                           user_block=16, per_user=False, n_neighbours=None):
        """din.py bundles, after `set_catalogue` and `build_neighbours`: did the retrieval stage keep each user's held-out
        items, and where do the kept ones land in the list `recommend_two_stage` would return?  Histories, `exclude` and
        held_out as in `evaluate_recommend`; `two_stage_ranks_host` is the definition of the ranks, `two_stage_metrics` of the
        metrics -> two_stage_metrics(rank, retrieved, n_candidates, ks, per_user) plus 'rank' (int32 [U, T] / [T]: 0-based among
        the user's candidates, RANK_MISSING = -1 for an id that was not retrieved, is not in the catalogue or is excluded,
        RANK_PAD = -2 for padding), 'retrieved' (int8: 1 retrieved, 0 eligible and not retrieved, -1 not in the catalogue or
        excluded, -2 padding), 'target_index' (int32: the catalogue position of the lowest CANDIDATE entry that holds the id,
        -1 where retrieved != 1), 'target_prob' (float32, NaN there) and 'n_candidates' (int32 [U]; an int for one user).
        n_neighbours = m (an integer in [1, the built n]; None: the built n) evaluates the first m neighbours of every row --
        `build_neighbours(m)`'s table, from the one already built -- with cap = candidate_capacity(N, P', m).
        `evaluate_two_stage_path_for(T, hist_len, m)` says where a request ranks.  "device" (the table on the device,
        rank_path == "fused", cap <= max_candidates, T <= 32, at most 256 distinct positive exclusion ids per user): the host
        classifies every slot (padding, missing / excluded, eligible) and ships the histories, the exclusion ids and the
        eligible ids; per block of at most `user_block` users ONE captured graph per (users, target capacity, exclusion
        capacity, cap, seeds, m) runs rsx_din_retrieve_candidates, rsx_predict_din_rank over [U, cap] and
        rsx_rank_count_lists, and ONE copy of 12 bytes per (user, slot) plus n_cand comes back; a narrowed contiguous copy of
        the device table is kept per m < n (`neighbours_buffer_bytes` counts it).  "host": `retrieve_candidates_host` on the
        narrowed table, `rank_candidates` on the padded lists, then numpy.  Both give the same integers and probability bits."""
        import torch
        self._need_neighbours("evaluate_two_stage")
        ks = check_ks(ks)
        if isinstance(user_block, (bool, np.bool_)) or not isinstance(user_block, (int, np.integer)) or int(user_block) < 1:
            raise _lib.RsxError("evaluate_two_stage: user_block must be an integer >= 1, not %r" % (user_block,))
        user_block = int(user_block)
        m = self._eval_neighbours(n_neighbours)
        P, n_item, n_cate, _ = self._din_sizes()
        shape = tuple(u_iid_seq.shape) if hasattr(u_iid_seq, "shape") else np.shape(u_iid_seq)
        one = np.zeros((shape[0], 1) if len(shape) == 2 else 1, np.int32)      # a stand-in candidate: the histories' checks
        U, _, Pq, single = check_rank_request(u_iid_seq, u_icat_seq, one, one, P, n_item, n_cate)
        held = check_held_out(held_out, U, single, "evaluate_two_stage")
        T = held.shape[1]
        ids = _exclusion_ids(u_iid_seq, exclude, U, exclude_seen)
        ci, cc = self._cat["host"]
        cap = candidate_capacity(self.catalogue_size, Pq, m)
        nb = self._narrowed_neighbours(m)
        hi, hc = (self._dev32(x, U) if Pq else torch.zeros((U, 0), dtype=torch.int32) for x in (u_iid_seq, u_icat_seq))
        # every slot's class, on the host: padding, missing / excluded, or eligible (what the retrieval stage may keep or lose)
        known = _target_positions(self._cat["first"], held) >= 0
        for u in range(U):
            known[u] &= ~np.isin(held[u], ids[u][ids[u] > 0])
        rank = np.where(held > 0, RANK_MISSING, RANK_PAD).astype(np.int32)
        retrieved = np.where(held > 0, np.where(known, 0, RETRIEVED_MISSING), RETRIEVED_PAD).astype(np.int8)
        tindex = np.full((U, T), -1, np.int32)
        tprob = np.full((U, T), np.nan, np.float32)
        n_cand = np.zeros(U, np.int32)
        excl = self._device_exclusion(ids) if self._evaluate_two_stage_on_device(T, cap) else None
        if excl is not None:
            self.evaluate_two_stage_path = "device"
            Tc = self._target_capacity(T)
            tgt = np.zeros((U, Tc), np.int32)                        # slots without an eligible target: id 0, which matches nothing
            tgt[:, :T] = np.where(known, held, 0)
            self._rank_setup(min(U, user_block))
            for b in range(0, U, user_block):
                e = min(U, b + user_block)
                count, pos, score, n_cand[b:e] = self._eval_two_stage_block(hi[b:e], hc[b:e], P, Pq, excl[b:e],
                                                                            np.ascontiguousarray(tgt[b:e]), cap, not exclude_seen, nb)
                ok = count[:, :T] >= 0
                rank[b:e][ok], retrieved[b:e][ok] = count[:, :T][ok], 1
                tindex[b:e][ok], tprob[b:e][ok] = pos[:, :T][ok], score[:, :T][ok]
        else:
            self.evaluate_two_stage_path = "host"
            hist_np = hi.cpu().numpy()
            ex_np = None
            if exclude is not None:
                ex_np = (exclude.detach().cpu().numpy() if hasattr(exclude, "detach") else np.asarray(exclude)).reshape(U, -1)
            npos, _, ncnt = nb["host"]
            for b in range(0, U, user_block):
                e = min(U, b + user_block)
                rows = retrieve_candidates_host(npos, ncnt, ci, hist_np[b:e], None if ex_np is None else ex_np[b:e], exclude_seen)
                width = max(1, max(len(x) for x in rows))
                li, lc = np.zeros((e - b, width), np.int32), np.zeros((e - b, width), np.int32)     # padded with (item 0, category 0)
                for u, x in enumerate(rows):
                    li[u, :len(x)], lc[u, :len(x)] = ci[x], cc[x]
                prob = self.rank_candidates(hi[b:e], hc[b:e], li, lc)["prob"].reshape(e - b, width)
                for u, x in enumerate(rows):
                    n_cand[b + u] = len(x)
                    s, cid = prob[u, :len(x)], ci[x].astype(np.int64)
                    for t in np.flatnonzero(known[b + u]):
                        at = np.flatnonzero(cid == held[b + u, t])
                        if len(at):
                            c = int(at[0])
                            rank[b + u, t], retrieved[b + u, t] = _list_place(s, c), 1
                            tindex[b + u, t], tprob[b + u, t] = x[c], s[c]
        out = two_stage_metrics(rank, retrieved, n_cand, ks, per_user)
        if single:
            out.update(rank=rank[0], retrieved=retrieved[0], target_index=tindex[0], target_prob=tprob[0], n_candidates=int(n_cand[0]))
        else:
            out.update(rank=rank, retrieved=retrieved, target_index=tindex, target_prob=tprob, n_candidates=n_cand)
        return out

    # -- public ------------------------------------------------------------------------------------------------------------
    def _parse(self, serialized):
        from . import input_pipeline as ip
        if self.script == "din":
            return ip.parse_din_examples(serialized, int(self.manifest["params"].get("hist_len", 100)))[0]
        if self.manifest["feature_set"] == "uid_iid":
            return {"ids": parse_uid_iid_examples(serialized, self.layout)}
        return ip.parse_criteo_examples(serialized, self.layout)[0]

    def predict(self, features):
        """One parsed batch ({'ids': int32 [B, F]}, + 'cont_log' for xdeepfm.py; din.py: its four id arrays), host or device
        -> {'prob': float32 numpy [B]}."""
        import torch
        from .estimator import ModeKeys
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
