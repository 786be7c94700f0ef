"""Item ranking for the model the reference serves: deepfm/deepfm.py AS COMMITTED (`--feature_set uid_iid`: two int64
features u_id / i_id).  "This user, these N items: score them and give me the best k" -- what `serving_din.DinRanking` answers
for din.py, for bundles whose manifest says feature_set == "uid_iid".  `serving.Predictor` inherits `PairRanking`.

  expand_pair_request(layout, u_id, i_id)   the DEFINITION: a ranking request is `predict` on this expansion, reshaped.
  Predictor.rank_items(u_id, i_id, top_k)   prob [C] / [U, C], or the k best of every user in `topk_rows_host`'s order.
  Predictor.set_item_catalogue(i_id)        N distinct raw ids >= 0, hashed once, resident.
  Predictor.recommend_items(u_id, top_k, exclude)   the best catalogue entries `exclude` does not name;
                                            `recommend_items_host` is the definition.

pair_path == "fused": inside rsx_predict_pair_rank's envelope (csrc/predict_pair.hip; D in {8, 16, 32}, 1..3 layers): the ids
are hashed ONCE on the host (U + C hashes for a shared list, not 2 U C), a chunk of the request is ONE launch -- a workgroup
scores 16 items of one user, the user's row fetched once per workgroup -- and with top_k rsx_topk_rows runs behind it and keeps
the running list on the device.  The rsx_predict_model points at what the Predictor already holds (the fused buffers when
path == "fused", else the rebuilt Estimator's store): no second copy of the tables, and nothing is allocated before the first
ranking request.  pair_path == "layers" (any other shape): `predict(expand_pair_request(...))` and the selection on the host,
the same API and the same order.  `path`, `predict` and `predict_examples` are untouched either way.

Scores are RAW, as for the din.py request kinds, also on a bundle with a calibration map: a non-strict isotonic map can create
ties and so change the order.  `Predictor.calibrate` maps a returned array for callers who want mapped probabilities.
"""
import ctypes as C

import numpy as np

from . import _lib
from .serving_din import EXCL_MAX, TOPK_MAX_K, DinRanking, _check_int, _fit_slice, _one_user, _ship_exclusion, check_top_k, \
    topk_rows_host

USER_KEY, ITEM_KEY = "u_id", "i_id"
PAIR_GRAPH_KINDS = ("pair_rank", "pair_topk", "pair_recommend")


# ---- requests: pure numpy (+ the library's host hash), no device -----------------------------------------------------------
def _raw_ids(what, name, x):
    """Raw int64 ids of a request argument (numpy, torch, list, scalar) -> numpy int64 of the same shape; RsxError unless it
    holds integers (no bool)."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.size == 0:                                            # (an empty list has no integer dtype of its own)
        return np.zeros(a.shape, np.int64)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise _lib.RsxError("%s: %s must hold integers, not %s" % (what, name, a.dtype))
    return a.astype(np.int64)


def pair_slots(layout):
    """(slot of u_id, slot of i_id) in input_layer's name order; RsxError unless the layout is exactly those two fields."""
    keys = [c.key for c in layout.columns]
    if sorted(keys) != [ITEM_KEY, USER_KEY]:
        raise _lib.RsxError("pair ranking needs the two fields %s and %s, this layout has %s" % (USER_KEY, ITEM_KEY, keys))
    return keys.index(USER_KEY), keys.index(ITEM_KEY)


def hash_pair_ids(layout, key, raw):
    """Table-local ids of raw int64 keys of ONE field (deepfm/deepfm.py:41,46: Fingerprint64 of the decimal string modulo the
    column's buckets) -> int32, the shape of `raw`.  What `layout.transform_int64` computes for that column."""
    col = next(c for c in layout.columns if c.key == key)
    keys = np.ascontiguousarray(np.asarray(raw, np.int64).reshape(-1))
    out = np.empty(keys.shape[0], np.int32)
    if keys.shape[0]:
        _lib.check(_lib.lib().rsx_hash_int64_keys_h(keys.ctypes.data_as(C.c_void_p), keys.shape[0], col.rows,
                                                    out.ctypes.data_as(C.c_void_p)), "rsx_hash_int64_keys_h")
    return out.reshape(np.shape(raw))


def check_pair_request(u_id, i_id, what="rank_items"):
    """Argument checking of `rank_items` -> (u int64 [U], items int64 [C] (shared) or [U, C], single).  u_id: a raw int64
    scalar (`single`: the answer drops the user axis) or [U]; i_id: [C], one list for all users, or [U, C].  Refuses
    non-integers, other shapes, a scalar user with a 2-D list, U rows of items for another number of users, an empty request."""
    u, it = _raw_ids(what, USER_KEY, u_id), _raw_ids(what, ITEM_KEY, i_id)
    single = u.ndim == 0
    if u.ndim > 1 or it.ndim not in (1, 2) or (single and it.ndim != 1):
        raise _lib.RsxError("%s: expected u_id a scalar or [U] and i_id [C] or [U, C] (a scalar user takes one list [C]); got u_id %s, "
                            "i_id %s" % (what, u.shape, it.shape))
    u = u.reshape(-1)
    if it.ndim == 2 and it.shape[0] != u.shape[0]:
        raise _lib.RsxError("%s: %d rows of items for %d users" % (what, it.shape[0], u.shape[0]))
    if u.shape[0] < 1 or it.shape[-1] < 1:
        raise _lib.RsxError("%s: an empty request (U = %d users, C = %d items)" % (what, u.shape[0], it.shape[-1]))
    return u, it, single


def expand_pair_request(layout, u_id, i_id):
    """The batch that asks `predict` the question of `rank_items`: example u * C + c is (user u, item c of user u) -> ids int32
    [U * C, 2] in slot order through `layout.transform_int64` (every pair hashed on its own: 2 U C hashes)."""
    u, it, _ = check_pair_request(u_id, i_id, "expand_pair_request")
    pair_slots(layout)
    U, Cn = u.shape[0], it.shape[-1]
    items = np.broadcast_to(it, (U, Cn))
    return layout.transform_int64({USER_KEY: np.repeat(u, Cn), ITEM_KEY: np.ascontiguousarray(items).reshape(-1)})


def check_item_catalogue(i_id):
    """`set_item_catalogue`'s argument -> int64 [N]: a 1-D integer array, N >= 1, every id >= 0 and distinct; RsxError names
    the first offender."""
    a = _raw_ids("set_item_catalogue", ITEM_KEY, i_id)
    if a.ndim != 1 or a.shape[0] < 1:
        raise _lib.RsxError("set_item_catalogue: expected i_id [N] with N >= 1, got %s" % (a.shape,))
    neg = np.flatnonzero(a < 0)
    if neg.size:
        raise _lib.RsxError("set_item_catalogue: i_id[%d] = %d is negative (ids are >= 0)" % (int(neg[0]), int(a[neg[0]])))
    order = np.argsort(a, kind="stable")
    same = np.flatnonzero(a[order][1:] == a[order][:-1])
    if same.size:
        at = int(order[same + 1].min())                      # the first position that repeats an earlier one
        raise _lib.RsxError("set_item_catalogue: i_id[%d] = %d repeats i_id[%d] (ids are distinct)"
                            % (at, int(a[at]), int(np.flatnonzero(a == a[at])[0])))
    return a


def check_pair_exclude(exclude, U, single, what="recommend_items"):
    """`exclude` of `recommend_items` -> int64 [U, E']: None (nothing), [E'] for the one-user form, [U, E'] for U users."""
    if exclude is None:
        return np.zeros((U, 0), np.int64)
    e = _raw_ids(what, "exclude", exclude)
    if e.ndim != (1 if single else 2) or (not single and e.shape[0] != U):
        raise _lib.RsxError("%s: exclude %s does not match the users: [E] for a scalar u_id, [U, E] for U = %d users"
                            % (what, e.shape, U))
    return e.reshape(U, -1)


def exclusion_positions(cat_item, exclude):
    """exclude: int64 [U, E'] raw ids (< 0 padding) -> int64 [U, E']: the catalogue position + 1 of every id, 0 for padding and
    for ids the catalogue does not hold.  cat_item: distinct ids (`check_item_catalogue`).  This is how rsx_topk_rows_excl's
    int32 "positive entries" contract serves any int64 id: the selection's cand_id is arange(1, N + 1)."""
    cat = np.asarray(cat_item, np.int64)
    order = np.argsort(cat, kind="stable")
    at = np.minimum(np.searchsorted(cat[order], exclude), len(cat) - 1)
    hit = (exclude >= 0) & (cat[order][at] == exclude)
    return np.where(hit, order[at] + 1, 0).astype(np.int64)


def recommend_items_host(prob, cat_item, exclude, top_k):
    """The definition of `Predictor.recommend_items`, in numpy.  prob: float32 [N] (one user) or [U, N], the scores of the N
    catalogue entries; cat_item: int64 [N], their raw ids; exclude: None or raw ids [E'] / [U, E'], entries < 0 padding (item 0
    is a real item), ids the catalogue does not hold exclude nothing.  The entries `exclude[u]` does not name, in the order of
    `topk_rows_host` (higher score first, equal ones -- two ids in one hash bucket -- by the lower position, NaN last), the first
    top_k of them -> {'prob': float32 [U, kk], 'item': int64 [U, kk], 'index': int32 [U, kk], 'count': int32 [U]},
    kk = min(top_k, N), count[u] = min(top_k, eligible entries); entries at and beyond count[u] are NaN / -1 / -1.  The
    one-user form returns the three arrays cut to count, and count as an int."""
    k = _check_int("recommend_items", "top_k", top_k)
    a, cat = np.asarray(prob, np.float32), np.asarray(cat_item)
    if a.ndim not in (1, 2) or cat.ndim != 1 or a.shape[-1] != cat.shape[0] or cat.shape[0] < 1:
        raise _lib.RsxError("recommend_items_host: expected scores [N] or [U, N] over a catalogue [N], N >= 1; got %s and %s"
                            % (a.shape, cat.shape))
    rows = np.atleast_2d(a)
    U, N = rows.shape
    ex = check_pair_exclude(exclude, U, a.ndim == 1, "recommend_items_host")
    kk = min(k, N)
    out = {"prob": np.full((U, kk), np.nan, np.float32), "item": np.full((U, kk), -1, np.int64),
           "index": np.full((U, kk), -1, np.int32), "count": np.zeros(U, np.int32)}
    for u in range(U):
        pos = np.flatnonzero(~np.isin(cat, ex[u][ex[u] >= 0]))
        order = pos[np.lexsort((pos, -rows[u, pos]))][:kk]
        c = len(order)
        out["prob"][u, :c], out["item"][u, :c], out["index"][u, :c], out["count"][u] = rows[u, order], cat[order], order, c
    return out if a.ndim == 2 else _one_user(out)


# ---- PairRanking -----------------------------------------------------------------------------------------------------------
class PairRanking:
    """The requests of a uid_iid deepfm.py bundle, as `serving.Predictor` inherits them beside `DinRanking`: no __init__.  It
    reads what `Predictor.load` sets (`script`, `manifest`, `layout`, `path`, `_model`, `_est`, `_pair`, `_item_cat` ...) and
    calls its `_run`, `_drop_graphs`, `predict`.  Its static buffers live in `_pair`, a dictionary of its own (DinRanking's
    `_scratch` keeps din.py's in `_rank`), created by the first ranking request."""

    def _is_pair_bundle(self):
        return getattr(self, "script", None) == "deepfm" and self.manifest.get("feature_set") == "uid_iid"

    def _need_pairs(self, what):
        if not self._is_pair_bundle():
            script = getattr(self, "script", None)
            fs = (getattr(self, "manifest", None) or {}).get("feature_set")
            raise _lib.RsxError("%s: only deepfm.py bundles exported with --feature_set uid_iid rank items for a user; this bundle "
                                "is %s.py%s" % (what, script, " with feature_set %s" % fs if fs else ""))

    def _pair_shape(self):
        """(D, widths, their C array or None) of the bundle's tower."""
        widths, wa = self._tower_widths()
        return int(self.manifest["params"]["embedding_size"]), widths, wa

    @property
    def pair_path(self):
        """"fused": ranking requests run rsx_predict_pair_rank; "layers": through `predict` on the expansion; None for a
        bundle that ranks no items.  A pure function of the bundle and `max_candidates`: nothing is allocated by asking."""
        if not self._is_pair_bundle():
            return None
        D, widths, wa = self._pair_shape()
        ok = wa is not None and self.layout.F == 2 and bool(
            _lib.lib().rsx_predict_pair_rank_supported(1, self.max_candidates, D, len(widths), wa))
        if ok and self.path == "layers":          # the model points into the store: every variable must be stored dense
            st = self._est.store
            ok = all(st.dense[k].is_contiguous() for k in self._pair_dense_names(widths))
        return "fused" if ok else "layers"

    @staticmethod
    def _pair_dense_names(widths):
        return ["dnn.%s%d" % (v, l) for l in range(len(widths)) for v in ("W", "b", "gamma", "beta")] + \
            ["dnn.Wout", "dnn.bout", "b1", "out.W", "out.b"]

    def _pair_model(self):
        """rsx_predict_model over what the Predictor already holds: the fused path's own model (a D = 16 bundle, its table as
        stored), or pointers into the rebuilt Estimator's store.  Nothing is copied."""
        if self.path == "fused":
            return self._model, ()
        D, widths, _ = self._pair_shape()
        st = self._est.store
        arena, dn = st.embeddings["input_layer"], st.dense
        pm = _lib.PredictModel()
        pm.tables, pm.w1, pm.row_off = arena.tables.data_ptr(), arena.w1.data_ptr(), arena.row_off.data_ptr()
        for l, n in enumerate(widths):
            pm.W[l], pm.b[l] = dn["dnn.W%d" % l].data_ptr(), dn["dnn.b%d" % l].data_ptr()
            pm.gamma[l], pm.beta[l] = dn["dnn.gamma%d" % l].data_ptr(), dn["dnn.beta%d" % l].data_ptr()
            pm.widths[l] = n
        pm.wd, pm.bd, pm.c0 = dn["dnn.Wout"].data_ptr(), dn["dnn.bout"].data_ptr(), dn["b1"].data_ptr()
        pm.wo, pm.bo = dn["out.W"].data_ptr(), dn["out.b"].data_ptr()
        pm.w1_field_mask, pm.bn_eps = int(arena.w1_mask), float(self.manifest["batch_norm_epsilon"])
        pm.F, pm.D, pm.L = 2, D, len(widths)
        pm.table_dtype = _lib.TABLE_DTYPES["float32"]         # (the layers path widened a 16-bit table on the host)
        return pm, (arena, dn)

    def _pair_setup(self, U):
        """The model and the static request buffers for U users: user ids [U], item ids and probabilities
        [U, max_candidates].  A request of fewer users or items uses leading parts; more users reallocate (the graphs captured
        over the smaller buffers go, with every scratch entry)."""
        import torch
        r = self._pair
        if r is None:
            pm, keep = self._pair_model()
            r = self._pair = {"model": pm, "keep": keep, "U": 0, "user_slot": pair_slots(self.layout)[0]}
        if U > r["U"]:
            dev = self.device
            self._drop_graphs(*PAIR_GRAPH_KINDS)
            for name in ("topk", "rec"):
                r.pop(name, None)
            r["user"] = torch.zeros(U, dtype=torch.int32, device=dev)
            r["item"] = torch.zeros(U * self.max_candidates, dtype=torch.int32, device=dev)
            r["prob"] = torch.zeros(U * self.max_candidates, dtype=torch.float32, device=dev)
            r["U"] = U
        return r

    def _pair_scratch(self, name, kind, need, alloc):
        """`DinRanking._scratch` over `_pair`: the buffers one request kind keeps beside the rank buffers, reallocated (the
        graphs of `kind` dropped) when a request needs more "pairs" than they hold."""
        t = self._pair.get(name)
        if t is None or need > t["pairs"]:
            self._drop_graphs(kind)
            t = self._pair[name] = alloc()
            t["pairs"] = need
        return t

    def pair_buffer_bytes(self, U=1, top_k=None):
        """Bytes of the static buffers a ranking request of U users holds (with top_k: the device selection's included)."""
        n = 4 * (U + 2 * U * self.max_candidates)
        if top_k is not None and self._pair_topk_on_device(check_top_k(top_k)):
            n += 4 * (2 * U * int(top_k) + 2 * U)
        return n

    def _pair_launch(self, U, n, item_ptr, item_ld):
        import torch
        r = self._pair
        _lib.check(_lib.lib().rsx_predict_pair_rank(C.byref(r["model"]), r["user_slot"], r["user"].data_ptr(), item_ptr,
                                                    int(item_ld), r["prob"].data_ptr(), int(U), int(n),
                                                    torch.cuda.current_stream().cuda_stream), "rsx_predict_pair_rank")

    def _pair_chunk_in(self, r, U, rows, s, e, shared):
        """Items [s, e) of the request's hashed rows into the static buffer -> item_ld of the launch."""
        import torch
        n = e - s
        if shared:
            r["item"][:n].copy_(torch.from_numpy(rows[s:e]), non_blocking=True)
            return 0
        r["item"][:U * n].view(U, n).copy_(torch.from_numpy(np.ascontiguousarray(rows[:, s:e])), non_blocking=True)
        return n

    # -- top-k, selected on the device (csrc/topk.hip) ----------------------------------------------------------------------
    def _pair_topk_on_device(self, k):
        return self.pair_path == "fused" and k <= TOPK_MAX_K and bool(_lib.lib().rsx_topk_rows_supported(1, k))

    def pair_topk_path_for(self, top_k):
        """Where `rank_items(..., top_k=top_k)` selects: "device" or "host" (None for a bundle that ranks no items).  A pure
        function of the bundle and k; `pair_topk_path` records what the latest request took."""
        if not self._is_pair_bundle():
            return None
        return "device" if self._pair_topk_on_device(check_top_k(top_k)) else "host"

    def _pair_topk_launch(self, U, n, k, item_ld):
        import torch
        r = self._pair
        t = r["topk"]
        self._pair_launch(U, n, r["item"].data_ptr(), item_ld)
        _lib.check(_lib.lib().rsx_topk_rows(r["prob"].data_ptr(), int(n), int(U), int(n), int(k), t["buf"].data_ptr(),
                                            t["buf"].data_ptr() + 4 * U * k, t["state"].data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "rsx_topk_rows")

    def rank_items(self, u_id, i_id, top_k=None):
        """uid_iid deepfm.py bundles: score C items for ONE user -- u_id a raw int64 scalar, i_id raw [C] ->
        {'prob': float32 numpy [C]} -- or for U users: u_id [U] with i_id [C] (one list for all users) or [U, C] -> prob [U, C].
        prob[u, c] is `predict` on the example (u_id[u], i_id[u, c]): `expand_pair_request` is the definition.  RAW scores,
        also on a calibrated bundle (`Predictor.calibrate` maps an array; a non-strict map can create ties).
        top_k=k: only the k' = min(k, C) best items of every user -> {'prob': [k'] / [U, k'], 'index': int32, positions on the
        request's item axis}, in `topk_rows_host`'s order.  `pair_topk_path_for(k)` says where: "device" (pair_path == "fused",
        k <= 1024): rsx_topk_rows behind every chunk's rank launch, in the chunk's graph, ONE copy of k' pairs at the end;
        "host": the probabilities, then `topk_rows_host`.  Both give the same bits.
        pair_path == "fused": ids hashed once on the host (U + C for a shared list), the request cut along C at max_candidates
        (with top_k: fitted to the selection's n + k <= 16384), one launch of rsx_predict_pair_rank per chunk, a request shape
        captured as a graph on its second use.  pair_path == "layers": `predict(expand_pair_request(...))`."""
        import torch
        self._need_pairs("rank_items")
        u, it, single = check_pair_request(u_id, i_id)
        U, Cn, shared = u.shape[0], it.shape[-1], it.ndim == 1
        shape = (Cn,) if single else (U, Cn)
        if top_k is not None:
            k = check_top_k(top_k)
            if not self._pair_topk_on_device(k):
                self.pair_topk_path = "host"
                out = topk_rows_host(self.rank_items(u, it)["prob"], k)
                return {key: v[0] for key, v in out.items()} if single else out
            self.pair_topk_path = "device"
        elif self.pair_path != "fused":
            ids = expand_pair_request(self.layout, u, it)
            return {"prob": self.predict({"ids": ids}, raw=True)["prob"].reshape(shape)}
        L = _lib.lib()
        urows, rows = hash_pair_ids(self.layout, USER_KEY, u), hash_pair_ids(self.layout, ITEM_KEY, it)
        cap = min(Cn, self.max_candidates)
        with torch.no_grad():
            r = self._pair_setup(U)
            r["user"][:U].copy_(torch.from_numpy(urows), non_blocking=True)
            if top_k is None:
                out = np.empty((U, Cn), np.float32)
                for s in range(0, Cn, cap):
                    e = min(Cn, s + cap)
                    ld = self._pair_chunk_in(r, U, rows, s, e, shared)
                    self._run(("pair_rank", U, e - s, ld), lambda: self._pair_launch(U, e - s, r["item"].data_ptr(), ld))
                    out[:, s:e] = r["prob"][:U * (e - s)].view(U, e - s).cpu().numpy()
                return {"prob": out.reshape(shape)}
            Ub = r["U"]
            t = self._pair_scratch("topk", "pair_topk", Ub * k, lambda: {
                "buf": torch.zeros(2 * Ub * k, dtype=torch.float32, device=self.device),
                "state": torch.zeros(2 * Ub, dtype=torch.int32, device=self.device)})
            t["state"].zero_()
            step = _fit_slice(cap, lambda n: L.rsx_topk_rows_supported(n, k))
            for s in range(0, Cn, step):
                e = min(Cn, s + step)
                ld = self._pair_chunk_in(r, U, rows, s, e, shared)
                self._run(("pair_topk", U, e - s, k, ld), lambda: self._pair_topk_launch(U, e - s, k, ld))
            h = t["buf"][:2 * U * k].cpu().numpy()                     # the ONE device-to-host copy of the request
        kk = min(k, Cn)
        out = {"prob": np.ascontiguousarray(h[:U * k].reshape(U, k)[:, :kk]),
               "index": np.ascontiguousarray(h[U * k:].view(np.int32).reshape(U, k)[:, :kk])}
        return {key: v[0] for key, v in out.items()} if single else out

    # -- recommendation over a resident catalogue (csrc/topk_excl.hip) --------------------------------------------------------
    def set_item_catalogue(self, i_id):
        """The servable items: [N] raw ids, every id >= 0 and distinct (`check_item_catalogue` names the first offender).  Hashed
        once; on the fused path the rows stay on the device as int32 [N] beside arange(1, N + 1), the selection's cand_id.
        `item_catalogue_size` reports N.  A second call replaces the catalogue and drops the graphs captured over the old one."""
        import torch
        self._need_pairs("set_item_catalogue")
        raw = check_item_catalogue(i_id)
        self._drop_graphs("pair_recommend")
        cat = {"raw": raw}
        if self.pair_path == "fused":
            N = raw.shape[0]
            cat["rows"] = torch.from_numpy(hash_pair_ids(self.layout, ITEM_KEY, raw)).to(self.device)
            cat["cand"] = torch.arange(1, N + 1, dtype=torch.int32, device=self.device)
        self._item_cat = cat
        self.item_catalogue_size = int(raw.shape[0])

    def _recommend_items_on_device(self, k):
        return self.pair_path == "fused" and k <= TOPK_MAX_K and bool(_lib.lib().rsx_topk_rows_excl_supported(1, k, 0))

    def recommend_items_path_for(self, top_k):
        """Where `recommend_items(..., top_k=top_k)` runs: "device" or "host" (None for a bundle that ranks no items).  A
        request that excludes more than 256 distinct catalogue entries for one user still takes the host path;
        `recommend_items_path` records what the latest request took."""
        if not self._is_pair_bundle():
            return None
        return "device" if self._recommend_items_on_device(check_top_k(top_k)) else "host"

    def _recommend_items_launch(self, U, k, E):
        """The whole request, one chain: the state's zeroing, then per chunk of max_candidates catalogue entries the rank launch
        over the resident rows (item_ld = 0) and the filtered selection, sliced where n + k is beyond its envelope.  Every
        address is fixed, so `_run` captures it as ONE graph per (U, k, E)."""
        import torch
        r, L = self._pair, _lib.lib()
        t, cat = r["rec"], self._item_cat
        val = t["buf"].data_ptr()
        idx, state = val + 4 * U * k, val + 8 * U * k
        t["buf"][2 * U * k:2 * U * k + 2 * U].zero_()
        stream = torch.cuda.current_stream().cuda_stream
        N = self.item_catalogue_size
        for s in range(0, N, self.max_candidates):
            n = min(self.max_candidates, N - s)
            self._pair_launch(U, n, cat["rows"].data_ptr() + 4 * s, 0)
            step = _fit_slice(n, lambda n_s: L.rsx_topk_rows_excl_supported(n_s, k, E))
            for s2 in range(0, n, step):
                _lib.check(L.rsx_topk_rows_excl(r["prob"].data_ptr() + 4 * s2, int(n), cat["cand"].data_ptr() + 4 * (s + s2),
                                                t["excl"].data_ptr(), int(E), int(U), min(step, n - s2), int(k), val, idx, state,
                                                stream), "rsx_topk_rows_excl")

    def recommend_items(self, u_id, top_k, exclude=None):
        """After `set_item_catalogue`: the top_k best catalogue entries for ONE user (u_id a scalar) or U users ([U]) that
        `exclude` does not name -- raw ids [E'] / [U, E'], entries < 0 padding, item 0 a real item, ids outside the catalogue
        exclude nothing.  -> {'prob': float32 [U, kk], 'item': int64 [U, kk] (the catalogue's raw id), 'index': int32 [U, kk]
        (the catalogue position), 'count': int32 [U]}, kk = min(top_k, N); entries at and beyond count[u] are NaN / -1 / -1.  One
        user: the arrays cut to count, count an int.  `recommend_items_host` is the definition; RAW scores as in `rank_items`.
        Two catalogue ids in one hash bucket score identically; the lower catalogue position wins the tie on both paths.
        `recommend_items_path_for(k)`: "device" (pair_path == "fused", k <= 1024, at most 256 distinct excluded entries per
        user): the host resolves every exclusion id to its catalogue position + 1 and ships U user ids plus those; the request
        is ONE captured graph per (U, k, exclusion capacity) -- per catalogue chunk rsx_predict_pair_rank with item_ld = 0, then
        rsx_topk_rows_excl -- and one copy brings the answer back.  "host": `rank_items` over the catalogue, then
        `recommend_items_host`.  Both give the same items, indices and probability bits."""
        import torch
        self._need_pairs("recommend_items")
        if self._item_cat is None:
            raise _lib.RsxError("recommend_items: no catalogue set -- call set_item_catalogue(i_id) first")
        k = _check_int("recommend_items", "top_k", top_k)
        raw = self._item_cat["raw"]
        u, _, single = check_pair_request(u_id, raw[:1], "recommend_items")
        U = u.shape[0]
        ex = check_pair_exclude(exclude, U, single)
        padded = None
        if self._recommend_items_on_device(k):
            padded = DinRanking._device_exclusion(exclusion_positions(raw, ex))
        if padded is None:
            self.recommend_items_path = "host"
            prob = self.rank_items(u[0] if single else u, raw)["prob"]
            return recommend_items_host(prob, raw, exclude, k)
        self.recommend_items_path = "device"
        with torch.no_grad():
            r = self._pair_setup(U)
            Ub = r["U"]
            t = self._pair_scratch("rec", "pair_recommend", Ub * k, lambda: {
                "buf": torch.zeros(2 * Ub * k + 2 * Ub, dtype=torch.float32, device=self.device),
                "excl": torch.zeros(Ub * EXCL_MAX, dtype=torch.int32, device=self.device)})
            r["user"][:U].copy_(torch.from_numpy(hash_pair_ids(self.layout, USER_KEY, u)), non_blocking=True)
            E = _ship_exclusion(t["excl"], padded, U)
            self._run(("pair_recommend", U, k, E), lambda: self._recommend_items_launch(U, k, E))
            h = t["buf"][:2 * U * k + 2 * U].cpu().numpy()           # the ONE device-to-host copy: pairs and `filled`
        kk = min(k, self.item_catalogue_size)
        count = h[2 * U * k:].view(np.int32).reshape(U, 2)[:, 0].copy()
        prob = np.ascontiguousarray(h[:U * k].reshape(U, k)[:, :kk])
        index = np.ascontiguousarray(h[U * k:2 * U * k].view(np.int32).reshape(U, k)[:, :kk])
        pad = np.arange(kk)[None, :] >= count[:, None]               # entries past `filled` are unspecified on the device
        prob[pad], index[pad] = np.nan, 0
        item = raw[index]
        item[pad], index[pad] = -1, -1
        out = {"prob": prob, "item": item, "index": index, "count": count}
        return _one_user(out) if single else out
