"""What a din.py bundle's `Predictor` answers beside `predict`: the pure-numpy definitions and argument checks, then
`DinRanking`, the base class `serving.Predictor` inherits the requests from (serving.py keeps the bundle, `load`, the
one-launch and layers paths, `_run` and `predict*`, and imports every public name of this module).
  Predictor   (continued from serving.py's module docstring)
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
              `recommend_two_stage(..., categories=, exclude_categories=, max_per_category=m)` puts `recommend`'s category
              rules on that list, restricted to the candidates: a disallowed entry is not retrieved, not scored and not counted
              (rsx_din_retrieve_candidates_rules, csrc/retrieve.hip, with the bitmap beside the exclusion ids) and the cap is
              applied over the candidates' own categories (rsx_topk_lists_capped, csrc/topk_capped.hip), still ONE graph and one
              copy back; `rules_on_device = False` sends such requests to the host path.  The same bits either way.
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

import numpy as np

from . import _lib


def _check_int(what, name, value, lo=1, hi=None, none_ok=False, message=None):
    """An integer argument (Python or numpy, no bool) >= lo, and <= hi if given -> int (None stays None when none_ok), else
    RsxError "<what>: <name> must be [None or ]an integer >= lo | in [lo, hi], not <value>"; `message`: another text before ", not"."""
    if value is None and none_ok:
        return None
    if (isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < lo
            or (hi is not None and int(value) > hi)):
        if message is None:
            message = "%s: %s must be %san integer %s" % (what, name, "None or " if none_ok else "",
                                                         ">= %d" % lo if hi is None else "in [%d, %d]" % (lo, hi))
        raise _lib.RsxError("%s, not %r" % (message, value))
    return int(value)


def _fit_slice(n, supported):
    """n halved (rounding up) until `supported(slice)` -- a kernel's `*_supported` with its other arguments bound -- takes it."""
    step = n
    while not supported(step):
        step = (step + 1) // 2
    return step


def _ship_exclusion(buf, ids, U):
    """ids: int32 [U, E] host (`_device_exclusion`) into the leading U * E words of an exclusion buffer -> E."""
    import torch
    E = int(ids.shape[1])
    if E:
        buf[:U * E].view(U, E).copy_(torch.from_numpy(ids), non_blocking=True)
    return E


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
    return _check_int("rank_candidates", "top_k", top_k)


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
    return _check_int("recommend", "max_per_category", max_per_category, none_ok=True)


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


def _catalogue_scores(what, prob, cat_item):
    """The first check of the host definitions: prob [N] / [U, N] over cat_item [N] -> (prob float32, cat_item, rows [U, N])."""
    a = np.asarray(prob, np.float32)
    cat = np.asarray(cat_item)
    if a.ndim not in (1, 2) or cat.ndim != 1 or a.shape[-1] != cat.shape[0] or cat.shape[0] < 1:
        raise _lib.RsxError("%s: expected scores [N] or [U, N] over a catalogue [N], N >= 1; got %s and %s" % (what, a.shape, cat.shape))
    return a, cat, np.atleast_2d(a)


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
    a, cat, rows = _catalogue_scores("recommend_host", prob, cat_item)
    U, N = rows.shape
    ids = _exclusion_ids(hist_item, exclude, U, exclude_seen)
    cc, only, deny, m = _category_rules("recommend_host", U, a.ndim == 1, cat, cat_cate, categories, exclude_categories,
                                        max_per_category, n_cate)
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
        order = order[:kk] if m is None else _capped_walk(order, cc, m, kk)
        c = len(order)
        out["prob"][u, :c], out["item"][u, :c], out["index"][u, :c], out["count"][u] = rows[u, order], cat[order], order, c
    return out if a.ndim == 2 else _one_user(out)


def _capped_walk(order, cc, m, kk):
    """The cap, as the plain greedy walk: `order` (catalogue positions, best first) walked once, a position kept only when
    fewer than m kept positions of its category cc[position] precede it, until kk are kept -> the kept positions."""
    taken, keep = {}, []
    for p in order:
        g = int(cc[p])
        if taken.get(g, 0) < m:
            taken[g] = taken.get(g, 0) + 1
            keep.append(p)
            if len(keep) == kk:
                break
    return np.asarray(keep, order.dtype)


def _category_rules(what, U, single, cat, cat_cate, categories, exclude_categories, max_per_category, n_cate):
    """The category arguments of a host definition checked -> (cc, only, deny, m): the two lists (`check_category_list`), the
    cap (`check_max_per_category`) and, when any of them is given, cat_cate as an integer array [N] like cat (RsxError
    otherwise); cc is None when no rule is given."""
    m = check_max_per_category(max_per_category)
    only = check_category_list(categories, "categories", U, single, n_cate)
    deny = check_category_list(exclude_categories, "exclude_categories", U, single, n_cate)
    if m is None and only is None and deny is None:
        return None, None, None, None
    cc = None if cat_cate is None else np.asarray(cat_cate)
    if cc is None or cc.shape != cat.shape or not np.issubdtype(cc.dtype, np.integer):
        raise _lib.RsxError("%s: a category rule needs cat_cate, integers [N] like cat_item; got %s"
                            % (what, None if cc is None else (cc.dtype, cc.shape)))
    return cc, only, deny, m


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
    a, cat, rows = _catalogue_scores("target_ranks_host", prob, cat_item)
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
    return [_check_int("ranking_metrics", "ks", k, message="ranking_metrics: ks must hold integers >= 1") for k in ks]


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
    return _check_int("build_neighbours", "n_neighbours", n_neighbours, hi=NBR_MAX)


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


def retrieve_candidates_host(nbr_pos, nbr_count, cat_item, hist_item, exclude=None, exclude_seen=True, cat_cate=None,
                             categories=None, exclude_categories=None, n_cate=None):
    """The definition of `Predictor.retrieve_candidates`, in numpy.  nbr_pos [N, n] / nbr_count [N]: `item_neighbours_host`'s
    table; cat_item int [N]; hist_item [P'] / [U, P']; exclude None or [E'] / [U, E'].  Per user: the SEEDS are the positive
    history ids that occur in the catalogue, each resolved to its lowest position (`catalogue_first_positions`); the candidates
    are the union of the seeds' neighbour rows -- with exclude_seen=False joined by every position whose item id is a seed id
    -- without every position whose item id is a positive id of the exclusion list (`_exclusion_ids`: the history when
    exclude_seen, then `exclude`; the list `recommend` uses).  -> a list of U int32 arrays: the sorted distinct positions.
    CATEGORY FILTERS (off by default; they need cat_cate: int [N], the category of every catalogue entry).  categories /
    exclude_categories: `recommend_host`'s lists ([G'] / [U, G'], negative ids padding, 0 a real category, an empty `categories`
    allows nothing, ids >= n_cate refused when n_cate is given).  A position whose category is not ALLOWED for the user is not
    a candidate at all.  The seeds are not filtered: a history item of a denied category still contributes its neighbours."""
    cat = np.asarray(cat_item).astype(np.int64)
    N = cat.shape[0]
    pos, cnt = check_neighbours(nbr_pos, nbr_count, N)
    h = hist_item.detach().cpu().numpy() if hasattr(hist_item, "detach") else np.asarray(hist_item)
    if h.ndim not in (1, 2):
        raise _lib.RsxError("retrieve_candidates_host: expected histories [P] or [U, P], got %s" % (h.shape,))
    U = 1 if h.ndim == 1 else h.shape[0]
    cc, only, deny, _ = _category_rules("retrieve_candidates_host", U, h.ndim == 1, cat, cat_cate, categories, exclude_categories,
                                        None, n_cate)
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
        if only is not None:
            mark &= np.isin(cc, only[u][only[u] >= 0])
        if deny is not None:
            mark &= ~np.isin(cc, deny[u][deny[u] >= 0])
        out.append(np.flatnonzero(mark).astype(np.int32))
    return out


def recommend_two_stage_host(prob, nbr_pos, nbr_count, cat_item, hist_item, exclude, top_k, exclude_seen=True, cat_cate=None,
                             categories=None, exclude_categories=None, max_per_category=None, n_cate=None):
    """The definition of `Predictor.recommend_two_stage`, in numpy.  prob: float32 [N] (one user) or [U, N], the scores of ALL
    catalogue entries (`rank_candidates` over the whole catalogue).  `recommend_host`'s order (higher score first, equal ones
    by the lower position, NaN last) restricted to the positions `retrieve_candidates_host` gives ->
    `recommend_host`'s dictionary, kk = min(top_k, N), count[u] = min(top_k, candidates of u): it can stay below top_k and can
    be 0 -- nothing is filled in from the rest of the catalogue.
    CATEGORY RULES (`recommend_host`'s, restricted to the retrieved candidates; all off by default, any of them needs cat_cate).
    categories / exclude_categories filter the candidates as `retrieve_candidates_host` does: a disallowed entry is not
    retrieved, not scored and not counted.  max_per_category = m: walk the user's candidates in the order above and keep an
    entry only when fewer than m kept entries of its category precede it; stop at top_k.  The cap counts entries, not ids, and
    count[u] can stay below top_k while candidates remain; there is still no back-fill."""
    k = check_top_k(top_k)
    a, cat, rows = _catalogue_scores("recommend_two_stage_host", prob, cat_item)
    U, N = rows.shape
    cc, _, _, m = _category_rules("recommend_two_stage_host", U, a.ndim == 1, cat, cat_cate, categories, exclude_categories,
                                  max_per_category, n_cate)
    cands = retrieve_candidates_host(nbr_pos, nbr_count, cat, hist_item, exclude, exclude_seen, cat_cate=cc, categories=categories,
                                     exclude_categories=exclude_categories, n_cate=n_cate)
    if len(cands) != U:
        raise _lib.RsxError("recommend_two_stage_host: %d histories for %d rows of scores" % (len(cands), U))
    kk = min(k, N)
    out = {"prob": np.full((U, kk), np.nan, np.float32), "item": np.full((U, kk), -1, np.int32),
           "index": np.full((U, kk), -1, np.int32), "count": np.zeros(U, np.int32)}
    for u, pos in enumerate(cands):
        pos = pos.astype(np.int64)
        order = pos[np.lexsort((pos, -rows[u, pos]))]
        order = order[:kk] if m is None else _capped_walk(order, cc, m, kk)
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
    a, cat, rows = _catalogue_scores("two_stage_ranks_host", prob, cat_item)
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
    m = _check_int("narrow_neighbours_host", "n_neighbours", m, hi=pos.shape[1],
                   message="n_neighbours must be an integer in [1, %d] (the table built)" % pos.shape[1])
    return np.ascontiguousarray(pos[:, :m]), np.minimum(cnt, m).astype(cnt.dtype)


# ---- DinRanking --------------------------------------------------------------------------------------------------------------
# What a captured graph of each key kind replays over: the rank buffers (with the scratch entries beside them), the catalogue,
# the neighbour table.  Replacing one drops the kinds that name it; a new request kind adds a row here and one `_scratch` caller.
GRAPH_DEPENDS = {"rank": ("buffers",), "rank_topk": ("buffers",),
                 "recommend": ("buffers", "catalogue"), "eval_recommend": ("buffers", "catalogue"),
                 "two_stage": ("buffers", "catalogue", "neighbours"), "eval_two_stage": ("buffers", "catalogue", "neighbours")}


class DinRanking:
    """The requests of a din.py bundle, as `serving.Predictor` inherits them: no __init__, no state of its own.  It reads what
    `Predictor.load` sets (`script`, `manifest`, `_est`, `_rank`, `_cat`, `_nbr` ...) and calls its `_run`, `_drop_graphs`, `predict`."""

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
            # (a request of fewer users or candidates uses leading parts of them; graphs captured over smaller buffers go, and
            # so does every scratch entry, sized by r["U"]: `_scratch` keeps them as dicts and nothing else in r is one)
            dev, i32 = self.device, torch.int32
            self._drop_dependents("buffers")
            for name in [k for k, v in r.items() if isinstance(v, dict)]:
                del r[name]
            r["hist"] = [torch.zeros(U * P, dtype=i32, device=dev) for _ in range(2)]
            r["cand"] = [torch.zeros(U * self.max_candidates, dtype=i32, device=dev) for _ in range(2)]
            r["prob"] = torch.zeros(U * self.max_candidates, dtype=torch.float32, device=dev)
            r["U"] = U
        return r

    def _drop_dependents(self, what):
        """Forgets the captured graphs of every kind that replays over `what` (a name of GRAPH_DEPENDS' right-hand sides)."""
        self._drop_graphs(*(kind for kind, deps in GRAPH_DEPENDS.items() if what in deps))

    def _scratch(self, name, graph_kinds, need, alloc):
        """-> self._rank[name], the static buffers one request kind keeps beside the rank buffers, sized by the users those
        hold.  `alloc()` -> {buffer name: tensor} is called, after the graphs of `graph_kinds` are dropped, when the entry is
        absent or its "pairs" are fewer than `need` (0: an entry of fixed size, which gets no "pairs").  `alloc` may return
        the current entry with some buffers replaced (`_ts_setup`)."""
        t = self._rank.get(name)
        if t is None or need > t.get("pairs", 0):
            self._drop_graphs(*graph_kinds)
            t = self._rank[name] = alloc()
            if need:
                t["pairs"] = need
        return t

    def _path_for(self, on_device):
        """What every `*_path_for` answers: None for a bundle that ranks no candidates -- it is asked nothing, its arguments
        are not looked at -- else "device" / "host" by `on_device()`, which checks the arguments first."""
        if self.script != "din":
            return None
        return "device" if on_device() else "host"

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
        return self._path_for(lambda: self._topk_on_device(check_top_k(top_k)))

    def _topk_setup(self, U, k):
        """The static buffers of the selection beside the rank buffers: one flat buffer that holds out_val [U, k] and, behind
        it, out_idx [U, k] of the request at hand (so both come back in ONE copy), and state [U, 2].  Reallocated like the
        rank buffers: when a request needs more than they hold (the graphs captured over the smaller ones go)."""
        import torch
        Ub = self._rank["U"]
        return self._scratch("topk", ("rank_topk",), Ub * k, lambda: {
            "buf": torch.zeros(2 * Ub * k, dtype=torch.float32, device=self.device),
            "state": torch.zeros(2 * Ub, dtype=torch.int32, device=self.device)})

    def _rank_topk_launch(self, U, n, k):
        """The rank launch of one chunk, then the selection over its probabilities: one launch, or -- when n + k is beyond
        rsx_topk_rows' envelope (n + k > 16 384) -- one per slice of the chunk, the chunk halved until a slice fits (the running
        list carries over; n = 16 000 with k = 1 024: two slices of 8 000, three launches for the chunk)."""
        import torch
        self._rank_launch(U, n)
        r = self._rank
        t, L = r["topk"], _lib.lib()
        step = _fit_slice(n, lambda m: L.rsx_topk_rows_supported(m, k))
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
        self._need_din("rank_candidates", "rank candidates against a history")
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
            return {"prob": self.predict(expand_rank_request(*host, hist_len=P), raw=True)["prob"].reshape(shape)}

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
    def _need_din(self, what, does="rank a catalogue against a history"):
        if getattr(self, "script", None) != "din":
            raise _lib.RsxError("%s: only din.py bundles %s; this bundle is %s.py" % (what, does, getattr(self, "script", None)))

    def _need_catalogue(self, what):
        self._need_din(what)
        if self._cat is None:
            raise _lib.RsxError("%s: no catalogue set -- call set_catalogue(i_id, i_cate) first" % what)

    def _need_neighbours(self, what):
        self._need_catalogue(what)
        if self._nbr is None:
            raise _lib.RsxError("%s: no neighbour table -- call build_neighbours() after set_catalogue" % what)
        return self._nbr

    def _history_request(self, what, u_iid_seq, u_icat_seq, exclude_seen, exclude, held_out=None):
        """The prologue of every request that takes histories and no candidates -> (U, P, Pq, single, ids): the histories
        checked as `rank_candidates` checks them (its messages) and the ids they name for exclusion (`_exclusion_ids`).  With
        held_out (the evaluations) -> (U, P, Pq, single, ids, held): `check_held_out` under `what`'s name, before `exclude`."""
        P, n_item, n_cate, _ = self._din_sizes()
        shape = tuple(u_iid_seq.shape) if hasattr(u_iid_seq, "shape") else np.shape(u_iid_seq)
        one = np.zeros((shape[0], 1) if len(shape) == 2 else 1, np.int32)      # a stand-in candidate: the histories' checks
        U, _, Pq, single = check_rank_request(u_iid_seq, u_icat_seq, one, one, P, n_item, n_cate)
        held = () if held_out is None else (check_held_out(held_out, U, single, what),)
        return (U, P, Pq, single, _exclusion_ids(u_iid_seq, exclude, U, exclude_seen)) + held

    def set_catalogue(self, i_id, i_cate):
        """din.py bundles: the servable items and their categories, two 1-D integer arrays of equal length N >= 1 (numpy or
        torch; `check_catalogue` refuses anything else and ids outside the tables).  Uploaded once as int32, a host copy is
        kept; `catalogue_size` reports N.  A second call replaces the catalogue and drops the graphs captured over the old one
        and `build_neighbours`' table, which names positions of the old catalogue."""
        import torch
        self._need_din("set_catalogue")
        _, n_item, n_cate, _ = self._din_sizes()
        ci, cc = check_catalogue(i_id, i_cate, n_item, n_cate)
        self._drop_dependents("catalogue")
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
        def on_device():
            k, m = check_top_k(top_k), check_max_per_category(max_per_category)
            return self._rules_on_device(k, m) if m is not None or rules else self._recommend_on_device(k)
        return self._path_for(on_device)

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
        Ub = self._rank["U"]
        t = self._scratch("rec", ("recommend",), Ub * k, lambda: {
            "buf": torch.zeros(2 * Ub * k + 2 * Ub, dtype=torch.float32, device=self.device),
            "excl": torch.zeros(Ub * EXCL_MAX, dtype=torch.int32, device=self.device)})
        if rules and "allow" not in t:
            t["allow"] = torch.zeros(Ub * ((self._din_sizes()[2] + 31) // 32), dtype=torch.int32, device=self.device)
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
        val = t["buf"].data_ptr()
        idx, state = val + 4 * U * k, val + 8 * U * k
        t["buf"][2 * U * k:2 * U * k + 2 * U].zero_()
        stream = torch.cuda.current_stream().cuda_stream
        if rules is None:                   # the two selection kernels differ in the envelope and the call of one slice
            fits, more = L.rsx_topk_rows_excl_supported, ()
            def select(scores, n, at, n_s):
                _lib.check(L.rsx_topk_rows_excl(scores, int(n), cat_i + 4 * at, t["excl"].data_ptr(), int(E), int(U), n_s, int(k),
                                                val, idx, state, stream), "rsx_topk_rows_excl")
        else:
            bitmap, m = rules
            G = self._din_sizes()[2]
            fits, more = L.rsx_topk_rows_rules_supported, (G, m)
            def select(scores, n, at, n_s):
                _lib.check(L.rsx_topk_rows_rules(scores, int(n), cat_i + 4 * at, t["excl"].data_ptr(), int(E), cat_c, G,
                                                 t["allow"].data_ptr() if bitmap else None, int(m), int(U), n_s, int(k),
                                                 val, idx, state, stream), "rsx_topk_rows_rules")
        for s, n in self._catalogue_chunks():
            self._rank_shared_launch(U, s, n)
            step = _fit_slice(n, lambda n_s: fits(n_s, k, E, *more))
            for s2 in range(0, n, step):
                select(r["prob"].data_ptr() + 4 * s2, n, s + s2, min(step, n - s2))

    def _catalogue_chunks(self):
        """(s, n) of every chunk of at most max_candidates catalogue positions [s, s + n), in order."""
        for s in range(0, self.catalogue_size, self.max_candidates):
            yield s, min(self.max_candidates, self.catalogue_size - s)

    def _rank_shared_launch(self, U, s, n):
        """rsx_predict_din_rank_shared: the U histories in place against the catalogue positions [s, s + n) -> r["prob"] [U, n]."""
        import torch
        r = self._rank
        cat_i, cat_c = (x.data_ptr() for x in self._cat["dev"])
        _lib.check(_lib.lib().rsx_predict_din_rank_shared(C.byref(r["model"]), r["hist"][0].data_ptr(), r["hist"][1].data_ptr(),
                                                          cat_i + 4 * s, cat_c + 4 * s, r["prob"].data_ptr(), int(U), int(n),
                                                          self._din_sizes()[0], torch.cuda.current_stream().cuda_stream),
                   "rsx_predict_din_rank_shared")

    def _recommend_device(self, U, k, P, Pq, u_iid_seq, u_icat_seq, ids, rules=None):
        """ids: int32 [U, E] host, E one of the exclusion capacities -> the answer of `recommend_host` for U users.
        rules: None, or (bitmap: uint32 [U, W] host or None, m: the cap or 0) of a request with a category rule; its graph is
        keyed by (U, k, E, bitmap present, m)."""
        import torch
        with torch.no_grad():
            r = self._rank_setup(U)
            t = self._rec_setup(U, k, rules is not None)
            self._rank_histories(r, U, P, Pq, u_iid_seq, u_icat_seq)
            E = _ship_exclusion(t["excl"], ids, U)
            how = None if rules is None else (rules[0] is not None, int(rules[1]))
            if how and how[0]:
                W = rules[0].shape[1]
                t["allow"][:U * W].view(U, W).copy_(torch.from_numpy(rules[0].view(np.int32)), non_blocking=True)
            self._run(("recommend", U, k, E) + (how or ()), lambda: self._recommend_launch(U, k, E, how))
            h = t["buf"][:2 * U * k + 2 * U].cpu().numpy()           # the ONE device-to-host copy: pairs and `filled`
        return self._unpack_list(h, U, k)

    def _unpack_list(self, h, U, k):
        """h: the host copy of out_val [U, k] | catalogue positions [U, k] | state [U, 2] -> `recommend_host`'s dictionary."""
        kk = min(k, self.catalogue_size)
        count = h[2 * U * k:].view(np.int32).reshape(U, 2)[:, 0].copy()
        prob = np.ascontiguousarray(h[:U * k].reshape(U, k)[:, :kk])
        index = np.ascontiguousarray(h[U * k:2 * U * k].view(np.int32).reshape(U, k)[:, :kk])
        pad = np.arange(kk)[None, :] >= count[:, None]               # entries past `filled` are unspecified on the device
        prob[pad], index[pad] = np.nan, 0
        item = self._cat["host"][0][np.maximum(index, 0)]
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
        self._need_catalogue("recommend")
        k = check_top_k(top_k)
        U, P, Pq, single, ids = self._history_request("recommend", u_iid_seq, u_icat_seq, exclude_seen, exclude)
        n_cate = self._din_sizes()[2]
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
            return recommend_host(prob, ci, u_iid_seq, exclude, k, exclude_seen, cat_cate=cc, categories=categories,
                                  exclude_categories=exclude_categories, max_per_category=m, n_cate=n_cate)
        return _one_user(out) if single else out

    # -- two-stage recommendation: item neighbours, candidates on the device (din.py; csrc/rows_dot.hip, retrieve.hip) ---------
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
        chunk = _fit_slice(min(N, self.max_candidates), lambda m: L.rsx_topk_rows_excl_supported(m, n, 1))
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
        self._drop_dependents("neighbours")
        self._nbr = None                                             # (with it go `evaluate_two_stage`'s narrowed copies)
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

    def _two_stage_rules_on_device(self, k, cap, m):
        """A two-stage request with a category rule (m: the cap, None or 0 for none): the plain request's conditions, the
        switch, m <= 16, and the envelopes of rsx_din_retrieve_candidates_rules and rsx_topk_lists_capped for this bundle's
        n_cate (each asked whether or not the request needs it: the answer is one per (k, cap, m))."""
        m = int(m or 0)
        if not (self.rules_on_device and self._two_stage_on_device(k, cap) and m <= RULES_MAX_M):
            return False
        P, _, G, _ = self._din_sizes()
        L = _lib.lib()
        return (bool(L.rsx_din_retrieve_candidates_rules_supported(self.catalogue_size, P, self._nbr["n"], 0, G))
                and bool(L.rsx_topk_lists_capped_supported(cap, k, G, m)))

    def two_stage_path_for(self, top_k, hist_len=None, max_per_category=None, rules=False):
        """Where `recommend_two_stage(..., top_k=top_k)` runs for histories of hist_len positions (default: the bundle's):
        "device" or "host" (None for a bundle that ranks no candidates).  "device" needs `build_neighbours`' table on the
        device, rank_path == "fused", k <= 1024 and a candidate capacity -- min(N, hist_len (n + 1)) rounded up to 64 -- of at
        most max_candidates.  A request that names more than 256 distinct positive exclusion ids for one user still takes the
        host path; `two_stage_path` records what the latest request took.  With max_per_category or rules=True (a request that
        names categories / exclude_categories) the answer is that of a request with a category rule: "device" needs
        `rules_on_device`, a cap of at most 16 and the envelopes of rsx_din_retrieve_candidates_rules and rsx_topk_lists_capped
        as well."""
        def on_device():
            k, m = check_top_k(top_k), check_max_per_category(max_per_category)
            if self._nbr is None:
                return False
            cap = self._two_stage_cap(self._din_sizes()[0] if hist_len is None else hist_len)
            return self._two_stage_rules_on_device(k, cap, m) if m is not None or rules else self._two_stage_on_device(k, cap)
        return self._path_for(on_device)

    def _ts_setup(self, U, k, rules=False):
        """The static buffers of a device two-stage request beside the rank buffers: cand_pos [U, max_candidates], n_cand [U],
        the exclusion ids [U, 256], and ONE flat buffer that holds out_val [U, k], behind it the catalogue positions [U, k] and
        state [U, 2] (so the answer and `filled` come back in one copy) and, last, out_idx [U, k], which stays on the device.
        The category bitmap [U, ceil(n_cate / 32)] joins them with the first request that names a category filter (rules)."""
        import torch
        Ub, dev, i32 = self._rank["U"], self.device, torch.int32

        def alloc():          # a longer list replaces "buf" alone: `evaluate_two_stage`'s graphs replay over "pos" and "excl"
            t = self._rank.get("ts") or {"pairs": 0, "buf": None, "pos": torch.zeros(Ub * self.max_candidates, dtype=i32, device=dev),
                                         "n_cand": torch.zeros(Ub, dtype=i32, device=dev),
                                         "excl": torch.zeros(Ub * EXCL_MAX, dtype=i32, device=dev)}
            if k:
                t["buf"] = torch.zeros(3 * Ub * k + 2 * Ub, dtype=torch.float32, device=dev)
            return t
        t = self._scratch("ts", ("two_stage",), Ub * k, alloc)
        if rules and "allow" not in t:
            t["allow"] = torch.zeros(Ub * ((self._din_sizes()[2] + 31) // 32), dtype=i32, device=dev)
        return t

    def _retrieve_launch(self, U, E, cap, seeds, nb, n_cand_ptr, bitmap=False):
        """rsx_din_retrieve_candidates over the U histories in place and the table `nb` (the built one or a narrowed copy): the
        positions into r["ts"]["pos"], the ids straight into the rank launch's candidate buffers, the counts to n_cand_ptr.
        bitmap: rsx_din_retrieve_candidates_rules with the category bitmap of r["ts"]["allow"] instead."""
        import torch
        r, t = self._rank, self._rank["ts"]
        cat_i, cat_c = (x.data_ptr() for x in self._cat["dev"])
        P, n_item, G = self._din_sizes()[:3]
        pos, _, count = nb["dev"]
        L = _lib.lib()
        head = (r["hist"][0].data_ptr(), P, self._nbr["first"].data_ptr(), n_item, pos.data_ptr(), count.data_ptr(), nb["n"], cat_i,
                cat_c, self.catalogue_size, t["excl"].data_ptr(), int(E), int(seeds))
        tail = (t["pos"].data_ptr(), r["cand"][0].data_ptr(), r["cand"][1].data_ptr(), n_cand_ptr, int(cap), int(U),
                torch.cuda.current_stream().cuda_stream)
        if bitmap:
            _lib.check(L.rsx_din_retrieve_candidates_rules(*head, t["allow"].data_ptr(), G, *tail), "rsx_din_retrieve_candidates_rules")
        else:
            _lib.check(L.rsx_din_retrieve_candidates(*head, *tail), "rsx_din_retrieve_candidates")

    def _two_stage_launch(self, U, k, E, cap, seeds, rules=None):
        """The whole request, one chain: the state's zeroing, rsx_din_retrieve_candidates (the candidates' ids straight into
        the rank launch's candidate buffers), rsx_predict_din_rank over [U, cap], rsx_topk_rows_counted, and the gather that
        turns the selected columns into catalogue positions.  Every address is fixed, so `_run` captures it as ONE graph per
        (U, k, E, cap, seeds).  k = 0: the retrieval alone (`retrieve_candidates`).
        rules = (bitmap present, m) for a request with a category rule: with a bitmap rsx_din_retrieve_candidates_rules takes
        the retrieval's place, and with m > 0 rsx_topk_lists_capped the selection's, over the candidate categories the
        retrieval wrote into the rank launch's buffer [U, cap]."""
        import torch
        r, t = self._rank, self._rank["ts"]
        bitmap, m = rules or (False, 0)
        if k:
            t["buf"][2 * U * k:2 * U * k + 2 * U].zero_()
        self._retrieve_launch(U, E, cap, seeds, self._nbr, t["n_cand"].data_ptr(), bitmap)
        if not k:
            return
        self._rank_launch(U, cap)
        val = t["buf"].data_ptr()
        state, idx = val + 8 * U * k, val + 8 * U * k + 8 * U
        L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
        if m:
            _lib.check(L.rsx_topk_lists_capped(r["prob"].data_ptr(), int(cap), t["n_cand"].data_ptr(), r["cand"][1].data_ptr(),
                                               int(cap), self._din_sizes()[2], int(m), int(U), int(cap), int(k), val, idx, state,
                                               stream), "rsx_topk_lists_capped")
        else:
            _lib.check(L.rsx_topk_rows_counted(r["prob"].data_ptr(), int(cap), t["n_cand"].data_ptr(), int(U), int(cap), int(k),
                                               val, idx, state, stream), "rsx_topk_rows_counted")
        ints = t["buf"].view(torch.int32)
        col = ints[2 * U * k + 2 * U:3 * U * k + 2 * U].view(U, k).clamp(0, cap - 1).long()     # (past `filled`: unspecified)
        torch.gather(t["pos"][:U * cap].view(U, cap), 1, col, out=ints[U * k:2 * U * k].view(U, k))

    def _two_stage_device(self, U, k, P, Pq, cap, u_iid_seq, u_icat_seq, ids, seeds, rules=None):
        """ids: int32 [U, E] host, E one of the exclusion capacities.  k = 0 -> (cand_pos [U, cap], n_cand [U]); otherwise the
        answer of `recommend_two_stage_host` for U users.  rules: None, or (bitmap: uint32 [U, W] host or None, m: the cap or
        0) of a request with a category rule; its graph's key ends in (bitmap present, m), a plain request's key is unchanged."""
        import torch
        with torch.no_grad():
            r = self._rank_setup(U)
            how = None if rules is None else (rules[0] is not None, int(rules[1]))
            t = self._ts_setup(U, k, bool(how and how[0]))
            self._rank_histories(r, U, P, Pq, u_iid_seq, u_icat_seq)
            E = _ship_exclusion(t["excl"], ids, U)
            if how and how[0]:
                W = rules[0].shape[1]
                t["allow"][:U * W].view(U, W).copy_(torch.from_numpy(rules[0].view(np.int32)), non_blocking=True)
            self._run(("two_stage", U, k, E, cap, bool(seeds)) + (how or ()),
                      lambda: self._two_stage_launch(U, k, E, cap, seeds, how))
            if not k:
                return t["pos"][:U * cap].view(U, cap).cpu().numpy(), t["n_cand"][:U].cpu().numpy()
            h = t["buf"][:2 * U * k + 2 * U].cpu().numpy()           # the ONE device-to-host copy: pairs and `filled`
        return self._unpack_list(h, U, k)

    def _two_stage_request(self, what, u_iid_seq, u_icat_seq, exclude_seen, exclude, categories=None, exclude_categories=None,
                           max_per_category=None):
        """-> (U, P, Pq, single, ids, cap, rules): rules is None for a request without a category rule, else (bitmap: uint32
        [U, W] or None when no list is given, m: the cap or 0) -- what `recommend` makes of the same three arguments."""
        self._need_neighbours(what)
        U, P, Pq, single, ids = self._history_request(what, u_iid_seq, u_icat_seq, exclude_seen, exclude)
        n_cate = self._din_sizes()[2]
        m = check_max_per_category(max_per_category)
        only = check_category_list(categories, "categories", U, single, n_cate)
        deny = check_category_list(exclude_categories, "exclude_categories", U, single, n_cate)
        rules = None
        if m is not None or only is not None or deny is not None:
            rules = (category_bitmap(only, deny, n_cate) if only is not None or deny is not None else None, m or 0)
        return U, P, Pq, single, ids, self._two_stage_cap(Pq), rules

    def _rank_lists_host(self, hi, hc, rows):
        """rows: per user the catalogue positions of a candidate list (`retrieve_candidates_host`) -> prob float32 [U, width]:
        `rank_candidates` over the lists padded to the longest with (item 0, category 0)."""
        ci, cc = self._cat["host"]
        width = max(1, max(len(x) for x in rows))
        li, lc = np.zeros((len(rows), width), np.int32), np.zeros((len(rows), width), np.int32)
        for u, x in enumerate(rows):
            li[u, :len(x)], lc[u, :len(x)] = ci[x], cc[x]
        return self.rank_candidates(hi, hc, li, lc)["prob"].reshape(len(rows), width)

    def retrieve_candidates(self, u_iid_seq, u_icat_seq, exclude_seen=True, exclude=None, categories=None, exclude_categories=None):
        """After `build_neighbours`: the catalogue positions stage two of `recommend_two_stage` would score for these histories
        ([P'] or [U, P']) -- `retrieve_candidates_host` is the definition -> {'index': int32 [U, cap], ascending, -1 beyond the
        count; 'count': int32 [U]}, cap = min(N, P' (n + 1)) rounded up to 64.  One user: index cut to count, count an int.
        With held-out items this measures the candidate recall of the retrieval stage.  categories / exclude_categories
        (`recommend`'s lists) keep only / drop the positions of those categories: the filtered positions come back, on the
        device through rsx_din_retrieve_candidates_rules when `rules_on_device` and its envelope allow."""
        U, P, Pq, single, ids, cap, rules = self._two_stage_request("retrieve_candidates", u_iid_seq, u_icat_seq, exclude_seen,
                                                                    exclude, categories, exclude_categories)
        on_device = self._retrieve_on_device(cap)
        if on_device and rules is not None:
            on_device = self.rules_on_device and bool(_lib.lib().rsx_din_retrieve_candidates_rules_supported(
                self.catalogue_size, self._din_sizes()[0], self._nbr["n"], 0, self._din_sizes()[2]))
        padded = self._device_exclusion(ids) if on_device else None
        if padded is not None:
            index, count = self._two_stage_device(U, 0, P, Pq, cap, u_iid_seq, u_icat_seq, padded, not exclude_seen, rules)
        else:
            pos, _, cnt = self._nbr["host"]
            ci, cc = self._cat["host"]
            rows = retrieve_candidates_host(pos, cnt, ci, u_iid_seq, exclude, exclude_seen, cat_cate=cc, categories=categories,
                                            exclude_categories=exclude_categories, n_cate=self._din_sizes()[2])
            index = np.full((U, cap), -1, np.int32)
            count = np.zeros(U, np.int32)
            for u, x in enumerate(rows):
                index[u, :len(x)], count[u] = x, len(x)
        if single:
            return {"index": index[0, :int(count[0])], "count": int(count[0])}
        return {"index": index, "count": count}

    def recommend_two_stage(self, u_iid_seq, u_icat_seq, top_k, exclude_seen=True, exclude=None, categories=None,
                            exclude_categories=None, max_per_category=None):
        """din.py bundles, after `set_catalogue` and `build_neighbours`: `recommend` over a RETRIEVED candidate set instead of
        the whole catalogue.  Stage one takes the neighbour rows of the history's items (`retrieve_candidates`), stage two scores
        those candidates exactly as `rank_candidates` scores them and returns the top_k best -- `recommend`'s result dictionary
        and one-user / U-user forms; `recommend_two_stage_host` is the definition.  count[u] = min(top_k, candidates of u): it
        can stay below top_k and can be 0 (an empty history, a history the catalogue does not hold).  There is NO back-fill
        from the rest of the catalogue, and the list differs from `recommend`'s by design: an entry outside the candidate set
        is never returned, however well it would score.
        `two_stage_path_for(k)` says where a request runs: "device": only the histories and the exclusion ids are shipped and
        the whole request -- rsx_din_retrieve_candidates, rsx_predict_din_rank over [U, cap], rsx_topk_rows_counted, the
        gather of the catalogue positions -- is ONE captured graph per (U, k, exclusion capacity, cap), one copy brings the
        answer back; "host": `retrieve_candidates_host`, `rank_candidates` on the padded lists, `topk_rows_host` over each
        list's valid part.  Both give the same bits.
        CATEGORY RULES (`recommend`'s arguments, `recommend_two_stage_host` defines them; a request without one is exactly
        the request above -- its graph key, its launches, its bits).  categories / exclude_categories keep only / drop the
        CANDIDATES of those categories: a disallowed entry is not retrieved, not scored and not counted, while a history item
        of a denied category still contributes its neighbours.  max_per_category = m keeps at most m entries of one category
        in the list, walking the candidates best first; count[u] can stay below top_k and nothing is filled in.
        `two_stage_path_for(k, hist_len, m, rules=True)` says where such a request runs: "device" (the conditions above,
        `rules_on_device`, m <= 16, the two kernels' envelopes): the lists are folded into a bitmap [U, ceil(n_cate / 32)]
        that is shipped with the exclusion ids; with a list rsx_din_retrieve_candidates_rules takes the retrieval's place and
        with a cap rsx_topk_lists_capped (csrc/topk_capped.hip) the selection's, over the candidate categories the retrieval
        wrote; still ONE captured graph, per (U, k, exclusion capacity, cap, seeds, bitmap present, m), and one copy back.
        "host": `retrieve_candidates_host` with the lists, `rank_candidates` on the padded lists, the greedy walk of
        `recommend_host`.  Both give the same bits."""
        k = check_top_k(top_k)
        U, P, Pq, single, ids, cap, rules = self._two_stage_request("recommend_two_stage", u_iid_seq, u_icat_seq, exclude_seen,
                                                                    exclude, categories, exclude_categories, max_per_category)
        on_device = self._two_stage_on_device(k, cap) if rules is None else self._two_stage_rules_on_device(k, cap, rules[1])
        padded = self._device_exclusion(ids) if on_device else None
        if padded is not None:
            self.two_stage_path = "device"
            out = self._two_stage_device(U, k, P, Pq, cap, u_iid_seq, u_icat_seq, padded, not exclude_seen, rules)
        else:
            self.two_stage_path = "host"
            pos, _, cnt = self._nbr["host"]
            ci, cc = self._cat["host"]
            rows = retrieve_candidates_host(pos, cnt, ci, u_iid_seq, exclude, exclude_seen, cat_cate=cc, categories=categories,
                                            exclude_categories=exclude_categories, n_cate=self._din_sizes()[2])
            hi, hc = (x.reshape(U, -1) if hasattr(x, "reshape") else np.asarray(x).reshape(U, -1) for x in (u_iid_seq, u_icat_seq))
            prob = self._rank_lists_host(hi, hc, rows)
            kk = min(k, self.catalogue_size)
            out = {"prob": np.full((U, kk), np.nan, np.float32), "item": np.full((U, kk), -1, np.int32),
                   "index": np.full((U, kk), -1, np.int32), "count": np.zeros(U, np.int32)}
            for u, x in enumerate(rows):
                if len(x):
                    if rules is not None and rules[1]:                 # the cap: every candidate in order, then the walk
                        best = topk_rows_host(prob[u, :len(x)], len(x))
                        keep = _capped_walk(best["index"], cc[x], rules[1], kk)
                        best = {"prob": prob[u, keep], "index": keep}
                    else:
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
        return self._path_for(lambda: self._evaluate_on_device(_check_int("evaluate_recommend", "T", T)))

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
        Ub = self._rank["U"]
        return self._scratch("eval", ("eval_recommend",), 0, lambda: {
            "buf": torch.zeros(2 * Ub * RANK_MAX_T, dtype=torch.float32, device=self.device),
            "tgt": torch.zeros(3 * Ub * RANK_MAX_T, dtype=torch.int32, device=self.device),
            "excl": torch.zeros(Ub * EXCL_MAX, dtype=torch.int32, device=self.device)})

    def _eval_launch(self, U, T, E):
        """One block of users, one chain: count's zeroing, the targets' own scores (one rsx_predict_din_rank launch over
        [U, T] pairs), then for every chunk of max_candidates catalogue entries the shared rank launch and the count of the
        entries that precede each target.  Every address is fixed, so `_run` captures it as ONE graph per (U, T, E)."""
        import torch
        r, t, L = self._rank, self._rank["eval"], _lib.lib()
        cat_i = self._cat["dev"][0].data_ptr()
        count = t["buf"].data_ptr()
        score = count + 4 * U * T
        item = t["tgt"].data_ptr()
        cate, pos = item + 4 * U * T, item + 8 * U * T
        t["buf"][:U * T].zero_()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(L.rsx_predict_din_rank(C.byref(r["model"]), r["hist"][0].data_ptr(), r["hist"][1].data_ptr(), item, cate, score,
                                          int(U), int(T), self._din_sizes()[0], stream), "rsx_predict_din_rank")
        for s, n in self._catalogue_chunks():
            self._rank_shared_launch(U, s, n)
            _lib.check(L.rsx_rank_count_rows(r["prob"].data_ptr(), int(n), cat_i + 4 * s, int(s), t["excl"].data_ptr(), int(E),
                                             score, pos, int(T), count, int(U), int(n), stream), "rsx_rank_count_rows")

    def _eval_device_block(self, hi, hc, P, Pq, excl, tgt):
        """hi, hc: int32 [U, P'] tensors; excl: int32 [U, E] host; tgt: int32 [3, U, T] host (item, category, position; T a
        target capacity) -> (count int32 [U, T], tgt_score float32 [U, T]) of one block of users."""
        import torch
        _, U, T = tgt.shape
        with torch.no_grad():
            r = self._rank
            t = self._eval_setup()
            self._rank_histories(r, U, P, Pq, hi, hc)
            E = _ship_exclusion(t["excl"], excl, U)
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
        self._need_catalogue("evaluate_recommend")
        ks = check_ks(ks)
        user_block = _check_int("evaluate_recommend", "user_block", user_block)
        U, P, Pq, single, ids, held = self._history_request("evaluate_recommend", u_iid_seq, u_icat_seq, exclude_seen, exclude, held_out)
        T = held.shape[1]
        ci, cc = self._cat["host"]
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
        return _check_int("evaluate_two_stage", "n_neighbours", n_neighbours, hi=n, none_ok=True, message="evaluate_two_stage: "
                          "n_neighbours must be None or an integer in [1, %d] (the table built)" % n) or n

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
        def on_device():
            Tn = _check_int("evaluate_two_stage", "T", T)
            if self._nbr is None:
                return False
            m = self._eval_neighbours(n_neighbours)
            cap = candidate_capacity(self.catalogue_size, self._din_sizes()[0] if hist_len is None else hist_len, m)
            return self._evaluate_two_stage_on_device(Tn, cap)
        return self._path_for(on_device)

    def _ets_setup(self):
        """The static buffers of a device `evaluate_two_stage` beside the rank buffers and the two-stage ones (cand_pos and the
        exclusion ids are `_ts_setup`'s), for the users the rank buffers hold and 32 targets each: the eligible targets' item
        ids [U, T], and ONE flat buffer with count, position and score, three [U, T], and behind them n_cand [U] of the block
        at hand -- so everything comes back in one copy."""
        import torch
        Ub = self._rank["U"]
        self._ts_setup(Ub, 0)
        return self._scratch("ets", ("eval_two_stage",), 0, lambda: {
            "tgt": torch.zeros(Ub * RANK_MAX_T, dtype=torch.int32, device=self.device),
            "out": torch.zeros(3 * Ub * RANK_MAX_T + Ub, dtype=torch.float32, device=self.device)})

    def _eval_two_stage_launch(self, U, T, E, cap, seeds, nb):
        """One block of users, one chain: rsx_din_retrieve_candidates (the candidates' ids straight into the rank launch's
        candidate buffers, as in `_two_stage_launch`; n_cand into the answer's buffer), rsx_predict_din_rank over [U, cap],
        rsx_rank_count_lists.  The last writes every output slot, so nothing is zeroed.  Every address is fixed, so `_run`
        captures it as ONE graph per (U, T, E, cap, seeds, m)."""
        import torch
        r, ts, t = self._rank, self._rank["ts"], self._rank["ets"]
        out = t["out"].data_ptr()
        n_cand = out + 12 * U * T
        self._retrieve_launch(U, E, cap, seeds, nb, n_cand)
        self._rank_launch(U, cap)
        _lib.check(_lib.lib().rsx_rank_count_lists(r["prob"].data_ptr(), int(cap), r["cand"][0].data_ptr(), ts["pos"].data_ptr(),
                                                   n_cand, t["tgt"].data_ptr(), int(T), out, out + 4 * U * T, out + 8 * U * T,
                                                   int(U), int(cap), torch.cuda.current_stream().cuda_stream),
                   "rsx_rank_count_lists")

    def _eval_two_stage_block(self, hi, hc, P, Pq, excl, tgt, cap, seeds, nb):
        """hi, hc: int32 [U, P'] tensors; excl: int32 [U, E] host; tgt: int32 [U, T] host (T a target capacity; 0 where the slot
        has no eligible target) -> (count int32 [U, T], position int32 [U, T], score float32 [U, T], n_cand int32 [U])."""
        import torch
        U, T = tgt.shape
        with torch.no_grad():
            r = self._rank
            t = self._ets_setup()
            self._rank_histories(r, U, P, Pq, hi, hc)
            E = _ship_exclusion(r["ts"]["excl"], excl, U)
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
        user_block = _check_int("evaluate_two_stage", "user_block", user_block)
        m = self._eval_neighbours(n_neighbours)
        U, P, Pq, single, ids, held = self._history_request("evaluate_two_stage", u_iid_seq, u_icat_seq, exclude_seen, exclude, held_out)
        T = held.shape[1]
        ci = self._cat["host"][0]
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
                prob = self._rank_lists_host(hi[b:e], hc[b:e], rows)
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
