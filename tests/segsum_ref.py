"""Reference of the sorted segment-sum (csrc/embedding.hip: rsx_segsum_bwd, rsx_segsum_partials, rsx_segsum_bwd_packed,
rsx_segsum_rows, rsx_segsum_adam_rows2) for tests/test_gpu_segsum_forms.py and tests/test_segsum_ref_cpu.py: the case table (with
the form each case was derived to take), the id generators, the inputs of a case, the fp64 reference and the float32
ascending-order restatement.  Nothing here touches the HIP library, so the CPU suite can import it.

The operation.  Per entry (example b, field f, row = row_off[f] + ids[b, f]) the term
    t[b, f, :] = (gy2[b] * S[b, :] - gy2[b] * T[row, :]) + dX[b, f*D:(f+1)*D]          (absent inputs dropped)
and the sums G[row] = sum_b t[b, f, :], g1[row] = sum_b gy1[b] over the fields in w1_field_mask (0 elsewhere).  S is an INPUT
here (the GPU test passes the kernel's own gather output, the CPU test the float32 field sum), so what is compared is the
scatter's arithmetic alone.

Forms (the host code of segsum_impl / rsx_segsum_adam_rows2, restated by `form_of` & co. below):
    two     B > TWO_STAGE_MIN_B = 1024: stage A (segsum_tiles_k<D, FM, W1>: position tiles of (256 / (D/4)) * 16 sorted positions,
            finishes every segment of <= 16 entries, leaves 16-position chunk partials of the longer ones) + stage B (row
            owners, a helper GROUP per segment of 17..256 entries, a helper WAVE per segment of > 256; at most 1024 workgroups,
            grid stride over the compact unit list)
    lds     single stage through LDS: B <= 512, waves per field a multiple of 4, staging <= 64 KiB
    wave    single stage, one wave per 64 / (D/4) unique rows: everything else up to B = 1024
Within the single-stage forms a field whose unique rows are at most its waves is SPREAD (one row per wave; the wave's lane
groups cooperate on a segment of 3 .. GPW entries, one entry each, and on every segment of more than 16); the others are DEALT
(several rows per wave, cooperation from 17)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import models, nn
from tests.parity_util import synth_ids

SEG_SHORT = 16            # csrc/embedding.hip
SEG_CHUNK = 16
SEG_HUGE = 256
SEG_LDS_MAX_B = 512
SEG_STAGE_B_MAX_WG = 1024
TWO_STAGE_MIN_B = 1024    # recsys_amd.ops.EmbeddingArena.TWO_STAGE_MIN_B

# the project's numbers for this comparison (tests/test_gpu_embedding.py test_segsum_bwd: rtol 2e-5; the absolute part as
# tests/test_gpu_tower_bn.py states it: 2e-7 of the tensor's largest reference magnitude, 1e-7 where that is exactly zero)
RTOL = 2e-5
ATOL_REL = 2e-7
ATOL_ZERO = 1e-7
MOMENT_EPS = 2.0 ** -22   # first-step moments: one rounding of the constant (1 - beta) and one multiply

# Bounds wider than the defaults for the KERNELS, per (case id, tensor), as a multiple of max|reference|: 4 x the figure of the
# float32 ascending-order restatement for that tensor and case (profiles/segsum_fp64_errors.txt) -- never taken from the kernels'
# own error.  Empty: the kernels are inside the default bounds in every tensor of every case.
LOOSER = {}
# Tensors whose float32 ascending-order RESTATEMENT is outside the default bounds although the kernels are inside them (a segment
# of ~370 entries whose sum nearly cancels in one element: the plain sequential float32 sum carries the rounding of every partial
# sum, the kernels add 16-entry chunk partials).  The restatement is held to 4 x its figure; the kernels keep the default bound.
#                                   restatement's figure (the kernels': profiles/segsum_fp64_errors.txt)
RESTATEMENT_OUTSIDE = {
    ("t1100x32-x-uniform", "G"): 6.02e-6,       # fp32 1.505e-06 (kernel 1.144e-07)
    ("t1100x32-x12-uniform", "G"): 3.04e-6,     # fp32 7.618e-07 (kernel 1.402e-07)
}


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def gpw_of(D):
    """unique rows per wave: 64 lanes / (D / 4 lanes per row)"""
    return 64 // (D // 4)


def seg_lds_bytes(B, D):
    idx4 = (3 * B + 4 + 3) // 4
    return (idx4 * 4 + 2 * B * D + 2 * B) * 4


def seg_lds_ok(B, D, two_stage):
    wpf = -(-B // gpw_of(D))
    return (not two_stage) and B <= SEG_LDS_MAX_B and wpf % 4 == 0 and seg_lds_bytes(B, D) <= 64 * 1024


def form_of(B, D):
    two = B > TWO_STAGE_MIN_B
    if two:
        return "two"
    return "lds" if seg_lds_ok(B, D, False) else "wave"


def seg_waves_per_field(B, gpw, two_stage):
    own = -(-B // gpw)
    return own + (B // (SEG_SHORT + 1) + gpw - 1) // gpw + B // (SEG_HUGE + 1) + 2 if two_stage else own


def stage_b_workgroups(B, D, F):
    """(uncapped, launched) workgroups of the stage-B / single-stage launch"""
    waves = F * seg_waves_per_field(B, gpw_of(D), B > TWO_STAGE_MIN_B)
    wgs = (waves + 3) // 4
    return wgs, (min(wgs, SEG_STAGE_B_MAX_WG) if B > TWO_STAGE_MIN_B else wgs)


def tile_positions(D):
    """sorted positions of one field per stage-A workgroup"""
    return (256 // (D // 4)) * SEG_CHUNK


def stage_b_units(ids, D):
    """wave-sized units of stage B's compact list (seg_units): per field ceil(nu / GPW) + ceil(nlong / GPW) + nhuge"""
    gpw, total = gpw_of(D), 0
    for f in range(ids.shape[1]):
        cnt = np.unique(ids[:, f], return_counts=True)[1]
        nl = int(((cnt > SEG_SHORT) & (cnt <= SEG_HUGE)).sum())
        total += -(-len(cnt) // gpw) + -(-nl // gpw) + int((cnt > SEG_HUGE).sum())
    return total


def segment_classes(ids, D):
    """What the drawn ids actually hold, as a set of tags:
      short / group / wave      a segment of <= 16 / 17..256 / > 256 entries
      edges                     segments of exactly 1, 16, 17, 256 and 257 entries
      slot1                     a 16-position chunk in which one long (> 16) segment ends and the next one starts right behind it
      mixed                     a chunk holding the end of a long segment, short segments, and the start of a long one
      tile                      a long segment crossing a stage-A position-tile boundary
      onerow                    a field whose whole batch is one segment
      spread / dealt            single stage: a field with unique rows <= / > its waves (ceil(B / GPW))
      spread_mid                a spread field with a segment of GPW < entries <= 16 (D >= 32): the cooperative walk would cut it
                                in sub-ranges of 2..4 entries, so it must be walked by its own lane group"""
    B, F = ids.shape
    tags, lens = set(), set()
    wpf, pos = -(-B // gpw_of(D)), tile_positions(D)
    for f in range(F):
        cnt = np.unique(ids[:, f], return_counts=True)[1]
        beg = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        end = beg + cnt
        lens |= set(cnt.tolist())
        tags |= {"short"} if (cnt <= SEG_SHORT).any() else set()
        tags |= {"group"} if ((cnt > SEG_SHORT) & (cnt <= SEG_HUGE)).any() else set()
        tags |= {"wave"} if (cnt > SEG_HUGE).any() else set()
        if len(cnt) == 1:
            tags.add("onerow")
        sp = len(cnt) <= wpf
        tags.add("spread" if sp else "dealt")
        if sp and ((cnt > gpw_of(D)) & (cnt <= SEG_SHORT)).any():
            tags.add("spread_mid")
        lg = np.flatnonzero(cnt > SEG_SHORT)
        for a, b in zip(lg[:-1], lg[1:]):                     # consecutive long segments of the field
            if end[a] % SEG_CHUNK != 0 and (end[a] - 1) // SEG_CHUNK == beg[b] // SEG_CHUNK:
                tags.add("slot1" if beg[b] == end[a] else "mixed")
        if (beg[lg] // pos != (end[lg] - 1) // pos).any():
            tags.add("tile")
    if {1, 16, 17, 256, 257} <= lens:
        tags.add("edges")
    return tags


# ------------------------------------------------------------------------------------------------ id generators
def zipf_ids(rng, B, rows, a=1.3):
    """[B, F] int32: a Zipf draw per field with the head on id 0"""
    return np.stack([((rng.zipf(a, B) - 1) % int(n)).astype(np.int32) for n in rows], 1)


def _fill(lengths, B, unit):
    """lengths + segments of `unit` entries (the last one shorter) up to B entries in all"""
    out, left = list(lengths), B - sum(lengths)
    assert left >= 0, (lengths, B)
    out += [unit] * (left // unit) + ([left % unit] if left % unit else [])
    return out


def layout_std(B, D):
    """Segment lengths per field, in sorted order, for a two-stage batch: the helper-group / helper-wave boundaries, two long
    segments sharing a chunk, a chunk with a long end + shorts + a long start, a long segment across the first tile boundary
    (where the batch has one), a one-row field, an all-distinct field."""
    pos = tile_positions(D)
    fields = [_fill([1, 16, 17, 256, 257], B, 3),
              _fill([40, 40], B, 5),                           # 0..39 | 40..79: chunk 2 holds the end of one and the start of the other
              _fill([40, 2, 1, 30, 300, 7, 19], B, 2),         # chunk 2: the end of 0..39, segments of 2 and 1, the start of 43..72
              [B],
              _fill([], B, 1)]
    if pos + 30 <= B:
        head = _fill([], pos - 100, 3)
        fields.append(head + _fill([min(300, B - (pos - 100))], B - sum(head), 4))   # pos - 100 .. pos + 199 (or the end of the batch)
    return fields


def layout_wide(B, D):
    """16 fields with (nearly) all-distinct ids: more stage-B units than 1024 workgroups hold waves"""
    return [_fill([], B, 1)] * 14 + [_fill([1, 16, 17, 256, 257], B, 1), _fill([40, 40], B, 1)]


LAYOUTS = {"std": layout_std, "wide": layout_wide}


def ids_from_lengths(rng, fields, B):
    """-> (ids [B, F] int32, rows per field).  Segment j of a field is id 2 j (so every other row stays untouched; a one-segment
    field has one row); a seeded permutation of the examples decides which b land where."""
    ids = np.zeros((B, len(fields)), np.int32)
    rows = []
    for f, lengths in enumerate(fields):
        assert sum(lengths) == B and min(lengths) > 0
        one = len(lengths) == 1
        ids[rng.permutation(B), f] = np.repeat(np.arange(len(lengths), dtype=np.int32) * (1 if one else 2), lengths)
        rows.append(1 if one else 2 * len(lengths) + 1)
    return ids, tuple(rows)


# ------------------------------------------------------------------------------------------------ the case table
# entry   bwd      EmbeddingArena.segsum (rsx_segsum_partials + rsx_segsum_bwd)
#         blocks   the same through rsx_example_blocks: 3 rank blocks of `blk` examples
#         packed   EmbeddingArena.ux_segsum_local (rsx_segsum_bwd_packed): output packed at goff
#         rows     SparseTable.finalize (rsx_segsum_partials + rsx_segsum_rows), F = 1, D = K, B = N entries
#         adam     EmbeddingArena.segsum_adam (rsx_segsum_adam_rows2): the gradient read back out of the first-step moments
# terms   which of dX ("x"), gy1 ("1"), gy2 ("2") are given
# ids     uniform (tests.parity_util.synth_ids) | zipf | std / wide (LAYOUTS; `rows` is then derived)
# null    rows entry: none | key (an ordinary key, 0) | dummy (null_row == rows, lookups with pad_id = 0)
# second  adam entry: a second table set sharing the sort
Case = namedtuple("Case", "id entry B D rows terms ids form expect blk null second seed")

SMALL_ROWS = (3, 7, 40, 11, 600, 1)
BIG_ROWS = (3, 1000, 50, 20000, 1)
TERMS = ("x", "x1", "x2", "x12", "2", "12")


def _cases():
    out = []

    def add(cid, entry, B, D, rows, terms, ids, form, expect, blk=0, null="none", second=False):
        out.append(Case(cid, entry, B, D, rows, terms, ids, form, frozenset(expect), blk, null, second, zlib.crc32(cid.encode())))

    # single stage.  lds: (256, 16) and (64, 64) have 16 waves per field; (442, 16) is the largest D = 16 batch the staging admits
    # (28 waves, 65 440 of 65 536 bytes).  wave: (443, 16) is refused by the staging SIZE alone (28 waves, 65 592 bytes), (432, 16)
    # and (200, 32) by their 27 / 25 waves, (300, 4) by its 5, (9, 64) by its 3, (520, 16) and (1024, 16) by B > 512.
    for B, D, form in ((256, 16, "lds"), (64, 64, "lds"), (442, 16, "lds"),
                       (300, 4, "wave"), (520, 16, "wave"), (1024, 16, "wave"), (9, 64, "wave"), (1, 16, "wave"),
                       (443, 16, "wave"), (432, 16, "wave"), (200, 32, "wave")):
        for t in TERMS:
            exp = {"short", "onerow"}
            if B >= 200:
                exp |= {"group", "spread", "dealt"}
            if D >= 32:
                exp |= {"spread_mid"}
            add("s%dx%d-%s" % (B, D, t), "bwd", B, D, SMALL_ROWS, t, "uniform", form, exp)
    # two stage: every (FM, W1) combination of segsum_tiles_k at every D, constructed and uniform ids, B rotating
    i = 0
    for D in (4, 8, 16, 32, 64):
        for t in ("x", "x1", "x2", "x12"):
            for kind in ("std", "uniform"):
                B = (1025, 1100, 2100)[i % 3]
                i += 1
                if kind == "std":
                    exp = {"short", "group", "wave", "edges", "slot1", "mixed", "onerow"}
                    if tile_positions(D) + 30 <= B:
                        exp.add("tile")
                else:
                    exp = {"short", "group", "wave", "onerow"}
                add("t%dx%d-%s-%s" % (B, D, t, kind), "bwd", B, D, BIG_ROWS if kind == "uniform" else None, t, kind, "two", exp)
    add("t1100x16-2-std", "bwd", 1100, 16, None, "2", "std", "two", {"short", "group", "wave", "slot1", "mixed"})
    add("t2100x16-12-zipf", "bwd", 2100, 16, (3, 1000, 50, 20000, 1), "12", "zipf", "two", {"short", "group", "wave"})
    # the stage-B grid at its cap (16 fields, D = 64, B = 1100: 1188 workgroups uncapped) with more units than the 4096 waves
    add("t1100x64-x1-wide", "bwd", 1100, 64, None, "x1", "wide", "two", {"short", "group", "wave", "edges", "slot1"})
    # rank-blocked inputs: 3 blocks of blk examples, B no multiple of blk
    add("b270x16-x12", "blocks", 270, 16, SMALL_ROWS, "x12", "uniform", "wave", {"short", "group"}, blk=100)
    add("b256x16-x1", "blocks", 256, 16, SMALL_ROWS, "x1", "uniform", "lds", {"short", "group"}, blk=100)
    add("b1100x16-x12", "blocks", 1100, 16, None, "x12", "std", "two", {"short", "group", "wave", "slot1", "mixed", "tile"}, blk=400)
    add("b1100x32-x", "blocks", 1100, 32, BIG_ROWS, "x", "uniform", "two", {"short", "group", "wave"}, blk=400)
    # packed output
    add("p300x16-x12", "packed", 300, 16, SMALL_ROWS, "x12", "uniform", "wave", {"short", "group"})
    add("p1100x16-x12", "packed", 1100, 16, None, "x12", "std", "two", {"short", "group", "wave", "slot1"})
    # SparseTable: N = 700 entries single stage, 1500 two stage
    for K in (4, 16, 32, 64):
        for N in (700, 1500):
            for null in ("none", "key", "dummy"):
                add("r%dx%d-%s" % (N, K, null), "rows", N, K, (300,), "x", "zipf", form_of(N, K), {"short", "group"}, null=null)
    # fused scatter + Adam
    for B, D, form in ((256, 16, "lds"), (300, 16, "wave"), (1100, 16, "two"), (64, 64, "lds"), (1100, 32, "two")):
        for t in ("x12", "x"):
            std = form == "two"
            add("a%dx%d-%s" % (B, D, t), "adam", B, D, None if std else SMALL_ROWS, t, "std" if std else "uniform", form,
                {"short", "group", "wave", "slot1", "mixed"} if std else {"short", "group"})
    add("a300x16-x12-second", "adam", 300, 16, SMALL_ROWS, "x12", "uniform", "wave", {"short", "group"}, second=True)
    add("a1100x16-x1-second", "adam", 1100, 16, None, "x1", "std", "two", {"short", "group", "wave"}, second=True)
    return out


CASES = _cases()
CASE = {c.id: c for c in CASES}
assert len(CASE) == len(CASES)


def ids_of(entry=None, form=None):
    return [c.id for c in CASES if (entry is None or c.entry == entry) and (form is None or c.form == form)]


ROWS_HEAD = 100           # rows entry: the first lookup (target items); the rest of the N entries is the history lookup


class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def draw(cid):
    """The case's inputs as float32 / int32 numpy arrays, a function of the case alone (shared: never written to).
    tables ~ 0.25 N(0,1), w1 ~ 0.1 N(0,1), dX / gy1 / gy2 ~ 1e-2 N(0,1): one entry's term is ~1e-2."""
    c = CASE[cid]
    rng = np.random.default_rng(c.seed)
    d = Inputs()
    B, D = c.B, c.D
    if c.ids in LAYOUTS:
        ids, rows = ids_from_lengths(rng, LAYOUTS[c.ids](B, D), B)
    else:
        rows = c.rows
        row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        ids = synth_ids(rng, B, row_off) if c.ids == "uniform" else zipf_ids(rng, B, rows)
    d.rows_per_field = tuple(int(r) for r in rows)
    d.row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    F, R = len(rows), int(d.row_off[-1])
    d.F, d.R = F, R
    d.tables = (rng.standard_normal((R, D)) * 0.25).astype(np.float32)
    d.w1 = (rng.standard_normal(R) * 0.1).astype(np.float32)
    d.dX = (rng.standard_normal((B, F * D)) * 1e-2).astype(np.float32) if "x" in c.terms else None
    d.gy1 = (rng.standard_normal(B) * 1e-2).astype(np.float32) if "1" in c.terms else None
    d.gy2 = (rng.standard_normal(B) * 1e-2).astype(np.float32) if "2" in c.terms else None
    d.dX2 = (rng.standard_normal((B, F * D)) * 1e-2).astype(np.float32) if c.second else None
    d.tables2 = (rng.standard_normal((R, D)) * 0.25).astype(np.float32) if c.second else None
    # a partial first-order mask: every field but the second and the last (the full one is (1 << F) - 1)
    d.mask_full = (1 << F) - 1
    d.mask_part = d.mask_full & ~(1 << 1) & ~(1 << (F - 1)) if F >= 3 else d.mask_full
    d.pad = None
    if c.entry == "rows":
        # entries [0, ROWS_HEAD): the target lookup, ids 0 among them; the rest: the history lookup, Zipf with its head on the
        # padding id 0.  key: EVERY entry of id 0 carries zeros (the contract of an explicit null key); dummy: the history's
        # padding entries only (they are keyed to the dummy row), the targets' id-0 entries are ordinary gradients of row 0
        ids[:5, 0] = 0
        pad = ids[:, 0] == 0
        if c.null == "dummy":
            pad[:ROWS_HEAD] = False
        if c.null != "none":
            d.dX[pad] = 0.0
            d.pad = pad
    d.ids = ids
    d.keys = ids.astype(np.int64) + d.row_off[None, :-1]          # global rows [B, F]
    if c.entry == "rows" and c.null == "dummy":
        d.keys = np.where(d.pad[:, None], R, d.keys)               # the dummy key one past the table
    return d


def field_sum_f32(d):
    """S as the CPU test takes it: the float32 field sum in ascending field order (oracle.models.gather_fm_fwd)"""
    S = np.zeros((d.ids.shape[0], d.tables.shape[1]), np.float32)
    for f in range(d.F):
        S = S + d.tables[np.minimum(d.keys[:, f], d.R - 1)]          # (the dummy key of a `rows` case: S is not used there)
    return S


# ------------------------------------------------------------------------------------------------ the references
def entry_terms(d, S, dtype=np.float64, dX=None, gy2="own", tables=None):
    """t [B, F, D] in `dtype` from the float32 inputs"""
    B, F = d.ids.shape
    T = (d.tables if tables is None else tables).astype(dtype)
    D = T.shape[1]
    dX = d.dX if dX is None else dX
    gy2 = d.gy2 if isinstance(gy2, str) else gy2
    t = np.zeros((B, F, D), dtype)
    if gy2 is not None:
        g = gy2.astype(dtype)[:, None, None]
        t = g * S.astype(dtype)[:, None, :] - g * T[np.minimum(d.keys, T.shape[0] - 1)]
    if dX is not None:
        t = t + dX.astype(dtype).reshape(B, F, D)
    return t


def ref64(d, S, mask=None, dX=None, gy2="own", gy1="own", tables=None, drop=None):
    """-> (G [R + 1, D], g1 [R + 1]) float64, dense over the rows (row R: the dummy key of a `rows` case; untouched rows 0).
    drop = (b, f): that one entry left out (the dropped-entry margin of test_segsum_ref_cpu.py)."""
    t = entry_terms(d, S, np.float64, dX, gy2, tables)
    keep = np.ones(d.keys.shape, bool)
    if drop is not None:
        keep[drop] = False
    G = np.zeros((d.R + 1, t.shape[2]))
    np.add.at(G, d.keys[keep], t[keep])
    g1 = np.zeros(d.R + 1)
    gy1 = d.gy1 if isinstance(gy1, str) else gy1
    if gy1 is not None:
        mask = d.mask_full if mask is None else mask
        for f in range(d.F):
            if (mask >> f) & 1:
                np.add.at(g1, d.keys[keep[:, f], f], gy1.astype(np.float64)[keep[:, f]])
    return G, g1


def oracle_sums(d, S, dtype=np.float32, mask=None, dX=None, gy2="own", gy1="own", tables=None):
    """The oracle's path (models.fm2_bwd, models._pairs_field_major, nn.segment_sum_rows): sums in ascending example order,
    multiply and add unfused, in `dtype` -- float32: the restatement whose bits the kernels promise for short segments.
    -> (uniq [U] global rows, G [U, D], g1 [U], entries per unique row [U])"""
    B, F = d.ids.shape
    T = (d.tables if tables is None else tables).astype(dtype)
    D = T.shape[1]
    dX = d.dX if dX is None else dX
    gy2 = d.gy2 if isinstance(gy2, str) else gy2
    gy1 = d.gy1 if isinstance(gy1, str) else gy1
    if gy2 is not None:
        dE = models.fm2_bwd(T[np.minimum(d.keys, T.shape[0] - 1)], S.astype(dtype), gy2.astype(dtype))
        if dX is not None:
            dE = dE + dX.astype(dtype).reshape(B, F, D)
    else:
        dE = dX.astype(dtype).reshape(B, F, D)
    r, v = models._pairs_field_major(d.keys, dE)
    uniq, G = nn.segment_sum_rows(r, v)
    cnt = np.bincount(np.searchsorted(uniq, r), minlength=len(uniq))
    g1 = np.zeros(len(uniq), dtype)
    if gy1 is not None:
        mask = d.mask_full if mask is None else mask
        _, g1 = nn.segment_sum_rows(*models._pairs_field_major(d.keys, np.repeat(gy1.astype(dtype)[:, None], F, 1)))
        fld = np.searchsorted(d.row_off, uniq, side="right") - 1
        g1 = np.where((mask >> np.minimum(fld, d.F - 1)) & 1 == 1, g1, dtype(0))
    return uniq, G, g1, cnt


def bound(ref, key=None, rtol=RTOL):
    """elementwise |got - ref| admitted for a tensor with reference `ref` (float64)"""
    m = float(np.abs(ref).max()) if ref.size else 0.0
    if key is not None and key in LOOSER:
        return rtol * np.abs(ref) + LOOSER[key] * m
    return rtol * np.abs(ref) + (ATOL_REL * m if m > 0.0 else ATOL_ZERO)


def figure(got, ref):
    """max|got - ref| / max|ref| (the absolute error where the reference is exactly zero)"""
    m = float(np.abs(ref).max()) if ref.size else 0.0
    e = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    return e / m if m > 0.0 else e


def exact_entries(c):
    """Segments of at most this many entries hold the bits of the float32 ascending-order restatement: 16 in every form
    (csrc/embedding.hip SEG_SHORT; two stages: a longer segment is by definition summed from chunk partials).  The single-stage
    rsx_segsum_rows launch also keeps them up to 64 / (K / 4) entries (tests/test_gpu_din.py: one entry per lane group, added in
    ascending order), which is more than 16 at K = 4."""
    if c.entry == "rows" and c.form != "two":
        return max(SEG_SHORT, gpw_of(c.D))
    return SEG_SHORT


def references(c, d, S, mask=None):
    """-> (uniq [U] global keys, entries per key [U], {tensor: (fp64 reference [U, ...], float32 restatement [U, ...])}):
    G, gw1 when gy1 is given, G2 (the second table set: dX2 alone) for a `second` case"""
    G64, g64 = ref64(d, S, mask)
    uniq, G32, g32, cnt = oracle_sums(d, S, np.float32, mask)
    out = {"G": (G64[uniq], G32)}
    if d.gy1 is not None:
        out["gw1"] = (g64[uniq], g32)
    if c.second:
        H64, _ = ref64(d, S, dX=d.dX2, gy2=None, gy1=None, tables=d.tables2)
        u2, H32, _, _ = oracle_sums(d, S, np.float32, dX=d.dX2, gy2=None, gy1=None, tables=d.tables2)
        assert np.array_equal(u2, uniq)
        out["G2"] = (H64[uniq], H32)
    return uniq, cnt, out
