"""The fused DIN attention MLP (csrc/din_attn.hip, called through the C ABI with raw pointers so that strides, offsets and entry
points are the test's) against a plain torch fp64 restatement, in every dispatch form of rsx_din_attn_fwd and attn_bwd_impl --
tests/din_attn_ref.py holds the case table (with the kernels each case was derived to take), the inputs and the reference;
tests/test_din_attn_ref_cpu.py checks the reference and the table's coverage without a GPU.

Compared per case, one assertion reporting every failing tensor: the forward's w, a1, a2; the backward's dH, dq and each of dW0,
db0, dW1, db1, dW2, db2 (so a wrong scale, which Adam's update hides from the model-level tests, fails here).  The backward is fed
the fp32 rounding of the fp64 forward's a1 / a2, so its gates (a > 0) are the reference's.  Bars: the project's numbers for this
comparison (tests/test_gpu_tower_bn.py, from tests/test_gpu_mlp_fused.py) -- rtol 1e-4 with atol 2e-7 * max|reference| of the
tensor (1e-7 absolute where the reference is exactly zero); for the `scaled` cases max|reference| of the per-example tensors is
taken per example.  Every comparison prints max|got - ref| / max|ref| next to the same figure of the restatement run in fp32
(profiles/din_attn_fp64_errors.txt is one run's table).  Every forward and every backward runs twice -- the backward from
NaN-filled workspaces -- and must repeat bit for bit: the file promises fixed-order sums."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import din_attn_ref as ar

pytestmark = pytest.mark.gpu

SENT = -777.25                                   # written to every output before a launch: what is not addressed keeps it
RTOL, ATOL_REL, ATOL_ZERO = 1e-4, 2e-7, 1e-7
PER_EXAMPLE = ("w", "a1", "a2", "dH", "dq")      # the tensors with one slice per example (`scaled`: compared slice by slice)
GRAD_NAMES = ("dW0", "db0", "dW1", "db1", "dW2", "db2")

# Bounds wider than the defaults, per (case, tensor), as a multiple of max|reference|: 4 x the figure of the fp32 torch restatement
# for that case and tensor (profiles/din_attn_fp64_errors.txt) -- never taken from the kernels' own error.  A factor 2 because the
# split products carry one rounding per product where an FMA chain carries none, a factor 2 for a different summation order over
# the maximum of thousands of elements.  Empty: in the recorded run every (case, tensor) is inside the default bars.
LOOSER = {
}


def _api():
    from recsys_amd.ops import _ptr, _stream, check, lib
    return lib(), _ptr, _stream, check


def _at(t, floats):
    """pointer `floats` floats behind t's first element"""
    return C.c_void_p(t.data_ptr() + 4 * floats)


def _placed(t, off, nan_rows=None):
    """A copy of t on the device, `off` floats into a sentinel-filled buffer (off = 1: not 16-byte aligned) -> (view, buffer)."""
    n = t.numel()
    buf = torch.full((n + 4,), SENT, device="cuda")
    v = buf[off:off + n].view(t.shape)
    v.copy_(t)
    if nan_rows is not None:
        v[nan_rows] = float("nan")
    assert v.data_ptr() % 16 == (4 * off) % 16 and buf.data_ptr() % 16 == 0
    return v, buf


def _slack_kept(v, buf):
    """the floats of the buffer around the placed view still hold the sentinel"""
    off = (v.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:off] == SENT).all()) and bool((buf[off + v.numel():] == SENT).all())


def _key(case):
    return case._replace(id="", a_off=False, w_off=False)


@functools.lru_cache(maxsize=3)
def _reference(key):
    """The case's inputs and forward references, built once per case (and shared by a case and its offset twin): fp64 and fp32
    forward on the device, and the fp32 rounding of the fp64 a1 / a2 that every backward is fed."""
    d = ar.draw(key)
    masks = ar.masks_of(key, d)
    with torch.no_grad():
        a1, a2, w = ar.forward_ref(d, masks, device="cuda")
        b1, b2, bw = ar.forward_ref(d, masks, dtype=torch.float32, device="cuda")
    assert bool((a1.float() > 0).eq(a1 > 0).all()) and bool((a2.float() > 0).eq(a2 > 0).all())    # fp32 rounding keeps the gates
    return dict(d=d, masks=masks, fwd=dict(a1=a1, a2=a2, w=w), fwd32=dict(a1=b1, a2=b2, w=bw), a1f=a1.float(), a2f=a2.float())


def _bwd_refs(R, **kw):
    """fp64 and fp32 backward references from the activations the kernel is fed"""
    with torch.no_grad():
        r64 = ar.backward_ref(R["d"], R["a1f"], R["a2f"], R["masks"], device="cuda", **kw)
        r32 = ar.backward_ref(R["d"], R["a1f"], R["a2f"], R["masks"], dtype=torch.float32, device="cuda", **kw)
    return r64, r32


class Inputs:
    """A case's inputs on the device: W0 / W1 one float into their buffers under w_off; H, q, dH and the masks always aligned (the
    kernels read H and q with 16-byte loads unconditionally).  drop == "hash": no mask buffers."""

    def __init__(self, case, R):
        d = R["d"]
        self.case = case
        for k in ("H", "q", "b0", "b1", "W2", "b2", "dw", "dH0", "dq_add"):
            setattr(self, k, d[k].cuda())
        off = 1 if case.w_off else 0
        (self.W0, self.W0buf), (self.W1, self.W1buf) = _placed(d["W0"], off), _placed(d["W1"], off)
        self.m = [m.cuda() for m in R["masks"]] if case.drop == "masks" else [None, None]
        self.step = torch.tensor([ar.RNG_STEP], dtype=torch.int32, device="cuda")
        self.a_off = 1 if case.a_off else 0
        self.ng = ar.n_grads(case)

    def act(self, src_or_n, nan_rows=None):
        """an a1 / a2 buffer (under a_off one float in): sentinel-filled [M, n], or a copy of `src` (NaN at nan_rows)"""
        M = self.case.B * self.case.P
        if isinstance(src_or_n, int):
            src_or_n = torch.full((M, src_or_n), SENT, device="cuda")
        return _placed(src_or_n, self.a_off, nan_rows)


def _fwd(x, rows=None, cnt=None, w=None):
    """One forward into sentinel-filled outputs -> dict a1, a2, w (and that nothing around a1 / a2 was written)."""
    L, _ptr, _stream, check = _api()
    c = x.case
    (a1, a1buf), (a2, a2buf) = x.act(c.N1), x.act(c.N2)
    w = torch.full((c.B * c.P,), SENT, device="cuda") if w is None else w.clone()
    check(L.rsx_din_attn_fwd(_ptr(x.H), _ptr(x.q), _ptr(x.W0), _ptr(x.b0), _ptr(x.W1), _ptr(x.b1), _ptr(x.W2), _ptr(x.b2), _ptr(a1),
                             _ptr(a2), _ptr(w), _ptr(x.m[0]), _ptr(x.m[1]), _ptr(x.step), ar.HASH_SEED, ar.LAYER0, c.rate, _ptr(rows),
                             _ptr(cnt), c.B, c.P, c.K, c.N1, c.N2, _stream()), "rsx_din_attn_fwd")
    torch.cuda.synchronize()
    assert _slack_kept(a1, a1buf) and _slack_kept(a2, a2buf), c.id
    return dict(a1=a1, a2=a2, w=w)


def _bwd(x, a1, a2, dw, entry="bwd", acc=False, add=False, rows=None, cnt=None, ids=None):
    """One backward from a NaN-filled workspace into sentinel-filled outputs.  entry "bwd": rsx_din_attn_bwd, dense dH / dq.
    entry "ld": rsx_din_attn_bwd_ld the way din.py's step addresses it -- dH = columns [K, 2K) of an [M, 2K] buffer, dq = columns
    [K, 2K) of a [B, 3K] buffer, dq_add = columns [2K, 3K) of another.  acc: accumulate_dH = 1 onto dH0.
    -> dict dH, dq, the six gradients, `grads` (the packed vector), `bufs` (every buffer written into, for identity checks)."""
    L, _ptr, _stream, check = _api()
    c = x.case
    B, P, K, M = c.B, c.P, c.K, c.B * c.P
    nan = float("nan")
    ws = torch.full((int(L.rsx_din_attn_bwd_workspace_floats(B, P, K, c.N1, c.N2)),), nan, device="cuda")
    gbuf = torch.full((x.ng + 64,), SENT, device="cuda")
    common = (_ptr(x.m[0]), _ptr(x.m[1]), _ptr(x.step), ar.HASH_SEED, ar.LAYER0, c.rate, int(acc), _ptr(rows), _ptr(cnt), _ptr(ids),
              B, P, K, c.N1, c.N2)
    ops = (_ptr(x.H), _ptr(x.q), _ptr(x.W0), _ptr(x.W1), _ptr(x.W2), _ptr(a1), _ptr(a2), _ptr(dw))
    if entry == "bwd":
        assert not add
        Hb = x.dH0.clone() if acc else torch.full((M, K), SENT, device="cuda")
        Qb = torch.full((B, K), SENT, device="cuda")
        check(L.rsx_din_attn_bwd(*ops, _ptr(Hb), _ptr(Qb), _ptr(gbuf), _ptr(ws), *common, _stream()), "rsx_din_attn_bwd")
        dH, dq = Hb, Qb
    else:
        Hb = torch.full((M, 2 * K), SENT, device="cuda")
        if acc:
            Hb[:, K:] = x.dH0
        Qb = torch.full((B, 3 * K), SENT, device="cuda")
        Ab = torch.full((B, 3 * K), nan, device="cuda")
        Ab[:, 2 * K:] = x.dq_add
        check(L.rsx_din_attn_bwd_ld(*ops, _at(Hb, K), _at(Qb, K), _ptr(gbuf), _ptr(ws), *common, 2 * K, 3 * K,
                                    _at(Ab, 2 * K) if add else None, 3 * K, _stream()), "rsx_din_attn_bwd_ld")
        dH, dq = Hb[:, K:], Qb[:, K:2 * K]
    torch.cuda.synchronize()
    out = dict(dH=dH, dq=dq, grads=gbuf[:x.ng], bufs=(Hb, Qb, gbuf))
    for name, (o, shape) in ar.grad_slices(c).items():
        out[name] = gbuf[o:o + int(np.prod(shape))].view(shape)
    # every float outside the addressed blocks keeps its sentinel: the tail of grads, the other columns of the wide buffers
    assert bool((gbuf[x.ng:] == SENT).all()), c.id
    if entry == "ld":
        assert bool((Hb[:, :K] == SENT).all()) and bool((Qb[:, :K] == SENT).all()) and bool((Qb[:, 2 * K:] == SENT).all()), c.id
    return out


def _same(a, b):
    """bit-identical, NaN included (sentinels and untouched rows compare equal to themselves)"""
    return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


def _compare(cid, tag, pairs, B=None):
    """pairs of (name, got, fp64 reference, fp32 restatement): prints the error table, -> the list of misses.  B: compare the
    per-example tensors example by example (max|reference| over THAT example's slice)."""
    bad = []
    for name, got, ref, ref32 in pairs:
        rows = B if (B is not None and name in PER_EXAMPLE) else 1
        g, r, r32 = got.double().reshape(rows, -1), ref.double().reshape(rows, -1), ref32.double().reshape(rows, -1)
        assert g.shape == r.shape and g.numel() > 0, (tag, name)
        m = r.abs().amax(1, keepdim=True)
        den = torch.where(m > 0, m, torch.ones_like(m))
        err = (g - r).abs()
        fig = float((err.amax(1, keepdim=True) / den).max())
        fig32 = float(((r32 - r).abs().amax(1, keepdim=True) / den).max())
        print("DIN_ATTN_ERR %-26s %-4s kernel %.3e  fp32-torch %.3e" % (tag, name, fig, fig32))
        if (cid, name) in LOOSER:
            atol = LOOSER[(cid, name)] * m
        else:
            atol = torch.where(m > 0, ATOL_REL * m, torch.full_like(m, ATOL_ZERO))
        miss = ~(err <= atol + RTOL * r.abs())            # (a NaN or an infinity in `got` misses)
        if bool(miss.any()):
            worst = int((err - atol - RTOL * r.abs()).nan_to_num(nan=float("inf")).argmax())
            bad.append("%s %s: %d of %d elements outside rtol %g + atol; figure %.3e (fp32-torch %.3e); worst at flat index %d: got %r, "
                       "reference %r" % (tag, name, int(miss.sum()), g.numel(), RTOL, fig, fig32, worst, float(g.reshape(-1)[worst]),
                                         float(r.reshape(-1)[worst])))
    for b in bad:
        print("DIN_ATTN_FAIL " + b)
    return bad


def _fwd_pairs(got, R, sel=None):
    s = (lambda t: t) if sel is None else (lambda t: t[sel])
    return [(k, s(got[k]), s(R["fwd"][k]), s(R["fwd32"][k])) for k in ("w", "a1", "a2")]


def _bwd_pairs(got, r64, r32, sel=None):
    s = (lambda t: t) if sel is None else (lambda t: t[sel])
    return [("dH", s(got["dH"]), s(r64["dH"]), s(r32["dH"])), ("dq", got["dq"], r64["dq"], r32["dq"])] + \
           [(k, got[k], r64[k], r32[k]) for k in GRAD_NAMES]


@pytest.mark.parametrize("cid", [c.id for c in ar.CASES])
def test_forward_and_backward_match_fp64(cid):
    """rsx_din_attn_fwd and rsx_din_attn_bwd over the whole case table; the "hash" cases pass no mask buffers and are compared
    with the host's restatement of the hash (seed, step 7, layers 2 and 3, element m * N + n): an exact-pattern test."""
    case = ar.CASE[cid]
    print("DIN_ATTN_FORMS %-18s %s" % (cid, "; ".join(ar.forms(case))))
    R = _reference(_key(case))
    x = Inputs(case, R)
    per = case.B if case.scaled else None
    f, f2 = _fwd(x), _fwd(x)
    assert _same([f[k] for k in ("w", "a1", "a2")], [f2[k] for k in ("w", "a1", "a2")]), "the forward does not repeat bit for bit"
    bad = _compare(cid, cid, _fwd_pairs(f, R), per)
    (a1, _), (a2, _) = x.act(R["a1f"]), x.act(R["a2f"])
    b, b2 = _bwd(x, a1, a2, x.dw), _bwd(x, a1, a2, x.dw)
    assert _same(b["bufs"], b2["bufs"]), "the backward does not repeat bit for bit"
    bad += _compare(cid, cid, _bwd_pairs(b, *_bwd_refs(R)), per)
    assert not bad, "\n".join(bad)


def _row_list(case, ids):
    """rsx_din_valid_rows -> rows, count (views of one buffer, as ops.py lays them out), w zeroed at the padded positions"""
    L, _ptr, _stream, check = _api()
    M = case.B * case.P
    rows = torch.full((M + 2 + (M + 1023) // 1024,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((M,), SENT, device="cuda")
    check(L.rsx_din_valid_rows(_ptr(ids), case.B, case.P, _ptr(rows), _ptr(rows[M:]), _ptr(w), _stream()), "rsx_din_valid_rows")
    torch.cuda.synchronize()
    return rows, rows[M:], w


@pytest.mark.parametrize("mode", ar.ID_MODES)
@pytest.mark.parametrize("cid", ar.LIST_CASES)
def test_row_list_skips_padding_and_tolerates_anything_there(cid, mode):
    """The row list (rows / count / ids) at count 0, 1, M and with padding anywhere.  Forward: the listed rows equal the reference,
    every other row of a1 / a2 keeps its sentinel and w the 0 rsx_din_valid_rows wrote.  Backward: a1, a2 and dw hold NaN at every
    row NOT in the list and the workspace is NaN throughout (the header comment: the skipped rows "may hold anything") -- every
    output must be finite and equal the reference; dH outside the list keeps its sentinel (dH0 under accumulate_dH); dq of an
    all-padding example is exactly 0 (exactly dq_add[b]).  Through rsx_din_attn_bwd and, with accumulate_dH and dq_add, through
    rsx_din_attn_bwd_ld at din.py's strides."""
    case = ar.CASE[cid]
    R = _reference(_key(case))
    x = Inputs(case, R)
    ids = ar.draw_ids(case, mode).cuda()
    valid = ids.reshape(-1) > 0
    count = int(valid.sum())
    rows, cnt, w0 = _row_list(case, ids)
    assert int(cnt[0]) == count and torch.equal(rows[:count].long(), torch.nonzero(valid).reshape(-1))
    bad = []
    # ---- forward
    f, f2 = _fwd(x, rows, cnt, w0), _fwd(x, rows, cnt, w0)
    assert _same([f[k] for k in ("w", "a1", "a2")], [f2[k] for k in ("w", "a1", "a2")])
    assert bool((f["a1"][~valid] == SENT).all()) and bool((f["a2"][~valid] == SENT).all()) and bool((f["w"][~valid] == 0).all())
    if count:
        bad += _compare(cid, "%s/%s" % (cid, mode), _fwd_pairs(f, R, valid))
    # ---- backward
    (a1, _), (a2, _) = x.act(R["a1f"], ~valid), x.act(R["a2f"], ~valid)
    dw = x.dw.clone()
    dw[~valid] = float("nan")
    allpad = torch.nonzero(~(ids > 0).any(1)).reshape(-1)
    assert mode == "full" or len(allpad) >= 1
    for entry, acc in (("bwd", False), ("ld", True)):
        kw = dict(entry=entry, acc=acc, add=acc, rows=rows, cnt=cnt, ids=ids)
        b, b2 = _bwd(x, a1, a2, dw, **kw), _bwd(x, a1, a2, dw, **kw)
        assert _same(b["bufs"], b2["bufs"]), "the backward does not repeat bit for bit"
        tag = "%s/%s/%s" % (cid, mode, entry)
        for k in ("dq", "grads"):
            assert bool(torch.isfinite(b[k]).all()), (tag, k)
        r64, r32 = _bwd_refs(R, ids=ids, accumulate_dH=acc, dq_add=acc)
        keep = x.dH0 if acc else torch.full_like(x.dH0, SENT)
        assert torch.equal(b["dH"][~valid], keep[~valid]), tag + ": dH outside the list was written"
        want_q = x.dq_add if acc else torch.zeros_like(x.dq_add)
        assert torch.equal(b["dq"][allpad], want_q[allpad]), tag + ": dq of an all-padding example"
        pairs = _bwd_pairs(b, r64, r32, valid)
        bad += _compare(cid, tag, pairs if count else pairs[1:])
        if mode == "zero":          # every workgroup writes a zero partial even when it walks no block
            assert bool((b["grads"] == 0).all()) and torch.equal(b["dq"], want_q), tag
        if mode == "full" and entry == "bwd":       # the list of every row against no list
            u = _bwd(x, a1, a2, dw)
            bad += _compare(cid, tag + "/vs-unlisted", [(n_, got, u[n_], ref32) for n_, got, _, ref32 in pairs])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("defer", [False, True], ids=["finish_pair", "finish_pair_defer"])
def test_nofinish_twice_then_one_finish_for_both_blocks(defer):
    """din.py's fused TRAIN step: rsx_din_attn_bwd_nofinish for each of the two attention blocks (accumulate_dH = 1, ld_dH = 2K,
    a row list), then ONE rsx_din_attn_finish_pair (ld_dq = 2K; dq_add with ld 3K for block 0, none for block 1) -- or
    rsx_din_attn_finish_pair_defer with a reduce_out array followed by rsx_vec_reduce_run on the two returned jobs.  The two blocks
    get DIFFERENT inputs, weights included: each block's gradients must equal ITS reference, so a swap of the two sets fails."""
    from recsys_amd import _lib
    L, _ptr, _stream, check = _api()
    base = ar.CASE["r1237"]
    B, P, K, M = base.B, base.P, base.K, base.B * base.P
    nan = float("nan")
    Qb = torch.full((B, 2 * K), SENT, device="cuda")         # block t's dq = columns [t K, (t + 1) K)
    sets = []
    for t in range(2):
        case = base._replace(id="r1237/blk%d" % t, seed=base.seed + t)
        R = _reference(_key(case))
        x = Inputs(case, R)
        ids = ar.draw_ids(case, "anywhere").cuda()
        valid = ids.reshape(-1) > 0
        rows, cnt, _ = _row_list(case, ids)
        (a1, _), (a2, _) = x.act(R["a1f"], ~valid), x.act(R["a2f"], ~valid)
        dw = x.dw.clone()
        dw[~valid] = nan
        ws = torch.full((int(L.rsx_din_attn_bwd_workspace_floats(B, P, K, case.N1, case.N2)),), nan, device="cuda")
        Hb = torch.full((M, 2 * K), SENT, device="cuda")
        Hb[:, K:] = x.dH0
        check(L.rsx_din_attn_bwd_nofinish(_ptr(x.H), _ptr(x.q), _ptr(x.W0), _ptr(x.W1), _ptr(x.W2), _ptr(a1), _ptr(a2), _ptr(dw),
                                          _at(Hb, K), _ptr(ws), _ptr(x.m[0]), _ptr(x.m[1]), _ptr(x.step), ar.HASH_SEED, 2 * t, case.rate,
                                          1, _ptr(rows), _ptr(cnt), _ptr(ids), B, P, K, case.N1, case.N2, 2 * K, _stream()),
              "rsx_din_attn_bwd_nofinish")
        gbuf = torch.full((x.ng + 64,), SENT, device="cuda")
        Ab = torch.full((B, 3 * K), nan, device="cuda")
        Ab[:, :K] = x.dq_add
        sets.append(dict(case=case, R=R, x=x, ids=ids, valid=valid, ws=ws, Hb=Hb, gbuf=gbuf, Ab=Ab, keep=(a1, a2, dw, rows)))
    s0, s1 = sets
    args = (_ptr(s0["ws"]), _ptr(s0["gbuf"]), _at(Qb, 0), _ptr(s0["ids"]), _ptr(s0["Ab"]),
            _ptr(s1["ws"]), _ptr(s1["gbuf"]), _at(Qb, K), _ptr(s1["ids"]), None, B, P, K, base.N1, base.N2, 2 * K, 3 * K)
    if defer:
        jobs = (_lib.VecReduceJob * 2)()
        check(L.rsx_din_attn_finish_pair_defer(*args, jobs, _stream()), "rsx_din_attn_finish_pair_defer")
        torch.cuda.synchronize()
        for t in range(2):          # the launch kept the query sums only: the weight gradients come back as jobs
            assert jobs[t].n == sets[t]["x"].ng and jobs[t].G == min((M + 63) // 64, 256) and jobs[t].out == sets[t]["gbuf"].data_ptr()
            assert bool((sets[t]["gbuf"] == SENT).all())
        check(L.rsx_vec_reduce_run(jobs, 2, _stream()), "rsx_vec_reduce_run")
    else:
        check(L.rsx_din_attn_finish_pair(*args, _stream()), "rsx_din_attn_finish_pair")
    torch.cuda.synchronize()
    bad = []
    for t, s in enumerate(sets):
        x, valid = s["x"], s["valid"]
        got = dict(dH=s["Hb"][:, K:], dq=Qb[:, t * K:(t + 1) * K], grads=s["gbuf"][:x.ng])
        for name, (o, shape) in ar.grad_slices(s["case"]).items():
            got[name] = s["gbuf"][o:o + int(np.prod(shape))].view(shape)
        assert bool((s["gbuf"][x.ng:] == SENT).all()) and bool((s["Hb"][:, :K] == SENT).all())
        assert bool(torch.isfinite(got["dq"]).all()) and bool(torch.isfinite(got["grads"]).all()), t
        assert torch.equal(got["dH"][~valid], x.dH0[~valid])
        r64, r32 = _bwd_refs(s["R"], ids=s["ids"], accumulate_dH=True, dq_add=(t == 0))
        bad += _compare("r1237", "r1237/%s/blk%d" % ("defer" if defer else "pair", t), _bwd_pairs(got, r64, r32, valid))
    assert not bad, "\n".join(bad)


def test_invalid_strides_and_lists_stay_refused():
    """the argument checks the entry points above rely on (codes only: nothing is launched, the pointers are never read)"""
    L, _, _, _ = _api()
    Pn, u32 = C.c_void_p(0x1000), C.c_uint32
    ptrs = [Pn] * 12 + [None, None, Pn]
    ld = lambda rows, count, ids, ld_dH, ld_dq, add, ld_add: L.rsx_din_attn_bwd_ld(
        *ptrs, u32(1), 0, 0.0, 0, rows, count, ids, 4, 10, 32, 80, 40, ld_dH, ld_dq, add, ld_add, None)
    assert ld(None, None, None, 31, 32, None, 0) == -1          # ld_dH < K
    assert ld(None, None, None, 32, 31, None, 0) == -1          # ld_dq < K
    assert ld(None, None, None, 32, 32, Pn, 31) == -1           # ld_dq_add < K
    assert ld(Pn, Pn, None, 32, 32, None, 0) == -1              # a list without the ids it was made from
    assert ld(Pn, None, Pn, 32, 32, None, 0) == -1              # rows without count
    assert L.rsx_din_attn_bwd_nofinish(*([Pn] * 10), None, None, Pn, u32(1), 0, 0.0, 0, Pn, Pn, None, 4, 10, 32, 80, 40, 64, None) == -1
    assert L.rsx_din_attn_bwd_nofinish(*([Pn] * 10), None, None, Pn, u32(1), 0, 0.0, 0, None, None, None, 4, 10, 32, 80, 40, 31, None) == -1
