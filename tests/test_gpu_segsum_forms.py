"""The sorted segment-sum (csrc/embedding.hip: rsx_segsum_partials, rsx_segsum_bwd, rsx_segsum_bwd_packed, rsx_segsum_rows,
rsx_segsum_adam_rows2) against a plain fp64 sum, in every dispatch form -- tests/segsum_ref.py holds the case table (with the
form each case was derived to take), the id generators and the references; tests/test_segsum_ref_cpu.py checks the references,
every case's form and segment classes and the margins without a GPU.

Compared per case at slot[uniq]: G and gw1; for the fused scatter + Adam launch the gradient read back out of the first-step
moments (zero state: m = (1 - beta1) g, v = (1 - beta2) g g) -- the variables after TF-1 Adam's first step move by ~lr * sign(g)
whatever |g| is, so only the moments see a wrong sum.

Bounds (tests/segsum_ref.py): rtol 2e-5 with atol = 2e-7 x max|reference| of the tensor (1e-7 where the reference is exactly
zero); + 2^-22 relative for m (one rounding of the constant, one multiply); for v the bound of g carried through the square,
2 |g| bound(g) + bound(g)^2, + 2^-22 relative.  ONE dropped or doubled entry is ~1e-2 in these inputs: three orders of
magnitude above any of these bounds (test_segsum_ref_cpu.py asserts > 100 x for the longest segment of every case), and that
is the property the bounds have to keep.  Segments of at most 16 entries (segsum_ref.exact_entries) must hold the
BITS of the float32 ascending-order restatement.  Every comparison prints
    SEGSUM_ERR <case> <tensor> kernel <max|got - ref| / max|ref|> fp32 <the same figure of the float32 restatement>
(profiles/segsum_fp64_errors.txt is one run's table)."""
import numpy as np
import pytest

from tests import segsum_ref as sr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAN = float("nan")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _arena(d, D, cap, mask=None, tables=None):
    from recsys_amd.ops import EmbeddingArena
    return EmbeddingArena(d.row_off, D, cap, "cuda", with_w1=True, w1_field_mask=mask,
                          tables=d.tables if tables is None else tables, w1=d.w1)


def _sorted_arena(c, d, cap, mask=None):
    """arena with the case's ids sorted -> (arena, ids on the device, S of the kernel's own gather or None)"""
    a = _arena(d, c.D, cap, mask)
    idt = _t(d.ids)
    a.field_sort(idt)
    S = a.gather(idt, fm=True, first_order=False)[1] if d.gy2 is not None else None
    return a, idt, S


def _check_slots(a, uniq, R):
    slot = a.slot.cpu().numpy()[:R]
    assert (slot[uniq] >= 0).all() and int((slot >= 0).sum()) == len(uniq) == int(a.nuniq.sum())
    return slot[uniq]


class Report:
    """The comparisons of one case: prints the error table, collects the misses."""

    def __init__(self, c):
        self.c, self.bad = c, []

    def sums(self, name, got, r64, r32, cnt, tag=""):
        """got [U, ...] against the fp64 reference and, on short segments, the bits of the float32 restatement"""
        c = self.c
        got = got.reshape(r64.shape)
        print("SEGSUM_ERR %-22s %-5s kernel %.3e fp32 %.3e" % (c.id + tag, name, sr.figure(got, r64), sr.figure(r32, r64)))
        err = np.abs(got.astype(np.float64) - r64)
        if not np.isfinite(got).all() or (err > sr.bound(r64, (c.id, name))).any():
            i = np.unravel_index(np.nanargmax(np.where(np.isfinite(err), err, np.inf)), err.shape)
            self.bad.append("%s%s %s: |got - ref| = %.3e at %s (ref %.6e, %d entries), bound %.3e" % (
                c.id, tag, name, err[i], i, r64[i], cnt[i[0]], sr.bound(r64, (c.id, name))[i]))
        short = cnt <= sr.exact_entries(c)
        assert short.any()
        if not np.array_equal(got[short], r32[short]):
            k = np.flatnonzero((got[short] != r32[short]).reshape(int(short.sum()), -1).any(1))
            self.bad.append("%s%s %s: %d of %d segments of <= %d entries differ from the float32 ascending-order sums "
                            "(entries of the first ones: %s)" % (c.id, tag, name, len(k), int(short.sum()), sr.exact_entries(c),
                                                               cnt[short][k][:8].tolist()))

    def done(self):
        for b in self.bad:
            print("SEGSUM_FAIL " + b)
        assert not self.bad, "\n".join(self.bad)


def _segsum(a, c, d, S, blocks=None, bufs=None):
    """one EmbeddingArena.segsum into NaN-filled outputs -> (G, gw1) as host copies"""
    a.G.fill_(NAN)
    a.gw1.fill_(NAN)
    dX, gy1, gy2 = bufs if bufs is not None else (_t(d.dX), _t(d.gy1), _t(d.gy2))
    a.segsum(c.B, S, dX, gy1, gy2, blocks=blocks)
    torch.cuda.synchronize()
    return a.G.cpu().numpy(), a.gw1.cpu().numpy()


@pytest.mark.parametrize("cid", sr.ids_of("bwd"))
def test_segsum_matches_fp64(cid):
    """rsx_segsum_partials + rsx_segsum_bwd.  Also: a second call returns the same bits; capacity B + 3 with a partial
    w1_field_mask returns the same G bits, the masked reference's gw1, and on the fields inside the mask the same gw1 bits."""
    c, d = sr.CASE[cid], sr.draw(cid)
    a, idt, S = _sorted_arena(c, d, c.B)
    G, gw1 = _segsum(a, c, d, S)
    Sn = None if S is None else S.cpu().numpy()
    uniq, cnt, refs = sr.references(c, d, Sn)
    sl = _check_slots(a, uniq, d.R)
    rep = Report(c)
    rep.sums("G", G[sl], *refs["G"], cnt)
    if d.gy1 is not None:
        rep.sums("gw1", gw1[sl], *refs["gw1"], cnt)
    G2, gw2 = _segsum(a, c, d, S)
    assert np.array_equal(G2[sl], G[sl]) and (d.gy1 is None or np.array_equal(gw2[sl], gw1[sl]))       # deterministic
    # capacity != B, partial mask
    b, idt, Sb = _sorted_arena(c, d, c.B + 3, d.mask_part)
    assert S is None or torch.equal(S, Sb)
    Gb, gwb = _segsum(b, c, d, Sb)
    slb = _check_slots(b, uniq, d.R)
    assert np.array_equal(Gb[slb], G[sl]), "capacity B + 3: other G bits"
    if d.gy1 is not None:
        _, _, refs_m = sr.references(c, d, Sn, d.mask_part)
        rep.sums("gw1", gwb[slb], *refs_m["gw1"], cnt, tag="/mask")
        fld = np.searchsorted(d.row_off, uniq, side="right") - 1
        on = ((d.mask_part >> fld) & 1) == 1
        assert np.array_equal(gwb[slb][on], gw1[sl][on]) and not gwb[slb][~on].any()
    rep.done()


def _blocked(c, d, S):
    """The inputs as dist.DataParallel.gather_example_grads(blocked=True) leaves them: rank block r = [dX | S | gy2 | gy1] of its
    blk examples back to back (sections at multiples of 4 floats), blocks Lp floats apart, NaN wherever no example lives.
    -> (dX, S, gy1, gy2 views of block 0, (blk, Lp), the buffer)"""
    blk, B = c.blk, c.B
    parts = [("dX", d.dX.reshape(B, -1))]
    if d.gy2 is not None:
        parts += [("S", S.cpu().numpy()), ("gy2", d.gy2.reshape(B, 1))]
    if d.gy1 is not None:
        parts += [("gy1", d.gy1.reshape(B, 1))]
    L = sum(blk * p.shape[1] for _, p in parts)
    Lp = ((L + 3) & ~3) + 8                                   # (a dense-gradient tail rides behind the example block)
    nb = -(-B // blk)
    host = np.full((nb, Lp), np.nan, np.float32)
    off, o = {}, 0
    for name, p in parts:
        assert o % 4 == 0
        off[name] = (o, blk * p.shape[1])
        for r in range(nb):
            rows = p[r * blk:min((r + 1) * blk, B)]
            host[r, o:o + rows.size] = rows.reshape(-1)
        o += blk * p.shape[1]
    buf = torch.from_numpy(host).cuda()
    view = lambda n: buf[0, off[n][0]:off[n][0] + off[n][1]] if n in off else None
    return view("dX"), view("S"), view("gy1"), view("gy2"), (blk, Lp), buf


@pytest.mark.parametrize("cid", sr.ids_of("blocks"))
def test_rank_blocked_inputs_match_fp64_and_the_contiguous_bits(cid):
    """rsx_example_blocks: 3 rank blocks, the last one partly filled.  Same association as the contiguous launch, so the same
    bits; one block holding the whole batch (examples >= B) IS the contiguous launch."""
    c, d = sr.CASE[cid], sr.draw(cid)
    a, idt, S = _sorted_arena(c, d, c.B)
    G, gw1 = _segsum(a, c, d, S)
    Sn = None if S is None else S.cpu().numpy()
    uniq, cnt, refs = sr.references(c, d, Sn)
    sl = _check_slots(a, uniq, d.R)
    dXv, Sv, g1v, g2v, blocks, buf = _blocked(c, d, S)
    Gk, gwk = _segsum(a, c, d, Sv, blocks=blocks, bufs=(dXv, g1v, g2v))
    rep = Report(c)
    rep.sums("G", Gk[sl], *refs["G"], cnt)
    if d.gy1 is not None:
        rep.sums("gw1", gwk[sl], *refs["gw1"], cnt)
    rep.done()
    assert np.array_equal(Gk[sl], G[sl]) and (d.gy1 is None or np.array_equal(gwk[sl], gw1[sl]))
    G1, gw1b = _segsum(a, c, d, S, blocks=(c.B + 5, 8))
    assert np.array_equal(G1[sl], G[sl]) and (d.gy1 is None or np.array_equal(gw1b[sl], gw1[sl]))
    Gk2, _ = _segsum(a, c, d, Sv, blocks=blocks, bufs=(dXv, g1v, g2v))
    assert np.array_equal(Gk2[sl], Gk[sl])                                                          # deterministic


@pytest.mark.parametrize("cid", sr.ids_of("packed"))
def test_packed_output_matches_fp64_at_the_packed_offsets(cid):
    """rsx_segsum_bwd_packed through EmbeddingArena.ux_segsum_local: unique row j of field f at row goff[f] + j of the block."""
    c, d = sr.CASE[cid], sr.draw(cid)
    a = _arena(d, c.D, 2 * c.B)
    ux = a.enable_unique_exchange(2, c.B)
    loc, goff = ux.local, ux.goff_np
    assert loc.stride == c.B and loc._two_stage(c.B) == (c.form == "two")
    idt = _t(d.ids)
    a.ux_sort_pack([idt])
    S = a.gather(idt, fm=True, first_order=False)[1] if d.gy2 is not None else None
    uniq, cnt, refs = sr.references(c, d, None if S is None else S.cpu().numpy())
    outs = []
    for rep_ in range(2):
        G_out = torch.full((ux.capT, c.D), NAN, device="cuda")
        gw_out = torch.full((ux.capT,), NAN, device="cuda")
        a.ux_segsum_local(c.B, S, _t(d.dX), _t(d.gy1), _t(d.gy2), G_out, gw_out)
        torch.cuda.synchronize()
        outs.append((G_out.cpu().numpy(), gw_out.cpu().numpy()))
    nu = loc.nuniq.cpu().numpy()
    ur = loc.uniq_row.cpu().numpy().reshape(d.F, loc.stride)
    assert np.array_equal(np.concatenate([ur[f, :nu[f]] for f in range(d.F)]), uniq)
    at = np.concatenate([goff[f] + np.arange(nu[f]) for f in range(d.F)])
    assert (nu <= np.diff(goff)).all()
    rep = Report(c)
    rep.sums("G", outs[0][0][at], *refs["G"], cnt)
    rep.sums("gw1", outs[0][1][at], *refs["gw1"], cnt)
    rep.done()
    assert np.array_equal(outs[0][0][at], outs[1][0][at]) and np.array_equal(outs[0][1][at], outs[1][1][at])
    rest = np.ones(ux.capT, bool)
    rest[at] = False
    assert np.isnan(outs[0][0][rest]).all()                  # nothing written outside the fields' unique rows


@pytest.mark.parametrize("cid", sr.ids_of("rows"))
def test_sparse_table_sums_match_fp64(cid):
    """rsx_segsum_rows through SparseTable: two lookups (targets, then a Zipf history whose head is the padding id 0), null_row
    none / an ordinary key / the dummy key one past the table (lookup(..., pad_id=0))."""
    from recsys_amd.ops import SparseTable
    c, d = sr.CASE[cid], sr.draw(cid)
    N, K, R, H = c.B, c.D, d.R, sr.ROWS_HEAD
    null_key = {"none": -1, "key": 0, "dummy": R}[c.null]
    tbl = SparseTable(R, K, N + 3, table=d.tables, null_row=null_key)
    uniq, cnt, refs = sr.references(c, d, None)
    t1, t2 = _t(d.ids[:H, 0]), _t(d.ids[H:, 0])
    g1, g2 = _t(d.dX[:H]), _t(d.dX[H:])
    outs = []
    for rep_ in range(2):
        tbl.G.fill_(NAN)
        r1, r2 = tbl.lookup(t1), tbl.lookup(t2, pad_id=0 if c.null == "dummy" else None)
        assert torch.equal(r2.detach(), tbl.table[t2.long()])
        ((r1 * g1).sum() + (r2 * g2).sum()).backward()
        tbl.finalize()
        torch.cuda.synchronize()
        U = int(tbl.nuniq.item())
        assert U == len(uniq) and np.array_equal(tbl.uniq_row.cpu().numpy()[:U], uniq)
        slot = tbl.slot.cpu().numpy()[:R + 1]
        assert np.array_equal(np.flatnonzero(slot >= 0), uniq) and np.array_equal(slot[uniq], np.arange(U))
        outs.append(tbl.G.cpu().numpy()[:U])
    rep = Report(c)
    rep.sums("G", outs[0], *refs["G"], cnt)
    rep.done()
    assert np.array_equal(outs[0], outs[1])                                                         # deterministic
    if c.null != "none":
        k = int(np.searchsorted(uniq, null_key))
        assert uniq[k] == null_key and cnt[k] == cnt.max() and not outs[0][k].any()     # the longest segment; its sum exactly zero
    if c.null == "dummy":      # the real row 0 keeps the gradients of the lookup that declared no padding
        assert uniq[0] == 0 and cnt[0] >= 5 and np.abs(refs["G"][0][0]).max() > 1e-3


def _moments(rep, name, m, v, r64, r32, cnt, omb1, omb2):
    """first-step moments [U, ...] of rows whose summed gradient is r64 (fp64) / r32 (float32 restatement)"""
    c = rep.c
    m, v = m.reshape(r64.shape), v.reshape(r64.shape)
    g_back = m.astype(np.float64) / float(omb1)
    v_back = v.astype(np.float64) / float(omb2)
    bg = sr.bound(r64, (c.id, name))
    em, ev = np.abs(g_back - r64), np.abs(v_back - r64 * r64)
    print("SEGSUM_ERR %-22s %-5s kernel %.3e fp32 %.3e" % (c.id, "m/" + name, sr.figure(g_back, r64), sr.figure(r32, r64)))
    print("SEGSUM_ERR %-22s %-5s kernel %.3e fp32 %.3e" % (c.id, "v/" + name, sr.figure(v_back, r64 * r64),
                                                          sr.figure(r32.astype(np.float64) ** 2, r64 * r64)))
    if not np.isfinite(m).all() or (em > bg + sr.MOMENT_EPS * np.abs(r64)).any():
        i = np.unravel_index(np.argmax(em), em.shape)
        rep.bad.append("%s m/%s: |m / (1 - beta1) - ref| = %.3e at %s (ref %.6e, %d entries)" % (c.id, name, em[i], i, r64[i], cnt[i[0]]))
    if not np.isfinite(v).all() or (ev > 2.0 * np.abs(r64) * bg + bg * bg + sr.MOMENT_EPS * r64 * r64).any():
        i = np.unravel_index(np.argmax(ev), ev.shape)
        rep.bad.append("%s v/%s: |v / (1 - beta2) - ref^2| = %.3e at %s (ref %.6e, %d entries)" % (c.id, name, ev[i], i, r64[i], cnt[i[0]]))
    short = cnt <= sr.exact_entries(c)
    assert short.any()
    if not (np.array_equal(m[short], (r32 * omb1)[short]) and np.array_equal(v[short], ((r32 * r32) * omb2)[short])):
        rep.bad.append("%s %s: the moments of segments of <= %d entries are not (1 - beta) x the float32 ascending-order sums"
                       % (c.id, name, sr.exact_entries(c)))


@pytest.mark.parametrize("cid", sr.ids_of("adam"))
def test_fused_scatter_adam_gradient_matches_fp64(cid):
    """rsx_segsum_adam_rows2 (EmbeddingArena.segsum_adam; no sweep, no window, no extra segments, zero moments): the summed
    gradient out of m and v.  Untouched rows: table bits unchanged, moments exactly zero."""
    from recsys_amd.ops import AdamTF1, EmbeddingArena
    c, d = sr.CASE[cid], sr.draw(cid)
    a, idt, S = _sorted_arena(c, d, c.B)
    second = None
    if c.second:
        a2 = EmbeddingArena(d.row_off, c.D, c.B, "cuda", tables=d.tables2)
        a2.share_sort_of(a)
        a2.field_sort(idt)
        second = (a2, _t(d.dX2))
    opt = AdamTF1(lr=1e-3)
    lr, b1, b2, eps = (np.float32(x) for x in opt.hp)
    omb1, omb2 = np.float32(1) - b1, np.float32(1) - b2
    assert not a.m_t.any() and not a.v_t.any() and not a.m_w.any() and not a.v_w.any()
    a.segsum_adam(c.B, S, _t(d.dX), _t(d.gy1), _t(d.gy2), opt, [], second=second)
    torch.cuda.synchronize()
    assert opt.global_step == 1
    uniq, cnt, refs = sr.references(c, d, None if S is None else S.cpu().numpy())
    _check_slots(a, uniq, d.R)
    rest = np.ones(d.R, bool)
    rest[uniq] = False
    rep = Report(c)
    sets = [("G", a, d.tables)] + ([("G2", second[0], d.tables2)] if c.second else [])
    for name, ar, t0 in sets:
        m, v, var = ar.m_t.cpu().numpy(), ar.v_t.cpu().numpy(), ar.tables.cpu().numpy()
        _moments(rep, name, m[uniq], v[uniq], *refs[name], cnt, omb1, omb2)
        assert np.array_equal(var[rest], t0[rest]) and not m[rest].any() and not v[rest].any(), name
        assert (var[uniq] != t0[uniq]).any(1).all(), name                 # every touched row moved
    mw, vw, w = a.m_w.cpu().numpy(), a.v_w.cpu().numpy(), a.w1.cpu().numpy()
    if d.gy1 is not None:
        _moments(rep, "gw1", mw[uniq], vw[uniq], *refs["gw1"], cnt, omb1, omb2)
        assert np.array_equal(w[rest], d.w1[rest]) and not mw[rest].any() and not vw[rest].any()
    else:
        assert np.array_equal(w, d.w1) and not mw.any() and not vw.any()
    rep.done()
