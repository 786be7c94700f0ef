"""DIN's history pooling (csrc/din.hip) against fp64 numpy in EVERY entry point recsys_amd/din.py launches and every form of each:
rsx_din_pool_fwd / _fwd_ld / _fwd_pair, rsx_din_pool_bwd / _bwd_ld / _bwd_pair / _bwd_pair_ride, accumulate 0 and 1, row strides
K, K + 4 and 3K (outputs and d(outputs)) and K and 2K (dH), at history lengths on both sides of one trip of the kernels' position
loop (RPW = 256 / K), of its four-trip batch and well past it, and batches on both sides of the four examples per workgroup.

The reference, the inputs (padding by zeros AND negatives, a wholly padded example, a padded first position) and the derived bounds:
tests/din_pool_ref.py.  Every output buffer is allocated with guard words; the guards, the gaps between strided rows and the
other history's slices hold a NaN bit pattern before a launch and must hold the same BITS after it (the d(outputs) a launch
reads sit in such a buffer too: a gap that was read would turn up as a NaN in the result)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import din_pool_ref as pr

pytestmark = pytest.mark.gpu

G = 64                        # guard words on both sides of every buffer (a multiple of 4: the float4 alignment survives)
NANBITS = 0x7FC0BEEF          # a quiet NaN with a payload


class Buf:
    """n floats between two guards, every word the NaN pattern; `mark` records what a launch is expected to write."""

    def __init__(self, n):
        self.n = n
        self.bits = torch.full((G + n + G,), NANBITS, dtype=torch.int32, device="cuda")
        self.f = self.bits.view(torch.float32)
        self.written = torch.zeros(G + n + G, dtype=torch.bool, device="cuda")

    def ptr(self, off=0):
        return C.c_void_p(self.bits.data_ptr() + 4 * (G + off))

    def rows(self, nrows, ld, col, K, row0=0):
        """the [nrows, K] view at column `col` of rows row0.. with stride ld"""
        return self.f[G:G + self.n].view(-1, ld)[row0:row0 + nrows, col:col + K]

    def mark(self, nrows, ld, col, K, row0=0):
        self.written[G:G + self.n].view(-1, ld)[row0:row0 + nrows, col:col + K] = True

    def snapshot(self):
        self.before = self.bits.clone()

    def assert_rest_untouched(self, tag):
        keep = ~self.written
        assert torch.equal(self.bits[keep], self.before[keep]), (tag, "a word outside the launch's outputs changed")


def _dev(h):
    return {k: torch.from_numpy(v).cuda() for k, v in h.items()}


def _strided(B_rows, ld, K):
    """(buffers, columns) of two histories' [rows, K] blocks with row stride ld: ld = 3K is din.py's MLP input (ONE buffer, the
    slices at columns K and 2K, columns 0 .. K-1 someone else's), ld = 2K (dH) the scatter's value block (one buffer, columns 0
    and K); anything else two buffers of their own."""
    if ld == 3 * K:
        b = Buf(B_rows * ld)
        return [b, b], [K, 2 * K]
    if ld == 2 * K:
        b = Buf(B_rows * ld)
        return [b, b], [0, K]
    return [Buf(B_rows * ld), Buf(B_rows * ld)], [0, 0]


def run_fwd(form, hs, dv, K, ld_out):
    """-> [out_0, out_1] (numpy [B, K]); form: plain (ld_out = K), ld, pair."""
    from recsys_amd import _lib
    from recsys_amd.ops import _ptr, _stream
    L = _lib.lib()
    B, P = hs[0]["ids"].shape
    bufs, cols = _strided(B, ld_out, K)
    for t in range(2):
        bufs[t].mark(B, ld_out, cols[t], K)
    for b in set(bufs):
        b.snapshot()
    a = [[_ptr(dv[t]["H"]), _ptr(dv[t]["w"]), _ptr(dv[t]["ids"]), bufs[t].ptr(cols[t])] for t in range(2)]
    if form == "pair":
        _lib.check(L.rsx_din_pool_fwd_pair(*a[0], *a[1], B, P, K, ld_out, _stream()), "rsx_din_pool_fwd_pair")
    else:
        for t in range(2):
            if form == "plain":
                assert ld_out == K
                _lib.check(L.rsx_din_pool_fwd(*a[t], B, P, K, _stream()), "rsx_din_pool_fwd")
            else:
                _lib.check(L.rsx_din_pool_fwd_ld(*a[t], B, P, K, ld_out, _stream()), "rsx_din_pool_fwd_ld")
    torch.cuda.synchronize()
    for b in set(bufs):
        b.assert_rest_untouched((form, K, P, B, ld_out))
    return [bufs[t].rows(B, ld_out, cols[t], K).cpu().numpy() for t in range(2)]


def run_bwd(form, hs, dv, K, ld_dout, ld_dH, acc, rider=None, row0=0):
    """-> ([dH_0, dH_1] numpy [B, P, K], [dw_0, dw_1] numpy [B, P]); form: plain (both strides K), ld, pair, ride.
    row0: rows of the dH buffer in front of the histories' (din.py: the B target rows of the value block)."""
    from recsys_amd import _lib
    from recsys_amd.ops import _ptr, _stream
    L = _lib.lib()
    B, P = hs[0]["ids"].shape
    gb, gc = _strided(B, ld_dout, K)                      # d(outputs): READ -- the values in their slices, the NaN pattern around
    hb, hc = _strided(row0 + B * P, ld_dH, K)
    wb = [Buf(B * P), Buf(B * P)]
    for t in range(2):
        gb[t].rows(B, ld_dout, gc[t], K).copy_(dv[t]["dout"])
        if acc:
            hb[t].rows(B * P, ld_dH, hc[t], K, row0).copy_(dv[t]["prev"].view(B * P, K))
        hb[t].mark(B * P, ld_dH, hc[t], K, row0)
        wb[t].mark(B * P, 1, 0, 1)
    every = set(gb) | set(hb) | set(wb)
    for b in every:
        b.snapshot()
    a = [[_ptr(dv[t]["H"]), _ptr(dv[t]["w"]), _ptr(dv[t]["ids"]), gb[t].ptr(gc[t]), hb[t].ptr(row0 * ld_dH + hc[t]), wb[t].ptr()]
         for t in range(2)]
    if form == "pair":
        _lib.check(L.rsx_din_pool_bwd_pair(*a[0], *a[1], acc, B, P, K, ld_dout, ld_dH, _stream()), "rsx_din_pool_bwd_pair")
    elif form == "ride":
        _lib.check(L.rsx_din_pool_bwd_pair_ride(*a[0], *a[1], acc, B, P, K, ld_dout, ld_dH,
                                                None if rider is None else C.byref(rider), _stream()), "rsx_din_pool_bwd_pair_ride")
    else:
        for t in range(2):
            if form == "plain":
                assert ld_dout == K and ld_dH == K
                _lib.check(L.rsx_din_pool_bwd(*a[t], acc, B, P, K, _stream()), "rsx_din_pool_bwd")
            else:
                _lib.check(L.rsx_din_pool_bwd_ld(*a[t], acc, B, P, K, ld_dout, ld_dH, _stream()), "rsx_din_pool_bwd_ld")
    torch.cuda.synchronize()
    for b in gb:
        b.written[:] = False                                  # (an input: nothing of it may change)
    for b in every:
        b.assert_rest_untouched((form, K, P, B, ld_dout, ld_dH, acc))
    dH = [hb[t].rows(B * P, ld_dH, hc[t], K, row0).cpu().numpy().reshape(B, P, K) for t in range(2)]
    return dH, [wb[t].f[G:G + B * P].cpu().numpy().reshape(B, P) for t in range(2)]


def _check_both(tag, hs, outs=None, dH=None, dw=None, acc=0):
    for t in range(2):
        if outs is not None:
            pr.check_fwd(tag + (t,), outs[t], hs[t])
        if dH is not None:
            pr.check_bwd(tag + (t,), dH[t], dw[t], hs[t], acc)


def _equal(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("K", pr.KS)
def test_every_form_matches_fp64_and_pair_equals_two_launches(K):
    lds = (K, K + 4, 3 * K)
    seen = set()
    for i, (P, B) in enumerate(pr.shapes(K)):
        hs = pr.draw(K, P, B, 1000 * K + i)
        dv = [_dev(h) for h in hs]
        # plain
        _check_both(("plain", K, P, B), hs, outs=run_fwd("plain", hs, dv, K, K))
        for acc in (0, 1):
            dH, dw = run_bwd("plain", hs, dv, K, K, K, acc)
            _check_both(("plain", K, P, B, acc), hs, dH=dH, dw=dw, acc=acc)
        # _ld: the strides rotate with the shape so that every combination turns up (asserted below)
        for j in range(3):
            ld_out, ld_dout, ld_dH, acc = lds[j], lds[(j + i) % 3], (K, 2 * K)[(i // 3 + j) % 2], (i // 6 + j) % 2
            seen.add((ld_out, ld_dout, ld_dH, acc))
            _check_both(("ld", K, P, B, ld_out), hs, outs=run_fwd("ld", hs, dv, K, ld_out))
            dH, dw = run_bwd("ld", hs, dv, K, ld_dout, ld_dH, acc)
            _check_both(("ld", K, P, B, ld_dout, ld_dH, acc), hs, dH=dH, dw=dw, acc=acc)
        # pair (different H, w and ids per history) in din.py's strides: two _ld launches, bit for bit
        acc = i % 2
        o1, o2 = run_fwd("ld", hs, dv, K, 3 * K), run_fwd("pair", hs, dv, K, 3 * K)
        _check_both(("pair", K, P, B), hs, outs=o2)
        assert _equal(o1, o2), ("pair fwd", K, P, B)
        (h1, w1), (h2, w2) = run_bwd("ld", hs, dv, K, 3 * K, 2 * K, acc), run_bwd("pair", hs, dv, K, 3 * K, 2 * K, acc)
        _check_both(("pair", K, P, B, acc), hs, dH=h2, dw=w2, acc=acc)
        assert _equal(h1, h2) and _equal(w1, w2), ("pair bwd", K, P, B, acc)
        # rider = NULL is the pair form
        h3, w3 = run_bwd("ride", hs, dv, K, 3 * K, 2 * K, acc, rider=None)
        assert _equal(h2, h3) and _equal(w2, w3), ("ride without a rider", K, P, B, acc)
    assert len(seen) == 3 * 3 * 2 * 2, sorted(seen)


@pytest.mark.parametrize("K", (4, 16, 64))
def test_ride_with_a_real_reduce_job_equals_pair_plus_the_stand_alone_reduce(K):
    """The pooling backward carrying the one-launch tower's weight-gradient reduce as extra workgroups (din.py's step): the
    pooling results are the pair launch's and the tower's gradients and loss the default form's, all bit for bit."""
    from tests import test_gpu_tower_nobn as tn
    case, d, Pm, tw, dev = tn._fused("f_48")
    want = tn._train(case, Pm, tw, dev, d["masks"])
    for i, (P, B) in enumerate(((1, 1), (pr.rpw(K) + 1, 5), (4 * pr.rpw(K) + 1, 9))):
        acc = i % 2
        hs = pr.draw(K, P, B, 77 * K + i)
        dv = [_dev(h) for h in hs]
        tn._train(case, Pm, tw, dev, d["masks"], reduce_rider=True)
        job = tw.mlp_reduce_job
        assert job is not None and job.e4_last > 0
        Pm.grad.fill_(-3.25)
        tw.loss.fill_(-3.25)
        h1, w1 = run_bwd("pair", hs, dv, K, 3 * K, 2 * K, acc, row0=B)
        assert bool((Pm.grad == -3.25).all())
        h2, w2 = run_bwd("ride", hs, dv, K, 3 * K, 2 * K, acc, rider=job, row0=B)
        _check_both(("ride", K, P, B, acc), hs, dH=h2, dw=w2, acc=acc)
        assert _equal(h1, h2) and _equal(w1, w2), ("ride", K, P, B, acc)
        assert torch.equal(tw.loss, want["loss"])
        for k in Pm.params:
            assert torch.equal(Pm[k].grad, want["grads"][k]), k


@pytest.mark.parametrize("K,P,B", [(16, 100, 9), (4, 17, 5), (64, 5, 4)])
def test_the_buffers_of_the_din_step(K, P, B):
    """Laid out exactly as recsys_amd/din.py's step lays them out: the pooled histories are the column slices [K, 2K) and [2K, 3K)
    of the MLP input X [B, 3K] (columns [0, K): the target item's embedding, written by someone else); d(pooled) are the same
    slices of the tower's dX; dH of history t is column block t of rows B .. B + B P - 1 of the scatter's value block
    [B + B P, 2, K] (rows 0 .. B-1: the target rows' gradients, written later by the attention backward)."""
    hs = pr.draw(K, P, B, 31 * K + P)
    dv = [_dev(h) for h in hs]
    outs = run_fwd("pair", hs, dv, K, 3 * K)
    _check_both(("din fwd", K, P, B), hs, outs=outs)
    dH, dw = run_bwd("ride", hs, dv, K, 3 * K, 2 * K, 0, rider=None, row0=B)
    _check_both(("din bwd", K, P, B), hs, dH=dH, dw=dw, acc=0)
