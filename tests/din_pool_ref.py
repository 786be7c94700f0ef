"""Reference of DIN's attention-weighted history pooling (csrc/din.hip, din/din.py:118-124) for tests/test_gpu_din_pool_forms.py
and tests/test_tower_nobn_ref_cpu.py: the shapes, the inputs, the fp64 numpy restatement and the comparison with DERIVED bounds.
Nothing here touches the HIP library.

    out[b, :]   = sum_p H[b, p, :] * w[b, p] * (ids[b, p] > 0)
    dw[b, p]    = <H[b, p, :], dout[b, :]> * (ids[b, p] > 0)
    dH[b, p, :] = (prev +) dout[b, :] * w[b, p] * (ids[b, p] > 0)

Bounds (u = 2^-24, the unit roundoff of fp32; every input is an fp32 value, so the fp64 restatement's own error is ~2^-53 of the
same sums and does not count):
    out   P products of one rounding each and at most P - 1 additions, in any order:  (P + 1) u sum_p |H w mask|, elementwise
    dw    K products and K - 1 additions:                                             (K + 1) u sum_k |H dout|
    dH    written: one product, one rounding:                                         2 u |ref|   (twice the rounding: 2^-23)
          accumulated: the product's rounding and the addition's:                     2 u (|prev| + |term|)
Padded positions (id <= 0: zeros AND negatives) give dw == 0 and dH == 0 (written) or dH == prev (accumulated) by value, and a
wholly padded example gives out == 0 (its bound is 0)."""
import numpy as np

U = 2.0 ** -24
KS = (4, 8, 16, 32, 64)
BS = (1, 3, 4, 5, 9)                 # four examples per workgroup: one partly filled, one full, one and a bit, two and a bit


def rpw(K):
    """history positions one wave takes per trip of its loop (64 lanes, K / 4 lanes per row; four trips are batched)"""
    return 256 // K


def positions(K):
    """P on both sides of one trip (RPW), of the four-trip batch (4 RPW) and well past it"""
    r = rpw(K)
    return (1, r - 1, r, r + 1, 4 * r - 1, 4 * r, 4 * r + 1, 9 * r + 3)


def shapes(K):
    return [(P, B) for P in positions(K) for B in BS]


def draw(K, P, B, seed):
    """Two histories' inputs (float32 / int32 numpy): finite H, w, dout, prev; ids in -3 .. 5 with about half padded, and by
    construction: example 0 starts with a padded position, example 1 (if any) is wholly padded with zeros and negatives
    alternating, the last example (B >= 3) ends with a negative id."""
    rng = np.random.default_rng(seed)
    hs = []
    for t in range(2):
        ids = rng.integers(-3, 6, size=(B, P)).astype(np.int32)
        ids[0, 0] = 0
        if B >= 2:
            ids[1, :] = np.where(np.arange(P) % 2 == 0, 0, -2)
        if B >= 3:
            ids[-1, -1] = -1
        hs.append(dict(H=rng.standard_normal((B, P, K)).astype(np.float32), w=rng.standard_normal((B, P)).astype(np.float32),
                       ids=ids, dout=rng.standard_normal((B, K)).astype(np.float32),
                       prev=rng.standard_normal((B, P, K)).astype(np.float32)))
    return hs


def ref_fwd(h):
    """-> (out, sum_p |terms|) in float64"""
    m = (h["ids"] > 0).astype(np.float64)
    t = h["H"].astype(np.float64) * (h["w"].astype(np.float64) * m)[:, :, None]
    return t.sum(1), np.abs(t).sum(1)


def ref_bwd(h):
    """-> (dw, sum_k |H dout|, the dH term) in float64"""
    m = (h["ids"] > 0).astype(np.float64)
    t = h["H"].astype(np.float64) * h["dout"].astype(np.float64)[:, None, :]
    term = h["dout"].astype(np.float64)[:, None, :] * (h["w"].astype(np.float64) * m)[:, :, None]
    return t.sum(2) * m, np.abs(t).sum(2), term


def check_fwd(tag, out, h):
    ref, mag = ref_fwd(h)
    P = h["ids"].shape[1]
    err = np.abs(out.astype(np.float64) - ref)
    assert np.isfinite(out).all(), tag
    assert (err <= (P + 1) * U * mag).all(), (tag, "out", float(err.max()), float((err / np.maximum((P + 1) * U * mag, 1e-300)).max()))


def check_bwd(tag, dH, dw, h, accumulate):
    ref_dw, mag, term = ref_bwd(h)
    K = h["H"].shape[2]
    pad = h["ids"] <= 0
    assert np.isfinite(dH).all() and np.isfinite(dw).all(), tag
    err = np.abs(dw.astype(np.float64) - ref_dw)
    assert (err <= (K + 1) * U * mag).all(), (tag, "dw", float(err.max()))
    assert (dw[pad] == 0).all(), (tag, "dw at padded positions")
    prev = h["prev"].astype(np.float64) if accumulate else np.zeros_like(term)
    err = np.abs(dH.astype(np.float64) - (prev + term))
    assert (err <= 2 * U * (np.abs(prev) + np.abs(term))).all(), (tag, "dH", float(err.max()))
    if accumulate:
        assert (dH[pad] == h["prev"][pad]).all(), (tag, "dH at padded positions: prev")
    else:
        assert (dH[pad] == 0).all(), (tag, "dH at padded positions")


# --------------------------------------------------------------------------- plain fp32 restatements (the CPU tests' stand-in kernel)
def f32_fwd(h, mask=None, drop=None):
    """fp32 numpy.  mask: the padding rule (default ids > 0).  drop = (b, p): that position is left out (a planted defect)."""
    m = (h["ids"] > 0) if mask is None else mask
    t = h["H"] * (h["w"] * m.astype(np.float32))[:, :, None]
    if drop is not None:
        t[drop[0], drop[1]] = 0.0
    return t.sum(1, dtype=np.float32)


def f32_bwd(h, accumulate, mask=None):
    m = ((h["ids"] > 0) if mask is None else mask).astype(np.float32)
    dw = (h["H"] * h["dout"][:, None, :]).sum(2, dtype=np.float32) * m
    dH = h["dout"][:, None, :] * (h["w"] * m)[:, :, None]
    return ((h["prev"] + dH) if accumulate else dH).astype(np.float32), dw.astype(np.float32)
