"""Reference of the DCN cross layers (csrc/cross.hip, csrc/cross_device.h, gather_cross_fwd_k in csrc/embedding.hip, the cross rider
of tower_bwd_big_k in csrc/tower.hip) for tests/test_gpu_cross_forms.py and tests/test_cross_ref_cpu.py: the case table (with the
form each case was derived to take), the inputs of a case, the fp64 reference, the plain float32 restatement and the host's
dispatch rules restated.  Nothing here touches the HIP library, so the CPU suite can import it.

The operation (dcn/dcn.py:132-142):
    x_{l+1} = (x_l . w_l) * x0 + x_l + b_l     l = 0 .. L-1,   s_l = x_l . w_l  (saved for the backward)
    cz      = <x_L, wout>                      the cross output's share of the logit
The backward is judged through the functional  sum(dxL * x_L) + sum(gz * cz)  with either term absent ("x", "z", "xz").

Forms (rsx_cross_bwd_defer and rsx_tower_bwd_layer_defer, restated by `bwd_form` / `rider_form` below):
    bwd4    cross_bwd4_k<L>: L <= 3 and 4 (2L+1) dim floats <= 80 KiB.  4 waves per workgroup, epw4 examples per wave (1 up to
            B = 1024, 2 up to 8192, else 4), one partial per workgroup: RT = ceil(B / (4 epw4))
    wave    cross_bwd_k: everything else whose (2L+1) dim floats fit 64 KiB.  One wave per workgroup, epw examples (1 up to 512,
            2 up to 2048, else 4), RT = ceil(B / epw)
    rider   cross_bwd4_body<3> as the last ceil(B / (4 xr_epw)) workgroups of the last tower layer's tower_bwd_big_k<2, NTD, false,
            true> launch; xr_epw is tower.hip's own copy of the epw4 rule"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

CROSS_MAX_L = 8           # csrc/cross_device.h
CROSS_MAX_DIM = 1024      # 256 float4 per wave x CROSS_NV = 4
LDS_BWD4 = 80 * 1024
LDS_WAVE = 64 * 1024
TOWER_BIG_MIN_B = 1024    # csrc/tower.hip

# the project's numbers for this comparison (tests/segsum_ref.py)
RTOL = 2e-5
ATOL_REL = 2e-7
ATOL_ZERO = 1e-7

# Bounds wider than the defaults for the KERNELS, per (case id, terms, tensor), as a multiple of max|reference|: 4 x the figure
# of the float32 restatement for that tensor (its line in profiles/cross_fp64_errors.txt) -- never taken from the kernels' own
# error.  Empty: the kernels are inside the default bounds in every tensor of every case.
LOOSER = {}
# Tensors whose float32 RESTATEMENT is outside the default bounds, with its figure (tests/test_cross_ref_cpu.py holds it to 4 x
# that).  All are the deepest chains of the table: 7 or 8 layers at the widest dims, where x_l has grown by an order of magnitude
# over x0 and a few elements that nearly cancel carry the rounding of the large terms.
RESTATEMENT_OUTSIDE = {
    ("f6x1024x8", "fwd", "xL"): 5.599e-07,
    ("g130x80x8", "fwd", "xL"): 5.794e-07,
    ("b70x1024x7", "x", "dW"): 3.348e-07,
    ("b70x1024x7", "x", "dB"): 4.018e-07,
    ("b70x1024x7", "xz", "dB"): 6.190e-07,
}


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def epw_wave(B):
    return 1 if B <= 512 else (2 if B <= 2048 else 4)


def epw_bwd4(B):
    return 1 if B <= 1024 else (2 if B <= 8192 else 4)


def bwd_form(B, dim, L, bwd4=True):
    """-> (form, epw, RT, LDS bytes per workgroup); form "unsupported": RSX_EUNSUPPORTED before any launch.
    bwd4=False: RSX_CROSS_BWD4=0, the one-wave form for every L."""
    if dim % 4 or dim > CROSS_MAX_DIM or L > CROSS_MAX_L:
        return "unsupported", 0, 0, 0
    lds4 = 4 * (2 * L + 1) * dim * 4
    if bwd4 and L <= 3 and lds4 <= LDS_BWD4:
        e = epw_bwd4(B)
        return "bwd4", e, -(-B // (4 * e)), lds4
    lds = (2 * L + 1) * dim * 4
    if lds > LDS_WAVE:
        return "unsupported", 0, 0, lds
    e = epw_wave(B)
    return "wave", e, -(-B // e), lds


def partials_needed(B, L, dim=32):
    """the most partials a batch of B writes in either form (the one-wave form is reachable for every L: RSX_CROSS_BWD4=0)"""
    return max(bwd_form(B, dim, L, bwd4=b4)[2] for b4 in (True, False))


def tower_bwd_is_big(B, K, N):
    return B >= TOWER_BIG_MIN_B and K >= (64 if B >= 4096 else 256) and N % 4 == 0 and N <= 128 and K % 4 == 0


def rider_form(B, dim, L, widths):
    """-> (NTD of the carrying tower_bwd_big_k<2, NTD, false, true>, xr_epw, cross workgroups, their LDS bytes, first layer wide),
    or None where rsx_tower_bwd_cross_ride_supported says no"""
    if len(widths) < 2:
        return None
    k_last, n_last = widths[-2], widths[-1]
    lds4 = 4 * (2 * L + 1) * dim * 4
    if not (tower_bwd_is_big(B, k_last, n_last) and k_last <= 128 and tower_bwd_is_big(B, dim, widths[0]) and L == 3
            and dim % 4 == 0 and dim <= CROSS_MAX_DIM and lds4 <= LDS_BWD4):
        return None
    e = 1 if B <= 1024 else (2 if B <= 8192 else 4)           # tower.hip p.xr_epw: its OWN copy of the epw4 rule
    return (4 if n_last <= 64 else 8), e, -(-B // (4 * e)), lds4, dim > 128


# ------------------------------------------------------------------------------------------------ the case table
# kind    fwd (cross_fwd_k) | gather (gather_cross_fwd_k: dim = 16 F, `rows` per field) | bwd | rider
# form / epw / RT / lds   what the case was derived to take (tests/test_cross_ref_cpu.py re-derives them from the rules above)
# defer   bwd: also through rsx_cross_bwd_defer + rsx_cross_reduce_run
# own_s   bwd: also on the kernel's own forward output s, as production runs it
Case = namedtuple("Case", "id kind B dim L form epw RT lds rows widths rate ntd defer own_s seed")

TERMS = ("x", "z", "xz")          # dxL only, gz only, both
FWD_OUTS = ("xL", "cz", "xLcz")   # s always
CRITEO_ROWS_CAP = 1000


def _criteo_rows():
    from oracle import criteo
    return tuple(min(int(r), CRITEO_ROWS_CAP) for r in np.diff(criteo.row_offsets()))


def _cases():
    out = []

    def add(kind, B, dim, L, form=None, epw=0, RT=0, lds=0, rows=None, widths=None, rate=0.0, ntd=0, defer=False, own_s=False,
            seed_bump=0):
        cid = "%s%dx%dx%d" % (kind[0], B, dim, L)
        out.append(Case(cid, kind, B, dim, L, form, epw, RT, lds, rows, widths, rate, ntd, defer, own_s,
                        zlib.crc32(cid.encode()) + seed_bump))

    # ---- forward, cross_fwd_k: a lane holds float4 #(lane + 64 v), v < 4; 4 examples per workgroup
    add("fwd", 5, 4, 1)            # n4 = 1: one live lane, 63 clamped loads; two workgroups, the second with one example
    add("fwd", 33, 256, 3)         # n4 = 64: exactly one full vector per lane; 9 workgroups, the last with one example
    add("fwd", 7, 260, 2)          # n4 = 65: the second vector has one live lane
    add("fwd", 6, 1024, 8)         # n4 = 256: four full vectors, the layer maximum
    add("fwd", 37, 624, 3)         # dcn.py's width (n4 = 156: the third vector has 28 live lanes)
    # ---- forward, gather_cross_fwd_k: lane = 4 j + q holds quarter q of fields j, j + 16, j + 32, j + 48
    add("gather", 9, 16, 2, rows=(50,))                           # F = 1: dim 16
    add("gather", 130, 80, 8, rows=(3, 7, 4, 11, 6))              # F = 5, tiny tables (every row shared by many examples)
    add("gather", 37, 624, 3, rows=_criteo_rows())                # F = 39: the Criteo layout (tables capped at 1000 rows)
    add("gather", 6, 1024, 2, rows=(20,) * 64)                    # F = 64: dim 1024
    # ---- backward, cross_bwd4_k<L>: LDS = 4 (2L+1) dim 4 bytes <= 81 920
    add("bwd", 5, 4, 1, "bwd4", 1, 2, 192)                        # the <1> instantiation; 2 workgroups, the second with one wave at work
    add("bwd", 1024, 64, 2, "bwd4", 1, 256, 5120)                 # epw4 = 1: the last B before the switch
    add("bwd", 1025, 64, 2, "bwd4", 2, 129, 5120, defer=True)     # epw4 = 2; workgroup 128 holds example 1024 alone: waves 1..3 idle
    add("bwd", 8193, 16, 3, "bwd4", 4, 513, 1792)                 # epw4 = 4; workgroup 512 holds example 8192 alone
    add("bwd", 9, 1024, 2, "bwd4", 1, 3, 81920)                   # 4 * 5 * 1024 * 4 = 81 920 B: exactly 80 KiB, still this form
    add("bwd", 9, 728, 3, "bwd4", 1, 3, 81536)                    # 4 * 7 * 728 * 4 = 81 536 B: the widest <3>
    add("bwd", 300, 624, 3, "bwd4", 1, 75, 69888, own_s=True)     # dcn.py's width
    # ---- backward, cross_bwd_k: LDS = (2L+1) dim 4 bytes <= 65 536
    add("bwd", 9, 732, 3, "wave", 1, 9, 20496)                    # 4 * 7 * 732 * 4 = 81 984 B > 80 KiB: L = 3 lands in this form
    add("bwd", 512, 64, 4, "wave", 1, 512, 2304)                  # epw 1: the last B before the switch
    add("bwd", 513, 64, 5, "wave", 2, 257, 2816, own_s=True)      # epw 2; the last wave holds example 512 alone
    add("bwd", 2049, 32, 4, "wave", 4, 513, 1152, defer=True)     # epw 4; the last wave holds example 2048 alone
    add("bwd", 11, 960, 8, "wave", 1, 11, 65280)                  # 17 * 960 * 4 = 65 280 B: the widest L = 8
    add("bwd", 70, 1024, 7, "wave", 1, 70, 61440)                 # the widest dim (15 * 1024 * 4 = 61 440 B)
    # ---- the rider: cross_bwd4_body<3> inside the last tower layer's tower_bwd_big_k<2, NTD, false, true>
    add("rider", 4100, 64, 3, "rider", 2, 513, 7168, widths=(64, 20), rate=0.5, ntd=4)      # xr_epw 2, 513 cross workgroups, the last ragged
    add("rider", 4096, 624, 3, "rider", 2, 512, 69888, widths=(100, 100), rate=0.5, ntd=8)  # dcn.py itself; first layer wide, acc_dx
    add("rider", 8200, 64, 3, "rider", 4, 513, 7168, widths=(128, 64), rate=0.0, ntd=4)     # xr_epw 4; K_last = 128: the envelope's edge
    add("rider", 4096, 728, 3, "rider", 2, 512, 81536, widths=(64, 16), rate=0.0, ntd=4)    # the rider's LDS maximum
    return out


CASES = _cases()
CASE = {c.id: c for c in CASES}
assert len(CASE) == len(CASES)
UNSUPPORTED = (11, 964, 8)        # 17 * 964 * 4 = 65 552 B > 64 KiB: RSX_EUNSUPPORTED before any launch
# capacity != batch: (dim, L, capacity, batches) -- the workspace is CrossLayers' own, sized once for the capacity
CAPACITY_CASES = ((32, 4, 3000, (2000, 3000)), (32, 3, 8193, (1024,)))


def ids_of(kind, form=None):
    return [c.id for c in CASES if c.kind == kind and (form is None or c.form == form)]


# ------------------------------------------------------------------------------------------------ inputs
class Inputs:
    pass


def draw_shape(B, dim, L, seed, rows=None):
    """float32 CPU tensors, a function of the arguments alone (shared: never written to).
    x0 = 0.5 N(0,1) (gather: the tables are, x0 = the gathered rows); W = N(0,1) / sqrt(dim), so |s_l| is of order 0.5 at every dim;
    Bc = 0.3 N(0,1); wout = N(0,1) / sqrt(dim); dxL = N(0,1); gz = +-U(0.5, 1.5) * 1e-2, so no example's share of a batch sum is
    negligible; pre = N(0,1), the unit prefill of dX for accumulate = 1 (scaled to the gradient by `prefill`)."""
    g = torch.Generator().manual_seed(seed)
    d = Inputs()
    d.B, d.dim, d.L = B, dim, L
    if rows is not None:
        F = len(rows)
        assert 16 * F == dim
        off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        d.row_off = torch.from_numpy(off.astype(np.int32))
        d.tables = 0.5 * torch.randn(int(off[-1]), 16, generator=g)
        d.ids = torch.stack([torch.randint(0, int(r), (B,), generator=g) for r in rows], 1).to(torch.int32)
        d.x0 = d.tables[(d.ids.long() + torch.from_numpy(off[:-1])[None, :])].reshape(B, dim).contiguous()
    else:
        d.x0 = 0.5 * torch.randn(B, dim, generator=g)
    d.W = torch.randn(L, dim, generator=g) / np.sqrt(dim)
    d.Bc = 0.3 * torch.randn(L, dim, generator=g)
    d.wout = torch.randn(dim, generator=g) / np.sqrt(dim)
    d.dxL = torch.randn(B, dim, generator=g)
    sign = torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0)
    d.gz = sign * (0.5 + torch.rand(B, generator=g)) * 1e-2
    d.pre = torch.randn(B, dim, generator=g)
    return d


@functools.lru_cache(maxsize=None)
def draw(cid):
    c = CASE[cid]
    return draw_shape(c.B, c.dim, c.L, c.seed, c.rows)


# ------------------------------------------------------------------------------------------------ the references
class Ref:
    pass


def forward(x0, W, Bc, wout=None, drop_layer=None):
    """dcn/dcn.py:132-142 -> (x_L, s [B, L], cz or None).  drop_layer: that layer's s_l * x0 term left out (the CPU test's teeth)."""
    x, ss = x0, []
    for l in range(W.shape[0]):
        s = (x * W[l]).sum(1)
        ss.append(s)
        x = (x + Bc[l]) if l == drop_layer else (s[:, None] * x0 + x + Bc[l])
    return x, torch.stack(ss, 1), (None if wout is None else x @ wout)


def run_ref(d, terms="xz", dtype=torch.float64, device="cpu", drop_layer=None, keep=None, gz=None):
    """The forward and, through torch autograd, the gradient of sum(dxL * x_L) + sum(gz * cz) in `dtype` (fp64: the reference;
    float32: the plain restatement).  terms: "x" dxL only, "z" gz only, "xz" both.  keep: a boolean mask [B] of the examples that
    take part (one example left out: the CPU test's teeth).  gz: another head gradient than the drawn one (the rider's).
    -> Ref with xL, s, cz and dX, dW, dB, dwout (dwout None without gz)."""
    to = lambda t: t.detach().to(device=device, dtype=dtype, copy=True)
    sel = (lambda t: t) if keep is None else (lambda t: t[keep])
    x0, W, Bc, wout = sel(to(d.x0)).requires_grad_(), to(d.W).requires_grad_(), to(d.Bc).requires_grad_(), to(d.wout).requires_grad_()
    xL, s, cz = forward(x0, W, Bc, wout, drop_layer)
    r = Ref()
    r.xL, r.s, r.cz = xL.detach(), s.detach(), cz.detach()
    loss = 0.0
    if "x" in terms:
        loss = loss + (sel(to(d.dxL)) * xL).sum()
    if "z" in terms:
        loss = loss + (sel(to(d.gz if gz is None else gz)) * cz).sum()
    loss.backward()
    r.dX, r.dW, r.dB = x0.grad, W.grad, Bc.grad
    r.dwout = wout.grad if "z" in terms else None
    return r


def prefill(d, ref_dX):
    """dX before an accumulate = 1 launch: the unit draw scaled to the gradient's rms, so that neither hides the other -> float32"""
    return (d.pre.to(ref_dX.device) * float(ref_dX.pow(2).mean().sqrt())).to(torch.float32)


def tensors(r, terms, pre=None):
    """{name: tensor} of a backward Ref; pre: the float32 prefill of an accumulate = 1 run (expected dX = prefill + gradient)"""
    out = {"dX": r.dX if pre is None else pre.to(r.dX.dtype) + r.dX, "dW": r.dW, "dB": r.dB}
    if "z" in terms:
        out["dwout"] = r.dwout
    return out


def bound(ref, key=None, rtol=RTOL):
    """elementwise |got - ref| admitted for a tensor with reference `ref` (float64)"""
    m = float(ref.abs().max()) if ref.numel() else 0.0
    if key is not None and key in LOOSER:
        return rtol * ref.abs() + LOOSER[key] * m
    return rtol * ref.abs() + (ATOL_REL * m if m > 0.0 else ATOL_ZERO)


def misses(got, ref, key=None):
    """number of elements of `got` outside the bounds around `ref` (a NaN is outside)"""
    ref = ref.double()
    got = got.to(ref.device).double().reshape(ref.shape)
    return int((~((got - ref).abs() <= bound(ref, key))).sum())


def figure(got, ref):
    """max|got - ref| / max|ref| (the absolute error where the reference is exactly zero)"""
    ref = ref.double()
    m = float(ref.abs().max()) if ref.numel() else 0.0
    e = float((got.to(ref.device).double().reshape(ref.shape) - ref).abs().max()) if ref.numel() else 0.0
    return e / m if m > 0.0 else e
