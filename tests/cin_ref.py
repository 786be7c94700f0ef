"""Reference of the fp32 CIN layer kernels and of the 'cin_net' head (csrc/cin.hip) for tests/test_gpu_cin_forms.py and
tests/test_cin_ref_cpu.py: the case tables (with the form each layer case was derived to take -- the tests read the forms from
rsx_cin_layer_plan and compare), the inputs of a case, the fp64 reference, two plain float32 restatements and the bounds.  Nothing
here touches the HIP library, so the CPU suite can import it.

The layer (xdeepfm/xdeepfm.py:145-172, oracle/models.py cin_layer_fwd / cin_layer_bwd), D = 16:
    Z[b,d,f*H+h] = X0[b,f,d] * Xk[b,h,d]         pre[b,n,d] = sum_j Z[b,d,j] W[j,n]         out = relu(pre + c[n])
    backward, with g = dout + gs[b] * wout[n] (either part may be absent) and dpre = g * (out > 0):
    dW = Z^T dpre,  dc[n] = sum_{b,d} dpre,  dXk[b,h,d] = sum_f X0[b,f,d] (dpre W^T)[b,d,f,h],  dX0[b,f,d] = sum_h Xk[b,h,d] (...)
The head (xdeepfm/xdeepfm.py:175-182):
    y[b] = relu(sum_k sum_n Wout[off_k + n] * sum_d out_k[b,n,d] + bout);   gs = gy * (y > 0);  dWout = sum_b gs * sum_d out_k;
    dbout = sum_b gs;   the rider  dwnum[j] = sum_b logx[b,j] * g_lin[b]

The backward takes `out` as an INPUT: it is judged apart from the forward on the float32 rounding of the reference's out, so both
sides use the same relu mask; the `own_out` cases also run on the kernel's own forward output (the reference then takes that mask).

Forms of rsx_cin_layer_bwd (HT = ceil(H / 16)):
    data gradients   tiled: cin_bwd_dx2_k<NSMAX, 4, 1> + cin_dx0_reduce_k when HT >= 5 and N % 4 == 0; else cin_bwd_dx_k<NSMAX> with
                     FS = 4 (HT <= 3), 2 (HT = 4), 1 (HT >= 5) field parts, HT * FS waves; NSMAX = 2 up to N = 32, else 8
    weight gradients one of five (FT, NT, NW) tiles by a cost formula over (F, H, N); a sweep slice riding forces configuration 2
    forward          cin_fwd_k<12> up to H = 48, else <32>"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

D = 16
CIN_MAXL = 8

# ------------------------------------------------------------------------------------------------ the bounds
# |got - ref| <= RTOL |ref| + A max|ref| per element, A by the tensor's kind: "fwd" (out, y) or "bwd" (every gradient).
# How the constants were set: for every case and tensor, max|x - ref| / max|ref| of both float32 restatements was computed on the CPU
# (tests/test_cin_ref_cpu.py holds every element to a quarter of the bound: the summation order is the only legitimate
# difference between two fp32 evaluations, and the matrix cores' internal order is a third one).  The largest figures are 4.7e-7
# forward (out of lds82, F H = 12 800 terms) and 7.0e-7 backward (dWout of the 515-example head case; 5.8e-7 in the layers), four
# times which is 1.9e-6 and 2.8e-6 -- so the constants are the bars tests/test_gpu_cin_split.py (TOL / BTOL) holds the same
# contraction to, no relative part is needed, and no kernel figure asked for more (profiles/cin_fp64_errors.txt: the kernels' largest
# are of the restatements' size).
# The restatements sum as the kernels' formulation does, in two short sums (over h, then over f; dW over blocks of examples).  The
# script's single product over K = F H terms is the worse float32 algorithm -- 5.9e-7 through torch's matmul and 1.1e-6 through
# numpy's einsum at these shapes -- and four times that would be past the split path's bars; layer_fwd_chain keeps it for fp64.
RTOL = 0.0
A_FWD = 2e-6
A_BWD = 3e-6
ATOL_ZERO = 1e-7        # a reference that is zero throughout
MARGIN = 4.0
KIND = {"out": "fwd", "y": "fwd"}      # everything else: "bwd"


def bound(ref, name, margin=1.0):
    """elementwise |got - ref| admitted for tensor `name` with reference `ref` (float64 torch)"""
    a = A_FWD if KIND.get(name, "bwd") == "fwd" else A_BWD
    m = float(ref.abs().max()) if ref.numel() else 0.0
    return (RTOL * ref.abs() + (a * m if m > 0.0 else ATOL_ZERO)) / margin


def _t(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


def misses(got, ref, name, margin=1.0):
    """number of elements of `got` outside the bounds around `ref` (a NaN is outside)"""
    ref = _t(ref).double()
    got = _t(got).to(ref.device).double().reshape(ref.shape)
    return int((~((got - ref).abs() <= bound(ref, name, margin))).sum())


def figure(got, ref):
    """max|got - ref| / max|ref| (the absolute error where the reference is exactly zero)"""
    ref = _t(ref).double()
    m = float(ref.abs().max()) if ref.numel() else 0.0
    e = float((_t(got).to(ref.device).double().reshape(ref.shape) - ref).abs().max()) if ref.numel() else 0.0
    return e / m if m > 0.0 else e


# ------------------------------------------------------------------------------------------------ the layer cases
# first     Xk is X0 and dXk is dX0 (one gradient buffer for both roles, acc_dx0 = 1)
# tiled / nsmax / FS / cfg / hsmax / optin   the form the case was derived to take (rsx_cin_layer_plan out[1], [2], [3], [6], [0], [5])
# lds       the data-gradient launch's LDS bytes where the case is about them
# variants  backward runs: gradient mode d (dout only), g (gs / wout only), b (both) + acc_dxk + acc_dx0
# own_out   also on the kernel's own forward output
LayerCase = namedtuple("LayerCase", "id B F H N first tiled nsmax FS cfg hsmax optin lds variants own_out seed")


def _layer_cases():
    out = []

    def add(cid, B, F, H, N, tiled, nsmax, FS, cfg, hsmax, variants, first=False, optin=0, lds=None, own_out=False):
        out.append(LayerCase(cid, B, F, H, N, first, tiled, nsmax, FS, cfg, hsmax, optin, lds, tuple(variants.split()), own_out,
                             zlib.crc32(cid.encode())))

    # B is ragged against every unit: 4 examples per forward workgroup, EB = 4 of the tiled form, NW = 4 / 8 waves of the weight
    # gradients, 4 NW examples per trip of their batch loop
    add("l2_c0", 37, 39, 128, 128, 1, 8, 1, 0, 32, "b00 d11", own_out=True)        # the product's second layer
    add("l1_c3", 35, 39, 39, 128, 0, 8, 4, 3, 12, "b01 g11", first=True, own_out=True)   # ... and its first
    add("c1", 9, 39, 128, 64, 1, 8, 1, 1, 32, "g10 b01")
    add("c2", 34, 39, 128, 100, 1, 8, 1, 2, 32, "d00 b11")
    add("fs1", 6, 39, 128, 50, 0, 8, 1, 1, 32, "b00 g11")                          # N % 4 != 0 at H > 64: 8 waves, one field part
    add("fs1_7", 5, 39, 100, 50, 0, 8, 1, 1, 32, "d01 b10")                        # 7 waves
    add("fs2", 5, 39, 64, 32, 0, 2, 2, 4, 32, "b00 d11", own_out=True)             # HT = 4: two field parts
    add("t5_n2", 7, 39, 80, 24, 1, 2, 1, 4, 32, "g00 b11")                         # tiled at HT = 5 with NSMAX = 2
    add("h48", 4, 7, 48, 16, 0, 2, 4, 4, 12, "b10 d01")                            # the last H of cin_fwd_k<12> and of FS = 4
    add("h49", 4, 7, 49, 16, 0, 2, 2, 4, 32, "b01 g10")                            # the first H of cin_fwd_k<32> and of FS = 2
    add("tiny", 3, 5, 6, 20, 0, 2, 4, 4, 12, "d00 b11")
    add("one", 1, 3, 16, 16, 0, 2, 4, 4, 12, "b00 g11")
    add("b67", 67, 39, 39, 128, 0, 8, 4, 3, 12, "b01 d11", first=True)             # three trips of the 32-stride batch loop
    # (126 + 100 + 128) 16 + 8 * 100 * 16 + 8 * 256 floats = 82 048 B: above 64 KiB, the launcher opts the kernel in
    add("lds82", 5, 100, 128, 126, 0, 8, 1, 1, 32, "b00 d11", optin=1, lds=82048)
    return out


LAYER_CASES = _layer_cases()
LAYER = {c.id: c for c in LAYER_CASES}
assert len(LAYER) == len(LAYER_CASES)
LAYER_IDS = [c.id for c in LAYER_CASES]
# every (data-gradient form, weight-gradient configuration, forward HSMAX) the table must hold; form = (tiled, NSMAX, FS)
FORMS_REQUIRED = {((1, 8, 1), 0, 32), ((0, 8, 4), 3, 12), ((1, 8, 1), 1, 32), ((1, 8, 1), 2, 32), ((0, 8, 1), 1, 32),
                  ((0, 2, 2), 4, 32), ((1, 2, 1), 4, 32), ((0, 2, 4), 4, 12)}
SWEEP_SAME_CFG = "c2"       # configuration 2 with or without a slice: every output bit-identical
SWEEP_OTHER_CFG = "l2_c0"   # configuration 0 becomes 2: another summation order of dW and dc
SWEEP_ROWS, SWEEP_TOUCHED = 5000, 400


def plan_of(c):
    """what rsx_cin_layer_plan must answer for the case, as (out[0], out[1], out[2], out[3], out[5], out[6], out[7])"""
    return (c.hsmax, c.tiled, c.nsmax, c.FS, c.optin, c.cfg, -(-c.H // 16))


def plan_key(p):
    """the same entries of a plan's eight"""
    return (p[0], p[1], p[2], p[3], p[5], p[6], p[7])


def parse_variant(v):
    return v[0], int(v[1]), int(v[2])


class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def draw_layer(cid):
    """float32 CPU tensors, a function of the case alone (shared: never written to).  X0 = 0.5 N(0,1), Xk = 0.5 |N(0,1)|
    (a later layer's input is a relu output; the first layer's is X0 itself); W = 4 N(0,1) / sqrt(F H),
    so pre is of order 1 at every shape and about half of the relus are open; c = 0.3 N(0,1); dout = N(0,1); gs = +-U(0.5, 1.5),
    wout = N(0,1): no example's and no part's share of a sum is negligible; pre_k / pre_0 = N(0,1), the unit prefills of dXk / dX0."""
    c = LAYER[cid]
    g = torch.Generator().manual_seed(c.seed)
    d = Inputs()
    d.X0 = 0.5 * torch.randn(c.B, c.F, D, generator=g)
    d.Xk = d.X0 if c.first else 0.5 * torch.randn(c.B, c.H, D, generator=g).abs()      # a later layer's input is a relu output
    d.W = 4.0 * torch.randn(c.F * c.H, c.N, generator=g) / np.sqrt(c.F * c.H)
    d.c = 0.3 * torch.randn(c.N, generator=g)
    d.dout = torch.randn(c.B, c.N, D, generator=g)
    sign = torch.where(torch.rand(c.B, generator=g) < 0.5, -1.0, 1.0)
    d.gs = sign * (0.5 + torch.rand(c.B, generator=g))
    d.wout = torch.randn(c.N, generator=g)
    d.pre_k = torch.randn(c.B, c.H, D, generator=g)
    d.pre_0 = torch.randn(c.B, c.F, D, generator=g)
    return d


def grad_in(d, mode, dtype=np.float64):
    """g [B,N,D] of a gradient mode, in numpy `dtype`"""
    dout, gs, wout = (t.numpy().astype(dtype) for t in (d.dout, d.gs, d.wout))
    direct = (gs[:, None] * wout[None, :])[:, :, None]
    return {"d": dout, "g": np.broadcast_to(direct, dout.shape).copy(), "b": dout + direct}[mode]


# ------------------------------------------------------------------------------------------------ the layer, three times
def _Z2(X0, Xk):
    B, F, _ = X0.shape
    H = Xk.shape[1]
    Z = X0[:, :, None, :] * Xk[:, None, :, :]                           # [B,F,H,D]
    return np.ascontiguousarray(Z.transpose(0, 3, 1, 2)).reshape(B * D, F * H)


def layer_fwd(X0, Xk, W, c):
    """the reference: the formula as the script writes it (Z, then one matrix product), numpy, in the arrays' own dtype
    -> (pre without bias [B,N,D], out)"""
    B = X0.shape[0]
    pre = (_Z2(X0, Xk) @ W).reshape(B, D, -1).transpose(0, 2, 1)
    return pre, np.maximum(pre + c[None, :, None], 0)


def layer_bwd(X0, Xk, W, mask, g):
    """-> dict(dpre, dXk, dX0, dW, dc); mask = out > 0"""
    B, F, _ = X0.shape
    H = Xk.shape[1]
    dpre = g * mask
    dp2 = np.ascontiguousarray(dpre.transpose(0, 2, 1)).reshape(B * D, -1)
    dZ = (dp2 @ W.T).reshape(B, D, F, H)
    return dict(dpre=dpre, dW=_Z2(X0, Xk).T @ dp2, dc=dpre.sum((0, 2)),
                dXk=np.einsum("bdfh,bfd->bhd", dZ, X0), dX0=np.einsum("bdfh,bhd->bfd", dZ, Xk))


def layer_fwd_einsum(X0, Xk, W, c):
    """restatement 1: numpy einsums in the formulation of csrc/cin.hip's header -- T_f = Xk . W_f summed over h, then
    pre = sum_f X0_f * T_f: two short sums where the script's product is one long one"""
    F, H = X0.shape[1], Xk.shape[1]
    T = np.einsum("bhd,fhn->bndf", Xk, W.reshape(F, H, -1), optimize=True)
    pre = (T * X0.transpose(0, 2, 1)[:, None, :, :]).sum(-1)         # over f, the contiguous axis: numpy's pairwise sum
    return pre, np.maximum(pre + c[None, :, None], 0)


def layer_bwd_einsum(X0, Xk, W, mask, g):
    """U_f = dpre . W_f^T summed over n, then dXk = sum_f X0_f U_f and dX0_f = <Xk, U_f>; dW over (b, d) in one einsum"""
    F, H = X0.shape[1], Xk.shape[1]
    dpre = g * mask
    U = np.einsum("bnd,fhn->bdfh", dpre, W.reshape(F, H, -1), optimize=True)
    return dict(dpre=dpre, dW=np.einsum("bfd,bhd,bnd->fhn", X0, Xk, dpre, optimize=True).reshape(W.shape), dc=dpre.sum((0, 2)),
                dXk=np.einsum("bdfh,bfd->bhd", U, X0), dX0=np.einsum("bdfh,bhd->bfd", U, Xk))


def layer_fwd_torch(X0, Xk, W, c):
    """restatement 2: the same two short sums as torch calls -- a batched matmul per field (K = H), then torch's sum over f"""
    F, H = X0.shape[1], Xk.shape[1]
    T = torch.matmul(Xk.transpose(1, 2)[:, None], W.reshape(F, H, -1)[None])          # [B,F,D,N]
    pre = (X0[:, :, :, None] * T).sum(1).transpose(1, 2)
    return pre, torch.relu(pre + c[None, :, None])


def layer_fwd_chain(X0, Xk, W, c):
    """the script's own chain as torch calls: Z [B,D,F*H], then ONE product with K = F H.  In fp64 under autograd it is the check
    of the reference (tests/test_cin_ref_cpu.py).  In float32 it is NOT a yardstick: a single sum of up to 12 800 terms is the worse
    fp32 algorithm (5.9e-7 of max|ref| at l1_c3, 1.1e-6 through numpy's einsum), and four times that is past the bars the
    project holds this contraction to"""
    B, F, _ = X0.shape
    H = Xk.shape[1]
    Z = (X0.transpose(1, 2)[:, :, :, None] * Xk.transpose(1, 2)[:, :, None, :]).reshape(B, D, F * H)
    pre = torch.matmul(Z, W).transpose(1, 2)
    return pre, torch.relu(pre + c[None, :, None])


DW_BLOCK = 8      # examples per partial product of the torch restatement's dW


def layer_bwd_torch(X0, Xk, W, mask, g):
    """U = dpre . W^T as one matmul (K = N), the sums over f and h by torch.sum; dW as partial products over blocks of DW_BLOCK
    examples (K = 16 DW_BLOCK: the kernel's waves split the batch likewise), added by torch.sum"""
    B, F, _ = X0.shape
    H = Xk.shape[1]
    dpre = g * mask
    dp = dpre.transpose(1, 2)                                              # [B,D,N]
    U = torch.matmul(dp, W.t()).reshape(B, D, F, H)
    nb = -(-B // DW_BLOCK)
    pad = lambda t: torch.cat([t, t.new_zeros((nb * DW_BLOCK - B,) + t.shape[1:])]) if nb * DW_BLOCK > B else t
    Z = pad(X0.transpose(1, 2)[:, :, :, None] * Xk.transpose(1, 2)[:, :, None, :]).reshape(nb, DW_BLOCK * D, F * H)
    dW = torch.matmul(Z.transpose(1, 2), pad(dp.contiguous()).reshape(nb, DW_BLOCK * D, -1)).sum(0)
    return dict(dpre=dpre, dW=dW, dc=dpre.sum((0, 2)),
                dXk=(U * X0.transpose(1, 2)[:, :, :, None]).sum(2).transpose(1, 2),
                dX0=(U * Xk.transpose(1, 2)[:, :, None, :]).sum(3).transpose(1, 2))


IMPLS = {"ref": (layer_fwd, layer_bwd, np.float64), "einsum": (layer_fwd_einsum, layer_bwd_einsum, np.float32),
         "torch": (layer_fwd_torch, layer_bwd_torch, np.float32)}


def _ops(d, impl):
    dt = IMPLS[impl][2]
    a = [t.numpy().astype(dt) for t in (d.X0, d.Xk, d.W, d.c)]
    return [torch.from_numpy(x) for x in a] if impl == "torch" else a


def _np(x):
    return x.numpy() if isinstance(x, torch.Tensor) else x


@functools.lru_cache(maxsize=None)
def fwd_of(cid, impl="ref"):
    """-> (pre, out) as numpy arrays in the evaluation's dtype (shared: never written to)"""
    pre, out = IMPLS[impl][0](*_ops(draw_layer(cid), impl))
    return np.ascontiguousarray(_np(pre)), np.ascontiguousarray(_np(out))


def out32_of(cid):
    """the backward's `out` input: the float32 rounding of the reference's"""
    return fwd_of(cid)[1].astype(np.float32)


def bwd_of(cid, mode, impl="ref", mask=None):
    """the gradients of one mode, as numpy arrays; mask: out > 0 as a bool array (default: of out32_of)"""
    d = draw_layer(cid)
    dt = IMPLS[impl][2]
    X0, Xk, W, _ = _ops(d, impl)
    mask = (out32_of(cid) > 0) if mask is None else mask
    g, m = grad_in(d, mode, dtype=dt), mask.astype(dt)
    if impl == "torch":
        g, m = torch.from_numpy(g), torch.from_numpy(m)
    return {k: np.ascontiguousarray(_np(v)) for k, v in IMPLS[impl][1](X0, Xk, W, m, g).items()}


@functools.lru_cache(maxsize=None)
def bwd_cached(cid, mode, impl="ref"):
    return bwd_of(cid, mode, impl)


def prefills(d, r):
    """(dXk, dX0) before an accumulating launch: the unit draws scaled to the gradients' rms, so that neither hides the other"""
    return ((d.pre_k.numpy() * np.sqrt((r["dXk"] ** 2).mean())).astype(np.float32),
            (d.pre_0.numpy() * np.sqrt((r["dX0"] ** 2).mean())).astype(np.float32))


def expected(c, r, acc_k, acc_0, pre):
    """{name: array} of one backward run.  first layer: ONE tensor dX = (acc_dxk ? prefill : 0) + dXk + dX0 (acc_dx0 = 1 always)"""
    pk, p0 = pre
    f = lambda a: a.astype(r["dW"].dtype)
    out = {"dW": r["dW"], "dc": r["dc"]}
    if c.first:
        out["dX"] = (f(p0) if acc_k else 0) + r["dXk"] + r["dX0"]
    else:
        out["dXk"] = (f(pk) if acc_k else 0) + r["dXk"]
        out["dX0"] = (f(p0) if acc_0 else 0) + r["dX0"]
    return out


# ------------------------------------------------------------------------------------------------ the head
# (B; layer sizes; nnum; what it exercises)
HeadCase = namedtuple("HeadCase", "id B sizes nnum seed")


def _head_cases():
    def mk(B, sizes, nnum):
        cid = "h%d_%dL%d_%d" % (B, len(sizes), sizes[0], nnum)
        return HeadCase(cid, B, tuple(sizes), nnum, zlib.crc32(cid.encode()))
    return [mk(1, (16,), 0),               # the smallest case
            mk(7, (128, 128), 13),         # the product's shape
            mk(131, (20, 10, 10), 13),     # second trip of the 128-stride batch loop; tiles clipped to their layer
            mk(515, (33,), 17),            # second trip of the 512-stride dwnum loop and of its 16-column loop
            mk(5, (8,) * CIN_MAXL, 0),     # CIN_MAXL layers
            mk(3, (130,), 0)]              # second trip of the forward's 512-float4 loop (the ABI sets no limit on a layer's width)


HEAD_CASES = _head_cases()
HEAD = {c.id: c for c in HEAD_CASES}
assert len(HEAD) == len(HEAD_CASES)
HEAD_IDS = [c.id for c in HEAD_CASES]


def _draw_head(c, seed):
    g = torch.Generator().manual_seed(seed)
    d = Inputs()
    tot = sum(c.sizes)
    d.maps = [torch.relu(torch.randn(c.B, n, D, generator=g)) for n in c.sizes]
    w = torch.randn(tot, generator=g)
    d.Wout = 2.0 * (w - w.mean()) / np.sqrt(16.0 * tot)
    d.bout = torch.tensor([0.1])
    sg = lambda: torch.where(torch.rand(c.B, generator=g) < 0.25, -1.0, 1.0)
    d.gy = sg() * (0.5 + torch.rand(c.B, generator=g))
    d.logx = 2.0 + torch.randn(c.B, max(c.nnum, 1), generator=g)[:, :c.nnum].contiguous()
    d.g_lin = sg() * (0.5 + torch.rand(c.B, generator=g)) * 1e-2
    return d


@functools.lru_cache(maxsize=None)
def draw_head(cid):
    """maps = relu(N(0,1)) (they are relu outputs); Wout = 2 N(0,1) / sqrt(16 tot) made zero-sum (the maps' common mean must not set
    y's sign for the whole batch), bout = 0.1: the logit is of order 1 and about half of the examples have y exactly 0.
    gy = +-U(0.5, 1.5) and g_lin = +-U(0.5, 1.5) * 1e-2, a quarter of them negative (the loss's gradient: the sign of label - p at
    Criteo's label rate), so the batch sums are not the remainder of a cancellation; logx = N(2, 1).
    The draw is the first of seed, seed + 1, ... whose largest y is at least 1 and, from three examples on, which has a y that is
    exactly 0: in a batch of three a single nearly cancelled logit would otherwise set the scale the tensor is judged on.
    y_bwd, the backward's y input: the float32 rounding of the reference's y with every seventh example (from 3) set to -0.5 and
    (from 5) to 0 -- y < 0 never leaves the forward, but the ABI takes any y, and the gate is y > 0."""
    c = HEAD[cid]
    for bump in range(64):
        d = _draw_head(c, c.seed + bump)
        y = head_fwd(d, "ref")
        if y.max() >= 1.0 and (c.B < 3 or bool((y == 0).any())):
            break
    else:
        raise AssertionError(cid)
    d.y_bwd = y.astype(np.float32)
    d.y_bwd[3::7] = -0.5
    d.y_bwd[5::7] = 0.0
    return d


def head_fwd(d, impl="ref"):
    """y [B] as numpy.  ref: fp64 numpy; einsum: float32 numpy, one einsum per layer; torch: float32, the script's concat, reduce_sum and
    dense as torch calls"""
    dt = np.float64 if impl == "ref" else np.float32
    W, b = d.Wout.numpy().astype(dt), d.bout.numpy().astype(dt)
    if impl == "torch":
        S = torch.cat([torch.from_numpy(m.numpy().astype(dt)) for m in d.maps], 1).sum(-1)
        return torch.relu(S @ torch.from_numpy(W) + torch.from_numpy(b)).numpy()
    off, s = 0, np.zeros(d.maps[0].shape[0], dt)
    for m in d.maps:
        n = m.shape[1]
        mm = m.numpy().astype(dt)
        s = s + ((mm.sum(2) * W[None, off:off + n]).sum(1))
        off += n
    return np.maximum(s + b, 0)


def head_bwd(d, impl="ref", y=None, gate=lambda y: y > 0, keep=None):
    """-> dict(gs, dWout, dbout, dwnum (None without numeric columns)) as numpy; y: the backward's y input (default d.y_bwd).
    gate / keep: the CPU test's teeth (another gate; a boolean mask [B] of the examples the sums over the batch take)"""
    dt = np.float64 if impl == "ref" else np.float32
    y = d.y_bwd if y is None else y
    gs = d.gy.numpy().astype(dt) * gate(y).astype(dt)
    k = np.ones(len(gs), bool) if keep is None else keep
    maps = [m.numpy().astype(dt) for m in d.maps]
    logx, gl = d.logx.numpy().astype(dt), d.g_lin.numpy().astype(dt)
    if impl == "torch":
        S = torch.cat([torch.from_numpy(m) for m in maps], 1).sum(-1)
        tg, k = torch.from_numpy(gs), torch.from_numpy(k)
        dW, db = (tg[k][:, None] * S[k]).sum(0).numpy(), tg[k].sum().reshape(1).numpy()
        dwn = (torch.from_numpy(gl)[k][:, None] * torch.from_numpy(logx)[k]).sum(0).numpy() if logx.shape[1] else None
    elif impl == "einsum":
        dW = np.concatenate([np.einsum("b,bn->n", gs[k], m[k].sum(2)) for m in maps])
        db, dwn = gs[k].sum().reshape(1), (np.einsum("b,bj->j", gl[k], logx[k]) if logx.shape[1] else None)
    else:
        dW = np.concatenate([(gs[k][:, None] * m[k].sum(2)).sum(0) for m in maps])
        db, dwn = gs[k].sum().reshape(1), ((logx[k] * gl[k][:, None]).sum(0) if logx.shape[1] else None)
    return dict(gs=gs, dWout=dW, dbout=db, dwnum=dwn)
