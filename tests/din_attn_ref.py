"""Reference of the fused DIN attention MLP (csrc/din_attn.hip) for tests/test_gpu_din_attn.py and tests/test_din_attn_ref_cpu.py:
the case table, the dispatch form each case takes, the inputs of a case, a plain torch restatement of the forward and of the
documented backward (any dtype, any device) and the dropout hash on the host.  Nothing here touches the HIP library, so the CPU
suite can import it.

The expression (DinAttnFn's docstring; din/din.py:111-121), per history position m = b * P + p:
    x  = [h, q, h*q, h-q]                      h = H[m], q = q[b]                          [4K]
    a1 = relu(x W0 + b0);   o1 = a1 * mask1 / (1 - rate)                                    [N1]
    a2 = relu(o1 W1 + b1);  o2 = a2 * mask2 / (1 - rate)                                    [N2]
    w  = o2 . W2 + b2
The backward takes a1 / a2 as INPUTS, exactly as rsx_din_attn_bwd does (the kernel's header comment):
    g2 = dw * W2 * drop2 * (a2 > 0);  g1 = (g2 W1^T) * drop1 * (a1 > 0);  dx = g1 W0^T
    dH = dx_h + dx_hq * q + dx_(h-q)  (+ dH0 under accumulate_dH);   dq = sum_p (dx_q + dx_hq * h - dx_(h-q))  (+ dq_add)
    grads = [dW0 | db0 | dW1 | db1 | dW2 | db2]
The GPU test feeds the kernels the fp32 rounding of the fp64 forward's a1 / a2 -- a positive fp64 value stays positive in fp32 at
these magnitudes --, so the kernel's gates (a > 0) ARE the reference's: the ReLU kink needs no threshold here.  With a row list
only the positions with ids > 0 contribute."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import tower_ref

RNG_STEP = 7          # the value of the device step counter in every test
HASH_SEED = 0xD1A77   # the `seed` argument in every test
LAYER0 = 2            # the `layer0` argument in every test: din.py's second attention block (a dropped layer0 shows)
FWD_ROWS, BWD_ROWS, MAX_GRID = 256, 64, 256      # rows per forward / backward block, the persistent grids' cap

# drop: "none" (rate 0), "masks" (injected Bernoulli keep masks) or "hash" (no mask buffers: the kernels' counter hash)
# a_off: a1 / a2 start one float into their buffers (not 16-byte aligned);  w_off: the same for W0 / W1
# scaled: H and q of example b are multiplied by (1/4, 1, 4)[b % 3] and the per-example tensors are compared per example
Case = namedtuple("Case", "id B P K N1 N2 rate drop a_off w_off scaled seed")


def _c(id, B, P, K=32, N1=80, N2=40, rate=0.0, drop="none", a_off=False, w_off=False, scaled=False, seed=0):
    return Case(id, B, P, K, N1, N2, rate, drop, a_off, w_off, scaled, seed)


# The kernels every case takes, derived from the conditions in rsx_din_attn_fwd and attn_bwd_impl (csrc/din_attn.hip), default
# environment -- forms(case) below restates them and tests/test_din_attn_ref_cpu.py asserts that every form is reached:
#   fwd split<KB> = din_attn_fwd_split_k: N1 % 4 == 0, N2 % 4 == 0, H | q | a1 | a2 16-byte aligned;  else fwd fp32<KB> =
#                   din_attn_fwd_k<KB,5,3>.  Both walk 256-row blocks with a grid of at most 256.
#   bwd<KB,VEC>   = din_attn_bwd_k<KB,5,3,VEC>: VEC on the same widths with a1 | a2 aligned; W staging in 16-byte pieces
#                   (stage_matrix4) when VEC and W0 | W1 are aligned, else element-wise (stage_matrix).  64-row blocks,
#                   G = min(256, blocks) workgroups = partials; the finish adds them as 16 waves x per = ceil(G / 16).
CASES = [
    # M = 1: one lane of one wave; G = 1; the P-sum of dq is one term.  split<2>, bwd<2,true>, vec4
    _c("one", 1, 1, seed=100),
    # the forward's 256-row block edge (255 / 256 / 257 rows); f257: P = 1 and B % 4 = 1 in the finish.  split<2>, bwd<2,true>
    _c("f255", 3, 85, seed=110), _c("f256", 4, 64, seed=120), _c("f257", 257, 1, seed=130),
    # the backward's 64-row block edge (63 / 65 rows)
    _c("b63", 7, 9, seed=140), _c("b65", 5, 13, seed=150),
    # K = 16: split<1> (lane-dependent segment select), bwd<1,true>; ng = 16 position groups in the finish, P = 70: the 4-wide
    # P loop is taken once by every group, the tail by groups 0..5 only;  3 forward blocks, 10 backward blocks
    _c("k16", 9, 70, K=16, rate=0.5, drop="masks", seed=160),
    # K = 16 with P < ng: position groups 9..15 add nothing
    _c("k16small", 5, 9, K=16, seed=170),
    # N2 at the envelope: no padding column tile in layer 2
    _c("w8048", 7, 13, N1=80, N2=48, seed=180),
    # whole 16-column tiles only (64 / 32): a whole padding tile in each layer
    _c("w6432", 7, 13, N1=64, N2=32, seed=190),
    # % 4 == 0, % 16 != 0 (76 / 36): a last tile with 3 (76) / 1 (36) of 4 quads valid.  split / bwd VEC at K = 32 and K = 16
    _c("w7636", 7, 13, N1=76, N2=36, rate=0.5, drop="masks", seed=200),
    _c("w7636-k16", 7, 13, K=16, N1=76, N2=36, rate=0.5, drop="masks", seed=210),
    # one quad per layer
    _c("w44", 7, 13, N1=4, N2=4, seed=220),
    # % 4 != 0 (78 / 38): fwd fp32<KB>, bwd<KB,false>, scalar W staging.  K = 32 and K = 16
    _c("w7838", 7, 13, N1=78, N2=38, rate=0.5, drop="masks", seed=230),
    _c("w7838-k16", 7, 13, K=16, N1=78, N2=38, rate=0.5, drop="masks", seed=240),
    # the same kernels with N < 16 and odd (7 / 5); 340 rows: 2 forward blocks, 6 backward blocks
    _c("w75", 20, 17, N1=7, N2=5, seed=250),
    # din.py's widths with a1 / a2 one float into their buffers: fwd fp32<2> and bwd<2,false> AT 80 / 40; hash dropout.
    # 6 400 rows: 25 forward blocks, 100 backward blocks (G = 100, per = 7)
    _c("a_off", 64, 100, rate=0.5, drop="hash", a_off=True, seed=260),
    # W0 / W1 one float into their buffers: bwd<2,true> with scalar W staging; the forward is unaffected (split<2>).
    # M = 1 023: G = 16, per = 1
    _c("w_off", 33, 31, w_off=True, seed=270),
    # G = 17, per = 2: waves 9..15 of the partial reduce are empty
    _c("g17", 35, 31, seed=280),
    # G = 130, per = 9: one 8-wide trip plus a tail of 1
    _c("g130", 130, 64, seed=290),
    # 16 448 rows at K = 16: the backward wraps (257 blocks over 256 workgroups, per = 16); split<1>, bwd<1,true>
    _c("bwrap16", 257, 64, K=16, rate=0.5, drop="masks", seed=300),
    # 65 600 rows: the forward wraps (257 blocks, the last with 4 of its 16 waves live), the backward wraps (1 025 blocks);
    # hash dropout.  Once through split<2> / bwd<2,true>, once (a1 / a2 offset) through fp32<2> / bwd<2,false>
    _c("wrap", 656, 100, rate=0.5, drop="hash", seed=310),
    _c("wrap-a_off", 656, 100, rate=0.5, drop="hash", a_off=True, seed=310),
    # per-example scales 1/4, 1, 4 on H and q, compared per example: an error relative to the small examples' products (a dropped
    # low-order plane product, a wrong plane order in split_mma) shows here and not against the whole tensor's maximum
    _c("scaled", 48, 37, scaled=True, seed=320),
    _c("scaled-k16", 48, 37, K=16, scaled=True, seed=330),
    _c("scaled-a_off", 48, 37, scaled=True, a_off=True, seed=320),
    _c("scaled-k16-a_off", 48, 37, K=16, scaled=True, a_off=True, seed=330),
    # the K = 32 case of the row-list and entry-point variants (with k16): 444 rows, 2 forward blocks, 7 backward blocks
    _c("r1237", 12, 37, rate=0.5, drop="masks", seed=340),
]
CASE = {c.id: c for c in CASES}
LIST_CASES = ("k16", "r1237")                     # the row-list / entry-point variants run on these
ID_MODES = ("anywhere", "zero", "one", "full")    # draw_ids


def _cdiv(a, b):
    return (a + b - 1) // b


def forms(case):
    """The labels of the dispatch forms `case` takes: rsx_din_attn_fwd's and attn_bwd_impl's conditions restated (default
    environment: RSX_DIN_ATTN_SPLIT unset; H, q, dH and the masks are always aligned in the tests)."""
    M, KB = case.B * case.P, case.K // 16
    assert case.K in (16, 32) and 0 < case.N1 <= 80 and 0 < case.N2 <= 48, case.id
    quads = case.N1 % 4 == 0 and case.N2 % 4 == 0
    split = quads and not case.a_off
    vec = quads and not case.a_off
    fwd = "split" if split else "fp32"
    out = ["fwd %s<%d>" % (fwd, KB), "bwd<%d,%s>" % (KB, "true" if vec else "false"),
           "W-staging vec4" if (vec and not case.w_off) else "W-staging scalar"]
    fblk, bblk = _cdiv(M, FWD_ROWS), _cdiv(M, BWD_ROWS)
    G = min(bblk, MAX_GRID)
    out.append("fwd wrap %s" % fwd if fblk > MAX_GRID else "fwd blocks %d <= grid" % fblk)
    out.append("bwd wrap K=%d" % case.K if bblk > MAX_GRID else "bwd blocks %d <= grid" % bblk)
    out += ["G=%d" % G, "per=%d" % _cdiv(G, 16)]
    return out


def n_grads(case):
    return 4 * case.K * case.N1 + case.N1 + case.N1 * case.N2 + 2 * case.N2 + 1


def grad_slices(case):
    """{name: (offset, shape)} of the packed weight-gradient vector [dW0 | db0 | dW1 | db1 | dW2 | db2]."""
    K4, N1, N2 = 4 * case.K, case.N1, case.N2
    out, o = {}, 0
    for name, shape in (("dW0", (K4, N1)), ("db0", (N1,)), ("dW1", (N1, N2)), ("db1", (N2,)), ("dW2", (N2,)), ("db2", (1,))):
        out[name] = (o, shape)
        o += int(np.prod(shape))
    assert o == n_grads(case)
    return out


def draw(case):
    """The case's inputs (see _draw); a case and its a_off / w_off twin share ONE set of tensors: never written to."""
    return _draw(case._replace(id="", a_off=False, w_off=False))


@functools.lru_cache(maxsize=8)
def _draw(case):
    """The inputs as float32 CPU tensors, a function of (shapes, scaled, rate, drop, seed) alone -- so a case and its
    a_off / w_off twin share them.  Weights are scaled for unit-scale pre-activations: H, q ~ N(0,1) (times the per-example scale),
    W0 ~ N(0,1)/sqrt(4K), b0, b1 ~ 0.5 N(0,1), W1 ~ 1.5 N(0,1)/sqrt(N1), W2 ~ N(0,1)/sqrt(N2), b2, dw ~ N(0,1); dH0
    (accumulate_dH) and dq_add ~ N(0,1); keep masks Bernoulli(1 - rate) for drop == "masks"."""
    g = torch.Generator().manual_seed(case.seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    B, P, K, N1, N2 = case.B, case.P, case.K, case.N1, case.N2
    M = B * P
    H, q = rn(M, K), rn(B, K)
    if case.scaled:
        s = torch.tensor([0.25, 1.0, 4.0])[torch.arange(B) % 3]
        H, q = (H.reshape(B, P, K) * s[:, None, None]).reshape(M, K), q * s[:, None]
    d = dict(H=H, q=q, W0=rn(4 * K, N1) / np.sqrt(4 * K), b0=0.5 * rn(N1), W1=1.5 * rn(N1, N2) / np.sqrt(N1), b1=0.5 * rn(N2),
             W2=rn(N2) / np.sqrt(N2), b2=rn(1), dw=rn(M), dH0=rn(M, K), dq_add=rn(B, K), rate=case.rate)
    d["masks"] = [(torch.rand(M, n, generator=g) >= case.rate).float() for n in (N1, N2)] if case.drop == "masks" else None
    return d


def draw_ids(case, mode):
    """History ids [B, P] int32 of a row-list variant.  anywhere: rng.integers(0, 4) -- about a quarter padding, anywhere in the
    row --, example B // 2 all padding and position (0, 0) padding (lanes past the end of the list read row 0: it must be one
    of the rows that "may hold anything");  zero: every id 0 (count 0);  one: a single valid position, in the middle (count 1);
    full: no padding (count M)."""
    rng = np.random.default_rng(case.seed + 7)
    B, P = case.B, case.P
    if mode == "anywhere":
        ids = rng.integers(0, 4, (B, P)).astype(np.int32)
        ids[B // 2] = 0
        ids[0, 0] = 0
    elif mode == "zero":
        ids = np.zeros((B, P), np.int32)
    elif mode == "one":
        ids = np.zeros((B, P), np.int32)
        ids[B // 2, P // 2] = 5
    else:
        assert mode == "full", mode
        ids = rng.integers(1, 50, (B, P)).astype(np.int32)
    return torch.from_numpy(ids)


def masks_of(case, d):
    """The keep masks of the case as float32 CPU tensors (None at rate 0): the drawn ones, or the documented hash over the
    ORIGINAL row (element m * N + n, layers LAYER0 and LAYER0 + 1)."""
    if case.drop == "none":
        return None
    if case.drop == "masks":
        return d["masks"]
    return tower_ref.hash_masks(case.B * case.P, (case.N1, case.N2), case.rate, step=RNG_STEP, seed=HASH_SEED, layer0=LAYER0)


def _att_in(H, q):
    B, K = q.shape
    M = H.shape[0]
    qq = q[:, None, :].expand(B, M // B, K).reshape(M, K)
    return torch.cat([H, qq, H * qq, H - qq], 1), qq


def _drop_scales(d, masks, dtype, device):
    if masks is None or d["rate"] == 0.0:
        return 1.0, 1.0
    return tuple(m.to(device=device, dtype=dtype) / (1.0 - d["rate"]) for m in masks)


def forward_ref(d, masks=None, dtype=torch.float64, device="cpu"):
    """-> a1 [M, N1], a2 [M, N2] (the relu outputs BEFORE dropout), w [M].  Tensors of `d` already in `dtype` on `device` are
    used as they are (autograd leaves stay leaves)."""
    to = lambda k: d[k].to(device=device, dtype=dtype)
    s1, s2 = _drop_scales(d, masks, dtype, device)
    x, _ = _att_in(to("H"), to("q"))
    a1 = torch.relu(x @ to("W0") + to("b0"))
    a2 = torch.relu((a1 * s1) @ to("W1") + to("b1"))
    w = (a2 * s2) @ to("W2") + to("b2")
    return a1, a2, w


def backward_ref(d, a1, a2, masks=None, dtype=torch.float64, device="cpu", ids=None, accumulate_dH=False, dq_add=False):
    """The documented backward from GIVEN activations -> dict dH [M, K], dq [B, K], dW0, db0, dW1, db1, dW2, db2 and `grads`, the
    six packed.  ids ([B, P], a row list's history ids): only positions with ids > 0 contribute -- they are selected, so the
    rest of a1 / a2 / dw may hold anything -- and dH is 0 (dH0 under accumulate_dH) at the others."""
    to = lambda k: d[k].to(device=device, dtype=dtype)
    s1, s2 = _drop_scales(d, masks, dtype, device)
    H, q, W0, W1, W2, dw = to("H"), to("q"), to("W0"), to("W1"), to("W2"), to("dw")
    a1, a2 = a1.to(device=device, dtype=dtype), a2.to(device=device, dtype=dtype)
    B, K = q.shape
    M = H.shape[0]
    if ids is not None:
        valid = (ids.reshape(-1) > 0).to(device)
        zero = torch.zeros((), dtype=dtype, device=device)
        dw, a1, a2 = torch.where(valid, dw, zero), torch.where(valid[:, None], a1, zero), torch.where(valid[:, None], a2, zero)
    x, qq = _att_in(H, q)
    g2 = dw[:, None] * W2[None, :] * s2 * (a2 > 0)
    g1 = (g2 @ W1.T) * s1 * (a1 > 0)
    dx = g1 @ W0.T
    dxh, dxq, dxhq, dxd = dx[:, :K], dx[:, K:2 * K], dx[:, 2 * K:3 * K], dx[:, 3 * K:]
    r = dict(dH=dxh + dxhq * qq + dxd, dq=(dxq + dxhq * H - dxd).reshape(B, M // B, K).sum(1))
    if accumulate_dH:
        r["dH"] = r["dH"] + to("dH0")
    if dq_add:
        r["dq"] = r["dq"] + to("dq_add")
    r.update(dW0=x.T @ g1, db0=g1.sum(0), dW1=(a1 * s1).T @ g2, db1=g2.sum(0), dW2=((a2 * s2) * dw[:, None]).sum(0),
             db2=dw.sum().reshape(1))
    r["grads"] = torch.cat([r[k].reshape(-1) for k in ("dW0", "db0", "dW1", "db1", "dW2", "db2")])
    return r
