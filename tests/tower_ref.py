"""Reference of the batch-norm tower for tests/test_gpu_tower_bn.py and tests/test_tower_ref_cpu.py: the case table, the
inputs of a case, a plain torch autograd restatement of one FusedTower.train_step / infer (any dtype, any device) and the
documented dropout hash on the host.  Nothing here touches the HIP library, so the CPU suite can import it.
The batch-norm-free tower (Case.bn = False: tests/test_gpu_tower_nobn.py, tests/test_tower_nobn_ref_cpu.py) is the same
restatement without the moments; its tables (NOBN_CASES, FUSED_CASES) are at the end of this file.

The step restated (csrc/tower.hip; deepfm/deepfm.py:100-112 with fm/fm.py:146-149):
    per layer  a = relu(h @ W + b);  h = BN_train(a) * mask / (1 - rate)      (batch moments, biased variance, eps 1e-3)
    head       u = h @ wd + bd;  z = wo[0]*act0(s0 + c0) + wo[1]*s1 + wo[2]*act2(u) + bo   (no wo: z = s0 + u + s1)
    loss       mean sigmoid-CE(z, y);  backward of ce.sum() / (B * replicas)

The ReLU kink.  An fp32 pre-activation within rounding of zero may take the other gate than the fp64 one, and one flipped
element moves a dW column by ~1/sqrt(B) of its size.  The reference therefore applies the gate as a constant 0/1 tensor
(`pre * gate`): the fp64 sign where the fp64 |pre| > TAU, the gate the kernel took (`tower.a[l] > 0`) where |pre| <= TAU.
The share of such elements is a condition of every case (GATE_CAP per layer).  Head rows with |s0 + c0| or |u| <= TAU under
an active relu flag must not exist at all: a case's seed is the first of its SEED_TRIES consecutive seeds without one."""
import functools
from collections import namedtuple

import numpy as np
import torch

BN_EPS = 1e-3
TAU = 1e-5            # |pre-activation| at or below which the reference borrows the kernel's gate
GATE_CAP = 1e-4       # largest admitted share of such elements per layer (expected ~8e-6 at unit scale)
SEED_TRIES = 8
RNG_STEP = 7          # the value of the device step counter in every test
HASH_SEED = 0xD1AD    # the `seed` argument of train_step in every test

# head forms (FusedTower.train_step's head / s0 / c0 / s1 / relu0 / relu2):
#   deepfm  s0 + bias c0, s1, out.W [3], out.b, both relus      (deepfm.py)
#   dcn     the sum head: wd = the first n_last entries of a longer out.W, bd = out.b, s0 only, no relus   (dcn.py)
#   nos0    out.W [3] / out.b with s1 and relu2 but WITHOUT s0 (and so without c0)
#   (tail: the dcn form's out.W has this many entries behind the tower's n_last -- dcn.py: the cross output's weights.  The cases
#   here carry DCN_TAIL = 5 untouched ones; tests/test_gpu_cross_forms.py's rider cases carry the cross layers' dim.)
#   din     (bn = False only) z = s0 + h @ mlp.Wout + mlp.bout, no relus, no out.W; s0 absent when the case's s0 is False  (din.py)
DCN_TAIL = 5
# bn = False: L x [dense(relu) -> dropout] (FusedTower(batch_norm=False)), variables mlp.W{i} / mlp.b{i} / mlp.Wout / mlp.bout.
# fused: the case is run by the one-launch form (csrc/mlp_fused.hip) and follows ITS seed rule (case_seed).
# pad = (l, n): layer l stores widths[l] units of which only the first n exist (din.py stores 50 as 52): the columns n.. of W_l
# and b_l and the rows n.. of the next weight matrix are zero.
Case = namedtuple("Case", "id B k0 widths rate head replicas base_seed tail bn s0 fused pad",
                  defaults=(DCN_TAIL, True, True, False, None))

# The kernel every layer takes, derived from the conditions in rsx_tower_fwd_layer / rsx_tower_head /
# rsx_tower_bwd_layer_defer (csrc/tower.hip), default knobs.  Abbreviations:
#   fwd small = tower_fwd_k;  fwd big<NTW> = tower_fwd_big_k: B >= 1024, K >= 256 (64 from B >= 4096), 16 rows of K padded to 128
#                             (+ 8) floats and 2 K floats of LDS within 64 KB;  NTW = ceil(N / 64)
#   bwd big<NTX,NTD> = tower_bwd_big_k: B >= 1024, K >= 256 (64 from B >= 4096), N % 4 == 0, N <= 128;  NTX = 5 when K > 128
#                             else 2;  NTD = 4 when N <= 64 else 8
#   bwd small<SPLIT> = tower_bwd_k, SPLIT (sb = ceil(B / 512) > 1 dW row blocks) from B >= 1024.  Its d(input) tiles are
#                             grouped (dxg = 4) when N % 4 == 0, N <= 128 and (SPLIT or ceil(K/16) * ceil(B/16) >= 256), else
#                             one-tile (dxg = 0; SPLIT: din_rtw = 4 row tiles per workgroup)
#   head<CPL> = tower_head_k: 4 for N <= 64, 8 for N <= 128, else 16
#   statistics: row partials for B <= 512, the fixed-point rows from B = 513
CASES = [
    # L0 K=20 N=12, L1 K=12 N=7: fwd small; bwd small<false> one-tile (2 * 1 and 1 * 1 tiles < 256), L1 with N % 4 != 0 (scalar
    # operand loads); head<4> with a last width that is no multiple of 4; N < 16 everywhere
    Case("tiny3", 3, 20, (12, 7), 0.0, "deepfm", 1, 1100),
    # the same kernels with two row tiles (17 = 16 + 1)
    Case("tiny17", 17, 20, (12, 7), 0.5, "dcn", 1, 1200),
    # B = 1: variance 0, BN output = beta, d(a) = 0 so dW = db = dX = 0 exactly; kernels as tiny
    Case("b1", 1, 20, (12, 8), 0.0, "deepfm", 1, 1300),
    # deepfm.py's default widths.  fwd small x3.  bwd small<false>: L0 K=260 has 17 * 16 = 272 >= 256 d(input) tiles, so the
    # grouped form is WANTED and refused by N = 200 > 128 (dxg = 0 because of N); L1, L2 K=200: 13 * 16 = 208 < 256, one-tile.
    # head<16> (N = 200)
    Case("default", 250, 260, (200, 200, 200), 0.5, "deepfm", 2, 1400),
    # L0 K=260 N=36: fwd small; bwd small<false> GROUPED (272 >= 256, N % 4 == 0, N <= 128): dxg = 4 with N % 16 != 0, a last
    # group of one column tile (17 = 4 * 4 + 1) and a ragged last row tile (250 = 15 * 16 + 10); head<4>
    Case("grouped", 250, 260, (36,), 0.3, "nos0", 1, 1500),
    # both sides of the row-partial / fixed-point switch; fwd small, bwd small<false> one-tile (6 * 33 and 7 * 33 < 256), head<4>
    Case("edge512", 512, 96, (100, 20), 0.5, "dcn", 1, 1600),
    Case("edge513", 513, 96, (100, 20), 0.0, "deepfm", 1, 1700),
    # fixed-point statistics without the split dW (sb = 1), ragged (520 = 32 * 16 + 8); fwd small x3, bwd small<false> one-tile
    # (6 * 33, 7 * 33, 4 * 33 < 256), head<4>
    Case("fix", 520, 96, (100, 52, 20), 0.5, "nos0", 1, 1800),
    # L0 K=260 N=100: fwd big<2>; bwd big<5,8>, K % 16 != 0, nfg = ceil(261 / 64) = 5 feature groups
    # L1 K=100 N=64:  fwd small (K < 256); bwd small<true> grouped (sb = 3, dxg = 4)
    # L2 K=64  N=200: fwd small; bwd small<true> one-tile (N > 128)
    # L3 K=200 N=7:   fwd small; bwd small<true> one-tile (N % 4 != 0); head<4>
    # 4 layers: the reduces are deferred, jobs of both kinds (big: L0; small: L1-L3) in ONE rsx_tower_reduce_dw_jobs launch
    Case("splitA", 1030, 260, (100, 64, 200, 7), 0.5, "deepfm", 1, 1900),
    # L0 K=256 N=48:  fwd big<1>; bwd big<5,4> (K > 128, N <= 64)
    # L1 K=48  N=256: fwd small (K < 256); bwd small<true> one-tile (N > 128)
    # L2 K=256 N=60:  fwd big<1>; bwd big<5,4>; head<4>
    Case("splitB", 1030, 256, (48, 256, 60), 0.5, "dcn", 2, 2000),
    # L0 K=1024 N=16: the big forward would need 16 * 1032 + 2048 floats = 74 240 B of LDS > 64 KB -> fwd small, paired with
    # bwd big<5,4>: 64 d(input) column tiles = 16 per wave = 4 passes of NTX = 5 (the last with one live tile), 17 feature
    # groups of which the last holds the ones-row alone; head<4>
    Case("wideK", 1030, 1024, (16,), 0.0, "nos0", 1, 2100),
    # B >= 4096: the large-batch kernels from K = 64
    # L0 K=64  N=128: fwd big<2>; bwd big<2,8>
    # L1 K=128 N=192: fwd big<3>; bwd small<true> one-tile (N > 128; sb = 9)
    # L2 K=192 N=256: fwd big<4>; bwd small<true> one-tile
    # L3 K=256 N=68:  fwd big<2>; bwd big<5,8>
    # L4 K=68  N=36:  fwd big<1>; bwd big<2,4>; head<4>
    # 5 layers: nothing is deferred, tower_reduce_dw_big_k (L0, L3, L4) and tower_reduce_dw_k (L1, L2) are launched directly
    Case("b4k", 4100, 64, (128, 192, 256, 68, 36), 0.5, "deepfm", 1, 2200),
]
CASE = {c.id: c for c in CASES}
HASH_CASES = ("tiny17", "default", "splitA", "splitB", "b4k")      # masks=None against the host hash, bit for bit
INFER_CASES = ("default", "fix", "splitA", "b4k")


def param_shapes(case):
    """{name: shape} of the case's DenseArena (the names of deepfm.py / dcn.py)."""
    shapes, d = {}, case.k0
    if not case.bn:
        for i, n in enumerate(case.widths):
            shapes[f"mlp.W{i}"], shapes[f"mlp.b{i}"] = (d, n), (n,)
            d = n
        shapes["mlp.Wout"], shapes["mlp.bout"] = (d, 1), (1,)
        return shapes
    for i, n in enumerate(case.widths):
        shapes[f"dnn.W{i}"], shapes[f"dnn.b{i}"] = (d, n), (n,)
        shapes[f"dnn.gamma{i}"], shapes[f"dnn.beta{i}"] = (n,), (n,)
        d = n
    if case.head == "dcn":
        shapes["out.W"], shapes["out.b"] = (d + case.tail, 1), (1,)
    else:
        shapes["dnn.Wout"], shapes["dnn.bout"] = (d, 1), (1,)
        shapes["out.W"], shapes["out.b"] = (3,), (1,)
        if case.head == "deepfm":
            shapes["b1"] = (1,)
    return shapes


def head_flags(case):
    """(uses s0, uses s1, relu0, relu2)"""
    if case.head == "din":
        return (bool(case.s0), False, False, False)
    return {"deepfm": (True, True, True, True), "dcn": (True, False, False, False), "nos0": (False, True, False, True)}[case.head]


@functools.lru_cache(maxsize=None)
def draw(case, seed):
    """The case's inputs as float32 CPU tensors, a function of (case, seed) alone: weights N(0, 1/sqrt(fan_in)), biases 0.3 N(0,1),
    gamma in 1 +- 0.3 and beta in +- 0.3 (NOT the initial 1 and 0), X ~ N(0,1), s0 / s1 ~ 0.2 N(0,1), labels Bernoulli(0.4), keep masks
    Bernoulli(1 - rate)."""
    g = torch.Generator().manual_seed(seed)
    vals = {}
    for k, shp in param_shapes(case).items():
        leaf = k.split(".")[-1]
        if leaf.startswith("gamma"):
            v = 1.0 + 0.3 * (2.0 * torch.rand(shp, generator=g) - 1.0)
        elif leaf.startswith("beta"):
            v = 0.3 * (2.0 * torch.rand(shp, generator=g) - 1.0)
        elif leaf.startswith("W"):
            v = torch.randn(shp, generator=g) / np.sqrt(shp[0])
        else:
            v = 0.3 * torch.randn(shp, generator=g)
        vals[k] = v
    if case.pad is not None:        # (after the draw: the values of every other entry are those of the unpadded case)
        l, n = case.pad
        vals[f"mlp.W{l}"][:, n:] = 0.0
        vals[f"mlp.b{l}"][n:] = 0.0
        vals[f"mlp.W{l + 1}" if l + 1 < len(case.widths) else "mlp.Wout"][n:] = 0.0
    B = case.B
    d = dict(vals=vals, X=torch.randn(B, case.k0, generator=g), s0=0.2 * torch.randn(B, generator=g),
             s1=0.2 * torch.randn(B, generator=g), y=(torch.rand(B, generator=g) < 0.4).float())
    d["masks"] = [(torch.rand(B, n, generator=g) >= case.rate).float() for n in case.widths] if case.rate > 0.0 else None
    return d


class Ref:
    """What one restated step produced (tensors on the device it ran on)."""
    pass


def run_ref(case, d, *, train=True, masks=None, kernel_a=None, gates=None, dtype=torch.float64, device="cpu", backward=True):
    """The step (train) or the EVAL forward (BN with mean 0 / variance 1, no dropout) in `dtype` on `device`.
    masks: the keep masks of a TRAIN step at rate > 0.  kernel_a: the kernel's relu outputs, lent to the gates of elements with
    |pre| <= TAU (None: the restatement's own sign everywhere).  gates: explicit 0/1 gates per layer (the fp32 restatement takes the
    fp64 run's).  -> Ref with loss, prob, pre[l], a[l], gates[l], near[l] (elements with |pre| <= TAU), head_near (rows on a
    head relu's kink) and, after backward, grads {name}, dX, gs0, gs1."""
    to = lambda t: t.detach().to(device=device, dtype=dtype, copy=True)      # (the drawn inputs are shared: never touched)
    use_s0, use_s1, relu0, relu2 = head_flags(case)
    W = {k: to(v).requires_grad_(train) for k, v in d["vals"].items()}
    X, s0, s1, y = to(d["X"]).requires_grad_(train), to(d["s0"]).requires_grad_(train), to(d["s1"]).requires_grad_(train), to(d["y"])
    r = Ref()
    r.pre, r.a, r.gates, r.near = [], [], [], []
    h = X
    pfx = "dnn" if case.bn else "mlp"
    for l, n in enumerate(case.widths):
        pre = h @ W[f"{pfx}.W{l}"] + W[f"{pfx}.b{l}"]
        if not train:
            a = torch.relu(pre)           # (the forward is continuous at the kink: no gate to choose)
            gate = None
        else:
            with torch.no_grad():
                if gates is not None:
                    gate = gates[l].to(device=device, dtype=dtype)
                else:
                    near = pre.abs() <= TAU
                    if not case.bn:       # (a pad unit's pre-activation is exactly 0: gate 0 on both sides, not a kink)
                        near &= pre != 0
                    own = pre > 0
                    gate = (torch.where(near, kernel_a[l].to(device) > 0, own) if kernel_a is not None else own).to(dtype)
                    r.near.append(int(near.sum()))
            a = pre * gate
        r.pre.append(pre.detach())
        r.a.append(a.detach())
        r.gates.append(gate)
        if not case.bn:           # no moments, train or eval
            h = a
            if train and case.rate > 0.0:
                h = h * to(masks[l]) / (1.0 - case.rate)
        elif train:
            mean = a.mean(0, keepdim=True)
            var = ((a - mean) ** 2).mean(0, keepdim=True)
            h = (a - mean) * torch.rsqrt(var + BN_EPS) * W[f"dnn.gamma{l}"] + W[f"dnn.beta{l}"]
            if case.rate > 0.0:
                h = h * to(masks[l]) / (1.0 - case.rate)
        else:
            h = a * W[f"dnn.gamma{l}"] / np.sqrt(1.0 + BN_EPS) + W[f"dnn.beta{l}"]
    n_last = case.widths[-1]
    if case.head == "din":
        u = h @ W["mlp.Wout"].reshape(-1) + W["mlp.bout"]
        z = (s0 + u) if use_s0 else u
        v0 = None
    elif case.head == "dcn":
        u = h @ W["out.W"].reshape(-1)[:n_last] + W["out.b"]
        z = s0 + u
        v0 = None
    else:
        u = h @ W["dnn.Wout"].reshape(-1) + W["dnn.bout"]
        wo = W["out.W"]
        v0 = (s0 + W["b1"]) if use_s0 else None
        t0 = (torch.relu(v0) if relu0 else v0) if use_s0 else 0.0
        z = wo[0] * t0 + wo[1] * (s1 if use_s1 else 0.0) + wo[2] * (torch.relu(u) if relu2 else u) + W["out.b"]
    with torch.no_grad():
        hn = torch.zeros_like(u, dtype=torch.bool)
        if relu0 and v0 is not None:
            hn |= v0.abs() <= TAU
        if relu2:
            hn |= u.abs() <= TAU
        r.head_near = int(hn.sum())
    ce = torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    r.loss = ce.mean().detach()
    r.prob = torch.sigmoid(z).detach()
    if train and backward:
        (ce.sum() / (case.B * case.replicas)).backward()
        r.grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in W.items()}
        r.dX, r.gs0, r.gs1 = X.grad, s0.grad, s1.grad
    return r


@functools.lru_cache(maxsize=None)
def case_seed(case, device="cpu"):
    """The first of the case's SEED_TRIES consecutive seeds whose fp64 reference alone has no head row on a relu kink.
    A fused case (the one-launch form keeps its activations in LDS: no kernel gate to borrow): the first of FUSED_SEED_TRIES
    consecutive seeds with, in addition, no pre-activation with 0 < |pre| <= TAU at all, under the masks the test runs with."""
    tries = FUSED_SEED_TRIES if case.fused else SEED_TRIES
    for seed in range(case.base_seed, case.base_seed + tries):
        d = draw(case, seed)
        with torch.no_grad():
            r = run_ref(case, d, masks=case_masks(case, d), device=device, backward=False)
        if r.head_near == 0 and (not case.fused or sum(r.near) == 0):
            return seed
    raise AssertionError(f"{case.id}: every seed {case.base_seed}..+{tries - 1} puts a head row within {TAU} of a relu kink"
                         + (" or a pre-activation inside it" if case.fused else ""))


def case_masks(case, d):
    """The keep masks of the case's main comparison: the drawn ones, or the documented hash's for a case that runs with
    masks=None (FUSED_HASH: its seed rule has to hold under THOSE masks)."""
    if case.rate > 0.0 and case.id in FUSED_HASH:
        return hash_masks(case.B, case.widths, case.rate)
    return d["masks"]


# ------------------------------------------------------------------------------------------ the dropout hash on the host
def hash32(x):
    """rsx_hash32 (csrc/drop_device.h) on a uint64 array holding 32-bit values."""
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def hash_masks(B, widths, rate, step=RNG_STEP, seed=HASH_SEED, layer0=0):
    """The keep masks the kernels derive when none is injected: element b * n + col of layer l is dropped when
    hash32(element ^ key) < rate * 2^32, key = hash32(seed ^ step * 0x9E3779B9 ^ (l * 0x85EBCA6B + 0x27220A95)) (32-bit arithmetic;
    the rate is the fp32 value the kernels are handed).  layer0: the layer number of widths[0] (the tower counts from 0; the two
    attention blocks of din.py from 0 and 2)."""
    M = 0xFFFFFFFF
    thresh = np.uint64(int(float(np.float32(rate)) * 2.0 ** 32))
    out = []
    for l, n in enumerate(widths, start=layer0):
        key = hash32(np.array([(seed ^ ((step * 0x9E3779B9) & M) ^ ((l * 0x85EBCA6B + 0x27220A95) & M)) & M]))[0]
        h = hash32((np.arange(B * n, dtype=np.uint64) & np.uint64(M)) ^ key)
        out.append(torch.from_numpy((h >= thresh).astype(np.float32).reshape(B, n)))
    return out


# ------------------------------------------------------------------------------------------ the batch-norm-free tower
FUSED_SEED_TRIES = 32


def _nobn(cid, B, k0, widths, rate, replicas, base_seed, s0=True, fused=False, pad=None):
    return Case(cid, B, k0, widths, rate, "din", replicas, base_seed, DCN_TAIL, False, s0, fused, pad)


# The launch-per-layer form of a batch-norm-free tower (gamma == nullptr in csrc/tower.hip).  Dispatch does not depend on BN
# (rsx_tower_fwd_layer / rsx_tower_bwd_layer_defer: only B, K and N enter), so the derivations are those of CASES above; what is
# new is the branch every kernel takes inside: h = a * mask / (1 - rate) instead of the normalisation, no statistics rows.
NOBN_CASES = [
    # L0 K=20 N=12, L1 K=12 N=7: fwd small; bwd small<false> one-tile, L1 with N % 4 != 0; head<4>, last width no multiple of 4
    _nobn("tiny", 3, 20, (12, 7), 0.0, 1, 3100),
    # the same kernels with two row tiles (17 = 16 + 1), dropout
    _nobn("tiny17", 17, 20, (12, 7), 0.5, 1, 3200, s0=False),
    # B = 1: without BN nothing cancels -- the gradients are NOT zero; kernels as tiny
    _nobn("b1", 1, 20, (12, 8), 0.0, 1, 3300),
    # L0 K=260 N=36: fwd small; bwd small<false> GROUPED (17 * 16 = 272 >= 256 d(input) tiles, N % 4 == 0, N <= 128); head<4>
    _nobn("grouped", 250, 260, (36,), 0.3, 1, 3400),
    # din.py's own tower (stored widths) launch per layer.  B = 1024: L0 K=96, L1 K=100, L2 K=52 all < 256 -> fwd small x3;
    # bwd small<true> (sb = 2) grouped (N % 4 == 0, N <= 128) x3; head<4>; 3 layers: the reduce jobs are deferred
    _nobn("din1024", 1024, 96, (100, 52, 20), 0.5, 2, 3500, pad=(1, 50)),
    # B = 1000 < 1024: fwd small x3; bwd small<false> (sb = 1, direct dW): L0 (6 * 63 = 378 >= 256 d(input) tiles) and L1
    # (7 * 63 = 441) grouped, L2 (4 * 63 = 252 < 256) one-tile; ragged last row tile (1000 = 62 * 16 + 8); head<4>
    _nobn("din1000", 1000, 96, (100, 52, 20), 0.5, 1, 3600, pad=(1, 50)),
    # L0 K=260 N=100: fwd big<2>; bwd big<5,8>, K % 16 != 0
    # L1 K=100 N=64:  fwd small; bwd small<true> grouped (sb = 3)
    # L2 K=64  N=200: fwd small; bwd small<true> one-tile (N > 128)
    # L3 K=200 N=7:   fwd small; bwd small<true> one-tile (N % 4 != 0); head<4>
    # 4 layers: the reduces are deferred, jobs of both kinds in ONE rsx_tower_reduce_dw_jobs launch
    _nobn("splitA", 1030, 260, (100, 64, 200, 7), 0.5, 1, 3700),
    # L0 K=256 N=48: fwd big<1>; bwd big<5,4>.  L1 K=48 N=256: fwd small; bwd small<true> one-tile.  L2 K=256 N=60: fwd big<1>;
    # bwd big<5,4>; head<4>.  replicas 2
    _nobn("splitB", 1030, 256, (48, 256, 60), 0.5, 2, 3800, s0=False),
    # B >= 4096: L0 K=64 N=128 fwd big<2>, bwd big<2,8>; L1 K=128 N=192 fwd big<3>, bwd small<true> one-tile (sb = 9); L2 K=192
    # N=256 fwd big<4>, bwd small<true> one-tile; L3 K=256 N=68 fwd big<2>, bwd big<5,8>; L4 K=68 N=36 fwd big<1>, bwd big<2,4>;
    # head<4>.  5 layers: nothing deferred, both reduce kernels launched directly
    _nobn("b4k", 4100, 64, (128, 192, 256, 68, 36), 0.5, 1, 3900),
    # inside the one-launch form's width envelope but 172 608 B of LDS: default forms, no override -- rsx_mlp_nobn_supported says
    # no and the tower takes the launch-per-layer kernels: fwd small x3, bwd small<false> one-tile (6 * 4, 7 * 4, 7 * 4 < 256), head<4>
    _nobn("fallback", 64, 96, (100, 100, 20), 0.5, 1, 4000),
]
NOBN_CASE = {c.id: c for c in NOBN_CASES}
NOBN_HASH_CASES = ("tiny17", "din1024", "splitA", "splitB", "b4k")     # the big kernels and one small case
NOBN_INFER_CASES = ("grouped", "splitA", "b4k")

# The one-launch form (csrc/mlp_fused.hip): one 16-row tile per workgroup, nwg = ceil(B / 16).  nks = ceil(K / 16) k-steps of
# tile_fwd (K = the layer's input width) and of tile_bwd (K = the layer's OWN width N: d(input) = da . W^T); an odd nks takes the
# tail MFMA group behind the two-accumulator loop, nks = 1 the tail alone.  LDS = mlp_lds_layout's bytes (> 64 KB: the opt-in
# dynamic size).  mlp_reduce_body<32> keeps 32 partials in flight: nwg = 33 is the first batch with a second trip.
FUSED_CASES = [
    # L = 1; fwd nks 1 (tail only), bwd nks 1; N = 4 < 16 (one partly filled column tile); nwg = 1 with ONE live row; 5 KB
    _nobn("f_b1", 1, 16, (4,), 0.0, 1, 5000, fused=True),
    # L = 1; fwd nks 2 (even, no tail), bwd nks 4; N = 64 a multiple of 16; nwg = 1 full; 24 KB
    _nobn("f_l1", 16, 32, (64,), 0.3, 2, 5100, fused=True, s0=False),
    # L = 2; fwd nks 3 (odd) and 3, bwd nks 3 and 3; nwg = 2 with a one-row last tile; 50 880 B: under 64 KB
    _nobn("f_48", 17, 48, (48, 48), 0.5, 1, 5200, fused=True),
    # L = 2; fwd nks 7 (odd) and 7, bwd nks 7 (N = 112) and 1 (N = 4); 250 = 15 * 16 + 10; hash dropout; 101 KB
    _nobn("f_112", 250, 112, (112, 4), 0.5, 1, 5300, fused=True, s0=False),
    # L = 3; N = 4 everywhere, K0 = 16; nwg = 33: the reduce's second trip holds ONE partial
    _nobn("f_33", 520, 16, (4, 4, 4), 0.0, 2, 5400, fused=True),
    # din.py's storage: L = 3; fwd nks 6, 7, 4 and bwd nks 7, 4, 2; N = 100, 52, 20 (none a multiple of 16); 137 856 B; the pad
    # units 50, 51 of layer 1.  B = 1030: nwg = 65 (three trips of the reduce, the last with one partial), explicit masks
    _nobn("f_din", 1030, 96, (100, 52, 20), 0.5, 2, 5500, fused=True, pad=(1, 50)),
    # the same at nwg = 33 with hash dropout and without s0
    _nobn("f_din520", 520, 96, (100, 52, 20), 0.5, 1, 5600, fused=True, s0=False, pad=(1, 50)),
    # the largest admitted layout worth running: 152 640 B; fwd nks 7, 7, 4 and bwd nks 7, 4, 2; N = 112 and 64 multiples of 16
    _nobn("f_max", 1030, 112, (112, 64, 32), 0.0, 1, 5700, fused=True),
]
FUSED_CASE = {c.id: c for c in FUSED_CASES}
FUSED_HASH = ("f_112", "f_din520")             # run with masks=None: the reference takes hash_masks(..., layer0=0)
# the seeds case_seed picks for them (tests/test_tower_nobn_ref_cpu.py pins them: a change of the draw or of the rule shows)
FUSED_SEEDS = {"f_b1": 5000, "f_l1": 5100, "f_48": 5200, "f_112": 5303, "f_33": 5400, "f_din": 5500, "f_din520": 5601,
               "f_max": 5702}
