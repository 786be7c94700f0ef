"""The first-order vector in the stand-alone window sweep (csrc/adam_device.h adam_window_vec_block): 512-float4 blocks,
every load of a block in flight at once, adam_zero_grad1 for the live elements, and two shortcuts under a launch-uniform
gate -- void elements (m = v = +0) are not stored, idle ones (m = +0, v in [+0, +inf)) move v alone.

The reference is never the routine under test: k single-step sweeps (rsx_adam_slice_run without window maps, the IEEE
adam_block) over the union of the window's maps, the beta powers advanced between them as the step would.  Everything is
compared as BIT PATTERNS -- signs of zero and NaN payloads included -- for w1, m_w, v_w and for the tables next to them."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

f32 = np.float32
# the value lists of test_gpu_adam_window.py::test_window_sweep_with_adversarial_state_is_the_bits_of_k_single_sweeps
M_VALS = [0.0, -0.0, 1e-45, -1e-45, 4e-45, -6e-42, 1e-39, -1.2e-38, 2.0 ** -100, -(2.0 ** -90), 2.0 ** -81, 2.0 ** -80,
          -(2.0 ** -79), 1e-20, -3e-12, 1e-7, -2.5e-3, 0.3, -7.0, 2.0 ** 29, 2.0 ** 30, -(2.0 ** 31), np.inf, -np.inf, np.nan]
V_VALS = [0.0, -0.0, 1e-45, 1e-40, 2.0 ** -126, 2.0 ** -100, 2.0 ** -96, 2.0 ** -87, 2.0 ** -86, 2.0 ** -85, 1e-20, 1e-15,
          3e-9, 1e-4, 0.5, 100.0, 2.0 ** 39, 2.0 ** 40, 2.0 ** 41, 1e30, np.inf, np.nan, -1e-4, -3.0]      # (+ negative v)
VAR_VALS = [0.0, -0.0, 1e-45, -1e-40, 2.0 ** -60, -(2.0 ** -25), 2.0 ** -24, -(2.0 ** -23), 1e-5, -0.013, 0.5, -3.0, 1e6,
            np.inf, np.nan]
HYPERS = {"default": {}, "b1_half": dict(b1=0.5), "b1_negative": dict(b1=-0.9)}
SHAPES = [(5, 1031, 4099), (3,), (2048,)]


def _vector_state(n, seed):
    """var, m, v of n elements.  n >= 4 608: elements [0, 1 024) ordinary live state and [1 024, 2 048) live state on the
    bounds of the packed chain's guard (block 0 entirely live, every wave of it on the packed chain), [2 048, 4 096) void
    (block 1 entirely void), the rest the mix.  The mix: the full (m, v) grid of the value lists with var cycling through
    its list, then independent draws from the three lists and from ordinary / idle / void state -- every class next to
    every other inside one wave's 256 elements."""
    rng = np.random.default_rng(seed)
    with np.errstate(over="ignore"):
        mv, vv, xv = np.array(M_VALS, f32), np.array(V_VALS, f32), np.array(VAR_VALS, f32)

    def ordinary(c):
        return (rng.standard_normal(c).astype(f32) * f32(0.05),
                rng.standard_normal(c).astype(f32) * f32(1e-2) * (f32(0.9) ** rng.integers(0, 700, c)).astype(f32),
                (rng.random(c).astype(f32) * f32(1e-2)) ** 2 + f32(1e-12))

    def mix(c):
        var, m, v = ordinary(c)
        gm, gv = (x.reshape(-1) for x in np.meshgrid(mv, vv, indexing="ij"))
        g = min(c, len(gm))
        order = rng.permutation(len(gm))[:g]
        m[:g], v[:g], var[:g] = gm[order], gv[order], xv[np.arange(g) % len(xv)]
        kind = rng.integers(0, 6, c)
        kind[:g] = -1
        for arr, vals in ((var, xv), (m, mv), (v, vv)):     # 0: all three from the lists; 1: one of them
            pick = vals[rng.integers(0, len(vals), c)]
            one = rng.integers(0, 3, c) == (0 if arr is var else 1 if arr is m else 2)
            sel = (kind == 0) | ((kind == 1) & one)
            arr[sel] = pick[sel]
        m[(kind == 2) | (kind == 3)] = 0.0                    # 2: idle (m = +0 over an ordinary v); 3: void
        v[kind == 3] = 0.0
        m[(kind == 4) & (rng.random(c) < 0.3)] = -0.0         # 4 / 5: ordinary live, some with m = -0
        return var, m, v

    def bounds(c):
        """State that passes adam_win_guard1 AT its bounds, so that (with block 0's ordinary half) every wave of block 0 takes
        the PACKED chain under the default hyper-parameters: v = 2^-86 and 2^40, |m| = m_lo = 2^-90 / min alpha (for k = 8,
        and a few ulp around it: below it the element is the guard's tiny-m case) and 2^30, denormal m and m = -0 -- all
        over |var| >= 2^-24, which the tiny-m case needs."""
        p1, p2 = f32(1.0), f32(1.0)
        amin = None
        for _ in range(8):
            p1, p2 = f32(p1 * f32(0.9)), f32(p2 * f32(0.999))
            al = f32(f32(1e-3) * np.sqrt(f32(1.0) - p2, dtype=f32) / (f32(1.0) - p1))
            amin = al if amin is None else min(amin, al)
        m_lo = f32(f32(2.0 ** -90) / amin)
        ulps = [np.nextafter(m_lo, f32(np.inf), dtype=f32), np.nextafter(m_lo, f32(0), dtype=f32), f32(m_lo * f32(4.0))]
        ms = np.array([m_lo, -m_lo] + ulps + [-ulps[0], 2.0 ** 30, -(2.0 ** 30), 2.0 ** 29, 1e-45, -6e-42, 1e-39, -1.2e-38,
                       -0.0, 2.0 ** -100, 3e-3, -0.2], f32)
        vs = np.array([2.0 ** -86, 2.0 ** 40, np.nextafter(f32(2.0 ** -86), f32(1)), np.nextafter(f32(2.0 ** 40), f32(0)),
                       2.0 ** -85, 2.0 ** 39, 1e-20, 3e-9, 1e-4, 100.0], f32)
        xs = np.array([2.0 ** -24, -(2.0 ** -23), -(2.0 ** -24), 1e-5, -0.013, 0.5, -3.0, 1e6], f32)
        gm, gv = (x.reshape(-1) for x in np.meshgrid(ms, vs, indexing="ij"))
        idx = np.arange(c)
        return xs[idx % len(xs)].copy(), gm[idx % len(gm)].copy(), gv[idx % len(gv)].copy()

    if n >= 4608:
        # block 0 = float4 0 .. 511; its wave w takes elements [256 w, 256 w + 256) and [1024 + 256 w, 1024 + 256 w + 256)
        blk0 = [np.concatenate([o, b]) for o, b in zip(ordinary(1024), bounds(1024))]
        parts = [blk0, ordinary(2048), mix(n - 4096)]
        parts[1][1][:] = 0.0
        parts[1][2][:] = 0.0
        var, m, v = (np.concatenate([p[i] for p in parts]) for i in range(3))
        # the scalar tail (n % 4 elements): a live one, an idle one, whatever the mix put last
        t = n // 4 * 4
        if n - t >= 2:
            m[t], v[t] = f32(-3e-3), f32(2e-5)
            m[t + 1], v[t + 1] = f32(0.0), f32(7e-6)
        return var, m, v
    return mix(n)


def _maps(n, k, touch, seed):
    """k slot maps over n elements (>= 0: the step touches the element).  'mixed': ~8 elements per step (a batch of 8), one
    element touched at step 0 only, one at step k - 1 only, one at several steps -- in the mix, one of them in the scalar
    tail where there is one.  'none': nothing touched."""
    maps = np.full((k, n), -1, np.int32)
    if touch == "none":
        return maps
    rng = np.random.default_rng(1000 + seed)
    special = rng.permutation(np.arange(n - min(n, 600), n))[:3] if n > 8 else np.arange(n)[:3]
    taken = set(int(x) for x in special)
    free = np.array([i for i in range(n) if i not in taken]) if n <= 8 else None
    for i in range(k):
        if n > 8:
            idx = rng.integers(0, n, 8)
            idx = idx[~np.isin(idx, special)]
            maps[i, idx] = np.arange(len(idx))
        elif len(free) and i == 1:
            maps[i, free[:1]] = 5
    if len(special) > 0:
        maps[0, special[0]] = 1
    if len(special) > 1:
        maps[k - 1, special[1]] = 2
    if len(special) > 2:
        maps[[0, k // 2, k - 1], special[2]] = 3
        if n % 4 and n > 8:                                   # one of the scalar tail's elements, at two steps
            maps[[0, k - 1], n - 1] = 4
    return maps


def _hp(hyper):
    h = HYPERS[hyper]
    return dict(lr=h.get("lr", 1e-3), beta1=h.get("b1", 0.9), beta2=h.get("b2", 0.999), eps=h.get("eps", 1e-8))


def _initial(shape, seed):
    n = int(sum(shape))
    var, m, v = _vector_state(n, seed)
    rng = np.random.default_rng(50 + seed)
    D = 16
    tab = rng.standard_normal((n, D)).astype(f32)
    tm = rng.standard_normal((n, D)).astype(f32) * f32(1e-2)
    tv = rng.random((n, D)).astype(f32) * f32(1e-4) + f32(1e-12)
    u = rng.random(n)
    tm[u < 0.5] = 0.0
    tv[u < 0.3] = 0.0
    return [torch.from_numpy(np.ascontiguousarray(x)) for x in (tab, tm, tv, var, m, v)]


def _arena(shape, k, init, maps):
    from recsys_amd.ops import EmbeddingArena
    row_off = np.concatenate([[0], np.cumsum(shape)]).astype(np.int64)
    a = EmbeddingArena(row_off, 16, 8, "cuda", with_w1=True)
    bufs = a.window_bufs(k)
    n = int(row_off[-1])
    for i in range(k):
        bufs[i]["slot"].fill_(-1)
        bufs[i]["slot"][:n].copy_(torch.from_numpy(maps[i]))
    a.select(0)
    _load(a, init)
    return a


def _load(a, init):
    for dst, src in zip((a.tables, a.m_t, a.v_t, a.w1, a.m_w, a.v_w), init):
        dst.copy_(src)


def _read(a):
    torch.cuda.synchronize()
    return [x.cpu().contiguous().view(torch.int32).numpy().copy() for x in (a.tables, a.m_t, a.v_t, a.w1, a.m_w, a.v_w)]


@functools.lru_cache(maxsize=None)
def _reference(shape, k, hyper, touch):
    """k single-step sweeps (no window maps: adam_slice_k, the IEEE adam_block) that skip every element any step touches."""
    from recsys_amd import _lib
    from recsys_amd.ops import AdamTF1
    seed = k + 10 * len(shape)
    init, maps = _initial(shape, seed), _maps(int(sum(shape)), k, touch, seed)
    a = _arena(shape, k, init, maps)
    n = a.R
    hp = _hp(hyper)
    opt = AdamTF1(device="cuda", **hp)
    union = np.where((maps >= 0).any(0), 0, -1).astype(np.int32)
    union = torch.from_numpy(np.concatenate([union, np.full(4, -1, np.int32)])).cuda()
    segs = [dict(kind=_lib.RSX_ADAM_VEC_COLD, n=n, var=a.w1, m=a.m_w, v=a.v_w, slot=union),
            dict(kind=_lib.RSX_ADAM_TABLE_TF1_COLD, d=16, n=n, var=a.tables, m=a.m_t, v=a.v_t, slot=union)]
    for _ in range(k):
        for sl in opt.cold_slices(segs, [1.0]):
            opt.run_slice(sl)
        st = opt.state.cpu().numpy().copy()          # COLD slices never advance the powers: do it as the step would
        st[0], st[1] = f32(st[0] * f32(hp["beta1"])), f32(st[1] * f32(hp["beta2"]))
        opt.state.copy_(torch.from_numpy(st))
    out = _read(a)
    for x in out:
        x.setflags(write=False)
    return init, maps, out


@pytest.mark.parametrize("touch", ["mixed", "none"])
@pytest.mark.parametrize("hyper", list(HYPERS))
@pytest.mark.parametrize("k", [2, 3, 5, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_window_vector_is_the_bits_of_k_single_sweeps(shape, k, hyper, touch):
    from recsys_amd.ops import AdamTF1
    init, maps, want = _reference(shape, k, hyper, touch)
    a = _arena(shape, k, init, maps)
    touched = (maps >= 0).any(0)
    names = ("tables", "m_t", "v_t", "w1", "m_w", "v_w")
    for form in (0, 1):                                        # rsx_adam_slice.window_compact
        _load(a, init)
        opt = AdamTF1(device="cuda", **_hp(hyper))
        cold = a.adam_split_segments(window_k=k)[0][::-1]      # [VEC_COLD, TABLE_TF1_COLD], as the step lists them
        for sl in opt.cold_slices(cold, [1.0]):
            sl.window_compact = form
            opt.run_slice(sl)
        got = _read(a)
        for name, x, y in zip(names, got, want):
            bad = np.flatnonzero((x != y).reshape(len(touched), -1).any(1))
            assert len(bad) == 0, (name, "form %d" % form, len(bad), bad[:8],
                                   [tuple(float(t[i]) for t in init[3:]) for i in bad[:4]])
        # touched elements come back with the bits they had
        for x, x0 in zip(got[3:], init[3:]):
            assert np.array_equal(x[touched], x0.view(torch.int32).numpy()[touched])
    if touch == "mixed" and len(shape) == 3:
        assert 3 <= touched.sum() <= 8 * k + 4 and touched[-1]


def test_window_vector_sliced_and_after_the_tables():
    """The sweep cut into slices at block boundaries, and the segment list in the other order: the vector's blocks are found
    by their own block size wherever they sit in the launch's block index space."""
    from recsys_amd.ops import AdamTF1
    shape, k = SHAPES[0], 8
    init, maps, want = _reference(shape, k, "default", "mixed")
    a = _arena(shape, k, init, maps)
    for order, weights in ((-1, [1.0, 2.0, 0.5]), (1, [1.0]), (1, [3.0, 1.0])):
        _load(a, init)
        opt = AdamTF1(device="cuda", **_hp("default"))
        cold = a.adam_split_segments(window_k=k)[0][::order]
        for sl in opt.cold_slices(cold, weights):
            opt.run_slice(sl)
        for name, x, y in zip(("tables", "m_t", "v_t", "w1", "m_w", "v_w"), _read(a), want):
            assert np.array_equal(x, y), (name, order, weights)
