"""rsx_predict_dcn without a GPU: the envelope function, the argument refusals (host pointers and a null stream: every check
comes before any device call), and the falsifiability of the GPU tests' fixture (tests/dcn_serving_util.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import dcn_serving_util as U  # noqa: E402

RSX_EINVAL = -1


@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _widths(w):
    return (C.c_int32 * 3)(*w) if w else None


def test_einval_is_the_headers_value():
    hdr = open(os.path.join(ROOT, "include", "rsx.h")).read()
    import re
    m = re.search(r"\bRSX_EINVAL\s*=?\s*(-?\d+)", hdr)
    assert m and int(m.group(1)) == RSX_EINVAL


def test_envelope(L):
    sup = lambda B, F, D, w, Lc, n=None: L.rsx_predict_dcn_supported(B, F, D, len(w) if n is None else n, _widths(w), Lc)
    assert sup(4096, 39, 16, (100, 100), 3) == 1
    assert sup(4096, 5, 16, (32, 18), 1) == 1
    assert sup(4096, 64, 16, (64, 32, 16), 8) == 1
    assert sup(4096, 39, 8, (100, 100), 3) == 0                   # D 8
    assert sup(4096, 65, 16, (100, 100), 3) == 0                  # F 65
    assert sup(4096, 39, 16, (), 3) == 0                          # L 0 (an empty deep_layers is out of scope)
    assert sup(4096, 39, 16, (100, 100, 100), 3, n=4) == 0        # L 4
    assert sup(4096, 39, 16, (100, 100), 0) == 0                  # Lc 0
    assert sup(4096, 39, 16, (100, 100), 9) == 0                  # Lc 9
    assert sup(4096, 39, 16, (18, 32), 3) == 0                    # an inner width that is not a multiple of 4
    assert sup(4096, 39, 16, (100, 260), 3) == 0                  # a last width of 260
    assert sup(4096, 39, 16, (100000, 100), 3) == 0               # a width that overflows LDS
    assert sup(0, 39, 16, (100, 100), 3) == 0


def _aligned(n, dtype=np.float32, shift=0):
    """A host array of n elements whose address is 16-byte aligned, + `shift` bytes."""
    raw = np.zeros(n * np.dtype(dtype).itemsize + 32, np.uint8)
    o = (-raw.ctypes.data) % 16 + shift
    return raw[o:o + n * np.dtype(dtype).itemsize].view(dtype)


def _host_model(F=5, layers=(32, 16), Lc=2):
    from recsys_amd import _lib
    keep = {"tables": _aligned(64 * 16), "row_off": _aligned(F, np.int32), "cross_W": _aligned(Lc * 16 * F),
            "cross_b": _aligned(Lc * 16 * F), "wo": _aligned(layers[-1] + 16 * F), "bo": _aligned(1)}
    m = _lib.PredictDcnModel()
    K = 16 * F
    for l, n in enumerate(layers):
        for v, size in (("W", K * n), ("b", n), ("gamma", n), ("beta", n)):
            keep["%s%d" % (v, l)] = a = _aligned(size)
            getattr(m, v)[l] = a.ctypes.data
        m.widths[l], K = n, n
    for k in ("tables", "row_off", "cross_W", "cross_b", "wo", "bo"):
        setattr(m, k, keep[k].ctypes.data)
    m.bn_eps, m.F, m.D, m.L, m.Lc = 1e-3, F, 16, len(layers), Lc
    return m, keep


def test_argument_refusal_happens_before_any_device_call(L):
    """Host pointers and a null stream: a launch would fault, so RSX_EINVAL must come from the checks alone."""
    m, keep = _host_model()
    ids, prob = _aligned(4 * 5, np.int32), _aligned(4)
    call = lambda mm, i, p, B: L.rsx_predict_dcn(C.byref(mm) if mm is not None else None, i, p, B, None)
    pi, pp = ids.ctypes.data, prob.ctypes.data
    assert call(None, pi, pp, 4) == RSX_EINVAL
    assert call(m, None, pp, 4) == RSX_EINVAL
    assert call(m, pi, None, 4) == RSX_EINVAL
    assert call(m, pi, pp, 0) == RSX_EINVAL and call(m, pi, pp, -3) == RSX_EINVAL

    def broken(edit):
        mm, kk = _host_model()
        edit(mm, kk)
        return call(mm, pi, pp, 4), kk

    assert broken(lambda mm, kk: setattr(mm, "cross_W", None))[0] == RSX_EINVAL            # a missing cross_W
    assert broken(lambda mm, kk: mm.beta.__setitem__(1, None))[0] == RSX_EINVAL            # gamma without beta
    assert broken(lambda mm, kk: setattr(mm, "bn_eps", float("nan")))[0] == RSX_EINVAL
    assert broken(lambda mm, kk: setattr(mm, "bn_eps", float("inf")))[0] == RSX_EINVAL

    def misalign(mm, kk):
        kk["tables"] = t = _aligned(64 * 16, shift=4)
        assert t.ctypes.data % 16 == 4
        mm.tables = t.ctypes.data
    assert broken(misalign)[0] == RSX_EINVAL                                               # tables not 16-byte aligned


@pytest.mark.parametrize("cols", U.COLS)
@pytest.mark.parametrize("layers,Lc", U.CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_gpu_fixture_is_falsifiable(cols, layers, Lc):
    """Dropping any piece of the cross branch moves the oracle's probabilities by more than 1e-4, ten times the GPU tests'
    bar of 1e-5: a kernel that ignored cross.W, cross.b, the last cross layer or out.W's cross part could not pass them."""
    from tests.parity_util import synth_ids
    P, row_off = U.perturbed_dcn_params(cols, layers, Lc)
    ids = synth_ids(np.random.default_rng(7), 200, row_off)
    base = U.oracle_prob(P, row_off, layers, ids)
    nh = layers[-1]

    def moved(key, rows):
        Q = dict(P)
        Q[key] = P[key].copy()
        Q[key][rows] = 0
        return float(np.abs(U.oracle_prob(Q, row_off, layers, ids) - base).max())

    moves = {"cross.W": moved("cross.W", slice(None)), "cross.b": moved("cross.b", slice(None)),
             "last cross.W": moved("cross.W", slice(Lc - 1, Lc)), "last cross.b": moved("cross.b", slice(Lc - 1, Lc)),
             "out.W cross part": moved("out.W", slice(nh, None))}
    print("dcn fixture %s %s Lc=%d: %s" % (cols, layers, Lc, {k: "%.3g" % v for k, v in moves.items()}))
    for k, v in moves.items():
        assert v > 1e-4, (k, v)
