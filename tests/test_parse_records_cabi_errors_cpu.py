"""Argument validation of the records device parse (include/rsx.h rsx_criteo_parse_records and its host twin): every call
below is refused BEFORE any HIP call is made or any buffer is read, so the checks run without a GPU.  The device entry gets host
pointers and a null stream -- a launch would fault -- and fake non-NULL addresses that are never read."""
import ctypes as C

import numpy as np
import pytest

EINVAL, EUNSUPPORTED, OK = -1, -3, 0


@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _spec(F=39):
    from recsys_amd import _lib
    sp = _lib.ParseSpec()
    for k in ("slot_src", "slot_rows", "thr", "thr_off", "shift"):
        setattr(sp, k, 0x1000)
    sp.F, sp.null_hash = F, 1
    return sp


def _call(L, entry="dev", **kw):
    F = kw.pop("F", 39)
    a = dict(buf=0x1000, nb=4096, off=0x2000, ln=0x3000, n=64, spec=_spec(F), verify=1, out=0x4000, rows=64,
             stride=64 * 4 + 64 * 4 * F, ids_off=64 * 4, status=0x5000)
    a.update(kw)
    sp = C.byref(a["spec"]) if a["spec"] is not None else None
    args = (a["buf"], a["nb"], a["off"], a["ln"], a["n"], sp, a["verify"], a["out"], a["rows"], a["stride"], a["ids_off"], a["status"])
    if entry == "dev":
        return L.rsx_criteo_parse_records(*args, None)
    return L.rsx_criteo_parse_records_dev_h(*args)


@pytest.mark.parametrize("entry", ["dev", "twin"])
def test_records_parse_refuses_every_bad_argument_before_any_device_call(L, entry):
    for kw in ({"buf": None}, {"off": None}, {"ln": None}, {"spec": None}, {"out": None}, {"status": None},
               {"n": 0}, {"n": -3}, {"rows": 0}, {"rows": -1},
               {"nb": 0}, {"nb": -4}, {"nb": 4095}, {"nb": 1 << 31},
               {"buf": 0x1001}, {"off": 0x2002}, {"ln": 0x3001}, {"out": 0x4002}, {"status": 0x5003},
               {"stride": 64 * 4 + 64 * 4 * 39 - 4},           # too small for a batch
               {"stride": 64 * 4 + 64 * 4 * 39 + 2},           # not a multiple of 4
               {"ids_off": 64 * 4 - 4},                        # the ids would overlap the labels
               {"ids_off": 64 * 4 + 2},
               {"ids_off": 64 * 4 + 16},                       # ... and now the batch no longer fits its stride
               {"F": 0}, {"F": -1}):
        assert _call(L, entry, **kw) == EINVAL, (entry, kw)
    for member in ("slot_src", "slot_rows", "thr", "thr_off", "shift"):
        sp = _spec()
        setattr(sp, member, None)
        assert _call(L, entry, spec=sp) == EINVAL, (entry, member)
    assert _call(L, entry, F=65, stride=1 << 20) == EUNSUPPORTED
    assert _call(L, entry, F=65, stride=8) == EUNSUPPORTED       # (the envelope is answered before the stride is weighed)


def test_records_twin_accepts_what_passes_the_checks(L):
    """The same argument set with real host buffers goes through (bad offsets are a STATUS, not a refusal)."""
    from recsys_amd import _lib
    F = 3
    arr = {"slot_src": np.array([1, 2, 14], np.int32), "slot_rows": np.array([4, 4, 10], np.int32), "thr": np.array([1.0, 2.0], np.float32),
           "thr_off": np.array([0, 1, 2, 2], np.int32), "shift": np.ones(13, np.float32)}
    sp = _lib.ParseSpec()
    for k, v in arr.items():
        setattr(sp, k, v.ctypes.data)
    sp.F, sp.null_hash = F, 7
    buf = np.zeros(64, np.uint8)
    off, ln = np.array([0, 12, 60], np.int32), np.array([4, -1, 4], np.int32)
    out, status = np.full(256, 0xA5, np.uint8), np.full(3, -1, np.int32)
    rc = L.rsx_criteo_parse_records_dev_h(buf.ctypes.data, 64, off.ctypes.data, ln.ctypes.data, 3, C.byref(sp), 1, out.ctypes.data,
                                          4, 64, 16, status.ctypes.data)
    assert rc == OK and list(status) == [_lib.PARSE_BAD_OFFSETS] * 3 and np.all(out == 0xA5)
    assert L.rsx_masked_crc32c_dev_h(None, 5) == 0               # a NULL message of a length: refused, nothing read
