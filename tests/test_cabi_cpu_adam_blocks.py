"""CPU-only: the workgroup layout rsx_adam_num_blocks_u gives a segment list (csrc/adam_device.h adam_build_args; the host
side reads no device memory).  256 lanes per workgroup; float4 positions per lane: 8 for every kind but DENSE (2) -- and 2
for a VEC_COLD segment of a WINDOW sweep in full-size blocks (window maps given, window_block_u 0 / 8), whose blocks
adam_window_vec_block takes.  Tables: n * d / 4 positions; vectors: n / 4 + 1 (the scalar tail's position)."""
import ctypes as C

import numpy as np
import pytest

T = 256


@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _ceil(a, b):
    return (a + b - 1) // b


class _Mem:
    """Host buffers standing in for device pointers (the layout only checks them for NULL and the maps' spacing)."""

    def __init__(self, n, k):
        self.state = np.zeros(16, np.float32)
        self.maps = np.zeros((k, (n + 4 + 3) // 4 * 4 + 4), np.int32)
        base = self.maps.ctypes.data
        self.shift = (-base) % 16 // 4                  # the maps start on a 16-byte boundary (int4 reads)

    def ptr(self):
        return self.state.ctypes.data

    def map_ptr(self, i):
        return self.maps.ctypes.data + 4 * self.shift + i * self.maps.strides[0]


def _segs(kinds, n, d, nw, mem):
    from recsys_amd import _lib
    arr = (_lib.AdamSeg * len(kinds))()
    for a, kind in zip(arr, kinds):
        a.kind, a.n = kind, n
        a.d = d if kind == _lib.RSX_ADAM_TABLE_TF1_COLD else 0
        a.var = a.m = a.v = mem.ptr()
        a.slot = mem.map_ptr(0)
        for j in range(nw):
            a.slot_w[j] = mem.map_ptr(1 + j)
    return arr


def _expected(kinds, n, d, nw, u):
    from recsys_amd import _lib
    tot = 0
    for kind in kinds:
        if kind == _lib.RSX_ADAM_TABLE_TF1_COLD:
            tot += _ceil(n * (d // 4), T * (u if u in (2, 4) else 8))
        else:
            tot += _ceil(n // 4 + 1, T * (2 if nw > 0 and u in (0, 8) else 8))
    return tot


@pytest.mark.parametrize("n", [3, 2047, 2048, 5135, 8192, 840646])
@pytest.mark.parametrize("nw", [0, 1, 7])
def test_block_counts_of_cold_segment_lists(L, n, nw):
    from recsys_amd import _lib
    V, Tb = _lib.RSX_ADAM_VEC_COLD, _lib.RSX_ADAM_TABLE_TF1_COLD
    mem = _Mem(n, 8)
    for kinds in ([V], [Tb, V], [V, Tb]):
        arr = _segs(kinds, n, 16, nw, mem)
        for u in (0, 8):
            assert L.rsx_adam_num_blocks_u(arr, len(kinds), u) == _expected(kinds, n, 16, nw, u), (kinds, u)
        assert L.rsx_adam_num_blocks(arr, len(kinds)) == _expected(kinds, n, 16, nw, 0)
        if nw > 0:      # the riders' small table blocks: the vector keeps 8 float4 per lane there
            for u in (2, 4):
                assert L.rsx_adam_num_blocks_u(arr, len(kinds), u) == _expected(kinds, n, 16, nw, u), (kinds, u)


def test_counts_without_window_maps_are_2048_float4_per_block(L):
    """nw = 0: every kind but DENSE in blocks of 2 048 float4, as before the window sweep's vector blocks shrank."""
    from recsys_amd import _lib
    mem = _Mem(840646, 1)
    V, Tb = _lib.RSX_ADAM_VEC_COLD, _lib.RSX_ADAM_TABLE_TF1_COLD
    n = 840646
    assert L.rsx_adam_num_blocks(_segs([V], n, 0, 0, mem), 1) == _ceil(n // 4 + 1, 2048) == 103
    assert L.rsx_adam_num_blocks(_segs([Tb], n, 16, 0, mem), 1) == _ceil(n * 4, 2048) == 1642
    assert L.rsx_adam_num_blocks(_segs([V, Tb], n, 16, 0, mem), 2) == 103 + 1642
    assert L.rsx_adam_num_blocks(_segs([Tb, V], n, 16, 0, mem), 2) == 103 + 1642
    for kind in (_lib.RSX_ADAM_VEC_SLOT, _lib.RSX_ADAM_TABLE_TF1):
        arr = _segs([kind], n, 16, 0, mem)
        arr[0].d = 16 if kind == _lib.RSX_ADAM_TABLE_TF1 else 0
        arr[0].g = mem.ptr()
        assert L.rsx_adam_num_blocks(arr, 1) == (1642 if kind == _lib.RSX_ADAM_TABLE_TF1 else 103)


def test_window_vector_blocks_at_criteo_size(L):
    """840 646 first-order weights under 7 window maps: 411 blocks of 512 float4 (103 of 2 048 without maps)."""
    from recsys_amd import _lib
    n = 840646
    mem = _Mem(n, 8)
    arr = _segs([_lib.RSX_ADAM_VEC_COLD, _lib.RSX_ADAM_TABLE_TF1_COLD], n, 16, 7, mem)
    assert L.rsx_adam_num_blocks_u(arr, 2, 0) == 411 + 1642
