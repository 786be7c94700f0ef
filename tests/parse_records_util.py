"""Shared by tests/test_parse_records_cpu.py and tests/test_gpu_parse_records.py: TFRecord framing, the staging of framed
records as the device-parse stream stages them, the host parser with the label required, the kernel's host twin
(rsx_criteo_parse_records_dev_h) over such a staging, and the twin as the stream's injectable parse step."""
import ctypes as C
import os
import struct

import numpy as np

from tests import device_parse_util as U

SENTINEL = 0xA5
_p = U._p


def masked_crc(data):
    from recsys_amd import _lib
    return int(_lib.lib().rsx_masked_crc32c_h(data, len(data)))


def frame(payload, footer_of=None, length=None):
    """u64 length | u32 masked crc of it | payload | u32 masked crc of the payload.  footer_of: the bytes whose CRC goes into the
    footer (a mutated payload under its ORIGINAL footer); length: the length field written (and covered by the header's CRC)."""
    head = struct.pack("<Q", len(payload) if length is None else length)
    return head + struct.pack("<I", masked_crc(head)) + payload + struct.pack("<I", masked_crc(payload if footer_of is None else footer_of))


def stage(framed):
    """framed records -> (buf uint8, a multiple of 4 bytes; rec_off int32 [n]; rec_len int32 [n]): the payload of record r is
    buf[rec_off[r], rec_off[r] + rec_len[r]), behind its 12 header bytes and in front of its 4 footer bytes."""
    sizes = np.array([len(f) for f in framed], np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    raw = b"".join(framed)
    buf = np.zeros((len(raw) + 3) // 4 * 4, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    return buf, (starts + 12).astype(np.int32), (sizes - 16).astype(np.int32)


def packing(rows, F):
    """-> (ids_off, bytes of one batch, batch_stride) as the stream lays a batch of `rows` rows out (PackedBatch's packing)."""
    ids_off = (rows * 4 + 15) & ~15
    nbytes = (ids_off + rows * F * 4 + 15) & ~15
    return ids_off, nbytes, (nbytes + 255) & ~255


def unpack(out, n, rows, F):
    """The packed output of n records -> (label bits uint32 [n], ids int32 [n, F]) as they lie in `out` (uint8)."""
    ids_off, _, stride = packing(rows, F)
    lab, ids = np.empty(n, np.uint32), np.empty((n, F), np.int32)
    for b in range((n + rows - 1) // rows):
        m = min(rows, n - b * rows)
        base = b * stride
        lab[b * rows:b * rows + m] = out[base:base + 4 * m].view(np.uint32)
        ids[b * rows:b * rows + m] = out[base + ids_off:base + ids_off + 4 * F * m].view(np.int32).reshape(m, F)
    return lab, ids


def written_mask(n, rows, F, accepted, size):
    """uint8 mask [size] of the bytes of `out` that the records with accepted[r] own."""
    ids_off, _, stride = packing(rows, F)
    mask = np.zeros(size, bool)
    for r in np.flatnonzero(accepted):
        base, row = (r // rows) * stride, r % rows
        mask[base + 4 * row:base + 4 * row + 4] = True
        mask[base + ids_off + 4 * F * row:base + ids_off + 4 * F * (row + 1)] = True
    return mask


def twin_records(framed, lay, arrays, rows, verify_crc=1):
    """The host twin over framed records, `rows` rows per batch -> (out uint8 over a SENTINEL fill, status int32 [n])."""
    from recsys_amd import _lib
    sp, keep = U.spec_struct(arrays)
    buf, rec_off, rec_len = stage(framed)
    n = len(framed)
    ids_off, _, stride = packing(rows, lay.F)
    out = np.full(((n + rows - 1) // rows) * stride, SENTINEL, np.uint8)
    status = np.full(n, -1, np.int32)
    _lib.check(_lib.lib().rsx_criteo_parse_records_dev_h(_p(buf), buf.size, _p(rec_off), _p(rec_len), n, C.byref(sp), int(verify_crc),
                                                         _p(out), rows, stride, ids_off, _p(status)),
               "rsx_criteo_parse_records_dev_h")
    return out, status


def host_parse_labelled(records, lay):
    """rsx_criteo_parse_h with the label REQUIRED, one record per call -> (label bits uint32 [n], ids int32 [n, F], rc [n])."""
    from recsys_amd import _lib
    from recsys_amd.input_pipeline import _CriteoParser
    cp = _CriteoParser(lay, 1)
    L = _lib.lib()
    n = len(records)
    lab, ids, rc = np.zeros(n, np.uint32), np.full((n, lay.F), -1, np.int32), np.zeros(n, np.int64)
    label, cont, row = np.empty((1, 1), np.float32), np.empty((1, 13), np.float32), np.empty((1, lay.F), np.int32)
    off0 = np.zeros(1, np.int64)
    for i, r in enumerate(records):
        buf = np.frombuffer(r, np.uint8) if len(r) else np.zeros(1, np.uint8)
        ln = np.array([len(r)], np.int64)
        rc[i] = L.rsx_criteo_parse_h(_p(buf), _p(off0), _p(ln), 1, _p(cp.slot_src), _p(cp.slot_rows), _p(cp.bnd), _p(cp.bnd_off),
                                     _p(cp.shift), cp.F, _p(label), _p(cont), _p(row), 1)
        if rc[i] == 0:
            lab[i], ids[i] = label.view(np.uint32)[0, 0], row[0]
    return lab, ids, rc


LABELS = (0.0, 1.0, 1.0, 0.0, 0.5, -0.0, 3.0)


def with_labels(corpus):
    """Every record of the canonical corpus (serving requests, half of them without `_c0`) with a label: one more
    Example.features field holding `_c0` -- packed or unpacked -- behind the rest, so that it is the entry that wins."""
    return [rec + U.example([U.entry("_c0", LABELS[i % len(LABELS)], packed=bool(i % 3))]) for i, rec in enumerate(corpus)]


def long_record(label=1.0):
    """A valid 9 KB record: above the kernel's LDS stage, accepted by the host."""
    return U.example([U.entry("_c0", label)] + [U.entry("_c%d" % j, float(j)) for j in range(1, 14)] + [U.entry("pad", b"x" * 9000)])


def twin_parse_step(lay, arrays=None):
    """The kernel's host twin as criteo_input_fn's `parse_step`: the whole stream on numpy buffers, no GPU."""
    from recsys_amd import _lib
    from recsys_amd.input_pipeline import criteo_parse_spec
    sp, keep = U.spec_struct(arrays or criteo_parse_spec(lay))

    def step(stage_np, n, tab, buf_bytes, verify_crc, rows, n_batches, stride, ids_off):
        assert keep is not None
        out = np.full(n_batches * stride, SENTINEL, np.uint8)
        status = np.full(n, -1, np.int32)
        base = stage_np.ctypes.data
        _lib.check(_lib.lib().rsx_criteo_parse_records_dev_h(base + tab, buf_bytes, base, base + 4 * n, n, C.byref(sp), int(verify_crc),
                                                             _p(out), rows, stride, ids_off, _p(status)),
                   "rsx_criteo_parse_records_dev_h")
        return out, status
    return step


def write_shards(d, sizes, seed=1):
    """Criteo shards of `sizes` records each, written by the product's writer -> their paths."""
    from recsys_amd import synthetic
    from recsys_amd.input_pipeline import write_criteo_shard
    rng = np.random.default_rng(seed)
    paths = []
    for k, n in enumerate(sizes):
        label, cont, cat = synthetic.criteo_raw_batch(rng, n)
        p = os.path.join(str(d), "part-r-%05d" % k)
        write_criteo_shard(p, label, cont, cat)
        paths.append(p)
    return paths


def shard_records(path):
    from oracle import tfrecord
    return list(tfrecord.unframe(open(path, "rb").read()))


def write_framed(path, records):
    open(path, "wb").write(b"".join(frame(r) for r in records))
    return path
