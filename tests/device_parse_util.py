"""Shared by tests/test_device_parse_cpu.py and tests/test_gpu_device_parse.py: the canonical and the mutation corpus of
serialized Criteo Examples, the host parser and the device parser's host twin over lists of records."""
import ctypes as C
import struct

import numpy as np

from oracle import tfrecord

VALUE_LENGTHS = (0, 1, 3, 4, 7, 8, 9, 16, 17, 32, 33, 64, 65, 200)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def layout():
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    return CriteoLayout.from_columns(build_feature_columns(16)[1])


def spec_struct(arrays):
    """criteo_parse_spec's host arrays -> (rsx_parse_spec over them, the arrays: keep them alive)."""
    from recsys_amd import _lib
    sp = _lib.ParseSpec()
    for k in ("slot_src", "slot_rows", "thr", "thr_off", "shift"):
        setattr(sp, k, arrays[k].ctypes.data)
    sp.F, sp.null_hash = arrays["F"], arrays["null_hash"]
    return sp, arrays


def pack(records):
    """-> (buf uint8 with a length that is a multiple of 4, offs int32 [n + 1])."""
    offs = np.zeros(len(records) + 1, np.int32)
    np.cumsum([len(r) for r in records], out=offs[1:])
    raw = b"".join(records)
    buf = np.zeros((len(raw) + 3) // 4 * 4 + 4, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    return buf, offs


def twin_parse(records, lay, arrays=None):
    """The host twin over `records` -> (ids int32 [n, F], rows that were not written hold -1; status int32 [n])."""
    from recsys_amd import _lib
    from recsys_amd.input_pipeline import criteo_parse_spec
    sp, keep = spec_struct(arrays or criteo_parse_spec(lay))
    buf, offs = pack(records)
    n = len(records)
    ids, status = np.full((n, lay.F), -1, np.int32), np.full(n, -1, np.int32)
    _lib.check(_lib.lib().rsx_criteo_parse_dev_h(_p(buf), buf.size, _p(offs), n, C.byref(sp), _p(ids), _p(status)),
               "rsx_criteo_parse_dev_h")
    return ids, status


def host_parse(records, lay):
    """rsx_criteo_parse_h (label optional), ONE record per call -> (ids int32 [n, F], rc int [n]: 0 or the negative status)."""
    from recsys_amd import _lib
    from recsys_amd.input_pipeline import _CriteoParser
    cp = _CriteoParser(lay, 1, label_optional=True)
    L = _lib.lib()
    n = len(records)
    ids, rc = np.full((n, lay.F), -1, np.int32), np.zeros(n, np.int64)
    label, cont, row = np.empty((1, 1), np.float32), np.empty((1, 13), np.float32), np.empty((1, lay.F), np.int32)
    off0 = np.zeros(1, np.int64)
    for i, r in enumerate(records):
        buf = np.frombuffer(r, np.uint8) if len(r) else np.zeros(1, np.uint8)
        ln = np.array([len(r)], np.int64)
        rc[i] = L.rsx_criteo_parse_h(_p(buf), _p(off0), _p(ln), 1, _p(cp.slot_src), _p(cp.slot_rows), _p(cp.bnd), _p(cp.bnd_off),
                                     _p(cp.shift), cp.F, _p(label), _p(cont), _p(row), cp.threads)
        if rc[i] == 0:
            ids[i] = row[0]
    return ids, rc


# ---- a writer that can do what oracle.tfrecord.encode_example cannot: unpacked floats, duplicated keys, padded varints -------
def _varint(v, pad=0):
    """`pad` extra bytes make an over-long varint of the same value."""
    out = bytearray(tfrecord._varint(v))
    for _ in range(pad):
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def _ld(field, payload, pad=0):
    return _varint((field << 3) | 2, pad) + _varint(len(payload), pad) + payload


def entry(key, value, packed=True, pad=0):
    """One Features.feature entry; value: bytes (bytes_list) or float (float_list, packed or wire type 5)."""
    if isinstance(value, bytes):
        feat = _ld(1, _ld(1, value, pad), pad)
    elif packed:
        feat = _ld(2, _ld(1, struct.pack("<f", value), pad), pad)
    else:
        feat = _ld(2, _varint((1 << 3) | 5, pad) + struct.pack("<f", value), pad)
    return _ld(1, _ld(1, key.encode(), pad) + _ld(2, feat, pad), pad)


def example(entries, pad=0, split=0):
    """entries: encoded map entries -> one Example; split > 0 writes Example.features twice (the entries cut at `split`)."""
    if split:
        return _ld(1, b"".join(entries[:split]), pad) + _ld(1, b"".join(entries[split:]), pad)
    return _ld(1, b"".join(entries), pad)


def threshold_neighbours(lay, arrays):
    """Per numeric field j (1 .. 13): raw values x whose x + shift sits on or next to a threshold of its slot."""
    out = {}
    for s, c in enumerate(lay.columns):
        if c.boundaries is None:
            continue
        j = int(c.key[2:])
        sh = np.float32(c.log_shift)
        xs = []
        for t in arrays["thr"][arrays["thr_off"][s]:arrays["thr_off"][s + 1]]:
            if not np.isfinite(t):
                continue
            x = np.float32(t - sh)
            cand = [x]
            lo = hi = x
            for _ in range(3):
                lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
                cand += [lo, hi]
            xs += [float(v) for v in cand]
        out[j] = xs
    return out


SPECIAL_FLOATS = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), -1.0, -3.0, -4.0, -5.5, 1e-45, 1e-39, 3.4e38, 1.0, 2.0]


def canonical_corpus(lay, arrays, n=2000, seed=20240607):
    """About n valid serving requests covering what the issue lists (see tests/test_device_parse_cpu.py)."""
    from recsys_amd import _lib
    rng = np.random.default_rng(seed)
    near = threshold_neighbours(lay, arrays)

    def numeric(j):
        u = rng.random()
        if u < 0.35:
            return float(near[j][rng.integers(len(near[j]))])
        if u < 0.45:
            return SPECIAL_FLOATS[rng.integers(len(SPECIAL_FLOATS))]
        return float(np.float32(np.floor(np.exp(rng.normal(2, 2))) - (3 if j == 2 else 0)))

    def cat_value():
        ln = VALUE_LENGTHS[rng.integers(len(VALUE_LENGTHS))] if rng.random() < 0.5 else 8
        if ln == 8 and rng.random() < 0.7:
            return ("%08x" % rng.integers(0, 1 << 32)).encode()
        return bytes(rng.integers(0, 256, ln, dtype=np.uint8))

    out = []
    # (1) oracle.tfrecord.encode_example: shuffled order, with / without _c0, 0 .. 26 categoricals absent, unknown keys
    for i in range(n * 2 // 5):
        ex = {"_c%d" % j: [numeric(j)] for j in range(1, 14)}
        absent = set(rng.choice(np.arange(14, 40), i % 27, replace=False).tolist())
        for j in range(14, 40):
            if j not in absent:
                ex["_c%d" % j] = [cat_value()]
        if i % 2:
            ex["_c0"] = [float(i % 3 == 0)]
        for k in range(int(rng.integers(0, 4))):
            ex[("extra%d" % k, "_c40", "_c", "_cx1", "c14", "_c014")[rng.integers(6)]] = [b"zz", [1.5], [7]][rng.integers(3)]
        keys = list(ex)
        rng.shuffle(keys)
        out.append(tfrecord.encode_example({k: ex[k] for k in keys}))
    # (2) the product's own writer (rsx_criteo_encode_h: label first, "NULL" values omitted), unframed
    m = n // 5
    label = (rng.random(m) < 0.3).astype(np.float32)
    cont = np.array([[numeric(j) for j in range(1, 14)] for _ in range(m)], np.float32)
    cats = [[b"NULL" if rng.random() < 0.15 else cat_value() for _ in range(26)] for _ in range(m)]
    flat = [v for row in cats for v in row]
    cb = np.frombuffer(b"".join(flat), np.uint8)
    co = np.concatenate([[0], np.cumsum([len(v) for v in flat])]).astype(np.int64)
    L = _lib.lib()
    need = -int(L.rsx_criteo_encode_h(_p(label), _p(cont), _p(cb), _p(co), m, None, 0)) - 16
    shard = np.zeros(need, np.uint8)
    assert L.rsx_criteo_encode_h(_p(label), _p(cont), _p(cb), _p(co), m, _p(shard), need) == need
    out += list(tfrecord.unframe(shard.tobytes()))
    # (3) hand-written: packed and unpacked floats, duplicated keys (also ones whose later entry yields no value), padded
    # varints, Example.features written twice, more than 64 map entries
    while len(out) < n:
        i = len(out)
        pad = (0, 0, 1, 2)[i % 4]
        ents = [entry("_c%d" % j, numeric(j), packed=bool(rng.integers(2)), pad=pad) for j in range(1, 14)]
        ents += [entry("_c%d" % j, cat_value(), pad=pad) for j in range(14, 40) if rng.random() < 0.8]
        for _ in range(int(rng.integers(0, 5))):                       # duplicates: the last one with a value wins
            j = int(rng.integers(1, 40))
            ents.append(entry("_c%d" % j, numeric(j) if j <= 13 else cat_value(), packed=bool(rng.integers(2)), pad=pad))
        if i % 5 == 0:                                                 # a later duplicate WITHOUT a value changes nothing
            ents.append(entry("_c3", b"bytes where a float belongs", pad=pad))
            ents.append(entry("_c20", 2.5, pad=pad))
            ents.append(_ld(1, _ld(1, b"_c21")))                       # a key without a Feature
        if i % 7 == 0:                                                 # > 64 entries
            ents += [entry("pad%d" % k, b"v%d" % k) for k in range(int(rng.integers(30, 70)))]
            j = int(rng.integers(14, 40))
            ents.append(entry("_c%d" % j, cat_value()))                # ... with a winner in the second round of 64
        order = rng.permutation(len(ents))
        ents = [ents[k] for k in order]
        out.append(example(ents, pad=pad, split=(len(ents) // 2 if i % 3 == 0 else 0)))
    return out


def _length_positions(rec, depth=4):
    """Offsets of the length varints of the wire-type-2 fields, down to `depth` levels (best effort on valid records)."""
    pos = []

    def walk(a, b, d):
        p = a
        try:
            while p < b:
                tag, p = tfrecord._rd_varint(rec, p)
                wt = tag & 7
                if wt == 2:
                    lp = p
                    ln, p = tfrecord._rd_varint(rec, p)
                    if p + ln > b:
                        return
                    pos.append(lp)
                    if d > 1:
                        walk(p, p + ln, d - 1)
                    p += ln
                elif wt == 0:
                    _, p = tfrecord._rd_varint(rec, p)
                elif wt == 5:
                    p += 4
                elif wt == 1:
                    p += 8
                else:
                    return
        except IndexError:
            return
    walk(0, len(rec), depth)
    return pos


def mutation_corpus(corpus, n=20000, seed=77):
    """n mutations of corpus records from a fixed seed: truncations, byte flips, length fields raised or lowered, over-long
    varints (a length or tag byte b -> b | 0x80, 0x00)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        rec = bytearray(corpus[int(rng.integers(len(corpus)))])
        kind = i % 4
        if kind == 0:
            rec = rec[:int(rng.integers(0, len(rec)))]
        elif kind == 1:
            for _ in range(int(rng.integers(1, 4))):
                k = int(rng.integers(len(rec)))
                rec[k] = int(rng.integers(256)) if rng.random() < 0.5 else rec[k] ^ (1 << int(rng.integers(8)))
        else:
            lp = _length_positions(bytes(rec))
            k = lp[int(rng.integers(len(lp)))] if lp and rng.random() < 0.9 else int(rng.integers(len(rec)))
            if kind == 2:
                rec[k] = (rec[k] + int(rng.choice([-5, -2, -1, 1, 2, 5, 64, 127]))) & 0xff
            else:
                k = 0 if rng.random() < 0.1 else (1 if rng.random() < 0.1 else k)     # the outermost tag / length stay valid
                if not rec[k] & 0x80:
                    rec[k:k + 1] = bytes([rec[k] | 0x80, 0])
                else:
                    rec[k] ^= 0x80
        out.append(bytes(rec))
    return out
