"""The device parse of the input_fn stream without a GPU: the 64-lane masked CRC-32C against the host's, the records kernel's
host twin rsx_criteo_parse_records_dev_h (the same byte-level routines, csrc/parse_device.h, in a plain loop) against
rsx_criteo_parse_h with the label required -- good data at the packed offsets, the mutation corpus, the new status words --
and the whole stream of `criteo_input_fn(device_parse=True)` on numpy buffers with the twin injected as its parse step,
against the default path bit for bit."""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import device_parse_util as U  # noqa: E402
from tests import parse_records_util as R  # noqa: E402

_p = U._p
LONG_LENGTHS = (1023, 1024, 1025, 4095, 4096, 8191, 8192)


@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def lay(L):
    return U.layout()


@pytest.fixture(scope="module")
def arrays(L, lay):
    from recsys_amd.input_pipeline import criteo_parse_spec
    return criteo_parse_spec(lay)


@pytest.fixture(scope="module")
def labelled(lay, arrays):
    return R.with_labels(U.canonical_corpus(lay, arrays))


class _Recording(list):
    """A corpus that remembers which records were drawn from it."""

    def __init__(self, items):
        super().__init__(items)
        self.seen = []

    def __getitem__(self, i):
        self.seen.append(i)
        return list.__getitem__(self, i)


@pytest.fixture(scope="module")
def mutated(labelled):
    """(the 20 000 mutated payloads, the corpus record each one was made from)."""
    rec = _Recording(labelled)
    muts = U.mutation_corpus(rec)
    assert len(rec.seen) == len(muts) >= 20000
    return muts, [labelled[i] for i in rec.seen]


def test_version_status_values_and_bindings(L):
    import re
    from recsys_amd import _lib
    assert L.rsx_version() >= 103
    hdr = open(os.path.join(ROOT, "include", "rsx.h")).read()
    for name, v in (("MISSING_LABEL", 6), ("CRC", 7)):
        assert int(re.search(r"RSX_PARSE_%s = (\d+)" % name, hdr).group(1)) == v == getattr(_lib, "PARSE_" + name)
    assert L.rsx_criteo_parse_records_supported(1, 39) == 1 and L.rsx_criteo_parse_records_supported(1 << 20, 64) == 1
    assert L.rsx_criteo_parse_records_supported(1, 65) == 0 and L.rsx_criteo_parse_records_supported(0, 39) == 0


# ---- CRC ----------------------------------------------------------------------------------------------------------------------
def test_lane_crc_equals_the_host_crc_for_every_length_0_to_300(L):
    rng = np.random.default_rng(11)
    for n in range(0, 301):
        b = rng.integers(0, 256, max(n, 1), dtype=np.uint8)
        assert L.rsx_masked_crc32c_dev_h(_p(b), n) == L.rsx_masked_crc32c_h(_p(b), n), n


@pytest.mark.parametrize("fill", ["random", "zero", "ff"])
def test_lane_crc_equals_the_host_crc_at_the_long_lengths(L, fill):
    rng = np.random.default_rng(12)
    for n in LONG_LENGTHS:
        b = {"random": rng.integers(0, 256, n, dtype=np.uint8), "zero": np.zeros(n, np.uint8), "ff": np.full(n, 255, np.uint8)}[fill]
        assert L.rsx_masked_crc32c_dev_h(_p(b), n) == L.rsx_masked_crc32c_h(_p(b), n), (fill, n)


@pytest.mark.parametrize("fill", ["zero", "ff"])
def test_lane_crc_on_constant_buffers_of_every_short_length(L, fill):
    for n in range(0, 301):
        b = np.full(max(n, 1), 0 if fill == "zero" else 255, np.uint8)
        assert L.rsx_masked_crc32c_dev_h(_p(b), n) == L.rsx_masked_crc32c_h(_p(b), n), (fill, n)


# ---- the twin on good data ------------------------------------------------------------------------------------------------------
def _check_good(records, lay, arrays, batches_per_call):
    """`records` through the twin, 64 rows per batch and `batches_per_call` batches per call (the tail in calls of its own, the
    final partial batch with its own rows_per_batch): 0 declined, ids and label bits the host's, at the packed offsets, and not
    one byte of `out` touched besides."""
    want_lab, want_ids, rc = R.host_parse_labelled(records, lay)
    assert not rc.any(), "the host parser refuses records %s" % np.flatnonzero(rc)[:10]
    rows, per_call = 64, 64 * batches_per_call
    declined = 0
    s = 0
    while s < len(records):
        left = len(records) - s
        m = per_call if left >= per_call else (left // rows * rows or left)
        r = rows if m >= rows else m
        out, status = R.twin_records([R.frame(x) for x in records[s:s + m]], lay, arrays, r)
        declined += int((status != 0).sum())
        lab, ids = R.unpack(out, m, r, lay.F)
        assert np.array_equal(lab, want_lab[s:s + m]) and np.array_equal(ids, want_ids[s:s + m]), s
        mask = R.written_mask(m, r, lay.F, status == 0, out.size)
        assert np.all(out[~mask] == R.SENTINEL), s
        s += m
    assert declined == 0
    return want_lab


@pytest.mark.parametrize("batches_per_call", [2, 3])
def test_twin_on_a_written_shard(tmp_path, lay, arrays, batches_per_call):
    path = R.write_shards(tmp_path, [300])[0]
    recs = R.shard_records(path)
    assert len(recs) == 300
    _check_good(recs, lay, arrays, batches_per_call)


@pytest.mark.parametrize("batches_per_call", [2, 3])
def test_twin_on_the_canonical_corpus_with_labels(lay, arrays, labelled, batches_per_call):
    assert 1900 <= len(labelled) <= 2100 and max(map(len, labelled)) <= 8192
    lab = _check_good(labelled, lay, arrays, batches_per_call)
    assert len(np.unique(lab)) >= 5                              # 0, 1, 0.5, -0 and 3 as bit patterns, packed and unpacked


# ---- mutations ----------------------------------------------------------------------------------------------------------------
def test_mutated_payload_under_its_original_footer_is_a_crc_error(lay, arrays, mutated):
    """What a damaged record on disk looks like: the payload changed, the 4 bytes behind it still those of the original."""
    from recsys_amd import _lib
    muts, orig = mutated
    same = np.array([m == o for m, o in zip(muts, orig)])       # (a byte "replaced" by its own value: nothing was mutated)
    assert same.sum() < 100
    out, status = R.twin_records([R.frame(m, footer_of=o) for m, o in zip(muts, orig)], lay, arrays, 64, verify_crc=1)
    assert np.all(status[~same] == _lib.PARSE_CRC), np.unique(status[~same], return_counts=True)
    assert np.all(status[same] == 0)
    mask = R.written_mask(len(muts), 64, lay.F, same, out.size)
    assert np.all(out[~mask] == R.SENTINEL)


def test_mutated_header_is_a_crc_error(lay, arrays, labelled):
    from recsys_amd import _lib
    rng = np.random.default_rng(6)
    framed = []
    for i in range(2000):
        f = bytearray(R.frame(labelled[i % len(labelled)]))
        f[int(rng.integers(12))] ^= 1 << int(rng.integers(8))    # the length or its CRC
        framed.append(bytes(f))
    out, status = R.twin_records(framed, lay, arrays, 64, verify_crc=1)
    assert np.all(status == _lib.PARSE_CRC) and np.all(out == R.SENTINEL)
    # and a length field that differs from rec_len under a header CRC that is right for it
    rec = labelled[3]
    out, status = R.twin_records([R.frame(rec, length=len(rec) + 1), R.frame(rec)], lay, arrays, 64, verify_crc=1)
    assert list(status) == [_lib.PARSE_CRC, 0]


def test_mutation_corpus_declined_or_the_hosts_ids_and_label(lay, arrays, mutated):
    """20 000 mutations with their footers recomputed, verify_crc off: declined, or exactly the host's ids and label; never
    accepted where the host errors; a declined record leaves its sentinel."""
    muts = mutated[0]
    want_lab, want_ids, rc = R.host_parse_labelled(muts, lay)
    out, status = R.twin_records([R.frame(m) for m in muts], lay, arrays, 64, verify_crc=0)
    acc = status == 0
    lab, ids = R.unpack(out, len(muts), 64, lay.F)
    print("mutation corpus: %d records; twin accepts %d, declines %d (malformed %d, missing numeric %d, missing label %d); host "
          "accepts %d" % (len(muts), int(acc.sum()), int((~acc).sum()), int((status == 1).sum()), int((status == 2).sum()),
                          int((status == 6).sum()), int((rc == 0).sum())))
    assert len(muts) >= 20000
    assert not (acc & (rc != 0)).any(), "accepted where the host errors: %s" % np.flatnonzero(acc & (rc != 0))[:10]
    assert np.array_equal(ids[acc], want_ids[acc]) and np.array_equal(lab[acc], want_lab[acc])
    assert set(np.unique(status)) <= {0, 1, 2, 6}
    assert not (~acc & (rc == 0)).any()                          # the twin mirrors the host: none declined that it accepts
    mask = R.written_mask(len(muts), 64, lay.F, acc, out.size)
    assert np.all(out[~mask] == R.SENTINEL)
    assert acc.sum() > 1000 and (status == 1).sum() > 1000 and (status == 2).sum() > 100
    # with the CRC verified and the footers right, the same answers
    out2, status2 = R.twin_records([R.frame(m) for m in muts[:3000]], lay, arrays, 64, verify_crc=1)
    assert np.array_equal(status2, status[:3000])


def test_missing_label_and_too_long(lay, arrays, labelled):
    from recsys_amd import _lib
    no_label = U.example([U.entry("_c%d" % j, 2.0) for j in range(1, 14)] + [U.entry("_c20", b"abc")])
    no_label_no_numeric = U.example([U.entry("_c%d" % j, 2.0) for j in range(2, 14)])
    long_rec = R.long_record()
    exactly = U.example([U.entry("_c0", 1.0)] + [U.entry("_c%d" % j, 1.0) for j in range(1, 14)] + [U.entry("pad", b"x" * 7000)])
    pad = 8193 - len(exactly) - 3
    just_over = exactly + U._ld(2, b"y" * pad)                   # an unknown field of the Example: 8193 bytes
    assert len(just_over) == 8193
    recs = [labelled[0], no_label, long_rec, just_over, no_label_no_numeric, labelled[1]]
    out, status = R.twin_records([R.frame(r) for r in recs], lay, arrays, 64, verify_crc=1)
    assert list(status) == [0, _lib.PARSE_MISSING_LABEL, _lib.PARSE_TOO_LONG, _lib.PARSE_TOO_LONG, _lib.PARSE_MISSING_NUMERIC, 0]
    mask = R.written_mask(len(recs), 64, lay.F, status == 0, out.size)
    assert np.all(out[~mask] == R.SENTINEL) and not np.all(out[mask] == R.SENTINEL)
    lab, ids, rc = R.host_parse_labelled(recs, lay)
    assert list(rc != 0) == [False, True, False, False, True, False]          # the host: no label is an error, 9 KB is fine


# ---- the stream, on numpy buffers ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shards(tmp_path_factory, L):
    return R.write_shards(tmp_path_factory.mktemp("shards"), [150, 107])


def _same_stream(files, lay, arrays, **kw):
    from recsys_amd.input_pipeline import DeviceFeatures, criteo_input_fn
    a = list(criteo_input_fn(files, layout=lay, **kw))
    b = list(criteo_input_fn(files, layout=lay, device_parse=True, parse_step=R.twin_parse_step(lay, arrays), **kw))
    assert len(a) == len(b) and len(a) > 0
    for (fa, la), (fb, lb) in zip(a, b):
        assert isinstance(fb, DeviceFeatures) and set(fb) == {"ids"}            # no cont_log: nothing can read stale zeros
        assert fb["ids"].dtype == np.int32 and lb.dtype == np.float32 and lb.shape == (fb["ids"].shape[0], 1)
        assert np.array_equal(fa["ids"], fb["ids"]) and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    return [x[1].shape[0] for x in b]


def test_stream_equals_the_default_path_two_epochs(shards, lay, arrays):
    assert _same_stream(shards, lay, arrays, batch_size=64, num_epochs=2) == [64, 64, 64, 64, 1] * 2


def test_stream_equals_the_default_path_shuffled(shards, lay, arrays):
    rows = _same_stream(shards, lay, arrays, batch_size=64, num_epochs=3, need_shuffle=True, shuffle_buffer=3, seed=5)
    assert sorted(rows) == sorted([64, 64, 64, 64, 1] * 3) and rows != [64, 64, 64, 64, 1] * 3


@pytest.mark.parametrize("chunk", [1, 3])
def test_stream_equals_the_default_path_whatever_the_chunk(shards, lay, arrays, chunk):
    _same_stream(shards, lay, arrays, batch_size=32, num_epochs=1, parse_chunk_batches=chunk, prefetch=4)


def test_stream_one_batch_across_the_file_boundary(shards, lay, arrays):
    assert _same_stream(shards, lay, arrays, batch_size=257, num_epochs=1) == [257]


def test_stream_one_partial_batch_only(shards, lay, arrays):
    assert _same_stream(shards, lay, arrays, batch_size=300, num_epochs=1) == [257]


def test_stream_a_9kb_record_comes_back_through_the_host(tmp_path, shards, lay, arrays):
    from recsys_amd import input_pipeline as ip
    recs = R.shard_records(shards[0])
    recs[70] = R.long_record()
    path = R.write_framed(str(tmp_path / "part-long"), recs)
    before = dict(ip.device_parse_stats)
    assert _same_stream([path], lay, arrays, batch_size=64, num_epochs=1) == [64, 64, 22]
    assert ip.device_parse_stats["fallback_batches"] == before["fallback_batches"] + 1      # the second batch alone
    assert ip.device_parse_stats["bytes"] > before["bytes"]


def test_stream_a_flipped_payload_byte_raises_as_the_default_path(tmp_path, shards, lay, arrays):
    from recsys_amd._lib import RsxError
    from recsys_amd.input_pipeline import criteo_input_fn
    raw = bytearray(open(shards[0], "rb").read())
    raw[len(raw) // 2] ^= 0x10
    path = str(tmp_path / "part-flipped")
    open(path, "wb").write(bytes(raw))
    with pytest.raises(RsxError) as e_default:
        list(criteo_input_fn([path], 64, num_epochs=1, layout=lay))
    with pytest.raises(RsxError) as e_device:
        list(criteo_input_fn([path], 64, num_epochs=1, layout=lay, device_parse=True, parse_step=R.twin_parse_step(lay, arrays)))
    assert str(e_device.value) == str(e_default.value)
    # a truncated shard raises where the shard is indexed
    open(path, "wb").write(bytes(raw[:len(raw) - 7]))
    with pytest.raises(RsxError):
        list(criteo_input_fn([path], 64, num_epochs=1, layout=lay, device_parse=True, parse_step=R.twin_parse_step(lay, arrays)))


def test_stream_leaves_no_thread_behind_when_the_consumer_breaks_out(shards, lay, arrays):
    from recsys_amd.input_pipeline import criteo_input_fn

    def alive():
        return [t.name for t in threading.enumerate() if t.name.startswith("rsx-")]
    it = criteo_input_fn(shards, 16, num_epochs=-1, layout=lay, device_parse=True, parse_step=R.twin_parse_step(lay, arrays),
                         prefetch=4, parse_chunk_batches=2)
    for i, _ in enumerate(it):
        if i == 5:
            break
    assert alive() == ["rsx-device-parse"]
    it.close()
    assert alive() == []
    it = criteo_input_fn(shards, 16, num_epochs=1, layout=lay, device_parse=True, parse_step=R.twin_parse_step(lay, arrays))
    assert len(list(it)) == 17 and alive() == []                 # exhausted: gone as well


def test_stream_refusals(shards, lay):
    from recsys_amd import deepfm, xdeepfm
    from recsys_amd._lib import RsxError
    from recsys_amd.feature_columns import CriteoLayout, build_model_columns
    from recsys_amd.input_pipeline import DEVICE_PARSE_ONLY, criteo_input_fn
    uid = CriteoLayout.from_columns(build_model_columns(8)[1])
    for call in (lambda: criteo_input_fn(shards, 64, layout=lay, device_parse=True, shard=(0, 2)),
                 lambda: xdeepfm.input_fn(shards, 64, layout=lay, device_parse=True),
                 lambda: deepfm.input_fn(shards, 64, layout=uid, device_parse=True),
                 lambda: criteo_input_fn(shards, 64, layout=uid, device_parse=True)):
        with pytest.raises(RsxError, match=DEVICE_PARSE_ONLY):
            call()
    assert deepfm.define_flags().parse_args([]).device_parse is False
    assert xdeepfm.define_flags().parse_args(["--device_parse", "true"]).device_parse is True
    FLAGS = xdeepfm.define_flags().parse_args(["--device_parse", "true", "--mirror", "false"])
    with pytest.raises(RsxError, match=DEVICE_PARSE_ONLY):
        xdeepfm.run_main(xdeepfm.model_fn, FLAGS, xdeepfm.make_params)
