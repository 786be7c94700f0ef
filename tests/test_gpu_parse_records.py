"""The device parse of the input_fn stream on the GPU: rsx_criteo_parse_records (csrc/parse_records.hip) through the C ABI
against the host parser and against its host twin (values, status words, untouched bytes), its CRC on payload lengths around
every lane boundary, `criteo_input_fn(device_parse=True)` against the default path bit for bit (with the host fallback and the
corrupt-record error), and Estimator.train / evaluate / predict fed by it against the same run fed by the default path."""
import ctypes as C
import hashlib
import re

import numpy as np
import pytest

from tests import device_parse_util as U
from tests import parse_records_util as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CRC_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 8192)


@pytest.fixture(scope="module")
def lay():
    return U.layout()


@pytest.fixture(scope="module")
def arrays(lay):
    from recsys_amd.input_pipeline import criteo_parse_spec
    return criteo_parse_spec(lay)


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    return R.write_shards(tmp_path_factory.mktemp("shards"), [150, 107])


def _device_spec(arrays):
    from recsys_amd import _lib
    keep = {k: torch.from_numpy(arrays[k]).cuda() for k in ("slot_src", "slot_rows", "thr", "thr_off", "shift")}
    sp = _lib.ParseSpec()
    for k, t in keep.items():
        setattr(sp, k, t.data_ptr())
    sp.F, sp.null_hash = arrays["F"], arrays["null_hash"]
    return sp, keep


def _device_records(framed, lay, arrays, rows, verify_crc=1):
    """The kernel over framed records -> (out uint8 over a SENTINEL fill, status int32 [n] over a fill of -7 with 4 guard words)."""
    from recsys_amd import _lib
    sp, keep = _device_spec(arrays)
    buf, rec_off, rec_len = R.stage(framed)
    n = len(framed)
    ids_off, _, stride = R.packing(rows, lay.F)
    d_buf, d_off, d_len = (torch.from_numpy(x).cuda() for x in (buf, rec_off, rec_len))
    out = torch.full((((n + rows - 1) // rows) * stride,), R.SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 4,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().rsx_criteo_parse_records(d_buf.data_ptr(), buf.size, d_off.data_ptr(), d_len.data_ptr(), n, C.byref(sp),
                                                   int(verify_crc), out.data_ptr(), rows, stride, ids_off, status.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream), "rsx_criteo_parse_records")
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def test_kernel_against_the_host_parser_three_batches_and_a_tail(tmp_path, lay, arrays):
    """3 x 64 + 5 records: three batches in one launch, the 5-row batch in its own; ids and label bits the host's, every status
    OK, every byte outside the written fields still the sentinel, the whole output equal to the twin's."""
    recs = R.shard_records(R.write_shards(tmp_path, [3 * 64 + 5])[0])
    want_lab, want_ids, rc = R.host_parse_labelled(recs, lay)
    assert not rc.any()
    for a, b, rows in ((0, 192, 64), (192, 197, 5)):
        framed = [R.frame(r) for r in recs[a:b]]
        out, status = _device_records(framed, lay, arrays, rows)
        n = b - a
        assert np.all(status[:n] == 0) and np.all(status[n:] == -7), status
        lab, ids = R.unpack(out, n, rows, lay.F)
        assert np.array_equal(ids, want_ids[a:b]) and np.array_equal(lab, want_lab[a:b])
        mask = R.written_mask(n, rows, lay.F, status[:n] == 0, out.size)
        assert np.all(out[~mask] == R.SENTINEL)
        t_out, t_status = R.twin_records(framed, lay, arrays, rows)
        assert np.array_equal(out, t_out) and np.array_equal(status[:n], t_status)


def test_kernel_crc_on_payload_lengths_around_every_lane_boundary(lay, arrays):
    """Random payloads with correct framing: none is a CRC error (they are malformed Examples, which fixes the precedence); with
    the first, a middle or the last payload byte flipped under the unchanged footer, all are.  Statuses equal the twin's."""
    from recsys_amd import _lib
    rng = np.random.default_rng(21)
    good, bad = [], []
    for n in CRC_LENGTHS:
        p = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        good.append(R.frame(p))
        for k in sorted({0, n // 2, n - 1}) if n else ():
            q = bytearray(p)
            q[k] ^= 0x40
            bad.append(R.frame(bytes(q), footer_of=p))
    framed = good + bad
    out, status = _device_records(framed, lay, arrays, 16)
    status = status[:len(framed)]
    assert not np.any(status[:len(good)] == _lib.PARSE_CRC), status[:len(good)]
    assert np.all(status[len(good):] == _lib.PARSE_CRC), status[len(good):]
    t_out, t_status = R.twin_records(framed, lay, arrays, 16)
    assert np.array_equal(status, t_status) and np.array_equal(out, t_out)
    # a real record of every residue of its length mod 4 in front of it (the staging's alignment), CRC on: accepted
    rec = U.example([U.entry("_c0", 1.0)] + [U.entry("_c%d" % j, 1.0) for j in range(1, 14)])
    fr = [R.frame(rec + U._ld(2, b"z" * k)) for k in range(1, 9)]
    out, status = _device_records(fr, lay, arrays, 8)
    assert np.all(status[:8] == 0), status


def test_kernel_declines_as_the_twin_does(lay, arrays):
    """A missing label, a missing numeric, a 9 KB record and a malformed one between good records."""
    from recsys_amd import _lib
    ok = U.example([U.entry("_c0", 1.0)] + [U.entry("_c%d" % j, float(j)) for j in range(1, 14)] + [U.entry("_c20", b"abc")])
    no_label = U.example([U.entry("_c%d" % j, 2.0) for j in range(1, 14)])
    no_numeric = U.example([U.entry("_c0", 1.0)] + [U.entry("_c%d" % j, 2.0) for j in range(2, 14)])
    framed = [R.frame(r) for r in (ok, no_label, ok, no_numeric, R.long_record(), ok[:-3], ok)]
    out, status = _device_records(framed, lay, arrays, 4)
    t_out, t_status = R.twin_records(framed, lay, arrays, 4)
    assert list(t_status) == [0, _lib.PARSE_MISSING_LABEL, 0, _lib.PARSE_MISSING_NUMERIC, _lib.PARSE_TOO_LONG, _lib.PARSE_MALFORMED, 0]
    assert np.array_equal(status[:7], t_status) and np.array_equal(out, t_out)


# ---- the stream -----------------------------------------------------------------------------------------------------------------
def _same_stream(files, lay, **kw):
    from recsys_amd.input_pipeline import DeviceFeatures, criteo_input_fn
    a = list(criteo_input_fn(files, layout=lay, **kw))
    b = list(criteo_input_fn(files, layout=lay, device_parse=True, **kw))
    assert len(a) == len(b) and len(a) > 0
    for (fa, la), (fb, lb) in zip(a, b):
        assert isinstance(fb, DeviceFeatures) and set(fb) == {"ids"} and fb["ids"].is_cuda and lb.is_cuda
        assert fb["ids"].dtype == torch.int32 and lb.dtype == torch.float32 and tuple(lb.shape) == (fb["ids"].shape[0], 1)
        assert np.array_equal(fa["ids"], fb["ids"].cpu().numpy())
        assert np.array_equal(la.view(np.uint32), lb.cpu().numpy().view(np.uint32))
    return [x[1].shape[0] for x in b]


def test_stream_equals_the_default_path(shards, lay):
    from recsys_amd import input_pipeline as ip
    before = dict(ip.device_parse_stats)
    assert _same_stream(shards, lay, batch_size=64, num_epochs=2) == [64, 64, 64, 64, 1] * 2
    assert ip.device_parse_stats["launches"] > before["launches"] and ip.device_parse_stats["fallback_batches"] == before["fallback_batches"]
    rows = _same_stream(shards, lay, batch_size=64, num_epochs=3, need_shuffle=True, shuffle_buffer=3, seed=5)
    assert sorted(rows) == sorted([64, 64, 64, 64, 1] * 3)
    assert _same_stream(shards, lay, batch_size=257, num_epochs=1) == [257]
    assert _same_stream(shards, lay, batch_size=300, num_epochs=1) == [257]
    _same_stream(shards, lay, batch_size=32, num_epochs=1, parse_chunk_batches=3, prefetch=4)


def test_stream_fallback_batch_and_corrupt_record(tmp_path, shards, lay):
    from recsys_amd import input_pipeline as ip
    from recsys_amd._lib import RsxError
    recs = R.shard_records(shards[0])
    recs[70] = R.long_record()
    path = R.write_framed(str(tmp_path / "part-long"), recs)
    before = dict(ip.device_parse_stats)
    assert _same_stream([path], lay, batch_size=64, num_epochs=1) == [64, 64, 22]
    assert ip.device_parse_stats["fallback_batches"] == before["fallback_batches"] + 1
    raw = bytearray(open(shards[0], "rb").read())
    raw[len(raw) // 2] ^= 0x10
    path = str(tmp_path / "part-flipped")
    open(path, "wb").write(bytes(raw))
    with pytest.raises(RsxError) as e_default:
        list(ip.criteo_input_fn([path], 64, num_epochs=1, layout=lay))
    with pytest.raises(RsxError) as e_device:
        list(ip.criteo_input_fn([path], 64, num_epochs=1, layout=lay, device_parse=True))
    assert str(e_device.value) == str(e_default.value)


def test_refusals(shards, lay):
    from recsys_amd import deepfm, xdeepfm
    from recsys_amd._lib import RsxError
    from recsys_amd.feature_columns import CriteoLayout, build_model_columns
    from recsys_amd.input_pipeline import DEVICE_PARSE_ONLY, criteo_input_fn
    uid = CriteoLayout.from_columns(build_model_columns(8)[1])
    for call in (lambda: xdeepfm.input_fn(shards, 64, layout=lay, device_parse=True),
                 lambda: criteo_input_fn(shards, 64, layout=lay, device_parse=True, shard=(0, 2)),
                 lambda: deepfm.input_fn(shards, 64, layout=uid, device_parse=True)):
        with pytest.raises(RsxError, match=DEVICE_PARSE_ONLY):
            call()


def test_default_path_never_touches_the_device_parse(shards, lay, monkeypatch):
    from recsys_amd import input_pipeline as ip

    def boom(*a, **k):
        raise AssertionError("the default path built a device parse step")
    monkeypatch.setattr(ip, "_DeviceParseStep", boom)
    monkeypatch.setattr(ip, "_device_parse_batches", boom)
    before = dict(ip.device_parse_stats)
    assert len(list(ip.criteo_input_fn(shards, 64, num_epochs=1, layout=lay))) == 5
    assert ip.device_parse_stats == before


# ---- training ---------------------------------------------------------------------------------------------------------------
def _state_hash(est):
    h = hashlib.sha256()

    def walk(x):
        if isinstance(x, dict):
            for k in sorted(x):
                h.update(str(k).encode())
                walk(x[k])
        elif isinstance(x, torch.Tensor):
            h.update(x.detach().cpu().contiguous().numpy().tobytes())
        else:
            h.update(repr(x).encode())
    walk(est.store.state_dict())
    return h.hexdigest()


@pytest.mark.parametrize("kind", ["deepfm", "dcn"])
def test_training_evaluation_and_prediction_are_identical(kind, tmp_path, capsys):
    """24 steps at batch 64 through Estimator.train (HIP graphs, the default optimizer window) over shuffled input from two
    small shards, then evaluate over 5 batches and predict: device_parse=True against False.  The ids and labels are the host's
    bits and the batch order is the same, so the logged losses, a hash of every variable, the metrics and the probabilities
    are IDENTICAL -- no tolerance."""
    from recsys_amd import dcn, deepfm
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    from recsys_amd.input_pipeline import criteo_input_fn
    files = R.write_shards(tmp_path, [400, 330], seed=9)
    lin, emb = build_feature_columns(16, {"deepfm": "indicator_all", "dcn": "numeric"}[kind])
    layout = CriteoLayout.from_columns(emb)
    mfn = {"deepfm": deepfm.model_fn, "dcn": dcn.model_fn}[kind]
    res = []
    for flag in (False, True):
        params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-2,
                  "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": 64, "cross_layers": 2 if kind == "dcn" else None}
        est = Estimator(mfn, None, params, RunConfig(device="cuda", seed=3, log_step_count_steps=4))
        capsys.readouterr()
        est.train(lambda: criteo_input_fn(files, 64, -1, True, layout=layout, shuffle_buffer=5, seed=3, device_parse=flag), steps=24)
        losses = re.findall(r"INFO:loss = (\S+), step = (\d+)", capsys.readouterr().out)
        ev = est.evaluate(lambda: criteo_input_fn(files, 64, 1, False, layout=layout, device_parse=flag), steps=5)
        pr = np.array([p["prob"] for p in est.predict(lambda: criteo_input_fn(files[1:], 64, 1, False, layout=layout, device_parse=flag))])
        res.append((losses, _state_hash(est), ev, pr))
    (l0, h0, e0, p0), (l1, h1, e1, p1) = res
    assert len(l0) == 6 and l0 == l1, (l0, l1)
    assert h0 == h1
    assert e0 == e1, (e0, e1)
    assert p0.shape == (330,) and np.array_equal(p0, p1)
