"""The export bundle and the serving kernel's refusals, without a GPU: flags of the five scripts, the bundle writer / reader
(round trip bit for bit, atomic directory, settings-only manifest, every refusal of the reader), and the C ABI of
rsx_predict_fm_tower turning bad arguments and out-of-envelope shapes away before any HIP call."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

EINVAL, EUNSUPPORTED = -1, -3
P = 0x1000          # "some non-NULL, 16-byte aligned pointer" -- never read


@pytest.mark.parametrize("mod", ["fm", "deepfm", "xdeepfm", "dcn", "din"])
def test_scripts_accept_export_flags(mod):
    m = importlib.import_module("recsys_amd." + mod)
    F = m.define_flags().parse_args([])
    assert F.export_path == "./export/" and F.task_type == "train"
    F = m.define_flags().parse_args(["--task_type", "export", "--export_path", "/some/where/"])
    assert F.task_type == "export" and F.export_path == "/some/where/"


def _hand_made():
    from recsys_amd import serving
    from recsys_amd.feature_columns import build_feature_columns
    rng = np.random.default_rng(0)
    lin, emb = build_feature_columns(16, "indicator_all")
    tensors = {"emb.input_layer.tables": rng.standard_normal((40, 16)).astype(np.float32),
               "emb.input_layer.w1": rng.standard_normal(40).astype(np.float32),
               "dense.b1": np.array([0.25], np.float32),
               "dense.out.W": rng.standard_normal((2, 1)).astype(np.float32),
               "dense.out.b": np.array([-0.0], np.float32)}          # (a negative zero: bits, not values, must survive)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "deep_layers": "100,100",
              "learning_rate": 0.001, "dropout": 0.5, "max_batch_size": 256}
    return serving, params, emb, tensors


def test_bundle_round_trip_bit_for_bit(tmp_path):
    serving, params, emb, tensors = _hand_made()
    base = str(tmp_path / "export")
    d = serving.write_bundle(base, serving.make_manifest("fm", params, 123, tensors), tensors)
    assert os.path.dirname(d) == base and re.fullmatch(r"\d+", os.path.basename(d))          # decimal seconds
    assert abs(int(os.path.basename(d)) - __import__("time").time()) < 600
    assert sorted(os.listdir(base)) == [os.path.basename(d)]                                   # no temporary directory left
    assert sorted(os.listdir(d)) == ["model.json", "variables.npz"]
    with np.load(os.path.join(d, "variables.npz"), allow_pickle=False) as z:
        assert sorted(z.files) == sorted(tensors)
    manifest = json.load(open(os.path.join(d, "model.json")))
    assert manifest["format_version"] == serving.FORMAT_VERSION and manifest["script"] == "fm" and manifest["global_step"] == 123
    assert manifest["feature_set"] == "criteo" and manifest["linear_mode"] == "indicator_all"
    assert manifest["batch_norm_epsilon"] == 1e-3 and manifest["params"]["embedding_size"] == 16
    assert "learning_rate" not in manifest["params"] and "dropout" not in manifest["params"]   # no training flags
    m2, got = serving.read_bundle(d)
    assert m2 == manifest and sorted(got) == sorted(tensors)
    for k, v in tensors.items():
        assert got[k].dtype == np.float32 and got[k].shape == v.shape
        assert np.array_equal(got[k].view(np.uint32), v.view(np.uint32)), k
    # the manifest alone rebuilds the parsing layout
    from recsys_amd.feature_columns import CriteoLayout
    want = CriteoLayout.from_columns(emb)
    lay = serving.layout_from_manifest(m2)
    assert np.array_equal(lay.row_off, want.row_off) and [c.name for c in lay.columns] == [c.name for c in want.columns]
    assert [c.boundaries for c in lay.columns] == [c.boundaries for c in want.columns]
    assert serving.latest_bundle(base) == d and serving.latest_bundle(d) == d


def test_second_export_gets_its_own_newer_directory(tmp_path):
    serving, params, _, tensors = _hand_made()
    base = str(tmp_path)
    d1 = serving.write_bundle(base, serving.make_manifest("fm", params, 1, tensors), tensors)
    d2 = serving.write_bundle(base, serving.make_manifest("fm", params, 2, tensors), tensors)
    assert d1 != d2 and int(os.path.basename(d2)) > int(os.path.basename(d1))
    assert serving.latest_bundle(base) == d2 and serving.read_bundle(serving.latest_bundle(base))[0]["global_step"] == 2
    assert len(os.listdir(base)) == 2


def test_manifest_of_every_linear_mode_and_feature_set():
    from recsys_amd import serving
    from recsys_amd.feature_columns import build_feature_columns, build_model_columns
    for mode in ("indicator_all", "numeric+indicator", "numeric"):
        assert serving.linear_mode(build_feature_columns(16, mode)[0]) == mode
    lin, emb = build_model_columns(8)
    m = serving.make_manifest("deepfm", {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 8,
                                         "deep_layers": "32,16"}, 0, {})
    assert m["feature_set"] == "uid_iid" and [c["key"] for c in m["embedding_columns"]] == ["u_id", "i_id"]
    assert serving.make_manifest("din", {"embedding_size": 32, "hist_len": 30}, 0, {})["params"]["hist_len"] == 30
    p = serving.params_from_manifest(m, 512)
    assert p["max_batch_size"] == 512 and p["deep_layers"] == "32,16" and [c.rows for c in p["embedding_feature_columns"]] == [500000, 100000]


def _written(tmp_path):
    serving, params, _, tensors = _hand_made()
    return serving, serving.write_bundle(str(tmp_path), serving.make_manifest("fm", params, 7, tensors), tensors), tensors


def _rewrite_manifest(d, fn):
    p = os.path.join(d, "model.json")
    m = json.load(open(p))
    fn(m)
    json.dump(m, open(p, "w"))


def test_reader_refuses_unknown_format_version(tmp_path):
    from recsys_amd._lib import RsxError
    serving, d, _ = _written(tmp_path)
    _rewrite_manifest(d, lambda m: m.update(format_version=99))
    with pytest.raises(RsxError, match="format_version"):
        serving.read_bundle(d)


def test_reader_refuses_listed_tensor_missing_from_archive(tmp_path):
    from recsys_amd._lib import RsxError
    serving, d, tensors = _written(tmp_path)
    np.savez(open(os.path.join(d, "variables.npz"), "wb"), **{k: v for k, v in tensors.items() if k != "dense.b1"})
    with pytest.raises(RsxError, match="dense.b1"):
        serving.read_bundle(d)


def test_reader_refuses_archive_tensor_the_manifest_does_not_list(tmp_path):
    from recsys_amd._lib import RsxError
    serving, d, tensors = _written(tmp_path)
    np.savez(open(os.path.join(d, "variables.npz"), "wb"), **tensors, **{"dense.stowaway": np.zeros(3, np.float32)})
    with pytest.raises(RsxError, match="stowaway"):
        serving.read_bundle(d)


def test_reader_refuses_shape_and_dtype_mismatch(tmp_path):
    from recsys_amd._lib import RsxError
    serving, d, tensors = _written(tmp_path)

    def shape(m):
        [t for t in m["tensors"] if t["name"] == "dense.out.W"][0]["shape"] = [1, 2]
    _rewrite_manifest(d, shape)
    with pytest.raises(RsxError, match="shape"):
        serving.read_bundle(d)
    serving, d, tensors = _written(tmp_path / "b")
    bad = dict(tensors)
    bad["emb.input_layer.w1"] = tensors["emb.input_layer.w1"].astype(np.float64)
    np.savez(open(os.path.join(d, "variables.npz"), "wb"), **bad)
    with pytest.raises(RsxError, match="dtype"):
        serving.read_bundle(d)


def test_loading_nothing_names_the_cause(tmp_path):
    from recsys_amd import serving
    from recsys_amd._lib import RsxError
    with pytest.raises(RsxError, match="no exported model"):
        serving.latest_bundle(str(tmp_path))


def test_writer_refuses_object_arrays(tmp_path):
    from recsys_amd import serving
    from recsys_amd._lib import RsxError
    with pytest.raises(RsxError):
        serving.write_bundle(str(tmp_path), {"format_version": 1}, {"x": np.array([{}], dtype=object)})
    assert os.listdir(str(tmp_path)) == []


def test_export_without_a_checkpoint_names_the_cause(tmp_path):
    """Estimator.export_savedmodel on an empty model_dir fails before it touches the device."""
    from recsys_amd import deepfm
    from recsys_amd._lib import RsxError
    from recsys_amd.estimator import Estimator, RunConfig
    F = deepfm.define_flags().parse_args(["--model_dir", str(tmp_path / "model")])
    est = Estimator(deepfm.model_fn, F.model_dir, deepfm.make_params(F), RunConfig())
    with pytest.raises(RsxError, match="no checkpoint in model_dir"):
        est.export_savedmodel(str(tmp_path / "export"))
    assert not os.path.exists(str(tmp_path / "export"))


# ---- C ABI refusals (made before any HIP call) ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _model(F=39, D=16, widths=(100, 100), **kw):
    from recsys_amd import _lib
    m = _lib.PredictModel()
    m.tables = m.w1 = m.row_off = m.wd = m.bd = m.c0 = m.wo = m.bo = P
    for l in range(len(widths)):
        m.W[l] = m.b[l] = m.gamma[l] = m.beta[l] = P
        m.widths[l] = widths[l]
    m.w1_field_mask, m.bn_eps, m.F, m.D, m.L = (1 << F) - 1, 1e-3, F, D, len(widths)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _call(L, m, ids=P, prob=P, B=16):
    return L.rsx_predict_fm_tower(C.byref(m) if m is not None else None, ids, prob, B, None)


def test_predict_c_abi_refuses_bad_arguments(L):
    assert _call(L, None) == EINVAL
    assert _call(L, _model(), ids=None) == EINVAL
    assert _call(L, _model(), prob=None) == EINVAL
    assert _call(L, _model(), B=0) == EINVAL
    assert _call(L, _model(), B=-5) == EINVAL
    for f in ("tables", "row_off", "wo", "bo", "wd", "bd"):
        assert _call(L, _model(**{f: None})) == EINVAL, f
    for arr in ("W", "b"):
        for l in (0, 1):
            m = _model()
            getattr(m, arr)[l] = None
            assert _call(L, m) == EINVAL, (arr, l)
    m = _model()
    m.gamma[1] = None                                     # gamma without beta (both NULL = a layer without batch-norm)
    assert _call(L, m) == EINVAL
    m = _model()
    m.widths[0] = 0
    assert _call(L, m) == EINVAL
    assert _call(L, _model(tables=P + 4)) == EINVAL       # rows are read as float4
    assert _call(L, _model(F=0)) == EINVAL
    assert _call(L, _model(bn_eps=-1.0)) == EINVAL
    assert _call(L, _model(bn_eps=float("nan"))) == EINVAL


def test_predict_c_abi_envelope(L):
    from recsys_amd import _lib
    sup = lambda B, F, D, w: L.rsx_predict_fm_tower_supported(B, F, D, len(w), (C.c_int32 * 3)(*w) if w else None)
    for w in ((), (100, 100), (32, 16), (64, 32, 16), (400, 400, 256), (100, 50), (256,)):
        for B in (1, 7, 16, 17, 200, 4096, 1 << 20):
            for F in (1, 2, 39, 64):
                assert sup(B, F, 16, w) == 1, (B, F, w)
    assert sup(256, 39, 8, (100, 100)) == 0               # D != 16
    assert sup(256, 39, 32, (100, 100)) == 0
    assert sup(256, 65, 16, (100, 100)) == 0              # F > 64
    assert sup(256, 0, 16, ()) == 0
    assert sup(0, 39, 16, ()) == 0
    assert sup(256, 39, 16, (100, 100, 100)) == 1
    assert L.rsx_predict_fm_tower_supported(256, 39, 16, 4, (C.c_int32 * 4)(64, 64, 64, 64)) == 0     # more than 3 layers
    assert sup(256, 39, 16, (50, 100)) == 0               # an inner width that is no multiple of 4 (FusedTower.supports)
    assert sup(256, 39, 16, (100, 300)) == 0              # a last width above 256
    assert sup(256, 64, 16, (2048, 64)) == 0              # activation tiles beyond the LDS
    assert sup(1 << 30, 39, 16, ()) == 0                  # B * F beyond 2^31
    # the entry says the same, before any HIP call
    assert _call(L, _model(D=8)) == EUNSUPPORTED
    assert _call(L, _model(F=65)) == EUNSUPPORTED
    assert _call(L, _model(widths=(50, 100))) == EUNSUPPORTED
    assert _call(L, _model(widths=(100, 300))) == EUNSUPPORTED
    assert _call(L, _model(F=64, widths=(2048, 64))) == EUNSUPPORTED
    m = _model()
    m.L = 4
    assert _call(L, m) == EUNSUPPORTED
    # every width FusedTower.supports takes at deepfm.py's shapes is inside
    from recsys_amd.ops import FusedTower
    for w in ((100, 100), (32, 16), (64, 32, 16), (400, 256), (128,), (100, 50)):
        assert FusedTower.supports(624, w) and sup(4096, 39, 16, w) == 1
    assert _lib.PREDICT_MAX_LAYERS == 3
