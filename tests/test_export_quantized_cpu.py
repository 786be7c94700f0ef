"""16-bit embedding tables in the export bundle, without a GPU: the two conversions pinned bit for bit against torch / numpy,
the bundle of each dtype (format_version, table_dtype, stored dtype / encoding per tensor, what stays fp32, the size on disk),
the float32 bundle unchanged against the writer as it was before the option, the reader's five new refusals, and the C ABI of
rsx_predict_fm_tower / rsx_predict_dcn refusing a bad table_dtype before any HIP call (host pointers, a null stream)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.test_export_cpu import _hand_made, _model, _rewrite_manifest
from tests.test_predict_dcn_cpu import _aligned, _host_model

EINVAL, EUNSUPPORTED = -1, -3
DTYPES = ("bfloat16", "float16")


# ---- 1: the conversion recipes -------------------------------------------------------------------------------------------------
def _conversion_input():
    rng = np.random.default_rng(0)
    special = np.array([0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1e-40, -1e-40, 1.4e-45, 65504.0, -65504.0,
                        2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 6.0e-8, 6.1e-5], np.float32)
    return np.concatenate([rng.standard_normal(100000).astype(np.float32), special])


def test_quantize_rows_is_round_to_nearest_even_bit_for_bit():
    torch = pytest.importorskip("torch")
    from recsys_amd import serving
    x = _conversion_input()
    b = serving.quantize_rows(x, "bfloat16")
    assert b.dtype == np.uint16 and b.shape == x.shape
    assert np.array_equal(b, torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    h = serving.quantize_rows(x, "float16")
    assert h.dtype == np.float16
    assert np.array_equal(h.view(np.uint16), x.astype(np.float16).view(np.uint16))
    assert np.array_equal(h.view(np.uint16), torch.from_numpy(x).to(torch.float16).numpy().view(np.uint16))
    # the exact ties go to the even neighbour: 1 + 2^-8 down to 1, 1 + 3 * 2^-8 up to 1 + 2^-6
    ties = serving.dequantize_rows(serving.quantize_rows(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], np.float32), "bfloat16"), "bfloat16")
    assert ties.tolist() == [1.0, 1 + 2.0 ** -6]
    f = serving.quantize_rows(x, "float32")
    assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), x.view(np.uint32))
    # widening is exact and a second round trip changes nothing; signed zeros keep their sign
    for dt, enc in (("bfloat16", "bfloat16"), ("float16", None)):
        q = serving.quantize_rows(x, dt)
        w = serving.dequantize_rows(q, enc)
        assert w.dtype == np.float32 and w.shape == x.shape
        q2 = serving.quantize_rows(w, dt)
        assert np.array_equal(q2.view(np.uint16), q.view(np.uint16))
        assert np.array_equal(serving.dequantize_rows(q2, enc).view(np.uint32), w.view(np.uint32))
        z = serving.dequantize_rows(serving.quantize_rows(np.array([0.0, -0.0], np.float32), dt), enc)
        assert z.view(np.uint32).tolist() == [0, 0x80000000]
    w = serving.dequantize_rows(serving.quantize_rows(x, "float16"), None)
    assert np.array_equal(w, x.astype(np.float16).astype(np.float32))


def test_quantize_rows_refuses_what_has_no_finite_16_bit_value():
    from recsys_amd import serving
    from recsys_amd._lib import RsxError
    for dt in DTYPES:
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(RsxError, match=r"emb\.input_layer\.tables"):
                serving.quantize_rows(np.array([1.0, bad, 2.0], np.float32), dt, "emb.input_layer.tables")
    with pytest.raises(RsxError, match=r"emb\.input_layer\.tables.*infinity"):
        serving.quantize_rows(np.array([7e4], np.float32), "float16", "emb.input_layer.tables")
    with pytest.raises(RsxError, match=r"emb\.u\.table.*infinity"):
        serving.quantize_rows(np.array([np.finfo(np.float32).max], np.float32), "bfloat16", "emb.u.table")
    assert serving.quantize_rows(np.array([65504.0], np.float32), "float16").tolist() == [65504.0]
    assert serving.quantize_rows(np.array([7e4], np.float32), "bfloat16").dtype == np.uint16
    with pytest.raises(RsxError):
        serving.quantize_rows(np.zeros(3, np.float32), "int8")


# ---- 2: the bundle of each dtype -----------------------------------------------------------------------------------------------
def _estimator_shaped():
    """The hand-made fm.py tensors of test_export_cpu.py, a larger table (the size check needs R x D x 2 bytes to dwarf the zip
    headers), and din.py-shaped extras: a second table, a 4-wide bias table that must stay fp32."""
    serving, params, emb, tensors = _hand_made()
    rng = np.random.default_rng(1)
    tensors = dict(tensors)
    tensors["emb.input_layer.tables"] = rng.standard_normal((4000, 16)).astype(np.float32)
    tensors["emb.input_layer.w1"] = rng.standard_normal(4000).astype(np.float32)
    return serving, params, tensors


def _export(serving, base, script, params, tensors, dtype):
    stored = serving.quantize_tensors(tensors, params["embedding_size"], dtype) if dtype != "float32" else tensors
    return serving.write_bundle(base, serving.make_manifest(script, params, 5, stored, dtype), stored)


@pytest.mark.parametrize("dtype", DTYPES)
def test_16_bit_bundle_round_trip(tmp_path, dtype):
    serving, params, tensors = _estimator_shaped()
    d32 = _export(serving, str(tmp_path / "f32"), "fm", params, tensors, "float32")
    d = _export(serving, str(tmp_path / dtype), "fm", params, tensors, dtype)
    manifest, got = serving.read_bundle(d)
    assert manifest["format_version"] == 2 and manifest["table_dtype"] == dtype
    assert json.load(open(os.path.join(d32, "model.json")))["format_version"] == 1
    entries = {t["name"]: t for t in manifest["tensors"]}
    assert sorted(entries) == sorted(tensors) == sorted(got)
    for k, v in tensors.items():
        if k == "emb.input_layer.tables":
            if dtype == "bfloat16":
                assert entries[k]["dtype"] == "uint16" and entries[k]["encoding"] == "bfloat16" and got[k].dtype == np.uint16
            else:
                assert entries[k]["dtype"] == "float16" and "encoding" not in entries[k] and got[k].dtype == np.float16
            assert got[k].shape == v.shape
            assert np.array_equal(got[k].view(np.uint16), serving.quantize_rows(v, dtype).view(np.uint16))
            wide = serving.dequantize_rows(got[k], entries[k].get("encoding"))
            assert 0 < np.abs(wide - v).max() <= np.abs(v).max() * (2.0 ** -8 if dtype == "bfloat16" else 2.0 ** -11)
        else:                                                     # w1 and every dense tensor: the same fp32 bits
            assert entries[k]["dtype"] == "float32" and "encoding" not in entries[k] and got[k].dtype == np.float32, k
            assert np.array_equal(got[k].view(np.uint32), v.view(np.uint32)), k
    R, D = tensors["emb.input_layer.tables"].shape
    shrink = os.path.getsize(os.path.join(d32, "variables.npz")) - os.path.getsize(os.path.join(d, "variables.npz"))
    assert abs(shrink - R * D * 2) <= 1024, shrink                # (npz members are stored, not deflated)
    wide = serving.widen_tensors(manifest, got)
    assert all(v.dtype == np.float32 for v in wide.values())
    assert np.array_equal(serving.quantize_rows(wide["emb.input_layer.tables"], dtype).view(np.uint16),
                          got["emb.input_layer.tables"].view(np.uint16))


def test_every_table_of_din_and_xdeepfm_qualifies_and_the_bias_table_does_not():
    from recsys_amd import serving
    rng = np.random.default_rng(2)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    din = {"emb.i_id.table": f(30, 32), "emb.i_cate.table": f(8, 32), "emb.i_item.table": f(30, 4), "dense.mlp.W0": f(96, 32)}
    q = serving.quantize_tensors(din, 32, "bfloat16")
    assert q["emb.i_id.table"].dtype == q["emb.i_cate.table"].dtype == np.uint16
    assert q["emb.i_item.table"] is din["emb.i_item.table"] and q["dense.mlp.W0"] is din["dense.mlp.W0"]
    m = serving.make_manifest("din", {"embedding_size": 32, "hist_len": 30}, 0, q, "bfloat16")
    enc = {t["name"]: t.get("encoding") for t in m["tensors"]}
    assert enc == {"emb.i_id.table": "bfloat16", "emb.i_cate.table": "bfloat16", "emb.i_item.table": None, "dense.mlp.W0": None}
    xd = {"emb.input_layer.tables": f(20, 16), "emb.input_layer.w1": f(20), "emb.linear.tables": f(20, 16), "dense.cin.W0": f(16, 16)}
    q = serving.quantize_tensors(xd, 16, "float16")
    assert [str(q[k].dtype) for k in xd] == ["float16", "float32", "float16", "float32"]


def test_estimator_and_every_script_take_the_option(tmp_path):
    import importlib
    import inspect
    from recsys_amd._lib import RsxError
    from recsys_amd.estimator import Estimator
    assert inspect.signature(Estimator.export_savedmodel).parameters["table_dtype"].default == "float32"
    for mod in ("fm", "deepfm", "xdeepfm", "dcn", "din"):
        m = importlib.import_module("recsys_amd." + mod)
        assert m.define_flags().parse_args([]).export_table_dtype == "float32"
        for dt in ("float32",) + DTYPES:
            assert m.define_flags().parse_args(["--export_table_dtype", dt]).export_table_dtype == dt
        with pytest.raises(SystemExit):
            m.define_flags().parse_args(["--export_table_dtype", "int8"])
    from recsys_amd import serving
    with pytest.raises(RsxError, match="int8"):
        serving.make_manifest("fm", _hand_made()[1], 0, {}, "int8")


# ---- 3: the float32 bundle is what it was ------------------------------------------------------------------------------------
def _manifest_before_the_option(serving, script, params, global_step, tensors):
    """make_manifest as it was before table_dtype existed (criteo feature set), restated."""
    from recsys_amd.layers import BN_EPS
    emb, lin = params["embedding_feature_columns"], params["linear_feature_columns"]
    return {"format_version": 1, "script": script, "global_step": int(global_step), "feature_set": "criteo",
            "linear_mode": serving.linear_mode(lin), "batch_norm_epsilon": BN_EPS,
            "params": {k: params[k] for k in serving._NETWORK_PARAMS if k in params},
            "embedding_columns": [serving._column_json(c) for c in emb], "linear_columns": [serving._column_json(c) for c in lin],
            "signature": {"serving_default": {"inputs": "examples", "outputs": ["prob"]}},
            "tensors": [{"name": k, "shape": [int(d) for d in v.shape], "dtype": str(v.dtype)} for k, v in tensors.items()]}


def test_float32_export_is_unchanged(tmp_path):
    serving, params, tensors = _estimator_shaped()
    assert serving.FORMAT_VERSION == 1
    old = _manifest_before_the_option(serving, "fm", params, 5, tensors)
    d_old = serving.write_bundle(str(tmp_path / "old"), old, tensors)
    d_def = serving.write_bundle(str(tmp_path / "default"), serving.make_manifest("fm", params, 5, tensors), tensors)
    d_f32 = _export(serving, str(tmp_path / "f32"), "fm", params, tensors, "float32")
    m_old = json.load(open(os.path.join(d_old, "model.json")))
    for d in (d_def, d_f32):
        m = json.load(open(os.path.join(d, "model.json")))
        assert m == m_old and "table_dtype" not in m and not any("encoding" in t for t in m["tensors"])
        assert open(os.path.join(d, "model.json"), "rb").read() == open(os.path.join(d_old, "model.json"), "rb").read()
        m2, got = serving.read_bundle(d)
        assert m2 == m_old
        for k, v in tensors.items():
            assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.uint32), v.view(np.uint32)), k
        assert serving.widen_tensors(m2, got)["emb.input_layer.tables"] is got["emb.input_layer.tables"]


# ---- 4: the reader's refusals ------------------------------------------------------------------------------------------------
def _written16(tmp_path, dtype):
    serving, params, tensors = _estimator_shaped()
    return serving, _export(serving, str(tmp_path), "fm", params, tensors, dtype)


def _entry(m, name):
    return [t for t in m["tensors"] if t["name"] == name][0]


def test_reader_refuses_a_version_2_manifest_without_a_16_bit_table_dtype(tmp_path):
    from recsys_amd._lib import RsxError
    for i, bad in enumerate(("float32", "int8", None)):
        serving, d = _written16(tmp_path / str(i), "bfloat16")
        _rewrite_manifest(d, lambda m: m.update(table_dtype=bad))
        with pytest.raises(RsxError, match="table_dtype"):
            serving.read_bundle(d)
    serving, d = _written16(tmp_path / "gone", "float16")
    _rewrite_manifest(d, lambda m: m.pop("table_dtype"))
    with pytest.raises(RsxError, match="table_dtype"):
        serving.read_bundle(d)
    serving, d = _written16(tmp_path / "v3", "float16")
    _rewrite_manifest(d, lambda m: m.update(format_version=3))
    with pytest.raises(RsxError, match="format_version"):
        serving.read_bundle(d)


def test_reader_refuses_a_uint16_tensor_without_an_encoding(tmp_path):
    from recsys_amd._lib import RsxError
    serving, d = _written16(tmp_path, "bfloat16")
    _rewrite_manifest(d, lambda m: _entry(m, "emb.input_layer.tables").pop("encoding"))
    with pytest.raises(RsxError, match=r"emb\.input_layer\.tables.*without an encoding"):
        serving.read_bundle(d)


def test_reader_refuses_an_encoding_on_a_tensor_that_holds_no_embedding_rows(tmp_path):
    from recsys_amd._lib import RsxError
    for i, name in enumerate(("emb.input_layer.w1", "dense.out.W")):
        serving, d = _written16(tmp_path / str(i), "bfloat16")
        _rewrite_manifest(d, lambda m: _entry(m, name).update(encoding="bfloat16"))
        with pytest.raises(RsxError, match=name.replace(".", r"\.") + ".*no embedding-row tensor"):
            serving.read_bundle(d)


def test_reader_refuses_tables_stored_in_another_dtype_than_table_dtype(tmp_path):
    from recsys_amd._lib import RsxError
    serving, d = _written16(tmp_path / "a", "float16")
    _rewrite_manifest(d, lambda m: m.update(table_dtype="bfloat16"))          # float16 rows under a bfloat16 table_dtype
    with pytest.raises(RsxError, match=r"emb\.input_layer\.tables.*table_dtype"):
        serving.read_bundle(d)
    serving, d = _written16(tmp_path / "b", "bfloat16")
    _rewrite_manifest(d, lambda m: m.update(table_dtype="float16"))
    with pytest.raises(RsxError, match=r"emb\.input_layer\.tables.*table_dtype"):
        serving.read_bundle(d)
    # fp32 rows in a version 2 bundle
    serving, params, tensors = _estimator_shaped()
    m = serving.make_manifest("fm", params, 5, tensors)
    m.update(format_version=2, table_dtype="float16")
    d = serving.write_bundle(str(tmp_path / "c"), m, tensors)
    with pytest.raises(RsxError, match=r"emb\.input_layer\.tables.*table_dtype"):
        serving.read_bundle(d)


def test_reader_refuses_a_version_1_manifest_with_either_new_key(tmp_path):
    from recsys_amd._lib import RsxError
    serving, params, tensors = _estimator_shaped()
    d = _export(serving, str(tmp_path / "a"), "fm", params, tensors, "float32")
    _rewrite_manifest(d, lambda m: m.update(table_dtype="bfloat16"))
    with pytest.raises(RsxError, match="table_dtype"):
        serving.read_bundle(d)
    d = _export(serving, str(tmp_path / "b"), "fm", params, tensors, "float32")
    _rewrite_manifest(d, lambda m: _entry(m, "emb.input_layer.tables").update(encoding="bfloat16"))
    with pytest.raises(RsxError, match="encoding"):
        serving.read_bundle(d)
    # a version 2 bundle relabelled as version 1 (what an older reader would otherwise misread)
    serving, d = _written16(tmp_path / "c", "bfloat16")
    _rewrite_manifest(d, lambda m: m.update(format_version=1))
    with pytest.raises(RsxError, match="table_dtype"):
        serving.read_bundle(d)


# ---- 5: the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_and_ctypes_agree_on_the_table_dtypes():
    import re
    from recsys_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rsx.h")).read()
    for name, key in (("RSX_TABLE_F32", "float32"), ("RSX_TABLE_BF16", "bfloat16"), ("RSX_TABLE_F16", "float16")):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == _lib.TABLE_DTYPES[key]
    assert _lib.TABLE_DTYPES == {"float32": 0, "bfloat16": 1, "float16": 2}
    for S in (_lib.PredictModel, _lib.PredictDcnModel):
        assert S._fields_[-1][0] == "table_dtype" and S().table_dtype == 0          # the LAST member; zeroed means fp32
    assert C.sizeof(_lib.PredictDcnModel) % 8 == 0


def test_c_abi_refuses_a_bad_table_dtype_before_any_hip_call(L):
    assert L.rsx_version() >= 101
    fm = lambda m, B=16: L.rsx_predict_fm_tower(C.byref(m), 0x1000, 0x1000, B, None)
    for bad in (7, -1, 3):
        assert fm(_model(table_dtype=bad)) == EINVAL, bad
        assert fm(_model(widths=(), table_dtype=bad)) == EINVAL, bad
    assert fm(_model(table_dtype=1, tables=0x1000 + 8)) == EINVAL          # 16-bit rows still want 16-byte alignment
    assert fm(_model(table_dtype=2, tables=0x1000 + 8)) == EINVAL
    for td in (0, 1, 2):                                                  # a known dtype, a shape outside the envelope
        assert fm(_model(table_dtype=td, D=8)) == EUNSUPPORTED, td
        assert fm(_model(table_dtype=td, F=65)) == EUNSUPPORTED, td
        assert fm(_model(table_dtype=td, widths=(50, 100))) == EUNSUPPORTED, td

    ids, prob = _aligned(4 * 5, np.int32), _aligned(4)
    dcn = lambda m: L.rsx_predict_dcn(C.byref(m), ids.ctypes.data, prob.ctypes.data, 4, None)
    for bad in (7, -1):
        m, keep = _host_model()
        m.table_dtype = bad
        assert dcn(m) == EINVAL, bad
    m, keep = _host_model()
    keep["tables"] = t = _aligned(64 * 16, np.uint16, shift=8)
    assert t.ctypes.data % 16 == 8
    m.tables, m.table_dtype = t.ctypes.data, 1
    assert dcn(m) == EINVAL
    for td in (1, 2):
        m, keep = _host_model()
        keep["tables"] = t = _aligned(64 * 16, np.uint16)
        m.tables, m.table_dtype, m.D = t.ctypes.data, td, 8               # valid host pointers, D outside the envelope
        assert dcn(m) == EUNSUPPORTED, td
        m.D, m.Lc = 16, 9
        assert dcn(m) == EUNSUPPORTED, td
