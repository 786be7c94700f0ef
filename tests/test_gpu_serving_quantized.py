"""16-bit embedding tables on the one-launch serving paths, on the GPU: rsx_predict_fm_tower / rsx_predict_dcn with bfloat16
and float16 tables against the fp32 launch over the widened tables (bit for bit: widening is exact and only the row load
differs) and against the oracle on the rounded tables; `Predictor` on 16-bit bundles (fused: the table on the device in 16
bits; layers: widened on the host); device memory; deepfm.py's train -> export --export_table_dtype -> Predictor chain.

The recipes are tests/test_gpu_serving.py's `perturbed_params` and tests/dcn_serving_util.py's `perturbed_dcn_params`, by
import.  The criteo39 cases (87.9 KB of LDS with 100-100) need the raised LDS limit that every kernel instantiation has to ask
for itself; the 41-field case runs predict_dcn_k<8>."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from tests import dcn_serving_util as U
from tests import test_gpu_serving as S
from tests import test_gpu_serving_dcn as SD

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G = S.G
DTYPES = ("bfloat16", "float16")
ENC = {"bfloat16": "bfloat16", "float16": None}
BATCHES = (1, 17, 200)
F41_ROWS = [5] * 41                     # 41 fields of 5 rows: F > 40 takes predict_dcn_k<8>
_STORED = {}

# model = (family, cols, tower, cross layers)
FM_CASES = [("fm", "small", ()), ("fm", "criteo39", ()), ("deepfm", "small", (100, 100)), ("deepfm", "criteo39", (100, 100))]
DCN_CASES = [("dcn", "criteo39", (100, 100), 3), ("dcn", "small", (32, 18), 3), ("dcn", "f41", (32, 16), 2)]
_id = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _params(kind, cols, layers, Lc=0):
    """-> (P, row_off): the shared fp32 recipe (never modified here)."""
    if kind != "dcn":
        return S.perturbed_params(kind, cols, layers)
    if cols != "f41":
        return U.perturbed_dcn_params(cols, layers, Lc)
    key = ("f41", tuple(layers), Lc)
    if key not in _STORED:
        from oracle import init
        row_off = np.concatenate([[0], np.cumsum(F41_ROWS)]).astype(np.int64)
        P = init.dcn_params(0, 16, tuple(layers), Lc, np.float32, row_off)
        rng = np.random.default_rng(1000)                # the noise of dcn_serving_util.perturbed_dcn_params
        for k in sorted(P):
            leaf = k.split(".")[-1]
            if leaf.startswith("gamma"):
                P[k] = (P[k] + rng.uniform(-0.3, 0.3, P[k].shape)).astype(np.float32)
            elif leaf.startswith("beta") or leaf == "b" or (leaf.startswith("b") and leaf[1:].isdigit()):
                P[k] = (P[k] + rng.uniform(-0.2, 0.2, P[k].shape)).astype(np.float32)
        _STORED[key] = (P, row_off)
    return _STORED[key]


def _planted_fields(row_off):
    """The fields that get a planted row: those of more than 16 rows, where the requests' Zipf ids rarely land on one row by
    chance (test 2 sets the examples that do aside); every field when there is no such field (41 fields of 5 rows)."""
    big = np.flatnonzero(np.diff(np.asarray(row_off)) > 16)
    return big if len(big) else np.arange(len(row_off) - 1)


def _planted_ids(row_off):
    """One example that hits every planted row: local id 1 in the planted fields, 0 elsewhere."""
    ids = np.zeros(len(row_off) - 1, np.int32)
    ids[_planted_fields(row_off)] = 1
    return ids


def stored_tables(kind, cols, layers, Lc, dtype):
    """-> (tables in their stored 16-bit form, the same widened to fp32), computed once per model and dtype.  The rows of
    `_planted_ids` carry this dtype's subnormals (float16: 2^-24 .. 2^-15, normal numbers in fp32; bfloat16: fp32 subnormals
    with 7 mantissa bits) and negative zeros in half of their elements; the other half keeps the recipe's values."""
    from recsys_amd import serving
    key = (kind, cols, tuple(layers), Lc, dtype)
    if key not in _STORED:
        P, row_off = _params(kind, cols, layers, Lc)
        t = P["tables"].astype(np.float32, copy=True)
        rows = np.asarray(row_off[:-1], np.int64)[_planted_fields(row_off)] + 1
        if dtype == "float16":
            sub = np.array([2.0 ** -24, -3 * 2.0 ** -24, 1023 * 2.0 ** -24, -2.0 ** -15, 5.0e-5, -3.1e-5, 2.0 ** -17], np.float32)
        else:
            sub = np.array([2.0 ** -133, -3 * 2.0 ** -133, 127 * 2.0 ** -133, -2.0 ** -127, 2.0 ** -130], np.float64).astype(np.float32)
        for n, r in enumerate(rows):
            for e in range(0, 16, 2):
                t[r, e + (n & 1)] = -0.0 if (e // 2 + n) % 4 == 3 else sub[(e // 2 + n) % len(sub)]
        q = serving.quantize_rows(t, dtype, "tables")
        wide = serving.dequantize_rows(q, ENC[dtype])
        planted = wide[rows]
        assert np.signbit(planted[planted == 0]).all() and (planted == 0).any()          # the zeros are negative zeros
        tiny = np.abs(planted[planted != 0]).min()
        assert 0 < tiny < (6.2e-5 if dtype == "float16" else 1.2e-38)                    # subnormals survived the rounding
        _STORED[key] = q
    q = _STORED[key]
    return q, serving.dequantize_rows(q, ENC[dtype])


def _request(rng, B, row_off):
    from tests.parity_util import synth_ids
    ids = synth_ids(rng, B, row_off)
    ids[0] = _planted_ids(row_off)
    return ids


def _device_pair(kind, cols, layers, Lc, dtype):
    """-> (fp32 model over the widened tables, the same model over the 16-bit tables, launch function, keep-alive, P wide)."""
    from recsys_amd import _lib
    P, row_off = _params(kind, cols, layers, Lc)
    q, wide = stored_tables(kind, cols, layers, Lc, dtype)
    Pw = dict(P)
    Pw["tables"] = wide
    if kind == "dcn":
        m32, keep = SD.device_model(Pw, row_off, layers, Lc)
        m16, keep2 = SD.device_model(dict(Pw, tables=np.zeros(4, np.float32)), row_off, layers, Lc)
        fn, name = _lib.lib().rsx_predict_dcn, "rsx_predict_dcn"
    else:
        m32, keep = S.device_model(Pw, row_off, layers)
        m16, keep2 = S.device_model(dict(Pw, tables=np.zeros(4, np.float32)), row_off, layers)
        fn, name = _lib.lib().rsx_predict_fm_tower, "rsx_predict_fm_tower"
    d16 = torch.from_numpy(q.view(np.int16) if q.dtype == np.uint16 else q).cuda()
    assert d16.element_size() == 2 and d16.data_ptr() % 16 == 0
    m16.tables, m16.table_dtype = d16.data_ptr(), _lib.TABLE_DTYPES[dtype]

    def launch(m, ids, guard=64):
        B = ids.shape[0]
        d_ids = torch.from_numpy(ids).cuda()
        out = torch.full((B + guard,), -7.0, device="cuda")
        _lib.check(fn(C.byref(m), d_ids.data_ptr(), out.data_ptr(), B, torch.cuda.current_stream().cuda_stream), name)
        got = out.cpu().numpy()
        assert np.array_equal(got[B:].view(np.uint32), np.full(guard, -7.0, np.float32).view(np.uint32)), "wrote past prob[B]"
        return got[:B]

    return m32, m16, launch, (keep, keep2, d16), Pw, row_off


def _oracle(kind, P, row_off, layers, ids):
    return U.oracle_prob(P, row_off, layers, ids) if kind == "dcn" else S.oracle_prob(kind, P, row_off, layers, ids)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c + (0,) for c in FM_CASES] + DCN_CASES, ids=_id)
def test_16_bit_launch_is_bit_identical_to_the_fp32_launch_over_the_widened_tables(case, dtype):
    """1: np.array_equal probabilities at B = 1, 17, 200, planted subnormals and negative zeros included (example 0 of every
    request reads the planted rows); the guard after prob[B] keeps its bits."""
    kind, cols, layers, Lc = case
    m32, m16, launch, keep, Pw, row_off = _device_pair(kind, cols, layers, Lc, dtype)
    rng = np.random.default_rng(7)
    for B in BATCHES:
        ids = _request(rng, B, row_off)
        want, got = launch(m32, ids), launch(m16, ids)
        assert np.isfinite(got).all() and got.shape == (B,)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, float(np.abs(got - want).max()))


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [("fm", "criteo39", (), 0), ("deepfm", "criteo39", (100, 100), 0), ("dcn", "criteo39", (100, 100), 3)],
                         ids=_id)
def test_against_the_oracle_on_the_rounded_tables_and_really_16_bit(case, dtype):
    """2: |prob - oracle(rounded tables)| <= 1e-5, the project's bar, AND max |prob - oracle(original tables)| > 5e-5: the
    rounding moves these recipes' probabilities by 8.1e-5 (dcn, float16) to 5.5e-3 (deepfm, bfloat16), so a kernel or a loader
    that fell back to fp32 values fails the second condition."""
    kind, cols, layers, Lc = case
    m32, m16, launch, keep, Pw, row_off = _device_pair(kind, cols, layers, Lc, dtype)
    P, _ = _params(kind, cols, layers, Lc)
    ids = _request(np.random.default_rng(7), 200, row_off)
    got = launch(m16, ids)
    err = float(np.abs(got - _oracle(kind, Pw, row_off, layers, ids)).max())
    pf = _planted_fields(row_off)
    clean = ~(ids[:, pf] == 1).any(axis=1)               # examples that read no planted row: only the rounding moved them
    assert not clean[0] and clean.sum() >= 150, int(clean.sum())
    shift = float(np.abs(got - _oracle(kind, P, row_off, layers, ids))[clean].max())
    print("%s %s %s: max |prob - oracle(rounded)| = %.3g, max |prob - oracle(original)| = %.3g" % (kind, cols, dtype, err, shift))
    assert err <= 1e-5, err
    assert shift > 5e-5, shift


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def _exported(tmp_path, kind, dtype):
    """A criteo39 100-100 Estimator exported in `dtype`, and an fp32 bundle holding the same rounded tables."""
    from recsys_amd import serving
    if kind == "dcn":
        est, P, row_off = SD._estimator("criteo39", (100, 100), 3, 64)
    else:
        est, P, row_off = S._estimator("deepfm", "criteo39", (100, 100), 64)
    d16 = est.export_savedmodel(str(tmp_path / "e16"), table_dtype=dtype)
    manifest, arrays = serving.read_bundle(d16)
    wide = serving.widen_tensors(manifest, arrays)
    d32 = serving.write_bundle(str(tmp_path / "e32"), serving.make_manifest(kind, est.params, est.global_step, wide), wide)
    return est, row_off, d16, d32, arrays


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["deepfm", "dcn"])
def test_predictor_serves_a_16_bit_bundle_from_16_bit_device_tables(tmp_path, kind, dtype):
    """3: path == "fused", table_dtype, no Estimator; bit-equal to a Predictor over an fp32 bundle of the rounded tables at 1,
    37, 200 and 1000 rows (max_batch_size 512: the last is chunked); replayed == eager; a row alone == at position 37."""
    from recsys_amd import serving
    est, row_off, d16, d32, arrays = _exported(tmp_path, kind, dtype)
    del est
    kw = {"one_launch": True} if kind == "dcn" else {}
    p16 = serving.Predictor.load(d16, max_batch_size=512, **kw)
    p32 = serving.Predictor.load(d32, max_batch_size=512, **kw)
    eager = serving.Predictor.load(d16, max_batch_size=512, use_hip_graph=False, **kw)
    assert p16.path == p32.path == eager.path == "fused" and p16._est is None
    assert p16.table_dtype == dtype and p32.table_dtype == "float32" and p16.manifest["format_version"] == 2
    assert p16._tables.element_size() == 2 and p32._tables.element_size() == 4 and p16._model.table_dtype == {"bfloat16": 1, "float16": 2}[dtype]
    rng = np.random.default_rng(3)
    bits = lambda x: x.view(np.uint32)
    for B in (1, 37, 200, 1000):
        ids = _request(rng, B, row_off)
        want = p32.predict({"ids": ids})["prob"]
        for it in range(3):                              # eager warm-up, capture + replay, replay
            got = p16.predict({"ids": ids})["prob"]
            assert got.shape == (B,) and got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (B, it)
        assert np.array_equal(bits(eager.predict({"ids": ids})["prob"]), bits(want)), B
    assert "graph" in p16._graphs[200] and "graph" in p16._graphs[488] and not eager._graphs
    a = _request(rng, 200, row_off)
    whole = p16.predict({"ids": a})["prob"]
    for pr in (p16, eager):
        one = pr.predict({"ids": a[37:38]})["prob"]
        assert one.shape == (1,) and bits(one)[0] == bits(whole)[37]
    assert arrays["emb.input_layer.tables"].dtype == (np.uint16 if dtype == "bfloat16" else np.float16)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["deepfm", "dcn"])
def test_16_bit_load_saves_the_table_bytes_on_the_device(tmp_path, kind, dtype):
    """4: torch.cuda.memory_allocated around `load`: the 16-bit load is below the fp32 load of the same model by at least
    0.9 x R x 16 x 2 bytes, and below twice the bundle's own variable bytes."""
    from recsys_amd import serving
    est, row_off, d16, d32, arrays = _exported(tmp_path, kind, dtype)
    del est
    R, D = arrays["emb.input_layer.tables"].shape
    nbytes16 = sum(v.nbytes for v in arrays.values())
    assert D == 16 and arrays["emb.input_layer.tables"].nbytes == R * 16 * 2
    del arrays
    kw = {"one_launch": True} if kind == "dcn" else {}
    used = {}
    for name, d in (("float32", d32), (dtype, d16)):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        p = serving.Predictor.load(d, device="cuda", max_batch_size=4096, **kw)
        torch.cuda.synchronize()
        used[name] = torch.cuda.memory_allocated() - before
        assert p.path == "fused" and p.table_dtype == name
        del p
    print("%s Predictor.load: %d device bytes with float32 tables, %d with %s (%d bytes of variables in the bundle)"
          % (kind, used["float32"], used[dtype], dtype, nbytes16))
    assert used["float32"] - used[dtype] >= 0.9 * R * 16 * 2
    assert nbytes16 <= used[dtype] < 2 * nbytes16


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def _round_tables_in_place(est, dtype):
    """Sets every embedding-row tensor of the Estimator's store to its rounded values -> how many tensors that were."""
    from recsys_amd import serving
    D, n = int(est.params["embedding_size"]), 0
    with torch.no_grad():
        for name, a in est.store.embeddings.items():
            for attr in ("tables", "table"):
                t = getattr(a, attr, None)
                if t is not None and serving.is_embedding_rows("emb.%s.%s" % (name, attr), tuple(t.shape), D):
                    v = t.detach().float().cpu().numpy()
                    t.copy_(torch.from_numpy(serving.dequantize_rows(serving.quantize_rows(v, dtype, attr), ENC[dtype])))
                    n += 1
    return n


@pytest.mark.parametrize("mod", ["dcn", "din"])
def test_layers_path_answers_like_an_estimator_holding_the_rounded_tables(tmp_path, mod):
    """5: a bfloat16 dcn.py bundle without one_launch and a bfloat16 din.py bundle report path == "layers" and are
    bit-identical to the Estimator whose tables were set to the rounded values; din.py's rank_candidates works unchanged."""
    from recsys_amd import serving
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.feature_columns import build_feature_columns
    m = importlib.import_module("recsys_amd." + mod)
    if mod == "din":
        params = {"embedding_size": 32, "learning_rate": 1e-3, "dropout": 0.5, "max_batch_size": 64, "hist_len": 30,
                  "n_item": 300, "n_cate": 20}
        reqs = S._din_requests(tmp_path, 24, 30)
    else:
        lin, emb = build_feature_columns(16, "numeric")
        params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
                  "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": 64, "cross_layers": 3}
        reqs = S._requests(os.path.join(G, "criteo_24.tfrecord"), 24)
    est = Estimator(m.model_fn, None, params, RunConfig(device="cuda", seed=5))
    unrounded = est.predict_examples(reqs)["prob"]                            # (creates the variables)
    d = est.export_savedmodel(str(tmp_path / "export"), table_dtype="bfloat16")
    manifest, arrays = serving.read_bundle(d)
    assert manifest["table_dtype"] == "bfloat16"
    stored = sorted(k for k, v in arrays.items() if v.dtype == np.uint16)
    assert stored == (["emb.i_cate.table", "emb.i_id.table"] if mod == "din" else ["emb.input_layer.tables"])
    assert all(v.dtype == np.float32 for k, v in arrays.items() if k not in stored)
    assert _round_tables_in_place(est, "bfloat16") == len(stored)
    want = est.predict_examples(reqs)["prob"]
    assert not np.array_equal(want, unrounded)                                # the rounding is visible in the answer
    p = serving.Predictor.load(d, max_batch_size=64)
    assert p.path == "layers" and p.script == mod and p.table_dtype == "bfloat16"
    for _ in range(3):                                                        # eager, captured, replayed
        got = p.predict_examples(reqs)["prob"]
        assert got.shape == (24,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if mod == "din":
        from recsys_amd import synthetic
        b = synthetic.din_batch(np.random.default_rng(1), 24, P=30, n_item=300, n_cate=20)
        hi, hc, ci, cc = b["u_iid_seq"][0], b["u_icat_seq"][0], b["i_id"], b["i_cate"]
        got = p.rank_candidates(hi, hc, ci, cc)["prob"]
        ref = p.predict(serving.expand_rank_request(hi, hc, ci, cc, hist_len=30))["prob"]
        print("din bfloat16 bundle: rank_path %s, rank_candidates vs predict(expand_rank_request): %.3g"
              % (p.rank_path, float(np.abs(got - ref).max())))
        assert got.shape == (24,) and np.abs(got - ref).max() <= 2e-5


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_deepfm_script_train_export_bfloat16_predict(tmp_path):
    """6: python -m recsys_amd.deepfm --task_type train, then --task_type export --export_table_dtype bfloat16, then
    Predictor.load(export_path).predict_examples: finite, the right shape, within 1e-5 of the oracle on the bundle's own
    (rounded) tables."""
    from oracle import models, nn
    from recsys_amd import deepfm, serving
    d = str(tmp_path) + "/"
    S._golden_shards(d)
    model_dir, export_path = str(tmp_path / "model"), str(tmp_path / "export")
    common = ["--train_path", d, "--train_parts", "4", "--eval_parts", "1", "--batch_size", "8", "--model_dir", model_dir,
              "--save_checkpoints_steps", "8", "--log_steps", "4", "--dropout", "0.1", "--learning_rate", "0.01",
              "--export_path", export_path]
    res = deepfm.main(common + ["--task_type", "train", "--num_epochs", "3"])
    d1 = deepfm.main(common + ["--task_type", "export", "--export_table_dtype", "bfloat16"])
    p = serving.Predictor.load(export_path)
    assert p.bundle_dir == d1 and p.path == "fused" and p.table_dtype == "bfloat16" and p.global_step == res["global_step"]
    assert p._tables.element_size() == 2
    reqs = S._requests(d + "part-r-00003", 10)
    got = p.predict_examples(reqs)["prob"]
    manifest, arrays = serving.read_bundle(d1)
    assert arrays["emb.input_layer.tables"].dtype == np.uint16 and arrays["emb.input_layer.w1"].dtype == np.float32
    wide = serving.widen_tensors(manifest, arrays)
    P = {k.split(".", 2)[2] if k.startswith("emb.") else k[len("dense."):]: v for k, v in wide.items()}
    ids = p._parse(reqs)["ids"]
    want = nn.sigmoid(models.DeepFM(P, np.asarray(p.layout.row_off, np.int64), 2, 0.0).forward(np.asarray(ids), train=False)).reshape(-1)
    err = float(np.abs(got - want).max())
    print("deepfm --export_table_dtype bfloat16: Predictor vs oracle on the rounded tables: %.3g" % err)
    assert got.shape == (10,) and got.dtype == np.float32 and np.isfinite(got).all() and err <= 1e-5
    assert 0.0 < float(got.std())
