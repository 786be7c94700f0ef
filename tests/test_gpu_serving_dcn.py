"""dcn.py serving in one launch on the GPU: rsx_predict_dcn (csrc/predict_dcn.hip) against the oracle's inference forward
through the C ABI, `Predictor.load(..., one_launch=True)` against the `Estimator` it was exported from, one launch per
request, replayed == eager, row independence, device memory, and dcn.py's own train -> export -> Predictor chain.

The checker is nn.sigmoid(models.DCN(...).forward(ids, train=False)) on the recipe of tests/dcn_serving_util.py;
tests/test_predict_dcn_cpu.py shows that this fixture moves by more than 1e-4 when any piece of the cross branch is dropped."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from tests import dcn_serving_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCHES = (1, 7, 16, 17, 200, 256, 1000)


def device_model(P, row_off, layers, Lc):
    """-> (rsx_predict_dcn_model over device copies of the oracle's parameters, the tensors that keep them alive)."""
    from recsys_amd import _lib
    F = len(row_off) - 1
    t = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1)).cuda() for k, v in P.items()}
    t["row_off"] = torch.from_numpy(np.asarray(row_off[:-1], np.int32)).cuda()
    m = _lib.PredictDcnModel()
    m.tables, m.row_off = t["tables"].data_ptr(), t["row_off"].data_ptr()
    m.cross_W, m.cross_b = t["cross.W"].data_ptr(), t["cross.b"].data_ptr()
    for l, n in enumerate(layers):
        m.W[l], m.b[l] = t["dnn.W%d" % l].data_ptr(), t["dnn.b%d" % l].data_ptr()
        m.gamma[l], m.beta[l] = t["dnn.gamma%d" % l].data_ptr(), t["dnn.beta%d" % l].data_ptr()
        m.widths[l] = n
    m.wo, m.bo = t["out.W"].data_ptr(), t["out.b"].data_ptr()
    m.bn_eps, m.F, m.D, m.L, m.Lc = 1e-3, F, 16, len(layers), Lc
    return m, t


@pytest.mark.parametrize("cols", U.COLS)
@pytest.mark.parametrize("layers,Lc", U.CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_against_the_oracle_through_the_c_abi(cols, layers, Lc):
    """1: max |prob - oracle| <= 1e-5 (the bar every model of this project is held to) at every batch size, ragged ones
    included; a guard after prob[B] keeps its bits; (32, 18) reads out.W's cross part from an address that is only 4-byte
    aligned."""
    from recsys_amd import _lib
    from tests.parity_util import synth_ids
    P, row_off = U.perturbed_dcn_params(cols, layers, Lc)
    m, keep = device_model(P, row_off, layers, Lc)
    F = len(row_off) - 1
    L = _lib.lib()
    assert L.rsx_predict_dcn_supported(max(BATCHES), F, 16, len(layers), (C.c_int32 * 3)(*layers), Lc) == 1
    rng = np.random.default_rng(7)
    worst = 0.0
    for B in BATCHES:
        ids = synth_ids(rng, B, row_off)
        want = U.oracle_prob(P, row_off, layers, ids)
        d_ids = torch.from_numpy(ids).cuda()
        out = torch.full((B + 64,), -7.0, device="cuda")
        _lib.check(L.rsx_predict_dcn(C.byref(m), d_ids.data_ptr(), out.data_ptr(), B, torch.cuda.current_stream().cuda_stream),
                   "rsx_predict_dcn")
        got = out.cpu().numpy()
        err = float(np.abs(got[:B] - want).max())
        print("predict dcn %s %s Lc=%d B=%d: max |prob - oracle| = %.3g" % (cols, layers, Lc, B, err))
        worst = max(worst, err)
        assert np.all(got[B:] == -7.0), "B=%d: the kernel wrote past prob[B]" % B
        assert np.isfinite(got[:B]).all(), B
        assert err <= 1e-5, (B, err)
    print("predict dcn %s %s Lc=%d: worst %.3g" % (cols, layers, Lc, worst))
    assert worst <= 1e-5


def _estimator(cols, layers, Lc, B, use_graph=False):
    """An Estimator holding the perturbed oracle weights -> (est, P, row_off)."""
    from recsys_amd import dcn
    from recsys_amd.estimator import ModeKeys
    from recsys_amd.feature_columns import build_feature_columns
    from tests.parity_util import load_oracle_weights, make_estimator, small_columns
    P, row_off = U.perturbed_dcn_params(cols, layers, Lc)
    lin, emb = build_feature_columns(16, "numeric") if cols == "criteo39" else small_columns(U.SMALL_ROWS, 16)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
              "dropout": 0.5, "deep_layers": ",".join(map(str, layers)), "cross_layers": Lc, "max_batch_size": B}
    est = make_estimator(dcn.model_fn, params, use_graph=use_graph)
    with torch.no_grad():
        est._call_model_fn({"ids": torch.zeros(1, len(row_off) - 1, dtype=torch.int32, device="cuda")}, None, ModeKeys.PREDICT)
    load_oracle_weights(est, P)
    return est, P, row_off


def _est_prob(est, ids):
    from recsys_amd.estimator import ModeKeys
    with torch.no_grad():
        p = est._call_model_fn({"ids": torch.from_numpy(ids).cuda()}, None, ModeKeys.PREDICT).predictions["prob"]
    return p.reshape(-1).float().cpu().numpy()


def _requests(path, n):
    """The first n records of a shard as a serving client sends them: serialized Examples without the label."""
    from oracle import tfrecord
    out = []
    for rec in list(tfrecord.unframe(open(path, "rb").read()))[:n]:
        ex = tfrecord.decode_example(rec)
        ex.pop("_c0", None)
        out.append(tfrecord.encode_example(ex))
    return out


@pytest.mark.parametrize("cols,layers,Lc", [("criteo39", (100, 100), 3), ("small", (64, 32, 16), 2)])
def test_predictor_against_the_estimator_it_was_exported_from(tmp_path, cols, layers, Lc):
    """2: same inputs, <= 2e-5 (both sit within 1e-5 of the same oracle) on the fused path; without the flag the same bundle
    is served through the layers path."""
    from recsys_amd import serving
    from tests.parity_util import synth_ids
    est, P, row_off = _estimator(cols, layers, Lc, 1024)
    d = est.export_savedmodel(str(tmp_path / "export"))
    p = serving.Predictor.load(d, max_batch_size=512, one_launch=True)
    assert p.path == "fused" and p.script == "dcn" and p._est is None
    rng = np.random.default_rng(3)
    for B in (1, 37, 200, 512, 1000):                    # (1000 > max_batch_size: two chunks)
        ids = synth_ids(rng, B, row_off)
        got = p.predict({"ids": ids})["prob"]
        want = _est_prob(est, ids)
        err = float(np.abs(got - want).max())
        print("dcn Predictor(one_launch) vs Estimator %s B=%d: %.3g; vs oracle %.3g"
              % (cols, B, err, float(np.abs(got - U.oracle_prob(P, row_off, layers, ids)).max())))
        assert got.shape == (B,) and got.dtype == np.float32 and err <= 2e-5, (B, err)
    assert serving.Predictor.load(d, max_batch_size=512).path == "layers"
    if cols == "criteo39":
        reqs = _requests(os.path.join(G, "criteo_24.tfrecord"), 24)
        got, want = p.predict_examples(reqs)["prob"], est.predict_examples(reqs)["prob"]
        err = float(np.abs(got - want).max())
        print("dcn Predictor(one_launch).predict_examples vs Estimator.predict_examples, 24 golden records: %.3g" % err)
        assert got.shape == (24,) and err <= 2e-5


def test_the_flag_falls_back_outside_the_envelope_and_refuses_a_foreign_tensor_set(tmp_path):
    """A tower of 4 layers is outside rsx_predict_dcn's envelope: path says "layers".  A dcn bundle with a tensor a dcn.py
    store does not export is refused in _fused_setup's message form."""
    from recsys_amd import serving
    from recsys_amd._lib import RsxError
    est, P, row_off = _estimator("small", (64, 32, 16), 2, 64)
    d = est.export_savedmodel(str(tmp_path / "export"))
    manifest, arrays = serving.read_bundle(d)
    arrays["dense.b1"] = np.zeros(1, np.float32)
    bad = serving.write_bundle(str(tmp_path / "bad"), serving.make_manifest("dcn", est.params, 0, arrays), arrays)
    with pytest.raises(RsxError, match="a dcn bundle holds the tensors"):
        serving.Predictor.load(bad, max_batch_size=64, one_launch=True)
    from recsys_amd import dcn
    from recsys_amd.estimator import Estimator, RunConfig
    from tests.parity_util import small_columns
    lin, emb = small_columns(U.SMALL_ROWS, 16)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
              "dropout": 0.5, "deep_layers": "32,32,32,16", "cross_layers": 2, "max_batch_size": 64}
    est4 = Estimator(dcn.model_fn, None, params, RunConfig(device="cuda", seed=5))
    ids = np.zeros((3, 5), np.int32)
    want = _est_prob(est4, ids)                            # (creates the variables)
    p = serving.Predictor.load(est4.export_savedmodel(str(tmp_path / "deep")), max_batch_size=64, one_launch=True)
    assert p.path == "layers"
    assert np.abs(p.predict({"ids": ids})["prob"] - want).max() <= 2e-5


def test_one_launch_per_request(tmp_path):
    """3: the fused path is ONE library launch per request (eager mode); the layers path takes several."""
    from recsys_amd import _lib, serving
    from tests.parity_util import synth_ids
    est, P, row_off = _estimator("criteo39", (100, 100), 3, 256)
    d = est.export_savedmodel(str(tmp_path))
    p = serving.Predictor.load(d, max_batch_size=256, use_hip_graph=False, one_launch=True)
    q = serving.Predictor.load(d, max_batch_size=256, use_hip_graph=False)
    assert p.path == "fused" and q.path == "layers"
    L = _lib.lib()
    rng = np.random.default_rng(5)
    for B in (1, 16, 200, 256):
        ids = synth_ids(rng, B, row_off)
        p.predict({"ids": ids})
        n0 = L.rsx_dbg_launch_count()
        p.predict({"ids": ids})
        assert L.rsx_dbg_launch_count() - n0 == 1, B
        q.predict({"ids": ids})
        n0 = L.rsx_dbg_launch_count()
        q.predict({"ids": ids})
        n_layers = L.rsx_dbg_launch_count() - n0
        print("dcn B=%d: launches per request: fused 1, layers %d" % (B, n_layers))
        assert n_layers > 1, B


def test_replayed_equals_eager_and_rows_are_independent(tmp_path):
    """4: graph replay == eager bit for bit; a row's probability does not depend on its position or on the rows that share
    its batch; a replay reads the new request; the number of captured sizes is capped."""
    from recsys_amd import serving
    from tests.parity_util import synth_ids
    est, P, row_off = _estimator("criteo39", (100, 100), 3, 256)
    d = est.export_savedmodel(str(tmp_path))
    eager = serving.Predictor.load(d, max_batch_size=256, use_hip_graph=False, one_launch=True)
    graph = serving.Predictor.load(d, max_batch_size=256, use_hip_graph=True, one_launch=True)
    assert eager.path == graph.path == "fused"
    rng = np.random.default_rng(11)
    a, b = synth_ids(rng, 200, row_off), synth_ids(rng, 37, row_off)
    bits = lambda x: x.view(np.uint32)
    ea, eb = eager.predict({"ids": a})["prob"], eager.predict({"ids": b})["prob"]
    for it in range(4):                                   # call 0: eager warm-up, call 1: capture + replay, then replays
        ga, gb = graph.predict({"ids": a})["prob"], graph.predict({"ids": b})["prob"]
        assert np.array_equal(bits(ga), bits(ea)) and np.array_equal(bits(gb), bits(eb)), it
    assert "graph" in graph._graphs[200] and "graph" in graph._graphs[37]
    a2 = synth_ids(rng, 200, row_off)                     # a replay reads the NEW request, not the captured one
    assert np.array_equal(bits(graph.predict({"ids": a2})["prob"]), bits(eager.predict({"ids": a2})["prob"]))
    assert np.array_equal(bits(graph.predict({"ids": a})["prob"]), bits(ea))
    # the same row alone (position 0 of a 1-row request) and at position 37 of a 200-row one
    for pr in (eager, graph):
        for _ in range(3):
            one = pr.predict({"ids": a[37:38]})["prob"]
            assert one.shape == (1,) and bits(one)[0] == bits(ea)[37]
    # ... and next to other neighbours
    mixed = np.concatenate([b[:5], a[37:38], b[5:20]])
    assert bits(eager.predict({"ids": mixed})["prob"])[5] == bits(ea)[37]
    # ever-new request sizes: the number of captured sizes is capped, the rest stays eager and correct
    small = serving.Predictor.load(d, max_batch_size=256, use_hip_graph=True, one_launch=True)
    small.MAX_GRAPHS = 2
    for n in (3, 4, 5, 6, 3, 4, 5, 6, 3, 6):
        assert np.array_equal(bits(small.predict({"ids": a[:n]})["prob"]), bits(ea)[:n])
    assert len(small._graphs) == 2


def test_predictor_load_allocates_less_than_twice_the_variables(tmp_path):
    """5: the variables once plus request buffers of a few hundred KB at max_batch_size 4096."""
    from recsys_amd import serving
    est, P, row_off = _estimator("criteo39", (100, 100), 3, 256)
    d = est.export_savedmodel(str(tmp_path))
    manifest, arrays = serving.read_bundle(d)
    nbytes = sum(v.nbytes for v in arrays.values())
    del arrays
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    p = serving.Predictor.load(d, device="cuda", max_batch_size=4096, one_launch=True)
    torch.cuda.synchronize()
    used = torch.cuda.memory_allocated() - before
    print("dcn Predictor.load(one_launch): %d device bytes for %d bytes of variables (x %.3f)" % (used, nbytes, used / nbytes))
    assert p.path == "fused" and nbytes <= used < 2 * nbytes


def test_dcn_script_train_export_predict(tmp_path):
    """6: dcn.py's own `main`: train -> export -> Predictor.load(export_path, one_launch=True) answers the eval shard's
    records like --task_type infer."""
    from recsys_amd import dcn, serving
    d = str(tmp_path) + "/"
    for k in range(4):
        shutil.copy(os.path.join(G, "criteo_24.tfrecord"), os.path.join(d, "part-r-%05d" % k))
    model_dir, export_path = str(tmp_path / "model"), str(tmp_path / "export")
    common = ["--train_path", d, "--train_parts", "4", "--eval_parts", "1", "--batch_size", "8", "--model_dir", model_dir,
              "--save_checkpoints_steps", "8", "--log_steps", "4", "--dropout", "0.1", "--learning_rate", "0.01",
              "--export_path", export_path]
    res = dcn.main(common + ["--task_type", "train", "--num_epochs", "3"])
    d1 = dcn.main(common + ["--task_type", "export"])
    preds = dcn.main(common + ["--task_type", "infer"])
    want = np.array([float(p["prob"]) for p in preds], np.float32)
    p = serving.Predictor.load(export_path, one_launch=True)
    assert p.path == "fused" and p.bundle_dir == d1 and p.global_step == res["global_step"]
    got = p.predict_examples(_requests(d + "part-r-00003", 10))["prob"]       # the eval shard (--eval_parts 1)
    print("dcn: Predictor(one_launch) vs --task_type infer: %.3g" % float(np.abs(got - want).max()))
    assert got.shape == (10,) and np.abs(got - want).max() <= 2e-5
    assert 0.0 < float(want.std())
    assert serving.Predictor.load(export_path).path == "layers"
