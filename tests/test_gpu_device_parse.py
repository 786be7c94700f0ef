"""The device parse on the GPU: rsx_criteo_parse_examples (csrc/parse_examples.hip) through the C ABI against the host parser
and against its host twin's status words, and `Predictor.load(..., device_parse=True)` against the same Predictor without the
flag -- bit for bit, eager and replayed, two launches per request, with the host fallback for whatever the device declines and
for bundles outside the envelope."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import device_parse_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def lay():
    return U.layout()


@pytest.fixture(scope="module")
def arrays(lay):
    from recsys_amd.input_pipeline import criteo_parse_spec
    return criteo_parse_spec(lay)


@pytest.fixture(scope="module")
def corpus(lay, arrays):
    return U.canonical_corpus(lay, arrays)


@pytest.fixture(scope="module")
def pool(corpus):
    """Records with more than 64 map entries first, then every tenth record of the corpus (all three writers)."""
    return corpus[1260::70] + corpus[::10]


@pytest.fixture(scope="module")
def host_ids(pool, lay):
    ids, rc = U.host_parse(pool, lay)
    assert not rc.any()
    return ids


def _long_record():
    return U.example([U.entry("_c%d" % j, 1.0) for j in range(1, 14)] + [U.entry("pad", b"x" * 9000)])


def _device_spec(arrays):
    from recsys_amd import _lib
    keep = {k: torch.from_numpy(arrays[k]).cuda() for k in ("slot_src", "slot_rows", "thr", "thr_off", "shift")}
    sp = _lib.ParseSpec()
    for k, t in keep.items():
        setattr(sp, k, t.data_ptr())
    sp.F, sp.null_hash = arrays["F"], arrays["null_hash"]
    return sp, keep


def _device_parse(records, lay, arrays, guard=4):
    """-> (ids [n + guard, F] as the device left them over a fill of -1, status [n + guard] over a fill of -7)."""
    from recsys_amd import _lib
    sp, keep = _device_spec(arrays)
    buf, offs = U.pack(records)
    n = len(records)
    d_buf, d_offs = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
    ids = torch.full((n + guard, lay.F), -1, dtype=torch.int32, device="cuda")
    status = torch.full((n + guard,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().rsx_criteo_parse_examples(d_buf.data_ptr(), buf.size, d_offs.data_ptr(), n, C.byref(sp), ids.data_ptr(),
                                                    status.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "rsx_criteo_parse_examples")
    torch.cuda.synchronize()
    return ids.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 17, 200])
def test_kernel_through_the_c_abi_against_the_host_parser(n, pool, host_ids, lay, arrays):
    """ids array_equal to rsx_criteo_parse_h's and every status 0; nothing is written past row n."""
    recs = pool[:n]
    assert recs[0].count(b"pad") >= 30                          # more than 64 map entries in one record
    if n == 200:                                                # all four hash branches, absent categoricals, threshold ids
        null_id = arrays["null_hash"] % arrays["slot_rows"].astype(np.uint64)
        cat = arrays["slot_src"] >= 14
        assert (host_ids[:n][:, cat] == null_id[cat].astype(np.int32)).any(axis=0).all()
        assert max(map(len, recs)) > 2000
    ids, status = _device_parse(recs, lay, arrays)
    assert np.all(status[:n] == 0), status[:n]
    assert np.array_equal(ids[:n], host_ids[:n])
    assert np.all(ids[n:] == -1) and np.all(status[n:] == -7)


def test_declined_examples_carry_the_host_twins_status(corpus, pool, host_ids, lay, arrays):
    """8 declined examples (mutations the host twin declined on the CPU: 4 malformed, 3 without a numeric; and a record above
    the LDS stage) interleaved with 8 valid ones: the status words equal the twin's, the valid rows' ids are the host's."""
    muts = U.mutation_corpus(corpus, n=2000)
    _, st = U.twin_parse(muts, lay, arrays)
    declined = [muts[i] for i in np.flatnonzero(st == 1)[:4]] + [muts[i] for i in np.flatnonzero(st == 2)[:3]] + [_long_record()]
    assert len(declined) == 8
    recs = [r for pair in zip(declined, pool[:8]) for r in pair]
    t_ids, t_status = U.twin_parse(recs, lay, arrays)
    assert list(t_status) == [1, 0, 1, 0, 1, 0, 1, 0, 2, 0, 2, 0, 2, 0, 3, 0]
    ids, status = _device_parse(recs, lay, arrays)
    assert np.array_equal(status[:16], t_status)
    assert np.array_equal(ids[:16], t_ids)                      # (declined rows: not written, -1 on both sides)
    assert np.array_equal(ids[1:16:2], host_ids[:8])


# ---- Predictor level -------------------------------------------------------------------------------------------------------
def _bundle(tmp, kind, table_dtype="float32"):
    """A tiny exported model of `kind` (random variables) -> its bundle directory."""
    from recsys_amd import serving
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.feature_columns import build_feature_columns, build_model_columns
    script = {"uid_iid": "deepfm"}.get(kind, kind)
    m = importlib.import_module("recsys_amd." + script)
    if kind == "din":
        params = {"embedding_size": 32, "learning_rate": 1e-3, "dropout": 0.5, "max_batch_size": 64, "hist_len": 30,
                  "n_item": 300, "n_cate": 20}
    else:
        lin, emb = build_model_columns(16) if kind == "uid_iid" else \
            build_feature_columns(16, {"dcn": "numeric", "xdeepfm": "numeric+indicator"}.get(kind, "indicator_all"))
        params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
                  "dropout": 0.5, "deep_layers": "100,100" if kind == "xdeepfm" else "8,8", "max_batch_size": 64}
        if kind in ("dcn", "xdeepfm"):
            params["cross_layers"] = {"dcn": 3, "xdeepfm": "32,16"}[kind]
    est = Estimator(m.model_fn, None, params, RunConfig(device="cuda", seed=5))
    serving._build_store(est, script)
    return est.export_savedmodel(str(tmp / kind), table_dtype=table_dtype)


@pytest.fixture(scope="module")
def bundles(tmp_path_factory):
    tmp, made = tmp_path_factory.mktemp("bundles"), {}

    def get(kind, table_dtype="float32"):
        if (kind, table_dtype) not in made:
            made[kind, table_dtype] = _bundle(tmp / table_dtype, kind, table_dtype)
        return made[kind, table_dtype]
    return get


def _bits(x):
    return x.view(np.uint32)


@pytest.mark.parametrize("kind,table_dtype", [("deepfm", "float32"), ("fm", "float32"), ("dcn", "float32"), ("deepfm", "bfloat16")])
def test_predictor_device_parse_equals_host_parse_bit_for_bit(bundles, pool, kind, table_dtype):
    """n = 1, n = 200, and n = 150 with max_batch_size 64 (3 chunks, the last partial); eager, captured and replayed."""
    from recsys_amd import serving
    d = bundles(kind, table_dtype)
    kw = {"one_launch": True} if kind == "dcn" else {}
    for mbs, sizes in ((256, (1, 200)), (64, (150,))):
        off = serving.Predictor.load(d, max_batch_size=mbs, **kw)
        on = serving.Predictor.load(d, max_batch_size=mbs, device_parse=True, **kw)
        assert off.path == on.path == "fused" and off.parse_path == "host" and on.parse_path == "device"
        assert on.table_dtype == table_dtype
        for n in sizes:
            want = off.predict_examples(pool[:n])["prob"]
            assert want.shape == (n,) and (n == 1 or float(want.std()) > 0.0)
            for it in range(3):
                got = on.predict_examples(pool[:n])["prob"]
                assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)), (kind, n, it)
        if mbs == 64:
            assert "graph" in on._graphs[("examples", 64)] and ("examples", 22) in on._graphs


def test_two_launches_per_request_and_replay_equals_eager(bundles, pool):
    from recsys_amd import _lib, serving
    d = bundles("deepfm")
    eager = serving.Predictor.load(d, max_batch_size=256, use_hip_graph=False, device_parse=True)
    graph = serving.Predictor.load(d, max_batch_size=256, use_hip_graph=True, device_parse=True)
    L = _lib.lib()
    for n in (1, 16, 200, 256):
        reqs = (pool + pool)[:n]
        eager.predict_examples(reqs)
        n0 = L.rsx_dbg_launch_count()
        eager.predict_examples(reqs)
        assert L.rsx_dbg_launch_count() - n0 == 2, n            # the parse launch + the predict launch
    a, b = pool[:200], pool[100:137]
    ea, eb = eager.predict_examples(a)["prob"], eager.predict_examples(b)["prob"]
    for it in range(4):                                         # call 0: eager warm-up, call 1: capture + replay, then replays
        ga, gb = graph.predict_examples(a)["prob"], graph.predict_examples(b)["prob"]
        assert np.array_equal(_bits(ga), _bits(ea)) and np.array_equal(_bits(gb), _bits(eb)), it
    assert "graph" in graph._graphs[("examples", 200)] and "graph" in graph._graphs[("examples", 37)]
    a2 = pool[11:211]                                            # a replay reads the NEW request, not the captured one
    assert np.array_equal(_bits(graph.predict_examples(a2)["prob"]), _bits(eager.predict_examples(a2)["prob"]))
    assert np.array_equal(_bits(graph.predict_examples(a)["prob"]), _bits(ea))


def test_fallback_to_the_host_parse(bundles, corpus, pool, lay, arrays):
    from recsys_amd import _lib, serving
    from recsys_amd._lib import RsxError
    d = bundles("deepfm")
    off = serving.Predictor.load(d, max_batch_size=64, use_hip_graph=False)
    on = serving.Predictor.load(d, max_batch_size=64, use_hip_graph=False, device_parse=True)
    # a valid request the device declines (a record above 8 KB): the host path's probabilities
    reqs = pool[:5] + [_long_record()] + pool[5:9]
    assert np.array_equal(_bits(on.predict_examples(reqs)["prob"]), _bits(off.predict_examples(reqs)["prob"]))
    # a malformed one: the host path's error, word for word
    muts = U.mutation_corpus(corpus, n=2000)
    _, st = U.twin_parse(muts, lay, arrays)
    bad = pool[:3] + [muts[int(np.flatnonzero(st == 1)[0])]] + pool[3:5]
    with pytest.raises(RsxError) as e_off:
        off.predict_examples(bad)
    with pytest.raises(RsxError) as e_on:
        on.predict_examples(bad)
    assert str(e_on.value) == str(e_off.value)
    # a chunk over the byte budget: parsed on the host (ONE launch, not two), same probabilities
    tight = serving.Predictor.load(d, max_batch_size=64, use_hip_graph=False, device_parse=True, parse_row_bytes=16)
    assert tight.parse_path == "device"
    L = _lib.lib()
    n0 = L.rsx_dbg_launch_count()
    got = tight.predict_examples(pool[:20])["prob"]
    assert L.rsx_dbg_launch_count() - n0 == 1
    assert np.array_equal(_bits(got), _bits(off.predict_examples(pool[:20])["prob"]))
    assert np.array_equal(_bits(tight.predict_examples(pool[1:2])["prob"]), _bits(off.predict_examples(pool[1:2])["prob"]))


@pytest.mark.parametrize("kind", ["xdeepfm", "din", "uid_iid", "dcn_layers"])
def test_bundles_outside_the_envelope_keep_the_host_parse(bundles, tmp_path, kind):
    from oracle import tfrecord
    from recsys_amd import serving
    d = bundles("dcn" if kind == "dcn_layers" else kind)
    if kind == "din":
        from tests.test_gpu_serving import _din_requests
        reqs = _din_requests(tmp_path, 24, 30)
    elif kind == "uid_iid":
        reqs = [tfrecord.encode_example({"u_id": [3 * i + 1], "i_id": [7 * i + 2]}) for i in range(24)]
    else:
        # ordinary numerics only: xdeepfm.py's linear part consumes log(x + shift) itself, so the corpus' NaN, inf and
        # negative values would make most probabilities NaN and the comparison below say little
        rng = np.random.default_rng(3)
        reqs = [tfrecord.encode_example(dict(
            [("_c%d" % j, [float(np.floor(np.exp(rng.normal(2, 2))))]) for j in range(1, 14)] +
            [("_c%d" % j, [b"%08x" % rng.integers(0, 1 << 32)]) for j in range(14, 40)])) for _ in range(24)]
    off = serving.Predictor.load(d, max_batch_size=64)
    on = serving.Predictor.load(d, max_batch_size=64, device_parse=True)
    assert on.parse_path == "host" and on.path == off.path
    assert on.manifest["feature_set"] == {"din": "din", "uid_iid": "uid_iid"}.get(kind, "criteo")
    want = off.predict_examples(reqs)["prob"]
    for _ in range(2):
        assert np.array_equal(_bits(on.predict_examples(reqs)["prob"]), _bits(want))
    assert want.shape == (24,) and np.isfinite(want).all() and float(want.std()) > 0.0
