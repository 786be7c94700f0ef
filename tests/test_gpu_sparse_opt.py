"""FTRL / Adagrad (rsx_sparse_opt_multi, csrc/sparse_opt.hip) on the MI355X: the launch against the fp32 restatement
(tests/opt_ref.py), the four Criteo models against the oracle, HIP graphs against eager, the scripts end to end, and the
refusals."""
import glob
import os

import numpy as np
import pytest

from tests.opt_ref import SparseOptRef, model_parity_run
from tests.parity_util import synth_ids

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FTRL_REG = {"l1_regularization_strength": 1e-3, "l2_regularization_strength": 1e-2}


def _opt(name, lr, hp):
    from recsys_amd.ops import AdagradTF1, FtrlTF1
    return AdagradTF1(lr=lr, **hp) if name == "adagrad" else FtrlTF1(lr=lr, **hp)


OP_CASES = [
    ("adagrad", {}, True),
    ("ftrl", {"l1_regularization_strength": 0.02, "l2_regularization_strength": 0.5}, True),
    ("ftrl", {"l1_regularization_strength": 0.02, "l2_regularization_strength": 0.5,
              "l2_shrinkage_regularization_strength": 0.1}, True),
    ("ftrl", {"learning_rate_power": -0.3, "l1_regularization_strength": 0.02, "l2_regularization_strength": 0.5}, False),
    ("ftrl", {"learning_rate_power": 0.0, "l1_regularization_strength": 0.02}, False),
]


@pytest.mark.parametrize("D", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("name,hp,exact", OP_CASES)
def test_sparse_opt_launch_matches_the_restatement(D, name, hp, exact):
    """arena -> field_sort -> segsum -> ONE rsx_sparse_opt_multi over the table rows (sparse form), the first-order vector
    (dense form) and a dense arena (n not a multiple of 4), over 6 steps with duplicate ids, an empty batch, l1 clamping and
    first-order elements first touched after step 1.  sqrt path: bit for bit; powf path: within a few ulp."""
    from recsys_amd import _lib
    from recsys_amd.ops import EmbeddingArena
    rng = np.random.default_rng(D * 7 + len(hp))
    row_off = np.array([0, 3, 40, 640], np.int64)          # a 3-row field: duplicates in every batch
    F, R, B, lr = 3, 640, 24, 0.05
    tables = (rng.standard_normal((R, D)) * 0.25).astype(np.float32)
    w1 = (rng.standard_normal(R) * 0.1).astype(np.float32)
    a = EmbeddingArena(row_off, D, B, "cuda", with_w1=True, tables=tables, w1=w1)
    opt = _opt(name, lr, hp)
    acc0 = np.float32(opt.initial_accumulator_value)
    a.v_t.fill_(float(acc0))
    a.v_w.fill_(float(acc0))
    nd = 37
    dvar = (rng.standard_normal(nd) * 0.3).astype(np.float32)
    dense = {k: torch.from_numpy(v).cuda() for k, v in (("var", dvar), ("m", np.zeros(nd, np.float32)),
                                                         ("v", np.full(nd, acc0, np.float32)), ("g", np.zeros(nd, np.float32)))}
    ref = SparseOptRef(name, lr, **hp)
    T, W, DV = tables.copy(), w1.copy(), dvar.copy()
    touched_at = {}
    empty_step = 3
    for step in range(6):
        dg = (rng.standard_normal(nd) * 0.2).astype(np.float32)
        dense["g"].copy_(torch.from_numpy(dg))
        dseg = dict(kind=_lib.RSX_ADAM_DENSE, n=nd, var=dense["var"], m=dense["m"], v=dense["v"], g=dense["g"], zero_grad=1)
        if step == empty_step:
            # an empty batch: no table row, no touched element of the vector
            slot = torch.full((R + 4,), -1, dtype=torch.int32, device="cuda")
            segs = [dict(kind=_lib.RSX_ADAM_TABLE_ROWS, d=D, n=0, var=a.tables, m=a.m_t, v=a.v_t, g=a.G, uniq_row=a.uniq_row,
                         nuniq=a.nuniq, B=0, stride=a.stride),
                    dict(kind=_lib.RSX_ADAM_VEC_SLOT, n=R, var=a.w1, m=a.m_w, v=a.v_w, g=a.gw1, slot=slot), dseg]
            rows, G, gw = np.zeros(0, np.int64), np.zeros((0, D), np.float32), np.zeros(0, np.float32)
        else:
            ids = synth_ids(rng, B, row_off)
            dX = (rng.standard_normal((B, F * D)) * 0.3).astype(np.float32)
            gy1 = (rng.standard_normal(B) * 0.3).astype(np.float32)
            a.field_sort(torch.from_numpy(ids).cuda())
            a.segsum(B, None, torch.from_numpy(dX).cuda(), torch.from_numpy(gy1).cuda(), None)
            torch.cuda.synchronize()
            # the launch's inputs as the sort / segment-sum left them (this test is about the optimizer)
            nu, ur = a.nuniq.cpu().numpy(), a.uniq_row.cpu().numpy()
            Gd, gwd = a.G.cpu().numpy(), a.gw1.cpu().numpy()
            sl = np.concatenate([np.arange(f * a.stride, f * a.stride + nu[f]) for f in range(F)])
            rows, G, gw = ur[sl].astype(np.int64), Gd[sl], gwd[sl]
            assert len(rows) < F * B                      # duplicate ids were summed
            segs = a.sparse_opt_segments() + [dseg]
        for r in rows:
            touched_at.setdefault(int(r), step)
        opt.step(segs)
        ref.apply_sparse("t", T, rows, G)
        gfull = np.zeros(R, np.float32)
        gfull[rows] = gw
        ref.apply_dense("w", W, gfull)
        ref.apply_dense("d", DV, dg)
    torch.cuda.synchronize()
    assert min(touched_at.values()) == 0 and max(touched_at.values()) >= 2       # first touched after the first step
    assert opt.global_step == 6 and float(dense["g"].abs().max()) == 0.0       # every launch advanced the step; zero_grad
    got = {"tables": a.tables, "linear_t": a.m_t, "acc_t": a.v_t, "w1": a.w1, "linear_w": a.m_w, "acc_w": a.v_w,
           "dense": dense["var"], "linear_d": dense["m"], "acc_d": dense["v"]}
    want = {"tables": T, "linear_t": ref.slots["t"][0], "acc_t": ref.slots["t"][1], "w1": W, "linear_w": ref.slots["w"][0],
            "acc_w": ref.slots["w"][1], "dense": DV, "linear_d": ref.slots["d"][0], "acc_d": ref.slots["d"][1]}
    if name == "adagrad":
        for k in ("linear_t", "linear_w", "linear_d"):
            got.pop(k), want.pop(k)
    else:
        tr = np.array(sorted(touched_at))
        assert (T[tr] == 0).any() and (T[tr] != 0).any(), "l1 should clamp some touched rows to exactly 0"
    for k in got:
        g = got[k].cpu().numpy()
        if exact:
            assert np.array_equal(g.view(np.uint32), want[k].view(np.uint32)), (k, float(np.abs(g - want[k]).max()))
        else:
            np.testing.assert_allclose(g, want[k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_known_answers_through_the_kernel_as_dense_segments():
    """TF 1.x ftrl_test.py / adagrad_test.py vectors (tests/test_sparse_opt_cpu.py) through rsx_sparse_opt_multi."""
    from recsys_amd import _lib
    from tests.test_sparse_opt_cpu import FTRL_KNOWN
    cases = [("ftrl", v0, v1, n, hp, w0, w1, [0.1, 0.2], [0.01, 0.02]) for v0, v1, n, hp, w0, w1 in FTRL_KNOWN]
    cases.append(("adagrad", [1, 2], [3, 4], 3, {}, [-1.60260987, -0.60260987], [2.71567917, 3.71567917], [0.1, 0.1],
                  [0.01, 0.01]))
    for name, v0, v1, steps, hp, want0, want1, g0, g1 in cases:
        opt = _opt(name, 3.0, dict(hp, initial_accumulator_value=0.1))
        t = lambda x: torch.tensor(x, dtype=torch.float32, device="cuda")
        segs = [dict(kind=_lib.RSX_ADAM_DENSE, n=2, var=t(v), m=t([0, 0]), v=t([0.1, 0.1]), g=t(g)) for v, g in
                ((v0, g0), (v1, g1))]
        for _ in range(steps):
            opt.step(segs)
        np.testing.assert_allclose(segs[0]["var"].cpu().numpy(), want0, rtol=0, atol=1e-6, err_msg=str((name, hp)))
        np.testing.assert_allclose(segs[1]["var"].cpu().numpy(), want1, rtol=0, atol=1e-6, err_msg=str((name, hp)))


MODEL_CASES = [("fm", 0.0), ("deepfm", 0.0), ("deepfm", 0.5), ("dcn", 0.0), ("xdeepfm", 0.0)]


@pytest.mark.parametrize("opt_name,hp", [("adagrad", {}), ("ftrl", FTRL_REG)])
@pytest.mark.parametrize("kind,dropout", MODEL_CASES)
def test_models_train_like_the_oracle(kind, dropout, opt_name, hp):
    B = 64 if kind != "xdeepfm" else 32
    err, losses, perr = model_parity_run(kind, opt_name, hp, B=B, steps=4, seed=3, dropout=dropout,
                                         rows=None if kind == "xdeepfm" else (3, 7, 40, 11, 600))
    assert err < 1e-5, err
    for lg, lo in losses:
        assert abs(lg - lo) < 1e-5, losses
    assert max(perr.values()) < 1e-5, perr


@pytest.mark.parametrize("opt_name,hp", [("adagrad", {}), ("ftrl", FTRL_REG)])
def test_deepfm_criteo39_bs256_like_the_oracle(opt_name, hp):
    err, losses, perr = model_parity_run("deepfm", opt_name, hp, B=256, steps=4, seed=5, rows=None, layers=(100, 100))
    assert err < 1e-5, err
    for lg, lo in losses:
        assert abs(lg - lo) < 1e-5, losses
    assert max(perr.values()) < 5e-5, perr


def _deepfm_est(opt_name, hp, graph, dropout=0.5, lr=1e-3, model_dir=None, save_steps=None):
    from recsys_amd import deepfm
    from recsys_amd.estimator import Estimator, RunConfig
    from tests.parity_util import small_columns
    lin, emb = small_columns((3, 7, 40, 11, 600), 16)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": lr,
              "dropout": dropout, "deep_layers": "32,16", "max_batch_size": 64}
    return Estimator(deepfm.model_fn, model_dir, params,
                     RunConfig(use_hip_graph=graph, optimizer=opt_name, optimizer_hparams=hp, seed=4, log_step_count_steps=100,
                               save_checkpoints_steps=save_steps))


def _batches(n, seed=11):
    rng = np.random.default_rng(seed)
    row_off = np.concatenate([[0], np.cumsum((3, 7, 40, 11, 600))])
    return [(synth_ids(rng, 64, row_off), rng.integers(0, 2, 64).astype(np.float32)) for _ in range(n)]


def _input_fn(batches):
    def fn():
        for ids, y in batches:
            yield {"ids": ids}, y
    return fn


def _snapshot(est):
    torch.cuda.synchronize()
    a = est.store.embeddings["input_layer"]
    return {"tables": a.tables.clone(), "lin_t": a.m_t.clone(), "acc_t": a.v_t.clone(), "w1": a.w1.clone(),
            "lin_w": a.m_w.clone(), "acc_w": a.v_w.clone(), "dense": est.store.dense.flat.clone(),
            "dense_m": est.store.dense.m.clone(), "dense_v": est.store.dense.v.clone(), "step": est.store.opt.state[3:4].clone()}


@pytest.mark.parametrize("opt_name,hp", [("adagrad", {}), ("ftrl", FTRL_REG),
                                         ("ftrl", dict(FTRL_REG, l2_shrinkage_regularization_strength=0.05))])
def test_hip_graph_training_equals_eager(opt_name, hp):
    batches = _batches(8)
    res = []
    for graph in (True, False):
        est = _deepfm_est(opt_name, hp, graph)
        est.train(_input_fn(batches), steps=8)
        assert est.global_step == 8
        if graph:
            assert est._graphs, "no HIP graph was captured"
        res.append(_snapshot(est))
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), (k, float((res[0][k].float() - res[1][k].float()).abs().max()))


def test_replayed_launch_advances_the_dropout_seed():
    """The fused tower's dropout masks are a hash of the step word that rsx_sparse_opt_multi advances.  With a learning rate
    far below fp32 resolution (Adagrad: var - lr*g/sqrt(acc) == var) the same batch trained at two consecutive replayed
    steps sees the same parameters -- so different losses can only come from different masks."""
    ids, y = _batches(1, seed=2)[0]
    est = _deepfm_est("adagrad", {}, True, dropout=0.5, lr=1e-38)
    f, lab = {"ids": torch.from_numpy(ids).cuda()}, torch.from_numpy(y).cuda()
    losses, steps = [], []
    for _ in range(5):                                   # 2 eager warm-up steps, then capture + replays
        losses.append(float(est._train_step(f, lab)))
        steps.append(est.global_step)
    assert next(iter(est._graphs.values())).graph is not None
    assert steps == [1, 2, 3, 4, 5]
    w = est.store.embeddings["input_layer"].tables.clone()
    losses.append(float(est._train_step(f, lab)))
    torch.cuda.synchronize()
    assert torch.equal(w, est.store.embeddings["input_layer"].tables)       # the tables did not move
    assert losses[4] != losses[5] and losses[3] != losses[4], losses


def test_checkpoint_resume_equals_uninterrupted_and_refuses_another_optimizer(tmp_path):
    from recsys_amd import _lib
    hp = dict(FTRL_REG)
    batches = _batches(8, seed=5)
    full = _deepfm_est("ftrl", hp, True)
    full.train(_input_fn(batches), steps=8)
    d = str(tmp_path / "m")
    first = _deepfm_est("ftrl", hp, True, model_dir=d, save_steps=4)
    first.train(_input_fn(batches[:4]), steps=4)
    assert glob.glob(os.path.join(d, "model.ckpt-4.pt"))
    second = _deepfm_est("ftrl", hp, True, model_dir=d, save_steps=4)
    second.train(_input_fn(batches[4:]), steps=4)
    assert second.global_step == 8
    a, b = _snapshot(full), _snapshot(second)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for other in ("adam", "adagrad"):
        est = _deepfm_est(other, {} if other == "adam" else None, True, model_dir=d)
        with pytest.raises(_lib.RsxError, match="optimizer"):
            est.train(_input_fn(batches[:1]), steps=1)


def _make_shards(d):
    from tests.test_gpu_end_to_end import _make_shards as mk
    mk(d)


@pytest.mark.parametrize("mod,opt", [("deepfm", "ftrl"), ("fm", "ftrl"), ("deepfm", "adagrad")])
def test_script_main_train_eval_predict_resume(tmp_path, mod, opt, capsys):
    import importlib
    m = importlib.import_module("recsys_amd." + mod)
    d = str(tmp_path) + "/"
    _make_shards(d)
    model_dir = str(tmp_path / "model")
    common = ["--train_path", d, "--train_parts", "4", "--eval_parts", "1", "--batch_size", "256", "--model_dir", model_dir,
              "--save_checkpoints_steps", "8", "--log_steps", "4", "--dropout", "0.1", "--optimizer", opt]
    # (per-coordinate step sizes lr / sqrt(accumulator): TF's usual FTRL / Adagrad learning rates are 10x Adam's)
    common += ["--learning_rate", "0.1"] + (["--l1_regularization_strength", "0.001"] if opt == "ftrl" else [])
    res = m.main(common + ["--task_type", "train", "--num_epochs", "10"])
    assert "INFO:--optimizer %s: one replica" % opt in capsys.readouterr().out
    assert res is not None and np.isfinite(res["loss"])
    assert res["AUC"] > (0.6 if mod == "fm" else 0.75), res                  # it learns the planted signal
    step_after_train = res["global_step"]
    ev = m.main(common + ["--task_type", "eval"])
    assert ev["global_step"] == step_after_train
    assert abs(ev["AUC"] - res["AUC"]) < 1e-6 and abs(ev["loss"] - res["loss"]) < 1e-6
    preds = m.main(common + ["--task_type", "infer"])
    assert len(preds) == 10 and all(0.0 <= float(p["prob"]) <= 1.0 for p in preds)
    res2 = m.main(common + ["--task_type", "train", "--num_epochs", "1"])
    assert res2["global_step"] > step_after_train
    from recsys_amd import _lib
    adam = [x for x in common if x not in ("--optimizer", opt)]
    with pytest.raises(_lib.RsxError, match="optimizer"):
        m.main(adam + ["--task_type", "eval"])


def test_refusals_under_ftrl(tmp_path):
    import types
    from recsys_amd import _lib, din, deepfm
    from recsys_amd.estimator import Estimator, ModeKeys, RunConfig, VariableStore
    # DIN: its SparseTable views have no row-segment optimizer form
    store = VariableStore("cuda", 0, "tf1_dense", optimizer="ftrl")
    with pytest.raises(_lib.RsxError, match="din"):
        din.build_variables(store, {"embedding_size": 8}, 4, 5)
    # a data-parallel store
    est = _deepfm_est("ftrl", FTRL_REG, False)
    est.store.dp = types.SimpleNamespace(world=1, rank=0)
    ids, y = _batches(1)[0]
    with pytest.raises(_lib.RsxError, match="data-parallel"):
        est._call_model_fn({"ids": torch.from_numpy(ids).cuda()}, None, ModeKeys.PREDICT)
    # an optimizer window
    F = deepfm.define_flags().parse_args(["--optimizer", "ftrl", "--adam_window", "4"])
    with pytest.raises(_lib.RsxError, match="adam_window"):
        Estimator(deepfm.model_fn, None, deepfm.make_params(F), RunConfig(optimizer="ftrl"))
    with pytest.raises(_lib.RsxError, match="adam_window"):
        deepfm.main(["--optimizer", "ftrl", "--adam_window", "4", "--model_dir", str(tmp_path), "--task_type", "eval"])
