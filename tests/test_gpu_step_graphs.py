"""The Estimator's step graphs -- the records of Estimator._graphs (StepGraph, WindowSets / StagedWindow, ResidentPlan) and the
one capture path behind them: every way into a TRAIN step gives the same bits, a resident plan belongs to exactly one list of
batches, prepare_resident leaves nothing to capture, and a captured forward equals the eager one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N_BATCHES = 64, 8


def _est(graph=True, **params):
    from recsys_amd import deepfm
    from recsys_amd.estimator import Estimator, RunConfig
    from recsys_amd.feature_columns import build_feature_columns
    lin, emb = build_feature_columns(16, "indicator_all")
    p = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": 16, "learning_rate": 1e-3,
         "dropout": 0.5, "deep_layers": "100,100", "max_batch_size": B}
    p.update(params)
    return Estimator(deepfm.model_fn, None, p, RunConfig(use_hip_graph=graph, adam_mode="tf1_dense", device="cuda", seed=13,
                                                          log_step_count_steps=10 ** 9))


@pytest.fixture(scope="module")
def host():
    """8 batches of 64 on the host: (ids, labels, log-values); never written to."""
    from recsys_amd import synthetic
    from recsys_amd.feature_columns import CriteoLayout, build_feature_columns
    layout = CriteoLayout.from_columns(build_feature_columns(16, "indicator_all")[1])
    return synthetic.criteo_id_batches(layout, N_BATCHES, B, seed=2024)


def _resident(est, host):
    """The batches in HBM, and the variables of `est` created (by the first model_fn call)."""
    from recsys_amd.estimator import PackedBatch
    feats = [PackedBatch({"ids": i}, y, device="cuda") for i, y, _ in host]
    with torch.no_grad():
        est._call_model_fn(feats[0].views()[0], None, "infer")
    return feats


def _state(est):
    a = est.store.embeddings["input_layer"]
    torch.cuda.synchronize()
    return {"tables": a.tables.clone(), "m": a.m_t.clone(), "v": a.v_t.clone(), "w1": a.w1.clone(), "m_w": a.m_w.clone(),
            "v_w": a.v_w.clone(), "dense": est.store.dense.flat.clone(), "dense_m": est.store.dense.m.clone(),
            "dense_v": est.store.dense.v.clone(), "opt": est.store.opt.state[:4].clone()}


def _assert_same_state(a, b, what):
    for name in a:
        assert torch.isfinite(a[name].float()).all(), (what, name)
        assert torch.equal(a[name], b[name]), (what, name, float((a[name].float() - b[name].float()).abs().max()))


def _plans(est):
    return [g for k, g in est._graphs.items() if k[0] == "resident"]


def test_a_second_list_with_the_same_first_batch_gets_its_own_graphs(host):
    """The resident graphs read their batches in place, so they belong to ONE list: a reordered list (same length, same first
    batch) is captured on its own, and the first plan keeps its batches alive."""
    a = _est()
    feats = _resident(a, host)
    perm = [feats[i] for i in (0, 3, 2, 1, 4, 7, 6, 5)]
    a.train_resident(feats, 10, 4)
    a.train_resident(perm, 8, 4)
    b = _est(graph=False)
    feats_b = _resident(b, host)
    for i in [s % N_BATCHES for s in range(10)] + [0, 3, 2, 1, 4, 7, 6, 5]:
        b._train_step(feats_b[i])
    assert a.global_step == b.global_step == 18
    _assert_same_state(_state(a), _state(b), "two lists")
    plans = _plans(a)
    assert len(plans) == 2
    assert len(plans[0].batches) == N_BATCHES and all(x is y for x, y in zip(plans[0].batches, feats))
    assert all(x is y for x, y in zip(plans[1].batches, perm))


@pytest.mark.parametrize("steps,spg", [(8, 4), (10, 4), (5, 4)])
def test_prepare_resident_leaves_nothing_to_capture(host, steps, spg):
    est = _est()
    feats = _resident(est, host)
    est.prepare_resident(feats, steps, spg)
    (plan,) = _plans(est)
    captured = dict(plan.graphs)
    assert captured and plan.warm == 0
    if (steps, spg) == (5, 4):         # one full group + a tail shorter than half a group: ONE graph of 5 steps
        assert list(captured) == [(0, 5)]
    est.train_resident(feats, steps, spg)
    assert _plans(est) == [plan] and list(plan.graphs) == list(captured)
    assert all(plan.graphs[k][0] is g for k, (g, _) in captured.items())
    assert est.global_step == 2 + steps          # (prepare_resident's two eager warm-up steps are real steps)


def test_every_entry_path_gives_the_same_bits(host):
    """12 steps over the 8 batches in order, through every way into a TRAIN step."""
    order = [s % N_BATCHES for s in range(12)]

    def input_fn():
        for s in order:
            yield {"ids": host[s][0]}, host[s][1]

    def dict_steps(est, feats):
        for s in order:
            est._train_step(*feats[s].views())

    def packed_steps(est, feats):
        for s in order:
            est._train_step(feats[s])

    # (adam_window 2: six windows of two steps -- one eager, one captured per instance, the rest staged and replayed)
    paths = [("dict", _est(), dict_steps), ("packed", _est(), packed_steps),
             ("resident", _est(), lambda est, feats: est.train_resident(feats, 12, 4)),
             ("train", _est(adam_window=2), lambda est, feats: est.train(input_fn, steps=12)),
             ("train, no graphs", _est(graph=False), lambda est, feats: est.train(input_fn, steps=12))]
    states = {}
    for name, est, run in paths:
        run(est, _resident(est, host))
        assert est.global_step == 12, name
        states[name] = _state(est)
        kinds = sorted({k[0] if isinstance(k[0], str) else "dict" for k in est._graphs})
        if name == "dict":
            (g,) = est._graphs.values()
            assert g.graph is not None and g.warm == 0
        elif name == "packed":
            assert kinds == ["packed"] and est._graphs[next(iter(est._graphs))].graph is not None
        elif name == "resident":
            assert kinds == ["resident"]
        elif name == "train":
            assert kinds == ["packedwin"]
            (g,) = est._graphs.values()
            assert len(g.sets) == est._window_sets and all(st.graph is not None for st in g.sets)
        else:
            assert not est._graphs
    for name in states:
        _assert_same_state(states["dict"], states[name], name)


def test_infer_step_through_its_graph_equals_the_eager_forward(host):
    from recsys_amd.estimator import ModeKeys
    graph, eager = _est(), _est(graph=False)
    with torch.no_grad():
        for n, b in enumerate((0, 0, 5)):            # eager warm-up, capture + replay, replay with another batch
            ids, y, _ = host[b]
            got = graph._infer_step({"ids": ids}, y, ModeKeys.EVAL)
            want = eager._infer_step({"ids": ids}, y, ModeKeys.EVAL)
            (g,) = graph._graphs.values()
            assert (g.graph is not None) == (n > 0)
            for name, x, w in zip(("prob", "loss", "labels"), got, want):
                assert torch.equal(x, w), (n, name)
            assert torch.equal(graph._infer_features["ids"], eager._infer_features["ids"])
        assert not eager._graphs and graph._n_infer_graphs == 1
        # one record per signature up to MAX_INFER_GRAPHS; the signature after that stays eager and is not remembered
        ids = host[1][0]
        for b in range(1, graph.MAX_INFER_GRAPHS):
            graph._infer_step({"ids": ids[:b]}, None, ModeKeys.PREDICT)
        assert graph._n_infer_graphs == len(graph._graphs) == graph.MAX_INFER_GRAPHS
        b = graph.MAX_INFER_GRAPHS
        for _ in range(3):
            got = graph._infer_step({"ids": ids[:b]}, None, ModeKeys.PREDICT)
            want = eager._infer_step({"ids": ids[:b]}, None, ModeKeys.PREDICT)
            assert torch.equal(got[0], want[0]) and got[1] is None and got[2] is None
        assert graph._n_infer_graphs == len(graph._graphs) == graph.MAX_INFER_GRAPHS
        assert np.isfinite(got[0].cpu().numpy()).all()
