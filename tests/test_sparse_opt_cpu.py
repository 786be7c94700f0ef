"""FTRL / Adagrad (tf.train.FtrlOptimizer / AdagradOptimizer) without a GPU: the numpy restatement against TF 1.x's
published known answers (ftrl_test.py / adagrad_test.py), the zero-gradient fixed point the dense-form route relies on,
the flags and defaults, and the C ABI's refusals (made before any HIP call)."""
import ctypes as C

import numpy as np
import pytest

from tests.opt_ref import SparseOptRef

EINVAL = -1
P = C.c_void_p(0x1000)          # "some non-NULL pointer" -- never read


def _two_vars(opt, v0, v1, g0, g1, steps):
    var0, var1 = np.array(v0, np.float32), np.array(v1, np.float32)
    for _ in range(steps):
        opt.apply_dense("var0", var0, np.array(g0, np.float32))
        opt.apply_dense("var1", var1, np.array(g1, np.float32))
        opt.finish_step()
    return var0, var1


FTRL_KNOWN = [
    # (start var0, start var1, steps, hyper-parameters, expected var0, expected var1)
    ([0, 0], [0, 0], 3, {}, [-2.60260963, -4.29698515], [-0.28432083, -0.56694895]),
    ([1, 2], [4, 3], 3, {}, [-2.55607247, -3.98729396], [-0.28232238, -0.56096673]),
    ([1, 2], [4, 3], 10, {"l1_regularization_strength": 0.001}, [-7.66718769, -10.91273689], [-0.93460727, -1.86147261]),
    ([1, 2], [4, 3], 10, {"l1_regularization_strength": 0.001, "l2_regularization_strength": 2.0},
     [-0.24059935, -0.46829352], [-0.02406147, -0.04830509]),
    ([1, 2], [4, 3], 10, {"l1_regularization_strength": 0.001, "l2_regularization_strength": 2.0,
                          "l2_shrinkage_regularization_strength": 0.1},
     [-0.22578995, -0.44345796], [-0.14378493, -0.13229476]),
]


@pytest.mark.parametrize("v0,v1,steps,hp,want0,want1", FTRL_KNOWN)
def test_ftrl_restatement_matches_tf_known_answers(v0, v1, steps, hp, want0, want1):
    opt = SparseOptRef("ftrl", 3.0, initial_accumulator_value=0.1, **hp)
    var0, var1 = _two_vars(opt, v0, v1, [0.1, 0.2], [0.01, 0.02], steps)
    np.testing.assert_allclose(var0, want0, rtol=0, atol=1e-6)
    np.testing.assert_allclose(var1, want1, rtol=0, atol=1e-6)


def test_adagrad_restatement_matches_tf_known_answer():
    opt = SparseOptRef("adagrad", 3.0, initial_accumulator_value=0.1)
    var0, var1 = _two_vars(opt, [1, 2], [3, 4], [0.1, 0.1], [0.01, 0.01], 3)
    np.testing.assert_allclose(var0, [-1.60260987, -0.60260987], rtol=0, atol=1e-6)
    np.testing.assert_allclose(var1, [2.71567917, 3.71567917], rtol=0, atol=1e-6)


@pytest.mark.parametrize("name,hp,fixed", [
    ("adagrad", {}, True),
    ("ftrl", {}, True),
    ("ftrl", {"l1_regularization_strength": 0.05, "l2_regularization_strength": 0.3}, True),
    ("ftrl", {"learning_rate_power": -0.3, "l1_regularization_strength": 0.01}, True),
    ("ftrl", {"l2_shrinkage_regularization_strength": 0.1}, False),
])
def test_zero_gradient_dense_update_is_a_fixed_point_after_one_dense_step(name, hp, fixed):
    """The route the first-order vector takes (include/rsx.h RSX_ADAM_VEC_SLOT): once an element has had one dense update,
    a zero-gradient update leaves it bit for bit as it is -- except under FTRL's l2 shrinkage."""
    rng = np.random.default_rng(3)
    opt = SparseOptRef(name, 0.05, **hp)
    var = rng.standard_normal(4096).astype(np.float32)
    opt.apply_dense("w", var, (rng.standard_normal(4096) * 0.1).astype(np.float32))
    opt.apply_dense("w", var, np.where(rng.random(4096) < 0.5, rng.standard_normal(4096) * 0.1, 0).astype(np.float32))
    lin, acc = (x.copy() for x in opt.slots["w"])
    before = var.copy()
    opt.apply_dense("w", var, np.zeros(4096, np.float32))
    same = np.array_equal(before.view(np.uint32), var.view(np.uint32)) and \
        np.array_equal(lin.view(np.uint32), opt.slots["w"][0].view(np.uint32)) and \
        np.array_equal(acc.view(np.uint32), opt.slots["w"][1].view(np.uint32))
    assert same == fixed


def test_ftrl_dense_first_step_zeroes_untouched_weights():
    """TF's dense FTRL form with g = 0 and linear = 0 sets var to 0: the initial value of an untouched element is gone."""
    opt = SparseOptRef("ftrl", 0.05)
    var = np.array([0.3, -0.2, 0.1, 0.7], np.float32)
    opt.apply_dense("w", var, np.array([0.0, 0.5, 0.0, 0.0], np.float32))
    assert var[0] == 0 and var[2] == 0 and var[3] == 0 and var[1] != 0


@pytest.mark.parametrize("mod", ["deepfm", "fm", "dcn", "xdeepfm"])
def test_optimizer_flags_and_defaults(mod):
    import importlib
    m = importlib.import_module("recsys_amd." + mod)
    F = m.define_flags().parse_args([])
    assert F.optimizer == "adam"
    assert F.initial_accumulator_value == 0.1 and F.learning_rate_power == -0.5
    assert F.l1_regularization_strength == 0.0 and F.l2_regularization_strength == 0.0
    assert F.l2_shrinkage_regularization_strength == 0.0
    F = m.define_flags().parse_args(["--optimizer", "ftrl", "--l1_regularization_strength", "0.001",
                                     "--l2_shrinkage_regularization_strength", "0.2"])
    from recsys_amd.deepfm import optimizer_config
    name, hp = optimizer_config(F)
    assert name == "ftrl" and hp["l1_regularization_strength"] == 0.001 and hp["l2_shrinkage_regularization_strength"] == 0.2
    assert optimizer_config(m.define_flags().parse_args(["--optimizer", "adagrad"])) == \
        ("adagrad", {"initial_accumulator_value": 0.1})
    with pytest.raises(SystemExit):
        m.define_flags().parse_args(["--optimizer", "sgd"])


def test_run_config_defaults_to_adam():
    from recsys_amd.estimator import RunConfig
    assert RunConfig().optimizer == "adam" and RunConfig().optimizer_hparams is None


@pytest.mark.parametrize("cls,kw", [
    ("FtrlTF1", {"lr": 0.0}), ("FtrlTF1", {"lr": -1.0}), ("FtrlTF1", {"learning_rate_power": 0.5}),
    ("FtrlTF1", {"initial_accumulator_value": -0.1}), ("FtrlTF1", {"l1_regularization_strength": -1e-3}),
    ("FtrlTF1", {"l2_regularization_strength": -1.0}), ("FtrlTF1", {"l2_shrinkage_regularization_strength": -0.1}),
    ("AdagradTF1", {"lr": 0.0}), ("AdagradTF1", {"initial_accumulator_value": 0.0}),
])
def test_optimizer_classes_reject_bad_hyperparameters_before_touching_the_gpu(cls, kw):
    from recsys_amd import ops
    with pytest.raises(ValueError):
        getattr(ops, cls)(**kw)


def test_variable_store_rejects_unknown_optimizer():
    from recsys_amd.estimator import VariableStore
    with pytest.raises(ValueError):
        VariableStore("cpu", 0, "tf1_dense", optimizer="sgd")


@pytest.fixture(scope="module")
def L():
    from recsys_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _seg(kind, **kw):
    from recsys_amd import _lib
    s = _lib.AdamSeg()
    s.kind, s.d, s.n = kind, kw.get("d", 16), kw.get("n", 64)
    for f in ("var", "m", "v", "g", "slot", "uniq_row", "nuniq"):
        setattr(s, f, kw.get(f, 0x1000))
    s.B, s.stride, s.zero_grad = kw.get("B", 4), kw.get("stride", 4), 0
    return s


def _call(L, segs, hp, nseg=None, state=P):
    from recsys_amd import _lib
    arr = (_lib.AdamSeg * max(1, len(segs)))(*segs)
    return L.rsx_sparse_opt_multi(arr, len(segs) if nseg is None else nseg, state, C.byref(hp) if hp is not None else None, None)


def test_sparse_opt_c_abi_refusals(L):
    from recsys_amd import _lib
    ftrl = lambda **kw: _lib.SparseOptHp(_lib.RSX_OPT_FTRL, kw.get("lr", 0.1), kw.get("p", -0.5), kw.get("l1", 0.0),
                                         kw.get("l2", 0.0), kw.get("l2s", 0.0))
    dense = _seg(_lib.RSX_ADAM_DENSE)
    # bad hyper-parameters
    for hp in (ftrl(lr=0.0), ftrl(lr=-1.0), ftrl(lr=float("nan")), ftrl(p=0.5), ftrl(l1=-1e-3), ftrl(l2=-1.0), ftrl(l2s=-0.1),
               _lib.SparseOptHp(_lib.RSX_OPT_ADAGRAD, 0.0, -0.5, 0, 0, 0), _lib.SparseOptHp(7, 0.1, -0.5, 0, 0, 0),
               _lib.SparseOptHp(0, 0.1, -0.5, 0, 0, 0)):
        assert _call(L, [dense], hp) == EINVAL
    hp = ftrl()
    # nseg outside 1..RSX_ADAM_MAX_SEGS, missing state / hyper-parameters / segments
    assert _call(L, [dense], hp, nseg=0) == EINVAL
    assert _call(L, [dense] * (_lib.RSX_ADAM_MAX_SEGS + 1), hp) == EINVAL
    assert _call(L, [dense], hp, state=None) == EINVAL
    assert _call(L, [dense], None) == EINVAL
    assert L.rsx_sparse_opt_multi(None, 1, P, C.byref(hp), None) == EINVAL
    # unknown or Adam-only segment kinds
    for kind in (_lib.RSX_ADAM_TABLE_TF1, _lib.RSX_ADAM_VEC_ROWS, _lib.RSX_ADAM_TABLE_TF1_COLD, _lib.RSX_ADAM_VEC_COLD,
                 _lib.RSX_ADAM_VEC_ROWS_DENSE, 99, -1):
        assert _call(L, [_seg(kind)], hp) == EINVAL
    # missing pointers
    for f in ("var", "m", "v", "g"):
        assert _call(L, [_seg(_lib.RSX_ADAM_DENSE, **{f: 0})], hp) == EINVAL
    for f in ("uniq_row", "nuniq"):
        assert _call(L, [_seg(_lib.RSX_ADAM_TABLE_ROWS, **{f: 0})], hp) == EINVAL
    assert _call(L, [_seg(_lib.RSX_ADAM_VEC_SLOT, slot=0)], hp) == EINVAL
    # row width, batch shape, replicas, windows
    assert _call(L, [_seg(_lib.RSX_ADAM_TABLE_ROWS, d=6)], hp) == EINVAL
    assert _call(L, [_seg(_lib.RSX_ADAM_TABLE_ROWS, B=0)], hp) == EINVAL
    assert _call(L, [_seg(_lib.RSX_ADAM_TABLE_ROWS, B=8, stride=4)], hp) == EINVAL
    s = _seg(_lib.RSX_ADAM_TABLE_ROWS)
    s.g_replicas = 2
    assert _call(L, [s], hp) == EINVAL
    s = _seg(_lib.RSX_ADAM_DENSE)
    s.B = 2
    assert _call(L, [s], hp) == EINVAL
    s = _seg(_lib.RSX_ADAM_VEC_SLOT)
    s.slot_w[0] = 0x2000
    assert _call(L, [s], hp) == EINVAL
    # one bad segment among good ones is enough
    assert _call(L, [dense, _seg(_lib.RSX_ADAM_TABLE_TF1)], hp) == EINVAL
