"""fp32 numpy restatement of tf.train.FtrlOptimizer / AdagradOptimizer (TF 1.x training_ops, include/rsx.h
rsx_sparse_opt_multi), with the apply_dense / apply_sparse / finish_step interface of oracle.nn.AdamTF1 so that it plugs
into oracle.models.train_step.  Also the model-level parity runner of the sparse optimizers."""
import numpy as np

from oracle import criteo, init, models, nn
from tests.parity_util import load_oracle_weights, small_columns, synth_ids


class SparseOptRef:
    """name in {'adagrad', 'ftrl'}; hp: TF argument names (initial_accumulator_value, learning_rate_power,
    l1_/l2_/l2_shrinkage_regularization_strength)."""

    def __init__(self, name, lr, dtype=np.float32, **hp):
        self.name = name
        self.t = np.dtype(dtype).type
        t = self.t
        self.lr = t(lr)
        self.acc0 = t(hp.get("initial_accumulator_value", 0.1))
        self.p = float(hp.get("learning_rate_power", -0.5))
        self.l1 = t(hp.get("l1_regularization_strength", 0.0))
        self.l2 = t(hp.get("l2_regularization_strength", 0.0))
        self.l2s = t(hp.get("l2_shrinkage_regularization_strength", 0.0))
        self.slots = {}

    def _slot(self, name, var):
        if name not in self.slots:
            self.slots[name] = (np.zeros_like(var), np.full_like(var, self.acc0))    # (linear, accumulator)
        return self.slots[name]

    def _pow(self, x):
        return np.sqrt(x) if self.p == -0.5 else np.power(x, self.t(-self.p))

    def update(self, var, lin, acc, g):
        """One update of the arrays (same shapes) in TF's order of operations; returns the new (var, lin, acc)."""
        t = self.t
        if self.name == "adagrad":
            acc = acc + g * g
            return var - (self.lr * g) / np.sqrt(acc), lin, acc
        gs = g + (t(2) * self.l2s) * var if self.l2s > 0 else g
        na = acc + g * g
        pn = self._pow(na)
        lin = lin + (gs - (pn - self._pow(acc)) / self.lr * var)
        y = pn / self.lr + t(2) * self.l2
        with np.errstate(divide="ignore", invalid="ignore"):
            var = np.where(np.abs(lin) > self.l1, (np.where(lin > 0, self.l1, -self.l1) - lin) / y, t(0)).astype(var.dtype)
        return var, lin, na

    def apply_dense(self, name, var, g):
        lin, acc = self._slot(name, var)
        v, l, a = self.update(var, lin, acc, g.astype(var.dtype))
        var[...], lin[...], acc[...] = v, l, a

    def apply_sparse(self, name, var, rows, G, lazy=False):
        """SparseApplyFtrl / SparseApplyAdagrad: only the unique `rows` move, with their summed gradient G."""
        lin, acc = self._slot(name, var)
        rows = np.asarray(rows)
        v, l, a = self.update(var[rows], lin[rows], acc[rows], G.astype(var.dtype))
        var[rows], lin[rows], acc[rows] = v, l, a

    def finish_step(self):
        pass


def _run_config_kw(name, hp):
    return dict(optimizer=name, optimizer_hparams=dict(hp))


def model_parity_run(kind, opt_name, hp, B=64, steps=4, seed=0, rows=(3, 7, 40, 11, 600), D=16, layers=(32, 16),
                     dropout=0.0, tower="hip", use_graph=False, cin=(16, 16), lr=1e-3):
    """`steps` TRAIN steps of `kind` in {fm, deepfm, dcn, xdeepfm} under optimizer `opt_name` on the GPU and through
    oracle.models.train_step driven by SparseOptRef, from the same weights and batches (injected dropout masks).
    -> (max |prob| error over the steps, [(loss_gpu, loss_oracle)], {parameter: max abs error})."""
    import torch
    from recsys_amd import dcn, deepfm, fm, xdeepfm
    from recsys_amd.estimator import Estimator, ModeKeys, RunConfig
    from recsys_amd.feature_columns import build_feature_columns
    rng = np.random.default_rng(seed)
    if rows is None:
        lin, emb = build_feature_columns(D)
        row_off = criteo.row_offsets()
    else:
        lin, emb = small_columns(rows, D)
        row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    params = {"linear_feature_columns": lin, "embedding_feature_columns": emb, "embedding_size": D, "learning_rate": lr,
              "dropout": dropout, "deep_layers": ",".join(map(str, layers)), "max_batch_size": B, "tower": tower,
              "cross_layers": 3}
    if kind == "xdeepfm":
        return _xdeepfm_parity(params, opt_name, hp, B, steps, seed, rng, layers, dropout, use_graph, lr, cin)
    if kind == "dcn":
        P = init.dcn_params(seed, D, layers, 3, np.float32, row_off)
        mfn = dcn.model_fn
    elif kind == "fm":
        P = init.deepfm_params(seed, D, (), np.float32, row_off, with_dnn=False)
        mfn, layers = fm.model_fn, ()
        params["deep_layers"] = ""
    else:
        P = init.deepfm_params(seed, D, layers, np.float32, row_off)
        mfn = deepfm.model_fn
    if "b1" in P:
        P["b1"] += np.float32(0.05)
    est = Estimator(mfn, None, params, RunConfig(use_hip_graph=use_graph, **_run_config_kw(opt_name, hp)))
    batches = [(synth_ids(rng, B, row_off), rng.integers(0, 2, B).astype(np.float32)) for _ in range(steps)]
    est._call_model_fn({"ids": torch.from_numpy(batches[0][0]).cuda()}, None, ModeKeys.PREDICT)
    load_oracle_weights(est, P)
    om = {"dcn": lambda: models.DCN(P, row_off, len(layers), dropout), "fm": lambda: models.FM(P, row_off),
          "deepfm": lambda: models.DeepFM(P, row_off, len(layers), dropout)}[kind]()
    opt = SparseOptRef(opt_name, lr, **hp)
    err, losses = 0.0, []
    for ids, y in batches:
        f = {"ids": torch.from_numpy(ids).cuda()}
        with torch.no_grad():
            zg = est._call_model_fn(f, None, ModeKeys.PREDICT).predictions["prob"]
        mk = None
        if dropout > 0.0 and len(layers):
            mk = [(rng.random((B, n)) >= dropout).astype(np.float32) for n in layers]
            est.params["_dropout_masks"] = [torch.from_numpy(m).cuda() for m in mk]
        loss_g = est._train_step(f, torch.from_numpy(y).cuda())
        zo = nn.sigmoid(om.forward(ids, train=False))
        loss_o, _ = models.train_step(om, opt, (ids,), y, {"masks": mk} if mk else None)
        err = max(err, float(np.abs(zg.cpu().numpy().reshape(-1) - zo).max()))
        losses.append((float(loss_g), float(loss_o)))
    st = est.store
    a = st.embeddings["input_layer"]
    perr = {"tables": float(np.abs(a.tables.cpu().numpy() - P["tables"]).max())}
    if a.with_w1:
        perr["w1"] = float(np.abs(a.w1.cpu().numpy() - P["w1"]).max())
    for k, p in st.dense.params.items():
        perr[k] = float(np.abs(p.detach().cpu().numpy() - P[k].reshape(p.shape)).max())
    return err, losses, perr


def _xdeepfm_parity(params, opt_name, hp, B, steps, seed, rng, layers, dropout, use_graph, lr, cin):
    """tests/test_gpu_xdeepfm.py's runner under a sparse optimizer: Criteo-39, fp64 oracle (the CIN contraction's fp32
    summation orders differ by a few 1e-5 on the logits)."""
    import torch
    from recsys_amd import xdeepfm
    from recsys_amd.estimator import Estimator, ModeKeys, RunConfig
    from recsys_amd.feature_columns import build_feature_columns
    D = params["embedding_size"]
    lin, emb = build_feature_columns(D, "numeric+indicator")
    row_off = criteo.row_offsets()
    cat_slot, cat_off = init.xdeepfm_layout()
    P = init.xdeepfm_params(seed, D, layers, cin, np.float32, row_off)
    for k in ("lin.b", "cin.bout", "dnn.bout"):
        P[k] += np.float32(0.05)
    params = dict(params, linear_feature_columns=lin, embedding_feature_columns=emb,
                  cross_layers=",".join(map(str, cin)))
    est = Estimator(xdeepfm.model_fn, None, params, RunConfig(use_hip_graph=use_graph, **_run_config_kw(opt_name, hp)))
    batches = []
    for _ in range(steps):
        ids = synth_ids(rng, B, row_off)
        logx = np.log(np.floor(np.exp(rng.normal(2, 1, (B, 13)))) + 1.0).astype(np.float32)
        batches.append((ids, logx, rng.integers(0, 2, B).astype(np.float32)))

    def feats(ids, logx):
        return {"ids": torch.from_numpy(ids).cuda(), "cont_log": torch.from_numpy(logx).cuda()}

    est._call_model_fn(feats(*batches[0][:2]), None, ModeKeys.PREDICT)
    st = est.store
    w1 = np.zeros(int(row_off[-1]), np.float32)                     # oracle lin.wcat -> arena w1 (slot-order rows)
    for j in range(26):
        s = int(cat_slot[j])
        w1[row_off[s]:row_off[s + 1]] = P["lin.wcat"][cat_off[j]:cat_off[j + 1]]
    with torch.no_grad():
        st.embeddings["input_layer"].tables.copy_(torch.from_numpy(P["tables"]))
        st.embeddings["input_layer"].w1.copy_(torch.from_numpy(w1))
        st.embeddings["input_layer_1"].tables.copy_(torch.from_numpy(P["tables2"]))
    st.dense.load({k: v for k, v in P.items() if k in st.dense.params})
    P = {k: v.astype(np.float64) for k, v in P.items()}
    om = models.XDeepFM(P, row_off, cat_slot, cat_off, cin, len(layers), dropout)
    opt = SparseOptRef(opt_name, lr, dtype=np.float64, **hp)
    err, losses = 0.0, []
    for ids, logx, y in batches:
        mk = None
        if dropout > 0:
            mk = [(rng.random((B, n)) >= dropout).astype(np.float32) for n in layers]
            est.params["_dropout_masks"] = [torch.from_numpy(m).cuda() for m in mk]
        f = feats(ids, logx)
        with torch.no_grad():
            pg = est._call_model_fn(f, None, ModeKeys.PREDICT).predictions["prob"].cpu().numpy().reshape(-1)
        po = nn.sigmoid(om.forward(ids, logx.astype(np.float64), train=False))
        err = max(err, float(np.abs(pg - po).max()))
        lg = float(est._train_step(f, torch.from_numpy(y).cuda()))
        lo, _ = models.train_step(om, opt, (ids, logx.astype(np.float64)), y.astype(np.float64),
                                  {"masks": [m.astype(np.float64) for m in mk]} if mk else None)
        losses.append((lg, float(lo)))
    a1 = st.embeddings["input_layer"]
    w1g = a1.w1.cpu().numpy()
    wcat = np.concatenate([w1g[row_off[int(cat_slot[j])]:row_off[int(cat_slot[j]) + 1]] for j in range(26)])
    perr = {"tables": float(np.abs(a1.tables.cpu().numpy() - P["tables"]).max()),
            "tables2": float(np.abs(st.embeddings["input_layer_1"].tables.cpu().numpy() - P["tables2"]).max()),
            "lin.wcat": float(np.abs(wcat - P["lin.wcat"]).max())}
    for k, p in st.dense.params.items():
        perr[k] = float(np.abs(p.detach().cpu().numpy() - P[k].reshape(p.shape)).max())
    return err, losses, perr
