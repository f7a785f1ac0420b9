"""SGU2 (the LSTM signal gate unit) on the GPU: inference
and training, API-compatible with models/GateUnits.py:42-136 and
utils/scaler.py.

``SGU2Model`` is the weight container and checkpoint format (state_dict keys
lstm.* / fc.* as GateUnits.py:42-47); ``SGU2.predict`` runs libsgmm.so's
sgmm_sgu2_forward over all windows in one launch.  ``predict_device`` takes
the windows already on the device (sgmm_bar_windows' output) and applies the
StandardScaler3D fit in the kernel, so the bundle builder never moves the
windows to the host.

``SGU2.train`` (GateUnits.py:66-114) runs a whole fit -- every epoch and
minibatch, Adam, the validation pass, early stopping and the history -- as one
launch of sgmm_sgu2_train, one workgroup per fit; ``train_device`` takes
windows and labels already on the device with the scaler and the label scale
fused; ``train_sgu2_many`` runs K fits (seeds, learning rates, hidden sizes,
datasets) in one launch per hidden size.  The shuffle and the dropout masks
come from the device Philox stream of ``seed`` (include/sgmm.h documents the
counter layout) or from an explicit ``schedule``; torch's own shuffle and
dropout streams are not reproduced.  The reference's ``best_state`` aliases
the live parameters, so its final ``load_state_dict(best_state)`` restores
nothing and the model ends with the last epoch's weights:
``restore_best=False`` (the default) reproduces that, ``restore_best=True``
restores a real snapshot taken on the device after the best epoch.  The
scaler fit stays on the host.

``SGU1Forest`` is SGU1's inference side (GateUnits.py:7-40, an
xgboost.XGBRegressor): it reads xgboost's JSON model, packs the trees on the
host and runs sgmm_sgu1_predict over the device feature table of
``EventBarsGPU.sgu1_table`` (or any [n, 20] rows).  SGU1 *training* stays
with xgboost on the host.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr, stream_ptr

_KEYS = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc.weight", "fc.bias")


class SGU2Model(nn.Module):
    """GateUnits.py:42-54 (weights and state_dict layout)."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.lstm = nn.LSTM(input_size, hidden_size, batch_first=True)
        self.dropout = nn.Dropout(0.8)
        self.fc = nn.Linear(hidden_size, 1)

    def flat_weights(self) -> torch.Tensor:
        sd = self.state_dict()
        return torch.cat([sd[k].detach().reshape(-1).float().cpu() for k in _KEYS])


class StandardScaler3D:
    """utils/scaler.py: per-feature mean/std over (samples, time), + 1e-9."""

    def __init__(self, threshold=3.0):
        self.mean = None
        self.std = None
        self.threshold = threshold

    def fit(self, X):
        self.mean = np.mean(X, axis=(0, 1), keepdims=True)
        self.std = np.std(X, axis=(0, 1), keepdims=True) + 1e-9

    def transform(self, X):
        if self.mean is None or self.std is None:
            raise ValueError("Scaler has not been fitted yet.")
        return (X - self.mean) / self.std

    def fit_transform(self, X):
        self.fit(X)
        return self.transform(X)


class SGU2:
    """GateUnits.py:56-136 (inference side)."""

    def __init__(self, input_size=1, hidden_size=10, device="cpu"):
        if input_size != 1:
            raise ValueError("SGU2 windows carry one feature (HFTLoader.py:165-169)")
        self.device = torch.device(device)
        self.hidden_size = hidden_size
        self.model = SGU2Model(input_size, hidden_size)
        self.best_state = None
        self._w = None

    def _weights(self, dev):
        w = self.model.flat_weights()
        if self._w is None or self._w.device != dev or not torch.equal(self._w.cpu(), w):
            self._w = w.to(dev)
        return self._w

    def predict_device(self, X: torch.Tensor, scaler=None, out: torch.Tensor | None = None) -> torch.Tensor:
        """Windows [n, T, 1] (or [n, T]) float32 on the device -> float32 [n]
        (scaler: a fitted StandardScaler3D, applied in the kernel)."""
        _lib.require_gpu()
        L = _lib.load()
        X = X.contiguous()
        if X.dtype != torch.float32 or X.device.type != "cuda":
            raise TypeError("predict_device needs float32 windows on the device")
        n, T = int(X.shape[0]), int(X.shape[1]) if X.dim() > 1 else 0
        dev = X.device
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        m = s = None
        if scaler is not None:
            if np.asarray(scaler.mean).size != 1:
                raise ValueError("SGU2 windows carry one feature")
            m = torch.tensor(np.asarray(scaler.mean, np.float32).reshape(1), device=dev)
            s = torch.tensor(np.asarray(scaler.std, np.float32).reshape(1), device=dev)
        check(L.sgmm_sgu2_forward(ptr(self._weights(dev)), self.hidden_size, ptr(X), n, T, ptr(m), ptr(s),
                                  ptr(out), stream_ptr()), "sgmm_sgu2_forward")
        return out[:n]

    def predict(self, X):
        """GateUnits.py:116-120: numpy windows [n, T, 1] -> float32 [n, 1]."""
        X_t = torch.tensor(np.asarray(X), dtype=torch.float32).to("cuda")
        return self.predict_device(X_t).reshape(-1, 1).cpu().numpy()

    def train(self, X_train, y_train, X_val, y_val, batch_size=128, epochs=100, lr=0.001, *, seed=None,
              restore_best=False, schedule=None):
        """GateUnits.py:66-114 as one launch: numpy windows [n, T, 1] and labels [n]
        -> {'train_loss': [...], 'val_loss': [...]}; the trained weights are left
        in self.model.  seed=None draws one int64 from torch's default generator;
        schedule=(perm[epochs, n], keep[epochs, n, H]) replaces the Philox schedule."""
        return train_sgu2_many([self], X_train, y_train, X_val, y_val, batch_size, epochs, lrs=lr, seeds=seed,
                               restore_best=restore_best, schedules=None if schedule is None else [schedule])[0]

    def train_device(self, X_train, y_train, X_val, y_val, batch_size=128, epochs=100, lr=0.001, *, scaler=None,
                     label_scale=1.0, seed=None, restore_best=False, schedule=None):
        """train() on float32 windows / labels that are already on the device
        (sgmm_bar_windows' output); the fitted StandardScaler3D and the label
        scale (sgu_trainer.py:55) are applied in the kernel."""
        for t in (X_train, y_train, X_val, y_val):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda":
                raise TypeError("train_device needs float32 windows and labels on the device")
        return train_sgu2_many([self], X_train, y_train, X_val, y_val, batch_size, epochs, lrs=lr, seeds=seed,
                               restore_best=restore_best, schedules=None if schedule is None else [schedule],
                               scaler=scaler, label_scale=label_scale)[0]

    def save(self, path):
        torch.save(self.model.state_dict(), path)

    def load(self, path):
        self.model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
        self.model.eval()
        print(f"SGU2 model loaded from {path} and set to eval mode.")


# ----------------------------------------------------------------- training (sgmm_sgu2_train)
PATIENCE = 5  # GateUnits.py:78


def n_params(hidden: int) -> int:
    return 4 * hidden + 4 * hidden * hidden + 8 * hidden + hidden + 1


def _load_flat(model: SGU2Model, flat: torch.Tensor) -> None:
    """Copy flat weights (sgmm_sgu2_forward layout) into the model's parameters in place."""
    sd = model.state_dict()
    o = 0
    with torch.no_grad():
        for k in _KEYS:
            m = sd[k].numel()
            sd[k].copy_(flat[o:o + m].reshape(sd[k].shape))
            o += m


def _scaler_tensors(scaler, dev):
    if scaler is None:
        return None, None
    if np.asarray(scaler.mean).size != 1:
        raise ValueError("SGU2 windows carry one feature")
    return (torch.tensor(np.asarray(scaler.mean, np.float32).reshape(1), device=dev),
            torch.tensor(np.asarray(scaler.std, np.float32).reshape(1), device=dev))


def _windows(X, dev):
    X = torch.as_tensor(np.asarray(X) if not isinstance(X, torch.Tensor) else X, dtype=torch.float32).to(dev)
    if X.dim() == 3 and X.shape[2] == 1:
        X = X[:, :, 0]
    if X.dim() != 2:
        raise ValueError("SGU2 windows are [n, T, 1] or [n, T]")
    return X.contiguous()


def _labels(y, dev):
    y = torch.as_tensor(np.asarray(y) if not isinstance(y, torch.Tensor) else y, dtype=torch.float32).to(dev)
    return y.reshape(-1).contiguous()


def sgu2_schedule(seed: int, n: int, hidden: int, epochs: int, device="cuda"):
    """The schedule `seed` yields: (perm int32 [epochs, n], keep uint8 [epochs, n, hidden])."""
    _lib.require_gpu()
    L = _lib.load()
    perm = torch.empty((epochs, n), dtype=torch.int32, device=device)
    keep = torch.empty((epochs, n, hidden), dtype=torch.uint8, device=device)
    check(L.sgmm_sgu2_schedule(int(seed) & (2**64 - 1), n, hidden, epochs, ptr(perm), ptr(keep), stream_ptr()),
          "sgmm_sgu2_schedule")
    return perm, keep


def sgu2_loss_grad(weights: torch.Tensor, hidden: int, X: torch.Tensor, y: torch.Tensor, keep=None, scaler=None,
                   label_scale=1.0):
    """One minibatch of the trainer's device code: (loss [1], grad [P]) float32 on
    the device.  keep: uint8 [n, hidden] (train mode, h * keep * 5) or None (eval mode)."""
    _lib.require_gpu()
    L = _lib.load()
    dev = weights.device
    X, y = _windows(X, dev), _labels(y, dev)
    n, T = int(X.shape[0]), int(X.shape[1])
    m, s = _scaler_tensors(scaler, dev)
    if keep is not None:
        keep = torch.as_tensor(keep).to(device=dev, dtype=torch.uint8).contiguous()
    nbytes = L.sgmm_sgu2_train_workspace_bytes(hidden, T, 1)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grad = torch.empty(n_params(hidden), dtype=torch.float32, device=dev)
    check(L.sgmm_sgu2_loss_grad(ptr(weights), hidden, ptr(X), ptr(y), n, T, ptr(keep), ptr(m), ptr(s),
                                float(label_scale), ptr(loss), ptr(grad), ptr(ws), nbytes, stream_ptr()),
          "sgmm_sgu2_loss_grad")
    return loss, grad


def run_fits(hidden, weights, data, batch_size, epochs, lrs, seeds, *, snapshot=False, schedules=None, scaler=None,
             label_scale=1.0, patience=PATIENCE, device="cuda"):
    """K fits of one hidden size in one launch.  weights: float32 [K, P] initial
    weights (any device); data: K tuples (X_train, y_train, X_val, y_val), numpy or
    device tensors (shared objects are uploaded once).  Returns the raw outputs:
    dict(weights [K, P], best [K, P] or None, train_loss / val_loss float64 [K, epochs],
    epochs_run, best_epoch int32 [K]) as CPU tensors."""
    _lib.require_gpu()
    L = _lib.load()
    dev = torch.device(device)
    K, P = len(data), n_params(hidden)
    w = torch.as_tensor(weights, dtype=torch.float32).reshape(K, P).to(dev).clone().contiguous()
    best = torch.zeros((K, P), dtype=torch.float32, device=dev) if snapshot else None
    hist_t = torch.full((K, max(epochs, 1)), float("nan"), dtype=torch.float64, device=dev)
    hist_v = torch.full((K, max(epochs, 1)), float("nan"), dtype=torch.float64, device=dev)
    ran = torch.zeros(K, dtype=torch.int32, device=dev)
    best_epoch = torch.full((K,), -1, dtype=torch.int32, device=dev)
    cache, keepalive, T = {}, [], None

    def up(a, f):
        if id(a) not in cache:
            cache[id(a)] = f(a, dev)
        return cache[id(a)]

    tasks = (_lib.Sgu2Task * K)()
    for k, (Xt, yt, Xv, yv) in enumerate(data):
        Xt, yt, Xv, yv = up(Xt, _windows), up(yt, _labels), up(Xv, _windows), up(yv, _labels)
        n, nv = int(Xt.shape[0]), int(Xv.shape[0])
        if n == 0:
            raise ValueError("no training windows")
        if T is None:
            T = int(Xt.shape[1])
        if int(Xt.shape[1]) != T or (nv and int(Xv.shape[1]) != T) or yt.numel() != n or yv.numel() != nv:
            raise ValueError("windows / labels of one launch must agree in shape")
        perm = keep = None
        if schedules is not None and schedules[k] is not None:
            perm, keep = schedules[k]
            if perm is not None:
                perm = torch.as_tensor(perm).to(device=dev, dtype=torch.int32).contiguous()
                if tuple(perm.shape) != (epochs, n) or (epochs and (int(perm.min()) < 0 or int(perm.max()) >= n)):
                    raise ValueError("perm must be [epochs, n] with values in [0, n)")
            if keep is not None:
                keep = torch.as_tensor(keep).to(device=dev, dtype=torch.uint8).contiguous()
                if tuple(keep.shape) != (epochs, n, hidden):
                    raise ValueError("keep must be [epochs, n, hidden]")
            keepalive += [perm, keep]
        t = tasks[k]
        t.X_train, t.y_train = Xt.data_ptr(), yt.data_ptr()
        t.X_val, t.y_val = (Xv.data_ptr(), yv.data_ptr()) if nv else (None, None)
        t.weights = w[k].data_ptr()
        t.best_weights = best[k].data_ptr() if snapshot else None
        t.perm = perm.data_ptr() if perm is not None else None
        t.keep = keep.data_ptr() if keep is not None else None
        t.train_loss, t.val_loss = hist_t[k].data_ptr(), hist_v[k].data_ptr()
        t.epochs_run, t.best_epoch = ran[k:].data_ptr(), best_epoch[k:].data_ptr()
        t.n, t.nv = n, nv
        t.seed = int(seeds[k]) & (2**64 - 1)
        t.lr = float(lrs[k])
    tasks_dev = torch.frombuffer(bytearray(bytes(tasks)), dtype=torch.uint8).to(dev)
    m, s = _scaler_tensors(scaler, dev)
    nbytes = L.sgmm_sgu2_train_workspace_bytes(hidden, T, K)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dev)
    check(L.sgmm_sgu2_train(ptr(tasks_dev), tasks, K, hidden, T, int(batch_size), int(epochs), int(patience),
                            ptr(m), ptr(s), float(label_scale), ptr(ws), nbytes, stream_ptr()), "sgmm_sgu2_train")
    return dict(weights=w.cpu(), best=best.cpu() if snapshot else None, train_loss=hist_t.cpu(),
                val_loss=hist_v.cpu(), epochs_run=ran.cpu(), best_epoch=best_epoch.cpu())


def train_sgu2_many(models, X_train, y_train, X_val, y_val, batch_size=128, epochs=100, lrs=0.001, *, seeds=None,
                    restore_best=False, schedules=None, scaler=None, label_scale=1.0):
    """K independent SGU2 fits (GateUnits.py:66-114 each), the fits of one hidden
    size in one launch.  X_train / y_train / X_val / y_val: one dataset shared by
    every model, or lists of K datasets; lrs / seeds: one value or K values
    (seeds=None draws K int64 from torch's default generator).  Each model ends
    as SGU2.train would leave it; returns the K histories."""
    K = len(models)
    many = isinstance(X_train, (list, tuple))
    data = [(X_train[k], y_train[k], X_val[k], y_val[k]) if many else (X_train, y_train, X_val, y_val)
            for k in range(K)]
    lrs = [float(lrs)] * K if np.isscalar(lrs) else [float(v) for v in lrs]
    if seeds is None:
        seeds = torch.randint(0, 2**63 - 1, (K,), dtype=torch.int64).tolist()
    elif np.isscalar(seeds):
        seeds = [int(seeds)] * K
    if len(lrs) != K or len(seeds) != K or (schedules is not None and len(schedules) != K):
        raise ValueError("lrs, seeds and schedules must have one entry per model")
    histories = [None] * K
    for hidden in sorted({m.hidden_size for m in models}):
        idx = [k for k in range(K) if models[k].hidden_size == hidden]
        out = run_fits(hidden, torch.stack([models[k].model.flat_weights() for k in idx]), [data[k] for k in idx],
                       batch_size, epochs, [lrs[k] for k in idx], [seeds[k] for k in idx], snapshot=restore_best,
                       schedules=None if schedules is None else [schedules[k] for k in idx], scaler=scaler,
                       label_scale=label_scale)
        for i, k in enumerate(idx):
            ran, best = int(out["epochs_run"][i]), int(out["best_epoch"][i])
            sgu = models[k]
            if ran - 1 - best >= PATIENCE:  # strict improvement: the best epoch is the last one that improved
                print(f"Early stopping at epoch {ran - 1}")
            _load_flat(sgu.model, out["weights"][i])
            sgu.best_state = None
            if best >= 0:
                if restore_best:
                    _load_flat(sgu.model, out["best"][i])
                    sgu.best_state = {n: v.clone() for n, v in sgu.model.state_dict().items()}
                else:
                    sgu.best_state = sgu.model.state_dict()  # the reference's alias of the live parameters
            sgu._w = None
            histories[k] = {"train_loss": [float(v) for v in out["train_loss"][i][:ran]],
                            "val_loss": [float(v) for v in out["val_loss"][i][:ran]]}
    return histories


# ----------------------------------------------------------------- SGU1 inference (sgmm_sgu1_predict)
SGU1_FEATURES = tuple([f"f_trades_{p}" for p in (1, 2, 3, 5, 10)] + [f"f_vwap_{r}" for r in (1, 3, 5)] +
                      [f"f_slope_{s}" for s in (1, 3, 5)] + [f"f_lag_rr_{k}" for k in (1, 2, 3, 4, 5)] +
                      ["f_spread", "f_vol_imb", "f_total_vol", "f_hour"])
MAX_FOREST_DEPTH = 6


def pack_forest(left, right, feat, value, default_left, tree_off):
    """Node arrays of a forest (tree t owns nodes tree_off[t] .. tree_off[t+1]; children are
    tree-local, -1 at a leaf; value is the threshold of a split and the weight of a leaf) ->
    (depth, blob): every tree as a complete binary tree of the forest's depth in the layout of
    sgmm_sgu1_forest_bytes (include/sgmm.h), a leaf above that depth filling its subtree.
    Raises ValueError for children out of range, features outside the 20 columns and walks
    that do not end within depth 6 (deeper trees, cycles).  The filler splits below a shallow
    leaf carry a NaN threshold and no default-left bit: every row goes right there, so such a
    leaf is reported at the rightmost position of its subtree."""
    left, right = np.asarray(left, np.int64).ravel(), np.asarray(right, np.int64).ravel()
    feat, dl = np.asarray(feat, np.int64).ravel(), np.asarray(default_left).ravel().astype(bool)
    value, off = np.asarray(value, np.float32).ravel(), np.asarray(tree_off, np.int64).ravel()
    T, N = len(off) - 1, len(left)
    if T < 0 or off[0] != 0 or off[-1] != N or (np.diff(off) < 1).any() or not (
            len(right) == len(feat) == len(dl) == len(value) == N):
        raise ValueError("forest arrays disagree in length, or a tree without nodes")
    size = np.repeat(np.diff(off), np.diff(off))
    leaf = left == -1
    if ((right == -1) != leaf).any() or ((~leaf) & ((left < 0) | (left >= size) | (right < 0) | (right >= size))).any():
        raise ValueError("child index outside its tree")
    if ((~leaf) & ((feat < 0) | (feat >= len(SGU1_FEATURES)))).any():
        raise ValueError(f"split feature outside the {len(SGU1_FEATURES)} columns")
    base = np.repeat(off[:-1], np.diff(off))
    lg, rg = np.where(leaf, np.arange(N), left + base), np.where(leaf, np.arange(N), right + base)
    levels = [off[:-1].reshape(T, 1)]  # node behind every position of the complete tree, level by level
    while not leaf[levels[-1]].all():
        if len(levels) > MAX_FOREST_DEPTH:
            raise ValueError(f"a walk does not end within depth {MAX_FOREST_DEPTH}")
        cur = levels[-1]
        levels.append(np.stack([lg[cur], rg[cur]], axis=-1).reshape(T, -1))
    while len(levels) < 2:  # a forest of single leaves: one filler split whose sides agree
        levels.append(np.repeat(levels[-1], 2, axis=1))
    D = len(levels) - 1
    inner = np.concatenate(levels[:-1], axis=1)  # [T, 2^D - 1], level order
    blob = np.zeros((T, 3 * (1 << D) - 2), np.uint32)
    split = ~leaf[inner]
    blob[:, 0:2 * inner.shape[1]:2] = np.where(split, value[inner], np.float32(np.nan)).astype(np.float32).view(np.uint32)
    blob[:, 1:2 * inner.shape[1]:2] = np.where(split, feat[inner] | (dl[inner].astype(np.int64) << 31), 0)
    blob[:, 2 * inner.shape[1]:] = value[levels[-1]].view(np.uint32)
    return D, blob


class SGU1Forest:
    """SGU1 inference (GateUnits.py:7-40's XGBRegressor.predict) on the device:
    a gbtree model of reg:squarederror read from xgboost's JSON, packed into
    complete trees and walked by sgmm_sgu1_predict.  predict() uses the first
    best_iteration + 1 trees when the model carries that attribute, as
    XGBRegressor.predict does after early stopping (``n_trees`` overrides)."""

    feature_names = SGU1_FEATURES

    def __init__(self, model_path=None):
        self.model_path = model_path
        self.left = self.right = self.feat = self.value = self.default_left = self.tree_off = None
        self.base_score = np.float32(0.5)
        self.best_iteration = None
        self.n_trees = 0
        self.depth, self._blob, self._dev = 0, None, {}
        if model_path is not None:
            self.load(model_path)

    @classmethod
    def from_arrays(cls, left, right, feat, value, default_left, tree_off, base_score, best_iteration=None):
        self = cls()
        self.left, self.right = np.asarray(left, np.int32).ravel(), np.asarray(right, np.int32).ravel()
        self.feat, self.value = np.asarray(feat, np.int32).ravel(), np.asarray(value, np.float32).ravel()
        self.default_left = np.asarray(default_left).ravel().astype(np.uint8)
        self.tree_off = np.asarray(tree_off, np.int64).ravel()
        self.base_score = np.float32(base_score)
        total = len(self.tree_off) - 1
        self.best_iteration = None if best_iteration is None or int(best_iteration) < 0 else int(best_iteration)
        self.n_trees = total if self.best_iteration is None else min(self.best_iteration + 1, total)
        self.depth, self._blob = pack_forest(self.left, self.right, self.feat, self.value, self.default_left,
                                             self.tree_off)
        self._dev = {}
        return self

    def load(self, path):
        """xgboost's JSON model (Booster.save_model / XGBRegressor.save_model)."""
        import json
        with open(path) as fh:
            learner = json.load(fh)["learner"]
        booster = learner["gradient_booster"]
        if booster.get("name") != "gbtree":
            raise ValueError(f"booster {booster.get('name')!r}: only gbtree is supported")
        if learner["objective"]["name"] != "reg:squarederror":
            raise ValueError(f"objective {learner['objective']['name']!r}: only reg:squarederror is supported")
        par = learner["learner_model_param"]
        if int(par.get("num_target", "1")) != 1 or int(par.get("num_class", "0")) > 1:
            raise ValueError("only one target is supported")
        if int(par["num_feature"]) != len(SGU1_FEATURES):
            raise ValueError(f"model of {par['num_feature']} features: SGU1 has {len(SGU1_FEATURES)}")
        names = learner.get("feature_names") or list(SGU1_FEATURES)
        if tuple(names) != SGU1_FEATURES:
            raise ValueError("feature_names differ from SGU1DataPro.gen_dataset's columns")
        model = booster["model"]
        if int(model["gbtree_model_param"].get("num_parallel_tree", "1")) != 1:
            raise ValueError("num_parallel_tree != 1")
        trees = model["trees"]
        for t in trees:
            if any(int(s) != 0 for s in t.get("split_type", [])) or len(t.get("categories", [])):
                raise ValueError("categorical splits are not supported")
            if int(t["tree_param"].get("size_leaf_vector", "1")) > 1:
                raise ValueError("vector leaves are not supported")
        cat = lambda k, dt: np.concatenate([np.asarray(t[k], dt) for t in trees]) if trees else np.zeros(0, dt)
        best = learner.get("attributes", {}).get("best_iteration")
        other = self.from_arrays(cat("left_children", np.int32), cat("right_children", np.int32),
                                 cat("split_indices", np.int32), cat("split_conditions", np.float32),
                                 cat("default_left", np.uint8),
                                 np.concatenate([[0], np.cumsum([len(t["left_children"]) for t in trees])]),
                                 np.float32(str(par["base_score"]).strip("[] ")), None if best is None else int(best))
        self.__dict__.update(other.__dict__)
        self.model_path = path
        return self

    def _device_blob(self, dev):
        key = str(dev)
        if key not in self._dev:
            self._dev = {key: torch.from_numpy(self._blob.view(np.int32).reshape(-1).copy()).to(dev)}
        return self._dev[key]

    def predict_device(self, X: torch.Tensor, ld: int, n: int, *, n_trees=None, leaves=False):
        """X: the float32 feature-major matrix [20 * ld] on the device (sgmm_sgu1_features'
        layout) -> float32 [n] (and int32 leaf positions [n, n_trees] with leaves=True)."""
        _lib.require_gpu()
        L = _lib.load()
        if self._blob is None:
            raise ValueError("SGU1Forest holds no model")
        if X.dtype != torch.float32 or X.device.type != "cuda" or not X.is_contiguous():
            raise TypeError("predict_device needs a contiguous float32 matrix on the device")
        nt = self.n_trees if n_trees is None else int(n_trees)
        if not 0 <= nt <= len(self.tree_off) - 1 or not 0 <= n <= ld or X.numel() < len(SGU1_FEATURES) * ld:
            raise ValueError("n_trees, n or ld out of range")
        dev = X.device
        blob = self._device_blob(dev)
        out = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        lv = torch.empty((max(n, 1), max(nt, 1)), dtype=torch.int32, device=dev) if leaves else None
        check(L.sgmm_sgu1_predict(ptr(blob), blob.numel() * 4, self.depth, nt, float(self.base_score), ptr(X), ld, n,
                                  ptr(out), ptr(lv), stream_ptr()), "sgmm_sgu1_predict")
        return (out[:n], lv[:n, :nt]) if leaves else out[:n]

    def _matrix(self, X):
        """DataFrame / array [n, 20] -> xgboost's float32 matrix, feature-major on the device."""
        if hasattr(X, "columns"):
            if tuple(X.columns) != SGU1_FEATURES:
                raise ValueError("columns differ from SGU1DataPro.gen_dataset's")
            X = X.to_numpy(dtype=np.float64)
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != len(SGU1_FEATURES):
            raise ValueError(f"SGU1 rows carry {len(SGU1_FEATURES)} features")
        n = X.shape[0]
        Xt = np.ascontiguousarray(X.astype(np.float32).T).reshape(-1) if n else np.zeros(len(SGU1_FEATURES), np.float32)
        return torch.from_numpy(Xt).to("cuda"), max(n, 1), n

    def predict(self, X, n_trees=None):
        Xd, ld, n = self._matrix(X)
        return self.predict_device(Xd, ld, n, n_trees=n_trees).cpu().numpy()

    def pred_leaf(self, X, n_trees=None):
        """Position 0 .. 2^depth - 1 of the leaf every tree ends in (in the packed complete
        tree; the analogue of Booster.predict(pred_leaf=True)'s node ids): int32 [n, n_trees]."""
        Xd, ld, n = self._matrix(X)
        return self.predict_device(Xd, ld, n, n_trees=n_trees, leaves=True)[1].cpu().numpy()
