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
``EventBarsGPU.sgu1_table`` (or any [n, 20] rows).

``SGU1`` is GateUnits.py:7-40 with the fit on the device: ``train`` /
``train_device`` / ``train_sgu1_many`` run whole fits of histogram
gradient-boosted trees as one launch of sgmm_sgu1_train (one workgroup per
fit, K fits per launch), ``save`` writes xgboost's JSON model.  The trainer is
the deterministic contract of include/sgmm.h -- xgboost's objective, gain,
weight, node numbering and early stopping over cuts that are data values --
not xgboost's own (no quantile sketch, no subsample / colsample, no weights).
The cuts and the exactly rounded base score are computed on the host.
"""
from __future__ import annotations

import ctypes
import math

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


# ----------------------------------------------------------------- SGU1 training (sgmm_sgu1_train)
SGU1_PARAMS = {"max_depth": 4, "min_child_weight": 4, "subsample": 1.0, "colsample_bytree": 1.0,
               "learning_rate": 0.01, "reg_alpha": 0.01, "objective": "reg:squarederror", "n_estimators": 1000,
               "early_stopping_rounds": 20}  # GateUnits.py:12-22
_SGU1_DEFAULTS = {"reg_lambda": 1.0, "gamma": 0.0, "max_bin": 256}  # xgboost's defaults of what the reference leaves out
_SGU1_KNOWN = set(SGU1_PARAMS) | set(_SGU1_DEFAULTS)
MAX_TRAIN_ROWS = 1 << 20
MAX_VAL_ROWS = (1 << 23) - 1  # the metric's int64 sum of squares of |v| <= 2^20 stays below 2^63 (include/sgmm.h)
_NODE_OUT = (("left", torch.int32), ("right", torch.int32), ("feature", torch.int32), ("value", torch.float32),
             ("default_left", torch.uint8), ("base_weight", torch.float32), ("loss_change", torch.float32),
             ("sum_hessian", torch.float32))


def sgu1_fit_params(params) -> dict:
    """The reference's parameter dict (xgboost's names) -> the trainer's, everything the
    trainer does not do rejected (ValueError) before anything touches the device."""
    p = dict(_SGU1_DEFAULTS)
    p.update(params)
    unknown = set(p) - _SGU1_KNOWN
    if unknown:
        raise ValueError(f"SGU1 parameters {sorted(unknown)} are not supported")
    if float(p.get("subsample", 1.0)) != 1.0 or float(p.get("colsample_bytree", 1.0)) != 1.0:
        raise ValueError("subsample / colsample_bytree other than 1 are not supported")
    if p.get("objective", "reg:squarederror") != "reg:squarederror":
        raise ValueError(f"objective {p['objective']!r}: only reg:squarederror is supported")
    out = dict(max_depth=int(p["max_depth"]), min_child_weight=float(p["min_child_weight"]),
               eta=float(p["learning_rate"]), reg_lambda=float(p["reg_lambda"]), reg_alpha=float(p["reg_alpha"]),
               gamma=float(p["gamma"]), max_bin=int(p["max_bin"]), n_estimators=int(p["n_estimators"]),
               early_stopping_rounds=int(p["early_stopping_rounds"] or 0))
    if not 1 <= out["max_depth"] <= MAX_FOREST_DEPTH:
        raise ValueError(f"max_depth {out['max_depth']} not in 1..{MAX_FOREST_DEPTH}")
    if not 2 <= out["max_bin"] <= 256:
        raise ValueError(f"max_bin {out['max_bin']} not in 2..256")
    if out["n_estimators"] < 1 or out["early_stopping_rounds"] < 0:
        raise ValueError("n_estimators < 1 or early_stopping_rounds < 0")
    for k in ("min_child_weight", "reg_lambda", "reg_alpha", "gamma"):
        if not (np.isfinite(out[k]) and out[k] >= 0):
            raise ValueError(f"{k} must be finite and >= 0")
    if not np.isfinite(out["eta"]):
        raise ValueError("learning_rate must be finite")
    if out["reg_lambda"] == 0 and out["min_child_weight"] == 0:
        raise ValueError("reg_lambda and min_child_weight are both 0")
    return out


def sgu1_cuts(X: torch.Tensor, rows: torch.Tensor, max_bin: int):
    """The cut rule over the training rows of the device matrix X [20, ld]: per feature the
    sorted distinct non-NaN values v (-0 and +0 one value); v[1:] when len(v) <= max_bin,
    else v[ceil(k len(v) / max_bin)], k = 1 .. max_bin - 1.  Not xgboost's weighted quantile
    sketch.  Returns (cuts float32 [20, 256], n_cuts int32 [20]) on the host."""
    cuts, n_cuts = np.zeros((len(SGU1_FEATURES), 256), np.float32), np.zeros(len(SGU1_FEATURES), np.int32)
    Xr = X.index_select(1, rows)
    for f in range(len(SGU1_FEATURES)):
        col = Xr[f]
        v = torch.unique(col[~torch.isnan(col)] + 0.0).cpu().numpy()  # sorted
        if len(v) > max_bin:
            k = np.arange(1, max_bin, dtype=np.int64)
            c = v[(k * len(v) + max_bin - 1) // max_bin]
        else:
            c = v[1:]
        cuts[f, :len(c)], n_cuts[f] = c, len(c)
    return cuts, n_cuts


def _rows(rows, ld, what):
    rows = np.ascontiguousarray(np.asarray(rows).ravel())
    if rows.size and (not np.issubdtype(rows.dtype, np.integer) or rows.min() < 0 or rows.max() >= ld):
        raise ValueError(f"{what} rows outside the table of {ld} rows")
    return rows.astype(np.int32)


def run_sgu1_fits(specs, device="cuda"):
    """K SGU1 fits in one launch.  specs: K dicts of X_train (float32 device matrix
    [20, ld], sgmm_sgu1_features' layout), y_train (float32 device labels [ld]), rows_train
    (host int rows), X_val / y_val / rows_val (or rows_val empty) and params (sgu1_fit_params'
    output).  Returns K dicts: the node arrays of the n_trees trees back to back with
    tree_off, base_score, val_rmse, n_trees, best_iteration (-1 without validation rows),
    best_score, and the final float32 predictions pred_train / pred_val read from the
    workspace (host arrays)."""
    prepared = []
    for k, s in enumerate(specs):  # every host-side check before the device is touched
        p = s["params"]
        Xt, yt = s["X_train"], s["y_train"]
        ld_t = int(Xt.shape[1])
        if len(s.get("rows_val", ())) > MAX_VAL_ROWS:
            raise ValueError(f"fit {k}: {len(s['rows_val'])} validation rows, not in 0..2^23-1")
        rt = _rows(s["rows_train"], ld_t, "training")
        rv = _rows(s.get("rows_val", ()), int(s["X_val"].shape[1]) if len(s.get("rows_val", ())) else 1, "validation")
        if not 1 <= len(rt) <= MAX_TRAIN_ROWS:
            raise ValueError(f"fit {k}: {len(rt)} training rows, not in 1..2^20")
        if p["early_stopping_rounds"] and not len(rv):
            raise ValueError(f"fit {k}: early stopping needs validation rows")
        prepared.append((rt, rv))
    _lib.require_gpu()
    L = _lib.load()
    dev = torch.device(device)
    K = len(specs)
    tasks = (_lib.Sgu1Task * K)()
    keep, outs, cache = [], [], {}
    for k, s in enumerate(specs):
        p, (rt, rv) = s["params"], prepared[k]
        Xt, yt = s["X_train"], s["y_train"]
        Xv, yv = (s["X_val"], s["y_val"]) if len(rv) else (None, None)
        for t in (Xt, yt, Xv, yv):
            if t is not None and (t.dtype != torch.float32 or t.device.type != "cuda" or not t.is_contiguous()):
                raise TypeError("SGU1 training needs contiguous float32 tables on the device")
        if Xt.shape[0] != len(SGU1_FEATURES) or yt.numel() < Xt.shape[1] or (
                Xv is not None and (Xv.shape[0] != len(SGU1_FEATURES) or yv.numel() < Xv.shape[1])):
            raise ValueError("tables are [20, ld] with ld labels")
        key = (Xt.data_ptr(), yt.data_ptr(), rt.tobytes(), p["max_bin"])
        if key not in cache:
            rt_d = torch.from_numpy(rt).to(dev)
            y_host = yt.index_select(0, rt_d.long()).cpu().numpy()
            if not np.isfinite(y_host).all():
                raise ValueError(f"fit {k}: non-finite training label")
            cuts, n_cuts = sgu1_cuts(Xt, rt_d.long(), p["max_bin"])
            base = np.float32(math.fsum(float(v) for v in y_host) / len(y_host))  # exactly rounded: no row order
            cache[key] = (rt_d, torch.from_numpy(cuts).to(dev), torch.from_numpy(n_cuts).to(dev), base)
        rt_d, cuts_d, ncuts_d, base = cache[key]
        rv_d = torch.from_numpy(rv).to(dev) if len(rv) else None
        if rv_d is not None and not bool(torch.isfinite(yv.index_select(0, rv_d.long())).all()):
            raise ValueError(f"fit {k}: non-finite validation label")
        n_est, stride = p["n_estimators"], (2 << p["max_depth"]) - 1
        o = {name: torch.zeros(n_est * stride, dtype=dt, device=dev) for name, dt in _NODE_OUT}
        o["tree_nodes"] = torch.zeros(n_est, dtype=torch.int32, device=dev)
        o["val_rmse"] = torch.full((n_est,), float("nan"), dtype=torch.float64, device=dev)
        o["n_trees"] = torch.zeros(1, dtype=torch.int32, device=dev)
        o["best_iteration"] = torch.full((1,), -1, dtype=torch.int32, device=dev)
        o["best_score"] = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
        nbytes = int(L.sgmm_sgu1_train_workspace_bytes(len(rt), len(rv)))
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        ws = ws[(-ws.data_ptr()) % 256:][:nbytes]
        t = tasks[k]
        t.X_train, t.y_train, t.rows_train = Xt.data_ptr(), yt.data_ptr(), rt_d.data_ptr()
        if rv_d is not None:
            t.X_val, t.y_val, t.rows_val = Xv.data_ptr(), yv.data_ptr(), rv_d.data_ptr()
        t.cuts, t.n_cuts, t.workspace = cuts_d.data_ptr(), ncuts_d.data_ptr(), ws.data_ptr()
        for name in o:
            setattr(t, name, o[name].data_ptr())
        t.ld_train, t.ld_val = int(Xt.shape[1]), int(Xv.shape[1]) if Xv is not None else 0
        t.n_train, t.n_val = len(rt), len(rv)
        t.max_depth, t.n_estimators, t.early_stopping_rounds = p["max_depth"], n_est, p["early_stopping_rounds"]
        t.max_bin, t.base_score = p["max_bin"], float(base)
        t.min_child_weight, t.eta, t.lambda_ = p["min_child_weight"], p["eta"], p["reg_lambda"]
        t.alpha, t.gamma = p["reg_alpha"], p["gamma"]
        keep += [rv_d, ws]
        outs.append((o, ws, base, stride))
    tasks_dev = torch.frombuffer(bytearray(bytes(tasks)), dtype=torch.uint8).to(dev)
    check(L.sgmm_sgu1_train(ptr(tasks_dev), tasks, K, stream_ptr()), "sgmm_sgu1_train")
    results = []
    for k, (o, ws, base, stride) in enumerate(outs):
        h = {name: v.cpu().numpy() for name, v in o.items()}
        nt, counts = int(h["n_trees"][0]), h["tree_nodes"]
        take = np.concatenate([t * stride + np.arange(counts[t]) for t in range(nt)]).astype(np.int64)
        n_tr, n_va = tasks[k].n_train, tasks[k].n_val
        pred = ws[:4 * (n_tr + n_va)].view(torch.float32).cpu().numpy()
        best = int(h["best_iteration"][0])
        results.append(dict(left=h["left"][take], right=h["right"][take], feat=h["feature"][take],
                            value=h["value"][take], default_left=h["default_left"][take],
                            base_weight=h["base_weight"][take], loss_change=h["loss_change"][take],
                            sum_hessian=h["sum_hessian"][take],
                            tree_off=np.concatenate([[0], np.cumsum(counts[:nt])]).astype(np.int64),
                            base_score=base, val_rmse=h["val_rmse"][:nt] if n_va else np.zeros(0, np.float64),
                            n_trees=nt, best_iteration=best, best_score=float(h["best_score"][0]),
                            pred_train=pred[:n_tr].copy(), pred_val=pred[n_tr:].copy()))
    return results


def _f32_list(a):
    return [float(str(v)) for v in np.asarray(a, np.float32)]  # the shortest decimal that reads back to the float32


def sgu1_json(fit) -> dict:
    """xgboost's JSON model document (Booster.save_model, version [3, 1, 3]) of a fit."""
    nf, off, trees = len(SGU1_FEATURES), fit["tree_off"], []
    for t in range(len(off) - 1):
        a, b = int(off[t]), int(off[t + 1])
        left, right = fit["left"][a:b], fit["right"][a:b]
        parents = np.full(b - a, 2147483647, np.int64)
        inner = np.nonzero(left != -1)[0]
        parents[left[inner]] = parents[right[inner]] = inner
        trees.append({
            "base_weights": _f32_list(fit["base_weight"][a:b]), "categories": [], "categories_nodes": [],
            "categories_segments": [], "categories_sizes": [], "default_left": fit["default_left"][a:b].tolist(),
            "id": t, "left_children": left.tolist(), "loss_changes": _f32_list(fit["loss_change"][a:b]),
            "parents": parents.tolist(), "right_children": right.tolist(),
            "split_conditions": _f32_list(fit["value"][a:b]), "split_indices": fit["feat"][a:b].tolist(),
            "split_type": [0] * (b - a), "sum_hessian": _f32_list(fit["sum_hessian"][a:b]),
            "tree_param": {"num_deleted": "0", "num_feature": str(nf), "num_nodes": str(b - a),
                           "size_leaf_vector": "1"}})
    mant, exp = np.format_float_scientific(np.float32(fit["base_score"]), unique=True).split("e")
    attributes = {"scikit_learn": '{"_estimator_type": "regressor"}'}
    if fit["best_iteration"] >= 0:
        attributes.update(best_iteration=str(int(fit["best_iteration"])), best_score=repr(float(fit["best_score"])))
    return {"learner": {
        "attributes": attributes, "feature_names": list(SGU1_FEATURES),
        "feature_types": ["int" if n == "f_hour" else "float" for n in SGU1_FEATURES],  # the frame's dtypes
        "gradient_booster": {"model": {
            "cats": {"enc": [], "feature_segments": [], "sorted_idx": []},
            "gbtree_model_param": {"num_parallel_tree": "1", "num_trees": str(len(trees))},
            "iteration_indptr": list(range(len(trees) + 1)), "tree_info": [0] * len(trees), "trees": trees},
            "name": "gbtree"},
        "learner_model_param": {"base_score": f"[{mant.rstrip('.')}E{int(exp)}]", "boost_from_average": "1",
                                "num_class": "0", "num_feature": str(nf), "num_target": "1"},
        "objective": {"name": "reg:squarederror", "reg_loss_param": {"scale_pos_weight": "1"}}},
        "version": [3, 1, 3]}


def _feature_major(X):
    """DataFrame / array [n, 20] -> float32 [20, n] (xgboost's float32 matrix, feature-major)."""
    if hasattr(X, "columns"):
        if tuple(X.columns) != SGU1_FEATURES:
            raise ValueError("columns differ from SGU1DataPro.gen_dataset's")
        X = X.to_numpy(dtype=np.float64)
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != len(SGU1_FEATURES):
        raise ValueError(f"SGU1 rows carry {len(SGU1_FEATURES)} features")
    return np.ascontiguousarray(X.astype(np.float32).T)


def _host_spec(X_train, y_train, X_val, y_val, params):
    n_val = 0 if X_val is None else len(X_val)
    if n_val > MAX_VAL_ROWS:
        raise ValueError(f"{n_val} validation rows, not in 0..2^23-1")
    Xt = _feature_major(X_train)
    Xv = _feature_major(X_val) if n_val else np.zeros((len(SGU1_FEATURES), 0), np.float32)
    y = np.concatenate([np.asarray(y_train, np.float64).ravel(),
                        np.asarray(y_val, np.float64).ravel() if n_val else np.zeros(0)]).astype(np.float32)
    n = Xt.shape[1]
    if len(y) != n + n_val:
        raise ValueError("labels and rows disagree in length")
    if not 1 <= n <= MAX_TRAIN_ROWS:
        raise ValueError(f"{n} training rows, not in 1..2^20")
    if params["early_stopping_rounds"] and not n_val:
        raise ValueError("early stopping needs validation rows")
    if not np.isfinite(y).all():
        raise ValueError("non-finite label")
    return dict(X=np.concatenate([Xt, Xv], axis=1), y=y, rows_train=np.arange(n), rows_val=np.arange(n, n + n_val),
                params=params)


def _event_rows(ev):
    return np.concatenate([np.arange(int(a), int(a) + int(n)) for a, n in zip(ev.sgu1_row_off, ev.sgu1_n_rows)] +
                          [np.zeros(0, np.int64)]).astype(np.int64)


def _device_spec(ev_train, ev_val, params):
    for ev in (ev_train, ev_val):
        if ev is not None and not hasattr(ev, "sgu1_X"):
            ev.sgu1_table()
    spec = dict(X_train=ev_train.sgu1_X, y_train=(ev_train.sgu1_label * 1000).float(),  # sgu_trainer.py:48
                rows_train=_event_rows(ev_train), params=params)
    if ev_val is not None:
        spec.update(X_val=ev_val.sgu1_X, y_val=(ev_val.sgu1_label * 1000).float(), rows_val=_event_rows(ev_val))
    return spec


class SGU1:
    """GateUnits.py:7-40 with the fit on the device: the reference's surface (params,
    train, predict, save, load) over sgmm_sgu1_train and an SGU1Forest.  The trainer is the
    deterministic histogram trainer of include/sgmm.h (xgboost's objective, gain, weight,
    node numbering and early stopping over this project's own cut rule), not xgboost's: the
    trees differ from an xgboost fit of the same data, the file format does not.

    After a fit: ``forest`` (an SGU1Forest that predicts with the first best_iteration + 1
    trees, as XGBRegressor does after early stopping), ``evals_result``
    ({'validation_0': {'rmse': [...]}}), ``best_iteration``, ``best_score`` and ``fit_``
    (run_sgu1_fits' arrays)."""

    def __init__(self, model_path=None, **params):
        self.params = dict(SGU1_PARAMS)
        self.params.update(params)
        self.model_path = model_path
        self.forest = self.fit_ = self._doc = None
        self.evals_result, self.best_iteration, self.best_score = {}, None, None

    def _take(self, fit):
        self.fit_, self._doc = fit, None
        best = fit["best_iteration"] if fit["best_iteration"] >= 0 else None
        self.forest = SGU1Forest.from_arrays(fit["left"], fit["right"], fit["feat"], fit["value"], fit["default_left"],
                                             fit["tree_off"], fit["base_score"], best)
        self.evals_result = {"validation_0": {"rmse": [float(v) for v in fit["val_rmse"]]}} if best is not None else {}
        self.best_iteration, self.best_score = best, (fit["best_score"] if best is not None else None)

    def train(self, X_train, y_train, X_val=None, y_val=None):
        """GateUnits.py:26-31: DataFrames / arrays [n, 20] and labels; one launch."""
        train_sgu1_many([self], [(X_train, y_train, X_val, y_val)])

    def train_device(self, ev_train, ev_val=None):
        """The SGU1 branch of run_sgu_training (sgu_trainer.py:77-81) straight from the device
        tables of two EventBarsGPU (sgu1_table's matrix, label * 1000): no host feature table."""
        train_sgu1_many([self], [(ev_train, ev_val)])

    def predict(self, X):
        if self.forest is None:
            raise ValueError("SGU1 holds no model")
        return self.forest.predict(X)

    def save(self, path):
        import json
        if self.fit_ is None and self._doc is None:
            raise ValueError("SGU1 holds no model")
        with open(path, "w") as fh:
            json.dump(sgu1_json(self.fit_) if self.fit_ is not None else self._doc, fh)

    def load(self, path):
        import json
        self.forest = SGU1Forest(path)
        with open(path) as fh:
            self._doc = json.load(fh)
        attrs = self._doc["learner"].get("attributes", {})
        self.fit_, self.evals_result = None, {}
        self.best_iteration = self.forest.best_iteration
        self.best_score = float(attrs["best_score"]) if "best_score" in attrs else None
        self.model_path = path


def train_sgu1_many(models, datasets):
    """K independent SGU1 fits in one launch.  models: K SGU1 (each with its own params:
    depth, learning_rate, reg_alpha, min_child_weight, ...); datasets: one dataset shared by
    all, or K of them, each (X_train, y_train, X_val, y_val) on the host or
    (ev_train, ev_val) -- EventBarsGPU holding their device tables.  Every model ends as
    SGU1.train would leave it; returns the K validation histories."""
    K = len(models)
    if len(datasets) == 1 and K > 1:
        datasets = list(datasets) * K
    if len(datasets) != K:
        raise ValueError("one dataset, or one per model")
    params = [sgu1_fit_params(m.params) for m in models]
    specs, uploaded = [], {}
    for k, d in enumerate(datasets):
        if len(d) == 2:
            specs.append(_device_spec(d[0], d[1], params[k]))
            continue
        key = tuple(id(a) for a in d)
        if key not in uploaded:
            uploaded[key] = _host_spec(*d, params[k])
        specs.append(dict(uploaded[key], params=params[k]))
    for s in specs:  # host tables go up once per distinct dataset
        if "X" in s:
            key = id(s["X"])
            if key not in uploaded:
                uploaded[key] = (torch.from_numpy(s["X"]).to("cuda") if torch.cuda.is_available() else None,
                                 torch.from_numpy(s["y"]).to("cuda") if torch.cuda.is_available() else None)
            Xd, yd = uploaded[key]
            if Xd is None:
                _lib.require_gpu()
            s.update(X_train=Xd, y_train=yd, X_val=Xd, y_val=yd)
    fits = run_sgu1_fits(specs)
    for m, fit in zip(models, fits):
        m._take(fit)
    return [m.evals_result.get("validation_0", {}).get("rmse", []) for m in models]
