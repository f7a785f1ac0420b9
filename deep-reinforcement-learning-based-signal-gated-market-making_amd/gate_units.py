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
restores a real snapshot taken on the device after the best epoch.  SGU1
(xgboost) stays on the host; the scaler fit stays on the host too.
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
