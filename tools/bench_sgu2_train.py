#!/usr/bin/env python
"""Time SGU2 training: one reference-sized fit and K = 8 fits in one launch of
sgmm_sgu2_train, against the reference's loop (models/GateUnits.py:66-114:
DataLoader(shuffle=True), Dropout(0.8), MSELoss, Adam) run with torch on the
same GPU and on the CPU.

A reference-sized fit: H = 10, T = 10, batch 256, 50 epochs, the SGU2 windows
of the g6 fixture days tiled to about 50 000 training windows (10 % more for
validation).  Early stopping is switched off on both sides (patience = epochs)
so that every run does the same 50 x ceil(N / 256) Adam steps.  The torch loops
are timed over --torch-epochs epochs and scaled to 50 (their epochs cost the
same).  Prints one JSON line.

    python tools/bench_sgu2_train.py [--epochs 50] [--torch-epochs 3] [--fits 8] [--no-cpu]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import sgmm_pkg  # noqa: E402

sgmm_pkg.load()
from sgmm_amd import gate_units as gu  # noqa: E402


def windows(target):
    g6 = np.load(ROOT / "tests" / "golden" / "g6_bundle.npz", allow_pickle=False)
    real = np.concatenate([g6[f"d{k}_sgu2_X"] for k in range(len(g6["dates"])) if g6[f"d{k}_sgu2_X"].ndim == 3])
    sc = gu.StandardScaler3D()
    X = np.tile(sc.fit_transform(real.astype(np.float32)), (-(-target // len(real)), 1, 1)).astype(np.float32)
    rng = np.random.default_rng(0)
    X = X + 0.01 * rng.standard_normal(X.shape).astype(np.float32)  # the tiles are not exact copies
    y = (X[:, -1, 0] * 0.3 + rng.standard_normal(len(X))).astype(np.float32)
    nv = len(X) // 10
    return X[nv:], y[nv:], X[:nv], y[:nv]


class RefModel(gu.SGU2Model):
    def forward(self, x):  # GateUnits.py:49-54
        out, _ = self.lstm(x)
        return self.fc(self.dropout(out[:, -1, :]))


def torch_loop(X, y, Xv, yv, device, batch, epochs, lr=0.001):
    """The reference's loop, early stopping off; seconds per epoch."""
    from torch.utils.data import DataLoader, TensorDataset
    torch.manual_seed(0)
    model = RefModel(1, 10).to(device)
    Xt, yt = torch.tensor(X).to(device), torch.tensor(y).unsqueeze(1).to(device)
    Xv_t, yv_t = torch.tensor(Xv).to(device), torch.tensor(yv).unsqueeze(1).to(device)
    loader = DataLoader(TensorDataset(Xt, yt), batch_size=batch, shuffle=True)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    crit = torch.nn.MSELoss()
    per_epoch = []
    for _ in range(epochs + 1):  # the first epoch warms up (kernel selection, allocator)
        t0 = time.perf_counter()
        model.train()
        total = 0.0
        for bx, by in loader:
            opt.zero_grad()
            loss = crit(model(bx), by)
            loss.backward()
            opt.step()
            total += loss.item()
        model.eval()
        with torch.no_grad():
            crit(model(Xv_t), yv_t).item()
        per_epoch.append(time.perf_counter() - t0)
        print(f"  torch {device}: epoch {len(per_epoch) - 1} took {per_epoch[-1]:.3f} s", file=sys.stderr, flush=True)
    return float(np.median(per_epoch[1:]))


def device_fits(data, K, batch, epochs, repeats=3):
    ws = np.stack([gu.SGU2Model(1, 10).flat_weights().numpy() for _ in range(K)])
    times = []
    for _ in range(repeats + 1):  # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = gu.run_fits(10, ws, [data] * K, batch, epochs, [0.001] * K, list(range(1, K + 1)), patience=max(epochs, 1))
        times.append(time.perf_counter() - t0)  # run_fits returns host copies: the launch has finished
        assert int(out["epochs_run"].min()) == epochs and bool(torch.isfinite(out["val_loss"]).all())
    return float(np.median(times[1:])), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--windows", type=int, default=50_000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--torch-epochs", type=int, default=3)
    ap.add_argument("--fits", type=int, default=8)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    X, y, Xv, yv = windows(a.windows)
    # upload once: the timed region is the launch and the copy of its results
    data = tuple(torch.tensor(v).cuda() for v in (X, y, Xv, yv))
    steps = a.epochs * -(-len(X) // a.batch)
    one, out = device_fits(data, 1, a.batch, a.epochs)
    print(f"  device: 1 fit {one:.3f} s", file=sys.stderr, flush=True)
    many, _ = device_fits(data, a.fits, a.batch, a.epochs)
    print(f"  device: {a.fits} fits {many:.3f} s", file=sys.stderr, flush=True)
    res = {"n_train": len(X), "n_val": len(Xv), "hidden": 10, "time_steps": 10, "batch": a.batch, "epochs": a.epochs,
           "adam_steps": steps, "device_fit_s": one, "device_us_per_step": 1e6 * one / steps,
           f"device_{a.fits}_fits_s": many, "val_loss_first_last": [float(out["val_loss"][0][0]),
                                                                   float(out["val_loss"][0][a.epochs - 1])]}
    gpu_epoch = torch_loop(X, y, Xv, yv, "cuda", a.batch, a.torch_epochs)
    res.update(torch_gpu_fit_s=gpu_epoch * a.epochs, torch_gpu_us_per_step=1e6 * gpu_epoch * a.epochs / steps)
    if not a.no_cpu:
        cpu_epoch = torch_loop(X, y, Xv, yv, "cpu", a.batch, a.torch_epochs)
        res.update(torch_cpu_fit_s=cpu_epoch * a.epochs, torch_cpu_threads=torch.get_num_threads())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
