#!/usr/bin/env python
"""Time SGU1 training: the reference-shaped fit (8 812 training rows, 2 200
validation rows, 20 synthetic features, the reference's parameters: depth 4,
eta 0.01, alpha 0.01, min_child_weight 4, up to 1 000 rounds, early stopping
after 20 stale rounds) as one launch of sgmm_sgu1_train, at K = 1 and K = 8
fits per launch, and the numpy model of tests/sgu1_train_model.py on this
host for scale (timed over --model-rounds rounds and scaled to the rounds the
device fit ran).

There is no xgboost time to compare with: xgboost is not on the machines this
project is built on, and the trainer is this project's own contract, not
xgboost's.  The comparison is against a numpy model of the same contract.
Prints one JSON line.

    python tools/bench_sgu1_train.py [--fits 8] [--model-rounds 20] [--rounds 1000]
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
sys.path.insert(0, str(ROOT / "tests"))

import sgmm_pkg  # noqa: E402

sgmm_pkg.load()
import sgu1_train_model as tm  # noqa: E402
from sgmm_amd import _lib  # noqa: E402
from sgmm_amd import gate_units as gu  # noqa: E402

N_TRAIN, N_VAL = 8812, 2200


def table(seed=0):
    """Columns shaped like the SGU1 table: counts, a slowly moving price, small slopes, lagged
    labels on a 1e-4 grid, an hour; the label depends on a few of them plus noise."""
    rng = np.random.default_rng(seed)
    n = N_TRAIN + N_VAL
    X = np.empty((n, 20), np.float32)
    tr = rng.poisson(30, n).astype(np.float64)
    for j, p in enumerate((1, 2, 3, 5, 10)):
        X[:, j] = np.convolve(tr, np.ones(p))[:n]
    price = 3.0 + 0.001 * np.cumsum(rng.integers(-2, 3, n))
    for j, r in enumerate((1, 3, 5)):
        X[:, 5 + j] = np.convolve(price, np.ones(r) / r)[:n]
    X[:, 8] = 0.0
    X[:, 9], X[:, 10] = 1e-3 * rng.normal(size=n), 1e-3 * rng.normal(size=n)
    lab = np.round(np.abs(rng.normal(0.002, 0.001, n)), 4)
    for L in range(1, 6):
        X[:, 10 + L] = np.roll(lab, L)
    X[:, 16] = 0.001 * rng.integers(1, 4, n)
    X[:, 17] = rng.uniform(-1, 1, n)
    X[:, 18] = rng.integers(1, 400, n) * 100.0
    X[:, 19] = rng.integers(9, 15, n)
    y = 1000 * (0.5 * X[:, 11] + 0.2 * X[:, 12] + 0.3 * X[:, 16] * (X[:, 1] > 60)) + 0.4 * rng.normal(size=n)
    return X, y.astype(np.float32)


def device_fits(X, y, K, params, repeats=3):
    Xd, yd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda(), torch.from_numpy(y).cuda()
    spec = dict(X_train=Xd, y_train=yd, rows_train=np.arange(N_TRAIN), X_val=Xd, y_val=yd,
                rows_val=N_TRAIN + np.arange(N_VAL), params=params)
    wall, kern = [], []
    _lib.profile_enable(True)
    for _ in range(repeats + 1):  # the first run warms up
        torch.cuda.synchronize()
        _lib.profile_read()
        t0 = time.perf_counter()
        out = gu.run_sgu1_fits([spec] * K)
        wall.append(time.perf_counter() - t0)  # the results are on the host: the launch has finished
        prof = _lib.profile_read()
        kern.append((prof["sgu1_train"][0], prof["sgu1_bin"][0]))
    _lib.profile_enable(False)
    return float(np.median(wall[1:])), float(np.median([k[0] for k in kern[1:]])), \
        float(np.median([k[1] for k in kern[1:]])), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--fits", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=1000)
    ap.add_argument("--model-rounds", type=int, default=20)
    a = ap.parse_args()
    X, y = table()
    params = gu.sgu1_fit_params(dict(gu.SGU1_PARAMS, n_estimators=a.rounds))
    one_wall, one_ms, bin_ms, out = device_fits(X, y, 1, params)
    print(f"  device: 1 fit {one_wall:.3f} s wall, kernel {one_ms:.1f} ms", file=sys.stderr, flush=True)
    many_wall, many_ms, _, outs = device_fits(X, y, a.fits, params)
    print(f"  device: {a.fits} fits {many_wall:.3f} s wall, kernel {many_ms:.1f} ms", file=sys.stderr, flush=True)
    rounds = out[0]["n_trees"]
    assert all(tm.same_fit(o, out[0]) for o in outs)
    t0 = time.perf_counter()
    model = tm.fit(X[:N_TRAIN], y[:N_TRAIN], X[N_TRAIN:], y[N_TRAIN:],
                   **dict(params, n_estimators=min(a.model_rounds, rounds), early_stopping_rounds=0))
    model_s = time.perf_counter() - t0
    k = model["n_trees"]
    same = all(np.array_equal(model[key][:int(model["tree_off"][k])], out[0][key][:int(model["tree_off"][k])])
               for key in ("left", "right", "feat", "value"))
    print(json.dumps({
        "n_train": N_TRAIN, "n_val": N_VAL, "max_depth": params["max_depth"], "rounds_run": rounds,
        "best_iteration": out[0]["best_iteration"], "best_score": out[0]["best_score"],
        "nodes": int(len(out[0]["left"])), "device_fit_wall_s": one_wall, "device_fit_kernel_ms": one_ms,
        "device_bin_kernel_ms": bin_ms, "device_us_per_round": 1e3 * one_ms / max(rounds, 1),
        f"device_{a.fits}_fits_wall_s": many_wall, f"device_{a.fits}_fits_kernel_ms": many_ms,
        "numpy_model_rounds_timed": k, "numpy_model_s_per_round": model_s / max(k, 1),
        "numpy_model_fit_s_scaled": model_s / max(k, 1) * rounds, "model_first_trees_equal": bool(same),
        "comparison": "numpy model of the same contract on the host; no xgboost time exists"}))


if __name__ == "__main__":
    main()
