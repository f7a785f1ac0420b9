"""SGU2 training, the checks that need no GPU: the C ABI of sgmm_sgu2_train /
sgmm_sgu2_loss_grad / sgmm_sgu2_schedule / sgmm_sgu2_train_workspace_bytes
(declared, exported, bound; the task record's layout compiled from the header;
argument errors before any HIP call) and the checker itself:
tests/sgu2_train_ref.py in float32 against the reference's own SGU2.train
recorded in tests/golden/g13_sgu2_train.npz (gen_golden_sgu2_train.py).

The restatement reproduces the reference's history and final weights bit for
bit on the generating machine; the test allows e_ref = |float32 - float64| of
the fixture, since another BLAS may sum in another order."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import sgu2_train_ref as tr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "sgmm.h"
NEW = ("sgmm_sgu2_train", "sgmm_sgu2_loss_grad", "sgmm_sgu2_schedule", "sgmm_sgu2_train_workspace_bytes")
FIELDS = ("X_train", "y_train", "X_val", "y_val", "weights", "best_weights", "perm", "keep", "train_loss",
          "val_loss", "epochs_run", "best_epoch", "n", "nv", "seed", "lr")


@pytest.fixture(scope="module")
def g13(golden):
    return golden("g13_sgu2_train.npz")


def test_symbols_are_declared_exported_and_bound(sgmm):
    from sgmm_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    L = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert f" T {name}\n" in nm, name
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.sgmm_abi_version() == 5  # additive change


def test_task_record_layout_matches_header(sgmm, tmp_path):
    """sizeof / offsetof of sgmm_sgu2_task as a C compiler lays the header out."""
    from sgmm_amd import _lib
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "sgmm.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(sgmm_sgu2_task));\n'
                   + "".join(f'    printf(" %zu", offsetof(sgmm_sgu2_task, {f}));\n' for f in FIELDS)
                   + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", f"-I{HEADER.parent}", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.Sgu2Task) == 128
    assert got[1:] == [getattr(_lib.Sgu2Task, f).offset for f in FIELDS]
    assert [f for f, _ in _lib.Sgu2Task._fields_] == list(FIELDS)


def task(**over):
    from sgmm_amd import _lib
    p = 8
    t = _lib.Sgu2Task(p, p, p, p, p, None, None, None, p, p, p, p, 100, 10, 1, 0.001)
    for k, v in over.items():
        setattr(t, k, v)
    return t


def train_rc(t=None, dev=8, host=True, n_tasks=1, hidden=10, T=10, batch=128, epochs=3, patience=5, mean=None,
             std=None, ws=8, ws_bytes=1 << 30):
    from sgmm_amd import _lib
    L = _lib.load()
    t = t if t is not None else task()
    rc = L.sgmm_sgu2_train(dev, ctypes.pointer(t) if host else None, n_tasks, hidden, T, batch, epochs, patience,
                           mean, std, 1.0, ws, ws_bytes, None)
    return rc, L.sgmm_last_error()


def test_train_argument_errors_need_no_gpu(sgmm):
    """Every argument error returns -1 with a message before any HIP call (the
    pointers are the invalid address 8: a launch would fault)."""
    for kw, word in ((dict(dev=None), b"null tasks"), (dict(host=False), b"null tasks"),
                     (dict(n_tasks=0), b"n_tasks"), (dict(hidden=12), b"hidden"), (dict(hidden=8), b"hidden"),
                     (dict(hidden=64), b"hidden"), (dict(T=0), b"time_steps"), (dict(batch=0), b"batch"),
                     (dict(batch=1025), b"batch"), (dict(epochs=-1), b"epochs"), (dict(patience=0), b"patience"),
                     (dict(mean=8), b"mean and std"), (dict(std=8), b"mean and std"),
                     (dict(ws=None), b"null workspace")):
        rc, msg = train_rc(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    for over, word in ((dict(n=0), b"no training windows"), (dict(n=-1), b"no training windows"),
                       (dict(n=2**31), b"2^31"), (dict(nv=-1), b"negative nv"), (dict(X_train=None), b"null training"),
                       (dict(y_train=None), b"null training"), (dict(X_val=None), b"null validation"),
                       (dict(y_val=None), b"null validation"), (dict(weights=None), b"null weights"),
                       (dict(train_loss=None), b"null output"), (dict(val_loss=None), b"null output"),
                       (dict(epochs_run=None), b"null output"), (dict(best_epoch=None), b"null output")):
        rc, msg = train_rc(task(**over))
        assert rc == -1 and word in msg, (over, msg)
    rc, msg = train_rc(ws_bytes=1000)
    assert rc == -3 and b"workspace" in msg
    # nv == 0 is legal (val_loss is then NaN) and needs no validation pointers: the call
    # gets as far as the workspace check
    rc, msg = train_rc(task(nv=0, X_val=None, y_val=None), ws_bytes=1000)
    assert rc == -3 and b"workspace" in msg


def test_loss_grad_and_schedule_argument_errors_need_no_gpu(sgmm):
    from sgmm_amd import _lib
    L = _lib.load()
    p = 8

    def lg(w=p, hidden=10, X=p, y=p, n=64, T=10, keep=None, mean=None, std=None, loss=p, grad=p, ws=p, nbytes=1 << 30):
        return L.sgmm_sgu2_loss_grad(w, hidden, X, y, n, T, keep, mean, std, 1.0, loss, grad, ws, nbytes, None)

    for kw, word in ((dict(w=None), b"null"), (dict(X=None), b"null"), (dict(y=None), b"null"),
                     (dict(loss=None), b"null"), (dict(grad=None), b"null"), (dict(hidden=11), b"hidden"),
                     (dict(T=0), b"time_steps"), (dict(n=0), b"batch"), (dict(n=1025), b"batch"),
                     (dict(mean=p), b"mean and std"), (dict(ws=None), b"null workspace")):
        assert lg(**kw) == -1 and word in L.sgmm_last_error(), kw
    assert lg(nbytes=1000) == -3
    for args, word in (((1, 0, 10, 3, p, p), b"n 0"), ((1, 100, 12, 3, p, p), b"hidden"),
                       ((1, 100, 10, -1, p, p), b"epochs"), ((1, 2**31, 10, 1, p, p), b"2^31")):
        assert L.sgmm_sgu2_schedule(*args, None) == -1 and word in L.sgmm_last_error(), args
    # nothing to write: success without a launch
    assert L.sgmm_sgu2_schedule(1, 100, 10, 0, p, p, None) == 0
    assert L.sgmm_sgu2_schedule(1, 100, 10, 3, None, None, None) == 0


def test_workspace_bytes_is_a_pure_monotone_function(sgmm):
    from sgmm_amd import _lib
    L = _lib.load()
    f = L.sgmm_sgu2_train_workspace_bytes
    assert f(10, 10, 1) == 256 * 10 * 61 * 4  # 256 samples x T x (6H + 1) float32
    for h in (10, 16, 32):
        for T in (1, 2, 10, 37):
            for k in (1, 3, 8):
                v = f(h, T, k)
                assert v == f(h, T, k) == 256 * T * (6 * h + 1) * 4 * k
                assert f(h, T + 1, k) > v and f(h, T, k + 1) > v
    assert f(10, 10, 1) < f(16, 10, 1) < f(32, 10, 1)
    for bad in ((12, 10, 1), (10, 0, 1), (10, 10, 0), (0, 10, 1)):
        assert f(*bad) == 0


def test_restatement_reproduces_the_reference(g13):
    """sgu2_train_ref in float32 against the reference's SGU2.train on g13's
    recovered schedule: history and final weights within e_ref (measured on the
    generating machine: identical bits)."""
    torch.set_num_threads(1)
    H, B, E = int(g13["hidden"]), int(g13["batch"]), int(g13["epochs"])
    r = tr.train(g13["w0"], H, g13["X_train"], g13["y_train"], g13["X_val"], g13["y_val"], g13["perm"], g13["keep"],
                 B, E, float(g13["lr"]), dtype=torch.float32)
    assert r["epochs_run"] == E and not r["stopped"]
    for name, got in (("train_loss", r["train_loss"]), ("val_loss", r["val_loss"]), ("weights", r["weights"])):
        ref32, ref64 = g13[f"ref_{name}"].astype(np.float64), g13[f"f64_{name}"]
        e_ref = max(float(np.max(np.abs(ref32 - ref64))), tr.EPS32 * float(np.max(np.abs(ref64))))
        err = float(np.max(np.abs(np.asarray(got, np.float64) - ref32)))
        print(f"g13 {name}: |restatement - reference| = {err:.3e}, e_ref = {e_ref:.3e}")
        assert err <= e_ref, name
    # the condition on the reference: every |g| of the float64 run is 0 or >= 1e-6
    r64 = tr.train(g13["w0"], H, g13["X_train"], g13["y_train"], g13["X_val"], g13["y_val"], g13["perm"],
                   g13["keep"], B, E, float(g13["lr"]), dtype=torch.float64)
    assert r64["min_grad"] >= tr.MIN_GRAD
    assert np.allclose(r64["weights"], g13["f64_weights"], rtol=0, atol=1e-12)
    # each epoch's recovered order is a permutation; the masks keep about one unit in five
    assert all(np.array_equal(np.sort(p), np.arange(len(p))) for p in g13["perm"])
    assert set(np.unique(g13["keep"])) == {0, 1} and 0.15 < g13["keep"].mean() < 0.25


def test_train_needs_a_gpu_and_never_falls_back(sgmm):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sgmm_amd.gate_units import SGU2
    X = np.zeros((8, 10, 1), np.float32)
    with pytest.raises(RuntimeError, match="no HIP device"):
        SGU2(1, 10).train(X, np.zeros(8, np.float32), X, np.zeros(8, np.float32), epochs=1, seed=1)
