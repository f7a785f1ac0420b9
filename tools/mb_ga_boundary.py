"""Diagnostic: the stand-alone generation-boundary kernels, which bench.py on one
GPU never launches -- sgmm_ga_tell (label ga_tell), sgmm_ga_val_update
(ga_val_update) and sgmm_ga_step_multi (ga_step, K populations) at P = 512,
H = 32 with the adversary -- timed by the library's own profiler.  One JSON
line; A/B two libraries with SGMM_LIB, one fresh process each.
    python tools/mb_ga_boundary.py [launches=300] [K=5]"""
import ctypes
import json
import os
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
import sgmm_pkg
sg = sgmm_pkg.load()
from sgmm_amd import _lib
from sgmm_amd.drl_engine import STATE_DTYPE
N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
K = int(sys.argv[2]) if len(sys.argv) > 2 else 5
P, H, CAP = 512, 32, 1024
G_MM, G_ADV = H * H + 7 * H + 2, 1250
dev = torch.device("cuda")
L, ptr, s = _lib.load(), _lib.ptr, _lib.stream_ptr()
rec = np.zeros(K, STATE_DTYPE)
rec["sigma_mm"], rec["sigma_adv"], rec["best_val"], rec["patience"], rec["decay"] = 0.1, 0.3, -np.inf, 15, 0.5
rec["best_idx"] = rec["adv_best_idx"] = 3
st = torch.from_numpy(rec.view(np.uint8).reshape(K, -1).copy()).to(dev)
g = torch.Generator(device="cpu").manual_seed(1)
fit = torch.randn(K, P, generator=g, dtype=torch.float64).to(dev)
vfit = torch.randn(K, P, generator=g, dtype=torch.float64).to(dev)
trd = torch.arange(K * P, dtype=torch.int32).reshape(K, P).to(dev)
masters = torch.randn(K, G_MM, generator=g).to(dev)
madv = torch.randn(K, G_ADV, generator=g).to(dev)
slots = torch.zeros(K, G_MM, device=dev)
hist = torch.zeros((K, CAP, 40), dtype=torch.uint8, device=dev)
seeds = torch.arange(7, 7 + K, dtype=torch.int64).to(dev)
pops = _lib.Populations(K, P, H, CAP, st.data_ptr(), masters.data_ptr(), madv.data_ptr(), slots.data_ptr(),
                        seeds.data_ptr(), hist.data_ptr(), None)
calls = {
    "ga_tell": lambda: L.sgmm_ga_tell(ptr(st), ptr(fit), ptr(trd), P, ptr(masters), None, 0, ptr(madv), None, 0,
                                      G_MM, G_ADV, 7, ptr(hist), CAP, s),
    "ga_val_update": lambda: L.sgmm_ga_val_update(ptr(st), ptr(vfit), ptr(trd), 1, ptr(masters), ptr(slots), G_MM,
                                                  ptr(hist), CAP, s),
    "ga_step": lambda: L.sgmm_ga_step_multi(ctypes.byref(pops), ptr(fit), ptr(trd), ptr(vfit), ptr(trd), 8 * P, 4 * P,
                                            0, 0, s),
}
out = {"lib": os.path.basename(os.environ.get("SGMM_LIB", "libsgmm.so")), "launches": N, "P": P, "H": H, "K": K}
for label, call in calls.items():
    for _ in range(20):
        _lib.check(call(), label)
    torch.cuda.synchronize()
    _lib.profile_read()
    _lib.profile_enable(True)
    for _ in range(N):
        call()
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    assert list(prof) == [label] and prof[label][1] == N, prof
    out[label + "_us"] = prof[label][0] * 1e3 / N
print(json.dumps(out))
