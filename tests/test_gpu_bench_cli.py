"""bench.py's command line: a plain run times the generations and prints the
headline figures only, --full adds the kernel profile and roofline, and
--dump-outputs writes what the last timed generation computed -- the same
arrays run after run and with or without --full.  Small shape (config 2's
single population of 64, H=16, 300 + 60 ticks: the fused-validation path)."""
import json
import sys

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--config", "2", "--ticks", "300", "--val-ticks", "60"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"roofline", "cpu_baseline", "speedup_vs_cpu_baseline", "kernels", "dominant_kernel",
             "gen_kernel_time_us"}


def _run(monkeypatch, capsys, extra):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *ARGS, *extra])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}


def test_plain_line_dump_and_full(sgmm, tmp_path, monkeypatch, capsys):
    a = _run(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / "a")])
    assert HEADLINE <= set(a) and not FULL_ONLY & set(a)
    assert a["steps"] == 3 and a["warmup"] == 2 and a["unit"] == "env-steps/s" and a["higher_is_better"] is True
    # value = training env-steps of the timed generations / their seconds
    assert a["value"] == pytest.approx(64 * 300 / (a["ms_per_step"] * 1e-3), rel=1e-9)

    da = _load(tmp_path / "a")
    assert {"fitness", "trades", "masters", "best_masters", "history_last"} <= set(da)
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in da.values())
    # fused validation: per population 64 training results, then 64 validation results
    fit, trd, row = da["fitness"].reshape(1, 2, 64), da["trades"].reshape(1, 2, 64), da["history_last"][0]
    best = int(np.argmax(fit[0, 0]))
    assert row[0] == fit[0, 0, best] == a["final_train_f"][0]      # train_f of the last timed generation
    assert row[1] == fit[0, 1, best]                               # val_f: the best's validation episode
    assert (row[3], row[4], row[5]) == (trd[0, 0, best], trd[0, 1, best], best)
    assert da["masters"].shape == (1, 16 * 16 + 7 * 16 + 2)

    # the same arguments give the same arrays, with or without --full
    _run(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / "b")])
    f = _run(monkeypatch, capsys, ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "c")])
    for other in ("b", "c"):
        do = _load(tmp_path / other)
        assert set(do) == set(da)
        for k in da:
            assert np.array_equal(da[k], do[k]), (other, k)
    assert FULL_ONLY <= set(f) and f["cpu_baseline"] is None
    assert f["kernels"] and f["roofline"]["frac"] > 0 and f["final_train_f"] == a["final_train_f"]
