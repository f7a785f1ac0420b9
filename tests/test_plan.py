"""CPU checks of the launch plan (csrc/sgmm_plan.h): a stand-alone host program
(tests/plan_check.cpp, plain C++17, no GPU toolchain) resolves the plan of each
launch below and checks its workspace layout; the expected rows were derived by
hand from the rules, not from the code.  And the C ABI's workspace check agrees
with sgmm_rollout_workspace_bytes at the boundary."""
import ctypes
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "deep-reinforcement-learning-based-signal-gated-market-making_amd" / "csrc"


def launch(n, len=4560, **kw):
    """A launch line for plan_check: 1024 SIMDs, H = 32, 5 inventory values, no
    adversary, the training tail (mode 3) with 5 populations of n / 5 episodes
    (4 of n / 4 where 5 does not divide n: populations are whole), every knob
    at its default rule unless given."""
    d = dict(n=n, len=len, steps=n * len, nsi=5, H=32, arl=0, simds=1024, tail=1, mode=3,
             pop_eps=n // 5 if n % 5 == 0 else n // 4)
    d.update(kw)
    return d


# (name, launch, the fields of the plan the row pins)
ROWS = [
    ("config3", launch(2560),
     dict(policy="Frontier", g0=1, gtail=2, whole=1024, gmax=2, waves=4096, ls=1, spill=0, scan="Lanes", lanes_w=2,
          grid=1280, threads=128, seq_sum=1, rs=13025280)),
    ("n1536", launch(1536), dict(policy="Frontier", whole=1024, g0=1, gtail=2, waves=2048, ls=1)),
    ("n1024", launch(1024), dict(policy="Frontier", g0=2, gtail=2, waves=2048, ls=1, scan="Lanes", lanes_w=4)),
    ("n512", launch(512), dict(policy="Frontier", g0=4, ls=2, waves=2048, scan="Wave", threads=256, seq_sum=1)),
    ("n8192", launch(8192), dict(policy="Frontier", whole=8192, g0=1, gmax=1, scan="Fused")),
    ("n4096", launch(4096), dict(policy="Frontier", whole=4096, g0=1, gmax=1, scan="Fused")),
    ("n2048", launch(2048), dict(policy="Frontier", whole=2048, g0=1, gmax=1, scan="Fused")),
    ("n8192_mode0", launch(8192, mode=0), dict(policy="Frontier", scan="Wave", threads=64, seq_sum=1)),
    ("n8192_no_tail", launch(8192, tail=0, mode=0, pop_eps=0), dict(policy="Frontier", scan="Fused")),
    ("n64_h16", launch(64, H=16), dict(policy="TableV3", scan="Wave", threads=1024, seq_sum=0)),
    ("validation", launch(5, len=912, mode=4, pop_eps=1),
     dict(policy="TableSp", scan="Wave", threads=1024, seq_sum=1, gmax=8, validation=1)),
    ("arl_n256", launch(256, arl=1), dict(policy="TableMfma", scan="Arl", threads=1024, seq_sum=0)),
    ("arl_n2048", launch(2048, arl=1), dict(policy="TableMfma", scan="Arl", threads=256)),
    ("h64", launch(2560, H=64), dict(policy="TableMfma")),
    ("h8", launch(2560, H=8), dict(policy="TableValu")),
    ("long", launch(4, len=131073), dict(policy="Frontier")),
    # knobs
    ("groups17", launch(2560, groups=17),
     dict(policy="Frontier", g0=1, gtail=2, whole=1024, gmax=2, waves=4096, ls=1, spill=0, scan="Lanes", lanes_w=2,
          grid=1280, threads=128, seq_sum=1, rs=13025280)),
    ("groups2", launch(2560, groups=2), dict(g0=2, gtail=2, gmax=2, ls=1)),
    ("lane_split3", launch(512, lane_split=3), dict(ls=1)),
    ("fused_g2", launch(2560, fused_scan=1, groups=2), dict(scan="Fused")),
    ("fused_g3", launch(2560, fused_scan=1, groups=3), dict(scan="Lanes")),
    ("fused_g2_par", launch(2560, fused_scan=1, groups=2, seq_sum=0), dict(scan="Wave", seq_sum=0)),
    ("lanes1_n512", launch(512, lanes_scan=1), dict(scan="Lanes", lanes_w=4)),
    ("lanes3", launch(2560, lanes_scan=3), dict(scan="Lanes", lanes_w=2)),
    ("lanes3_n512", launch(512, lanes_scan=3), dict(scan="Lanes", lanes_w=4)),
    ("pop50", launch(2560, pop_eps=50), dict(scan="Wave", threads=64)),
    ("min_eps0", launch(512, min_eps=0), dict(policy="Frontier")),
    ("min_eps0_n511", launch(511, min_eps=0), dict(policy="TableV3")),
    ("valu", launch(2560, policy_path=3), dict(policy="TableValu")),
    ("path0_auto", launch(2560, policy_path=0), dict(policy="Frontier")),
    ("validation_v3", launch(5, len=912, mode=4, pop_eps=1, table_sp=0), dict(policy="TableV3")),
    # spill: microseconds -> 10 ns units, and no fused scan with it
    ("spill50", launch(8192, spill=50), dict(spill=5000, scan="Lanes", lanes_w=2)),
    ("spill_table", launch(64, H=16, spill=50), dict(policy="TableV3", spill=0)),
    # the walk-order feedback: whole + halves, one wave per walk, whole equal-length populations
    ("feedback", launch(2560, feedback=1, src_pop_eps=512), dict(reorder=1, w_whole=5, w_split=4)),
    ("feedback_weights", launch(2560, feedback=1, src_pop_eps=512, reorder_weights=5 << 8 | 3),
     dict(reorder=1, w_whole=5, w_split=3)),
    ("feedback_off", launch(2560, src_pop_eps=512), dict(reorder=0)),
    ("feedback_all_halves", launch(2560, feedback=1, src_pop_eps=512, groups=2), dict(reorder=0)),
    ("feedback_all_whole", launch(8192, feedback=1, src_pop_eps=2048), dict(reorder=0)),
    # the workspace sizes tests/test_capi.py pins through the C ABI
    ("ws_table", launch(4, len=250, tail=0, mode=0, pop_eps=0),
     dict(gmax=8, rs=9280,
          bytes=4 * 512 * 8 + 4 * 512 * 32 + 4 * 512 * 4 + 4 * 64 * 4 + 4 * 64 * 4 + 256 + 256 + 5 * 9280 * 8)),
    ("ws_arl", launch(4, len=250, arl=1, tail=0, mode=0, pop_eps=0), dict(rs=1024, bytes=8192 + 20 * 1024 * 8)),
    ("ws_arl_2", launch(1, len=5000, nsi=2, arl=1, tail=0, mode=0, pop_eps=0),
     dict(rs=5024, bytes=40192 + 8 * 5024 * 8)),
]


def one_population(P, H, arl, tail):
    """The launches of one population's 130 / 70-tick generation, as the
    single-population entry points describe them (pop_eps = src_pop_eps = 0)
    and as the sgmm_populations entries do with n_pop = 1 (= the launch's n):
    tail: sgmm_generation / sgmm_generation_multi (P training + P validation
    episodes, the whole generation's tail, mode 0); else the untailed asked
    rollout of sgmm_rollout_fitness_asked / _multi."""
    d = dict(n=2 * P, len=130, steps=P * 200, nsi=5, H=H, arl=arl, simds=1024, tail=tail, mode=0)
    return dict(d, pop_eps=0, src_pop_eps=0), dict(d, pop_eps=2 * P if tail else 0, src_pop_eps=2 * P)


# (name, the single-population launch, the same launch through sgmm_populations)
ONE_POP = [(f"P{P}_h{H}_arl{arl}_{'tail' if tail else 'asked'}",) + one_population(P, H, arl, tail)
           for P in (1, 24, 257, 600, 1100) for H in (16, 64) for arl in (0, 1) for tail in (1, 0)]
LAUNCHES = [(name, spec) for name, spec, _ in ROWS] + \
    [(f"{name}_{i}", spec) for name, *specs in ONE_POP for i, spec in enumerate(specs)]


@pytest.fixture(scope="module")
def plan_rows(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("plan") / "plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{CSRC}", "-o", str(exe),
                    str(ROOT / "tests" / "plan_check.cpp")], check=True)
    text = "".join(" ".join(f"{k}={v}" for k, v in spec.items()) + "\n" for _, spec in LAUNCHES)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr  # a layout violation names the section and the launch
    lines = run.stdout.splitlines()
    assert len(lines) == len(LAUNCHES)
    return {name: dict(tok.split("=") for tok in line.split()) for (name, _), line in zip(LAUNCHES, lines)}


@pytest.mark.parametrize("name,want", [(r[0], r[2]) for r in ROWS], ids=[r[0] for r in ROWS])
def test_plan_row(plan_rows, name, want):
    got = plan_rows[name]
    assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}, got


def test_groups17_is_the_default_plan(plan_rows):
    assert plan_rows["groups17"] == plan_rows["config3"]


@pytest.mark.parametrize("name", [r[0] for r in ONE_POP])
def test_one_population_plans_alike_through_either_entry(plan_rows, name):
    """pop_eps reaches the plan only through the mode-3 tail's rules (the lanes
    scan, the walk-order feedback), so a population driven through the
    sgmm_populations entries with n_pop = 1 launches what the single-population
    entries launch: the same kernels, groups, scan and workspace layout."""
    assert plan_rows[f"{name}_0"] == plan_rows[f"{name}_1"]


def _dummy_batch(_lib, n, length, adv):
    v = ctypes.c_void_p(8)  # never dereferenced: the workspace check precedes every HIP call
    ticks = _lib.Ticks(*[v] * 7)
    eps = _lib.Episodes(n, length, n * length, -2, 2, v, v if adv else None, v, v, v, v, None)
    return ticks, eps


@pytest.mark.parametrize("groups", [None, 2], ids=["default", "groups2"])
@pytest.mark.parametrize("n,length,hidden,adv", [(4, 250, 16, False), (600, 100, 32, False), (4, 250, 16, True)],
                         ids=["table", "frontier", "adversary"])
def test_workspace_check_agrees_with_reported_size(sgmm, plan, n, length, hidden, adv, groups):
    """One byte short of sgmm_rollout_workspace_bytes is refused, and the message
    quotes the same requirement: the size entry point and rollout_impl's carving
    share one layout."""
    from sgmm_amd import _lib
    L = _lib.load()
    if groups:
        plan(groups=groups)
    need = L.sgmm_rollout_workspace_bytes(n, n * length, 5, int(adv))
    assert need > 0
    ticks, eps = _dummy_batch(_lib, n, length, adv)
    v = ctypes.c_void_p(8)
    rc = L.sgmm_rollout_fitness(ctypes.byref(ticks), ctypes.byref(eps), v, v, hidden * hidden + 7 * hidden + 2, hidden,
                                v if adv else None, 74, v, v, v, need - 1, None)
    assert rc == -3, L.sgmm_last_error()  # SGMM_ERR_WORKSPACE
    assert f"workspace {need - 1} bytes < required {need}".encode() in L.sgmm_last_error()
