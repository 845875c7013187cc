"""The GEMM planner (csrc/gemm_plan.cpp: which tile and how many K slices a launch gets) is host-only C++.  g++ builds it with
tests/san/gemm_plan_main.cpp -- no HIP headers -- and the driver replays tests/golden/gemm_plan_choices.txt: the cost model on a
grid of (M, N, k tiles) per kernel family, and the full plan (tables, options, forced tiles and split counts, error statuses)
on every measured shape.  The fixture was written by the planner's first form, the engine's choose_tile* functions moved out
verbatim, so every (cfg, splits) the engine chose then must be reproduced exactly: the K-reduction order, and with it the bits
of every result, follows from this choice."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "stable_diffusion_burn_amd" / "csrc"
FIXTURE = ROOT / "tests" / "golden" / "gemm_plan_choices.txt"


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_planner_reproduces_recorded_choices(tmp_path):
    exe = tmp_path / "gemm_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "san" / "gemm_plan_main.cpp"), str(CSRC / "gemm_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert FIXTURE.stat().st_size < 256 * 1024
    r = subprocess.run([str(exe), str(FIXTURE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    n = len(FIXTURE.read_text().splitlines())
    assert r.stdout.strip() == f"{n} lines, 0 differ"
