"""The attention planner (csrc/attn_plan.cpp: which kernel, which workgroup form and how many key slices a call gets) is host-only
C++.  g++ builds it with tests/san/attn_plan_main.cpp -- no HIP headers -- and the driver replays
tests/golden/attn_plan_choices.txt: the plan on a grid of (storage, head dim, batch, heads, queries, keys) under every A/B option,
the masked, plane-output, unaligned and unfused cases, and a list of refusals with their error statuses.  The driver itself checks
that no case of the grid is refused and that every instantiated kernel form and every automatic slice count occurs.  The fixture
was written by the planner's first form -- the rules of Engine::attention and of the three launchers moved out verbatim -- and has
not been regenerated since, so every choice the engine made then must be reproduced exactly: the slice count fixes the order in
which partial results are merged, and with it the bits of every fp32 result."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "stable_diffusion_burn_amd" / "csrc"
FIXTURE = ROOT / "tests" / "golden" / "attn_plan_choices.txt"


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_planner_reproduces_recorded_choices(tmp_path):
    exe = tmp_path / "attn_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "san" / "attn_plan_main.cpp"), str(CSRC / "attn_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert FIXTURE.stat().st_size < 256 * 1024
    r = subprocess.run([str(exe), str(FIXTURE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    n = len(FIXTURE.read_text().splitlines())
    assert r.stdout.strip() == f"{n} lines, 0 differ"
