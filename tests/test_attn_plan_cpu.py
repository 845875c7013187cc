"""The attention planner (csrc/attn_plan.cpp: which kernel, which workgroup form and how many key slices a call gets) is host-only
C++.  g++ builds it with tests/san/attn_plan_main.cpp -- no HIP headers -- and the driver replays
tests/golden/attn_plan_choices.txt: the plan on a grid of (storage, head dim, batch, heads, queries, keys) under every A/B option,
the masked, plane-output, unaligned and unfused cases, and a list of refusals with their error statuses.  The driver itself checks
that no case of the grid is refused and that every instantiated kernel form and every automatic slice count occurs.  The fixture
was written by the planner's first form -- the rules of Engine::attention and of the three launchers moved out verbatim -- and has
not been regenerated since, so every choice the engine made then must be reproduced exactly: the slice count fixes the order in
which partial results are merged, and with it the bits of every fp32 result.

A second, small fixture, tests/golden/attn_plan_masked_cases.txt, names its cases itself ("attn_plan --replay"): the shapes of
tests/test_attention_mask_gpu.py, so that each of them provably reaches the k_attn.hip instance its test is about."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "stable_diffusion_burn_amd" / "csrc"
FIXTURE = ROOT / "tests" / "golden" / "attn_plan_choices.txt"
MASKED_FIXTURE = ROOT / "tests" / "golden" / "attn_plan_masked_cases.txt"


def _build(tmp_path):
    exe = tmp_path / "attn_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "san" / "attn_plan_main.cpp"), str(CSRC / "attn_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_planner_reproduces_recorded_choices(tmp_path):
    exe = _build(tmp_path)
    assert FIXTURE.stat().st_size < 256 * 1024
    r = subprocess.run([str(exe), str(FIXTURE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    n = len(FIXTURE.read_text().splitlines())
    assert r.stdout.strip() == f"{n} lines, 0 differ"


def test_masked_cases_fixture_is_the_gpu_tests_table():
    """tests/golden/attn_plan_masked_cases.txt against tests/attn_mask_cases.py, the table tests/test_attention_mask_gpu.py runs: the same cases in
    the same order, every masked one on k_attn.hip ("F") with the wave count plan_flash's rule gives for its shape, under all 80 option variants, with
    one key slice (no "/S"); and the table reaches all eight masked instances -- head dims 40, 64, 80, 160, each 4-wave and 8-wave."""
    import attn_mask_cases as A
    lines = [ln for ln in MASKED_FIXTURE.read_text().splitlines() if ln and not ln.startswith("#")]
    want = [f"{A.plan_header(c, True)}: F{A.waves(c)}*80" for c in A.MASKED]
    assert lines[:len(want)] == want
    assert [ln.split(":")[0] for ln in lines[len(want):]] == [A.plan_header(c, False) for c in A.UNMASKED_BF16]
    assert {(c.d, A.waves(c)) for c in A.MASKED} == {(d, w) for d in (40, 64, 80, 160) for w in (4, 8)}
    assert all(A.waves(c) == 4 for c in A.WAVE4) and all(A.waves(c) == 8 for c in A.WAVE8) and A.waves(A.CLIP_TINY) == 8
    assert set(A.REDUCED) <= set(A.WAVE4 + A.WAVE8) and {(c.d, A.waves(c)) for c in A.REDUCED} == {(40, 4), (64, 4), (80, 4), (160, 4), (64, 8)}
    assert all(A.KV_TILE[c.d] == (32 if c.d == 160 else 64) for c in A.MASKED)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_planner_sends_masked_test_shapes_to_their_instances(tmp_path):
    """the planner itself, over the cases the fixture names: a shape of the GPU file that fell back to the other workgroup form would leave its test
    green and vacuous"""
    exe = _build(tmp_path)
    r = subprocess.run([str(exe), "--replay", str(MASKED_FIXTURE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    n = len([ln for ln in MASKED_FIXTURE.read_text().splitlines() if ln and not ln.startswith("#")])
    assert n > 0 and r.stdout.strip() == f"{n} cases, 0 differ"
