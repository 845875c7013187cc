"""The pair planner (csrc/gemm_plan.cpp plan_gemm_pair) for Linear main problems: the tail of a fp32 transformer block, mlp_lin on the folded weight (K = 4C) carrying
proj_out (K = C) on extra K slices (Engine::linear_pair).  g++ builds it with tests/san/linear_pair_plan_main.cpp under -fsanitize=address,undefined -- a stand-alone
program, nothing loaded into python -- and the driver checks, for the batch-1 model's four tails and a sweep of Linear shapes, forced tiles and forced slice counts,
the promises the ResBlock pairs hold (tests/test_gemm_pair_plan_cpu.py): no empty slice, no more rounds of 256 workgroups than mlp_lin alone, plan_gemm's tile, "do not
pair" and a measured (cfg, kt) honoured from the pairs table.  plan_gemm itself must be untouched: tests/golden/gemm_plan_choices.txt replays unchanged."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "stable_diffusion_burn_amd"
CSRC = PKG / "csrc"
FIXTURE = ROOT / "tests" / "golden" / "gemm_plan_choices.txt"
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

# (rows, C) of the transformer tails of one batch-1 UNet forward (two CFG samples): the pair is rows, C, 4C + C
PAIRS = [(8192, 320), (2048, 640), (512, 1280), (128, 1280)]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _table():
    table = {}
    for ln in (PKG / "tuning" / "gfx950_fp32_pairs.txt").read_text().split():
        if "=" in ln and not ln.startswith("#"):
            key, val = ln.split("=")
            table[key] = tuple(int(v) for v in val.split(","))
    return table


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("linear_pair_plan") / "linear_pair_plan"
    r = subprocess.run(SAN + [str(ROOT / "tests" / "san" / "linear_pair_plan_main.cpp"), str(CSRC / "gemm_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def test_every_promise_holds_over_the_sweep(driver_output):
    m = re.search(r"^(\d+) cases, (\d+) bad$", driver_output, flags=re.M)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) == 0, driver_output[-500:]


def test_model_tails(driver_output):
    """one line per tail of the model; a paired one names its slices; a table row is honoured -- its (cfg, kt) taken as measured, a 0 row not paired"""
    table = _table()
    lines = {ln.split()[1]: ln for ln in driver_output.splitlines() if ln.startswith("pair ")}
    for M, C in PAIRS:
        key = f"{M},{C},{4 * C}+{C}"
        assert key in lines, key
        ln = lines[key]
        if key in table and table[key][1] == 0:
            assert " none " in ln, ln
            continue
        m = re.search(r"cfg=(\d+) kt=(\d+) main=(\d+) aux=(\d+) rounds=(\d+)/(\d+)", ln)
        assert m, ln
        cfg, kt, sm, sa, r_pair, r_today = map(int, m.groups())
        ktm, kta = 4 * C // 32, C // 32
        assert 300 <= cfg <= 308
        assert sm == -(-ktm // kt) and sa == -(-kta // kt) and (sm - 1) * kt < ktm and (sa - 1) * kt < kta      # no empty slice, every k tile once
        if key in table:
            assert (cfg, kt) == table[key]
        else:
            assert r_pair <= r_today


def test_table_rows_are_well_formed_and_compiled_in():
    from stable_diffusion_burn_amd import build
    before = (CSRC / "tuning_table_pairs.inc").read_text()
    build.gen_tuning_table()
    assert (CSRC / "tuning_table_pairs.inc").read_text() == before
    for key, (cfg, kt) in _table().items():
        assert re.fullmatch(r"\d+,\d+,\d+\+\d+", key) and 300 <= cfg <= 308 and kt >= 0, (key, cfg, kt)
        assert f'"{key}"' in before


def test_plan_gemm_is_unchanged(tmp_path):
    exe = tmp_path / "gemm_plan"
    r = subprocess.run(SAN + [str(ROOT / "tests" / "san" / "gemm_plan_main.cpp"), str(CSRC / "gemm_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(FIXTURE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip() == f"{len(FIXTURE.read_text().splitlines())} lines, 0 differ"
