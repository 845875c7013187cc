"""The pair planner (csrc/gemm_plan.cpp plan_gemm_pair: how many k tiles a slice of a paired launch holds -- a ResBlock's 1x1 shortcut riding on extra
K slices of conv_out's split-K launch) is host-only C++.  g++ builds it with tests/san/gemm_pair_plan_main.cpp under -fsanitize=address,undefined -- a
stand-alone program, nothing loaded into python -- and the driver checks, for the batch-1 model's ten shortcut pairs and a sweep of shapes, forced tiles and
forced slice counts: no empty slice, no more rounds of 256 workgroups than conv_out alone, the tile plan_gemm gives conv_out, "do not pair" and a measured kt
honoured from the pairs table.  plan_gemm itself must be untouched: tests/golden/gemm_plan_choices.txt replays unchanged."""
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

# (M, N, Kaux) of the shortcut GEMMs of one batch-1 UNet forward (two CFG samples); conv_out is M, N, 9 N
PAIRS = [(8192, 320, 640), (8192, 320, 960), (2048, 640, 960), (2048, 640, 1280), (2048, 640, 1920), (2048, 640, 320),
         (512, 1280, 1920), (512, 1280, 2560), (512, 1280, 640), (128, 1280, 2560)]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pair_plan") / "gemm_pair_plan"
    r = subprocess.run(SAN + [str(ROOT / "tests" / "san" / "gemm_pair_plan_main.cpp"), str(CSRC / "gemm_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def test_every_promise_holds_over_the_sweep(driver_output):
    m = re.search(r"^(\d+) cases, (\d+) bad$", driver_output, flags=re.M)
    assert m and int(m.group(1)) > 5000 and int(m.group(2)) == 0, driver_output[-500:]


def test_model_pairs(driver_output):
    """one line per pair of the model; a paired one names its slices, and every one that has no '0' row in the table pairs (conv_out is split at every level)"""
    table = {}
    for ln in (PKG / "tuning" / "gfx950_fp32_pairs.txt").read_text().split():
        if "=" in ln and not ln.startswith("#"):
            key, val = ln.split("=")
            table[key] = tuple(int(v) for v in val.split(","))
    lines = {ln.split()[1]: ln for ln in driver_output.splitlines() if ln.startswith("pair ")}
    for M, N, ka in PAIRS:
        key = f"{M},{N},{9 * N}+{ka}"
        assert key in lines, key
        ln = lines[key]
        if key in table and table[key][1] == 0:
            assert " none " in ln, ln
            continue
        m = re.search(r"cfg=(\d+) kt=(\d+) main=(\d+) aux=(\d+) rounds=(\d+)/(\d+)", ln)
        assert m, ln
        cfg, kt, sm, sa, r_pair, r_today = map(int, m.groups())
        ktm, kta = 9 * N // 32, ka // 32
        assert 300 <= cfg <= 308
        assert sm == -(-ktm // kt) and sa == -(-kta // kt) and (sm - 1) * kt < ktm and (sa - 1) * kt < kta      # no empty slice, every k tile once
        assert r_pair <= r_today
        if key in table:
            assert (cfg, kt) == table[key]


def test_pairs_table_is_compiled_in():
    """build.py turns tuning/gfx950_fp32_pairs.txt into csrc/tuning_table_pairs.inc like the other tables; the committed file matches"""
    from stable_diffusion_burn_amd import build
    before = (CSRC / "tuning_table_pairs.inc").read_text()
    build.gen_tuning_table()
    assert (CSRC / "tuning_table_pairs.inc").read_text() == before
    rows = [ln for ln in (PKG / "tuning" / "gfx950_fp32_pairs.txt").read_text().split() if "=" in ln and not ln.startswith("#")]
    assert before.count("{") == len(rows)
    for ln in rows:
        assert re.fullmatch(r"\d+,\d+,\d+\+\d+=30[0-8],\d+", ln), ln


def test_plan_gemm_is_unchanged(tmp_path):
    exe = tmp_path / "gemm_plan"
    r = subprocess.run(SAN + [str(ROOT / "tests" / "san" / "gemm_plan_main.cpp"), str(CSRC / "gemm_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(FIXTURE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip() == f"{len(FIXTURE.read_text().splitlines())} lines, 0 differ"
