"""conv3x3(nearest_2x(x)) as four folded 2x2 phase convolutions (tests/upsample_phase_ref.py; csrc/kernels.hpp ConvGemm::phases), the parts that need no GPU:
the identity itself in fp64 against the oracle's two-step form, the output row map, and the host-only planner (csrc/gemm_plan.cpp plan_ups_phase) -- built with
tests/san/ups_phase_plan_main.cpp by plain g++ under -fsanitize=address,undefined, a stand-alone program, nothing loaded into python."""
import re
import shutil
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import upsample_phase_ref as P
from oracle import sd_oracle as O

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "stable_diffusion_burn_amd" / "csrc"
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

# (n, cin, h, w, cout)
IDENTITY_CASES = [(2, 32, 5, 7, 48), (1, 64, 1, 1, 32), (2, 8, 3, 2, 8)]


def _operands(case):
    n, cin, h, w, cout = case
    g = np.random.default_rng(zlib.crc32(repr((case, "ups_phase")).encode()))
    x = g.standard_normal((n, cin, h, w))
    wt = g.standard_normal((cout, cin, 3, 3)) / np.sqrt(9.0 * cin)
    b = g.standard_normal(cout)
    return x, wt, b


@pytest.mark.parametrize("case", IDENTITY_CASES)
def test_phase_form_equals_conv_of_the_upsampled_tensor_in_fp64(case):
    x, wt, b = _operands(case)
    ref = O.conv2d(O.upsample2x(torch.from_numpy(x)), (torch.from_numpy(wt), torch.from_numpy(b)), stride=1, padding=1).numpy()
    got = P.phase_conv(x, wt, b)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12, np.abs(got - ref).max()


def test_a_folded_weight_is_a_sum_of_1_2_or_4_taps():
    w = np.ones((1, 1, 3, 3))
    wf = P.fold_weights(w)
    for py in range(2):
        for px in range(2):
            rows = [1, 2] if py == 0 else [2, 1]
            cols = [1, 2] if px == 0 else [2, 1]
            assert np.array_equal(wf[py * 2 + px, 0, 0], np.outer(rows, cols))
    assert wf.sum() == 4 * 9      # every tap of every phase exactly once


def test_packed_phase_image_k_order():
    """channel slice outer, taps inner (a * 2 + b), 32 channels: the k order of the plane kernel"""
    g = np.random.default_rng(5)
    w = g.standard_normal((3, 64, 3, 3))
    wf, img = P.fold_weights(w), P.packed_phase_image(w)
    assert img.shape == (4, 3, 256)
    for ph, o, cs, a, b, ci in [(0, 0, 0, 0, 0, 0), (3, 2, 1, 1, 0, 31), (1, 1, 1, 0, 1, 7), (2, 0, 0, 1, 1, 16)]:
        assert img[ph, o, (cs * 4 + a * 2 + b) * 32 + ci] == wf[ph, o, cs * 32 + ci, a, b]


@pytest.mark.parametrize("nb,hs,ws", [(3, 5, 7), (2, 1, 1), (2, 3, 9), (1, 7, 1)])
def test_row_map_is_a_bijection(nb, hs, ws):
    m = nb * hs * ws
    rows = sorted(P.phase_row(i, ph, hs, ws) for ph in range(4) for i in range(m))
    assert rows == list(range(4 * m))
    # and it is the pixel it says: phase (py, px) of source pixel (y, x) of sample b
    for ph in range(4):
        for i in (0, m // 2, m - 1):
            r = P.phase_row(i, ph, hs, ws)
            b, rem = divmod(r, 4 * hs * ws)
            oy, ox = divmod(rem, 2 * ws)
            sb, srem = divmod(i, hs * ws)
            assert (b, oy, ox) == (sb, 2 * (srem // ws) + (ph >> 1), 2 * (srem % ws) + (ph & 1))


# ---- the planner -----------------------------------------------------------------------------------------------------------------------------------------------
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# (NB, C, Hs, Ws) of the six up-convolutions at the 64 x 64 latent, then at 72 x 88 and 40 x 40
LAYERS = [(2, 1280, 8, 8), (2, 1280, 16, 16), (2, 640, 32, 32), (1, 512, 64, 64), (1, 512, 128, 128), (1, 256, 256, 256),
          (2, 1280, 9, 11), (2, 1280, 18, 22), (2, 640, 36, 44), (1, 512, 72, 88), (1, 512, 144, 176), (1, 256, 288, 352),
          (2, 1280, 5, 5), (2, 1280, 10, 10), (2, 640, 20, 20), (1, 512, 40, 40), (1, 512, 80, 80), (1, 256, 160, 160)]
BM = {300: 256, 301: 256, 302: 128, 303: 128, 304: 128, 305: 64, 306: 64, 307: 64, 308: 128}
BN = {300: 160, 301: 128, 302: 256, 303: 160, 304: 128, 305: 64, 306: 128, 307: 320, 308: 64}


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ups_phase_plan") / "ups_phase_plan"
    r = subprocess.run(SAN + [str(ROOT / "tests" / "san" / "ups_phase_plan_main.cpp"), str(CSRC / "gemm_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


@needs_gxx
def test_every_promise_holds_over_the_sweep(driver_output):
    """no empty K slice, the slices cover every k tile once, no tile straddles a phase; ups_phase = 0, a stale fold, forced non-plane tiles, gemm_planes = 0 and
    gemm_f32s = 0 give today's plan; forced plane tiles and split counts are honoured by ups_phase = 1 only"""
    m = re.search(r"^(\d+) cases, (\d+) bad$", driver_output, flags=re.M)
    assert m and int(m.group(1)) > 3000 and int(m.group(2)) == 0, driver_output[-500:]


@needs_gxx
def test_model_layers(driver_output):
    lines = {(int(ln.split()[1]), ln.split()[2]): ln for ln in driver_output.splitlines() if ln.startswith("phase ")}
    table = {}
    for ln in (ROOT / "stable_diffusion_burn_amd" / "tuning" / "gfx950_fp32_phases.txt").read_text().split():
        if "=" in ln and not ln.startswith("#"):
            key, val = ln.split("=")
            table[key] = tuple(int(v) for v in val.split(","))
    assert len(table) == 6 and all(300 <= cfg <= 308 for cfg, _ in table.values()), table      # the six up-convolutions of the batch-1 headline
    for nb, c, hs, ws in LAYERS:
        key = f"{nb},{c},{hs},{ws}"
        forced, default = lines[(1, key)], lines[(2, key)]
        assert " take " in forced, forced                      # ups_phase = 1: wherever supported
        rows = nb * hs * ws
        row = table.get(f"{rows},{c},{4 * c}")
        if row is not None and row[1] > 0:
            assert f" take cfg={row[0]} splits={row[1]} " in default, default      # a measured row is taken as written
        elif rows < 256:
            assert default.endswith(" decline"), default      # unmeasured, one M tile per phase: the fold reads 16/9 of the weights of a launch near the weight-stream limit
        for ln in (forced, default):
            m = re.search(r"cfg=(\d+) splits=(\d+) kt=(\d+) tiles=(\d+)", ln)
            if not m:
                continue
            cfg, splits, kt, tiles = map(int, m.groups())
            ktt = c // 8
            assert splits == -(-ktt // kt) and (splits - 1) * kt < ktt, ln
            assert tiles == 4 * -(-rows // BM[cfg]) * -(-c // BN[cfg]), ln      # M tiles are counted per phase
    # the other sizes' smallest level has no measured row: it stays on today's launch
    assert lines[(2, "2,1280,9,11")].endswith(" decline") and lines[(2, "2,1280,5,5")].endswith(" decline")


@needs_gxx
def test_plan_gemm_is_unchanged(tmp_path):
    """the phase planner sits beside plan_gemm: the fixture of recorded choices replays unchanged"""
    fixture = ROOT / "tests" / "golden" / "gemm_plan_choices.txt"
    exe = tmp_path / "gemm_plan"
    r = subprocess.run(SAN + [str(ROOT / "tests" / "san" / "gemm_plan_main.cpp"), str(CSRC / "gemm_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(fixture)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip() == f"{len(fixture.read_text().splitlines())} lines, 0 differ"
