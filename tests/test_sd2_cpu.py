"""Host side of the SD 2.x variant: the planner's d = 64 gate (option attn_d64), the v-prediction rewrite of the samplers' coefficient
tables, the checkpoint key rule against tests/golden/sd2_ckpt_keys.txt, the writer's fused in_proj, the family check and the configuration's refusals.  No GPU."""
import ctypes as C
import json
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ksampler_ref as K
import sd2_ref as S2
from oracle import sd_oracle as O

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "stable_diffusion_burn_amd" / "csrc"
PLAN_FIXTURE = ROOT / "tests" / "golden" / "attn_plan_choices.txt"
KEYS_FIXTURE = ROOT / "tests" / "golden" / "sd2_ckpt_keys.txt"
ERR_INVALID, ERR_WEIGHTS, ERR_UNSUPPORTED = -1, -3, -5
CUS = 256


@pytest.fixture(scope="module")
def sdmi():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)
    import stable_diffusion_burn_amd as pkg
    return pkg


# ---- planner ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """cases [(attn_d64, bf16, mask, aligned, d, n, h, q, k)] -> [(fixture-format line, default-option plan or None)]"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("attn_plan_d64")
    exe = tmp / "attn_plan_d64"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        str(ROOT / "tests" / "san" / "attn_plan_d64_main.cpp"), str(CSRC / "attn_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        path = tmp / "cases.txt"
        path.write_text("".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases))
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = []
        for ln in r.stdout.splitlines():
            line, _, detail = ln.partition(" | ")
            f = detail.split()
            out.append((line, None if f[0].startswith("E") else {"kernel": f[0], "waves": int(f[1]), "q_rows": int(f[2]), "kv_tile": int(f[3]), "kv_splits": int(f[4])}))
        assert len(out) == len(cases)
        return out
    return run


def _fixture_grid_d64():
    """the d = 64 lines of the fixture's two grid sections (the later sections repeat headers with other flags): {header: line}"""
    lines, section = {}, None
    for ln in PLAN_FIXTURE.read_text().splitlines():
        if ln.startswith("#"):
            section = ln
            continue
        if section in ("# grid fp32", "# grid bf16") and " d64 " in ln:
            lines[ln.split(":")[0]] = ln
    return lines


def _flash_line(bf16, n, h, q, k):
    """what the planner gives a d = 64 call on k_attn.hip, restated from csrc/attn_plan.cpp (plan_flash, plan_kv_splits) in the fixture's format; checked below
    against the fixture's own d = 64 lines before it is used for head counts the fixture does not have"""
    wg = lambda rows: -(-q // rows) * n * h     # noqa: E731
    w = 8 if 2 * wg(128) >= 3 * CUS else 4
    if bf16:
        return f"bf16 d64 n{n} h{h} q{q} k{k}: F{w}*20"
    tiles = -(-k // 64)
    toks = []
    for _split in (1, 0):
        for kv in (0, 1, 2, 8, 1000):
            if kv == 1:
                s = 1
            elif kv > 1:
                s = min(kv, max(1, tiles))
            else:
                s = max(1, min(CUS // wg(64) if 0 < wg(64) <= CUS // 2 else 1, min(tiles // 2, 8)))
            toks += [f"F{w}" + (f"/{s}" if s > 1 else "")] * 8
    folded, prev, count = [], None, 0
    for t in toks + [None]:
        if t == prev:
            count += 1
            continue
        if prev is not None:
            folded.append(prev + (f"*{count}" if count > 1 else ""))
        prev, count = t, 1
    return f"f32 d64 n{n} h{h} q{q} k{k}: " + " ".join(folded)


ISSUE_GRID = [(n, h, q, k) for n in (1, 2) for h in (5, 20) for q in (64, 1024, 4096) for k in sorted({77, q})]


def test_attn_d64_off_is_the_recorded_planner(plan):
    """option 0 (AttnPlanOpts' default): every d = 64 line of the fixture's grid is reproduced with the new table rows in place, and the restatement of the
    k_attn.hip rule agrees with those lines"""
    fix = _fixture_grid_d64()
    assert len(fix) == 2 * 4 * 2 * 5 * 4
    cases, want = [], []
    for header, line in fix.items():
        st, _, n, h, q, k = header.split()
        cases.append((0, st == "bf16", 0, 1, 64, int(n[1:]), int(h[1:]), int(q[1:]), int(k[1:])))
        want.append(line)
        assert _flash_line(st == "bf16", *cases[-1][5:]) == line, header
    got = plan(cases)
    assert [g[0] for g in got] == want
    assert all(g[1]["kernel"] == "F" for g in got)


def test_attn_d64_off_on_the_sd2_head_counts(plan):
    """... and with it off the SD 2.x shapes (5 / 20 heads) get what the fixture's rule gives d = 64: k_attn.hip, masked or not, aligned or not, fp32 and bf16"""
    cases = [(0, bf16, mask, aligned, 64, n, h, q, k) for n, h, q, k in ISSUE_GRID for bf16, mask, aligned in ((0, 0, 1), (0, 0, 0), (1, 0, 1))]
    for c, (line, p) in zip(cases, plan(cases)):
        assert line == _flash_line(c[1], *c[5:]), c
        assert p["kernel"] == "F" and p["q_rows"] == 16 * p["waves"] and p["kv_tile"] == 64
    masked = [(0, 0, 1, 1, 64, n, h, q, k) for n, h, q, k in ISSUE_GRID]
    for c, (line, p) in zip(masked, plan(masked)):
        w = _flash_line(True, *c[5:]).split("F")[1][0]
        assert line.endswith(f": F{w}*80") and p["kernel"] == "F" and p["kv_splits"] == 1, c


def test_attn_d64_on(plan):
    fp32 = [(1, 0, 0, 1, 64, n, h, q, k) for n, h, q, k in ISSUE_GRID]
    for c, (line, p) in zip(fp32, plan(fp32)):
        toks = line.split(": ")[1].split()
        n_split = sum(int(t.split("*")[1]) if "*" in t else 1 for t in toks if t.startswith("S"))
        assert n_split == 40 and toks[0].startswith("S"), (c, line)          # the 40 variants with attn_split = 1 come first; the others stay on k_attn.hip
        assert p["kernel"] == "S" and p["waves"] in (4, 8) and p["q_rows"] == 32 * p["waves"] and p["kv_tile"] == 64, (c, p)
        n, h, q, k = c[5:]
        tiles = -(-k // 64)
        assert 1 <= p["kv_splits"] <= max(1, min(8, tiles // 2)), (c, p)     # plan_kv_splits' bounds: at least two tiles per slice, at most 8
    # attn_split = 0 under attn_d64 = 1 is attn_d64 = 0: the second half of the line
    off = plan([(0,) + c[1:] for c in fp32])
    for (on_line, _), (off_line, _) in zip(plan(fp32), off):
        assert _unfold(on_line)[40:] == _unfold(off_line)[40:]
    # masked (CLIP) and unaligned calls stay on k_attn.hip, with the plan they had
    for mask, aligned in ((1, 1), (0, 0)):
        stay = [(1, 0, mask, aligned, 64, n, h, q, k) for n, h, q, k in ISSUE_GRID]
        for (on_line, p), (off_line, p0) in zip(plan(stay), plan([(0,) + c[1:] for c in stay])):
            assert on_line == off_line and p == p0 and p["kernel"] == "F"
    bf16 = [(1, 1, 0, 1, 64, n, h, q, k) for n, h, q, k in ISSUE_GRID]
    for c, (line, p) in zip(bf16, plan(bf16)):
        toks = _unfold(line)
        assert all(t[0] == "B" and "." not in t for t in toks[:10]) and all(t[0] == "F" for t in toks[10:]), (c, line)   # attn_bf16 = 1: QR = 1 forms only
        assert p["kernel"] == "B" and p["waves"] in (2, 4, 8) and p["q_rows"] == 32 * p["waves"] and p["kv_tile"] == 64 and p["kv_splits"] == 1
        n, h, q, k = c[5:]
        fills = lambda rows: -(-q // rows) * n * h >= CUS      # noqa: E731
        assert p["waves"] == (8 if fills(256) else 4 if fills(128) else 2), (c, p)


def _unfold(line):
    out = []
    for t in line.split(": ")[1].split():
        tok, _, cnt = t.partition("*")
        out += [tok] * (int(cnt) if cnt else 1)
    return out


def test_attn_d64_level_2_is_the_measured_rule(plan):
    """2 = 1 minus the fp32 calls the interleaved A/B measured slower on k_attn_split.hip (profiles/r13a_attn_d64_ab.txt): k_attn.hip's 64-row workgroups fit the CUs in
    one round and walk a handful of key tiles.  The full-width SD 2.x shapes at batch 1 (n = 2): the 256-token level stays on k_attn.hip, the others move; bf16: 2 is 1."""
    real = [(2, 5, 4096), (2, 10, 1024), (2, 20, 256), (2, 20, 64), (4, 20, 256), (8, 20, 256)]
    cases = [(2, 0, 0, 1, 64, n, h, q, k) for n, h, q in real for k in (q, 77)]
    got = {c[5:]: p["kernel"] for c, (_, p) in zip(cases, plan(cases))}
    assert got == {(2, 5, 4096, 4096): "S", (2, 5, 4096, 77): "S", (2, 10, 1024, 1024): "S", (2, 10, 1024, 77): "S", (2, 20, 256, 256): "F", (2, 20, 256, 77): "F",
                   (2, 20, 64, 64): "S", (2, 20, 64, 77): "S", (4, 20, 256, 256): "S", (4, 20, 256, 77): "S", (8, 20, 256, 256): "S", (8, 20, 256, 77): "S"}
    # where 2 keeps k_attn.hip it gives exactly the plan of 0; elsewhere exactly the plan of 1 -- over the issue's grid and a wider one, under every option variant
    grid = ISSUE_GRID + [(n, h, q, k) for n in (1, 2, 8) for h in (2, 20) for q in (100, 256, 512, 2085) for k in (77, 300, q)]
    two, one, zero = (plan([(f, 0, 0, 1, 64) + g for g in grid]) for f in (2, 1, 0))
    kept = 0
    for g, (l2, _), (l1, _), (l0, _) in zip(grid, two, one, zero):
        t2, t1, t0 = _unfold(l2), _unfold(l1), _unfold(l0)
        assert all(a in (b, c) for a, b, c in zip(t2, t1, t0)), g
        assert g[2] > 64 or t2 == t1, g
        kept += t2[0][0] == "F"
    assert 0 < kept < len(grid)
    bf = [(f, 1, 0, 1, 64) + g for f in (2, 1) for g in grid]
    res = plan(bf)
    assert [r for r in res[:len(grid)]] == [r for r in res[len(grid):]]


def test_attn_d64_leaves_the_other_head_dims_alone(plan):
    cases = [(f, bf16, 0, 1, d, 2, 8, q, k) for f in (0, 1) for bf16 in (0, 1) for d in (40, 80, 160) for q in (64, 4096) for k in (77, q)]
    got = plan(cases)
    half = len(cases) // 2
    assert got[:half] == got[half:]


# ---- v-prediction: the rewritten tables ---------------------------------------------------------------------------------------------------------------
def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max()
    bound = 1e-6 * max(1.0, np.abs(b).max())
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("n_steps", [1, 2, 7])
@pytest.mark.parametrize("kind,eta", [("ddim", 0.0), ("ddim", 1.0), ("dpmpp_2m", 0.0), ("plms", 0.0)])
def test_v_table_identity_sampler(sdmi, kind, eta, n_steps):
    """one step of the v table on (x, v(x, e)) is the eps table's step on (x, e), history pushed included; every other column is untouched"""
    from stable_diffusion_burn_amd import synthetic as syn
    a = syn.alphas_cumprod()
    ts, step = O.ddim_timesteps(n_steps, len(a))
    te = sdmi.sampler_coefs(kind, eta, a, ts, step)
    assert np.array_equal(te, sdmi.sampler_coefs(kind, eta, a, ts, step, prediction="eps"))
    tv = sdmi.sampler_coefs(kind, eta, a, ts, step, prediction="v")
    assert tv.shape == te.shape == (len(ts), 8) and not np.array_equal(tv, te)
    assert np.array_equal(tv[:, 2:6], te[:, 2:6])
    g = np.random.default_rng(n_steps * 10 + len(kind))
    for j, t in enumerate(ts):
        sa, sb = math.sqrt(float(a[t])), math.sqrt(1.0 - float(a[t]))
        x, e, z = g.standard_normal(64), g.standard_normal(64), g.standard_normal(64)
        hist = g.standard_normal((3, 64))
        v = S2.v_of(x, e, sa, sb)
        _close(sa * v + sb * x, e, "eps from v")
        res = {}
        for name, (cx, ce, h1, h2, h3, cz, qx, qe), out in (("eps", te[j], e), ("v", tv[j], v)):
            res[name] = (cx * x + ce * out + h1 * hist[0] + h2 * hist[1] + h3 * hist[2] + cz * z, qx * x + qe * out)
        _close(res["v"][0], res["eps"][0], f"{kind} eta={eta} step {j}: x'")
        _close(res["v"][1], res["eps"][1], f"{kind} eta={eta} step {j}: q")


@pytest.mark.parametrize("n_steps", [1, 2, 7])
@pytest.mark.parametrize("schedule", K.SCHEDULES)
@pytest.mark.parametrize("kind", K.KINDS)
def test_v_table_identity_ksampler(sdmi, kind, schedule, n_steps):
    from stable_diffusion_burn_amd import synthetic as syn
    a = syn.alphas_cumprod()
    for eta in ((0.0, 1.0) if kind in K.ETA_KINDS else (0.0,)):
        pe = sdmi.ksampler_plan(kind, a, n_steps, schedule=schedule, eta=eta)
        assert np.array_equal(pe, sdmi.ksampler_plan(kind, a, n_steps, schedule=schedule, eta=eta, prediction="eps"))
        pv = sdmi.ksampler_plan(kind, a, n_steps, schedule=schedule, eta=eta, prediction="v")
        from stable_diffusion_burn_amd.pipeline import KSAMPLER_PLAN_COLUMNS as cols
        same = [cols.index(c) for c in ("step", "stage", "t", "sigma", "h1", "cz", "cz2", "a_end")]
        assert pv.shape == pe.shape and np.array_equal(pv[:, same], pe[:, same]) and not np.array_equal(pv, pe)
        g = np.random.default_rng(n_steps * 100 + len(kind) * 10 + len(schedule))
        for j in range(len(pe)):
            sigma = pe[j, 3]
            sa, sb = 1.0 / math.sqrt(1.0 + sigma * sigma), sigma / math.sqrt(1.0 + sigma * sigma)
            x, e, q1, z, z2 = (g.standard_normal(64) for _ in range(5))
            v = S2.v_of(x, e, sa, sb)
            res = {}
            for name, row, out in (("eps", pe[j], e), ("v", pv[j], v)):
                _, _, _, _, cx, ce, h1, cz, cz2, qx, qe, _ = row
                res[name] = (cx * x + ce * out + h1 * q1 + cz * z + cz2 * z2, qx * x + qe * out)
            _close(res["v"][0], res["eps"][0], f"{kind} {schedule} eta={eta} row {j}: x'")
            _close(res["v"][1], res["eps"][1], f"{kind} {schedule} eta={eta} row {j}: q")


def test_prediction_argument_is_checked(sdmi):
    from stable_diffusion_burn_amd import synthetic as syn
    from stable_diffusion_burn_amd._capi import SdmiSampler, load_library
    a = syn.alphas_cumprod()
    with pytest.raises(ValueError):
        sdmi.sampler_coefs("ddim", 0.0, a, [999], 1000, prediction="x0")
    with pytest.raises(ValueError):
        sdmi.ksampler_plan("euler", a, 3, prediction="x0")
    lib = load_library()
    s, out, ts = SdmiSampler(), np.zeros(8), np.array([999], np.int32)
    args = (C.byref(s), a.ctypes.data_as(C.POINTER(C.c_float)), a.size, ts.ctypes.data_as(C.POINTER(C.c_int32)), 1, 1000)
    assert lib.sdmi_sampler_coefs_ex(*args, 2, out.ctypes.data_as(C.POINTER(C.c_double))) == ERR_INVALID
    assert lib.sdmi_sampler_coefs_ex(*args, 1, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert lib.sdmi_set_prediction(None, 1) < 0      # a null context is an error, not a crash


# ---- checkpoint keys ------------------------------------------------------------------------------------------------------------------------------------
def _key_rows():
    rows = [ln.split("\t") for ln in KEYS_FIXTURE.read_text().splitlines()]
    assert all(len(r) == 5 for r in rows)
    return [(d, k, tuple(int(v) for v in s.split(",")), t == "T", None if p == "-" else int(p)) for d, k, s, t, p in rows]


def test_sd2_key_map_reproduces_the_fixture(sdmi):
    import sys
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    try:
        import gen_sd2_ckpt_keys as G
    finally:
        sys.path.pop(0)
    rows = _key_rows()
    assert [(d, k, tuple(s), f == "T", None if p == "-" else int(p)) for d, k, s, f, p in G.rows()] == rows, "the committed fixture is not what its rule writes"
    assert KEYS_FIXTURE.stat().st_size < 256 * 1024 and len({r[0] for r in rows}) == len(rows)
    for dump, key, shape, transposed, part in rows:
        assert sdmi.checkpoint_key(dump, variant=1, with_slice=True) == (key, transposed, part), dump
        assert sdmi.checkpoint_key(dump, variant=1) == (key, transposed)
        if not dump.startswith("clip/"):
            assert sdmi.checkpoint_key(dump) == (key, transposed), dump        # UNet and VAE: SD v1's keys
    fused = [r for r in rows if r[4] is not None]
    assert len(fused) == 23 * 6 and {r[1].rsplit(".", 1)[1] for r in fused} == {"in_proj_weight", "in_proj_bias"}
    whole = [r[1] for r in rows if r[4] is None]
    assert len(set(whole)) == len(whole), "two dump names share a checkpoint key"
    by_dump = {r[0]: r for r in rows}
    assert by_dump["clip/blocks/22/attn/value/weight"][1:] == ("cond_stage_model.model.transformer.resblocks.22.attn.in_proj_weight", (3072, 1024), True, 2)
    assert by_dump["clip/position_embedding/weight"][1:] == ("cond_stage_model.model.positional_embedding", (77, 1024), False, None)
    assert by_dump["unet/middle_block/transformer/proj_out/weight"][2] == (1280, 1280)
    assert by_dump["unet/middle_block/transformer/transformer/attn2/value/weight"][2] == (1280, 1024)
    assert sdmi.checkpoint_key("clip/blocks/3/attn/query/weight", with_slice=True) == ("cond_stage_model.transformer.text_model.encoder.layers.3.self_attn.q_proj.weight", True, None)
    for bad in ("clip/position_embedding/bias", "clip/blocks/0/attn/query/eps", "clip/blocks/0/attn/query", "clip/token_embedding/bias"):
        with pytest.raises(sdmi.SdmiError) as ei:
            sdmi.checkpoint_key(bad, variant=1)
        assert ei.value.status == ERR_INVALID
    with pytest.raises(sdmi.SdmiError):
        sdmi.checkpoint_key("unet/conv_out/weight", variant=2)


def _read_safetensors(path):
    raw = Path(path).read_bytes()
    hlen = int.from_bytes(raw[:8], "little")
    header = json.loads(raw[8:8 + hlen])
    out = {}
    for key, m in header.items():
        if key == "__metadata__":
            continue
        assert m["dtype"] == "F32"
        b, e = m["data_offsets"]
        out[key] = np.frombuffer(raw[8 + hlen + b:8 + hlen + e], np.float32).reshape(m["shape"])
    return out


def _tiny_specs(c=8):
    specs = [("alphas_cumprod", (10,)), ("unet/middle_block/transformer/proj_in/weight", (c, c, 1, 1)), ("unet/middle_block/transformer/proj_in/bias", (c,)),
             ("unet/middle_block/transformer/transformer/attn2/key/weight", (12, c)), ("autoencoder/decoder/mid/attn/proj_out/weight", (c, c, 1, 1)),
             ("clip/layer_norm/weight", (c,)), ("clip/position_embedding/weight", (5, c)), ("clip/blocks/0/attn/out/weight", (c, c))]
    for part in ("query", "key", "value"):
        specs += [(f"clip/blocks/0/attn/{part}/weight", (c, c)), (f"clip/blocks/0/attn/{part}/bias", (c,))]
    return specs


def test_writer_fuses_in_proj_and_family_is_detected(sdmi, tmp_path):
    from stable_diffusion_burn_amd import weights as W
    specs = _tiny_specs()
    g = np.random.default_rng(5)
    data = {name: g.standard_normal(shape).astype(np.float32) for name, shape in specs}
    get = lambda name, shape: data[name]      # noqa: E731
    v2, v1 = tmp_path / "v2.safetensors", tmp_path / "v1.safetensors"
    W.write_checkpoint_safetensors(v2, specs, get, data["alphas_cumprod"], variant=1)
    W.write_checkpoint_safetensors(v1, specs, get, data["alphas_cumprod"])
    t2, t1 = _read_safetensors(v2), _read_safetensors(v1)
    pre = "cond_stage_model.model.transformer.resblocks.0.attn."
    assert t2[pre + "in_proj_weight"].shape == (24, 8) and t2[pre + "in_proj_bias"].shape == (24,)
    for part, (w, b) in enumerate(zip(np.split(t2[pre + "in_proj_weight"], 3), np.split(t2[pre + "in_proj_bias"], 3))):
        name = ("query", "key", "value")[part]
        np.testing.assert_array_equal(w, data[f"clip/blocks/0/attn/{name}/weight"].T)      # torch's [out, in]
        np.testing.assert_array_equal(b, data[f"clip/blocks/0/attn/{name}/bias"])
    np.testing.assert_array_equal(t2[pre + "out_proj.weight"], data["clip/blocks/0/attn/out/weight"].T)
    np.testing.assert_array_equal(t2["cond_stage_model.model.positional_embedding"], data["clip/position_embedding/weight"])
    pj = "model.diffusion_model.middle_block.1.proj_in.weight"
    assert t2[pj].shape == (8, 8) and t1[pj].shape == (8, 8, 1, 1) and np.array_equal(t2[pj], t1[pj][:, :, 0, 0])
    assert t2["first_stage_model.decoder.mid.attn_1.proj_out.weight"].shape == (8, 8, 1, 1)      # the VAE's stays a convolution
    np.testing.assert_array_equal(t2["model.diffusion_model.middle_block.1.transformer_blocks.0.attn2.to_k.weight"], data["unet/middle_block/transformer/transformer/attn2/key/weight"].T)
    assert "cond_stage_model.transformer.text_model.encoder.layers.0.self_attn.q_proj.weight" in t1 and len(t1) == len(t2) + 4
    assert sdmi.safetensors_model_family(v2) == "sd2" and sdmi.safetensors_model_family(v1) == "sd1"
    other = tmp_path / "unet_only.safetensors"
    W.write_safetensors(other, {k: v for k, v in t2.items() if k.startswith("model.diffusion_model.")})
    assert sdmi.safetensors_model_family(other) is None
    with pytest.raises(sdmi.SdmiError):
        sdmi.safetensors_model_family(tmp_path / "missing.safetensors")
    with pytest.raises(ValueError, match="query, key and value"):
        W.write_checkpoint_safetensors(tmp_path / "bad.safetensors", [s for s in specs if "attn/key/" not in s[0] or not s[0].startswith("clip/")], get, None, variant=1)


# ---- configuration ----------------------------------------------------------------------------------------------------------------------------------------
def test_variant_refusals(sdmi):
    """checked before the device is looked at, so a machine without one sees them too"""
    from stable_diffusion_burn_amd._capi import SdmiConfig, load_library
    lib = load_library()

    def create(**kw):
        cfg = SdmiConfig()
        assert lib.sdmi_default_config(C.byref(cfg)) == 0
        assert cfg.variant == 0 and cfg.control_hint_ch == 0
        for k, v in kw.items():
            setattr(cfg, k, v)
        ctx = C.c_void_p()
        st = lib.sdmi_create(C.byref(ctx), C.byref(cfg))
        if st == 0:
            lib.sdmi_destroy(ctx)
        return st, lib.sdmi_last_error().decode()
    for bad in (2, -1, 7):
        st, msg = create(variant=bad)
        assert st == ERR_INVALID and "variant" in msg, (bad, msg)
    st, msg = create(variant=1, model_channels=96)
    assert st == ERR_INVALID and "64" in msg
    st, msg = create(variant=1, control_hint_ch=3)
    assert st == ERR_UNSUPPORTED and "control_hint_ch" in msg
    st, msg = create(variant=1, n_head=0)        # n_head is ignored on a variant context: not this refusal
    assert "n_head" not in msg
    st, msg = create(variant=0, n_head=0)
    assert st == ERR_INVALID and "n_head" in msg


def test_config_surface(sdmi):
    """ModelConfig.variant / sd_v2, the ctypes mirror, the header and the Rust shim say the same"""
    import re
    from stable_diffusion_burn_amd._capi import SIGNATURES, SdmiAttnPlan, SdmiConfig
    v2 = sdmi.ModelConfig.sd_v2()
    v1 = sdmi.ModelConfig.sd_v1_4()
    assert (v2.variant, v2.ctx_dim, v2.clip_layers, v2.clip_heads) == (1, 1024, 23, 16) and sdmi.ModelConfig.sd_v2(precision=1, clip=False).clip_layers == 0
    assert v1.variant == 0 and sdmi.ModelConfig(variant=1).variant == 1
    import dataclasses
    assert dataclasses.replace(v2, variant=0, ctx_dim=768, clip_layers=12, clip_heads=12) == v1
    assert C.sizeof(SdmiConfig) == 64 and C.sizeof(SdmiAttnPlan) == 32
    cfg = SdmiConfig()
    cfg.variant = 1
    assert cfg.reserved[1] == 1 and cfg.reserved[0] == 0
    header = (ROOT / "include" / "sdmi.h").read_text()
    body = header.split("typedef struct sdmi_config {")[1].split("} sdmi_config;")[0]
    fields = re.findall(r"^\s*int32_t (\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    assert fields[-2:] == ["control_hint_ch", "variant"] and len(fields) == 16
    rs = (ROOT / "ffi" / "sdmi.rs").read_text()
    for sym in ("sdmi_attention_plan", "sdmi_set_prediction", "sdmi_sampler_coefs_ex", "sdmi_ksampler_plan_ex", "sdmi_checkpoint_key_ex", "sdmi_safetensors_model_family"):
        assert re.search(r"\bfn\s+%s\b" % sym, rs), sym
        assert sym in SIGNATURES, sym
    assert "pub fn variant(&self)" in rs and "pub struct SdmiAttnPlan" in rs
    doc = (ROOT / "INTEGRATION.md").read_text()
    for word in ("variant", "sdmi_attention_plan", "sdmi_set_prediction", "attn_d64"):
        assert word in doc, word
