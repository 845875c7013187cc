"""Sigma-schedule samplers on the host (no GPU): sdmi_ksampler_sigmas / sdmi_sigma_to_t / sdmi_ksampler_plan -- the one implementation of the schedules and of the
seven samplers the engine applies -- against the textbook forms of tests/ksampler_ref.py, their identities with sdmi_sampler_coefs, where noise may appear, the
point of the feature on a solvable case, and argument validation."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import ksampler_ref as K
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

ROOT = Path(__file__).resolve().parents[1]
SDMI_OK, SDMI_ERR_INVALID = 0, -1
NEW_SYMBOLS = ["sdmi_set_ksampler", "sdmi_get_ksampler", "sdmi_multi_set_ksampler", "sdmi_ksampler_sigmas", "sdmi_sigma_to_t", "sdmi_ksampler_plan",
               "sdmi_op_timestep_embedding_f"]
KARRAS_10_T = [999, 916.284, 815.045, 687.153, 523.199, 327.147, 145.939, 40.857, 6.732, 0]
COL = {name: i for i, name in enumerate(("step", "stage", "t", "sigma", "cx", "ce", "h1", "cz", "cz2", "qx", "qe", "a_end"))}
CASES = [(kind, eta) for kind in K.KINDS for eta in ((0.0, 0.5, 1.0) if kind in K.ETA_KINDS else (0.0,))]


@pytest.fixture(scope="module")
def lib():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)  # hipcc cross-compiles gfx950 without a GPU
    from stable_diffusion_burn_amd import _capi
    return _capi.load_library()


@pytest.fixture(scope="module")
def alphas():
    return syn.alphas_cumprod()


def _plan(lib, kind, a, n, schedule="karras", strength=1.0, **kw):
    from stable_diffusion_burn_amd import ksampler_plan
    return ksampler_plan(kind, a, n, schedule=schedule, strength=strength, **kw)


def _sigmas(lib, a, n, schedule, **kw):
    from stable_diffusion_burn_amd import ksampler_sigmas
    return ksampler_sigmas("euler", a, n, schedule=schedule, **kw)


def _toy_predict(x, t, sigma):
    """tests/test_sampler_cpu.py's predictor at a float t (sqrt(1 - a) = sigma / sqrt(1 + sigma^2)): smooth, no closed-form trajectory"""
    return 0.8 * math.sin(1.3 * x + 0.002 * t) + 0.35 * x * sigma / math.sqrt(1.0 + sigma * sigma)


def _toy_noise(s, r):
    return math.sin(12.9898 * (s + 1) + 4.1 * r) * 1.7


# ---- 1. symbols ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_declared(lib):
    header = (ROOT / "include" / "sdmi.h").read_text()
    capi = (ROOT / "stable_diffusion_burn_amd" / "_capi.py").read_text()
    rust = (ROOT / "ffi" / "sdmi.rs").read_text()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(rf"\b{s}\s*\(", header), f"{s} is not declared in include/sdmi.h"
        assert f'"{s}"' in capi, f"{s} has no signature in _capi.py"
        assert re.search(rf"\bfn {s}\s*\(", rust), f"{s} is not declared in ffi/sdmi.rs"
    assert "typedef struct sdmi_ksampler" in header and "pub struct SdmiKSampler" in rust
    import stable_diffusion_burn_amd as pkg
    from stable_diffusion_burn_amd import sharding
    for name in ("ksampler_sigmas", "sigma_to_t", "ksampler_plan"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    for cls in (pkg.StableDiffusion, pkg.MultiStableDiffusion):
        assert callable(cls.set_ksampler)
    assert callable(pkg.StableDiffusion.get_ksampler) and callable(pkg.StableDiffusion.op_timestep_embedding_f) and callable(sharding.set_shard_ksampler)
    from stable_diffusion_burn_amd._capi import SdmiKSampler
    assert C.sizeof(SdmiKSampler) == 4 + 4 + 4 * 8 + 8 + 8 + 4 * 8   # the header's layout: no padding


# ---- 2. sigma <-> t --------------------------------------------------------------------------------------------------------------
def test_sigma_to_t_round_trips_the_table_and_is_monotone(lib, alphas):
    from stable_diffusion_burn_amd import sigma_to_t
    S = K.model_sigmas(alphas)
    assert abs(S[0] - 0.02917) < 1e-5 and abs(S[-1] - 14.6146) < 1e-4 and (np.diff(S) > 0).all()
    assert [sigma_to_t(alphas, float(s)) for s in S] == [float(j) for j in range(len(S))]
    grid = np.exp(np.linspace(math.log(S[0]), math.log(S[-1]), 4001))
    t = np.array([sigma_to_t(alphas, float(s)) for s in grid])
    assert (np.diff(t) >= 0).all() and t[0] == 0.0 and t[-1] == len(S) - 1
    for s in grid[::97]:
        assert abs(sigma_to_t(alphas, float(s)) - K.sigma_to_t(alphas, float(s))) <= 1e-9
    assert sigma_to_t(alphas, float(S[0]) / 2) == 0.0 and sigma_to_t(alphas, float(S[-1]) * 2) == len(S) - 1   # clamped outside the table


# ---- 3. schedules ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 10, 30, 1000])
@pytest.mark.parametrize("schedule", K.SCHEDULES)
def test_schedules(lib, alphas, schedule, n):
    S = K.model_sigmas(alphas)
    sg = _sigmas(lib, alphas, n, schedule)
    ref = K.sigmas(schedule, alphas, n)
    assert len(sg) == len(ref) and np.allclose(sg, ref, rtol=1e-12, atol=0.0)
    assert sg[0] == S[-1] and sg[-1] == 0.0 and (np.diff(sg) < 0).all()
    if schedule == "model":
        ts, _ = O.ddim_timesteps(n, len(alphas))
        assert len(sg) == len(ts) + 1 and np.array_equal(sg[:-1], S[ts])     # Q5: n = 3 runs 4 steps, n = 30 runs 31
        if n == 3:
            assert len(ts) == 4
        if n == 30:
            assert len(ts) == 31
    else:
        assert len(sg) == n + 1
        if n > 1:
            assert sg[-2] == S[0]


def test_karras_10_maps_to_the_stated_timesteps(lib, alphas):
    from stable_diffusion_burn_amd import sigma_to_t
    sg = _sigmas(lib, alphas, 10, "karras")
    got = [sigma_to_t(alphas, float(s)) for s in sg[:-1]]
    assert np.abs(np.array(got) - np.array(KARRAS_10_T, np.float64)).max() <= 1e-3, got
    assert np.allclose(_plan(lib, "euler", alphas, 10)[:, COL["t"]], got, rtol=0, atol=1e-12)


def test_sigma_bounds_and_rho(lib, alphas):
    sg = _sigmas(lib, alphas, 8, "karras", sigma_min=0.1, sigma_max=10.0, rho=5.0)
    assert np.allclose(sg, K.sigmas("karras", alphas, 8, rho=5.0, sigma_min=0.1, sigma_max=10.0), rtol=1e-12) and sg[0] == 10.0 and sg[-2] == 0.1
    assert np.array_equal(_sigmas(lib, alphas, 8, "karras", rho=0.0), _sigmas(lib, alphas, 8, "karras", rho=7.0))   # 0 = 7
    sg = _sigmas(lib, alphas, 8, "exponential", sigma_min=0.1, sigma_max=10.0)
    assert np.allclose(sg, K.sigmas("exponential", alphas, 8, sigma_min=0.1, sigma_max=10.0), rtol=1e-12)


# ---- 4. the plan, run as the kernel runs it, against the textbook loop ---------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5, 20])
@pytest.mark.parametrize("schedule", K.SCHEDULES)
@pytest.mark.parametrize("kind,eta", CASES)
def test_plan_matches_textbook_form(lib, alphas, kind, eta, schedule, n):
    rows = _plan(lib, kind, alphas, n, schedule, eta=eta)
    sg = K.sigmas(schedule, alphas, n)
    got = K.sample_plan(rows, 1.0, _toy_predict, _toy_noise)
    ref = K.sample_textbook(kind, eta, alphas, sg, 0, 1.0, _toy_predict, _toy_noise)
    assert abs(got - ref) <= 1e-12 * max(1.0, abs(ref)), f"{kind} eta={eta} {schedule} n={n}: plan {got!r} vs textbook {ref!r}"
    L = len(sg) - 1
    assert len(rows) == (2 * L - 1 if kind in K.TWO_STAGE else L)   # two evaluations on every step but the last
    assert rows[:, COL["step"]].tolist() == sorted(rows[:, COL["step"]].tolist()) and rows[-1, COL["step"]] == L - 1


@pytest.mark.parametrize("schedule", K.SCHEDULES)
@pytest.mark.parametrize("kind,eta", CASES)
def test_plan_matches_textbook_form_on_an_img2img_tail(lib, alphas, kind, eta, schedule):
    """history starts at the first step of the CALL; the noise index stays the full schedule's"""
    rows = _plan(lib, kind, alphas, 20, schedule, strength=0.6, eta=eta)
    sg = K.sigmas(schedule, alphas, 20)
    first = K.tail(sg, 0.6)
    assert len(sg) - 1 - first == 12 and rows[0, COL["step"]] == first and rows[0, COL["h1"]] == 0.0
    seen = []

    def noise(s, r):
        seen.append((s, r))
        return _toy_noise(s, r)

    got = K.sample_plan(rows, 0.7, _toy_predict, noise)
    ref = K.sample_textbook(kind, eta, alphas, sg, first, 0.7, _toy_predict, _toy_noise)
    assert abs(got - ref) <= 1e-12 * max(1.0, abs(ref)), f"{kind} eta={eta} {schedule}"
    if eta > 0:
        assert sorted({s for s, _ in seen}) == list(range(first, len(sg) - 2))   # every step of the call draws but the last (s' = 0)
    else:
        assert not seen
    # the mask blend follows a step's last evaluation, toward a_end = 1 / (1 + s'^2)
    last = rows[:, COL["a_end"]] >= 0
    assert last.sum() == 12 and np.allclose(rows[last, COL["a_end"]], 1.0 / (1.0 + np.array(sg[first + 1:]) ** 2), rtol=1e-13)
    blend = lambda x, a: 0.25 * x + 0.75 * (math.sqrt(a) * 0.3 + math.sqrt(1.0 - a) * -0.4)   # noqa: E731
    got = K.sample_plan(rows, 0.7, _toy_predict, _toy_noise, blend)
    ref = K.sample_textbook(kind, eta, alphas, sg, first, 0.7, _toy_predict, _toy_noise, blend)
    assert abs(got - ref) <= 1e-12 * max(1.0, abs(ref)), f"{kind} eta={eta} {schedule}: blended"


# ---- 5. identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 5, 20, 50])
def test_model_schedule_reproduces_sampler_coefs(lib, alphas, n):
    """euler / dpmpp_2m on schedule `model` ARE sdmi_sampler's kind 0 (same eta) / kind 1: the rows of sdmi_sampler_coefs"""
    from stable_diffusion_burn_amd import sampler_coefs
    ts, step = O.ddim_timesteps(n, len(alphas))
    for kind, old, eta in (("euler", "ddim", 0.0), ("euler", "ddim", 0.5), ("euler", "ddim", 1.0), ("dpmpp_2m", "dpmpp_2m", 0.0)):
        rows = _plan(lib, kind, alphas, n, "model", eta=eta)
        c = sampler_coefs(old, eta, alphas, ts, step)      # cx, ce, h1, h2, h3, cz, qx, qe
        assert len(rows) == len(ts) and rows[:, COL["t"]].tolist() == [float(t) for t in ts]
        for mine, theirs in (("cx", 0), ("ce", 1), ("h1", 2), ("cz", 5), ("qx", 6), ("qe", 7)):
            assert np.abs(rows[:, COL[mine]] - c[:, theirs]).max() <= 1e-14, (kind, eta, mine)
        assert (rows[:, COL["cz2"]] == 0).all() and (c[:, 3:5] == 0).all()


@pytest.mark.parametrize("schedule", K.SCHEDULES)
def test_dpmpp_2m_sde_at_eta_0_is_dpmpp_2m(lib, alphas, schedule):
    for n, strength in ((1, 1.0), (5, 1.0), (20, 1.0), (20, 0.6)):
        a = _plan(lib, "dpmpp_2m_sde", alphas, n, schedule, strength=strength)
        b = _plan(lib, "dpmpp_2m", alphas, n, schedule, strength=strength)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-14


@pytest.mark.parametrize("schedule", K.SCHEDULES)
def test_two_stage_kinds_with_one_step_are_eulers_single_row(lib, alphas, schedule):
    ref = _plan(lib, "euler", alphas, 1000 if schedule == "model" else 1, schedule)
    ref = ref[-1:] if schedule == "model" else ref          # (schedule `model` has one step only where n = total: compare its LAST step there)
    for kind in K.TWO_STAGE:
        for eta in ((0.0, 1.0) if kind in K.ETA_KINDS else (0.0,)):
            rows = _plan(lib, kind, alphas, 1000 if schedule == "model" else 1, schedule, eta=eta)
            assert np.abs(rows[-1:] - ref).max() <= 1e-14, (kind, eta)
            if schedule != "model":
                assert len(rows) == 1


# ---- 6. noise only where it belongs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", K.SCHEDULES)
@pytest.mark.parametrize("kind,eta", CASES)
def test_noise_only_where_it_belongs(lib, alphas, kind, eta, schedule):
    rows = _plan(lib, kind, alphas, 7, schedule, eta=eta)
    sg = K.sigmas(schedule, alphas, 7)
    cz, cz2, step, stage = (rows[:, COL[k]] for k in ("cz", "cz2", "step", "stage"))
    final = step == len(sg) - 2
    assert (cz[final] == 0).all() and (cz2[final] == 0).all()        # a step that ends at 0 draws nothing
    if eta == 0.0:
        assert (cz == 0).all() and (cz2 == 0).all()
        return
    if kind == "dpmpp_sde":
        assert (cz[~final] != 0).all() and ((cz2 != 0) == ((stage == 1) & ~final)).all()
        for row in rows[(stage == 1) & ~final]:
            s, s2 = sg[int(row[COL["step"]])], sg[int(row[COL["step"]]) + 1]
            _, u2 = K.anc(s, s2, eta)
            al, be = row[COL["cz"]] / (u2 * K._c(s2)), row[COL["cz2"]] / (u2 * K._c(s2))
            assert abs(al * al + be * be - 1.0) <= 1e-12 and al > 0 and be > 0
    else:
        assert (cz2 == 0).all()
        if kind == "dpmpp_2s":
            assert ((cz != 0) == ((stage == 1) & ~final)).all()
        else:
            assert (cz[~final] != 0).all()


# ---- 7. the point of the feature -----------------------------------------------------------------------------------------------------
def _gauss_error(lib, alphas, kind, n, s, schedule="karras"):
    """data N(0, s^2) from x_T = 1: e(x, a) = x sqrt(1 - a) / (a s^2 + 1 - a), the exact end point s / sqrt(a_T s^2 + 1 - a_T)"""
    def predict(x, t, sigma):
        a = 1.0 / (1.0 + sigma * sigma)
        return x * math.sqrt(1.0 - a) / (a * s * s + 1.0 - a)
    rows = _plan(lib, kind, alphas, n, schedule)
    a_T = 1.0 / (1.0 + rows[0, COL["sigma"]] ** 2)
    exact = s / math.sqrt(a_T * s * s + 1.0 - a_T)
    return abs(K.sample_plan(rows, 1.0, predict) - exact) / exact


def test_second_order_kinds_end_closer_than_euler(lib, alphas):
    stated = {0.5: dict(euler=0.0436, heun=0.0016, dpm2=0.0002, dpmpp_2m=0.0016, dpmpp_2s=0.0035),
              1.5: dict(euler=0.0361, heun=0.0022, dpm2=0.0012, dpmpp_2m=0.0023, dpmpp_2s=0.0015)}
    print("| n = 40 | euler | heun | dpm2 | dpmpp_2m | dpmpp_2s |")
    for s in (0.5, 1.5):
        err = {k: _gauss_error(lib, alphas, k, 40, s) for k in stated[s]}
        print(f"| s = {s} | " + " | ".join(f"{err[k]:.4f}" for k in stated[s]) + " |")
        for k, v in stated[s].items():
            assert abs(err[k] - v) <= 6e-5, (s, k, err[k])           # the table of DESIGN.md section 9i, to its last printed digit
        for k in ("heun", "dpm2", "dpmpp_2m", "dpmpp_2s"):
            assert 5.0 * err[k] <= err["euler"], (s, k, err[k], err["euler"])
        heun20, euler20 = _gauss_error(lib, alphas, "heun", 20, s), _gauss_error(lib, alphas, "euler", 20, s)
        print(f"  s = {s}: heun at n = 20 (39 evaluations) {heun20:.4f}, euler at n = 20 {euler20:.4f}")
        assert len(_plan(lib, "heun", alphas, 20)) == 39 and heun20 < err["euler"]
        assert abs(heun20 - {0.5: 0.0129, 1.5: 0.0103}[s]) <= 6e-5
        assert 1.6 <= euler20 / err["euler"] <= 2.4                  # first order: the error halves from n = 20 to 40


# ---- 8. validation -------------------------------------------------------------------------------------------------------------------
def test_invalid_structs_and_arguments_are_refused(lib, alphas):
    from stable_diffusion_burn_amd._capi import SdmiKSampler
    a = np.ascontiguousarray(alphas, np.float32)
    ap = a.ctypes.data_as(C.POINTER(C.c_float))
    S = K.model_sigmas(alphas)
    buf = (C.c_double * (12 * 2100))()
    count = C.c_int32()

    def status(n=10, strength=1.0, cap=2100, total=a.size, **f):
        k = SdmiKSampler()
        for name, v in f.items():
            setattr(k, name, v)
        st = (lib.sdmi_ksampler_sigmas(C.byref(k), ap, total, n, buf, cap, C.byref(count)),
              lib.sdmi_ksampler_plan(C.byref(k), ap, total, n, strength, buf, cap, C.byref(count)))
        return st

    assert status() == (SDMI_OK, SDMI_OK) and status(kind=6, schedule=3, eta=1.0, rho=3.0, sigma_min=float(S[0]), sigma_max=float(S[-1])) == (SDMI_OK, SDMI_OK)
    bad = [dict(kind=7), dict(kind=-1), dict(schedule=4), dict(schedule=-1), dict(eta=-0.01), dict(eta=1.0001), dict(eta=float("nan")),
           dict(kind=1, eta=0.5), dict(kind=2, eta=1.0), dict(kind=3, eta=0.25), dict(rho=-1.0), dict(rho=float("inf")), dict(rho=float("nan")),
           dict(sigma_min=-0.1), dict(sigma_max=float("inf")), dict(sigma_min=float("nan")), dict(sigma_min=float(S[0]) * 0.99), dict(sigma_max=float(S[-1]) * 1.01),
           dict(sigma_min=2.0, sigma_max=1.0), dict(sigma_min=1.0, sigma_max=1.0)]
    for f in bad:
        assert status(**f) == (SDMI_ERR_INVALID, SDMI_ERR_INVALID), f
    for kind in (0, 4, 5, 6):
        assert status(kind=kind, eta=1.0) == (SDMI_OK, SDMI_OK)
    # arguments: steps, capacity (the count needed still comes back), strength, pointers
    assert status(n=0) == (SDMI_ERR_INVALID, SDMI_ERR_INVALID) and status(n=a.size + 1) == (SDMI_ERR_INVALID, SDMI_ERR_INVALID)
    assert status(kind=2, cap=10) == (SDMI_ERR_INVALID, SDMI_ERR_INVALID) and count.value == 19
    assert status(kind=2, cap=19)[1] == SDMI_OK and status(cap=11)[0] == SDMI_OK and status(cap=10)[0] == SDMI_ERR_INVALID
    for strength in (0.0, -0.5, 1.0001, float("nan"), 0.09):         # 0.09 x 10 steps leaves none
        assert status(strength=strength)[1] == SDMI_ERR_INVALID, strength
    assert status(strength=0.1)[1] == SDMI_OK and count.value == 1
    k = SdmiKSampler()
    assert lib.sdmi_ksampler_plan(None, ap, a.size, 10, 1.0, buf, 2100, C.byref(count)) == SDMI_ERR_INVALID
    assert lib.sdmi_ksampler_plan(C.byref(k), None, a.size, 10, 1.0, buf, 2100, C.byref(count)) == SDMI_ERR_INVALID
    assert lib.sdmi_ksampler_plan(C.byref(k), ap, a.size, 10, 1.0, buf, 2100, None) == SDMI_ERR_INVALID
    assert lib.sdmi_ksampler_sigmas(C.byref(k), ap, 0, 10, buf, 2100, C.byref(count)) == SDMI_ERR_INVALID
    t = C.c_double()
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.sdmi_sigma_to_t(ap, a.size, sigma, C.byref(t)) == SDMI_ERR_INVALID
    assert lib.sdmi_sigma_to_t(ap, a.size, 1.0, None) == SDMI_ERR_INVALID and lib.sdmi_sigma_to_t(None, a.size, 1.0, C.byref(t)) == SDMI_ERR_INVALID
    # the Python layer refuses unknown names before the library sees them
    from stable_diffusion_burn_amd import ksampler_plan
    with pytest.raises(ValueError):
        ksampler_plan("lms", alphas, 10)
    with pytest.raises(ValueError):
        ksampler_plan("euler", alphas, 10, schedule="polyexponential")


def test_sample_cli_reads_the_environment_variable():
    src = (ROOT / "stable_diffusion_burn_amd" / "csrc" / "sample_main.cpp").read_text()
    assert 'getenv("SDMI_KSAMPLER")' in src and "sdmi_set_ksampler" in src
