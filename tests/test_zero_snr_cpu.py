"""Zero-terminal-SNR schedules on the host (no GPU; include/sdmi.h "CFG rescale and zero-terminal-SNR schedules"): sdmi_rescale_zero_snr
against a numpy f64 restatement, the coefficient rows sdmi_sampler_coefs_ex writes where a_t = 0 (natively in v: x0 = -v, eps = x) against their closed forms,
that no other row moved, the trajectory on a solvable case against a textbook (x0, eps_hat)-basis loop, the refusals, and that tables without a zero entry are
what they were."""
import math

import numpy as np
import pytest

import sampler_ref as S
import zero_snr_ref as Z
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

SDMI_ERR_INVALID, SDMI_ERR_UNSUPPORTED = -1, -5
KINDS = [("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp_2m", 0.0), ("plms", 0.0)]


@pytest.fixture(scope="module")
def lib():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)
    from stable_diffusion_burn_amd import _capi
    return _capi.load_library()


@pytest.fixture(scope="module")
def zt(lib):
    from stable_diffusion_burn_amd import rescale_zero_snr
    return rescale_zero_snr(syn.alphas_cumprod())


def _coefs(kind, eta, a, ts, step, prediction="v"):
    from stable_diffusion_burn_amd import sampler_coefs
    return sampler_coefs(kind, eta, a, ts, step, prediction)


def _ulps(a, b):
    ia, ib = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(ia - ib)


# ---- 1. the schedule rescale ---------------------------------------------------------------------------------------------------------
def test_error_codes():
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parents[1] / "include" / "sdmi.h").read_text()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"(SDMI_ERR_\w+)\s*=\s*(-?\d+)", text)}
    assert (codes["SDMI_ERR_INVALID"], codes["SDMI_ERR_UNSUPPORTED"]) == (SDMI_ERR_INVALID, SDMI_ERR_UNSUPPORTED)


def test_new_symbols_exported(lib):
    for s in ("sdmi_rescale_zero_snr", "sdmi_set_zero_snr", "sdmi_schedule", "sdmi_set_guidance_rescale", "sdmi_multi_set_zero_snr",
              "sdmi_multi_set_guidance_rescale", "sdmi_op_sampler_step"):
        assert hasattr(lib, s), s


@pytest.mark.parametrize("table", ["synthetic", "ldm", "short"])
def test_rescale_matches_numpy(lib, table):
    from stable_diffusion_burn_amd import default_alphas_cumprod, rescale_zero_snr
    a = {"synthetic": syn.alphas_cumprod, "ldm": lambda: default_alphas_cumprod(1000), "short": lambda: np.float32([0.9, 0.5, 0.2])}[table]()
    a = np.asarray(a, np.float32)
    got = rescale_zero_snr(a)
    ref = Z.rescale_zero_snr(a)
    assert got.dtype == np.float32 and got.shape == a.shape
    assert _ulps(got, ref).max() <= 1, _ulps(got, ref).max()
    assert got[-1] == 0.0 and not np.signbit(got[-1])
    assert got[0].tobytes() == a[0].tobytes()
    assert (np.diff(got.astype(np.float64)) < 0.0).all()
    assert np.array_equal(a, np.asarray({"synthetic": syn.alphas_cumprod, "ldm": lambda: default_alphas_cumprod(1000),
                                         "short": lambda: np.float32([0.9, 0.5, 0.2])}[table](), np.float32))   # the input is not written


def test_rescale_refusals(lib):
    from stable_diffusion_burn_amd import SdmiError, rescale_zero_snr
    for bad in ([0.5], [], [0.5, 0.5], [0.3, 0.2, 0.3], [0.2, 0.5]):
        with pytest.raises(SdmiError) as e:
            rescale_zero_snr(np.float32(bad))
        assert e.value.status == SDMI_ERR_INVALID, bad
    out = np.zeros(3, np.float32)
    assert lib.sdmi_rescale_zero_snr(None, out.ctypes.data_as(lib.sdmi_rescale_zero_snr.argtypes[1]), 3) == SDMI_ERR_INVALID


# ---- 2. the coefficient rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [1, 2, 5, 20])
@pytest.mark.parametrize("kind,eta", KINDS)
def test_zero_rows(zt, kind, eta, n_steps):
    ts, step = O.ddim_timesteps(n_steps, len(zt))
    assert zt[ts[0]] == 0.0
    k = _coefs(kind, eta, zt, ts, step)
    assert k.shape == (len(ts), 8) and np.isfinite(k).all()
    prev = float(zt[ts[0] - step]) if ts[0] >= step else 1.0
    sp, om = math.sqrt(prev), 1.0 - prev
    if kind == "ddim":
        sigma = eta * math.sqrt(om)
        want = [math.sqrt(om - sigma * sigma), -sp, 0, 0, 0, sigma, 0, 0]
    elif kind == "dpmpp_2m":
        want = [0.0, -1.0, 0, 0, 0, 0, 0.0, -1.0] if prev >= 1.0 else [math.sqrt(om), -sp, 0, 0, 0, 0, 0.0, -1.0]
    else:
        want = [math.sqrt(om), -sp, 0, 0, 0, 0, 1.0, 0.0]
    assert np.abs(k[0] - np.float64(want)).max() <= 1e-14, (k[0], want)
    # no other row moved: the same call on the table whose last entry alone is replaced
    near = zt.copy()
    near[-1] = 1e-3
    kn = _coefs(kind, eta, near, ts, step)
    first = 2 if kind == "dpmpp_2m" else 1   # 2M's row 1 looks back at row 0's lambda
    assert k[first:].tobytes() == kn[first:].tobytes()
    if kind == "dpmpp_2m" and len(ts) > 1:
        assert k[1, 2] == 0.0   # first order behind a zero row, written out
        # and it is the first-order row: the one the same timesteps give as the FIRST step of a call
        alone = _coefs(kind, eta, zt, ts[1:], step)
        assert k[1].tobytes() == alone[0].tobytes()


# ---- 3. the trajectory ---------------------------------------------------------------------------------------------------------------
def _gauss_v(s):
    """data N(0, s^2): eps = x sqrt(1 - a) / (a s^2 + 1 - a), x0 = x sqrt(a) s^2 / (a s^2 + 1 - a) exactly, v = sqrt(a) eps - sqrt(1 - a) x0"""
    return lambda x, t, cur: x * math.sqrt(cur) * math.sqrt(1.0 - cur) * (1.0 - s * s) / (cur * s * s + 1.0 - cur)


def _toy_v(x, t, cur):
    return 0.8 * math.sin(1.3 * x + 0.002 * t) + 0.35 * x * math.sqrt(1.0 - cur)


def _toy_noise(s):
    return math.sin(12.9898 * (s + 1)) * 1.7


@pytest.mark.parametrize("n_steps", [1, 2, 5, 10, 20, 40])
@pytest.mark.parametrize("kind,eta", KINDS)
def test_linear_form_matches_textbook_form(zt, kind, eta, n_steps):
    ts, step = O.ddim_timesteps(n_steps, len(zt))
    k = _coefs(kind, eta, zt, ts, step)
    for predict in (_gauss_v(1.5), _toy_v):
        got = S.sample_linear(k, zt, ts, step, 1.0, predict, _toy_noise)
        ref = Z.sample_x0_eps(kind, eta, zt, ts, step, 1.0, predict, _toy_noise)
        assert abs(got - ref) <= 1e-12 * max(1.0, abs(ref)), f"{kind} eta={eta} n={n_steps}: linear {got!r} vs textbook {ref!r}"


@pytest.mark.parametrize("s", [0.5, 1.5])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m", "plms"])
def test_gaussian_end_point_converges(zt, kind, s):
    """from x_T = 1 on the zero-terminal-SNR table the exact end point is s (a_T = 0)"""
    err = []
    for n in (10, 20, 40):
        ts, step = O.ddim_timesteps(n, len(zt))
        end = S.sample_linear(_coefs(kind, 0.0, zt, ts, step), zt, ts, step, 1.0, _gauss_v(s))
        err.append(abs(end - s) / s)
    print(f"{kind} s={s}: rel err at 10 / 20 / 40 steps {err[0]:.4g} {err[1]:.4g} {err[2]:.4g}")
    assert err[0] > err[1] > err[2]


def test_img2img_tail_never_touches_the_zero_entry(zt):
    from stable_diffusion_burn_amd import img2img_timesteps
    ts, step = img2img_timesteps(10, 0.5, len(zt)), len(zt) // 10
    assert (zt[np.asarray(ts)] > 0.0).all()
    near = zt.copy()
    near[-1] = 1e-3
    for kind, eta in KINDS:
        assert _coefs(kind, eta, zt, ts, step).tobytes() == _coefs(kind, eta, near, ts, step).tobytes()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_eps_on_a_zero_table_is_refused(zt):
    from stable_diffusion_burn_amd import SdmiError, img2img_timesteps
    ts, step = O.ddim_timesteps(5, len(zt))
    tail = img2img_timesteps(10, 0.5, len(zt))
    for kind, eta in KINDS:
        for t, st in ((ts, step), (tail, len(zt) // 10)):   # the table, not the timesteps of the call
            with pytest.raises(SdmiError) as e:
                _coefs(kind, eta, zt, t, st, "eps")
            assert e.value.status == SDMI_ERR_INVALID and "x0" in str(e.value)


def test_ksamplers_on_a_zero_table_are_refused(zt):
    from stable_diffusion_burn_amd import SdmiError, ksampler_plan, ksampler_sigmas
    for f in (lambda: ksampler_sigmas("euler", zt, 10, "karras"), lambda: ksampler_plan("heun", zt, 10, "karras"),
              lambda: ksampler_plan("dpmpp_2m", zt, 10, "model", prediction="v")):
        with pytest.raises(SdmiError) as e:
            f()
        assert e.value.status == SDMI_ERR_UNSUPPORTED and "sigma_max" in str(e.value)
    assert ksampler_sigmas("euler", syn.alphas_cumprod(), 10, "karras").size == 11   # and the loaded table still plans


# ---- 5. untouched tables ---------------------------------------------------------------------------------------------------------------
def _parent_coefs(kind, eta, a, ts, step, v):
    """sdmi_sampler_coefs_ex as it was before zero rows existed, expression for expression (f64)"""
    lam = lambda x: 0.5 * math.log(x / (1.0 - x))   # noqa: E731
    rows = []
    for j, t in enumerate(ts):
        cur = float(a[t])
        prev = float(a[t - step]) if t >= step else 1.0
        sc, sn, sp = math.sqrt(cur), math.sqrt(1.0 - cur), math.sqrt(prev)
        k = [0.0] * 8
        if kind == "ddim":
            sigma = eta * math.sqrt((1.0 - prev) / (1.0 - cur)) * math.sqrt(1.0 - cur / prev)
            k[0], k[1], k[5] = sp / sc, math.sqrt(1.0 - prev - sigma * sigma) - sp * sn / sc, sigma
        elif kind == "dpmpp_2m":
            qx, qe = 1.0 / sc, -sn / sc
            k[6], k[7] = qx, qe
            if prev >= 1.0:
                k[0], k[1] = qx, qe
            else:
                h = lam(prev) - lam(cur)
                A, B = math.sqrt((1.0 - prev) / (1.0 - cur)), -sp * math.expm1(-h)
                w0, w1 = 1.0, 0.0
                if j > 0:
                    r = (lam(cur) - lam(float(a[ts[j - 1]]))) / h
                    w0, w1 = 1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)
                k[0], k[1], k[2] = A + B * w0 * qx, B * w0 * qe, B * w1
        else:
            ce = math.sqrt(1.0 - prev) - sp * sn / sc
            w = list(S.AB[min(j, 3)]) + [0.0] * 4
            k[0] = sp / sc
            k[1], k[2], k[3], k[4] = ce * w[0], ce * w[1], ce * w[2], ce * w[3]
            k[7] = 1.0
        if v:
            k[0] += k[1] * sn
            k[1] *= sc
            k[6] += k[7] * sn
            k[7] *= sc
        rows.append(k)
    return np.float64(rows)


@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("kind,eta", KINDS)
def test_tables_without_a_zero_entry_are_what_they_were(lib, kind, eta, prediction):
    from stable_diffusion_burn_amd import default_alphas_cumprod, img2img_timesteps
    for a in (syn.alphas_cumprod(), default_alphas_cumprod(1000)):
        for n_steps in (1, 3, 5, 20):
            ts, step = O.ddim_timesteps(n_steps, len(a))
            got = _coefs(kind, eta, a, ts, step, prediction)
            assert got.tobytes() == _parent_coefs(kind, eta, a, ts, step, prediction == "v").tobytes(), (n_steps,)
        ts, step = img2img_timesteps(10, 0.6, len(a)), len(a) // 10
        assert _coefs(kind, eta, a, ts, step, prediction).tobytes() == _parent_coefs(kind, eta, a, list(ts), step, prediction == "v").tobytes()
