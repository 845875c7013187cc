"""CFG rescale at the operator level (include/sdmi.h "CFG rescale and zero-terminal-SNR schedules"): sampler_step_rescale_kernel through
sdmi_op_sampler_step against numpy float64 (tests/guidance_ref.py).  The bar on latent_out and q_out is
    |gpu - f64| <= 4 |f32 - f64| + 1e-6 max|f64|
with f32 the same formula restated in numpy float32 the way the kernel sums (two-pass statistics, float32 partials, float64 merges).  Shapes: 4 elements; fewer
pixels than lanes; three images of different scale; 64 x 64, the last size a 1024-thread workgroup keeps in registers; a size that is no multiple of the workgroup;
the first size that reads its image again; 128 x 128."""
import numpy as np
import pytest

import guidance_ref as G

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 3, 5), (3, 8, 8), (2, 64, 64), (1, 72, 56), (1, 80, 80), (1, 128, 128)]
# depth, cz, cz2, mask
FORMS = [(0, 0.0, 0.0, False), (1, 0.0, 0.0, False), (3, 0.0, 0.0, False), (0, 0.3, 0.0, True), (1, 0.3, 0.2, False), (3, 0.3, 0.0, True), (1, 0.3, 0.2, True),
         (0, 0.0, 0.0, True)]
PHIS = [0.3, 0.7, 1.0]
SCALES = [1.0, 7.5]
KEY, KEY2 = 0x5EED00000001, 0x4000000000000000 + 77


def _case(n, h, w, depth, cz, cz2, mask, seed, mean=0.0):
    rng = np.random.default_rng(seed)
    img_scale = np.float32([0.1, 1.0, 30.0])[:n].reshape(n, 1, 1, 1) if n == 3 else np.float32(1.0)
    eu = (rng.standard_normal((n, 4, h, w)).astype(np.float32) * img_scale + np.float32(mean)).astype(np.float32)
    mix = np.float32([0.2, 0.6, 0.95])[:n].reshape(n, 1, 1, 1) if n == 3 else np.float32(0.6)   # (per image, so that the factors differ)
    ec = (eu * mix + rng.standard_normal((n, 4, h, w)).astype(np.float32) * img_scale * np.float32(0.5) + np.float32(0.4 * mean)).astype(np.float32)
    d = {"eps": np.concatenate([eu, ec]), "latent": rng.standard_normal((n, 4, h, w)).astype(np.float32),
         "row": np.float64([0.93, -0.41, 0.17, -0.09, 0.05, cz, cz2, 1.07, -0.38]), "depth": depth,
         "q_hist": rng.standard_normal((depth, n, 4, h, w)).astype(np.float32) if depth else None, "mask": None, "z0": None, "e0": None}
    if depth < 3:
        d["row"][3:5] = 0.0
    if depth < 1:
        d["row"][2] = 0.0
    if mask:
        d["mask"] = rng.uniform(0.0, 1.0, (n, h, w)).astype(np.float32)
        d["mask"][:, :, : max(1, w // 3)] = 1.0
        d["z0"], d["e0"] = (rng.standard_normal((n, 4, h, w)).astype(np.float32) for _ in range(2))
    return d


def _gpu(sd, d, scale, phi):
    return sd.op_sampler_step(d["eps"], d["latent"], scale, d["row"], rescale=phi, depth=d["depth"], q_hist=d["q_hist"], noise_key=KEY, noise_key2=KEY2,
                              mask=d["mask"], z0=d["z0"], e0=d["e0"], blend_prev=0.8, blend_dir=0.6)


def _ref(dtype, d, scale, phi):
    return G.step(dtype, d["eps"], d["latent"], scale, phi, d["row"], d["q_hist"] if d["depth"] else (), KEY, KEY2, d["mask"], d["z0"], d["e0"], 0.8, 0.6)


def _bar(got, r32, r64, what):
    got, r32 = np.asarray(got, np.float64), np.asarray(r32, np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    e, e32, top = np.abs(got - r64).max(), np.abs(r32 - r64).max(), np.abs(r64).max()
    bound = 4.0 * e32 + 1e-6 * top
    print(f"{what}: max|gpu-f64| = {e:.3e}  |f32-f64| = {e32:.3e}  max|f64| = {top:.3e}  bound {bound:.3e}")
    assert e <= bound, f"{what}: max|gpu-f64| = {e:.3e} > {bound:.3e}"


@pytest.mark.parametrize("form", range(len(FORMS)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_parity(sd_ops, shape, form):
    n, h, w = shape
    depth, cz, cz2, mask = FORMS[form]
    d = _case(n, h, w, depth, cz, cz2, mask, seed=1000 * form + h * w + n)
    for phi, scale in [(p, s) for p in PHIS for s in SCALES]:
        got_x, got_q = _gpu(sd_ops, d, scale, phi)
        x64, q64, f64 = _ref(np.float64, d, scale, phi)
        x32, q32, _ = _ref(np.float32, d, scale, phi)
        what = f"{shape} depth {depth} cz {cz} cz2 {cz2} mask {mask} phi {phi} scale {scale}"
        _bar(got_x, x32, x64, what + " latent")
        if depth:
            _bar(got_q, q32, q64, what + " q")
        else:
            assert got_q is None
        if n == 3 and scale != 1.0:   # (at scale 1 the guided output is the conditional one and every factor is 1)
            assert np.ptp(f64) > 0.05, f64   # (the three images do get three factors)


@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 64, 64), (1, 80, 80)], ids=lambda s: "x".join(map(str, s)))
def test_large_mean(sd_ops, shape):
    """eu, ec = 50 + N(0, 1) (test_group_norm_large_mean's regime): the factor recovered from q (qx = 0, qe = 1: q = f g) is within the bar of float64.  A one-pass
    sum-of-squares form loses it: in float32 sum x^2 / N - mean^2 carries an error of about 2500 * 2^-24 * sqrt(N) against a variance of order 1."""
    n, h, w = shape
    d = _case(n, h, w, 1, 0.0, 0.0, False, seed=77, mean=50.0)
    d["row"][7:9] = (0.0, 1.0)
    for phi in PHIS:
        _, got_q = _gpu(sd_ops, d, 7.5, phi)
        _, q64, f64 = _ref(np.float64, d, 7.5, phi)
        _, q32, _ = _ref(np.float32, d, 7.5, phi)
        _bar(got_q, q32, q64, f"large mean {shape} phi {phi} q")
        g64 = q64 / f64.reshape(n, 1, 1, 1)
        big = np.abs(g64) > 1.0
        f_gpu = np.float64([np.median((np.asarray(got_q[b], np.float64) / g64[b])[big[b]]) for b in range(n)])
        f_32 = np.float64([np.median((np.asarray(q32[b], np.float64) / g64[b])[big[b]]) for b in range(n)])
        e, e32 = np.abs(f_gpu - f64).max(), np.abs(f_32 - f64).max()
        print(f"large mean {shape} phi {phi}: f = {f64}  |f_gpu - f64| = {e:.3e}  |f_f32 - f64| = {e32:.3e}")
        assert e <= 4.0 * e32 + 1e-6 * np.abs(f64).max()


@pytest.mark.parametrize("form", range(len(FORMS)))
def test_degenerate_images_keep_factor_one(sd_ops, form):
    """ec == eu == a constant per image: std(g) = 0, f = 1 -- finite, and the rescale = 0 result within 1 ulp.  The kernel writes the step's contractions out in
    the order the elementwise kernels compile to, so q and the unmasked latent are in fact the same bits (results that cancel to a small value would otherwise differ
    by several of THEIR ulps).  The mask blend m x' + (1 - m) t is the exception: the elementwise instantiations themselves contract it two ways (fma(m, x', (1 - m) t)
    in some, fma(1 - m, t, m x') in others), so no one form matches them all.  Either way one product is rounded (half an ulp of that term) and then the sum (half an
    ulp of the result): under a mask the bar is 1 ulp of the larger term plus 1 ulp of the result."""
    n, h, w = 2, 8, 8
    depth, cz, cz2, mask = FORMS[form]
    d = _case(n, h, w, depth, cz, cz2, mask, seed=5)
    const = np.float32([0.0, 3.25]).reshape(n, 1, 1, 1) * np.ones((n, 4, h, w), np.float32)
    d["eps"] = np.concatenate([const, const])
    want_x, want_q = _gpu(sd_ops, d, 7.5, 0.0)
    tol = np.spacing(np.abs(want_x))
    if mask:
        bare = dict(d, mask=None, z0=None, e0=None)
        pre, _ = _gpu(sd_ops, bare, 7.5, 0.0)
        m = d["mask"].reshape(n, 1, h, w)
        t = np.float32(0.8) * d["z0"] + np.float32(0.6) * d["e0"]
        tol = tol + np.spacing(np.maximum(np.abs(m * pre), np.abs((np.float32(1.0) - m) * t)).astype(np.float32))
    for phi in PHIS:
        got_x, got_q = _gpu(sd_ops, d, 7.5, phi)
        assert np.isfinite(got_x).all()
        bad = np.abs(got_x - want_x) > tol
        assert not bad.any(), f"phi {phi}: {int(bad.sum())} of {bad.size} latent elements past the bar, max|d| = {np.abs(got_x - want_x).max():.3e}"
        if depth:
            assert np.isfinite(got_q).all()
            bad = np.abs(got_q - want_q) > np.spacing(np.abs(want_q))
            assert not bad.any(), f"phi {phi}: {int(bad.sum())} of {bad.size} q elements differ by more than 1 ulp, max|d| = {np.abs(got_q - want_q).max():.3e}"


@pytest.mark.parametrize("hw", [(8, 8), (72, 56)])
def test_position_independence(sd_ops, hw):
    """an image alone and the same image at position 2 of n = 3: bit-identical; two runs: bit-identical (cz = 0: the noise key is the image's position)"""
    h, w = hw
    d3 = _case(3, h, w, 3, 0.0, 0.0, True, seed=9)
    d1 = dict(d3)
    d1["eps"] = np.concatenate([d3["eps"][2:3], d3["eps"][5:6]])
    for k in ("latent", "mask", "z0", "e0"):
        d1[k] = d3[k][2:3]
    d1["q_hist"] = d3["q_hist"][:, 2:3]
    x3, q3 = _gpu(sd_ops, d3, 7.5, 0.7)
    x1, q1 = _gpu(sd_ops, d1, 7.5, 0.7)
    assert np.array_equal(x3[2:3], x1) and np.array_equal(q3[2:3], q1)
    x3b, q3b = _gpu(sd_ops, d3, 7.5, 0.7)
    assert np.array_equal(x3, x3b) and np.array_equal(q3, q3b)


@pytest.mark.parametrize("form", range(len(FORMS)))
def test_rescale_0_is_the_elementwise_kernel(sd_ops, form):
    """rescale = 0 through the op: the float32 formula of the elementwise kernels -- and not the rescale kernel at f = 1, whose launch differs.  Both arms are this
    library's: the reference arm is the numpy float64 step within the op's own bar, the bits are compared between two calls and with phi at the degenerate f = 1."""
    depth, cz, cz2, mask = FORMS[form]
    d = _case(2, 16, 16, depth, cz, cz2, mask, seed=form)
    x0, q0 = _gpu(sd_ops, d, 7.5, 0.0)
    x0b, q0b = _gpu(sd_ops, d, 7.5, 0.0)
    assert np.array_equal(x0, x0b) and (q0 is None or np.array_equal(q0, q0b))
    x64, q64, _ = _ref(np.float64, d, 7.5, 0.0)
    x32, q32, _ = _ref(np.float32, d, 7.5, 0.0)
    _bar(x0, x32, x64, f"rescale 0 form {form} latent")
    if depth:
        _bar(q0, q32, q64, f"rescale 0 form {form} q")
    xr, _ = _gpu(sd_ops, d, 7.5, 0.7)
    assert not np.array_equal(xr, x0)


def test_op_refusals(sd_ops):
    from stable_diffusion_burn_amd import SdmiError
    d = _case(1, 4, 4, 1, 0.0, 0.0, False, seed=1)
    for phi in (-0.1, 1.01, float("nan")):
        with pytest.raises(SdmiError):
            _gpu(sd_ops, d, 7.5, phi)
    with pytest.raises(SdmiError):
        sd_ops.op_sampler_step(d["eps"], d["latent"], 7.5, d["row"], depth=2, q_hist=d["q_hist"])
    bad = dict(d)
    bad["row"] = d["row"].copy()
    bad["row"][6] = 0.2   # cz2 without cz
    with pytest.raises(SdmiError):
        _gpu(sd_ops, bad, 7.5, 0.7)
