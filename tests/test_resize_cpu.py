"""The resampling rule of the hires fix (sdmi_resize_weights) on the host: its tables, applied in float64 numpy
(tests/resize_ref.py), against torch.nn.functional.interpolate on the CPU in float64, which defines them.  No device."""
import ctypes as C

import numpy as np
import pytest

import resize_ref as RR

SDMI_ERR_INVALID = -1
AXES = [(8, 16), (8, 12), (16, 24), (8, 20), (24, 8), (16, 5)]
# (h -> out_h, w -> out_w): every axis case once per axis, the two axes of a pair always different
PAIRS = [(AXES[i], AXES[(i + 1) % len(AXES)]) for i in range(len(AXES))]
FILTERS = [(1, 0), (1, 1), (2, 0), (2, 1)]


@pytest.fixture(scope="module")
def lib():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)
    from stable_diffusion_burn_amd import _capi
    return _capi.load_library()


def _x(h, w, seed=0):
    return np.random.default_rng(seed).standard_normal((2, 4, h, w))


@pytest.mark.parametrize("mode,antialias", FILTERS)
@pytest.mark.parametrize("hh,ww", PAIRS)
def test_tables_match_torch_float64(lib, hh, ww, mode, antialias):
    """|table applied in f64 - torch f64| <= 1e-12 max|x|: both sides are float64 sums of at most a few dozen taps"""
    x = _x(hh[0], ww[0], seed=hh[0] * 100 + ww[1])
    got, s, tx, ty = RR.resize(x, hh[1], ww[1], mode, antialias)
    ref = RR.torch_resize(x, hh[1], ww[1], mode, antialias)
    diff = np.abs(got - ref).max()
    print(f"{hh[0]}x{ww[0]} -> {hh[1]}x{ww[1]} mode {mode} aa {antialias}: max|d| = {diff:.2e}, taps {ty} x {tx}")
    assert got.shape == ref.shape and diff <= 1e-12 * np.abs(x).max()
    assert (s >= np.abs(got) - 1e-12).all()


@pytest.mark.parametrize("hh,ww", PAIRS)
def test_nearest_matches_torch_exactly(lib, hh, ww):
    x = _x(hh[0], ww[0], seed=7)
    got, _, tx, ty = RR.resize(x, hh[1], ww[1], 0)
    assert tx == ty == 1 and np.array_equal(got, RR.torch_resize(x, hh[1], ww[1], 0))


def test_nearest_sweep_matches_torch_exactly(lib):
    """mode 0 over every size pair below 130 and the multiples of 8 up to 512 (the sizes the latent rule allows), against torch on a one-axis
    tensor [1,1,1,in] -> (1, out).  torch keeps two nearest-exact rules -- scale held in float, or in double -- that differ where scale (o + 0.5) is an
    integer in exact arithmetic (6 -> 37 at o = 18, 112 -> 24 at o = 13, 90 -> 129 at o = 21 ...) and picks by out_h + out_w <= 128; the table of one axis
    follows the one-axis call, switch included."""
    import torch
    import torch.nn.functional as F
    from stable_diffusion_burn_amd import resize_weights
    pairs = [(i, o) for i in range(1, 130) for o in range(1, 130)]
    pairs += [(i, o) for i in range(8, 513, 8) for o in range(8, 513, 8) if i >= 130 or o >= 130]
    bad = []
    for i, o in pairs:
        first, count, taps = resize_weights(i, o, "nearest")
        ref = F.interpolate(torch.arange(i, dtype=torch.float64).reshape(1, 1, 1, i), size=(1, o), mode="nearest-exact").reshape(-1).numpy()
        if taps.shape != (o, 1) or not ((taps == 1.0).all() and (count == 1).all() and np.array_equal(first, ref.astype(np.int32))):
            bad.append((i, o))
    assert not bad, f"{len(bad)} of {len(pairs)} size pairs differ from torch, e.g. {bad[:8]}"
    # the ties the two rules decide differently, one on each side of the switch
    assert resize_weights(6, 37, "nearest")[0][18] == 2 and resize_weights(112, 24, "nearest")[0][13] == 62
    assert resize_weights(90, 129, "nearest")[0][21] == 15 and resize_weights(8, 164, "nearest")[0][20] == 1


@pytest.mark.parametrize("i,o", [(8, 9), (9, 8), (7, 64), (64, 7), (3, 11), (1, 5), (5, 1), (40, 24), (64, 128), (64, 96)])
def test_other_sizes_match_torch(lib, i, o):
    """sizes beyond the latent rule (sdmi_op_resize takes any): every mode, one axis changed, the other one the identity"""
    x = _x(i, 6, seed=i + o)
    for mode, aa in [(0, 0)] + FILTERS:
        got, _, _, _ = RR.resize(x, o, 6, mode, aa)
        assert np.abs(got - RR.torch_resize(x, o, 6, mode, aa)).max() <= 1e-12 * np.abs(x).max(), (mode, aa)


@pytest.mark.parametrize("mode,antialias", [(0, 0)] + FILTERS)
def test_identity_axis_is_one_tap(lib, mode, antialias):
    from stable_diffusion_burn_amd import resize_weights
    first, count, taps = resize_weights(24, 24, RR.MODES[mode], bool(antialias))
    assert taps.shape == (24, 1) and (taps == 1.0).all() and (count == 1).all() and np.array_equal(first, np.arange(24))
    x = _x(8, 24)
    got, _, tx, _ = RR.resize(x, 16, 24, mode, antialias)     # the identity on w, a real resample on h
    assert tx == 1 and np.abs(got - RR.torch_resize(x, 16, 24, mode, antialias)).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("mode,antialias", FILTERS)
def test_rows_sum_to_one(lib, mode, antialias):
    for i, o in AXES + [(64, 128), (64, 96)]:
        m, _ = RR.axis_matrix(i, o, mode, antialias)
        assert np.abs(m.sum(axis=1) - 1.0).max() <= 1e-14, (i, o)


def test_capacity_query_and_argument_errors(lib):
    T, need = C.c_int32(-1), C.c_int32(-1)
    assert lib.sdmi_resize_weights(24, 8, 2, 1, None, None, None, 0, C.byref(T), C.byref(need)) == 0
    assert T.value >= 4 and need.value == 8 * T.value
    first, count = (C.c_int32 * 8)(), (C.c_int32 * 8)()
    taps = (C.c_double * need.value)(*([7.0] * need.value))
    # too small: refused, nothing written, the sizes still reported
    T2, need2 = C.c_int32(-1), C.c_int32(-1)
    assert lib.sdmi_resize_weights(24, 8, 2, 1, first, count, taps, need.value - 1, C.byref(T2), C.byref(need2)) == SDMI_ERR_INVALID
    assert (T2.value, need2.value) == (T.value, need.value) and all(v == 7.0 for v in taps) and b"capacity" in lib.sdmi_last_error()
    assert lib.sdmi_resize_weights(24, 8, 2, 1, first, count, taps, need.value, None, None) == 0
    assert max(count) == T.value and min(count) >= 1 and all(0 <= f and f + c <= 24 for f, c in zip(first, count))
    bad = [(0, 8, 1, 0), (8, 0, 1, 0), (-8, 8, 1, 0), (8, 16, 3, 0), (8, 16, -1, 0), (8, 16, 0, 1)]
    for i, o, mode, aa in bad:
        assert lib.sdmi_resize_weights(i, o, mode, aa, None, None, None, 0, C.byref(T), C.byref(need)) == SDMI_ERR_INVALID, (i, o, mode, aa)
    # some but not all outputs
    assert lib.sdmi_resize_weights(24, 8, 2, 1, first, None, taps, need.value, None, None) == SDMI_ERR_INVALID
    assert lib.sdmi_resize_weights(24, 8, 2, 1, None, count, None, need.value, None, None) == SDMI_ERR_INVALID
