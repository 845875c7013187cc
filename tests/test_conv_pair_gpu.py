"""The paired launch of a ResBlock's tail (Engine::conv_pair, option skip_slices): y = conv3x3(h, w_out) + b_out + conv1x1(x, w_skip) + b_skip as ONE split-K launch of
k_gemm3p.hip -- slices [0, z_aux) work on the 3x3 problem, slices [z_aux, splits) on the 1x1 shortcut (ConvGemm::z_aux) -- plus the reduce that sums every slab and
adds both biases.  Reference arithmetic: ResBlock::forward / ResnetBlock::forward (unet/mod.rs:713-733, autoencoder/mod.rs:514-527: skip_connection(x) + out_layers(h)).

Operator level (sdmi_op_conv2d_pair) against the fp64 oracle at the bar every fp32 operator holds (tests/test_ops_gpu.py: 2e-5 max(1, |ref|)), on five plane tiles
and four (main, auxiliary) slice requests, twice for bit-equality; planes output = split of the fp32 output; a sample's result does not depend on its place in the
batch; both settings of skip_slices.  Model level (sd_tiny): one UNet forward at the bar of test_unet_forward_with_producer_written_planes, and exactly the shortcut
launches gone from the launch count."""
import math
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sd_oracle as O  # noqa: E402

# (n, cin_x, cout, H, W)
CASES = [
    (1, 64, 32, 8, 8),        # one tile; auxiliary problem of 2 k tiles
    (2, 96, 160, 12, 12),     # ragged M
    (3, 64, 128, 8, 8),       # several samples per tile; general epilogue
    (1, 160, 64, 23, 19),     # ragged M; 5 auxiliary k tiles
    (2, 192, 320, 16, 16),    # two column tiles of 160
]
TILES = [300, 303, 304, 305, 308]
SLICES = [(1, 1), (3, 1), (2, 2), (1000, 1000)]   # the last: more than the k tiles of either problem -> clamped, one-tile slices
_OPTS = {"gemm_tile": "auto", "splitk": 0, "splitk_aux": 0, "skip_slices": None}   # skip_slices: restored to what the context had

_cache = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _case(case):
    """inputs and the fp64 reference of a case, computed once"""
    if case not in _cache:
        n, cin_x, cout, H, W = case
        g = np.random.default_rng(4200 + 7 * cin_x + cout + H)
        x = g.standard_normal((n, cin_x, H, W)).astype(np.float32)
        h = g.standard_normal((n, cout, H, W)).astype(np.float32)
        ws = (g.standard_normal((cout, cin_x, 1, 1)) / math.sqrt(cin_x)).astype(np.float32)
        wo = (g.standard_normal((cout, cout, 3, 3)) / math.sqrt(9 * cout)).astype(np.float32)
        bs = g.standard_normal(cout).astype(np.float32)
        bo = g.standard_normal(cout).astype(np.float32)
        ref = (O.conv2d(_t(h), (_t(wo), _t(bo)), padding=1) + O.conv2d(_t(x), (_t(ws), _t(bs)), padding=0)).numpy()
        ref.setflags(write=False)
        _cache[case] = (x, h, ws, bs, wo, bo, ref)
    return _cache[case]


def _check(got, ref, what, rel=2e-5):
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got.astype(np.float64) - ref).max()
    tol = rel * max(1.0, np.abs(ref).max())
    print(f"{what}: max err {err:.3e} (tol {tol:.3e})")
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


class _Opts:
    """engine options for the block, the defaults restored on exit (skip_slices: switched back off / on as the context's default has it)"""

    def __init__(self, sd, default_skip, **opts):
        self.sd, self.default_skip, self.opts = sd, default_skip, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.sd.set_option(k, v)
        return self.sd

    def __exit__(self, *a):
        for k in self.opts:
            self.sd.set_option(k, self.default_skip if k == "skip_slices" else _OPTS[k])


DEFAULT_SKIP_SLICES = 1   # the engine's default: what the tests leave the shared contexts at


@pytest.fixture(scope="module")
def default_skip():
    return DEFAULT_SKIP_SLICES


@pytest.mark.parametrize("case", CASES)
def test_conv2d_pair_tiles_and_slices(sd_ops, default_skip, case):
    x, h, ws, bs, wo, bo, ref = _case(case)
    for tile in TILES:
        for sm, sa in SLICES:
            with _Opts(sd_ops, default_skip, skip_slices=1, gemm_tile=tile, splitk=sm, splitk_aux=sa):
                got = sd_ops.op_conv2d_pair(x, h, ws, bs, wo, bo)
                again = sd_ops.op_conv2d_pair(x, h, ws, bs, wo, bo)
            _check(got, ref, f"pair {case} tile={tile} slices=({sm},{sa})")
            assert np.array_equal(got, again), f"pair {case} tile={tile} slices=({sm},{sa}): two runs differ"


@pytest.mark.parametrize("case", CASES)
def test_planes_output_is_the_split_of_the_fp32_output(sd_ops, default_skip, case):
    x, h, ws, bs, wo, bo, ref = _case(case)
    for tile in TILES:
        with _Opts(sd_ops, default_skip, skip_slices=1, gemm_tile=tile, splitk=2, splitk_aux=2):
            got, planes = sd_ops.op_conv2d_pair(x, h, ws, bs, wo, bo, planes=True)
            alone = sd_ops.op_conv2d_pair(x, h, ws, bs, wo, bo)
        assert np.array_equal(got.view(np.uint32), planes.view(np.uint32)), f"pair {case} tile={tile}: planes differ from the fp32 output"
        assert np.array_equal(got, alone), f"pair {case} tile={tile}: writing planes as well changed the fp32 output"
        _check(got, ref, f"pair + planes {case} tile={tile}")


@pytest.mark.parametrize("tile", TILES)
def test_result_does_not_depend_on_the_batch_position(sd_ops, default_skip, tile):
    x, h, ws, bs, wo, bo, _ = _case(CASES[2])
    x, h = x.copy(), h.copy()
    x[2], h[2] = x[0], h[0]
    for sm, sa in SLICES:
        with _Opts(sd_ops, default_skip, skip_slices=1, gemm_tile=tile, splitk=sm, splitk_aux=sa):
            got = sd_ops.op_conv2d_pair(x, h, ws, bs, wo, bo)
        assert np.array_equal(got[0], got[2]), f"tile={tile} slices=({sm},{sa}): positions 0 and 2 differ"
        assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("case", CASES)
def test_both_settings_of_skip_slices_hold_the_bar(sd_ops, default_skip, case):
    """0: the shortcut's own launch, then conv_out with it as the residual; 1: the paired launch.  Forced slices, then the planner's own choice -- which
    declines the first case (conv_out is not split there: the reduce would be a new dependent phase), an error at operator level, never a silent other path."""
    from stable_diffusion_burn_amd import SdmiError
    x, h, ws, bs, wo, bo, ref = _case(case)
    for skip in (0, 1):
        with _Opts(sd_ops, default_skip, skip_slices=skip, gemm_tile=304, splitk=2, splitk_aux=2):
            got = sd_ops.op_conv2d_pair(x, h, ws, bs, wo, bo)
        _check(got, ref, f"skip_slices={skip} forced {case}")
        with _Opts(sd_ops, default_skip, skip_slices=skip):
            if skip and case == CASES[0]:
                with pytest.raises(SdmiError):
                    sd_ops.op_conv2d_pair(x, h, ws, bs, wo, bo)
                continue
            got = sd_ops.op_conv2d_pair(x, h, ws, bs, wo, bo)
        _check(got, ref, f"skip_slices={skip} planned {case}")


# ---- model level ------------------------------------------------------------------------------------------------------------------------------------
def _forward(sd, tmp_path, skip, default_skip, lat, t, ctx):
    """one UNet forward under skip_slices = skip -> (result, launches, dump_choices lines)"""
    path = tmp_path / f"choices{skip}.txt"
    try:
        sd.set_option("skip_slices", skip)
        sd.set_option("record_shapes", 1)
        out = sd.unet.forward(lat, [t], ctx)
        kernels = sd.last_call_stats()["kernels"]
        sd.set_option("dump_choices", str(path))
    finally:
        sd.set_option("record_shapes", 0)
        sd.set_option("skip_slices", default_skip)
    return out, kernels, path.read_text().splitlines()


def test_unet_forward_with_paired_shortcuts(sd_tiny, synth, tiny_dims, default_skip, tmp_path):
    from stable_diffusion_burn_amd import synthetic as syn
    d = tiny_dims
    t = 999
    lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 7, d.ctx_dim) for i in range(2)])
    a = syn.alphas_cumprod()
    r32 = O.StableDiffusionOracle(synth, a, d, torch.float32).unet.forward(torch.from_numpy(lat), t, torch.from_numpy(ctx)).numpy()
    r64 = O.StableDiffusionOracle(synth, a, d, torch.float64).unet.forward(torch.from_numpy(lat), t, torch.from_numpy(ctx)).numpy()
    base, k0, lines0 = _forward(sd_tiny, tmp_path, 0, default_skip, lat, t, ctx)
    got, k1, lines1 = _forward(sd_tiny, tmp_path, 1, default_skip, lat, t, ctx)
    again, k1b, _ = _forward(sd_tiny, tmp_path, 1, default_skip, lat, t, ctx)
    e64 = np.abs(got.astype(np.float64) - r64).max()
    e32 = np.abs(r32.astype(np.float64) - r64).max()
    print(f"unet paired shortcuts: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e} |paired - two launches|={np.abs(got - base).max():.2e}; launches {k0} -> {k1}")
    assert np.isfinite(got).all() and e64 <= max(1e-4, 2 * e32)
    assert np.array_equal(got, again) and k1 == k1b
    assert np.abs(got - base).max() <= 2e-5 * max(1.0, np.abs(r64).max())
    # the launches that went: per paired ResBlock the shortcut's GEMM and, where that was split, its reduce.  dump_choices: "M,N,K k3 s1 u0 W<w> pair cfg=.. splits=..
    # +aux K<cin> z.. acc=0 x<count>" under skip_slices=1; the shortcut's own launch "M,N,<cin> k1 s1 u0 W<w> cfg=.. splits=<s> acc=.. x<count>" under 0
    pairs = [re.match(r"(\d+),(\d+),\d+ k3 s1 u0 W(\d+) pair cfg=\d+ splits=\d+ \+aux K(\d+) z\d+ acc=0 x(\d+)$", ln) for ln in lines1 if " pair " in ln]
    assert pairs and all(pairs), [ln for ln in lines1 if " pair " in ln]
    assert not any(" pair " in ln for ln in lines0)
    gone = 0
    for m in pairs:
        M, N, W, cin, count = map(int, m.groups())
        own = [re.match(rf"{M},{N},{cin} k1 s1 u0 W{W} cfg=\d+ splits=(\d+) .*x(\d+)$", ln) for ln in lines0]
        own = [o for o in own if o]
        assert len(own) == 1, (m.group(0), own)
        splits, count0 = int(own[0].group(1)), int(own[0].group(2))
        assert count0 >= count
        gone += count * (2 if splits > 1 else 1)
    assert k0 - k1 == gone, f"launches {k0} -> {k1}, expected {gone} fewer"
