"""The tail of a fp32 transformer block as ONE paired launch (Engine::linear_pair, option proj_out_fold): with Wf = proj_out x mlp_lin folded at load,
y = x + proj_out(h + mlp_lin(u)) = u Wf + h Wp + (bf + bp) + x -- slices [0, z_aux) of a k_gemm3p.hip split-K launch work on u Wf, slices [z_aux, splits) on h Wp
(ConvGemm::z_aux), and the reduce sums every slab and adds both biases and the residual.  Reference arithmetic: SpatialTransformer::forward / MLP::forward
(unet/mod.rs:462-480, 552-591).

Operator level (sdmi_op_linear_pair) against the fp64 product at the bar every fp32 operator holds (tests/test_ops_gpu.py: 2e-5 max(1, |ref|)): rows 100 / 300, cout
96 / 320, k_main 128 / 1280, k_aux 32 / 320, every plane tile, forced slice counts and the planner's own, with and without a (strided) residual, a strided output,
fp32 / planes / both, twice for bit-equality.  The fold builder (sdmi_op_linear_fold) within one fp32 ulp of the fp64 product.  Model level (the tiny UNet): a forward
under proj_out_fold 0 and 1 at the UNet bar, the launches that went, the same with a ControlNet, a LoRA adapter on both folded layers (a stale fold would show), and a
precision-1 engine untouched."""
import itertools
import math

import numpy as np
import pytest
import torch

import controlnet_ref as CR
import lora_ref as L
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import ModelConfig, SdmiError, StableDiffusion
from stable_diffusion_burn_amd import synthetic as syn
from test_model_gpu import _assert_close

pytestmark = pytest.mark.gpu

# (rows, cout, k_main, k_aux): ragged edge tiles and the general epilogue (100, 300 rows; cout 96), four k tiles (the slice floor) and a one-tile auxiliary slice
CASES = list(itertools.product((100, 300), (96, 320), (128, 1280), (32, 320)))
TILES = list(range(300, 309))
SLICES = [(1, 1), (3, 2), (1000, 1000)]   # the last: more than the k tiles of either problem -> clamped, one-tile slices
DEFAULT_FOLD = 2                          # the engine's default: what the tests leave the shared contexts at
_DEFAULTS = {"gemm_tile": "auto", "splitk": 0, "splitk_aux": 0, "proj_out_fold": DEFAULT_FOLD}

_cache = {}


def _case(case):
    """inputs and the fp64 references (with / without the residual) of a case, computed once"""
    if case not in _cache:
        rows, cout, km, ka = case
        g = np.random.default_rng(5100 + rows + 3 * cout + 5 * km + 7 * ka)
        u = g.standard_normal((rows, km)).astype(np.float32)
        h = g.standard_normal((rows, ka)).astype(np.float32)
        wm = (g.standard_normal((km, cout)) / math.sqrt(km)).astype(np.float32)
        wa = (g.standard_normal((ka, cout)) / math.sqrt(ka)).astype(np.float32)
        bm = g.standard_normal(cout).astype(np.float32)
        ba = g.standard_normal(cout).astype(np.float32)
        r = g.standard_normal((rows, cout)).astype(np.float32)
        f = np.float64
        ref0 = u.astype(f) @ wm.astype(f) + bm.astype(f) + h.astype(f) @ wa.astype(f) + ba.astype(f)
        ref1 = ref0 + r.astype(f)
        ref0.setflags(write=False)
        ref1.setflags(write=False)
        _cache[case] = (u, h, wm, bm, wa, ba, r, ref0, ref1)
    return _cache[case]


def _check(got, ref, what, rel=2e-5):
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got.astype(np.float64) - ref).max()
    tol = rel * max(1.0, np.abs(ref).max())
    print(f"{what}: max err {err:.3e} (tol {tol:.3e})")
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


class _Opts:
    """engine options for the block, the defaults restored on exit"""

    def __init__(self, sd, **opts):
        self.sd, self.opts = sd, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.sd.set_option(k, v)
        return self.sd

    def __exit__(self, *a):
        for k in self.opts:
            self.sd.set_option(k, _DEFAULTS[k])


@pytest.mark.parametrize("case", CASES)
def test_linear_pair_tiles_and_slices(sd_ops, case):
    u, h, wm, bm, wa, ba, r, _, ref = _case(case)
    for tile in TILES:
        for sm, sa in SLICES:
            with _Opts(sd_ops, proj_out_fold=1, gemm_tile=tile, splitk=sm, splitk_aux=sa):
                got = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r)
                again = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r)
            _check(got, ref, f"pair {case} tile={tile} slices=({sm},{sa})")
            assert np.array_equal(got, again), f"pair {case} tile={tile} slices=({sm},{sa}): two runs differ"


@pytest.mark.parametrize("case", CASES)
def test_outputs_residuals_and_strides(sd_ops, case):
    """fp32 only / planes only / both; no residual, a dense one, a strided one; a strided output: the same bits wherever the same sum is formed"""
    u, h, wm, bm, wa, ba, r, ref0, ref1 = _case(case)
    rows, cout, km, ka = case
    for tile in (300, 304, 305, 307):
        with _Opts(sd_ops, proj_out_fold=1, gemm_tile=tile, splitk=2, splitk_aux=2):
            plain = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba)
            dense = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r)
            strided = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r, resid_ld=cout + 4)
            wide = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r, resid_ld=cout + 8, out_ld=cout + 32)
            planes = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r, out="planes")
            both, both3 = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r, out="both")
            wide_both, wide_both3 = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r, out_ld=cout + 64, out="both")
            no_bias = sd_ops.op_linear_pair(u, h, wm, None, wa, ba, resid=r)
        _check(plain, ref0, f"no residual {case} tile={tile}")
        _check(dense, ref1, f"residual {case} tile={tile}")
        _check(no_bias, ref1 - bm.astype(np.float64), f"no main bias {case} tile={tile}")
        for what, x in (("strided residual", strided), ("strided output", wide), ("planes only", planes), ("both: fp32", both), ("both: planes", both3),
                        ("strided both: fp32", wide_both), ("strided both: planes", wide_both3)):
            assert np.array_equal(x.view(np.uint32), dense.view(np.uint32)), f"{what} {case} tile={tile}: differs from the dense fp32 result"
        assert not np.array_equal(plain, dense)


@pytest.mark.parametrize("case", CASES)
def test_both_settings_hold_the_bar(sd_ops, case):
    """0: two launches; 1: the paired launch.  Forced slices, then the planner's own choice -- which may decline (the main launch is not split today: the reduce
    would be a new dependent phase), an error at operator level, never a silent other path."""
    u, h, wm, bm, wa, ba, r, _, ref = _case(case)
    for fold in (0, 1):
        with _Opts(sd_ops, proj_out_fold=fold, gemm_tile=304, splitk=2, splitk_aux=2):
            got = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r)
        _check(got, ref, f"proj_out_fold={fold} forced {case}")
        with _Opts(sd_ops, proj_out_fold=fold):
            try:
                got = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r)
                again = sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r)
            except SdmiError as e:
                assert fold == 1 and "do not pair" in str(e), str(e)
                print(f"proj_out_fold=1 planned {case}: the planner does not pair")
                continue
        _check(got, ref, f"proj_out_fold={fold} planned {case}")
        assert np.array_equal(got, again)


def test_option_splitk_alone_does_not_pair(sd_ops):
    u, h, wm, bm, wa, ba, r, _, _ = _case(CASES[0])
    with _Opts(sd_ops, proj_out_fold=1, splitk=2):
        with pytest.raises(SdmiError):
            sd_ops.op_linear_pair(u, h, wm, bm, wa, ba, resid=r)


# ---- the fold builder ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [64, 320])
def test_fold_is_the_fp64_product_rounded_once(sd_ops, c):
    g = np.random.default_rng(77 + c)
    wl = (g.standard_normal((4 * c, c)) / math.sqrt(4 * c)).astype(np.float32)     # mlp_lin [in = 4c, out = c]
    bl = g.standard_normal(c).astype(np.float32)
    wp = (g.standard_normal((c, c)) / math.sqrt(c)).astype(np.float32)             # proj_out [cout, c] (1x1)
    wf, bf = sd_ops.op_linear_fold(wl, bl, wp)
    ref_w = wp.astype(np.float64) @ wl.astype(np.float64).T
    ref_b = wp.astype(np.float64) @ bl.astype(np.float64)
    for what, got, ref in (("Wf", wf, ref_w), ("bf", bf, ref_b)):
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        worst = float((np.abs(got.astype(np.float64) - ref) / ulp).max())
        print(f"fold c={c} {what}: worst error {worst:.3f} ulp; {np.mean(got == ref.astype(np.float32)) * 100:.2f} % correctly rounded")
        assert got.shape == ref.shape and np.isfinite(got).all() and worst <= 1.0
    again = sd_ops.op_linear_fold(wl, bl, wp)
    assert np.array_equal(wf, again[0]) and np.array_equal(bf, again[1])
    wf0, bf0 = sd_ops.op_linear_fold(wl, None, wp)
    assert np.array_equal(wf0, wf) and not bf0.any()


# ---- model level ------------------------------------------------------------------------------------------------------------------------------------
N_TRANSFORMERS = 16       # SpatialTransformers of the UNet; a ControlNet adds its encoder's 6 and its middle block's


def _unet_inputs(d):
    lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 7, d.ctx_dim) for i in range(2)])
    return lat, ctx


def _forward(sd, fold, lat, t, ctx):
    try:
        sd.set_option("proj_out_fold", fold)
        out = sd.unet.forward(lat, [t], ctx)
        return out, sd.last_call_stats()["kernels"]
    finally:
        sd.set_option("proj_out_fold", DEFAULT_FOLD)


def test_unet_forward_with_folded_proj_out(sd_tiny, synth, tiny_dims):
    d, t = tiny_dims, 999
    lat, ctx = _unet_inputs(d)
    a = syn.alphas_cumprod()
    r32 = O.StableDiffusionOracle(synth, a, d, torch.float32).unet.forward(torch.from_numpy(lat), t, torch.from_numpy(ctx)).numpy()
    r64 = O.StableDiffusionOracle(synth, a, d, torch.float64).unet.forward(torch.from_numpy(lat), t, torch.from_numpy(ctx)).numpy()
    base, k0 = _forward(sd_tiny, 0, lat, t, ctx)
    got, k1 = _forward(sd_tiny, 1, lat, t, ctx)
    again, k1b = _forward(sd_tiny, 1, lat, t, ctx)
    for what, x in (("proj_out_fold=0", base), ("proj_out_fold=1", got)):
        e64, e32 = _assert_close(x, r32, r64, f"unet_forward {what}", atol=1e-4)
        print(f"unet {what}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    print(f"|folded - two launches|={np.abs(got - base).max():.2e}; launches {k0} -> {k1}")
    assert np.array_equal(got, again) and k1 == k1b
    assert k0 - k1 >= N_TRANSFORMERS, f"launches {k0} -> {k1}: fewer than {N_TRANSFORMERS} gone"


def test_controlled_forward_with_folded_proj_out(tiny_dims, synth):
    d, t = tiny_dims, 999
    sd = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, control_hint_ch=3))
    try:
        sd.load_weights(synth, clip=False)
        lat, ctx = _unet_inputs(d)
        g = np.random.default_rng(901)
        hint = g.integers(0, 256, (2, 8 * d.latent_h, 8 * d.latent_w, 3), dtype=np.uint8)
        sd.set_control(hint, strength=0.6, start=0.5, end=0.5)
        refs = []
        for dt in (torch.float32, torch.float64):
            res = CR.ControlNetOracle(synth, d, dt).forward(torch.from_numpy(lat), t, torch.from_numpy(ctx), CR.hint01(hint))
            refs.append(CR.controlled_forward(O.UNetOracle(synth, d, dt), torch.from_numpy(lat), t, torch.from_numpy(ctx), res, 0.6).numpy())
        base, k0 = _forward(sd, 0, lat, t, ctx)
        got, k1 = _forward(sd, 1, lat, t, ctx)
        for what, x in (("proj_out_fold=0", base), ("proj_out_fold=1", got)):
            e64, e32 = _assert_close(x, refs[0], refs[1], f"controlled forward {what}")
            print(f"controlled {what}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
        print(f"controlled: launches {k0} -> {k1}")
        assert k0 - k1 >= N_TRANSFORMERS + 7, f"launches {k0} -> {k1}"
    finally:
        sd.close()


class _Effective:
    """the synthetic weights with the engine's effective (merged) tensors in place of the adapted ones"""

    def __init__(self, base, eff):
        self.base, self.eff = base, eff

    def get(self, name, shape, kind, fan_in=0):
        return self.eff[name] if name in self.eff else self.base.get(name, shape, kind, fan_in)


def test_lora_on_both_folded_layers_never_meets_a_stale_fold(tiny_dims, synth):
    """an adapter on ff.net.2 (mlp/lin) and proj_out of two blocks: after set_scale(0.7), set_scale(0) and detach the fold-on forward follows the oracle that runs
    effective_weight's tensors -- a fold left over from the weights before would be off by the adapter's whole effect"""
    d, t = tiny_dims, 500
    c = d.model_channels
    sd = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch))
    try:
        sd.set_option("keep_masters", 1)
        sd.load_weights(synth, clip=False, vae_encoder=False)
        lat, ctx = _unet_inputs(d)
        tl, tc = torch.from_numpy(lat), torch.from_numpy(ctx)
        mid = "unet/middle_block/transformer"
        targets = {L.TB + "/mlp/lin/weight": ((4 * c, c), 8), L.ST + "/proj_out/weight": ((c, c, 1, 1), 4),
                   mid + "/transformer/mlp/lin/weight": ((16 * c, 4 * c), 8), mid + "/proj_out/weight": ((4 * c, 4 * c, 1, 1), 4)}
        ad = L.make_adapter(targets, 61, rel=0.3)
        a = syn.alphas_cumprod()

        def check(what, moved_from=None):
            eff = {n: sd.effective_weight(n) for n in targets}
            prov = _Effective(synth, eff)
            r32 = O.StableDiffusionOracle(prov, a, d, torch.float32).unet.forward(tl, t, tc).numpy()
            r64 = O.StableDiffusionOracle(prov, a, d, torch.float64).unet.forward(tl, t, tc).numpy()
            out = {}
            for fold in (0, 1):
                out[fold], _ = _forward(sd, fold, lat, t, ctx)
                e64, e32 = _assert_close(out[fold], r32, r64, f"{what} proj_out_fold={fold}", atol=1e-4)
                print(f"{what} proj_out_fold={fold}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
            if moved_from is not None:
                moved = float(np.abs(out[1] - moved_from).max())
                print(f"{what}: the adapter moves the output by {moved:.2e}")
                assert moved > 100 * 1e-4
            return out[1]

        before = check("before attaching")
        h = sd.lora_attach(ad, scale=0.7)
        try:
            check("scale 0.7", moved_from=before)
            h.set_scale(0.0)
            at0 = check("scale 0")
            assert np.array_equal(at0, before)
            h.set_scale(0.7)
        finally:
            h.detach()
        after = check("after detach")
        assert np.array_equal(after, before)
    finally:
        sd.close()


def test_a_bf16_engine_builds_no_fold_and_is_unchanged(synth):
    d = O.Dims(320, 8, 768, 8, 8, 64)
    sd = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=1))
    try:
        sd.load_weights(synth, clip=False, vae_encoder=False)
        lat, ctx = _unet_inputs(d)
        base, k0 = _forward(sd, 0, lat, 500, ctx)
        got, k1 = _forward(sd, 1, lat, 500, ctx)
        assert np.isfinite(got).all() and np.array_equal(base, got) and k0 == k1
    finally:
        sd.close()
