"""The SD 2.x variant on the GPU (sdmi_config.variant = 1), through the C ABI, against the CPU restatements of tests/sd2_ref.py: the UNet
with 64-wide heads at every level, the OpenCLIP text tower (exact GELU, padding with token 0), v-prediction on the default path, a k-sampler and img2img with a
mask, and the Stability checkpoint layout's round trip.  Every bar is a neighbouring module's: test_img2img_gpu's f32 / f64 rule for fp32 results (the GPU's error
against the f64 oracle judged against the f32 oracle's own), test_bf16_gpu's relative RMS for the bf16 UNet, test_prompt_gpu's for the text encoder."""
from pathlib import Path

import numpy as np
import pytest
import torch

import prompt_ref as R
import sd2_ref as S2
from oracle import clip_oracle as CO
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn
from stable_diffusion_burn_amd import weights as W
from test_bf16_gpu import BAR_UNET, _rel_rms
from test_img2img_gpu import _assert_close
from test_prompt_gpu import CTX, EOT, LONG, MINI, MINI_VOCAB, SOT, _close

pytestmark = pytest.mark.gpu

SDMI_ERR_INVALID, SDMI_ERR_WEIGHTS, SDMI_ERR_STATE = -1, -3, -6
TINY = O.Dims(64, 1, 96, 8, 8, 32)            # levels 64 / 128 / 256: 1 / 2 / 4 heads of 64 (n_head is ignored)
WIDE = O.Dims(320, 8, 768, 16, 16, 64)        # the bf16 configuration: 5 / 10 / 20 heads
TEXT = CO.ClipDims(n_vocab=MINI_VOCAB, n_state=128, n_head=2, n_ctx=CTX, n_layer=2)
TEXT_DIMS = O.Dims(64, 1, 128, 8, 8, 32)


def _config(d, precision=0, variant=1, **kw):
    from stable_diffusion_burn_amd import ModelConfig
    return ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=precision, variant=variant, **kw)


def _text_config(variant=1):
    return _config(TEXT_DIMS, variant=variant, clip_layers=TEXT.n_layer, clip_heads=TEXT.n_head, clip_vocab=MINI_VOCAB, clip_ctx=CTX)


@pytest.fixture(scope="module")
def sd2(synth):
    from stable_diffusion_burn_amd import StableDiffusion
    sd = StableDiffusion(_config(TINY))
    sd.load_weights(synth, clip=False)
    yield sd
    sd.close()


@pytest.fixture(scope="module")
def sd2_text(synth):
    from stable_diffusion_burn_amd import StableDiffusion
    sd = StableDiffusion(_text_config())
    sd.set_option("keep_masters", 1)
    sd.load_weights(synth)
    yield sd
    sd.close()


@pytest.fixture(scope="module")
def tok():
    from stable_diffusion_burn_amd import SimpleTokenizer
    return SimpleTokenizer(MINI)


def _inputs(d, n=2, T=7, Tu=3, seed=0):
    ctx = np.stack([syn.cond_context(i, T, d.ctx_dim) for i in range(n)])
    unc = syn.uncond_context(Tu, d.ctx_dim)
    rng = np.random.default_rng(900 + seed)
    z0 = (rng.standard_normal((n, 4, d.latent_h, d.latent_w)) * 0.8).astype(np.float32)
    noise = np.stack([syn.initial_latent(10 + i, d.latent_h, d.latent_w) for i in range(n)])
    return ctx, unc, z0, noise


# ---- the model variant -----------------------------------------------------------------------------------------------------------------------------------------------
def test_variant_context_plans_and_metadata(sd2):
    """the defaults of a variant context: attn_d64 = 2, and its three levels' attentions -- 64 / 16 / 4 tokens, 1 / 2 / 4 heads of 64 -- run on k_attn_split.hip;
    the full-width shapes go where the A/B sent them (profiles/r13a_attn_d64_ab.txt): the 256-token level of a batch-1 call stays on k_attn.hip"""
    for heads, tokens in ((1, 64), (2, 16), (4, 4), (4, 1)):
        for nk in (tokens, 7):
            assert sd2.attention_plan(2, heads, tokens, nk, 64)["kernel"] == "split", (heads, tokens, nk)
    for (tokens, heads), kernel in (((4096, 5), "split"), ((1024, 10), "split"), ((256, 20), "flash"), ((64, 20), "split")):
        for nk in (tokens, 77):
            assert sd2.attention_plan(2, heads, tokens, nk, 64)["kernel"] == kernel, (heads, tokens, nk)
    assert sd2.attention_plan(4, 20, 256, 256, 64)["kernel"] == "split"        # two images: k_attn.hip would need a second round of workgroups
    from stable_diffusion_burn_amd import SdmiError
    try:
        sd2.set_option("attn_d64", 0)
        assert sd2.attention_plan(2, 1, 64, 64, 64)["kernel"] == "flash"
        sd2.set_option("attn_d64", 1)
        assert sd2.attention_plan(2, 20, 256, 77, 64)["kernel"] == "split"
        with pytest.raises(SdmiError):
            sd2.set_option("attn_d64", 3)
        sd2.set_option("attn_d64", "default")
        assert sd2.attention_plan(2, 1, 64, 64, 64)["kernel"] == "split" and sd2.attention_plan(2, 20, 256, 77, 64)["kernel"] == "flash"
    finally:
        sd2.set_option("attn_d64", "default")
    for name, heads in (("unet/input_blocks/rt1/transformer/transformer/attn1/n_head", 1), ("unet/input_blocks/rt3/transformer/transformer/attn2/n_head", 2),
                        ("unet/middle_block/transformer/transformer/attn1/n_head", 4)):
        sd2.set_weight(name, np.array([heads], np.float32))          # metadata: must equal what the engine is built for
        with pytest.raises(SdmiError) as ei:
            sd2.set_weight(name, np.array([8], np.float32))
        assert ei.value.status == SDMI_ERR_WEIGHTS


@pytest.mark.parametrize("t", [999, 1])
def test_unet_forward(sd2, synth, t):
    d = TINY
    ctx, _, lat, _ = _inputs(d, seed=t)
    got = sd2.unet.forward(lat, [t], ctx)
    refs = [S2.UNetOracleV2(synth, d, dt).forward(torch.from_numpy(lat), t, torch.from_numpy(ctx)).numpy() for dt in (torch.float32, torch.float64)]
    e64, e32 = _assert_close(got, refs[0], refs[1], f"SD 2.x unet_forward t={t}")
    print(f"SD 2.x unet_forward t={t}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    v1 = O.UNetOracle(synth, d, torch.float64).forward(torch.from_numpy(lat), t, torch.from_numpy(ctx)).numpy()
    assert np.abs(v1 - refs[1]).max() > 100 * max(e64, 1e-6), "the head count does not reach the output: the test could not tell the variants apart"
    try:                                                             # the same model on k_attn.hip: the route a context without the option would take
        sd2.set_option("attn_d64", 0)
        _assert_close(sd2.unet.forward(lat, [t], ctx), refs[0], refs[1], f"SD 2.x unet_forward t={t}, attn_d64=0")
    finally:
        sd2.set_option("attn_d64", "default")


@pytest.fixture(scope="module")
def sd2_bf16(synth):
    from stable_diffusion_burn_amd import StableDiffusion
    sd = StableDiffusion(_config(WIDE, precision=1))
    sd.load_weights(synth, clip=False, vae_encoder=False)
    yield sd
    sd.close()


@pytest.mark.parametrize("t", [999, 1])
def test_unet_forward_bf16(sd2_bf16, synth, t):
    d = WIDE
    ctx, _, lat, _ = _inputs(d, seed=20)
    for heads, tokens in ((5, 256), (10, 64), (20, 16), (20, 4)):
        assert sd2_bf16.attention_plan(2, heads, tokens, tokens, 64)["kernel"] == "bf16"
    got = sd2_bf16.unet.forward(lat, [t], ctx)
    ref = S2.UNetOracleV2(syn.SyntheticWeights(), d, torch.float64).forward(torch.from_numpy(lat), t, torch.from_numpy(ctx)).numpy()
    r = _rel_rms(got, ref)
    print(f"SD 2.x bf16 unet_forward t={t}: rel-RMS vs fp64 = {r:.3e}")
    assert np.isfinite(got).all() and r < BAR_UNET
    from stable_diffusion_burn_amd import SdmiError
    with pytest.raises(SdmiError) as ei:                              # the query weights are packed pre-scaled: the option that decides it cannot change now
        sd2_bf16.set_option("attn_d64", 0)
    assert ei.value.status == SDMI_ERR_STATE
    sd2_bf16.set_option("attn_d64", 1)                                # (1 and 2 pack the same weights: allowed)
    sd2_bf16.set_option("attn_d64", "default")
    assert sd2_bf16.attention_plan(2, 5, 256, 256, 64)["kernel"] == "bf16"


# ---- the text tower ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,k", [("a photo of a cat", 1), (LONG, 2)])
def test_encode_prompt(sd2_text, tok, synth, text, k):
    clip64 = S2.OpenClipOracle(synth, TEXT, torch.float64)
    ids, w, rows = S2.prompt_chunks(tok.encode, SOT, EOT, text, CTX)
    assert ids.shape == (k, CTX) and (w == 1).all() and ids[-1, -1] == 0 and (ids == EOT).sum() == k
    got = sd2_text.encode_prompt(tok, text)
    assert got.shape == (1, k * CTX, TEXT.n_state)
    ref = R.clip_forward_ex(clip64, ids).numpy().reshape(1, k * CTX, -1)
    _close(got, ref, f"SD 2.x encode_prompt, {k} chunk(s)")
    np.testing.assert_array_equal(got[0].reshape(k, CTX, -1), sd2_text.clip.forward(ids))     # the padded positions hold token 0's embedding path
    bar = 2e-5 * max(1.0, np.abs(ref).max())
    ids_eot, _, _ = R.prompt_chunks(tok.encode, SOT, EOT, text, CTX)                          # SD v1's padding in the reference: must not pass
    assert np.abs(R.clip_forward_ex(clip64, ids_eot).numpy().reshape(ref.shape) - got).max() > 10 * bar
    quick = CO.CLIPOracle(synth, TEXT, torch.float64)                                          # QuickGELU in the reference: must not pass either
    assert np.abs(R.clip_forward_ex(quick, ids).numpy().reshape(ref.shape) - got).max() > 10 * bar
    for skip in (1, 2):
        _close(sd2_text.encode_prompt(tok, text, clip_skip=skip), R.clip_forward_ex(clip64, ids, clip_skip=skip).numpy().reshape(ref.shape), f"clip_skip {skip}")


def test_sd_v1_context_keeps_its_padding_and_gelu(synth, tok):
    """the same widths with variant = 0: <|endoftext|> padding and QuickGELU, as before"""
    from stable_diffusion_burn_amd import StableDiffusion
    sd = StableDiffusion(_text_config(variant=0))
    try:
        sd.load_weights(synth)
        ids, _, _ = R.prompt_chunks(tok.encode, SOT, EOT, "a photo of a cat", CTX)
        ref = R.clip_forward_ex(CO.CLIPOracle(synth, TEXT, torch.float64), ids).numpy()
        _close(sd.encode_prompt(tok, "a photo of a cat")[0][None], ref, "SD v1 encode_prompt at the same widths")
    finally:
        sd.close()


# ---- v-prediction --------------------------------------------------------------------------------------------------------------------------------------------------------
def _oracles(synth, prediction):
    a = syn.alphas_cumprod()
    return [S2.SD2Oracle(synth, a, TINY, dt, prediction) for dt in (torch.float32, torch.float64)]


def _half_mask(n, h, w):
    m = np.zeros((n, 1, h, w), np.float32)
    m[..., : w // 2 - 1] = 1.0
    m[..., w // 2 - 1] = 0.75
    m[..., w // 2] = 0.25
    return m


def test_v_prediction(sd2, synth):
    d, steps = TINY, 4
    ctx, unc, z0, x_T = _inputs(d, seed=5)
    mask = _half_mask(2, d.latent_h, d.latent_w)
    fresh = {"default": sd2.sample_latent(ctx, unc, 7.5, steps, init_latent=x_T),
             "from": sd2.sample_latent_from(ctx, unc, 7.5, steps, 0.75, z0, mask=mask, noise=x_T)}
    eps_refs = [S2.sample_latent_default(o, ctx, unc, 7.5, steps, x_T).numpy() for o in _oracles(synth, "eps")]
    _assert_close(fresh["default"], eps_refs[0], eps_refs[1], "SD 2.x sample_latent, eps")
    o32, o64 = _oracles(synth, "v")
    try:
        sd2.set_prediction("v")
        got = sd2.sample_latent(ctx, unc, 7.5, steps, init_latent=x_T)
        launches = sd2.last_call_stats()["kernels"]
        refs = [S2.sample_latent_default(o, ctx, unc, 7.5, steps, x_T).numpy() for o in (o32, o64)]
        _assert_close(got, refs[0], refs[1], "v-prediction, default path")
        assert np.abs(got - fresh["default"]).max() > 1e-2, "v and eps give the same latent: the setting does not reach the loop"

        sd2.set_ksampler("dpmpp_2m", schedule="karras")
        got = sd2.sample_latent(ctx, unc, 7.5, steps, init_latent=x_T)
        refs = [S2.sample_latent_k(o, ctx, unc, 7.5, steps, x_T, "dpmpp_2m", "karras").numpy() for o in (o32, o64)]
        _assert_close(got, refs[0], refs[1], "v-prediction, dpmpp_2m / karras")
        sd2.set_ksampler(None)

        got = sd2.sample_latent_from(ctx, unc, 7.5, steps, 0.75, z0, mask=mask, noise=x_T)
        refs = [S2.sample_latent_from(o, ctx, unc, 7.5, steps, 0.75, z0, x_T, mask).numpy() for o in (o32, o64)]
        _assert_close(got, refs[0], refs[1], "v-prediction, img2img with a mask")
        assert np.array_equal(got[..., -1], z0[..., -1])            # kept columns end exactly at z0
        assert sd2._lib.sdmi_set_prediction(sd2._ctx, 2) == SDMI_ERR_INVALID      # refused, and nothing changes
        with pytest.raises(ValueError):
            sd2.set_prediction("x0")
    finally:
        sd2.set_ksampler(None)
        sd2.set_prediction("eps")
    # eps again: the launches and the bits of a context that never left it
    np.testing.assert_array_equal(sd2.sample_latent(ctx, unc, 7.5, steps, init_latent=x_T), fresh["default"])
    assert sd2.last_call_stats()["kernels"] == launches, "v-prediction changes the launch count"
    np.testing.assert_array_equal(sd2.sample_latent_from(ctx, unc, 7.5, steps, 0.75, z0, mask=mask, noise=x_T), fresh["from"])


# ---- the checkpoint layout -------------------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_checkpoint_round_trip(sd2_text, synth, tok, tmp_path):
    from stable_diffusion_burn_amd import SdmiError, StableDiffusion, checkpoint_key, safetensors_model_family
    specs = sd2_text.weight_specs()
    shapes = dict(specs)
    fixture = {ln.split("\t")[0] for ln in (Path(__file__).parent / "golden" / "sd2_ckpt_keys.txt").read_text().splitlines()}
    missing = [n for n, _ in specs if n not in fixture]
    assert not missing, missing[:5]                                 # every tensor of a variant model has a line in the key list
    path, v1_path = tmp_path / "sd2.safetensors", tmp_path / "sd1.safetensors"
    get = lambda n, s: syn.named_tensor(synth, n, s, shapes)        # noqa: E731
    W.write_checkpoint_safetensors(path, specs, get, syn.alphas_cumprod(1000), variant=1,
                                   extra={"cond_stage_model.model.text_projection": np.zeros((4, 4), np.float32), "cond_stage_model.model.logit_scale": np.zeros((), np.float32),
                                          "cond_stage_model.model.transformer.resblocks.2.ln_1.weight": np.zeros(128, np.float32), "model_ema.decay": np.zeros((), np.float32)})
    W.write_checkpoint_safetensors(v1_path, specs, get, syn.alphas_cumprod(1000))
    assert safetensors_model_family(path) == "sd2" and safetensors_model_family(v1_path) == "sd1"
    sd = StableDiffusion(_text_config())
    v1 = StableDiffusion(_text_config(variant=0))
    try:
        sd.set_option("keep_masters", 1)
        with pytest.raises(SdmiError) as ei:                        # the other family: refused before anything is uploaded, the key named
            sd.load_weights_safetensors(v1_path)
        assert ei.value.status == SDMI_ERR_WEIGHTS and "cond_stage_model.transformer.text_model.final_layer_norm.weight" in str(ei.value)
        with pytest.raises(SdmiError) as ei:
            v1.load_weights_safetensors(path)
        assert ei.value.status == SDMI_ERR_WEIGHTS and "cond_stage_model.model.ln_final.weight" in str(ei.value)
        assert sd._lib.sdmi_finalize_weights(sd._ctx) != 0          # ... and nothing was: the context is still empty
        sd.load_weights_safetensors(path)
        checked = fused = 0
        for name, shape in specs:
            if not (len(shape) == 4 or (len(shape) == 2 and "embedding" not in name)):
                continue
            assert np.array_equal(_bits(sd.effective_weight(name)), _bits(sd2_text.effective_weight(name))), f"{name} ({checkpoint_key(name, 1, with_slice=True)})"
            checked += 1
            fused += checkpoint_key(name, 1, with_slice=True)[2] is not None
        assert checked > 300 and fused == 3 * TEXT.n_layer
        ctx, _, lat, _ = _inputs(TEXT_DIMS, seed=3)
        for fn in (lambda s: s.unet.forward(lat, [500], ctx), lambda s: s.autoencoder.decode_latent(lat[:1]), lambda s: s.encode_prompt(tok, LONG),
                   lambda s: s.clip.forward(np.arange(2 * CTX, dtype=np.int32).reshape(2, CTX))):
            a, b = fn(sd), fn(sd2_text)
            assert np.isfinite(a).all() and np.abs(a).max() > 0 and np.array_equal(_bits(a), _bits(b))      # biases (the fused in_proj_bias included), norms, tables
    finally:
        sd.close()
        v1.close()
