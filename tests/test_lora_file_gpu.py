"""kohya-ss / LyCORIS LoRA files on the device (include/sdmi.h "LoRA adapters"; DESIGN.md section 9c "files").

What is pinned here: a file attach is, bit for bit, sdmi_lora_add of the host-widened factors -- in F32, F16 and BF16, so the merge kernel's widening is exact and
its F32 path kept its bits; LoHa against the float64 merge within a derived rounding bound (tests/lora_file_ref.py: merge_bound, never a measured number);
re-packing and reversibility at every precision with separate UNet / text-encoder scales; parity of an adapted model against the oracle running the merged
weights; every refusal on a live context, each leaving it unchanged; the multi-device surface.

Contexts are built once per module (tiny dims at precision 0, 320 channels at precision 1 / 2, each with a one-layer text encoder) and every test leaves them
without adapters.
"""
import numpy as np
import pytest
import torch

import lora_file_ref as R
import lora_ref as L
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import ModelConfig, MultiStableDiffusion, SdmiError, StableDiffusion
from stable_diffusion_burn_amd import synthetic as syn
from stable_diffusion_burn_amd import weights as W
from test_model_gpu import _assert_close

pytestmark = pytest.mark.gpu

WIDE = O.Dims(320, 8, 768, 8, 8, 64)          # precision 1 / 2 need channel counts that are multiples of 64 (as test_lora_gpu)
ERR_WEIGHTS, ERR_UNSUPPORTED, ERR_STATE = -3, -5, -6
FC1, FC2, TEQ = "clip/blocks/0/mlp/fc1/weight", "clip/blocks/0/mlp/fc2/weight", "clip/blocks/0/attn/query/weight"
CLIP_VOCAB, CLIP_CTX = 48, 8
TOKENS = np.array([[1, 5, 7, 11, 40, 3, 2, 47]], np.int32)


def _dims(precision, tiny_dims):
    return tiny_dims if precision == 0 else WIDE


def _config(d, precision=0):
    return ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=precision, clip_layers=1, clip_heads=d.ctx_dim // 64,
                       clip_vocab=CLIP_VOCAB, clip_ctx=CLIP_CTX)


@pytest.fixture(scope="module")
def contexts(synth, tiny_dims):
    """precision -> a loaded context that keeps its masters, with the one-layer text encoder; built on first use"""
    made = {}

    def get(precision):
        if precision not in made:
            sd = StableDiffusion(_config(_dims(precision, tiny_dims), precision))
            sd.set_option("keep_masters", 1)
            sd.load_weights(synth, clip=True, vae_encoder=False)
            made[precision] = sd
        return made[precision]

    yield get
    for sd in made.values():
        sd.close()


def _forward(sd, d, t=500):
    lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 7, d.ctx_dim) for i in range(2)])
    return sd.unet.forward(lat, [t], ctx)


def _w0(sd, synth, name):
    shapes = dict(sd.weight_specs())
    return syn.named_tensor(synth, name, shapes[name], shapes)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _api_form(adapter):
    """what lora_attach takes: an absent alpha is the rank"""
    return {n: (d, u, float(d.shape[0]) if a is None else a) for n, (d, u, a) in adapter.items()}


def _file_targets(d):
    """lora_ref.arithmetic_targets -- Cc = 36, R = 4, ranks 1 / 3 / 4 / 16 / 33; the rank-3 targets give up factors [out][3] whose 16-bit rows are 6 bytes, so every
    other row starts off a 4-byte boundary (every `in` of the model is even, so a down row cannot) -- plus a text-encoder Linear"""
    t = dict(L.arithmetic_targets(d))
    t[FC1] = ((d.ctx_dim, 4 * d.ctx_dim), 2)
    return t


def _adapter_without_one_alpha(d, seed):
    ad = L.make_adapter(_file_targets(d), seed)
    name = L.TB + "/attn1/value/weight"
    ad[name] = ad[name][:2] + (None,)              # no "alpha" key in the file: alpha = rank
    return ad


def sd_name(name):
    from stable_diffusion_burn_amd import lora_module_name
    return lora_module_name(name)


def _effective(sd, names):
    return {n: sd.effective_weight(n) for n in names}


def test_file_equals_api_f32(contexts, tiny_dims, tmp_path):
    """Test 1.  An F32 kohya file == lora_attach of the same factors, bit for bit, on every target: the F32 path of the merge kept its bits."""
    sd, d = contexts(0), tiny_dims
    ad = _adapter_without_one_alpha(d, 71)
    W.write_lora_safetensors(tmp_path / "f32.safetensors", ad, dtype="F32")
    a = sd.lora_load_safetensors(tmp_path / "f32.safetensors", scale=0.7)
    try:
        assert a.n_targets == len(ad) and a.n_skipped == 0 and a.scale == 0.7
        assert a.factor_bytes >= sum(dn.nbytes + up.nbytes for dn, up, _ in ad.values())
        from_file = _effective(sd, ad)
    finally:
        a.detach()
    b = sd.lora_attach(_api_form(ad), scale=0.7)
    try:
        from_api = _effective(sd, ad)
    finally:
        b.detach()
    for n in ad:
        assert _same(from_file[n], from_api[n]), n
        assert not _same(from_file[n], sd.effective_weight(n)), n          # ... and the adapter was in it


def _odd_offset_copy(src, dst):
    """the same file with one more space behind the header: the data section starts at an odd file offset"""
    data = src.read_bytes()
    n = int.from_bytes(data[:8], "little")
    assert (8 + n) % 2 == 0
    dst.write_bytes((n + 1).to_bytes(8, "little") + data[8:8 + n] + b" " + data[8 + n:])
    return dst


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
def test_half_precision_factors_equal_the_widened_api(contexts, tiny_dims, tmp_path, dtype):
    """Test 2.  The file in F16 / BF16 == lora_attach of the host-widened factors, bit for bit: the widening in the staging loops is exact, 6-byte factor rows
    included; and the same from a file whose data section starts at an odd offset."""
    sd, d = contexts(0), tiny_dims
    ad = _adapter_without_one_alpha(d, 72)
    W.write_lora_safetensors(tmp_path / "h.safetensors", ad, dtype=dtype)
    widened = _api_form(R.stored_adapter(ad, dtype))
    assert any(not np.array_equal(widened[n][0], ad[n][0]) for n in ad)     # the rounding to 16 bits did change the factors
    b = sd.lora_attach(widened, scale=-1.1)
    try:
        from_api = _effective(sd, ad)
    finally:
        b.detach()
    for path in (tmp_path / "h.safetensors", _odd_offset_copy(tmp_path / "h.safetensors", tmp_path / "odd.safetensors")):
        a = sd.lora_load_safetensors(path, scale=-1.1)
        try:
            assert a.n_targets == len(ad)
            # the raw 16-bit factors: half of what lora_attach holds (+ at most 15 bytes of padding per factor)
            assert a.factor_bytes <= sum(dn.nbytes + up.nbytes for dn, up, _ in ad.values()) // 2 + 32 * len(ad)
            from_file = _effective(sd, ad)
        finally:
            a.detach()
        for n in ad:
            assert _same(from_file[n], from_api[n]), (path.name, n)


def _loha_targets(d):
    """a Linear at rank 33 and 1, a 1x1 and a 3x3 convolution, the text encoder, and the R = 4 conv_out"""
    c, cd = d.model_channels, d.ctx_dim
    return {
        L.TB + "/attn1/query/weight": ((c, c), 33),
        L.TB + "/attn2/key/weight": ((cd, c), 1),
        L.TB + "/mlp/geglu/proj/weight": ((c, 8 * c), 5),
        L.ST + "/proj_in/weight": ((c, c, 1, 1), 4),
        "unet/input_blocks/rt1/res/conv_in/weight": ((c, c, 3, 3), 3),
        "unet/input_blocks/conv/weight": ((c, 4, 3, 3), 2),              # Cc = 36
        "unet/conv_out/weight": ((4, c, 3, 3), 33),                       # R = 4
        FC2: ((4 * cd, cd), 16),
    }


def _check_merge(sd, synth, name, terms, what=""):
    w0 = _w0(sd, synth, name)
    got = sd.effective_weight(name)
    exact, bound = R.merge_f64(w0, terms), R.merge_bound(w0, terms)
    err = np.abs(got.astype(np.float64) - exact)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}{name} {tuple(w0.shape)}: max |got - exact| = {err.max():.3e}, worst err / bound = {worst:.3f}")
    assert got.shape == w0.shape and np.isfinite(got).all()
    assert (err <= bound).all(), f"{name}: merge error exceeds the rounding bound (worst ratio {worst:.3f})"
    assert np.abs(got - w0).max() > 1e-3 * np.abs(w0).max(), f"{name}: the merge changed nothing"


@pytest.mark.parametrize("dtype", ["F32", "F16"])
def test_loha_against_the_f64_merge(contexts, synth, tiny_dims, tmp_path, dtype):
    """Test 3.  LoHa modules on every kind of target against W0 + c (w1_a w1_b) o (w2_a w2_b) in float64, within lora_file_ref.merge_bound."""
    sd, d = contexts(0), tiny_dims
    ad = R.make_loha(_loha_targets(d), 81)
    W.write_lora_safetensors(tmp_path / "loha.safetensors", ad, dtype=dtype)
    held = R.stored_adapter(ad, dtype)
    a = sd.lora_load_safetensors(tmp_path / "loha.safetensors", scale=0.8)
    try:
        assert a.n_targets == len(ad)
        for n in ad:
            _check_merge(sd, synth, n, [R.loha_terms(held[n], 0.8)], f"LoHa {dtype} ")
        again = sd.effective_weight(FC2)
        assert _same(again, sd.effective_weight(FC2))                     # deterministic run to run
    finally:
        a.detach()
    for n in ad:
        assert _same(sd.effective_weight(n), _w0(sd, synth, n)), n


def test_loha_stacks_with_plain_adapters_and_continues_in_place(contexts, synth, tiny_dims, tmp_path):
    """Test 3, stacking.  A LoHa and a plain adapter on one target, attached in both orders (two launches: a launch holds one kind), a plain F32 API adapter between
    two F16 file adapters, and nine LoHa terms on one tensor (more than one launch takes): all within the bound of the terms in attach order."""
    sd, d = contexts(0), tiny_dims
    c, cd = d.model_channels, d.ctx_dim
    q, k = L.TB + "/attn1/query/weight", L.TB + "/attn2/key/weight"
    loha = R.make_loha({q: ((c, c), 6)}, 91)
    plain = L.make_adapter({q: ((c, c), 17)}, 92)
    W.write_lora_safetensors(tmp_path / "loha.safetensors", loha, dtype="F16")
    W.write_lora_safetensors(tmp_path / "plain.safetensors", plain, dtype="F16")
    h_loha, h_plain = R.stored_adapter(loha, "F16"), R.stored_adapter(plain, "F16")
    t_loha, t_plain = R.loha_terms(h_loha[q], 0.6), R.plain_terms(h_plain[q], -0.9)
    base = _forward(sd, d)
    for order in ("loha first", "plain first"):
        live = []
        try:
            for which in (("loha", "plain") if order == "loha first" else ("plain", "loha")):
                live.append(sd.lora_load_safetensors(tmp_path / f"{which}.safetensors", scale=0.6 if which == "loha" else -0.9))
            _check_merge(sd, synth, q, [t_loha, t_plain] if order == "loha first" else [t_plain, t_loha], order + ": ")
        finally:
            for a in reversed(live):
                a.detach()
    # F16 file, F32 API, F16 file on one tensor: three launches that continue in place
    api = L.make_adapter({q: ((c, c), 3)}, 93)
    live = []
    try:
        live.append(sd.lora_load_safetensors(tmp_path / "plain.safetensors", scale=-0.9))
        live.append(sd.lora_attach(api, scale=0.4))
        live.append(sd.lora_load_safetensors(tmp_path / "loha.safetensors", scale=0.6))
        _check_merge(sd, synth, q, [t_plain, R.plain_terms(api[q], 0.4), t_loha], "mixed dtypes: ")
    finally:
        for a in reversed(live):
            a.detach()
    # nine LoHa terms
    ads = [R.make_loha({k: ((cd, c), 1 + i % 3)}, 100 + i) for i in range(9)]
    scales = [0.3 + 0.1 * i for i in range(9)]
    live = []
    try:
        for i, (ad, s) in enumerate(zip(ads, scales)):
            W.write_lora_safetensors(tmp_path / f"nine{i}.safetensors", ad, dtype="F32")
            live.append(sd.lora_load_safetensors(tmp_path / f"nine{i}.safetensors", scale=s))
        _check_merge(sd, synth, k, [R.loha_terms(ad[k], s) for ad, s in zip(ads, scales)], "nine LoHa terms: ")
        assert not _same(_forward(sd, d), base)
    finally:
        for a in reversed(live):
            a.detach()
    assert _same(_forward(sd, d), base)


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_repack_reversibility_and_the_two_scales(contexts, synth, tiny_dims, tmp_path, precision):
    """Test 4.  After a file attach the packed state is what sdmi_set_weight of the effective fp32 tensors packs (the comparison of test_repack_is_the_load_path: the same
    forward, bit for bit); detach() restores the loaded model; the UNet scale and the text-encoder scale each move only their half."""
    d = _dims(precision, tiny_dims)
    sd = contexts(precision)
    c, cd = d.model_channels, d.ctx_dim
    plain = L.make_adapter({**L.repack_targets(d), TEQ: ((cd, cd), 4)}, 111)
    loha = R.make_loha({"unet/input_blocks/rt1/res/conv_in/weight": ((c, c, 3, 3), 3), FC2: ((4 * cd, cd), 2)}, 112)
    W.write_lora_safetensors(tmp_path / "both.safetensors", {**plain, **loha}, dtype="F16")
    names = list(plain) + list(loha)
    base_u, base_c = _forward(sd, d), sd.clip.forward(TOKENS)
    a = sd.lora_load_safetensors(tmp_path / "both.safetensors", scale=0.9, te_scale=0.6)
    try:
        assert a.scale == (0.9, 0.6) and a.te.n_targets == 2 and a.unet.n_targets == len(names) - 2
        out_u, out_c = _forward(sd, d), sd.clip.forward(TOKENS)
        eff = _effective(sd, names)
        a.set_scale(0.9, 0.0)
        assert _same(sd.clip.forward(TOKENS), base_c) and _same(_forward(sd, d), out_u)        # te_scale = 0: the text encoder is the loaded one
        a.set_scale(0.0, 0.6)
        assert _same(_forward(sd, d), base_u) and _same(sd.clip.forward(TOKENS), out_c)        # scale = 0: the UNet is the loaded one
    finally:
        a.detach()
    print(f"precision {precision}: max |adapted - base| unet {np.abs(out_u - base_u).max():.3e}, clip {np.abs(out_c - base_c).max():.3e}")
    assert np.isfinite(out_u).all() and np.isfinite(out_c).all() and not _same(out_u, base_u) and not _same(out_c, base_c)
    assert _same(_forward(sd, d), base_u) and _same(sd.clip.forward(TOKENS), base_c)            # detached: the loaded model, bit for bit
    try:
        for n, w in eff.items():
            sd.set_weight(n, w)
        assert sd._lib.sdmi_finalize_weights(sd._ctx) == 0
        set_u, set_c = _forward(sd, d), sd.clip.forward(TOKENS)
    finally:
        for n in names:
            sd.set_weight(n, _w0(sd, synth, n))
        assert sd._lib.sdmi_finalize_weights(sd._ctx) == 0
    assert _same(set_u, out_u) and _same(set_c, out_c)
    assert _same(_forward(sd, d), base_u) and _same(sd.clip.forward(TOKENS), base_c)


def test_parity_of_a_model_adapted_from_a_file(contexts, synth, tiny_dims, tmp_path):
    """Test 5.  lora_ref.parity_targets as an F16 kohya file plus LoHa modules on ResBlock convolutions: unet.forward at t = 999 / 49 against the f32 / f64 oracles
    running the merged weights of the 16-bit-rounded factors, at test_parity_of_an_adapted_model_fp32's bar (atol 1e-4); the un-adapted forward misses that bar."""
    d, sd = tiny_dims, contexts(0)
    shapes = dict(sd.weight_specs())
    plain = L.make_adapter(L.parity_targets(d), L.PARITY_SEED)
    loha_names = ["unet/input_blocks/rt1/res/conv_in/weight", "unet/input_blocks/rt5/res/conv_in/weight", "unet/middle_block/res2/conv_out/weight",
                  "unet/output_blocks/rt7/res/conv_in/weight"]
    loha = R.make_loha({n: (shapes[n], 4) for n in loha_names}, L.PARITY_SEED + 1)
    assert not set(loha) & set(plain)
    ad = {**plain, **loha}
    W.write_lora_safetensors(tmp_path / "parity.safetensors", ad, dtype="F16")
    prov = R.FileLoraProvider(synth, [(R.stored_adapter(ad, "F16"), L.PARITY_SCALE)])
    acp = syn.alphas_cumprod()
    o32, o64 = O.StableDiffusionOracle(prov, acp, d, torch.float32), O.StableDiffusionOracle(prov, acp, d, torch.float64)
    lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 7, d.ctx_dim) for i in range(2)])
    base = {t: sd.unet.forward(lat, [t], ctx) for t in (999, 49)}
    a = sd.lora_load_safetensors(tmp_path / "parity.safetensors", scale=L.PARITY_SCALE, skip_unknown=False)
    try:
        assert a.n_targets == len(ad)
        got = {t: sd.unet.forward(lat, [t], ctx) for t in (999, 49)}
    finally:
        a.detach()
    tl, tc = torch.from_numpy(lat), torch.from_numpy(ctx)
    for t in (999, 49):
        r32, r64 = o32.unet.forward(tl, t, tc).numpy(), o64.unet.forward(tl, t, tc).numpy()
        e64, e32 = _assert_close(got[t], r32, r64, f"file-adapted unet_forward t={t}", atol=1e-4)
        miss = float(np.abs(base[t].astype(np.float64) - r64).max())
        print(f"file-adapted unet t={t}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}; the un-adapted forward is {miss:.3e} away")
        assert miss > 100 * max(1e-4, 2 * e32)                                                      # the bar cannot be met without the adapter


def test_refusals_on_a_live_context(contexts, synth, tiny_dims, tmp_path):
    """Test 6.  Each refused file leaves effective_weight and the forward as they were, and no adapter behind."""
    d, sd = tiny_dims, contexts(0)
    c = d.model_channels
    q, conv = L.TB + "/attn1/query/weight", "unet/input_blocks/rt1/res/conv_in/weight"
    good = L.make_adapter({q: ((c, c), 4), conv: ((c, c, 3, 3), 3)}, 121)
    mq, mconv = sd_name(q), sd_name(conv)
    base, w_q, w_conv = _forward(sd, d), sd.effective_weight(q), sd.effective_weight(conv)

    ok = {}                                                       # the file's tensors, key by key: the Linear module first, the convolution last
    for name, (down, up, alpha) in good.items():
        m = sd_name(name)
        ok[m + ".lora_down.weight"] = down.astype(np.float16)
        ok[m + ".lora_up.weight"] = up.reshape(up.shape + (1, 1) if down.ndim == 4 else up.shape).astype(np.float16)
        ok[m + ".alpha"] = np.float16(alpha)
    z = np.zeros((4, 4), np.float16)
    cases = {
        "an unsupported key": ({**ok, mq + ".dora_scale": z}, ERR_UNSUPPORTED, mq + ".dora_scale"),
        "a Tucker core": ({**ok, mconv + ".lora_mid.weight": z}, ERR_UNSUPPORTED, mconv + ".lora_mid.weight"),
        # the conv module is the LAST of the file: the Linear before it is fine and must not stay attached
        "a shape error in the last module": ({**ok, mconv + ".lora_up.weight": np.zeros((c, 2, 1, 1), np.float16)}, ERR_WEIGHTS, mconv + ".lora_up.weight"),
        "a rank of 257": ({mq + ".lora_down.weight": np.zeros((257, c), np.float16), mq + ".lora_up.weight": np.zeros((c, 257), np.float16)}, ERR_UNSUPPORTED, "257"),
        "an unknown module": ({**ok, "lora_te_text_model_encoder_layers_1_mlp_fc1.lora_down.weight": z, "lora_te_text_model_encoder_layers_1_mlp_fc1.lora_up.weight": z},
                              ERR_UNSUPPORTED, "layers_1_mlp_fc1"),
    }
    assert list(cases["a shape error in the last module"][0])[-1].startswith(mconv) and list(ok)[0].startswith(mq)
    for what, (ts, status, needle) in cases.items():
        W.write_safetensors(tmp_path / "bad.safetensors", ts)
        with pytest.raises(SdmiError) as ei:
            sd.lora_load_safetensors(tmp_path / "bad.safetensors", scale=1.0)
        assert ei.value.status == status and needle in str(ei.value), (what, str(ei.value))
        assert _same(sd.effective_weight(q), w_q) and _same(sd.effective_weight(conv), w_conv), what
    assert _same(_forward(sd, d), base)
    # the unknown module is skipped on request, and reported
    W.write_safetensors(tmp_path / "bad.safetensors", cases["an unknown module"][0])
    a = sd.lora_load_safetensors(tmp_path / "bad.safetensors", scale=1.0, skip_unknown=True)
    try:
        assert a.n_targets == 2 and a.n_skipped == 1 and not _same(sd.effective_weight(q), w_q)
    finally:
        a.detach()
    assert _same(_forward(sd, d), base)


def test_refusals_that_need_another_context(synth, tiny_dims, tmp_path):
    """Test 6, continued.  No keep_masters: SDMI_ERR_STATE.  A padded (9-channel) conv_in: SDMI_ERR_UNSUPPORTED.  A context whose text encoder is not loaded: its
    modules are SDMI_ERR_STATE, or skipped on request.  Nothing changes in any of them."""
    d = tiny_dims
    c = d.model_channels
    q = L.TB + "/attn1/query/weight"
    ad = L.make_adapter({q: ((c, c), 4), FC1: ((d.ctx_dim, 4 * d.ctx_dim), 2)}, 131)
    W.write_lora_safetensors(tmp_path / "a.safetensors", ad, dtype="F16")
    # no masters
    sd = StableDiffusion(_config(d))
    try:
        sd.load_weights(synth, clip=True, vae_encoder=False)
        base = _forward(sd, d)
        with pytest.raises(SdmiError) as ei:
            sd.lora_load_safetensors(tmp_path / "a.safetensors")
        assert ei.value.status == ERR_STATE and "keep_masters" in str(ei.value)
        assert _same(_forward(sd, d), base)
    finally:
        sd.close()
    # masters, but the text encoder's weights were never loaded
    sd = StableDiffusion(_config(d))
    try:
        sd.set_option("keep_masters", 1)
        sd.load_weights(synth, clip=False, vae_encoder=False)
        base, w_q = _forward(sd, d), sd.effective_weight(q)
        with pytest.raises(SdmiError) as ei:
            sd.lora_load_safetensors(tmp_path / "a.safetensors")
        assert ei.value.status == ERR_STATE and FC1 in str(ei.value)
        assert _same(sd.effective_weight(q), w_q)
        a = sd.lora_load_safetensors(tmp_path / "a.safetensors", skip_unknown=True)
        try:
            assert a.n_targets == 1 and a.n_skipped == 1 and not _same(sd.effective_weight(q), w_q)
        finally:
            a.detach()
        assert _same(_forward(sd, d), base)
    finally:
        sd.close()
    # an inpainting UNet: its 9-channel conv_in is packed padded to 12
    import dataclasses
    sd = StableDiffusion(dataclasses.replace(_config(d), unet_in_ch=9))
    try:
        sd.set_option("keep_masters", 1)
        sd.load_weights(synth, clip=False, vae_encoder=False)
        name = "unet/input_blocks/conv/weight"
        w = sd.effective_weight(name)
        assert w.shape == (c, 9, 3, 3)
        pad = L.make_adapter({q: ((c, c), 4)}, 132)
        pad[name] = (np.zeros((2, 9, 3, 3), np.float32), np.zeros((c, 2), np.float32), 1.0)
        W.write_lora_safetensors(tmp_path / "pad.safetensors", pad, dtype="F16")
        w_q = sd.effective_weight(q)
        with pytest.raises(SdmiError) as ei:
            sd.lora_load_safetensors(tmp_path / "pad.safetensors", skip_unknown=True)
        assert ei.value.status == ERR_UNSUPPORTED and "conv_in" in str(ei.value)
        assert _same(sd.effective_weight(q), w_q) and _same(sd.effective_weight(name), w)
    finally:
        sd.close()


def test_multi_device_surface(synth, tiny_dims, tmp_path):
    """MultiStableDiffusion((0,)): lora_load_safetensors changes sample_image, detach restores it bit for bit."""
    d = tiny_dims
    ad = {**L.make_adapter(L.parity_targets(d), L.PARITY_SEED), **R.make_loha({"unet/input_blocks/rt1/res/conv_in/weight": ((d.model_channels, d.model_channels, 3, 3), 4)}, 141)}
    W.write_lora_safetensors(tmp_path / "m.safetensors", ad, dtype="BF16")
    m = MultiStableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch), devices=(0,))
    try:
        m.device_view(0).set_option("keep_masters", 1)
        m.load_weights(synth)
        ctx, unc = syn.cond_context(0, 7, d.ctx_dim), syn.uncond_context(2, d.ctx_dim)
        lat = syn.initial_latent(0, d.latent_h, d.latent_w)[None]
        before = m.sample_image(ctx, unc, 7.5, 2, 1, init_latents=lat)
        a = m.lora_load_safetensors(tmp_path / "m.safetensors", scale=1.0)
        try:
            assert a.scale == 1.0
            adapted = m.sample_image(ctx, unc, 7.5, 2, 1, init_latents=lat)
        finally:
            a.detach()
        after = m.sample_image(ctx, unc, 7.5, 2, 1, init_latents=lat)
        assert not np.array_equal(adapted, before)
        assert np.array_equal(after, before)
    finally:
        m.close()


def test_sample_cli_attaches_a_file(synth, tmp_path):
    """sdmi_sample with SDMI_LORA=<file>:<scale>:<te_scale> writes the PNG of the same calls through Python, byte for byte (it sets keep_masters itself), and a file it
    cannot attach ends it with the loader's message."""
    import ctypes as C
    import os
    import subprocess
    from pathlib import Path

    from stable_diffusion_burn_amd import SimpleTokenizer, build
    from stable_diffusion_burn_amd._capi import check
    mini = Path(__file__).parent / "golden" / "mini_merges.txt"
    vocab = 512 + 264 + 2
    sd = StableDiffusion(ModelConfig(160, 4, 64, 16, 16, 32, clip_layers=2, clip_heads=1, clip_vocab=vocab, clip_ctx=16))
    try:
        sd.set_option("keep_masters", 1)
        sd.load_weights(synth)
        specs = sd.weight_specs()
        shapes = dict(specs)
        W.write_dump_tree(tmp_path / "params", specs, lambda name, shape: syn.named_tensor(synth, name, shape, shapes), syn.alphas_cumprod(), n_head=4, clip_heads=1)
        te = "clip/blocks/1/mlp/fc1/weight"
        q = L.TB + "/attn1/query/weight"
        ad = {**L.make_adapter({q: (shapes[q], 4), te: (shapes[te], 2)}, 151, rel=0.5), **R.make_loha({"unet/input_blocks/rt1/res/conv_in/weight": ((160, 160, 3, 3), 3)}, 152, rel=0.5)}
        W.write_lora_safetensors(tmp_path / "cli.safetensors", ad, dtype="F16")
        env = dict(os.environ, SDMI_BPE_VOCAB=str(mini), SDMI_SEED="3",
                   SDMI_CONFIG=f"model_channels=160,n_head=4,ctx_dim=64,latent_h=16,latent_w=16,vae_ch=32,clip_layers=2,clip_heads=1,clip_vocab={vocab},clip_ctx=16")
        for k in ("SDMI_PROMPT_STYLE", "SDMI_NEGATIVE_PROMPT", "SDMI_CLIP_SKIP", "SDMI_LORA"):
            env.pop(k, None)

        def run(out, **extra):
            return subprocess.run([str(build.CLI), "dump", str(tmp_path / "params"), "7.5", "2", "a photo of a cat", str(out), "hip:0"], env=dict(env, **extra),
                                  capture_output=True, text=True, timeout=300)

        def png(img, path):
            check(sd._lib.sdmi_write_png(str(path).encode(), img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[1], img.shape[0]))
            return Path(path).read_bytes()

        tok = SimpleTokenizer(mini)
        plain = np.ascontiguousarray(sd.sample_image(sd.context(tok, "a photo of a cat"), sd.unconditional_context(tok), 7.5, 2, seed=3)[0])
        r = run(tmp_path / "with", SDMI_LORA=f"{tmp_path / 'cli.safetensors'}:0.8:0.5")
        assert r.returncode == 0 and "LoRA" in r.stdout, r.stderr
        a = sd.lora_load_safetensors(tmp_path / "cli.safetensors", scale=0.8, te_scale=0.5)
        try:
            ref = np.ascontiguousarray(sd.sample_image(sd.context(tok, "a photo of a cat"), sd.unconditional_context(tok), 7.5, 2, seed=3)[0])
        finally:
            a.detach()
        assert not np.array_equal(ref, plain)
        assert (tmp_path / "with0.png").read_bytes() == png(ref, tmp_path / "with_ref.png")
        r = run(tmp_path / "without")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "without0.png").read_bytes() == png(plain, tmp_path / "plain_ref.png")
        W.write_safetensors(tmp_path / "bad.safetensors", {"lora_unet_conv_out.dora_scale": np.zeros(4, np.float16)})
        r = run(tmp_path / "bad", SDMI_LORA=str(tmp_path / "bad.safetensors"))
        assert r.returncode == 1 and "Error loading LoRA" in r.stderr and "dora_scale" in r.stderr
    finally:
        sd.close()
