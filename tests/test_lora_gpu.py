"""LoRA adapters merged into the packed weights on the device (include/sdmi.h "LoRA adapters").

What is pinned here: the merge kernel's arithmetic against a derived rounding bound (never a measured one), that a re-merge packs exactly what
the loader packs at every precision, that scale 0 / detach give the loaded model back bit for bit, parity of an adapted model against the oracle
running the merged weights at test_model_gpu's own bars, stacking, every status code of the header, and the multi-device surface.

Contexts are built once per module and shared (the full-width loads are the expensive part); every test leaves them without adapters.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lora_ref as L
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import ModelConfig, MultiStableDiffusion, SdmiError, StableDiffusion
from stable_diffusion_burn_amd import synthetic as syn
from test_model_gpu import _assert_close

pytestmark = pytest.mark.gpu

WIDE = O.Dims(320, 8, 768, 8, 8, 64)          # precision 1 / 2 need channel counts that are multiples of 64 (as test_shared_cfg_prefix_equals_two_full_forwards)
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -5, -6


def _dims(precision, tiny_dims):
    return tiny_dims if precision == 0 else WIDE


def _new(d, precision, masters):
    sd = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=precision))
    if masters:
        sd.set_option("keep_masters", 1)
    return sd


@pytest.fixture(scope="module")
def contexts(synth, tiny_dims):
    """(precision, masters) -> a loaded context, built on first use"""
    made = {}

    def get(precision, masters):
        key = (precision, bool(masters))
        if key not in made:
            sd = _new(_dims(precision, tiny_dims), precision, masters)
            sd.load_weights(synth, clip=False, vae_encoder=False)
            made[key] = sd
        return made[key]

    yield get
    for sd in made.values():
        sd.close()


def _unet_inputs(d):
    lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 7, d.ctx_dim) for i in range(2)])
    return lat, ctx


def _forward(sd, d, t=500):
    lat, ctx = _unet_inputs(d)
    return sd.unet.forward(lat, [t], ctx)


def _w0(sd, synth, name):
    shapes = dict(sd.weight_specs())
    return syn.named_tensor(synth, name, shapes[name], shapes)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_merge(sd, synth, name, adapters):
    """effective_weight(name) against the f64 merge within the derived bound; adapters = [(tensors, scale)] in attach order"""
    w0 = _w0(sd, synth, name)
    terms = [(t[name][0], t[name][1], L.coef(s, t[name][2], t[name][0].shape[0])) for t, s in adapters if name in t]
    got = sd.effective_weight(name)
    exact, bound = L.merge_f64(w0, terms), L.merge_bound(w0, terms)
    err = np.abs(got.astype(np.float64) - exact)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{name} {tuple(w0.shape)} ranks {[t[0].shape[0] for t in terms]}: max |got - exact| = {err.max():.3e}, worst err / bound = {worst:.3f}")
    assert got.shape == w0.shape and np.isfinite(got).all()
    assert (err <= bound).all(), f"{name}: merge error exceeds the rounding bound (worst ratio {worst:.3f})"
    assert np.abs(got - w0).max() > 1e-3 * np.abs(w0).max(), f"{name}: the merge changed nothing"


def test_merge_arithmetic(contexts, synth, tiny_dims):
    """Test 1.  One adapter over every kind of target (Cc = 36 conv_in, 3x3 and 1x1 convolutions, the packed q | k | v members, the cross-attention key
    [64, 160], GEGLU [160, 1280], the fp32 time-embedding Linear) with ranks 1, 3, 4, 16, 33; a second one of rank 5 on two of them; scales 0.7 and -1.3."""
    sd, d = contexts(0, True), tiny_dims
    t1 = L.arithmetic_targets(d)
    assert sorted({r for _, r in t1.values()}) == [1, 3, 4, 16, 33]
    two = ["unet/input_blocks/conv/weight", L.TB + "/attn1/query/weight"]
    ad1, ad2 = L.make_adapter(t1, 21), L.make_adapter({n: (t1[n][0], 5) for n in two}, 22)
    untouched = [L.TB + "/attn1/out/weight", "unet/middle_block/res1/conv_in/weight", "unet/lin2_time_embed/weight"]
    a1 = sd.lora_attach(ad1, scale=0.7)
    a2 = sd.lora_attach(ad2, scale=-1.3)
    try:
        assert a1.scale == 0.7 and a2.scale == -1.3 and a1.n_targets == len(t1) and a2.n_targets == 2
        for name in t1:
            _check_merge(sd, synth, name, [(ad1, 0.7), (ad2, -1.3)])
        for name in untouched:
            assert np.array_equal(_bits(sd.effective_weight(name)), _bits(_w0(sd, synth, name))), name
        # deterministic run to run
        again = sd.effective_weight(two[1])
        assert np.array_equal(_bits(again), _bits(sd.effective_weight(two[1])))
    finally:
        a2.detach()
        a1.detach()
    for name in list(t1)[:3] + untouched[:1]:
        assert np.array_equal(_bits(sd.effective_weight(name)), _bits(_w0(sd, synth, name))), name


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_repack_is_the_load_path(contexts, synth, tiny_dims, precision):
    """Test 2.  Context A (masters) merges an adapter on the device; context B (no masters) is loaded through set_weight with A's effective weights.  The same fp32
    tensors through the same packing routine: unet.forward is bit-identical.  Covers pre_scale (attn1 query, precision >= 1), the packed q | k | v slots and their
    planes (precision 0), the MXFP8 copy of a ResBlock convolution (precision 2)."""
    d = _dims(precision, tiny_dims)
    A, B = contexts(precision, True), contexts(precision, False)
    targets = L.repack_targets(d)
    ad = L.make_adapter(targets, 31)
    base = _forward(B, d)
    a = A.lora_attach(ad, scale=0.9)
    try:
        eff = {n: A.effective_weight(n) for n in targets}
        out_a = _forward(A, d)
        try:
            for n, w in eff.items():
                B.set_weight(n, w)
            B._lib.sdmi_finalize_weights(B._ctx)
            out_b = _forward(B, d)
        finally:
            for n in targets:
                B.set_weight(n, _w0(B, synth, n))
            assert B._lib.sdmi_finalize_weights(B._ctx) == 0
    finally:
        a.detach()
    print(f"precision {precision}: max |adapted - base| = {np.abs(out_a - base).max():.3e}")
    assert np.isfinite(out_a).all() and not np.array_equal(out_a, base)
    assert np.array_equal(_bits(out_a), _bits(out_b))
    assert np.array_equal(_bits(_forward(B, d)), _bits(base))          # B is back to the loaded model


@pytest.mark.parametrize("precision", [0, 1])
def test_reversible_and_without_side_effects(contexts, synth, tiny_dims, precision):
    """Test 3.  Before attaching == after set_scale(0) == after detach() == a context that never kept masters, and s -> 0 -> s returns to the first result at s; all bit for bit."""
    d = _dims(precision, tiny_dims)
    A, P = contexts(precision, True), contexts(precision, False)
    ad = L.make_adapter(L.repack_targets(d), 41)
    plain = _forward(P, d)
    before = _forward(A, d)
    a = A.lora_attach(ad, scale=0.8)
    try:
        at_s = _forward(A, d)
        a.set_scale(0.0)
        at_0 = _forward(A, d)
        a.set_scale(0.8)
        at_s2 = _forward(A, d)
    finally:
        a.detach()
    after = _forward(A, d)
    assert not np.array_equal(at_s, before)
    for what, x in (("before attaching", before), ("at scale 0", at_0), ("after detach", after)):
        assert np.array_equal(_bits(x), _bits(plain)), what
    assert np.array_equal(_bits(at_s2), _bits(at_s))


def _parity_setup(synth, d):
    ad = L.make_adapter(L.parity_targets(d), L.PARITY_SEED)
    prov = L.LoraProvider(synth, [(ad, L.PARITY_SCALE)])
    a = syn.alphas_cumprod()
    return ad, O.StableDiffusionOracle(prov, a, d, torch.float32), O.StableDiffusionOracle(prov, a, d, torch.float64)


def test_parity_of_an_adapted_model_fp32(contexts, synth, tiny_dims):
    """Test 4, fp32: unet.forward at t = 999 / 49 and a 3-step CFG 7.5 latent of the adapted tiny model against the f32 / f64 oracles running the merged weights
    (LoraProvider), at test_model_gpu's bars; and the adapter moves the output by more than 100 x those bars (test_lora_cpu shows the oracle alone says so)."""
    d = tiny_dims
    sd = contexts(0, True)
    ad, o32, o64 = _parity_setup(synth, d)
    lat, ctx = _unet_inputs(d)
    unc = syn.uncond_context(2, d.ctx_dim)
    base_u = {t: sd.unet.forward(lat, [t], ctx) for t in (999, 49)}
    base_l = sd.sample_latent(ctx[:1], unc, 7.5, 3, init_latent=lat[:1])
    a = sd.lora_attach(ad, scale=L.PARITY_SCALE)
    try:
        got_u = {t: sd.unet.forward(lat, [t], ctx) for t in (999, 49)}
        got_l = sd.sample_latent(ctx[:1], unc, 7.5, 3, init_latent=lat[:1])
    finally:
        a.detach()
    tl, tc = torch.from_numpy(lat), torch.from_numpy(ctx)
    for t in (999, 49):
        e64, e32 = _assert_close(got_u[t], o32.unet.forward(tl, t, tc).numpy(), o64.unet.forward(tl, t, tc).numpy(), f"adapted unet_forward t={t}", atol=1e-4)
        moved = float(np.abs(got_u[t] - base_u[t]).max())
        print(f"adapted unet t={t}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}; max |adapted - base| = {moved:.3e}")
        assert moved > 100 * 1e-4
    args = (tc[:1], torch.from_numpy(unc), 7.5, 3, tl[:1])
    e64, e32 = _assert_close(got_l, o32.sample_latent(*args).numpy(), o64.sample_latent(*args).numpy(), "adapted sample_latent", atol=1e-3)
    moved = float(np.abs(got_l - base_l).max())
    print(f"adapted 3-step latent: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}; max |adapted - base| = {moved:.3e}")
    assert moved > 100 * 1e-3


def _rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def test_parity_of_an_adapted_model_bf16(contexts, synth):
    """Test 4, precision 1: a merge adds no error source beyond rounding the merged fp32 weights to bf16 -- the rounding the base weights get.  So the adapted latent's
    relative RMS error against the adapted fp64 oracle is at most 1.5 x the un-adapted model's against the un-adapted oracle, same inputs."""
    d = WIDE
    sd = contexts(1, True)
    ad = L.make_adapter(L.parity_targets(d), L.PARITY_SEED)
    a_cp = syn.alphas_cumprod()
    lat = syn.initial_latent(0, d.latent_h, d.latent_w)[None]
    ctx = syn.cond_context(0, 7, d.ctx_dim)[None]
    unc = syn.uncond_context(2, d.ctx_dim)
    args = (torch.from_numpy(ctx), torch.from_numpy(unc), 7.5, 2, torch.from_numpy(lat))
    ref_base = O.StableDiffusionOracle(synth, a_cp, d, torch.float64).sample_latent(*args).numpy()
    ref_ad = O.StableDiffusionOracle(L.LoraProvider(synth, [(ad, L.PARITY_SCALE)]), a_cp, d, torch.float64).sample_latent(*args).numpy()
    got_base = sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)
    a = sd.lora_attach(ad, scale=L.PARITY_SCALE)
    try:
        got_ad = sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)
    finally:
        a.detach()
    r_base, r_ad = _rel_rms(got_base, ref_base), _rel_rms(got_ad, ref_ad)
    print(f"bf16 2-step latent rel-RMS vs fp64 oracle: un-adapted {r_base:.3e}, adapted {r_ad:.3e}; adapter moved the oracle by {_rel_rms(ref_ad, ref_base):.3e}")
    assert np.isfinite(got_ad).all()
    assert r_ad <= 1.5 * r_base


def test_nine_adapters_on_one_target(contexts, synth, tiny_dims):
    """More active adapters on one tensor than one merge launch takes (8): the ninth continues the sum in place, in the same order, under the same bound."""
    d = tiny_dims
    sd = contexts(0, True)
    name, c = L.TB + "/attn2/key/weight", d.model_channels
    base = _forward(sd, d)
    ads = [L.make_adapter({name: ((d.ctx_dim, c), 1 + i % 3)}, 60 + i) for i in range(9)]
    scales = [0.3 + 0.1 * i for i in range(9)]
    live = []
    try:
        for ad, s in zip(ads, scales):
            live.append(sd.lora_attach(ad, scale=s))
        _check_merge(sd, synth, name, list(zip(ads, scales)))
        assert not np.array_equal(_forward(sd, d), base)
    finally:
        for a in reversed(live):
            a.detach()
    assert np.array_equal(_bits(_forward(sd, d)), _bits(base))


def _raw(sd):
    lib = sd._lib
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731

    def create():
        h = C.c_void_p()
        return lib.sdmi_lora_create(sd._ctx, C.byref(h)), h

    def add(h, name, down, up, rank, alpha):
        return lib.sdmi_lora_add(h, name.encode(), f(down), f(up), rank, alpha)

    return lib, create, add


def test_stacking_and_errors(contexts, sd_tiny, synth, tiny_dims):
    """Test 5.  Two adapters on one target sum; every status code of the header; a refused call changes nothing."""
    d = tiny_dims
    sd = contexts(0, True)
    q = L.TB + "/attn1/query/weight"
    c = d.model_channels
    ad1, ad2 = L.make_adapter({q: ((c, c), 6)}, 51), L.make_adapter({q: ((c, c), 17)}, 52)
    base = _forward(sd, d)
    a1, a2 = sd.lora_attach(ad1, scale=1.0), sd.lora_attach(ad2, scale=0.5)
    try:
        _check_merge(sd, synth, q, [(ad1, 1.0), (ad2, 0.5)])
        a1.set_scale(0.0)          # changing one adapter re-merges the target with the other still active
        _check_merge(sd, synth, q, [(ad2, 0.5)])
        a1.set_scale(1.0)
        stacked = _forward(sd, d)

        lib, create, add = _raw(sd)
        st, h = create()
        assert st == 0 and h.value
        down, up = ad1[q][0], ad1[q][1]
        nan = float("nan")
        assert add(h, "unet/nope/weight", down, up, 6, 1.0) == ERR_INVALID                                   # unknown target
        assert add(h, L.TB + "/norm1/weight", down, up, 6, 1.0) == ERR_INVALID                                # a norm
        assert add(h, L.TB + "/attn1/out/bias", down, up, 6, 1.0) == ERR_INVALID                              # a bias
        assert add(h, "alphas_cumprod", down, up, 6, 1.0) == ERR_INVALID
        assert add(h, q, down, up, 0, 1.0) == ERR_INVALID and add(h, q, down, up, 257, 1.0) == ERR_INVALID    # rank outside 1 .. 256
        assert add(h, q, down, up, 6, nan) == ERR_INVALID and add(h, q, down, up, 6, float("inf")) == ERR_INVALID
        assert add(h, q, down, up, 6, 3.0) == 0
        assert add(h, q, down, up, 6, 3.0) == ERR_INVALID                                                     # already in this adapter
        assert lib.sdmi_lora_set_scale(h, nan) == ERR_INVALID and lib.sdmi_lora_set_scale(h, float("inf")) == ERR_INVALID
        s, n = C.c_double(-1), C.c_int32(-1)
        assert lib.sdmi_lora_get_scale(h, C.byref(s), C.byref(n)) == 0 and s.value == 0.0 and n.value == 1    # a refused scale changed nothing
        assert np.array_equal(_bits(_forward(sd, d)), _bits(stacked))
        assert lib.sdmi_lora_set_scale(h, 0.25) == 0
        assert add(h, L.TB + "/attn1/key/weight", down, up, 6, 1.0) == ERR_STATE                              # add only at scale 0
        # sdmi_set_weight on a tensor under an active adapter
        with pytest.raises(SdmiError) as ei:
            sd.set_weight(q, _w0(sd, synth, q))
        assert ei.value.status == ERR_STATE
        assert lib.sdmi_lora_destroy(h) == 0
        assert np.array_equal(_bits(_forward(sd, d)), _bits(stacked))
        # shape mismatches never reach the library from Python
        with pytest.raises(ValueError, match="down must be"):
            sd.lora_attach({q: (down[:, :-1], up, 1.0)})
        with pytest.raises(SdmiError) as ei:
            sd.effective_weight(L.TB + "/norm1/weight")
        assert ei.value.status == ERR_INVALID
        out = np.empty(5, np.float32)
        assert lib.sdmi_lora_effective_weight(sd._ctx, q.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), 5) == ERR_INVALID
        assert np.array_equal(_bits(_forward(sd, d)), _bits(stacked))
    finally:
        a2.detach()
        a1.detach()
    assert np.array_equal(_bits(_forward(sd, d)), _bits(base))

    # with masters kept and no active adapter, sdmi_set_weight replaces W0 too
    k = L.TB + "/attn1/key/weight"
    w0 = _w0(sd, synth, k)
    try:
        sd.set_weight(k, (2 * w0).astype(np.float32))
        assert sd._lib.sdmi_finalize_weights(sd._ctx) == 0
        assert np.array_equal(_bits(sd.effective_weight(k)), _bits(2 * w0))
    finally:
        sd.set_weight(k, w0)
        assert sd._lib.sdmi_finalize_weights(sd._ctx) == 0
    assert np.array_equal(_bits(_forward(sd, d)), _bits(base))

    # create: not without masters, not before finalize; keep_masters: not after loading
    ref = _forward(sd_tiny, d)
    lib, create, _ = _raw(sd_tiny)
    st, h = create()
    assert st == ERR_STATE and not h.value
    with pytest.raises(SdmiError) as ei:
        sd_tiny.set_option("keep_masters", 1)
    assert ei.value.status == ERR_STATE
    with pytest.raises(SdmiError) as ei:
        sd_tiny.effective_weight(q)
    assert ei.value.status == ERR_STATE
    assert np.array_equal(_bits(_forward(sd_tiny, d)), _bits(ref))
    assert np.array_equal(_bits(ref), _bits(base))                    # masters on or off: the same model
    fresh = _new(d, 0, True)
    try:
        st, h = _raw(fresh)[1]()
        assert st == ERR_STATE and not h.value
    finally:
        fresh.close()


def test_unsupported_rgb_conv_in(synth, tiny_dims):
    """the 3-channel conv_in of the VAE encoder is packed in a padded form: SDMI_ERR_UNSUPPORTED; its effective weight comes back in the reference's 3-channel layout.
    A context with the CLIP group: its embedding tables are refused, its Linear layers are not."""
    d = tiny_dims
    sd = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, clip_layers=1, clip_heads=1, clip_vocab=48, clip_ctx=8))
    sd.set_option("keep_masters", 1)
    try:
        sd.load_weights(synth, clip=True, vae_encoder=True)
        name = "autoencoder/encoder/conv_in/weight"
        lib, create, add = _raw(sd)
        st, h = create()
        assert st == 0
        down, up = np.zeros((2, 3, 3, 3), np.float32), np.zeros((d.vae_ch, 2), np.float32)
        assert add(h, name, down, up, 2, 1.0) == ERR_UNSUPPORTED
        # an embedding table is 2-D like a Linear weight, and is none
        assert add(h, "clip/token_embedding/weight", np.zeros((2, 48), np.float32), np.zeros((d.ctx_dim, 2), np.float32), 2, 1.0) == ERR_INVALID
        assert add(h, "clip/position_embedding/weight", np.zeros((2, 8), np.float32), np.zeros((d.ctx_dim, 2), np.float32), 2, 1.0) == ERR_INVALID
        # ... while the text encoder's Linear layers are targets like any other (masters of the CLIP group)
        fc1 = "clip/blocks/0/mlp/fc1/weight"
        assert add(h, fc1, np.zeros((2, d.ctx_dim), np.float32), np.zeros((4 * d.ctx_dim, 2), np.float32), 2, 1.0) == 0
        assert np.array_equal(_bits(sd.effective_weight(fc1)), _bits(_w0(sd, synth, fc1)))
        assert lib.sdmi_lora_destroy(h) == 0
        assert np.array_equal(_bits(sd.effective_weight(name)), _bits(_w0(sd, synth, name)))
    finally:
        sd.close()


def test_multi_device_surface(synth, tiny_dims):
    """Test 6.  MultiStableDiffusion((0,)): lora_attach changes sample_image, detach restores it bit for bit."""
    d = tiny_dims
    m = MultiStableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch), devices=(0,))
    try:
        m.device_view(0).set_option("keep_masters", 1)
        m.load_weights(synth)
        ctx, unc = syn.cond_context(0, 7, d.ctx_dim), syn.uncond_context(2, d.ctx_dim)
        lat = syn.initial_latent(0, d.latent_h, d.latent_w)[None]
        before = m.sample_image(ctx, unc, 7.5, 2, 1, init_latents=lat)
        a = m.lora_attach(L.make_adapter(L.parity_targets(d), L.PARITY_SEED), scale=1.0)
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
