"""Web-UI prompt encoding on the GPU: the extended CLIP forward -- bank rows, CLIP skip, the emphasis launch -- through the C ABI against
tests/prompt_ref.py on the f64 CLIP oracle, textual-inversion files, sdmi_encode_prompt end to end and the CLI twin's web-UI mode.

Bars.  Parity with the f64 oracle: test_clip_gpu.py's own, |gpu - ref| <= 2e-5 max(1, |ref|_inf).  The weighting is checked apart from CLIP's error, on the GPU's own
unweighted z: e = fl32(z w) * fl32(sum z / sum fl32(z w)), sums in f64, and |gpu - e| <= 4 * 2^-24 |e| elementwise (three fp32 roundings plus one; the two f64
sums are exact to ~1e-16 at these sizes).  Everything that says "bits" is assert_array_equal."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import prompt_ref as R
from oracle import clip_oracle as CO
from stable_diffusion_burn_amd import synthetic as syn

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"
MINI = GOLD / "mini_merges.txt"
MINI_VOCAB = 512 + 264 + 2
SOT, EOT = MINI_VOCAB - 2, MINI_VOCAB - 1
CTX, CD = 16, 64
TINY = CO.ClipDims(n_vocab=MINI_VOCAB, n_state=CD, n_head=1, n_ctx=CTX, n_layer=2)
ULP = 2.0 ** -24
LONG = " ".join(["a photo of a cat"] * 4)   # 20 content tokens: two chunks


def _close(got, ref, what, rel=2e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref).max()
    bound = rel * max(1.0, np.abs(ref).max())
    print(f"{what}: max|gpu - ref| = {err:.3e} (bar {bound:.3e})")
    assert err <= bound, f"{what}: max|d| = {err:.3e} > {bound:.3e}"


def _weighting_close(got, z, w, what):
    e = R.reweight_f32_model(z, w).astype(np.float64)
    d = np.abs(np.asarray(got, np.float64) - e)
    worst = float((d / np.maximum(np.abs(e), 1e-300)).max()) if d.max() > 0 else 0.0
    print(f"{what}: max |gpu - e| / |e| = {worst / ULP:.2f} x 2^-24")
    assert np.isfinite(got).all() and (d <= 4 * ULP * np.abs(e)).all(), f"{what}: {worst / ULP:.2f} x 2^-24"


@pytest.fixture(scope="module")
def sd():
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion(ModelConfig(160, 4, CD, 16, 16, 32, clip_layers=2, clip_heads=1, clip_vocab=MINI_VOCAB, clip_ctx=CTX))
    sd.load_weights(syn.SyntheticWeights())
    yield sd
    sd.close()


@pytest.fixture(scope="module")
def tok():
    from stable_diffusion_burn_amd import SimpleTokenizer
    return SimpleTokenizer(MINI)


@pytest.fixture(scope="module")
def clip64():
    return CO.CLIPOracle(syn.SyntheticWeights(), TINY, torch.float64)


@pytest.fixture(scope="module")
def bank():
    return np.random.default_rng(11).standard_normal((5, CD)).astype(np.float32) * 0.05


@pytest.fixture()
def sd_emb(sd, tok, bank):
    """the context with two embeddings: "zx" = rows 0..2, "q" = rows 3..4; removed afterwards"""
    sd.add_embedding(tok, "zx", bank[:3])
    sd.add_embedding(tok, "q", bank[3:])
    assert sd.embeddings() == [("zx", 3), ("q", 2)]
    yield sd
    sd.remove_embedding("zx")
    assert sd.embeddings() == [("q", 2)]
    sd.remove_embedding("q")
    assert sd.embeddings() == []


@pytest.mark.parametrize("text,k", [("a photo of a cat", 1), (" ".join(["a photo of a cat"] * 7), 3)])
def test_unweighted_is_the_plain_forward(sd, tok, text, k):
    """no weight but 1, no bank row, clip_skip 1: the launches and the bits of sdmi_clip_forward; emphasis that changes a weight: exactly one launch more"""
    ids, w, rows = tok.prompt_chunks(text, CTX, emphasis=False)
    assert ids.shape == (k, CTX) and (w == 1).all() and (rows == -1).all()
    got = sd.encode_prompt(tok, text, emphasis=False)
    kernels = sd.last_call_stats()["kernels"]
    assert got.shape == (1, k * CTX, CD)
    batch = sd.clip.forward(ids)
    assert sd.last_call_stats()["kernels"] == kernels
    np.testing.assert_array_equal(got[0].reshape(k, CTX, CD), batch)
    np.testing.assert_array_equal(sd.encode_prompt(tok, text), got)          # emphasis on, nothing to emphasise
    assert sd.last_call_stats()["kernels"] == kernels
    for i in range(k):
        np.testing.assert_array_equal(got[0, i * CTX:(i + 1) * CTX], sd.clip.forward(ids[i:i + 1])[0])
    weighted = sd.encode_prompt(tok, "(a:1.3) " + text[2:])
    assert sd.last_call_stats()["kernels"] == kernels + 1
    assert weighted.shape == got.shape and not np.array_equal(weighted, got)


PARITY = {
    "n1 skip1 rows first": (1, 1, [(0, 1, 0, 3)]),
    "n1 skip2 rows end at 14": (1, 2, [(0, 12, 0, 3)]),
    "n3 skip1 rows in the second chunk": (3, 1, [(1, 5, 3, 2)]),
    "n3 skip2 rows in every chunk": (3, 2, [(0, 1, 3, 2), (1, 12, 0, 3), (2, 13, 3, 2)]),
    "n3 skip2 no rows": (3, 2, []),
}


@pytest.mark.parametrize("case", PARITY, ids=list(PARITY))
def test_extended_forward_matches_oracle(sd_emb, clip64, bank, case):
    n, skip, spans = PARITY[case]
    g = np.random.default_rng(n * 10 + skip)
    tokens = g.integers(0, MINI_VOCAB - 2, (n, CTX)).astype(np.int32)
    tokens[:, 0] = SOT
    tokens[:, CTX - 1] = EOT
    rows = np.full((n, CTX), -1, np.int32)
    for b, pos, first, v in spans:
        rows[b, pos:pos + v] = np.arange(first, first + v)
        tokens[b, pos:pos + v] = EOT
    got = sd_emb.clip.forward(tokens, emb_row=rows if spans else None, clip_skip=skip)
    _close(got, R.clip_forward_ex(clip64, tokens, rows, bank, None, skip).numpy(), case)


def test_bank_rows_copied_from_the_token_table_give_the_token_bits(sd, tok, clip64):
    table = clip64._table("token_embedding", MINI_VOCAB).numpy().astype(np.float32)
    tokens, _ = R.emphasis_inputs(MINI_VOCAB, CTX)
    rows = np.full(tokens.shape, -1, np.int32)
    rows[0, 1:4] = [0, 1, 2]
    rows[2, 12:15] = [2, 0, 1]
    as_tokens = tokens.copy()
    as_tokens[0, 1:4] = [300, 7, 512]
    as_tokens[2, 12:15] = [512, 300, 7]
    sd.add_embedding(tok, "zx", table[[300, 7, 512]])
    try:
        kernels = []
        got = sd.clip.forward(tokens, emb_row=rows)
        kernels.append(sd.last_call_stats()["kernels"])
        ref = sd.clip.forward(as_tokens)
        kernels.append(sd.last_call_stats()["kernels"])
    finally:
        sd.remove_embedding("zx")
    np.testing.assert_array_equal(got, ref)
    assert kernels[0] == kernels[1]        # the bank embed launch replaces the plain one
    assert not np.array_equal(got, sd.clip.forward(tokens))


def test_weighting_arithmetic(sd):
    """three chunks with different weights in one call: above and below 1, negative, zero; the middle chunk has all weights 1 and keeps its bits (the kernel does not
    skip it: its two sums are equal, its factor is exactly 1)"""
    tokens, w = R.emphasis_inputs(MINI_VOCAB, CTX)
    assert (w[0] > 1).any() and ((w[0] < 1) & (w[0] > 0)).any() and (w[0] < 0).any() and (w[0] == 0).any() and (w[1] == 1).all()
    z = sd.clip.forward(tokens)
    kernels = sd.last_call_stats()["kernels"]
    got = sd.clip.forward(tokens, weights=w)
    assert sd.last_call_stats()["kernels"] == kernels + 1
    _weighting_close(got, z, w, "tiny, 3 chunks")
    np.testing.assert_array_equal(got[1], z[1])
    assert np.abs(got[0] - z[0]).max() > 100 * 2e-5 * max(1.0, np.abs(z).max())
    np.testing.assert_array_equal(sd.clip.forward(tokens, weights=w), got)           # run to run
    np.testing.assert_array_equal(sd.clip.forward(tokens[:1], weights=w[:1])[0], got[0])   # a chunk's factor is its own
    # all weights 1 given explicitly: the host drops the launch
    np.testing.assert_array_equal(sd.clip.forward(tokens, weights=np.ones_like(w)), z)
    assert sd.last_call_stats()["kernels"] == kernels


def test_zero_weighted_sum_gives_factor_one(sd):
    tokens, w = R.emphasis_inputs(MINI_VOCAB, CTX)
    w[0] = 0.0
    got = sd.clip.forward(tokens, weights=w)
    assert np.isfinite(got).all() and (got[0] == 0).all()
    _weighting_close(got, sd.clip.forward(tokens), w, "a chunk of zero weights")


def test_errors(sd, tok, tmp_path):
    from stable_diffusion_burn_amd import ModelConfig, SdmiError, StableDiffusion, weights as wio
    tokens = np.array([[SOT, 5, 6, EOT]], np.int32)

    def status(fn, *a, **kw):
        with pytest.raises(SdmiError) as ei:
            fn(*a, **kw)
        return ei.value.status

    assert status(sd.clip.forward, tokens, clip_skip=0) == -1
    assert status(sd.clip.forward, tokens, clip_skip=3) == -1
    assert status(sd.encode_prompt, tok, "a", clip_skip=3) == -1
    assert status(sd.clip.forward, tokens, emb_row=np.array([[-1, 0, -1, -1]])) == -1          # no embeddings: every row is out of range
    assert status(sd.add_embedding, tok, "zx", np.zeros((15, CD), np.float32)) == -1          # longer than L = 14
    assert status(sd.add_embedding, tok, "", np.zeros((1, CD), np.float32)) == -1
    sd.add_embedding(tok, "zx", np.zeros((14, CD), np.float32))
    try:
        assert status(sd.add_embedding, tok, "zx", np.zeros((1, CD), np.float32)) == -1       # duplicate
        assert status(sd.clip.forward, tokens, emb_row=np.array([[-1, 14, -1, -1]])) == -1
        assert status(sd.clip.forward, tokens, emb_row=np.array([[-1, -2, -1, -1]])) == -1
        assert status(sd.clip.forward, np.array([[SOT, MINI_VOCAB, 6, EOT]]), emb_row=np.array([[-1, 13, -1, -1]])) == -1
        sd.clip.forward(tokens, emb_row=np.array([[-1, 13, -1, -1]]))
    finally:
        sd.remove_embedding("zx")
    assert status(sd.remove_embedding, "zx") == -1
    wio.write_safetensors(tmp_path / "wrong_c.safetensors", {"emb_params": np.zeros((2, CD + 32), np.float32)})
    assert status(sd.load_embedding, tok, "zx", tmp_path / "wrong_c.safetensors") == -1
    wio.write_safetensors(tmp_path / "two.safetensors", {"x": np.zeros((2, CD), np.float32), "y": np.zeros((2, CD), np.float32)})
    assert status(sd.load_embedding, tok, "zx", tmp_path / "two.safetensors") == -3
    (tmp_path / "cut.safetensors").write_bytes((tmp_path / "two.safetensors").read_bytes()[:-8])
    assert status(sd.load_embedding, tok, "zx", tmp_path / "cut.safetensors") in (-3, -4)
    assert sd.embeddings() == []
    # capacity too small: *T is still set
    out = np.empty((CTX, CD), np.float32)
    T = C.c_int32(-1)
    st = sd._lib.sdmi_encode_prompt(sd._ctx, tok._tok, LONG.encode(), None, out.ctypes.data_as(C.POINTER(C.c_float)), CTX, C.byref(T))
    assert st == -1 and T.value == 2 * CTX
    # the CLIP group not loaded
    bare = StableDiffusion(ModelConfig(64, 1, CD, 8, 8, 64, clip_layers=2, clip_heads=1, clip_vocab=MINI_VOCAB, clip_ctx=CTX))
    try:
        bare.load_weights(syn.SyntheticWeights(), clip=False)
        assert status(bare.encode_prompt, tok, "a") == -6
        assert status(bare.clip.forward, tokens, clip_skip=2) == -6
    finally:
        bare.close()


def test_embedding_files(sd, tok, tmp_path):
    """F32 / F16 / BF16, under "emb_params" (alone or among others) or as the file's only tensor, [C] and [v, C]: exactly the widened values"""
    from stable_diffusion_burn_amd import weights as wio
    g = np.random.default_rng(3)
    text = "a zx (zx:1.3) b"
    for shape in ((CD,), (3, CD)):
        src = (g.standard_normal(shape) * 0.05).astype(np.float32)
        forms = {"F32": (src, src), "F16": (src.astype(np.float16), src.astype(np.float16).astype(np.float32)),
                 "BF16": ((wio.bf16_bits(src), "BF16"), wio.bf16_to_f32(wio.bf16_bits(src)))}
        for tag, (stored, wide) in forms.items():
            sd.add_embedding(tok, "zx", wide)
            ref = sd.encode_prompt(tok, text)
            sd.remove_embedding("zx")
            for keys in ({"emb_params": stored}, {"<zx>": stored}, {"other": np.zeros(3, np.float32), "emb_params": stored}):
                path = tmp_path / f"{tag}_{len(shape)}_{len(keys)}_{list(keys)[0][:1]}.safetensors"
                wio.write_safetensors(path, keys)
                sd.load_embedding(tok, "zx", path)
                try:
                    assert sd.embeddings() == [("zx", 1 if len(shape) == 1 else 3)]
                    np.testing.assert_array_equal(sd.encode_prompt(tok, text), ref)
                finally:
                    sd.remove_embedding("zx")
        assert not np.array_equal(ref, sd.encode_prompt(tok, text))   # without the embedding the name is ordinary text


def test_encode_prompt_with_embeddings_and_emphasis_matches_oracle(sd_emb, tok, clip64, bank):
    """the whole call against the oracle: chunker, bank, weighting; the negative prompt padded to the same count"""
    text = "a (zx:1.2) of [a cat] BREAK q on (a:0.7) photo"
    ids, w, rows = R.prompt_chunks(tok.encode, SOT, EOT, text, CTX, embeddings=[("zx", 3), ("q", 2)])
    assert len(ids) == 2 and (rows >= 0).sum() == 5
    for skip in (1, 2):
        got = sd_emb.encode_prompt(tok, text, clip_skip=skip)
        z = sd_emb.clip.forward(ids, emb_row=rows, clip_skip=skip)
        _close(z, R.clip_forward_ex(clip64, ids, rows, bank, None, skip).numpy(), f"unweighted, clip_skip {skip}")
        _weighting_close(got[0].reshape(2, CTX, CD), z, w, f"encode_prompt, clip_skip {skip}")
    neg = sd_emb.encode_prompt(tok, "", min_chunks=2)
    assert neg.shape == (1, 2 * CTX, CD)
    np.testing.assert_array_equal(neg[0, :CTX], neg[0, CTX:])
    np.testing.assert_array_equal(neg[0, :CTX], sd_emb.clip.forward(np.array([[SOT] + [EOT] * (CTX - 1)], np.int32))[0])


def test_long_prompt_feeds_sampling_and_the_unet(sd, tok, synth, tiny_dims):
    from oracle import sd_oracle as O
    from test_model_gpu import _assert_close
    ctx = sd.encode_prompt(tok, LONG)
    unc = sd.encode_prompt(tok, "", min_chunks=2)[0]
    assert ctx.shape == (1, 2 * CTX, CD) and unc.shape == (2 * CTX, CD)
    lat = syn.initial_latent(0, 16, 16)[None]
    img = sd.sample_image(ctx, unc, 7.5, 2, init_latent=lat)
    assert img.shape == (1, 128, 128, 3) and img.dtype == np.uint8 and img.std() > 1
    got = sd.unet.forward(lat, [500], ctx)
    a = syn.alphas_cumprod()
    r32 = O.StableDiffusionOracle(synth, a, tiny_dims, torch.float32).unet.forward(torch.from_numpy(lat), 500, torch.from_numpy(ctx)).numpy()
    r64 = O.StableDiffusionOracle(synth, a, tiny_dims, torch.float64).unet.forward(torch.from_numpy(lat), 500, torch.from_numpy(ctx)).numpy()
    e64, e32 = _assert_close(got, r32, r64, "unet_forward T=32", atol=1e-4)
    print(f"unet T=32: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")


def test_sample_cli_web_ui_mode(sd, tok, tmp_path):
    """sdmi_sample with SDMI_PROMPT_STYLE=webui writes the PNG of the same calls through Python, byte for byte; without it, the reference's rule as before"""
    from stable_diffusion_burn_amd import build, weights as wio
    specs = sd.weight_specs()
    shapes = dict(specs)
    W = syn.SyntheticWeights()
    wio.write_dump_tree(tmp_path / "params", specs, lambda name, shape: syn.named_tensor(W, name, shape, shapes), syn.alphas_cumprod(), n_head=4, clip_heads=1)
    env = dict(os.environ, SDMI_BPE_VOCAB=str(MINI), SDMI_SEED="3",
               SDMI_CONFIG=f"model_channels=160,n_head=4,ctx_dim=64,latent_h=16,latent_w=16,vae_ch=32,clip_layers=2,clip_heads=1,clip_vocab={MINI_VOCAB},clip_ctx=16")
    for k in ("SDMI_PROMPT_STYLE", "SDMI_NEGATIVE_PROMPT", "SDMI_CLIP_SKIP"):
        env.pop(k, None)
    prompt, negative = "a (photo:1.3) of a cat BREAK " + LONG, "[a] b"

    def run(prompt, out, **extra):
        r = subprocess.run([str(build.CLI), "dump", str(tmp_path / "params"), "7.5", "2", prompt, str(out), "hip:0"], env=dict(env, **extra), capture_output=True,
                           text=True, timeout=300)
        return r

    def png(img, path):
        from stable_diffusion_burn_amd._capi import check
        check(sd._lib.sdmi_write_png(str(path).encode(), img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[1], img.shape[0]))
        return Path(path).read_bytes()

    r = run(prompt, tmp_path / "web", SDMI_PROMPT_STYLE="webui", SDMI_NEGATIVE_PROMPT=negative, SDMI_CLIP_SKIP="2")
    assert r.returncode == 0, r.stderr
    ctx = sd.encode_prompt(tok, prompt, clip_skip=2)
    assert ctx.shape[1] == 3 * CTX
    unc = sd.encode_prompt(tok, negative, clip_skip=2, min_chunks=3)[0]
    ref = np.ascontiguousarray(sd.sample_image(ctx, unc, 7.5, 2, seed=3)[0])
    assert (tmp_path / "web0.png").read_bytes() == png(ref, tmp_path / "web_ref.png")
    # unset: today's path, where the two variables are ignored and a long prompt stays an error
    r = run("a photo of a cat", tmp_path / "plain", SDMI_NEGATIVE_PROMPT=negative, SDMI_CLIP_SKIP="2")
    assert r.returncode == 0, r.stderr
    ref = np.ascontiguousarray(sd.sample_image(sd.context(tok, "a photo of a cat"), sd.unconditional_context(tok), 7.5, 2, seed=3)[0])
    assert (tmp_path / "plain0.png").read_bytes() == png(ref, tmp_path / "plain_ref.png")
    r = run(prompt, tmp_path / "long")
    assert r.returncode == 1 and "Error encoding the prompt" in r.stderr
    r = run("a", tmp_path / "bad", SDMI_PROMPT_STYLE="other")
    assert r.returncode == 1 and "SDMI_PROMPT_STYLE" in r.stderr


def test_full_size_weighted_two_chunks_clip_skip_2(bpe_vocab):
    """SD v1's text encoder (12 layers, 768 wide, 77 tokens, synthetic weights): the only shape with the 59 136-element reduction and C = 768"""
    from stable_diffusion_burn_amd import ModelConfig, SimpleTokenizer, StableDiffusion
    tok = SimpleTokenizer(bpe_vocab)
    text = ("a (highly detailed:1.3) photograph of an [old] lighthouse on a (((rocky))) coast at (dusk:0.8), waves, (fog:-0.2), (birds:0) " * 4).strip()
    ids, w, rows = tok.prompt_chunks(text, 77)
    assert ids.shape == (2, 77) and (w != 1).sum() > 10 and (w[1] != 1).any()
    sd = StableDiffusion(ModelConfig(64, 1, 768, 8, 8, 64, clip_layers=12))
    try:
        sd.load_weights(syn.SyntheticWeights())
        z = sd.clip.forward(ids, clip_skip=2)
        got = sd.encode_prompt(tok, text, clip_skip=2)
    finally:
        sd.close()
    ref = R.clip_forward_ex(CO.CLIPOracle(syn.SyntheticWeights(), CO.ClipDims(), torch.float64), ids, clip_skip=2).numpy()
    _close(z, ref, "full size, clip_skip 2, unweighted")
    assert got.shape == (1, 154, 768)
    _weighting_close(got[0].reshape(2, 77, 768), z, w, "full size, 2 chunks")
    assert np.abs(got[0].reshape(2, 77, 768) - z).max() > 100 * 2e-5 * max(1.0, np.abs(z).max())
