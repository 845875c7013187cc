"""IP-Adapter without a GPU (include/sdmi.h "IP-Adapter"): the layer rule against the golden key list, the file writer against the C++ reader,
every refusal of the loader's host-only check on hand-made small files with the key named, the identities of the CPU restatement the GPU tests are held against,
and the built kernel's register use."""
from pathlib import Path

import numpy as np
import pytest
import torch

import ip_adapter_ref as IR
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import ModelConfig, SdmiError, ip_adapter_check_safetensors, ip_adapter_key, safetensors_list
from stable_diffusion_burn_amd import synthetic as syn
from stable_diffusion_burn_amd.weights import write_ip_adapter_safetensors, write_safetensors

GOLDEN = Path(__file__).parent / "golden" / "ip_adapter_keys.txt"
SDMI_ERR_INVALID, SDMI_ERR_WEIGHTS, SDMI_ERR_UNSUPPORTED = -1, -3, -5
SMALL = O.Dims(160, 4, 64, 16, 16, 32)


def _golden():
    """{(mc, cd, D, T): (projection rows [(key, shape)], layer rows [(ctx_index, block, key, shape)])}"""
    out, cur = {}, None
    for ln in GOLDEN.read_text().splitlines():
        if ln.startswith("#"):
            cur = tuple(int(kv.split("=")[1]) for kv in ln[1:].split())
            out[cur] = ([], [])
            continue
        f = ln.split("\t")
        shape = tuple(int(v) for v in f[-1].split(","))
        if len(f) == 2:
            out[cur][0].append((f[0], shape))
        else:
            out[cur][1].append((int(f[0]), f[1], f[2], shape))
    return out


def _status(fn):
    try:
        fn()
    except SdmiError as e:
        return e.status, str(e)
    return 0, ""


def test_error_codes_are_the_headers():
    text = (Path(__file__).resolve().parents[1] / "include" / "sdmi.h").read_text()
    for name, value in (("SDMI_ERR_INVALID", SDMI_ERR_INVALID), ("SDMI_ERR_WEIGHTS", SDMI_ERR_WEIGHTS), ("SDMI_ERR_UNSUPPORTED", SDMI_ERR_UNSUPPORTED)):
        assert f"{name} = {value}" in text.replace("  ", " "), name


@pytest.mark.parametrize("model", [(320, 768, 1024, 4), (160, 64, 64, 4)])
def test_key_map_against_the_golden_list(model):
    mc, cd, D, T = model
    proj, layers = _golden()[model]
    assert len(layers) == 32
    cfg = ModelConfig(model_channels=mc, ctx_dim=cd)
    seen = set()
    for i, block, key, shape in layers:
        which = "k" if ".to_k_ip." in key else "v"
        got, j, c = ip_adapter_key(cfg, i, which, with_shape=True)
        assert (got, (c, cd)) == (key, shape), (i, block)
        assert j % 2 == 1 and got == f"ip_adapter.{j}.to_{which}_ip.weight"
        seen.add(j)
    assert seen == set(range(1, 32, 2))
    # the list a synthetic file is written from (it asks the library), and the synthetic adapter's shapes
    assert [(kk, kv, c) for kk, kv, c in syn.ip_adapter_layers(mc)] == [(layers[2 * i][2], layers[2 * i + 1][2], layers[2 * i][3][0]) for i in range(16)]
    if mc == 160:
        ad = syn.ip_adapter(mc, cd, D, T)
        assert {k: tuple(a.shape) for k, a in ad.items()} == {**dict(proj), **{key: shape for _, _, key, shape in layers}}
    for bad in (-1, 16):
        assert _status(lambda: ip_adapter_key(cfg, bad))[0] == SDMI_ERR_INVALID


def test_the_order_is_down_up_mid():
    cfg = ModelConfig()
    js = [ip_adapter_key(cfg, i, "k", with_shape=True)[1] for i in range(16)]
    assert js[:6] == [1, 3, 5, 7, 9, 11] and js[6] == 31 and js[7:] == list(range(13, 31, 2))


@pytest.mark.parametrize("dtype", ["F32", "F16", "BF16"])
def test_writer_round_trip(tmp_path, dtype):
    d = SMALL
    ad = syn.ip_adapter(d.model_channels, d.ctx_dim, 64, 4)
    path = tmp_path / f"ip_{dtype}.safetensors"
    write_ip_adapter_safetensors(path, ad, dtype)
    listed = {key: (dt, shape) for key, dt, shape, _, _ in safetensors_list(path)}
    assert listed == {k: (dtype, tuple(a.shape)) for k, a in ad.items()}
    assert ip_adapter_check_safetensors(ModelConfig(d.model_channels, d.n_head, d.ctx_dim), path) == (64, 4)


def test_refusals_name_the_key(tmp_path):
    d = SMALL
    cfg = ModelConfig(d.model_channels, d.n_head, d.ctx_dim)
    good = syn.ip_adapter(d.model_channels, d.ctx_dim, 64, 4)

    def check(ad, name="a.safetensors", raw=None):
        path = tmp_path / name
        if raw is not None:
            path.write_bytes(raw)
        else:
            write_safetensors(path, ad)
        return _status(lambda: ip_adapter_check_safetensors(cfg, path))

    assert check(good)[0] == 0
    # a missing layer, a missing projection tensor
    for gone in ("ip_adapter.7.to_v_ip.weight", "ip_adapter.31.to_k_ip.weight", "image_proj.norm.bias", "image_proj.proj.weight"):
        st, msg = check({k: v for k, v in good.items() if k != gone})
        assert st == SDMI_ERR_WEIGHTS and f"'{gone}'" in msg and "missing" in msg, (gone, st, msg)
    # an extra layer (an even index, one past the end)
    for extra in ("ip_adapter.2.to_k_ip.weight", "ip_adapter.33.to_v_ip.weight"):
        st, msg = check({**good, extra: good["ip_adapter.1.to_k_ip.weight"]})
        assert st == SDMI_ERR_WEIGHTS and f"'{extra}'" in msg, (extra, st, msg)
    # shapes that do not match the model: a layer's width, the context width, the projection's bias, another model's file
    for key, shape in (("ip_adapter.5.to_k_ip.weight", (160, 64)), ("ip_adapter.1.to_v_ip.weight", (160, 32)), ("image_proj.proj.bias", (128,)), ("image_proj.norm.weight", (32,))):
        st, msg = check({**good, key: np.zeros(shape, np.float32)})
        assert st == SDMI_ERR_WEIGHTS and f"'{key}'" in msg and str(list(shape)) in msg, (key, st, msg)
    st, msg = check(syn.ip_adapter(320, d.ctx_dim, 64, 4))
    assert st == SDMI_ERR_WEIGHTS and "'ip_adapter." in msg
    st, msg = check({**good, "image_proj.proj.weight": np.zeros((4 * d.ctx_dim, 48), np.float32)})
    assert st == SDMI_ERR_WEIGHTS and "'image_proj.proj.weight'" in msg
    # a dtype the loader does not read
    st, msg = check({**good, "ip_adapter.9.to_k_ip.weight": good["ip_adapter.9.to_k_ip.weight"].astype(np.float64)})
    assert st == SDMI_ERR_WEIGHTS and "'ip_adapter.9.to_k_ip.weight'" in msg and "F64" in msg
    # the "plus" Resampler
    for key in ("image_proj.latents", "image_proj.layers.0.0.to_q.weight"):
        st, msg = check({**good, key: np.zeros((1, 4, 8), np.float32)})
        assert st == SDMI_ERR_UNSUPPORTED and f"'{key}'" in msg and "Resampler" in msg, (key, st, msg)
    # pickles: by name, and by content under a .safetensors name
    for name, raw in (("ip-adapter_sd15.bin", b"PK\x03\x04" + b"\0" * 64), ("zip.safetensors", b"PK\x03\x04" + b"\0" * 64), ("pkl.safetensors", b"\x80\x02}q\x00." + b"\0" * 64)):
        st, msg = check(None, name, raw)
        assert st == SDMI_ERR_UNSUPPORTED and "pickle" in msg, (name, st, msg)


@pytest.mark.parametrize("header_len", [0x380, 0x1080, 0x4B50, 0x14B50], ids=hex)
def test_a_header_length_that_looks_like_a_pickle_is_no_pickle(tmp_path, header_len):
    """A .safetensors file opens with its header's length as a little-endian u64, so its first byte can be 0x80 (a pickle stream's) and its first two "PK" (a zip
    archive's): a valid adapter whose header is padded to such a length loads like any other."""
    d = SMALL
    src, path = tmp_path / "a.safetensors", tmp_path / "padded.safetensors"
    write_ip_adapter_safetensors(src, syn.ip_adapter(d.model_channels, d.ctx_dim, 64, 4), "F16")
    raw = src.read_bytes()
    n = int.from_bytes(raw[:8], "little")
    header = raw[8:8 + n].rstrip(b" ")
    if header_len < len(header):
        header_len += (len(header) - header_len + 0xFFFF) // 0x10000 * 0x10000      # the same low 16 bits, long enough
    path.write_bytes(header_len.to_bytes(8, "little") + header.ljust(header_len, b" ") + raw[8 + n:])
    first = path.read_bytes()[:2]
    assert first[0] == 0x80 or first == b"PK"
    assert ip_adapter_check_safetensors(ModelConfig(d.model_channels, d.n_head, d.ctx_dim), path) == (64, 4)
    assert {key: shape for key, _, shape, _, _ in safetensors_list(path)} == {key: shape for key, _, shape, _, _ in safetensors_list(src)}


# ---- the reference's own identities -------------------------------------------------------------------------------------------------------------------------
def test_one_image_token_adds_its_value():
    """T_ip = 1: the softmax over one key is 1, so the image term is V_ip itself"""
    g = np.random.default_rng(0)
    n, nq, heads, dh = 2, 5, 4, 40
    c = heads * dh
    q, o = g.standard_normal((n, nq, c)), g.standard_normal((n, nq, c))
    k, v = g.standard_normal((n, 1, c)), g.standard_normal((n, 1, c))
    s = np.array([0.7, -1.3])
    assert np.allclose(IR.op(q, k, v, o, s, heads), o + s[:, None, None] * v, rtol=0, atol=1e-15)
    assert np.array_equal(IR.op(q, k, v, o, [0.0, 0.0], heads), o)


def test_the_operator_is_the_oracles_attention():
    g = np.random.default_rng(1)
    n, nq, T, heads, dh = 2, 7, 5, 2, 80
    c = heads * dh
    q, k, v = g.standard_normal((n, nq, c)), g.standard_normal((n, T, c)), g.standard_normal((n, T, c))
    ref = O.qkv_attention(torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(v), None, heads).numpy()
    assert np.abs(IR.attention(q, k, v, heads) - ref).max() < 1e-13


def test_image_proj_is_torch_layer_norm():
    d = SMALL
    ad = syn.ip_adapter(d.model_channels, d.ctx_dim, 64, 4)
    e = syn.image_embeds(0, 3, 64)
    w, b = (torch.from_numpy(ad[f"image_proj.proj.{k}"]).double() for k in ("weight", "bias"))
    y = (torch.from_numpy(e).double() @ w.T + b).reshape(3, 4, d.ctx_dim)
    ref = torch.nn.functional.layer_norm(y, (d.ctx_dim,), torch.from_numpy(ad["image_proj.norm.weight"]).double(), torch.from_numpy(ad["image_proj.norm.bias"]).double(), 1e-5)
    got = IR.image_proj(ad, e, d.ctx_dim)
    assert got.shape == (3, 4, d.ctx_dim) and np.abs(got - ref.numpy()).max() < 1e-12
    assert IR.tokens_of(ad, e, d.ctx_dim).shape == (12, d.ctx_dim)
    z = IR.zero_tokens(ad, d.ctx_dim, 2)
    assert np.array_equal(z[:4], z[4:]) and np.abs(z).max() > 0        # image_proj(0) is the bias through the norm, not zero


def test_scale_zero_is_the_plain_forward():
    d = O.Dims(32, 1, 32, 8, 8, 32)     # the identity needs no particular width: the smallest model the oracle builds
    w = syn.SyntheticWeights(cache=True)
    ad = syn.ip_adapter(d.model_channels, d.ctx_dim, 32, 4)
    lat = torch.from_numpy(np.stack([syn.initial_latent(i, 8, 8) for i in range(2)]))
    ctx = torch.from_numpy(np.stack([syn.cond_context(i, 5, d.ctx_dim) for i in range(2)]))
    tokens = np.stack([IR.tokens_of(ad, syn.image_embeds(i, 1, 32), d.ctx_dim) for i in range(2)])
    unet = IR.IpUNetOracle(w, d, torch.float64)
    plain = O.UNetOracle(w, d, torch.float64).forward(lat, 500, ctx)
    assert torch.equal(IR.ip_forward(unet, lat, 500, ctx, None), plain)
    assert torch.equal(IR.ip_forward(unet, lat, 500, ctx, (ad, tokens, 0.0)), plain)
    on = IR.ip_forward(unet, lat, 500, ctx, (ad, tokens, 1.0))
    assert (on - plain).abs().max() > 1e-4, "the image term does not reach the output"
    pred = IR.IpPredictor(w, d, torch.float64, ad, tokens, tokens, 1.0, 0.5, 0.5, 4)
    assert pred.on == set()


def test_the_kernel_does_not_spill(tmp_path):
    """test_code_objects_cpu's check, on the new translation unit (its HOT list is that file's own)"""
    from test_code_objects_cpu import _functions
    funcs = _functions("k_ipattn", tmp_path)
    kernels = {k: v for k, v in funcs.items() if "ip_attention_kernel" in k}
    assert len(kernels) == 12, sorted(kernels)          # head widths 40 / 64 / 80 / 160 x the three output forms
    for name, body in kernels.items():
        assert "scratch_" not in body, f"{name} uses scratch memory"
