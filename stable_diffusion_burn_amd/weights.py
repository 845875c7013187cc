"""The reference's npy-dump weight format, reader and writer.

Format (defined by the reference's exporters python/save.py:6-68 and read by
src/model/load.rs:17-160): every tensor is a 1-D float32 `.npy` whose first D values are the
shape and whose remaining values are the row-major data; a scalar s is stored as `[1.0, s]`;
Linear `weight` is stored TRANSPOSED to [in, out] (save.py:19); a Conv2d directory holds
`weight [Cout,Cin,kh,kw]`, `bias`, and the 2-vectors `stride`, `padding`, `dilation`,
`kernel_size` plus scalars `n_group`, `n_channels_in`, `n_channels_out`; a GroupNorm directory
holds `weight`, `bias`, `eps`, `n_group`, `n_channel`; a LayerNorm directory `weight`, `bias`, `eps`.
Directory names are the Rust struct field names (src/model/unet/load.rs, autoencoder/load.rs).

The engine's C++ reader (`sdmi_load_weights_dir`, csrc/engine.cpp) reads the `weight` / `bias`
files of the hot-path subset; `write_dump_tree` here writes the COMPLETE per-module file set the
Rust loaders expect, so a tree written from any provider (e.g. synthetic weights) is loadable by
both.  tests/test_reference_python_cpu.py checks the writer byte-for-byte against files produced
by the reference's own exporters (tests/golden/refdump/).
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np


def encode_tensor(a) -> np.ndarray:
    """save_tensor (python/save.py:10-15): [dims..., values...] as float32."""
    a = np.asarray(a, dtype=np.float32)
    return np.concatenate((np.array(a.shape, dtype=np.float64), a.reshape(-1).astype(np.float64))).astype(np.float32)


def encode_scalar(s) -> np.ndarray:
    """save_scalar (python/save.py:6-8)."""
    return np.array([1.0, float(s)]).astype(np.float32)


def read_tensor(path, ndim: int) -> np.ndarray:
    """numpy_to_tensor (src/model/load.rs:17-28) for a tensor of known rank."""
    raw = np.load(path)
    if raw.ndim != 1 or raw.dtype != np.float32:
        raise ValueError(f"{path}: expected a 1-D float32 array")
    dims = tuple(int(v) for v in raw[:ndim])
    if raw.size != ndim + int(np.prod(dims)):
        raise ValueError(f"{path}: shape prefix {dims} does not match {raw.size - ndim} values")
    return raw[ndim:].reshape(dims)


def _save(path: Path, arr: np.ndarray) -> None:
    path.parent.mkdir(parents=True, exist_ok=True)
    np.save(path, arr)


def write_conv2d(dirpath, weight, bias, stride=1, padding=0, dilation=1) -> None:
    """save_conv2d (python/save.py:52-68)."""
    d = Path(dirpath)
    weight = np.asarray(weight, np.float32)
    _save(d / "weight.npy", encode_tensor(weight))
    if bias is not None:
        _save(d / "bias.npy", encode_tensor(bias))
    for name, v in (("stride", stride), ("padding", padding), ("dilation", dilation), ("kernel_size", weight.shape[2:])):
        pair = (v, v) if np.isscalar(v) else tuple(v)
        _save(d / f"{name}.npy", encode_tensor(np.array(pair, np.float32)))
    _save(d / "n_group.npy", encode_scalar(1))
    _save(d / "n_channels_in.npy", encode_scalar(weight.shape[1]))
    _save(d / "n_channels_out.npy", encode_scalar(weight.shape[0]))


def write_linear(dirpath, weight_in_out, bias) -> None:
    """save_linear (python/save.py:17-21); `weight_in_out` is already [in, out] (what the file holds)."""
    d = Path(dirpath)
    _save(d / "weight.npy", encode_tensor(weight_in_out))
    if bias is not None:
        _save(d / "bias.npy", encode_tensor(bias))


def write_group_norm(dirpath, gamma, beta, eps=1e-5, n_group=32) -> None:
    """save_group_norm (python/save.py:29-37)."""
    d = Path(dirpath)
    _save(d / "weight.npy", encode_tensor(gamma))
    _save(d / "bias.npy", encode_tensor(beta))
    _save(d / "eps.npy", encode_scalar(eps))
    _save(d / "n_group.npy", encode_scalar(n_group))
    _save(d / "n_channel.npy", encode_scalar(len(gamma)))


def write_layer_norm(dirpath, gamma, beta, eps=1e-5) -> None:
    """save_layer_norm (python/save.py:23-27)."""
    d = Path(dirpath)
    _save(d / "weight.npy", encode_tensor(gamma))
    _save(d / "bias.npy", encode_tensor(beta))
    _save(d / "eps.npy", encode_scalar(eps))


def write_embedding(dirpath, weight) -> None:
    """save_embedding (python/save.py:97-99): the table as it is, [rows, width] (not transposed)."""
    _save(Path(dirpath) / "weight.npy", encode_tensor(weight))


def write_dump_tree(dump_dir, specs, get_tensor, alphas_cumprod, n_head: int = 8, clip_heads: int = 12) -> None:
    """Write the hot-path subset of the dump tree (+ the clip/ subtree when `specs` lists it).

    specs: [(name, shape)] from StableDiffusion.weight_specs(); get_tensor(name, shape) -> ndarray in
    the dump's own layout (Linear [in,out], Conv [Cout,Cin,kh,kw]).
    """
    root = Path(dump_dir)
    shapes = dict(specs)
    modules = {}
    for name, shape in specs:
        if name == "alphas_cumprod":
            continue
        parent, leaf = name.rsplit("/", 1)
        modules.setdefault(parent, {})[leaf] = get_tensor(name, shape)
    for parent, t in modules.items():
        w = t["weight"]
        b = t.get("bias")
        leaf_dir = parent.rsplit("/", 1)[1]
        if parent.startswith("clip/") and leaf_dir.endswith("_embedding"):
            write_embedding(root / parent, w)                                   # python/clip.py:32-35
        elif parent.startswith("clip/") and w.ndim == 1:
            write_layer_norm(root / parent, w, b)                               # attn_ln / mlp_ln / layer_norm
        elif w.ndim == 4 and parent.endswith("/downsampler/conv"):
            write_conv2d(root / parent, w, b, stride=2, padding=0)              # save_padded_conv2d (python/save.py:70-77)
        elif w.ndim == 4:
            k = w.shape[2]
            stride = 2 if parent.rsplit("/", 1)[1] in ("d1", "d2", "d3") else 1   # Downsample (unet/mod.rs:408-427)
            if parent in ("controlnet/hint/c2", "controlnet/hint/c4", "controlnet/hint/c6"):
                stride = 2                                                        # a ControlNet's input_hint_block halves the picture three times
            write_conv2d(root / parent, w, b, stride=stride, padding=1 if k == 3 else 0)
        elif w.ndim == 2:
            write_linear(root / parent, w, b)
        elif parent.rsplit("/", 1)[1] in ("norm1", "norm2", "norm3") and "/transformer/transformer/" in parent + "/":
            write_layer_norm(root / parent, w, b)
        else:
            write_group_norm(root / parent, w, b)
        if parent.rsplit("/", 1)[1] in ("attn1", "attn2"):
            pass
    for parent in {p.rsplit("/", 1)[0] for p in modules if p.rsplit("/", 1)[1] in ("query",)}:
        heads = clip_heads if parent.startswith("clip/") else n_head               # unet/load.rs:46, clip/load.rs:33
        _save(root / parent / "n_head.npy", encode_scalar(heads))
    clip_blocks = {p.split("/")[2] for p in modules if p.startswith("clip/blocks/")}
    if clip_blocks:
        _save(root / "clip" / "n_layer.npy", encode_scalar(len(clip_blocks)))      # python/clip.py:29, clip/load.rs:74
    a = np.asarray(alphas_cumprod, np.float32)
    _save(root / "n_steps.npy", encode_scalar(len(a)))                                # stablediffusion/load.rs:20
    _save(root / "alphas_cumprod.npy", encode_tensor(a))
    if any(n.startswith("autoencoder/decoder/blocks/") for n in shapes):
        _save(root / "autoencoder/decoder/n_block.npy", encode_scalar(4))           # autoencoder/load.rs:139
    if any(n.startswith("autoencoder/encoder/blocks/") for n in shapes):
        _save(root / "autoencoder/encoder/n_block.npy", encode_scalar(4))           # autoencoder/load.rs:163


# ---- .safetensors: SD v1.x checkpoints in the CompVis layout ---------------------------------------------
# The format: 8 bytes little-endian header length, a JSON header {key: {"dtype", "shape", "data_offsets": [begin, end]}} (+ an optional
# "__metadata__" {str: str}), then the tensors' bytes back to back; offsets are relative to the end of the header.

_ST_DTYPES = {np.dtype(np.float32): "F32", np.dtype(np.float16): "F16", np.dtype(np.float64): "F64", np.dtype(np.int64): "I64",
              np.dtype(np.int32): "I32", np.dtype(np.uint8): "U8"}


def bf16_bits(a) -> np.ndarray:
    """float32 -> the uint16 bit patterns of its bfloat16 rounding (to nearest, ties to even; NaN stays NaN)."""
    a = np.ascontiguousarray(a, np.float32)
    bits = a.view(np.uint32)
    rounded = ((bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(a), np.uint16(0x7FC0), rounded).astype(np.uint16)


def bf16_to_f32(bits) -> np.ndarray:
    """uint16 bfloat16 bit patterns -> float32 (exact)."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def write_safetensors(path, tensors: dict, metadata: dict | None = None) -> None:
    """Write {key: ndarray} as one .safetensors file, without the safetensors package.

    The dtype follows the array: float32 F32, float16 F16, float64 F64, int64 I64, int32 I32, uint8 U8.  bfloat16 has no numpy type: pass
    (uint16 array of bit patterns, "BF16") -- any (array, tag) pair stores the array's bytes under that tag.
    """
    header, arrays, off = {}, [], 0
    if metadata:
        header["__metadata__"] = {str(k): str(v) for k, v in metadata.items()}
    for key, value in tensors.items():
        if isinstance(value, tuple):
            arr, tag = np.asarray(value[0]), str(value[1])
        else:
            arr = np.asarray(value)
            if arr.dtype not in _ST_DTYPES:
                raise TypeError(f"write_safetensors: '{key}' has dtype {arr.dtype}; pass (array, tag) for anything but {sorted(_ST_DTYPES.values())}")
            tag = _ST_DTYPES[arr.dtype]
        shape = [int(d) for d in arr.shape]
        arr = np.ascontiguousarray(arr.astype(arr.dtype.newbyteorder("<"), copy=False)).reshape(-1)   # little-endian bytes, row-major
        header[str(key)] = {"dtype": tag, "shape": shape, "data_offsets": [off, off + arr.nbytes]}
        arrays.append(arr)
        off += arr.nbytes
    text = json.dumps(header, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 8)
    with open(path, "wb") as f:
        f.write(len(text).to_bytes(8, "little"))
        f.write(text)
        for arr in arrays:
            if arr.nbytes:
                f.write(arr.view(np.uint8).data)


def write_checkpoint_safetensors(path, specs, get_tensor, alphas_cumprod, dtype: str = "F32", key_of=None, extra: dict | None = None, variant: int = 0) -> None:
    """Write a model in the CHECKPOINT's naming and layouts: the inverse of the loader's key map and the twin of write_dump_tree.

    specs: [(dump name, shape)] from StableDiffusion.weight_specs(); get_tensor(name, shape) -> ndarray in the dump's own layout (Linear
    [in,out], Conv [Cout,Cin,kh,kw]): a Linear weight is stored transposed back to torch's [out,in].  dtype "F32" | "F16" | "BF16" for the
    model's tensors; alphas_cumprod stays F32 (None: the file gets none).  key_of(dump name) -> (checkpoint key, transposed?), default
    pipeline.checkpoint_key (the C++ rules).  extra: further {key: tensor} entries, written as write_safetensors takes them.
    variant (ModelConfig.variant of the context the specs come from) 1: Stability's SD 2.x layout -- the text encoder's query / key / value weights and biases
    fused into attn.in_proj_weight [3C, C] / in_proj_bias [3C] (all three must be among the specs), the transformers' proj_in / proj_out written 2-D [C, C].
    """
    if dtype not in ("F32", "F16", "BF16"):
        raise ValueError(f"write_checkpoint_safetensors: dtype must be F32, F16 or BF16, got {dtype!r}")
    if variant not in (0, 1):
        raise ValueError(f"write_checkpoint_safetensors: variant must be 0 or 1, got {variant!r}")
    if key_of is None:
        from .pipeline import checkpoint_key
        key_of = (lambda name: checkpoint_key(name, variant, with_slice=True)) if variant else checkpoint_key
    tensors, fused = {}, {}
    for name, shape in specs:
        if name == "alphas_cumprod":
            if alphas_cumprod is not None:
                tensors["alphas_cumprod"] = np.asarray(alphas_cumprod, np.float32)
            continue
        key, transposed, *part = key_of(name)
        a = np.asarray(get_tensor(name, shape), np.float32)
        if transposed:
            a = np.ascontiguousarray(a.T)
        if variant == 1 and a.ndim == 4 and a.shape[2:] == (1, 1) and key.startswith("model.diffusion_model.") and key.endswith((".proj_in.weight", ".proj_out.weight")):
            a = a.reshape(a.shape[:2])   # nn.Linear in SD 2.x
        if part and part[0] is not None:   # a third of a fused tensor: kept until the key's three parts are there
            fused.setdefault(key, {})[part[0]] = a
            tensors.setdefault(key, None)   # the key's place in the file's order
            continue
        tensors[key] = a if dtype == "F32" else a.astype(np.float16) if dtype == "F16" else (bf16_bits(a), "BF16")
    for key, parts in fused.items():
        if sorted(parts) != [0, 1, 2]:
            raise ValueError(f"write_checkpoint_safetensors: '{key}' needs its query, key and value parts, got {sorted(parts)}")
        a = np.concatenate([parts[0], parts[1], parts[2]], axis=0)
        tensors[key] = a if dtype == "F32" else a.astype(np.float16) if dtype == "F16" else (bf16_bits(a), "BF16")
    tensors.update(extra or {})
    write_safetensors(path, tensors)


def write_lora_safetensors(path, tensors: dict, dtype: str = "F16", style: str = "kohya", extra: dict | None = None) -> None:
    """Write an adapter as a kohya-ss / LyCORIS .safetensors file: the inverse of StableDiffusion.lora_load_safetensors (and the way to convert an .npz:
    write_lora_safetensors(path, load_lora_npz(npz))).

    tensors: {dump target: (down, up, alpha)} as lora_attach takes them -- written as "<module>.lora_down.weight" ([r, in], a conv's [r, cin, k, k]),
    "<module>.lora_up.weight" ([out, r], a conv's [out, r, 1, 1]) and "<module>.alpha" (left out when alpha is None: the loader then takes alpha = r) -- or
    {dump target: (w1_a, w1_b, w2_a, w2_b, alpha)}, a LoHa module: "<module>.hada_w1_a" [out, r], "hada_w1_b" [r, in] (a conv's [r, cin k k]), and w2 alike.
    dtype "F32" | "F16" | "BF16" for the factors; alpha is one number of the same dtype, as the trainers write it.  style "kohya": modules named after
    the diffusers path (pipeline.lora_module_name); "compvis": after the CompVis key with "_" for ".".  extra: further {key: tensor} entries."""
    if dtype not in ("F32", "F16", "BF16"):
        raise ValueError(f"write_lora_safetensors: dtype must be F32, F16 or BF16, got {dtype!r}")
    if style not in ("kohya", "compvis"):
        raise ValueError(f"write_lora_safetensors: style must be 'kohya' or 'compvis', got {style!r}")
    from .pipeline import checkpoint_key, lora_module_name

    def stored(a):
        a = np.asarray(a, np.float32)   # (a 0-d alpha stays 0-d: kohya-ss writes a scalar)
        return a if dtype == "F32" else a.astype(np.float16) if dtype == "F16" else (bf16_bits(a).reshape(a.shape), "BF16")

    out = {}
    for target, item in tensors.items():
        module = lora_module_name(target)
        if style == "compvis" and module.startswith("lora_unet_"):
            module = "lora_unet_" + checkpoint_key(target)[0][len("model.diffusion_model."):-len(".weight")].replace(".", "_")
        if len(item) == 3:
            down, up, alpha = item
            down, up = np.asarray(down, np.float32), np.asarray(up, np.float32)
            if down.ndim == 4:
                up = up.reshape(up.shape[0], up.shape[1], 1, 1)
            out[module + ".lora_down.weight"], out[module + ".lora_up.weight"] = stored(down), stored(up)
        elif len(item) == 5:
            w1_a, w1_b, w2_a, w2_b, alpha = item
            for key, w in (("hada_w1_a", w1_a), ("hada_w1_b", w1_b), ("hada_w2_a", w2_a), ("hada_w2_b", w2_b)):
                w = np.asarray(w, np.float32)
                out[f"{module}.{key}"] = stored(w.reshape(w.shape[0], -1))
        else:
            raise ValueError(f"write_lora_safetensors: '{target}': expected (down, up, alpha) or (w1_a, w1_b, w2_a, w2_b, alpha)")
        if alpha is not None:
            out[module + ".alpha"] = stored(np.float32(alpha))
    out.update(extra or {})
    write_safetensors(path, out)


# ---- ControlNet: the weight group controlnet/... and its cldm-layout .safetensors file ---------------------
CONTROL_HINT_WIDTHS = (16, 16, 32, 32, 96, 96, 256)   # ControlNet's constants: they do not scale with model_channels


def control_specs(dims, hint_ch: int = 3) -> list:
    """[(dump name, shape)] of the ControlNet group of a model with `dims` (.model_channels, .ctx_dim), in the engine's order
    (StableDiffusion.weight_specs() of a context with control_hint_ch = 3 lists the same entries): the time MLP, the 12 input
    blocks and the middle block under the UNet's own names, the hint convolutions, the zero convolutions, middle_block_out."""
    mc, cd = int(dims.model_channels), int(dims.ctx_dim)
    ed, c1, c2, c4 = 4 * mc, mc, 2 * mc, 4 * mc
    out = []

    def conv(p, cin, cout, k):
        out.extend([(p + "/weight", (cout, cin, k, k)), (p + "/bias", (cout,))])

    def lin(p, cin, cout, bias=True):
        out.append((p + "/weight", (cin, cout)))
        if bias:
            out.append((p + "/bias", (cout,)))

    def norm(p, c):
        out.extend([(p + "/weight", (c,)), (p + "/bias", (c,))])

    def res(p, cin, cout):
        norm(p + "/norm_in", cin)
        conv(p + "/conv_in", cin, cout, 3)
        lin(p + "/lin_embed", ed, cout)
        norm(p + "/norm_out", cout)
        conv(p + "/conv_out", cout, cout, 3)
        if cin != cout:
            conv(p + "/skip_connection", cin, cout, 1)

    def mha(p, c, cctx):
        lin(p + "/query", c, c, False)
        lin(p + "/key", cctx, c, False)
        lin(p + "/value", cctx, c, False)
        lin(p + "/out", c, c)

    def spatial(p, c):
        norm(p + "/norm", c)
        conv(p + "/proj_in", c, c, 1)
        t = p + "/transformer"
        norm(t + "/norm1", c)
        mha(t + "/attn1", c, c)
        norm(t + "/norm2", c)
        mha(t + "/attn2", c, cd)
        norm(t + "/norm3", c)
        lin(t + "/mlp/geglu/proj", c, 8 * c)
        lin(t + "/mlp/lin", 4 * c, c)
        conv(p + "/proj_out", c, c, 1)

    root = "controlnet"
    lin(root + "/lin1_time_embed", mc, ed)
    lin(root + "/lin2_time_embed", ed, ed)
    blocks = [("conv", "conv", 4, c1), ("rt", "rt1", c1, c1), ("rt", "rt2", c1, c1), ("down", "d1", c1, c1), ("rt", "rt3", c1, c2), ("rt", "rt4", c2, c2),
              ("down", "d2", c2, c2), ("rt", "rt5", c2, c4), ("rt", "rt6", c4, c4), ("down", "d3", c4, c4), ("r", "r1", c4, c4), ("r", "r2", c4, c4)]
    for kind, name, cin, cout in blocks:
        p = f"{root}/input_blocks/{name}"
        if kind in ("conv", "down"):
            conv(p, cin, cout, 3)
        elif kind == "r":
            res(p, cin, cout)
        else:
            res(p + "/res", cin, cout)
            spatial(p + "/transformer", cout)
    res(root + "/middle_block/res1", c4, c4)
    spatial(root + "/middle_block/transformer", c4)
    res(root + "/middle_block/res2", c4, c4)
    widths = (int(hint_ch),) + CONTROL_HINT_WIDTHS + (mc,)
    for i in range(8):
        conv(f"{root}/hint/c{i}", widths[i], widths[i + 1], 3)
    for j, (_, _, _, cout) in enumerate(blocks):
        conv(f"{root}/zero_convs/{j}", cout, cout, 1)
    conv(root + "/middle_block_out", c4, c4, 1)
    return out


def write_control_safetensors(path, provider_or_dict, dims, dtype: str = "F32", key_of=None, extra: dict | None = None) -> None:
    """Write a ControlNet in the cldm layout ("control_model.…"): the inverse of sdmi_load_control_safetensors.

    provider_or_dict: a provider (.get(name, shape, kind, fan_in), e.g. synthetic.SyntheticWeights) or {dump name: ndarray in the dump's
    layout} holding every entry of control_specs(dims).  dtype "F32" | "F16" | "BF16".  key_of / extra: as write_checkpoint_safetensors."""
    specs = control_specs(dims)
    if hasattr(provider_or_dict, "get") and not isinstance(provider_or_dict, dict):
        from .synthetic import named_tensor
        shapes = dict(specs)
        get = lambda name, shape: named_tensor(provider_or_dict, name, shape, shapes)   # noqa: E731
    else:
        def get(name, shape):
            a = np.asarray(provider_or_dict[name], np.float32)
            if tuple(a.shape) != tuple(shape):
                raise ValueError(f"write_control_safetensors: '{name}' has shape {tuple(a.shape)}, expected {tuple(shape)}")
            return a
    write_checkpoint_safetensors(path, specs, get, None, dtype, key_of=key_of, extra=extra)


# ---- IP-Adapter: h94's ip-adapter_sd15.safetensors layout -------------------------------------------------------
def write_ip_adapter_safetensors(path, arrays: dict, dtype: str = "F32") -> None:
    """Write an IP-Adapter {file key: array in the file's layout} (synthetic.ip_adapter makes one): the inverse of sdmi_ip_adapter_load_safetensors.
    dtype "F32" | "F16" | "BF16": what every tensor is stored as."""
    if dtype not in ("F32", "F16", "BF16"):
        raise ValueError(f"write_ip_adapter_safetensors: dtype must be F32, F16 or BF16, got {dtype!r}")
    out = {}
    for key, a in arrays.items():
        a = np.ascontiguousarray(a, np.float32)
        out[key] = a if dtype == "F32" else a.astype(np.float16) if dtype == "F16" else (bf16_bits(a).reshape(a.shape), "BF16")
    write_safetensors(path, out)
