"""Host side of the SD v1.x .safetensors checkpoint loader: the key map against the fixture the reference's own Python
model and exporters wrote (tests/golden/gen_ckpt_keys.py), the reader's listing on files written by weights.write_safetensors (and by the
safetensors package when it imports), every malformed case the reader must refuse, the reader and the key rules under ASan + UBSan as a
plain program, and the default schedule.  No GPU."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "stable_diffusion_burn_amd" / "csrc"
FIXTURE = ROOT / "tests" / "golden" / "sd14_ckpt_keys.txt"
ERR_INVALID, ERR_WEIGHTS, ERR_IO = -1, -3, -4


@pytest.fixture(scope="module")
def sdmi():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)
    import stable_diffusion_burn_amd as pkg
    return pkg


def fixture_rows():
    rows = [ln.split("\t") for ln in FIXTURE.read_text().splitlines()]
    assert all(len(r) == 4 for r in rows)
    return [(d, k, tuple(int(v) for v in s.split(",")), t == "T") for d, k, s, t in rows]


def test_status_codes_are_the_headers():
    text = (ROOT / "include" / "sdmi.h").read_text()
    for name, value in (("SDMI_ERR_INVALID", ERR_INVALID), ("SDMI_ERR_IO", ERR_IO), ("SDMI_ERR_WEIGHTS", ERR_WEIGHTS)):
        import re
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text), name


def test_key_map_reproduces_the_fixture(sdmi):
    rows = fixture_rows()
    assert len(rows) == 1131 and FIXTURE.stat().st_size < 256 * 1024
    keys = set()
    for dump, key, shape, transposed in rows:
        assert sdmi.checkpoint_key(dump) == (key, transposed), dump
        assert not transposed or len(shape) == 2
        keys.add(key)
    assert len(keys) == len(rows), "two dump names share a checkpoint key"
    assert len({r[0] for r in rows}) == len(rows)
    by_dump = {r[0]: r for r in rows}
    assert by_dump["unet/input_blocks/rt1/transformer/transformer/mlp/geglu/proj/weight"][1:] == (
        "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.ff.net.0.proj.weight", (2560, 320), True)
    assert by_dump["autoencoder/encoder/mid/attn/v/weight"][1:] == ("first_stage_model.encoder.mid.attn_1.v.weight", (512, 512, 1, 1), False)
    assert by_dump["alphas_cumprod"][1:] == ("alphas_cumprod", (1000,), False)


@pytest.mark.parametrize("name", ["n_steps", "unet/norm_out/eps", "unet/norm_out/n_group", "unet/input_blocks/conv/stride", "clip/n_layer",
                                  "unet/input_blocks/rt1/transformer/transformer/attn1/n_head", "autoencoder/decoder/n_block", "", "unet",
                                  "unet/input_blocks/rt7/res/conv_in/weight", "clip/token_embedding/bias", "unet/conv_out/weight/",
                                  "unet/input_blocks/rt1/transformer/transformer/attn1/query/bias", "unet/middle_block/transformer/transformer/attn2/value/bias"])
def test_names_without_a_checkpoint_source_are_invalid(sdmi, name):
    with pytest.raises(sdmi.SdmiError) as ei:
        sdmi.checkpoint_key(name)
    assert ei.value.status == ERR_INVALID and "no checkpoint source" in str(ei.value)


def test_key_buffer_convention(sdmi):
    from stable_diffusion_burn_amd._capi import load_library
    lib = load_library()
    need, tr = C.c_size_t(), C.c_int32(7)
    assert lib.sdmi_checkpoint_key(b"unet/lin1_time_embed/weight", None, 0, C.byref(need), C.byref(tr)) == 0
    assert need.value == len("model.diffusion_model.time_embed.0.weight") + 1 and tr.value == 1
    small = C.create_string_buffer(4)
    assert lib.sdmi_checkpoint_key(b"unet/lin1_time_embed/weight", small, 4, C.byref(need), None) == ERR_INVALID
    assert lib.sdmi_checkpoint_key(None, None, 0, C.byref(need), None) == ERR_INVALID


def _sample_tensors(W):
    g = np.random.default_rng(3)
    return {
        "model.diffusion_model.out.2.weight": g.standard_normal((4, 8, 3, 3)).astype(np.float16),
        "model.diffusion_model.time_embed.0.weight": g.standard_normal((12, 5)).astype(np.float32),
        "first_stage_model.decoder.up.0.block.2.norm1.bias": (W.bf16_bits(g.standard_normal(7).astype(np.float32)), "BF16"),
        "cond_stage_model.transformer.text_model.embeddings.position_ids": np.arange(77, dtype=np.int64)[None],
        "model_ema.decay": np.array(0.9999, np.float32),
        "alphas_cumprod": np.linspace(1, 0, 10, dtype=np.float64),
        'odd "key"\\ \n\té \U0001F680': np.zeros((2, 0, 3), np.float32),
    }


def test_listing_of_a_written_file(sdmi, tmp_path):
    from stable_diffusion_burn_amd import weights as W
    tensors = _sample_tensors(W)
    path = tmp_path / "a.safetensors"
    W.write_safetensors(path, tensors, metadata={"format": "pt", "note": "x"})
    raw = path.read_bytes()
    hlen = int.from_bytes(raw[:8], "little")
    header = json.loads(raw[8:8 + hlen])
    listing = sdmi.safetensors_list(path)
    assert [r[0] for r in listing] == list(tensors)            # header order; escapes (quote, backslash, control, \u, a surrogate pair) decoded
    want_names = {"model.diffusion_model.out.2.weight": "unet/conv_out/weight", "model.diffusion_model.time_embed.0.weight": "unet/lin1_time_embed/weight",
                  "first_stage_model.decoder.up.0.block.2.norm1.bias": "autoencoder/decoder/blocks/3/res3/norm1/bias", "alphas_cumprod": "alphas_cumprod"}
    for key, dtype, shape, off, name in listing:
        v = tensors[key]
        arr = v[0] if isinstance(v, tuple) else v
        assert dtype == header[key]["dtype"] and shape == tuple(arr.shape) and name == want_names.get(key)
        assert off == 8 + hlen + header[key]["data_offsets"][0]
        assert raw[off:off + arr.nbytes] == arr.tobytes()
    assert {r[1] for r in listing} == {"F16", "F32", "BF16", "I64", "F64"}


def test_listing_of_a_file_written_by_the_safetensors_package(sdmi, tmp_path):
    st = pytest.importorskip("safetensors.numpy")
    g = np.random.default_rng(4)
    tensors = {"model.diffusion_model.input_blocks.0.0.weight": g.standard_normal((8, 4, 3, 3)).astype(np.float16),
               "cond_stage_model.transformer.text_model.final_layer_norm.bias": g.standard_normal(16).astype(np.float32),
               "something.else": np.arange(6, dtype=np.int64).reshape(2, 3)}
    path = tmp_path / "pkg.safetensors"
    st.save_file(tensors, str(path), metadata={"format": "pt"})
    raw = path.read_bytes()
    listing = {r[0]: r for r in sdmi.safetensors_list(path)}
    assert set(listing) == set(tensors)
    for key, arr in tensors.items():
        _, dtype, shape, off, name = listing[key]
        assert dtype == {"float16": "F16", "float32": "F32", "int64": "I64"}[arr.dtype.name] and shape == arr.shape
        assert raw[off:off + arr.nbytes] == arr.tobytes()
    assert listing["model.diffusion_model.input_blocks.0.0.weight"][4] == "unet/input_blocks/conv/weight"
    assert listing["cond_stage_model.transformer.text_model.final_layer_norm.bias"][4] == "clip/layer_norm/bias"
    assert listing["something.else"][4] is None
    # and the writer here produces what the package reads
    from stable_diffusion_burn_amd import weights as W
    W.write_safetensors(tmp_path / "own.safetensors", tensors, metadata={"format": "pt"})
    back = st.load_file(str(tmp_path / "own.safetensors"))
    assert set(back) == set(tensors) and all(np.array_equal(back[k], tensors[k]) and back[k].dtype == tensors[k].dtype for k in tensors)


def test_listing_names_every_key_of_the_fixture(sdmi, tmp_path):
    """one file holding EVERY checkpoint key of the fixture (1-element tensors: the listing does not look at shapes), a 13th CLIP layer and foreign keys"""
    from stable_diffusion_burn_amd import weights as W
    rows = fixture_rows()
    one = np.zeros(1, np.float16)
    tensors = {key: one for _, key, _, _ in rows}
    layer = "cond_stage_model.transformer.text_model.encoder.layers."
    tensors[layer + "23.mlp.fc1.weight"] = one
    foreign = ["model_ema.decay", layer + "0.mlp.fc3.weight", layer + "x.mlp.fc1.weight", "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_q.bias",
               "model.diffusion_model.input_blocks.12.0.in_layers.0.weight", "first_stage_model.decoder.up.4.block.0.conv1.weight"]
    tensors.update({k: one for k in foreign})
    W.write_safetensors(tmp_path / "all.safetensors", tensors)
    listing = {r[0]: r[4] for r in sdmi.safetensors_list(tmp_path / "all.safetensors")}
    assert len(listing) == len(rows) + 1 + len(foreign)
    wrong = [(dump, key, listing[key]) for dump, key, _, _ in rows if listing[key] != dump]
    assert not wrong, wrong[:5]
    assert listing[layer + "23.mlp.fc1.weight"] == "clip/blocks/23/mlp/fc1/weight"
    assert all(listing[k] is None for k in foreign)


def _file(path, header: bytes, data: bytes = b"", hlen=None):
    path.write_bytes((len(header) if hlen is None else hlen).to_bytes(8, "little") + header + data)
    return path


def _entry(dtype="F32", shape=(2,), offsets=(0, 8)):
    return {"dtype": dtype, "shape": list(shape), "data_offsets": list(offsets)}


MALFORMED = {
    # name: (header bytes or dict, data bytes, forced header length or None, words the message must hold)
    "header length larger than the file": ({"a": _entry()}, b"\0" * 8, 10_000, "exceeds the file"),
    "header length larger than 100 MB": ({"a": _entry()}, b"\0" * 8, 100_000_001, "100 MB"),
    "header length 2^63": ({"a": _entry()}, b"\0" * 8, 1 << 63, "100 MB"),
    "offsets outside the data section": ({"a": _entry(offsets=(0, 8))}, b"\0" * 4, None, "outside the data section"),
    "offsets far outside": ({"a": _entry(shape=(1 << 40,), offsets=(0, 1 << 42))}, b"\0" * 8, None, "outside the data section"),
    "offsets reversed": ({"a": _entry(offsets=(8, 0))}, b"\0" * 8, None, "reversed"),
    "offsets overlapping": ({"a": _entry(offsets=(0, 8)), "b": _entry(offsets=(4, 12))}, b"\0" * 12, None, "overlap"),
    "shape does not match the byte length": ({"a": _entry(shape=(3,), offsets=(0, 8))}, b"\0" * 8, None, "data_offsets span 8"),
    "dtype size does not match": ({"a": _entry(dtype="F16", shape=(2,), offsets=(0, 8))}, b"\0" * 8, None, "data_offsets span 8"),
    "duplicate key": (b'{"a":{"dtype":"F32","shape":[1],"data_offsets":[0,4]},"a":{"dtype":"F32","shape":[1],"data_offsets":[4,8]}}', b"\0" * 8, None, "duplicate key"),
    "duplicate key through an escape": (b'{"a":{"dtype":"F32","shape":[1],"data_offsets":[0,4]},"\\u0061":{"dtype":"F32","shape":[1],"data_offsets":[4,8]}}', b"\0" * 8, None, "duplicate key"),
    "nested metadata": (b'{"__metadata__":{"a":{"b":"c"}},"a":{"dtype":"F32","shape":[1],"data_offsets":[0,4]}}', b"\0" * 4, None, "nested"),
    "metadata value not a string": (b'{"__metadata__":{"a":1}}', b"", None, "strings"),
    "nested tensor field": (b'{"a":{"dtype":"F32","shape":[[1]],"data_offsets":[0,4]}}', b"\0" * 4, None, "integer"),
    "top level is an array": (b'[{"dtype":"F32","shape":[1],"data_offsets":[0,4]}]', b"\0" * 4, None, "expected '{'"),
    "unknown field": (b'{"a":{"dtype":"F32","shape":[1],"data_offsets":[0,4],"extra":1}}', b"\0" * 4, None, "unexpected"),
    "control character in a key": (b'{"a\nb":{"dtype":"F32","shape":[1],"data_offsets":[0,4]}}', b"\0" * 4, None, "control character"),
    "unknown escape": (b'{"a\\qb":{"dtype":"F32","shape":[1],"data_offsets":[0,4]}}', b"\0" * 4, None, "escape"),
    "lone surrogate": (b'{"a\\ud83db":{"dtype":"F32","shape":[1],"data_offsets":[0,4]}}', b"\0" * 4, None, "surrogate"),
    "unterminated string": (b'{"a":{"dtype":"F32', b"\0" * 4, None, "unterminated"),
    "negative dimension": (b'{"a":{"dtype":"F32","shape":[-1],"data_offsets":[0,4]}}', b"\0" * 4, None, "negative dimension"),
    "negative offset": (b'{"a":{"dtype":"F32","shape":[1],"data_offsets":[-4,4]}}', b"\0" * 4, None, "negative offset"),
    "product overflows": ({"a": _entry(shape=(1 << 40, 1 << 40), offsets=(0, 0))}, b"", None, "overflows"),
    "product times element size overflows": ({"a": _entry(dtype="F64", shape=(1 << 31, 1 << 30), offsets=(0, 0))}, b"", None, "overflows"),
    "dimension overflows int64": (b'{"a":{"dtype":"F32","shape":[99999999999999999999],"data_offsets":[0,4]}}', b"\0" * 4, None, "overflows"),
    "fractional dimension": (b'{"a":{"dtype":"F32","shape":[1.0],"data_offsets":[0,4]}}', b"\0" * 4, None, "not an integer"),
    "unknown dtype": ({"a": _entry(dtype="F128", shape=(1,), offsets=(0, 4))}, b"\0" * 4, None, "unknown dtype"),
    "missing field": (b'{"a":{"dtype":"F32","shape":[1]}}', b"\0" * 4, None, "lacks"),
    "trailing garbage": (b'{"a":{"dtype":"F32","shape":[1],"data_offsets":[0,4]}}x', b"\0" * 4, None, "trailing"),
    "truncated header": (b'{"a":{"dtype":"F32","shape":[1],"data_offsets":[0,', b"", None, "integer"),
    "empty header": (b"", b"", None, "expected '{'"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_files_are_refused(sdmi, tmp_path, case):
    header, data, hlen, words = MALFORMED[case]
    if isinstance(header, dict):
        header = json.dumps(header).encode()
    path = _file(tmp_path / "bad.safetensors", header, data, hlen)
    with pytest.raises(sdmi.SdmiError) as ei:
        sdmi.safetensors_list(path)
    print(f"{case}: status {ei.value.status}: {ei.value}")
    assert ei.value.status == ERR_WEIGHTS and words in str(ei.value) and "bad.safetensors" in str(ei.value)


def test_unreadable_and_short_files(sdmi, tmp_path):
    with pytest.raises(sdmi.SdmiError) as ei:
        sdmi.safetensors_list(tmp_path / "missing.safetensors")
    assert ei.value.status == ERR_IO and "cannot open" in str(ei.value)
    with pytest.raises(sdmi.SdmiError) as ei:
        sdmi.safetensors_list(tmp_path)          # a directory
    assert ei.value.status == ERR_IO
    for n in (0, 7):
        (tmp_path / "short.safetensors").write_bytes(b"\0" * n)
        with pytest.raises(sdmi.SdmiError) as ei:
            sdmi.safetensors_list(tmp_path / "short.safetensors")
        assert ei.value.status == ERR_WEIGHTS and "8-byte" in str(ei.value)
    # well formed: an empty object, padding after it, an empty tensor
    assert sdmi.safetensors_list(_file(tmp_path / "e.safetensors", b"{}   ")) == []
    assert sdmi.safetensors_list(_file(tmp_path / "z.safetensors", b' { "a" : {"shape":[0], "dtype":"F32", "data_offsets":[0,0]} } ')) == [("a", "F32", (0,), 8 + 62, None)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_reader_and_key_rules_under_sanitizers(tmp_path):
    """tests/san/safetensors_main.cpp, a program of its own: the well-formed file, every truncation of its header, byte flips at every header position."""
    from stable_diffusion_burn_amd import weights as W
    W.write_safetensors(tmp_path / "ok.safetensors", _sample_tensors(W), metadata={"format": "pt"})
    exe = tmp_path / "safetensors_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "san" / "safetensors_main.cpp"), str(CSRC / "safetensors_reader.cpp"), str(CSRC / "ckpt_keys.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    r = subprocess.run([str(exe), str(tmp_path / "ok.safetensors"), str(FIXTURE), str(scratch)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("ok: ") and int(last.split()[1]) > 5000, r.stdout


def test_default_schedule_is_the_synthetic_one(sdmi):
    from stable_diffusion_burn_amd import synthetic as syn
    got = sdmi.default_alphas_cumprod(1000)
    want = syn.alphas_cumprod(1000)
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for n in (1, 2, 50):
        assert np.array_equal(sdmi.default_alphas_cumprod(n).view(np.uint32), syn.alphas_cumprod(n).view(np.uint32)), n
    from stable_diffusion_burn_amd._capi import load_library
    assert load_library().sdmi_default_alphas_cumprod(None, 10) == ERR_INVALID


def test_checkpoint_writer_is_the_inverse_of_the_map(sdmi, tmp_path):
    """write_checkpoint_safetensors: checkpoint names, Linear weights back in torch's [out, in], F16 / BF16 rounding, alphas optional."""
    from stable_diffusion_burn_amd import weights as W
    g = np.random.default_rng(5)
    specs = [("alphas_cumprod", (1000,)), ("unet/lin1_time_embed/weight", (6, 10)), ("unet/lin1_time_embed/bias", (10,)),
             ("unet/input_blocks/conv/weight", (5, 4, 3, 3)), ("clip/token_embedding/weight", (9, 4))]
    vals = {n: g.standard_normal(s).astype(np.float32) for n, s in specs}
    for dtype in ("F32", "F16", "BF16"):
        path = tmp_path / f"m_{dtype}.safetensors"
        W.write_checkpoint_safetensors(path, specs, lambda n, s: vals[n], vals["alphas_cumprod"] if dtype != "F16" else None, dtype=dtype)
        raw = path.read_bytes()
        listing = {r[4]: r for r in sdmi.safetensors_list(path)}
        assert set(listing) == {n for n, _ in specs} - ({"alphas_cumprod"} if dtype == "F16" else set())
        key, dt, shape, off, _ = listing["unet/lin1_time_embed/weight"]
        assert (key, dt, shape) == ("model.diffusion_model.time_embed.0.weight", dtype, (10, 6))
        t = np.ascontiguousarray(vals["unet/lin1_time_embed/weight"].T)
        want = t.tobytes() if dtype == "F32" else t.astype(np.float16).tobytes() if dtype == "F16" else W.bf16_bits(t).tobytes()
        assert raw[off:off + len(want)] == want
        assert listing["clip/token_embedding/weight"][2] == (9, 4) and listing["unet/input_blocks/conv/weight"][2] == (5, 4, 3, 3)
        if dtype != "F16":
            assert listing["alphas_cumprod"][1] == "F32"
    # bf16 rounding: to nearest, ties to even
    x = np.array([1.0, 1.00390625, 1.01171875, -0.0, np.inf], np.float32)
    assert [hex(v) for v in W.bf16_bits(x)] == ["0x3f80", "0x3f80", "0x3f82", "0x8000", "0x7f80"]
    assert np.array_equal(W.bf16_to_f32(W.bf16_bits(x))[[0, 3, 4]], x[[0, 3, 4]])
