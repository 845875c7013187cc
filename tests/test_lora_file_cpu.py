"""kohya-ss / LyCORIS LoRA files, the host side (include/sdmi.h "LoRA adapters"; DESIGN.md section 9c "files"): the module-name map against an independent Python
restatement (tests/lora_file_ref.py) and the pinned table tests/golden/kohya_lora_keys.txt; every refusal of the loader that needs no device, through the host-only
sdmi_lora_check_safetensors; the same code under AddressSanitizer / UBSan in a stand-alone driver (tests/san/lora_keys_main.cpp, its own process, nothing
preloaded); and the resource figures of the merge kernel's F32 instance, which must stay the parent commit's.  No device is needed."""
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lora_file_ref as R
import lora_ref as L

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "stable_diffusion_burn_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden"
ERR_INVALID, ERR_WEIGHTS, ERR_UNSUPPORTED = -1, -3, -5

Q = "unet/input_blocks/rt1/transformer/transformer/attn1/query/weight"
CONV = "unet/input_blocks/rt1/res/conv_in/weight"
CONV_IN = "unet/input_blocks/conv/weight"
FC1 = "clip/blocks/0/mlp/fc1/weight"
# a small host entry list: a Linear, a 3x3 conv, a 9-channel (padded) conv_in, one text-encoder layer -- "clip_layers = 1"
SPECS = [(Q, (16, 16)), (CONV, (16, 16, 3, 3)), (CONV_IN, (16, 9, 3, 3)), (FC1, (8, 32)), ("unet/norm_out/weight", (16,)), ("clip/token_embedding/weight", (48, 8))]


@pytest.fixture(scope="module")
def sdmi():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)
    import stable_diffusion_burn_amd as S
    return S


def _table():
    return [ln.split("\t") for ln in (GOLDEN / "kohya_lora_keys.txt").read_text().splitlines()]


def test_name_table(sdmi):
    """lora_module_name over every conv / Linear entry of the full-size SD v1 spec == the Python restatement == the pinned table; the anchors literally; injective;
    names of anything else are refused."""
    targets = R.sd14_targets(GOLDEN / "sd14_ckpt_keys.txt")
    table = {row[0]: (row[1], row[2]) for row in _table()}
    assert len(table) == 354 and sum(n.startswith("clip/") for n in table) == 72        # 16 transformers x 12 + 22 ResBlocks x 3 + 12 shortcuts + 3 + 3 samplers + 4; 12 x 6
    seen = {}
    for name, key, _ in targets:
        ref = R.module_names(key)
        if ref is None:
            assert name not in table and name.split("/")[0] in ("autoencoder",), name
            with pytest.raises(sdmi.SdmiError) as ei:
                sdmi.lora_module_name(name)
            assert ei.value.status == ERR_INVALID
            continue
        got = sdmi.lora_module_name(name)
        assert got == ref[0] == table[name][0], name
        assert ref[1] == table[name][1]
        assert sdmi.checkpoint_key(name)[0] == key
        seen.setdefault(got, name)
        assert seen[got] == name, f"{got} names {seen[got]} and {name}"
    assert len(seen) == len(table)                                                         # injective, and the table has nothing else
    by_module = {v[0]: k for k, v in table.items()}
    for module, key in R.ANCHORS.items():
        assert sdmi.checkpoint_key(by_module[module])[0] == key + ".weight", module
    for bad in ("unet/norm_out/weight", "unet/conv_out/bias", "clip/token_embedding/weight", "clip/position_embedding/weight", "clip/layer_norm/weight",
                "unet/input_blocks/rt1/transformer/norm/weight", "controlnet/input_blocks/rt1/res/conv_in/weight", "alphas_cumprod", "", "unet/nope/weight"):
        with pytest.raises(sdmi.SdmiError) as ei:
            sdmi.lora_module_name(bad)
        assert ei.value.status == ERR_INVALID, bad


def _lora_item(shape, rank, seed=0):
    return L.make_adapter({"x": (shape, rank)}, seed)["x"]


def test_both_spellings_resolve_at_tiny_dims_and_one_clip_layer(sdmi, tmp_path):
    """A file in the kohya spelling and one in the CompVis-style spelling name the same entries of a small model with one text-encoder layer; a module of a layer the
    model lacks is unknown: refused, or skipped and counted."""
    from stable_diffusion_burn_amd import weights as W
    ad = {Q: _lora_item((16, 16), 3), CONV: _lora_item((16, 16, 3, 3), 4), FC1: _lora_item((8, 32), 2)}
    for style in ("kohya", "compvis"):
        W.write_lora_safetensors(tmp_path / f"{style}.safetensors", ad, dtype="F16", style=style)
        assert sdmi.lora_check_safetensors(tmp_path / f"{style}.safetensors", SPECS) == (3, 0)
        assert sdmi.lora_check_safetensors(tmp_path / f"{style}.safetensors", SPECS, which=sdmi.LORA_UNET) == (2, 0)
        assert sdmi.lora_check_safetensors(tmp_path / f"{style}.safetensors", SPECS, which=sdmi.LORA_TE) == (1, 0)
    keys = {k for k, *_ in sdmi.safetensors_list(tmp_path / "kohya.safetensors")}
    assert "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q.lora_down.weight" in keys and "lora_te_text_model_encoder_layers_0_mlp_fc1.alpha" in keys
    keys = {k for k, *_ in sdmi.safetensors_list(tmp_path / "compvis.safetensors")}
    assert "lora_unet_input_blocks_1_1_transformer_blocks_0_attn1_to_q.lora_up.weight" in keys and "lora_unet_input_blocks_1_0_in_layers_2.lora_down.weight" in keys
    # a second text-encoder layer: not in this model
    ad2 = dict(ad)
    ad2["clip/blocks/1/mlp/fc1/weight"] = _lora_item((8, 32), 2)
    W.write_lora_safetensors(tmp_path / "two.safetensors", ad2, dtype="BF16")
    with pytest.raises(sdmi.SdmiError) as ei:
        sdmi.lora_check_safetensors(tmp_path / "two.safetensors", SPECS)
    assert ei.value.status == ERR_UNSUPPORTED and "lora_te_text_model_encoder_layers_1_mlp_fc1" in str(ei.value)
    assert sdmi.lora_check_safetensors(tmp_path / "two.safetensors", SPECS, skip_unknown=True) == (3, 1)
    assert sdmi.lora_check_safetensors(tmp_path / "two.safetensors", SPECS, which=sdmi.LORA_UNET) == (2, 0)          # the other half is passed over, not judged


def _kohya(sdmi, name):
    return sdmi.lora_module_name(name)


def test_refusals_that_need_no_device(sdmi, tmp_path):
    """Every unsupported key kind (SDMI_ERR_UNSUPPORTED, the key named), shape mismatches (SDMI_ERR_WEIGHTS, the key named), a rank of 257, a padded conv_in, an
    unknown module with and without the skip flag, bad arguments, a truncated file."""
    from stable_diffusion_burn_amd import weights as W
    q = _kohya(sdmi, Q)
    down, up, alpha = _lora_item((16, 16), 4)
    good = {q + ".lora_down.weight": down.astype(np.float16), q + ".lora_up.weight": up.astype(np.float16), q + ".alpha": np.float16(alpha)}

    def check(tensors, **kw):
        W.write_safetensors(tmp_path / "f.safetensors", tensors)
        return sdmi.lora_check_safetensors(tmp_path / "f.safetensors", SPECS, **kw)

    def refused(tensors, status, needle, **kw):
        with pytest.raises(sdmi.SdmiError) as ei:
            check(tensors, **kw)
        assert ei.value.status == status and needle in str(ei.value), str(ei.value)

    assert check(good) == (1, 0)
    assert check({k: v for k, v in good.items() if not k.endswith("alpha")}) == (1, 0)                      # no alpha: alpha = rank
    z = np.zeros((4, 4), np.float16)
    for kind in ("lora_mid.weight", "hada_t1", "hada_t2", "lokr_w1", "lokr_w2", "lokr_w1_a", "lokr_t2", "dora_scale", "diff", "diff_b", "lora_A.weight", "weight"):
        refused({**good, f"{q}.{kind}": z}, ERR_UNSUPPORTED, f"{q}.{kind}")
        refused({**good, f"{q}.{kind}": z}, ERR_UNSUPPORTED, f"{q}.{kind}", skip_unknown=True)                 # the skip flag is for modules, not for key kinds
        refused({**good, f"lora_te_text_model_encoder_layers_0_mlp_fc1.{kind}": z}, ERR_UNSUPPORTED, kind, which=sdmi.LORA_UNET)   # ... whichever half holds it
    refused({**good, "no_module_at_all": z}, ERR_UNSUPPORTED, "no_module_at_all")
    # shapes, against the entry's dims
    refused({**good, q + ".lora_down.weight": np.zeros((4, 15), np.float16)}, ERR_WEIGHTS, q + ".lora_down.weight")
    refused({**good, q + ".lora_up.weight": np.zeros((16, 5), np.float16)}, ERR_WEIGHTS, q + ".lora_up.weight")
    refused({**good, q + ".lora_up.weight": np.zeros((15, 4), np.float16)}, ERR_WEIGHTS, q + ".lora_up.weight")
    refused({k: v for k, v in good.items() if "lora_up" not in k}, ERR_WEIGHTS, q + ".lora_up.weight")
    refused({**good, q + ".alpha": np.zeros(2, np.float16)}, ERR_WEIGHTS, q + ".alpha")
    refused({**good, q + ".alpha": np.float32("nan")}, ERR_WEIGHTS, q + ".alpha")
    c = _kohya(sdmi, CONV)
    conv = {c + ".lora_down.weight": np.zeros((3, 16, 3, 3), np.float32), c + ".lora_up.weight": np.zeros((16, 3, 1, 1), np.float32)}
    assert check(conv) == (1, 0)
    assert check({c + ".lora_down.weight": np.zeros((3, 144), np.float32), c + ".lora_up.weight": np.zeros((16, 3), np.float32)}) == (1, 0)
    refused({**conv, c + ".lora_down.weight": np.zeros((3, 16, 1, 1), np.float32)}, ERR_WEIGHTS, c + ".lora_down.weight")
    refused({**conv, c + ".lora_up.weight": np.zeros((16, 3, 3, 3), np.float32)}, ERR_WEIGHTS, c + ".lora_up.weight")
    # the shape error in the LAST module of a file is found before anything would be uploaded: the whole file is refused
    refused({**good, **conv, c + ".lora_up.weight": np.zeros((16, 2, 1, 1), np.float32)}, ERR_WEIGHTS, c + ".lora_up.weight")
    # LoHa
    a, b = np.zeros((16, 2), np.float16), np.zeros((2, 144), np.float16)
    loha = {c + ".hada_w1_a": a, c + ".hada_w1_b": b, c + ".hada_w2_a": a, c + ".hada_w2_b": b.reshape(2, 16, 3, 3), c + ".alpha": np.float32(1.0)}
    assert check(loha) == (1, 0)
    refused({k: v for k, v in loha.items() if "w2_b" not in k}, ERR_WEIGHTS, c + ".hada_w2_b")
    refused({**loha, c + ".hada_w2_a": np.zeros((16, 3), np.float16)}, ERR_WEIGHTS, c + ".hada_w2_a")
    refused({**loha, c + ".hada_w1_b": np.zeros((2, 143), np.float16)}, ERR_WEIGHTS, c + ".hada_w1_b")
    # dtypes, rank, the padded conv_in
    refused({q + ".lora_down.weight": down.astype(np.float64), q + ".lora_up.weight": up.astype(np.float64)}, ERR_UNSUPPORTED, "F64")
    assert check({q + ".lora_down.weight": np.zeros((256, 16), np.float16), q + ".lora_up.weight": np.zeros((16, 256), np.float16)}) == (1, 0)
    refused({q + ".lora_down.weight": np.zeros((257, 16), np.float16), q + ".lora_up.weight": np.zeros((16, 257), np.float16)}, ERR_UNSUPPORTED, "257")
    ci = _kohya(sdmi, CONV_IN)
    assert ci == "lora_unet_conv_in"
    pad = {ci + ".lora_down.weight": np.zeros((2, 9, 3, 3), np.float16), ci + ".lora_up.weight": np.zeros((16, 2, 1, 1), np.float16)}
    refused(pad, ERR_UNSUPPORTED, "conv_in")
    refused(pad, ERR_UNSUPPORTED, "conv_in", skip_unknown=True)
    # unknown modules: an SDXL text encoder, a transformer depth SD v1 does not have
    for module in ("lora_te1_text_model_encoder_layers_0_mlp_fc1", "lora_unet_down_blocks_0_attentions_0_transformer_blocks_1_attn1_to_q", "lora_unet_input_blocks_1_1_nope"):
        extra = {module + ".lora_down.weight": z, module + ".lora_up.weight": z}
        refused({**good, **extra}, ERR_UNSUPPORTED, module)
        assert check({**good, **extra}, skip_unknown=True) == (1, 1)
    # arguments
    refused(good, ERR_INVALID, "which", which=0)
    refused(good, ERR_INVALID, "which", which=4)
    # a truncated file: the reader's refusal, as for a checkpoint
    W.write_safetensors(tmp_path / "whole.safetensors", good)
    data = (tmp_path / "whole.safetensors").read_bytes()
    for cut in (len(data) - 1, len(data) - 70, 12, 7):
        (tmp_path / "cut.safetensors").write_bytes(data[:cut])
        with pytest.raises(sdmi.SdmiError) as ei:
            sdmi.lora_check_safetensors(tmp_path / "cut.safetensors", SPECS)
        assert ei.value.status == ERR_WEIGHTS, cut
    with pytest.raises(sdmi.SdmiError) as ei:
        sdmi.lora_check_safetensors(tmp_path / "absent.safetensors", SPECS)
    assert ei.value.status == -4


def test_writer_round_trip(sdmi, tmp_path):
    """write_lora_safetensors: the keys, shapes and dtypes kohya-ss writes (a scalar alpha, a conv's 4-D factors, 2-D LoHa factors), an alpha left out on request."""
    from stable_diffusion_burn_amd import weights as W
    ad = {Q: _lora_item((16, 16), 3), CONV: _lora_item((16, 16, 3, 3), 4)[:2] + (None,)}
    ad.update(R.make_loha({FC1: ((8, 32), 2)}, 5))
    for dtype in ("F32", "F16", "BF16"):
        W.write_lora_safetensors(tmp_path / "a.safetensors", ad, dtype=dtype)
        listing = {k: (dt, shape) for k, dt, shape, *_ in sdmi.safetensors_list(tmp_path / "a.safetensors")}
        c, q, f = (_kohya(sdmi, n) for n in (CONV, Q, FC1))
        assert listing[c + ".lora_down.weight"] == (dtype, (4, 16, 3, 3)) and listing[c + ".lora_up.weight"] == (dtype, (16, 4, 1, 1)) and c + ".alpha" not in listing
        assert listing[q + ".lora_down.weight"] == (dtype, (3, 16)) and listing[q + ".lora_up.weight"] == (dtype, (16, 3)) and listing[q + ".alpha"] == (dtype, ())
        assert listing[f + ".hada_w1_a"] == (dtype, (32, 2)) and listing[f + ".hada_w2_b"] == (dtype, (2, 8))
        assert sdmi.lora_check_safetensors(tmp_path / "a.safetensors", SPECS) == (3, 0)
    with pytest.raises(ValueError):
        W.write_lora_safetensors(tmp_path / "a.safetensors", ad, dtype="F64")
    with pytest.raises(sdmi.SdmiError):
        W.write_lora_safetensors(tmp_path / "a.safetensors", {"unet/norm_out/weight": ad[Q]})


def test_loha_bound_is_a_bound_for_an_fp32_emulation():
    """The derived LoHa bound against a numpy emulation of the kernel's order of operations in float32 (products and sums rounded separately, which is never more
    accurate than the FMA chain by more than the bound's own slack): a sanity check of the derivation, not a measurement of the device."""
    shape, rank = (24, 20), 33
    item = R.make_loha({"x": (shape, rank)}, 3)["x"]
    g = np.random.default_rng(1)
    w0 = (g.uniform(-1, 1, shape) / np.sqrt(shape[0])).astype(np.float32)
    c = L.coef(0.7, item[4], rank)
    d = []
    for a, b in ((item[0], item[1]), (item[2], item[3])):
        acc = np.zeros(shape, np.float32)
        for j in range(rank):
            acc = (acc.astype(np.float64) + np.outer(b[j].astype(np.float64), a[:, j].astype(np.float64))).astype(np.float32)   # one rounding per step, like an FMA
        d.append(acc)
    h = d[0] * d[1]
    w = (w0.astype(np.float64) + float(c) * h.astype(np.float64)).astype(np.float32)
    terms = [R.loha_terms(item, 0.7)]
    err = np.abs(w.astype(np.float64) - R.merge_f64(w0, terms))
    bound = R.merge_bound(w0, terms)
    assert (err <= bound).all() and err.max() > 0
    assert (bound <= (2 * rank + 4) * R.U * (np.abs(w0) + abs(float(c)) * R.loha_delta_f64(shape, *(np.abs(f) for f in item[:4])))).all()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_name_map_and_plan_under_sanitizers(tmp_path):
    """tests/san/lora_keys_main.cpp, a program of its own: the pinned table forwards and backwards, malformed module and dump names, fabricated tensor lists."""
    exe = tmp_path / "lora_keys_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "san" / "lora_keys_main.cpp"), str(CSRC / "lora_keys.cpp"), str(CSRC / "ckpt_keys.cpp"), str(CSRC / "safetensors_reader.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(GOLDEN / "kohya_lora_keys.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    m = re.fullmatch(r"(\d+) checks, 0 failed", r.stdout.strip())
    assert m and int(m.group(1)) > 40000, r.stdout


LLVM = Path("/opt/rocm/lib/llvm/bin")
PARENT_F32 = {"vgpr_count": 118, "group_segment_fixed_size": 10560, "private_segment_fixed_size": 0, "vgpr_spill_count": 0, "sgpr_spill_count": 0}


def test_f32_instance_of_the_merge_kernel_keeps_its_resources(sdmi, tmp_path):
    """The F32, non-LoHa instance of the merge -- sdmi::lora_merge_kernel(LoraMerge), what every sdmi_lora_add launch runs -- still exists in the gfx950 code object under
    its own name, and its kernel-descriptor figures are the parent commit's: there it had .vgpr_count 118, .group_segment_fixed_size 10560 (LDS bytes), no scratch and
    no spills (.sgpr_count 54, .kernarg_segment_size 480; the by-value argument has since grown to 928 bytes, which moves scalar registers only).  Read from the code
    object's metadata note (the object test_code_objects_cpu.py unbundles), not from instruction text.  The five instances a file brings (16-bit factors, LoHa) are
    lora_factor_merge_kernel<DT, HADA>: no scratch, twice the LDS for LoHa."""
    obj = ROOT / "stable_diffusion_burn_amd" / "build" / "k_lora.hip.o"
    from stable_diffusion_burn_amd import build
    build.OBJDIR.mkdir(exist_ok=True)
    assert build._compile("k_lora.hip") == obj and obj.exists()                    # the object of the library the sdmi fixture built; compiled here only if it is absent or stale
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("needs ROCm's llvm tools")
    fat, dev = tmp_path / "k_lora.fat", tmp_path / "k_lora.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(obj), str(tmp_path / "k_lora.copy.o")], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={dev}"], check=True)
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(dev)], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s+- \.", notes):                       # one YAML list item per kernel under amdhsa.kernels
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "merge_kernel" not in name.group(1):
            continue
        kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    print(json.dumps(kernels, indent=1))
    f32 = kernels["_ZN4sdmi17lora_merge_kernelENS_9LoraMergeE"]                                                        # the parent's symbol
    assert {k: f32[k] for k in PARENT_F32} == PARENT_F32
    inst = {(int(m.group(1)), int(m.group(2))): v for k, v in kernels.items() for m in [re.search(r"lora_factor_merge_kernelILi(\d)ELb([01])EEE", k)] if m}
    assert sorted(inst) == [(0, 1), (1, 0), (1, 1), (2, 0), (2, 1)] and len(kernels) == 6, sorted(kernels)
    for (dt, hada), fig in inst.items():
        assert fig["private_segment_fixed_size"] == 0 and fig["vgpr_spill_count"] == 0 and fig["sgpr_spill_count"] == 0, (dt, hada)
        assert fig["group_segment_fixed_size"] == (21120 if hada else 10560), (dt, hada)                              # LoHa stages two factor pairs
        assert fig["kernarg_segment_size"] <= 4096
