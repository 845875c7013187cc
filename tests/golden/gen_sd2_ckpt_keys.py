"""Write tests/golden/sd2_ckpt_keys.txt: the checkpoint key of every tensor of an SD 2.x model (ModelConfig.sd_v2) in Stability's layout.

    python tests/golden/gen_sd2_ckpt_keys.py

UNPINNED.  The reference has no SD 2 side, so unlike sd14_ckpt_keys.txt this list is not taken from a model object: it is WRITTEN DOWN BY RULE from the
public format, independently of csrc/ckpt_keys.cpp (this script never loads the library):

  * UNet and VAE: the rows of sd14_ckpt_keys.txt -- the module tree of SD 2.x's UNet and VAE is SD v1's -- with two changes of SHAPE: the transformers'
    proj_in / proj_out are nn.Linear, [C, C] instead of [C, C, 1, 1], and attn2's to_k / to_v read the 1024-wide OpenCLIP context;
  * text encoder: open_clip's text transformer under "cond_stage_model.model." -- token_embedding.weight [49408, 1024], positional_embedding [77, 1024]
    (a bare parameter: no ".weight"), ln_final, and per block transformer.resblocks.<i>.{ln_1, ln_2, attn.in_proj_weight [3072, 1024], attn.in_proj_bias
    [3072], attn.out_proj, mlp.c_fc [4096, 1024], mlp.c_proj}.  nn.MultiheadAttention fuses the three projections: rows 0..1023 are the query's, 1024..2047
    the key's, 2048..3071 the value's.  Blocks 0..22: SD 2.x conditions on the penultimate block's output, resblocks.23 is never run.

One line per tensor:   dump name <TAB> checkpoint key <TAB> checkpoint shape d0,d1,.. <TAB> T|- <TAB> -|0|1|2
T: the dump holds the transpose of the checkpoint tensor (Linear weights); the last column: the third of the key's rows the tensor is (fused in_proj), - = all.
tests/test_sd2_cpu.py checks csrc/ckpt_keys.cpp against it: a guard against drift, no proof of the layout.
"""
from pathlib import Path

HERE = Path(__file__).resolve().parent
WIDTH, LAYERS, VOCAB, CTX = 1024, 23, 49408, 77


def rows():
    out = []
    for ln in (HERE / "sd14_ckpt_keys.txt").read_text().splitlines():
        dump, key, shape, flag = ln.split("\t")
        if dump.startswith("clip/"):
            continue
        dims = [int(v) for v in shape.split(",")]
        if dump.startswith("unet/") and dump.endswith(("/transformer/proj_in/weight", "/transformer/proj_out/weight")):
            assert dims[2:] == [1, 1] and flag == "-"
            dims = dims[:2]
        if dump.startswith("unet/") and dump.endswith(("/attn2/key/weight", "/attn2/value/weight")):
            assert dims[1] == 768 and flag == "T"
            dims[1] = WIDTH
        out.append((dump, key, dims, flag, "-"))
    te = "cond_stage_model.model."
    out.append(("clip/token_embedding/weight", te + "token_embedding.weight", [VOCAB, WIDTH], "-", "-"))
    out.append(("clip/position_embedding/weight", te + "positional_embedding", [CTX, WIDTH], "-", "-"))
    for leaf in ("weight", "bias"):
        out.append((f"clip/layer_norm/{leaf}", te + f"ln_final.{leaf}", [WIDTH], "-", "-"))
    for i in range(LAYERS):
        d, k = f"clip/blocks/{i}/", te + f"transformer.resblocks.{i}."
        for leaf in ("weight", "bias"):
            out.append((d + f"attn_ln/{leaf}", k + f"ln_1.{leaf}", [WIDTH], "-", "-"))
            out.append((d + f"mlp_ln/{leaf}", k + f"ln_2.{leaf}", [WIDTH], "-", "-"))
        for part, name in enumerate(("query", "key", "value")):
            out.append((d + f"attn/{name}/weight", k + "attn.in_proj_weight", [3 * WIDTH, WIDTH], "T", str(part)))
            out.append((d + f"attn/{name}/bias", k + "attn.in_proj_bias", [3 * WIDTH], "-", str(part)))
        for dump_mod, mod, cout, cin in (("attn/out", "attn.out_proj", WIDTH, WIDTH), ("mlp/fc1", "mlp.c_fc", 4 * WIDTH, WIDTH), ("mlp/fc2", "mlp.c_proj", WIDTH, 4 * WIDTH)):
            out.append((d + dump_mod + "/weight", k + mod + ".weight", [cout, cin], "T", "-"))
            out.append((d + dump_mod + "/bias", k + mod + ".bias", [cout], "-", "-"))
    return sorted(out)


if __name__ == "__main__":
    text = "".join("\t".join((d, k, ",".join(str(v) for v in s), f, p)) + "\n" for d, k, s, f, p in rows())
    (HERE / "sd2_ckpt_keys.txt").write_text(text)
    print(f"wrote {len(text.splitlines())} lines, {len(text)} bytes")
