"""Writes ip_adapter_keys.txt: every key of an IP-Adapter file in h94's ip-adapter_sd15.safetensors layout with the shape the model needs, for the default model
(model_channels 320, ctx_dim 768, D 1024, T 4) and a small one (160, 64, 64, 4).  The layer rule is stated here from diffusers' published processor order
(down blocks, up blocks, mid; cross attentions at the odd indices) and pins sdmi_ip_adapter_key; no real file exists offline to hold it against.

    python tests/golden/gen_ip_adapter_keys.py
"""
from pathlib import Path

# (UNet block, channel multiple) of the 16 cross attentions in the ENGINE's order; the file's index counts input blocks, then output blocks, then the middle block
ENGINE_ORDER = [("input_blocks.1", 1), ("input_blocks.2", 1), ("input_blocks.4", 2), ("input_blocks.5", 2), ("input_blocks.7", 4), ("input_blocks.8", 4),
                ("middle_block", 4)] + [(f"output_blocks.{i}", m) for i, m in zip(range(3, 12), (4, 4, 4, 2, 2, 2, 1, 1, 1))]
FILE_ORDER = [b for b, _ in ENGINE_ORDER if b.startswith("input")] + [b for b, _ in ENGINE_ORDER if b.startswith("output")] + ["middle_block"]


def lines(mc, cd, D, T):
    out = [f"# model_channels={mc} ctx_dim={cd} D={D} T={T}",
           f"image_proj.proj.weight\t{T * cd},{D}", f"image_proj.proj.bias\t{T * cd}", f"image_proj.norm.weight\t{cd}", f"image_proj.norm.bias\t{cd}"]
    for i, (block, mult) in enumerate(ENGINE_ORDER):
        j = 2 * FILE_ORDER.index(block) + 1
        for which in ("k", "v"):
            out.append(f"{i}\t{block}\tip_adapter.{j}.to_{which}_ip.weight\t{mult * mc},{cd}")
    return out


if __name__ == "__main__":
    text = "\n".join(lines(320, 768, 1024, 4) + lines(160, 64, 64, 4)) + "\n"
    (Path(__file__).with_name("ip_adapter_keys.txt")).write_text(text)
