"""Pin the kohya-ss LoRA module name of every conv / Linear weight of the UNet and the text encoder of the full-size SD v1 model.

    python tests/golden/gen_kohya_lora_keys.py

Needs nothing but the repository: the entries and their CompVis keys come from tests/golden/sd14_ckpt_keys.txt (pinned against the reference's own Python
side by gen_ckpt_keys.py), the renaming CompVis -> diffusers is the Python restatement of the conversion table in tests/lora_file_ref.py.  Writes
tests/golden/kohya_lora_keys.txt, one line per target:

    dump name <TAB> kohya module name <TAB> CompVis-style module name

tests/test_lora_file_cpu.py checks csrc/lora_keys.cpp against the fixture and against the restatement.
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import lora_file_ref as R  # noqa: E402

OUT = HERE / "kohya_lora_keys.txt"


def main():
    lines = []
    for name, key, _ in R.sd14_targets(HERE / "sd14_ckpt_keys.txt"):
        names = R.module_names(key)
        if names is not None:
            lines.append(f"{name}\t{names[0]}\t{names[1]}")
    OUT.write_text("\n".join(sorted(lines)) + "\n")
    print(f"wrote {OUT}: {len(lines)} targets")


if __name__ == "__main__":
    main()
