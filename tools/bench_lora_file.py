#!/usr/bin/env python3
"""Attach time of a full-size kohya-ss LoRA file next to the route the .npz-only interface offered for the same factors, in one process:

    python tools/bench_lora_file.py --out lora_file_attach.txt [--dir /dev/shm] [--rank 32] [--precision 0]

A rank-`--rank` F16 adapter over every transformer target of the SD v1 UNet (proj_in / proj_out, the attention projections, the feed-forward layers: 192) and every
Linear layer of the text encoder (72) is written with weights.write_lora_safetensors -- nothing is downloaded; the base weights are random numbers (timing only).

  * file route: StableDiffusion.lora_load_safetensors -- upload of the raw factors (attach at scale 0) and the merge + re-pack (set_scale), median of --repeat;
  * Python route: read the file, widen every factor to fp32 and rename it to its dump-tree path on the host, then StableDiffusion.lora_attach;
  * device bytes held by the factors on either route;
  * GPU time of the merge launches by tag (F16 file against an F32 file of the same factors; HIP events, engine option profile=2).

Measured, not asserted: DESIGN.md section 9c quotes the figures.
"""
from __future__ import annotations

import argparse
import json
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="lora_file_attach.txt")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--precision", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion, lora_module_name, synthetic as syn, weights as W

    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    sd = StableDiffusion(ModelConfig.sd_v1_4(precision=args.precision, clip=True))
    sd.set_option("keep_masters", 1)
    specs = sd.weight_specs()
    groups = sd.GROUP_HOT | sd.GROUP_CLIP
    g = np.random.default_rng(0)
    t0 = time.perf_counter()
    n = int(sd._lib.sdmi_packed_size(sd._ctx, groups))
    flat = g.standard_normal(n, dtype=np.float32)
    flat *= 0.02
    off = 0
    for name, shape in specs:
        if not (sd._group_of(name) & groups):
            continue
        cnt = int(np.prod(shape))
        if name == "alphas_cumprod":
            flat[off:off + cnt] = syn.alphas_cumprod(shape[0])
        off += cnt
    sd.load_weights_packed(flat, groups=groups)
    del flat
    say(f"# SD v1 UNet + text encoder, precision {args.precision}, keep_masters: {n / 1e6:.0f} M parameters loaded in {time.perf_counter() - t0:.1f} s")

    r = args.rank
    targets = {}
    for name, shape in specs:
        if not name.endswith("/weight") or len(shape) not in (2, 4):
            continue
        if "/transformer/" in name and name.startswith("unet/") and "norm" not in name or (name.startswith("clip/blocks/") and "_ln" not in name):
            try:
                lora_module_name(name)
            except Exception:
                continue
            targets[name] = tuple(shape)
    ad = {}
    for name, shape in targets.items():
        n_in = shape[0] if len(shape) == 2 else shape[1] * shape[2] * shape[3]
        n_out = shape[1] if len(shape) == 2 else shape[0]
        down = (0.02 * g.standard_normal((r, n_in) if len(shape) == 2 else (r,) + shape[1:])).astype(np.float32)
        up = (0.02 * g.standard_normal((n_out, r))).astype(np.float32)
        ad[name] = (down, up, r / 2.0)
    tmp = Path(tempfile.mkdtemp(prefix="sdmi_lora_", dir=args.dir))
    try:
        f16, f32 = tmp / "lora_f16.safetensors", tmp / "lora_f32.safetensors"
        W.write_lora_safetensors(f16, ad, dtype="F16")
        W.write_lora_safetensors(f32, ad, dtype="F32")
        n_unet = sum(k.startswith("unet/") for k in ad)
        say(f"# rank {r}: {n_unet} UNet + {len(ad) - n_unet} text-encoder targets; {f16.name} {f16.stat().st_size / 1e6:.1f} MB, {f32.name} {f32.stat().st_size / 1e6:.1f} MB")
        module_to_dump = {lora_module_name(k): k for k in ad}

        def file_route(path):
            t0 = time.perf_counter()
            a = sd.lora_load_safetensors(path, scale=0.0)
            t1 = time.perf_counter()
            a.set_scale(1.0)
            t2 = time.perf_counter()
            nbytes = a.factor_bytes
            a.detach()
            return t1 - t0, t2 - t1, nbytes

        def python_route(path):
            t0 = time.perf_counter()
            data = Path(path).read_bytes()
            hn = int.from_bytes(data[:8], "little")
            header = json.loads(data[8:8 + hn])
            parts = {}
            for key, info in header.items():
                if key == "__metadata__":
                    continue
                b, e = info["data_offsets"]
                arr = np.frombuffer(data, np.float16 if info["dtype"] == "F16" else np.float32, count=(e - b) // (2 if info["dtype"] == "F16" else 4), offset=8 + hn + b)
                module, _, kind = key.partition(".")
                parts.setdefault(module_to_dump[module], {})[kind] = arr.reshape(info["shape"]).astype(np.float32)
            tensors = {}
            for name, p in parts.items():
                up = p["lora_up.weight"]
                tensors[name] = (p["lora_down.weight"], up.reshape(up.shape[0], up.shape[1]), float(p["alpha"]))
            t1 = time.perf_counter()
            a = sd.lora_attach(tensors, scale=0.0)
            t2 = time.perf_counter()
            a.set_scale(1.0)
            t3 = time.perf_counter()
            a.detach()
            return t1 - t0, t2 - t1, t3 - t2, sum(d.nbytes + u.nbytes for d, u, _ in tensors.values())

        file_route(f16), python_route(f16)          # first touch: page cache, pool
        fr = [file_route(f16) for _ in range(args.repeat)]
        pr = [python_route(f16) for _ in range(args.repeat)]
        med = lambda rows, i: statistics.median(x[i] for x in rows)   # noqa: E731
        say(f"# wall time, median of {args.repeat} (after one warm-up run of each)")
        say(f"file route   (lora_load_safetensors, F16): upload {med(fr, 0):.3f} s + merge and re-pack {med(fr, 1):.3f} s = {med(fr, 0) + med(fr, 1):.3f} s; "
            f"factors on the device {fr[0][2] / 1e6:.1f} MB")
        say(f"python route (read + widen + rename, lora_attach): host {med(pr, 0):.3f} s + upload {med(pr, 1):.3f} s + merge and re-pack {med(pr, 2):.3f} s = "
            f"{med(pr, 0) + med(pr, 1) + med(pr, 2):.3f} s; factors on the device {pr[0][3] / 1e6:.1f} MB")

        # the merge launches themselves, by tag
        rows = {}
        for label, path in (("F16", f16), ("F32", f32)):
            a = sd.lora_load_safetensors(path, scale=0.0)
            a.set_scale(0.5)                            # warm
            sd.set_option("profile_reset", 1)
            sd.set_option("profile", 2)
            for s in (1.0, 0.75, 1.25):
                a.set_scale(s)
            sd.set_option("profile", 0)
            raw = tmp / f"tags_{label}.raw"
            sd.set_option("dump_profile_tags", str(raw))
            a.detach()
            for line in raw.read_text().splitlines():
                nums, tag = line.split("\t", 1)
                ms, nl, _, by = nums.split()
                if tag.startswith("lora_merge"):
                    shape = tag.split()[2] if "loha" not in tag else tag.split()[3]
                    rows.setdefault(shape, {})[label] = (float(ms), int(nl), float(by))
        say("# merge launches by master shape [R x Cc] (3 re-merges each): launches, us / launch F16 factors, us / launch F32 factors, F16 / F32, GB/s of master bytes (F16)")
        tot = {"F16": 0.0, "F32": 0.0}
        for shape, v in sorted(rows.items(), key=lambda kv: -kv[1].get("F16", (0, 0, 0))[0]):
            if "F16" in v and "F32" in v:
                (m16, n16, b16), (m32, n32, _) = v["F16"], v["F32"]
                tot["F16"] += m16
                tot["F32"] += m32
                say(f"{shape:>12s} {n16:5d} {1e3 * m16 / n16:9.1f} {1e3 * m32 / n32:9.1f} {m16 / n16 / (m32 / n32):6.2f} {b16 / max(m16, 1e-9) / 1e6:9.0f}")
        say(f"# all merge launches of one re-merge: F16 factors {tot['F16'] / 3:.3f} ms, F32 factors {tot['F32'] / 3:.3f} ms")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        sd.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
