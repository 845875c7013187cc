#!/usr/bin/env python3
"""Load time of a full-size SD v1.4 fp16 .safetensors checkpoint (synthetic weights, ~2.1 GB) next to the other loaders of the same model, in one process:

    python tools/bench_safetensors_load.py --out safetensors_load.txt [--dir /dev/shm] [--precision 0]

  * wall time of load_weights_safetensors (F16, and F32 for the byte count), load_weights_packed and load_weights_dir: median of --repeat loads;
  * per-class GPU time of the loader's own launches (sdmi_profile_stats; the conversion kernel is class "other") and, per launch tag, the conversion
    kernel's achieved GB/s -- the transposing form on the [10240, 1280] F16 GEGLU projections among them;
  * a device-to-device copy of the same OUTPUT bytes (10240 x 1280 fp32) on the same device, for scale.

The files are written to a temporary directory under --dir and removed.  Measured, not asserted: DESIGN.md section 9e quotes the figures.
"""
from __future__ import annotations

import argparse
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="safetensors_load.txt")
    ap.add_argument("--dir", default=None, help="where the temporary files go (default: the system's temporary directory)")
    ap.add_argument("--precision", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--skip-dir", action="store_true", help="leave out load_weights_dir (4.3 GB of .npy files)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion, synthetic as syn, weights as W

    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    cfg = ModelConfig.sd_v1_4(precision=args.precision, clip=True)
    sd = StableDiffusion(cfg)
    specs = sd.weight_specs()
    shapes = dict(specs)
    provider = syn.SyntheticWeights(cache=True)
    get = lambda n, s: syn.named_tensor(provider, n, s, shapes)   # noqa: E731
    alphas = syn.alphas_cumprod(1000)
    tmp = Path(tempfile.mkdtemp(prefix="sdmi_ckpt_", dir=args.dir))
    try:
        t0 = time.perf_counter()
        flat = sd.pack_weights(provider, groups=7)
        say(f"# SD v1.4 + CLIP + VAE encoder, precision {args.precision}: {len(specs)} tensors, {flat.size / 1e6:.0f} M parameters; synthetic weights generated in {time.perf_counter() - t0:.1f} s")
        files = {}
        for dtype in ("F16", "F32"):
            files[dtype] = tmp / f"sd14_{dtype}.safetensors"
            t0 = time.perf_counter()
            W.write_checkpoint_safetensors(files[dtype], specs, get, alphas, dtype=dtype)
            say(f"# wrote {files[dtype].name}: {files[dtype].stat().st_size / 1e9:.2f} GB in {time.perf_counter() - t0:.1f} s")
        rows = []
        for dtype in ("F16", "F32"):
            sd.load_weights_safetensors(files[dtype])          # first touch: page cache, arenas
            med, ts = timed(lambda: sd.load_weights_safetensors(files[dtype]), args.repeat)
            rows.append((f"load_weights_safetensors {dtype}", med, ts, files[dtype].stat().st_size))
        sd.load_weights_packed(flat, groups=7)
        med, ts = timed(lambda: sd.load_weights_packed(flat, groups=7), args.repeat)
        rows.append(("load_weights_packed (flat fp32 image in memory)", med, ts, flat.nbytes))
        if not args.skip_dir:
            t0 = time.perf_counter()
            W.write_dump_tree(tmp / "dump", specs, get, alphas, n_head=cfg.n_head, clip_heads=cfg.clip_heads)
            nbytes = sum(p.stat().st_size for p in (tmp / "dump").rglob("*.npy"))
            say(f"# wrote the npy dump tree: {nbytes / 1e9:.2f} GB in {time.perf_counter() - t0:.1f} s")
            sd.load_weights_dir(tmp / "dump")
            med, ts = timed(lambda: sd.load_weights_dir(tmp / "dump"), args.repeat)
            rows.append(("load_weights_dir (npy dump tree)", med, ts, nbytes))
        say("# wall time per load (finalize included), median of %d; source bytes; GB/s of source" % args.repeat)
        for name, med, ts, nbytes in rows:
            say(f"{med:8.3f} s  {nbytes / 1e9:6.2f} GB  {nbytes / med / 1e9:6.2f} GB/s  {name}   (runs: {' '.join(f'{t:.3f}' for t in ts)})")

        # the loader's launches by class and by tag
        sd.set_option("profile_reset", 1)
        sd.set_option("profile", 2)
        sd.load_weights_safetensors(files["F16"])
        sd.set_option("profile", 0)
        prof = sd.profile_stats()
        say("# GPU time of one F16 load by kernel class (HIP events; the packing kernels are not profiled launches):")
        for cls, v in prof.items():
            if v["launches"]:
                say(f"{v['ms']:9.3f} ms  {v['launches']:6d} launches  {v['bytes'] / 1e9:7.3f} GB  {v['bytes'] / max(v['ms'], 1e-9) / 1e6:8.1f} GB/s  class {cls}")
        raw = tmp / "tags.raw"
        sd.set_option("dump_profile_tags", str(raw))
        tags = []
        for line in raw.read_text().splitlines():
            nums, tag = line.split("\t", 1)
            ms, n, _, by = nums.split()
            if tag.startswith("unpack"):
                tags.append((float(ms), int(n), float(by), tag))
        tags.sort(key=lambda r: -r[0])
        say("# conversion kernel by tag (dtype, transform 0 copy / 1 transpose / 2 channel pad, d0 x d1): ms total, launches, us/launch, GB/s (bytes read + written)")
        for ms, n, by, tag in tags[:14]:
            say(f"{ms:9.3f} ms {n:5d} {1e3 * ms / n:9.1f} us {by / max(ms, 1e-9) / 1e6:8.1f} GB/s  {tag}")
        geglu = [r for r in tags if r[3] == "unpack F16 t1 10240x1280"]
        torch.cuda.set_device(0)
        a = torch.empty(10240 * 1280, dtype=torch.float32, device="cuda")
        b = torch.empty_like(a)
        b.copy_(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        d2d = e0.elapsed_time(e1) / 20
        say(f"# device-to-device copy of 10240 x 1280 fp32 ({a.numel() * 4 / 1e6:.1f} MB, warm, 20 back to back): {1e3 * d2d:.1f} us = {2 * a.numel() * 4 / d2d / 1e6:.0f} GB/s read + written")
        if geglu:
            ms, n, by, tag = geglu[0]
            say(f"# transposing conversion [10240, 1280] F16 -> fp32 [1280, 10240] inside the load (cold source, {n} launches): {1e3 * ms / n:.1f} us = {by / ms / 1e6:.0f} GB/s read + written")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        sd.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
