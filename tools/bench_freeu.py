"""A/B of FreeU (sd.set_freeu) on a whole sample_latent: off -- the launches of before, which is the yardstick -- against version 1 and
version 2 (the paper's SD 1.4 values, every step).

    python tools/bench_freeu.py [--rounds 3] [--out FILE]

SD v1 at a 64 x 64 latent (synthetic weights), 20 steps, CFG 7.5, 77-token contexts: fp32 batch 1 and bf16 batch 16.  One context per precision, the three arms
ALTERNATING round by round in one process; per arm the median and the min .. max of the device time over the rounds (the run-to-run spread), "slower" only where
the arm's fastest round is behind the yardstick's slowest.  Then one profiled call per arm (option profile = 2): the time under the freeu_* tags and its share of
the call's profiled kernel time.
"""
import argparse
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from stable_diffusion_burn_amd import ModelConfig, StableDiffusion, synthetic as syn  # noqa: E402

STEPS = 20
PARAMS = dict(b1=1.2, b2=1.4, s1=0.9, s2=0.2)


def _set(sd, version):
    if version:
        sd.set_freeu(version=version, **PARAMS)
    else:
        sd.set_freeu(None)


def _tags(sd, path):
    """{tag: (ms, launches)} of the profiled samples since the last reset"""
    sd.set_option("dump_profile_tags", str(path))
    out = {}
    for ln in Path(path).read_text().splitlines():
        nums, tag = ln.split("\t", 1)
        ms, launches = nums.split()[:2]
        out[tag] = (float(ms), int(launches))
    return out


def model_ab(out, rounds):
    synth = syn.SyntheticWeights(cache=True)
    tmp = Path(tempfile.mkdtemp()) / "tags.txt"
    out(f"# SD v1 (synthetic weights), 64 x 64 latent, {STEPS} steps, CFG 7.5, 77-token contexts, FreeU {PARAMS} on every step; device ms per sample_latent call: "
        f"median [min .. max] over {rounds} alternating rounds; no threshold attaches")
    for precision, batch in ((0, 1), (1, 16)):
        cfg = ModelConfig(precision=precision)
        sd = StableDiffusion(cfg)
        sd.load_weights(synth, clip=False, vae_encoder=False)
        ctx = np.stack([syn.cond_context(i, 77, cfg.ctx_dim) for i in range(batch)])
        unc = syn.uncond_context(77, cfg.ctx_dim)
        lat = np.stack([syn.initial_latent(i, 64, 64) for i in range(batch)])
        arms = (0, 1, 2)
        times, kernels = {a: [] for a in arms}, {}
        for r in range(rounds + 1):                     # round 0 warms up
            for v in (arms if r % 2 == 0 else arms[::-1]):
                _set(sd, v)
                sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=lat)
                st = sd.last_call_stats()
                kernels[v] = st["kernels"]
                if r:
                    times[v].append(st["gpu_ms"])
        med = {a: statistics.median(t) for a, t in times.items()}
        out(f"precision {precision} batch {batch}:")
        for v in arms:
            verdict = "" if not v else (" slower" if min(times[v]) > max(times[0]) else " faster" if max(times[v]) < min(times[0]) else " inside the spread")
            out(f"  {'off' if not v else f'version {v}':9s} {med[v]:9.2f} [{min(times[v]):9.2f} .. {max(times[v]):9.2f}] ms per call, {med[v] / batch:8.2f} ms per image, "
                f"{kernels[v]} launches" + (f" | / off = {med[v] / med[0]:.4f}{verdict}, {(med[v] - med[0]) / batch:+.3f} ms per image" if v else ""))
        for v in (1, 2):                                # one profiled call per arm: where the added time goes
            _set(sd, v)
            sd.set_option("profile", 2)
            sd.set_option("profile_reset", 1)
            sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=lat)
            tags = _tags(sd, tmp)
            total = sum(p["ms"] for p in sd.profile_stats().values())
            sd.set_option("profile", 0)
            fu = {t: v_ for t, v_ in tags.items() if t.startswith("freeu_")}
            ms = sum(m for m, _ in fu.values())
            out(f"  version {v} profiled: freeu_* {ms:.3f} ms in {sum(n for _, n in fu.values())} launches = {100 * ms / total:.2f} % of {total:.1f} ms of kernels (" +
                ", ".join(f"{t} {m:.3f} ms / {n}" for t, (m, n) in sorted(fu.items())) + ")")
        sd.set_freeu(None)
        sd.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            Path(a.out).write_text("\n".join(lines) + "\n")
    model_ab(out, a.rounds)


if __name__ == "__main__":
    main()
