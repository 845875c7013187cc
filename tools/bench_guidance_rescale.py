"""A/B of CFG rescale (sd.set_guidance_rescale) on a whole sample_latent: phi = 0.7 -- every update on sampler_step_rescale_kernel, one workgroup
per image -- against phi = 0, the launches of before, which is the yardstick.

    python tools/bench_guidance_rescale.py [--rounds 3] [--out FILE]

SD v1 at a 64 x 64 latent (synthetic weights), 20 steps, CFG 7.5, 77-token contexts: fp32 batch 1 and bf16 batch 16.  One context per precision, the two arms
ALTERNATING round by round in one process; per arm the median and the min .. max of the device time over the rounds (the run-to-run spread), "slower" only where the
new arm's fastest round is behind the old arm's slowest.  The last columns: the "other" profile class (which holds the update launch) of one profiled call per arm,
and from it the time of one update launch more than the elementwise one it replaces.
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from stable_diffusion_burn_amd import ModelConfig, StableDiffusion, synthetic as syn  # noqa: E402

STEPS = 20
PHI = 0.7


def model_ab(out, rounds):
    synth = syn.SyntheticWeights(cache=True)
    out(f"# SD v1 (synthetic weights), 64 x 64 latent, {STEPS} steps, CFG 7.5, 77-token contexts; device ms per sample_latent call: median [min .. max] over {rounds} "
        "alternating rounds; no threshold attaches")
    for precision, batch in ((0, 1), (1, 16)):
        cfg = ModelConfig(precision=precision)
        sd = StableDiffusion(cfg)
        sd.load_weights(synth, clip=False, vae_encoder=False)
        ctx = np.stack([syn.cond_context(i, 77, cfg.ctx_dim) for i in range(batch)])
        unc = syn.uncond_context(77, cfg.ctx_dim)
        lat = np.stack([syn.initial_latent(i, 64, 64) for i in range(batch)])
        arms = (0.0, PHI)
        times, kernels, other = {a: [] for a in arms}, {}, {}
        for r in range(rounds + 1):                     # round 0 warms up
            for phi in (arms if r % 2 == 0 else arms[::-1]):
                sd.set_guidance_rescale(phi)
                sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=lat)
                st = sd.last_call_stats()
                kernels[phi] = st["kernels"]
                if r:
                    times[phi].append(st["gpu_ms"])
        for phi in arms:                                # one profiled call per arm: the class of the update launch
            sd.set_guidance_rescale(phi)
            sd.set_option("profile", 1)
            sd.set_option("profile_reset", 1)
            sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=lat)
            other[phi] = sd.profile_stats()["other"]
            sd.set_option("profile", 0)
        med = {a: statistics.median(t) for a, t in times.items()}
        verdict = "slower" if min(times[PHI]) > max(times[0.0]) else "faster" if max(times[PHI]) < min(times[0.0]) else "inside the spread"
        per_launch = (other[PHI]["ms"] - other[0.0]["ms"]) / STEPS * 1e3
        out(f"precision {precision} batch {batch}: " +
            " | ".join(f"phi={a} {med[a]:9.2f} [{min(times[a]):9.2f} .. {max(times[a]):9.2f}] ms, {kernels[a]} launches" for a in arms) +
            f" | phi / 0 = {med[PHI] / med[0.0]:.4f} {verdict} | class other: {other[0.0]['ms']:.3f} -> {other[PHI]['ms']:.3f} ms in {other[PHI]['launches']} launches, "
            f"{per_launch:+.1f} us per update launch")
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
