"""A/B of option attn_d64 on the attention shapes of an SD 2.x UNet at a 64 x 64 latent: head dim 64 on k_attn_split.hip (fp32) /
k_attn_bf16.hip (bf16), option 1, against the route it replaces, k_attn.hip, option 0 -- the yardstick, never the new kernel's own earlier run.

    python tools/bench_attention_d64.py [--rounds 7] [--out FILE]          the operator A/B (sd.bench_attention: HIP events around `iters` launches)
    python tools/bench_attention_d64.py --model [--out FILE]               + one whole-model figure: a 20-step sd_v2 sample_latent, fp32 batch 1 and bf16 batch 16

One process per precision's context, the two arms ALTERNATING round by round on the same buffers; per arm the median and the min .. max over the rounds (the
run-to-run spread), and "faster" only where the new arm's slowest round beats the old arm's fastest.  A merge launch behind key slices is inside the timed window.
The last column is what attn_d64 = 2, the default of an SD 2.x context, sends the shape to (csrc/attn_plan.cpp: d64_stays_on_flash); --grid adds the wider fp32
grid that rule was read from.
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from stable_diffusion_burn_amd import ModelConfig, StableDiffusion  # noqa: E402

LEVELS = [(4096, 5), (1024, 10), (256, 20), (64, 20)]      # (tokens, heads of 64) of model_channels = 320 at a 64 x 64 latent
KERNEL = {"flash": "k_attn.hip", "split": "k_attn_split.hip", "bf16": "k_attn_bf16.hip"}


def _iters(flops):
    """enough launches for a window of a few tens of milliseconds at ~ 100 TFLOP/s, at least 50"""
    return int(min(2000, max(50, 3e12 / max(flops, 1.0))))


def operator_ab(out, rounds):
    for precision, n in ((0, 2), (1, 16)):
        sd = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=precision))
        out(f"# precision {precision} ({'fp32' if precision == 0 else 'bf16'}), n = {n}, d = 64; us per call: median [min .. max] over {rounds} alternating rounds")
        for nq, heads in LEVELS:
            for nk in (nq, 77):
                flops = 4.0 * n * heads * nq * nk * 64
                iters = _iters(flops)
                shape = (n, nq, nk, 64 * heads, heads)
                times, plans = {0: [], 1: []}, {}
                for arm in (0, 1):                      # warm both arms' code objects and buffers
                    sd.set_option("attn_d64", arm)
                    plans[arm] = sd.attention_plan(n, heads, nq, nk, 64)
                    sd.bench_attention(*shape, iters=3)
                for r in range(rounds):
                    for arm in ((0, 1) if r % 2 == 0 else (1, 0)):
                        sd.set_option("attn_d64", arm)
                        times[arm].append(sd.bench_attention(*shape, iters=iters) * 1e3)
                med = {a: statistics.median(t) for a, t in times.items()}
                verdict = "faster" if max(times[1]) < min(times[0]) else "slower" if min(times[1]) > max(times[0]) else "inside the spread"
                desc = {a: f"{KERNEL[p['kernel']]} {p['waves']}w" + (f" /{p['kv_splits']}" if p["kv_splits"] > 1 else "") for a, p in plans.items()}
                sd.set_option("attn_d64", 2)
                two = KERNEL[sd.attention_plan(n, heads, nq, nk, 64)["kernel"]]
                out(f"n{n} nq{nq} nk{nk} h{heads}: 0 = {desc[0]:24s} {med[0]:8.1f} [{min(times[0]):8.1f} .. {max(times[0]):8.1f}] {flops / med[0] / 1e6:6.1f} TF | "
                    f"1 = {desc[1]:26s} {med[1]:8.1f} [{min(times[1]):8.1f} .. {max(times[1]):8.1f}] {flops / med[1] / 1e6:6.1f} TF | 0 / 1 = {med[0] / med[1]:.3f} {verdict} | 2 -> {two}")
        sd.close()


def grid_ab(out, rounds=5):
    """fp32 only: the shapes around the UNet's, to see WHERE k_attn_split.hip loses (wf / ws: 64- / 128-row workgroups of the two kernels before key slices)"""
    sd = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=0))
    out(f"# fp32 grid, d = 64; us per call, median of {rounds} alternating rounds: F<waves>/<slices> k_attn.hip (0), S<waves>/<slices> k_attn_split.hip (1)")
    for n in (1, 2, 4, 8):
        for h in (2, 5, 10, 20):
            for nq in (64, 100, 128, 256, 512, 1024, 2048):
                for nk in (77, nq):
                    if n * h * nq > 2 * 20 * 2048:
                        continue
                    shape = (n, nq, nk, 64 * h, h)
                    iters = int(min(1000, max(50, 2e12 / (4.0 * n * h * nq * nk * 64))))
                    t, plan = {0: [], 1: []}, {}
                    for arm in (0, 1):
                        sd.set_option("attn_d64", arm)
                        plan[arm] = sd.attention_plan(n, h, nq, nk, 64)
                        sd.bench_attention(*shape, iters=3)
                    for r in range(rounds):
                        for arm in ((0, 1) if r % 2 == 0 else (1, 0)):
                            sd.set_option("attn_d64", arm)
                            t[arm].append(sd.bench_attention(*shape, iters=iters) * 1e3)
                    m = {a: statistics.median(v) for a, v in t.items()}
                    sd.set_option("attn_d64", 2)
                    two = sd.attention_plan(n, h, nq, nk, 64)["kernel"]
                    out(f"n{n} h{h} q{nq} k{nk} wf{-(-nq // 64) * n * h} ws{-(-nq // 128) * n * h} F{plan[0]['waves']}/{plan[0]['kv_splits']} {m[0]:.1f} "
                        f"S{plan[1]['waves']}/{plan[1]['kv_splits']} {m[1]:.1f} ratio {m[0] / m[1]:.3f} | 2 -> {'S' if two == 'split' else 'F'}")
    sd.close()


def model_ab(out, rounds=3):
    from stable_diffusion_burn_amd import synthetic as syn
    synth = syn.SyntheticWeights(cache=True)
    out("# whole model: sd_v2 (synthetic weights), 64 x 64 latent, 20 steps, CFG 7.5, 77-token contexts; device ms per sample_latent call: median [min .. max]; no threshold attaches")
    for precision, batch in ((0, 1), (1, 16)):
        cfg = ModelConfig.sd_v2(precision=precision, clip=False)
        ctx = np.stack([syn.cond_context(i, 77, cfg.ctx_dim) for i in range(batch)])
        unc = syn.uncond_context(77, cfg.ctx_dim)
        lat = np.stack([syn.initial_latent(i, 64, 64) for i in range(batch)])
        # at precision >= 1 the option decides how the query weights are packed: one context per arm there (2 is 1 at bf16), one context with a switch at precision 0
        arms = {}
        levels = (0, 1, 2) if precision == 0 else (0, 1)
        for arm in levels:
            if precision == 0 and arms:
                arms[arm] = arms[0]
                continue
            sd = StableDiffusion(cfg)
            sd.set_option("attn_d64", arm)
            sd.load_weights(synth, clip=False, vae_encoder=False)
            arms[arm] = sd
        times, kernels = {a: [] for a in levels}, {}
        for r in range(rounds + 1):                     # round 0 warms up
            for arm in (levels if r % 2 == 0 else levels[::-1]):
                sd = arms[arm]
                if precision == 0:
                    sd.set_option("attn_d64", arm)
                sd.sample_latent(ctx, unc, 7.5, 20, init_latent=lat)
                st = sd.last_call_stats()
                kernels[arm] = st["kernels"]
                if r:
                    times[arm].append(st["gpu_ms"])
        med = {a: statistics.median(t) for a, t in times.items()}
        out(f"precision {precision} batch {batch}: " + " | ".join(f"attn_d64={a} {med[a]:9.1f} [{min(times[a]):9.1f} .. {max(times[a]):9.1f}] ms, {kernels[a]} launches" for a in levels) +
            " | " + ", ".join(f"0 / {a} = {med[0] / med[a]:.3f}" for a in levels[1:]))
        for sd in {id(s): s for s in arms.values()}.values():
            sd.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            Path(a.out).write_text("\n".join(lines) + "\n")
    operator_ab(out, a.rounds)
    if a.grid:
        grid_ab(out)
    if a.model:
        model_ab(out)


if __name__ == "__main__":
    main()
