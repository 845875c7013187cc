"""A/B of IP-Adapter (sd.set_ip_adapter) on a whole sample_latent: off -- the launches of before, which is the yardstick -- against one
picture (T_ip = 4) and four pictures (T_ip = 16) on every step.

    python tools/bench_ip_adapter.py [--rounds 3] [--out FILE]

SD v1 at a 64 x 64 latent (synthetic weights and a synthetic adapter with the published D = 1024, T = 4), 20 steps, CFG 7.5, 77-token contexts: fp32 batch 1 and
bf16 batch 16.  One context per precision, the three arms ALTERNATING round by round in one process; per arm the median and the min .. max of the device time over the
rounds (the run-to-run spread), "slower" only where the arm's fastest round is behind the yardstick's slowest.  Then one profiled call per arm (option profile = 2):
the time under the ip_attention tags, per launch at the 64 x 64 level against the kernel's traffic roof -- the bytes of q, O_text and O at the rate the
neighbouring elementwise kernel of the same call (the LayerNorm in front of the cross attention, same rows and width) reaches.
"""
import argparse
import re
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from stable_diffusion_burn_amd import ModelConfig, StableDiffusion, synthetic as syn  # noqa: E402

STEPS = 20
D_EMB, T_IMG = 1024, 4
ARMS = (0, 1, 4)       # pictures per image


def _set(sd, n_img):
    if n_img:
        sd.set_ip_adapter(embeds=syn.image_embeds(0, n_img, D_EMB), scale=1.0)
    else:
        sd.set_ip_adapter(None)


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
    out(f"# SD v1 (synthetic weights), 64 x 64 latent, {STEPS} steps, CFG 7.5, 77-token contexts, IP-Adapter (D = {D_EMB}, T = {T_IMG}) at scale 1 on every step; "
        f"device ms per sample_latent call: median [min .. max] over {rounds} alternating rounds; no threshold attaches")
    for precision, batch in ((0, 1), (1, 16)):
        cfg = ModelConfig(precision=precision)
        sd = StableDiffusion(cfg)
        sd.load_weights(synth, clip=False, vae_encoder=False)
        ad = syn.ip_adapter(cfg.model_channels, cfg.ctx_dim, D_EMB, T_IMG)
        layers = syn.ip_adapter_layers(cfg.model_channels)
        sd.set_ip_adapter_weights(ad["image_proj.proj.weight"], ad["image_proj.proj.bias"], ad["image_proj.norm.weight"], ad["image_proj.norm.bias"],
                                  [ad[kk] for kk, _, _ in layers], [ad[kv] for _, kv, _ in layers])
        ctx = np.stack([syn.cond_context(i, 77, cfg.ctx_dim) for i in range(batch)])
        unc = syn.uncond_context(77, cfg.ctx_dim)
        lat = np.stack([syn.initial_latent(i, 64, 64) for i in range(batch)])
        times, kernels = {a: [] for a in ARMS}, {}
        for r in range(rounds + 1):                     # round 0 warms up
            for v in (ARMS if r % 2 == 0 else ARMS[::-1]):
                _set(sd, v)
                sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=lat)
                st = sd.last_call_stats()
                kernels[v] = st["kernels"]
                if r:
                    times[v].append(st["gpu_ms"])
        med = {a: statistics.median(t) for a, t in times.items()}
        out(f"precision {precision} batch {batch}:")
        for v in ARMS:
            verdict = "" if not v else (" slower" if min(times[v]) > max(times[0]) else " faster" if max(times[v]) < min(times[0]) else " inside the spread")
            out(f"  {'off' if not v else f'T_ip = {T_IMG * v}':9s} {med[v]:9.2f} [{min(times[v]):9.2f} .. {max(times[v]):9.2f}] ms per call, {med[v] / batch:8.2f} ms per image, "
                f"{batch * STEPS / med[v] * 1e3 / STEPS:7.3f} images/s, {kernels[v]} launches" +
                (f" | / off = {med[v] / med[0]:.4f}{verdict}, {(med[v] - med[0]) / batch:+.3f} ms per image" if v else ""))
        es = 2 if precision else 4
        for v in ARMS[1:]:                               # one profiled call per arm: where the added time goes
            _set(sd, v)
            sd.set_option("profile", 2)
            sd.set_option("profile_reset", 1)
            sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=lat)
            tags = _tags(sd, tmp)
            total = sum(p["ms"] for p in sd.profile_stats().values())
            sd.set_option("profile", 0)
            ip = {t: v_ for t, v_ in tags.items() if t.startswith("ip_attention")}
            ms = sum(m for m, _ in ip.values())
            out(f"  T_ip = {T_IMG * v} profiled: ip_attention {ms:.3f} ms in {sum(n for _, n in ip.values())} launches = {100 * ms / total:.2f} % of {total:.1f} ms of kernels")
            for t, (m, n) in sorted(ip.items()):
                g = re.match(r"ip_attention n(\d+) nq(\d+) T(\d+) h(\d+) d(\d+)", t)
                nb, nq, _, h, d = (int(x) for x in g.groups())
                # q + O_text + O; at precision 0 the output is three bf16 planes, read and written (6 bytes per element each way)
                nbytes = nb * nq * h * d * (3 * es if precision else 4 + 6 + 6)
                ln = tags.get(f"layer_norm rows{nb * nq} c{h * d}")
                roof = ""
                if ln:
                    rate = 2.0 * nb * nq * h * d * es / (ln[0] / ln[1] * 1e-3)          # bytes / s of the LayerNorm of the same rows (read + write, dense)
                    roof = f", roof at the LayerNorm's {rate / 1e12:.2f} TB/s = {nbytes / rate * 1e6:.2f} us: x{m / n * 1e3 / (nbytes / rate * 1e6):.2f}"
                out(f"    {t}: {m / n * 1e3:.2f} us per launch x {n}, {nbytes / 1e6:.1f} MB{roof}")
        sd.set_ip_adapter(None)
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
