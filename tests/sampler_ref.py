"""CPU restatement of the sampler choice (include/sdmi.h "sampler choice") in TEXTBOOK form, independent of the
linear form sdmi_sampler_coefs returns: Song et al.'s DDIM with sigma, k-diffusion's sample_euler_ancestral and sample_dpmpp_2m in
sigma_k = sqrt((1 - a) / a) space, and PLMS as Adams-Bashforth on e from the coefficient table.  Scalars are Python floats (f64); x, e and
z may be floats, numpy arrays or torch tensors (the oracle's dtype is kept).  Plus the numpy restatement of the step-noise stream."""
import math

import numpy as np

from img2img_ref import normal_stream

KINDS = ("ddim", "dpmpp_2m", "plms", "euler_ancestral")   # the last: a restatement only -- the library runs it as "ddim" at eta = 1
AB = ((1.0,), (3.0 / 2, -1.0 / 2), (23.0 / 12, -16.0 / 12, 5.0 / 12), (55.0 / 24, -59.0 / 24, 37.0 / 24, -9.0 / 24))
M64 = (1 << 64) - 1


def schedule(alphas, ts, step):
    """[(t, cur, prev)] of a run over ts: cur = a[t], prev = a[t - step] or 1 past the end (sample_latent's rule)"""
    return [(t, float(alphas[t]), float(alphas[t - step]) if t >= step else 1.0) for t in ts]


def noise_key(noise_seed: int, image_base: int, b: int, s: int) -> int:
    """stream of image b (of a call whose first image has global index image_base) at index s of the FULL schedule; uint64 wraparound"""
    return (noise_seed + image_base + b + ((s + 1) << 32)) & M64


def step_noise(noise_seed: int, image_base: int, n: int, s: int, h: int, w: int) -> np.ndarray:
    """z [n,4,h,w] of schedule index s: element i (NCHW order) of image b = element i of stream noise_key(.., b, s)"""
    return np.stack([normal_stream(noise_key(noise_seed, image_base, b, s), 4 * h * w).reshape(4, h, w) for b in range(n)])


def _x0(x, e, cur):
    return (x - math.sqrt(1.0 - cur) * e) / math.sqrt(cur)


def ddim_step(x, e, cur, prev, eta, z):
    """Song et al. (DDIM, eq. 12 and 16)"""
    sigma = eta * math.sqrt((1.0 - prev) / (1.0 - cur)) * math.sqrt(1.0 - cur / prev)
    x = math.sqrt(prev) * _x0(x, e, cur) + math.sqrt(1.0 - prev - sigma * sigma) * e
    return x + sigma * z if sigma != 0.0 else x


def euler_ancestral_step(x, e, cur, prev, z):
    """k-diffusion sample_euler_ancestral (eta = 1) on x_k = x / sqrt(a), sigma_k = sqrt((1 - a) / a)"""
    sig, sig_n = math.sqrt((1.0 - cur) / cur), math.sqrt((1.0 - prev) / prev)
    xk, den = x / math.sqrt(cur), _x0(x, e, cur)
    up = min(sig_n, math.sqrt(sig_n ** 2 * (sig ** 2 - sig_n ** 2) / sig ** 2))      # get_ancestral_step
    down = math.sqrt(sig_n ** 2 - up ** 2)
    d = (xk - den) / sig                                                             # to_d
    xk = xk + d * (down - sig)
    if sig_n > 0.0:
        xk = xk + z * up
    return xk * math.sqrt(prev)


def dpmpp_2m_step(x, e, cur, prev, cur_last, den_last):
    """k-diffusion sample_dpmpp_2m on x_k = x / sqrt(a): t = -log sigma_k.  Returns (x', denoised)"""
    sig, sig_n = math.sqrt((1.0 - cur) / cur), math.sqrt((1.0 - prev) / prev)
    xk, den = x / math.sqrt(cur), _x0(x, e, cur)
    if sig_n == 0.0:                       # h = inf: sigma_next / sigma = 0, -expm1(-h) = 1
        return den * math.sqrt(prev), den
    t, t_n = -math.log(sig), -math.log(sig_n)
    h = t_n - t
    if den_last is None:
        xk = (sig_n / sig) * xk - math.expm1(-h) * den
    else:
        h_last = t - (-math.log(math.sqrt((1.0 - cur_last) / cur_last)))
        r = h_last / h
        den_d = (1.0 + 1.0 / (2.0 * r)) * den - (1.0 / (2.0 * r)) * den_last
        xk = (sig_n / sig) * xk - math.expm1(-h) * den_d
    return xk * math.sqrt(prev), den


def plms_step(x, e, cur, prev, e_hist):
    """Adams-Bashforth of order min(4, 1 + len(e_hist)) on e, then the eta = 0 DDIM update with e' (one UNet evaluation per step)"""
    w = AB[min(3, len(e_hist))]
    ep = w[0] * e
    for k in range(1, len(w)):
        ep = ep + w[k] * e_hist[k - 1]
    return ddim_step(x, ep, cur, prev, 0.0, None)


def sample_textbook(kind, eta, alphas, ts, step, x, predict, noise=None, blend=None):
    """Run `kind` over ts from x.  predict(x, t, cur) -> the CFG-combined e; noise(s) -> z of full-schedule index s (called only where the
    step has noise: eta > 0 and prev < 1); blend(x, prev) -> x after the img2img mask blend (history keeps the pre-blend quantities)."""
    total = len(alphas)
    cur_last, den_last, e_hist = None, None, []
    for t, cur, prev in schedule(alphas, ts, step):
        e = predict(x, t, cur)
        s = (total - 1 - t) // step
        if kind == "ddim":
            z = noise(s) if (eta != 0.0 and prev < 1.0) else None
            x = ddim_step(x, e, cur, prev, eta, z)
        elif kind == "euler_ancestral":
            x = euler_ancestral_step(x, e, cur, prev, noise(s) if prev < 1.0 else None)
        elif kind == "dpmpp_2m":
            x, den_last = dpmpp_2m_step(x, e, cur, prev, cur_last, den_last)
            cur_last = cur
        elif kind == "plms":
            x = plms_step(x, e, cur, prev, e_hist)
            e_hist = [e] + e_hist[:2]
        else:
            raise ValueError(kind)
        if blend is not None:
            x = blend(x, prev)
    return x


def sample_linear(coefs, alphas, ts, step, x, predict, noise=None, blend=None):
    """The loop the kernel executes, on the table of sdmi_sampler_coefs [len(ts), 8] = cx, ce, h1, h2, h3, cz, qx, qe"""
    total = len(alphas)
    hist = []
    for (t, cur, prev), (cx, ce, h1, h2, h3, cz, qx, qe) in zip(schedule(alphas, ts, step), np.asarray(coefs, np.float64).tolist()):
        e = predict(x, t, cur)
        q = qx * x + qe * e
        nx = cx * x + ce * e
        for hk, qk in zip((h1, h2, h3), hist):
            nx = nx + hk * qk
        if cz != 0.0:
            nx = nx + cz * noise((total - 1 - t) // step)
        x = nx
        hist = [q] + hist[:2]
        if blend is not None:
            x = blend(x, prev)
    return x


def gain(kind, coefs) -> float:
    """The largest per-step 1-norm of the weights a sampler puts on UNet outputs, normalised by their sum: 1 for DDIM, 1 + 1/r for
    DPM-Solver++(2M) (weights 1 + 1/(2r), -1/(2r) on x0, x0_last), 160/24 for PLMS -- the worst-case gain of the extrapolation on its
    inputs' rounding error."""
    if kind == "ddim":
        return 1.0
    g = 1.0
    for cx, ce, h1, h2, h3, cz, qx, qe in np.asarray(coefs, np.float64).tolist():
        w = [ce / qe, h1, h2, h3]          # weights on the current and the earlier q (q = x0: ce = B w0 qe; q = e: qe = 1)
        g = max(g, sum(abs(v) for v in w) / abs(sum(w)))
    return g


# ---- the oracle's sampler driven in textbook form (GPU parity tests) ---------------------------------------------------
def sample_latent(ora, context, uncond, scale, ts, step, x_start, kind, eta=0.0, noise_seed=0, image_base=0, mask=None, z0=None, eps=None):
    """x_start [n,4,h,w] = the latent at ts[0] (txt2img: x_T; img2img: the re-noised z0); step noise from the numpy stream; mask blend toward
    sqrt(a_prev) z0 + sqrt(1 - a_prev) eps after every update, as img2img_ref.sample_latent_from."""
    import torch
    dt = ora.dtype
    x = torch.as_tensor(x_start).to(dt)
    context, uncond = torch.as_tensor(context).to(dt), torch.as_tensor(uncond).to(dt)
    n, _, h, w = x.shape
    predict = lambda x_, t, cur: ora.forward_diffuser(x_, t, context, uncond, scale)                       # noqa: E731
    noise = lambda s: torch.from_numpy(step_noise(noise_seed, image_base, n, s, h, w)).to(dt)            # noqa: E731
    blend = None
    if mask is not None:
        m = torch.as_tensor(mask).to(dt).reshape(n, 1, h, w)
        z0_, eps_ = torch.as_tensor(z0).to(dt), torch.as_tensor(eps).to(dt)
        blend = lambda x_, prev: m * x_ + (1.0 - m) * (math.sqrt(prev) * z0_ + math.sqrt(1.0 - prev) * eps_)   # noqa: E731
    with torch.no_grad():
        return sample_textbook(kind, eta, ora.alphas, ts, step, x, predict, noise, blend)
