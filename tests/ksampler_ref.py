"""CPU restatement of the sigma-schedule samplers (include/sdmi.h "sigma-schedule samplers") in TEXTBOOK form: k-diffusion's
get_sigmas_karras / _exponential / get_sigmas, sigma_to_t, and sample_euler(_ancestral) / dpmpp_2m / heun / dpm_2 / dpmpp_2s_ancestral / dpmpp_sde (r = 1/2, two
increments of one Brownian path for its noise) / dpmpp_2m_sde (midpoint), all in k-space -- x_k = x sqrt(1 + sigma^2), D = x_k - sigma e -- and independent of
the linear table sdmi_ksampler_plan returns.  Scalars are Python floats (f64); x, e and z may be floats, numpy arrays or torch tensors (the oracle's dtype
is kept).  Plus the loop the kernel executes on that table, and the numpy restatement of the step-noise streams."""
import math

import numpy as np

from img2img_ref import normal_stream

KINDS = ("euler", "dpmpp_2m", "heun", "dpm2", "dpmpp_2s", "dpmpp_sde", "dpmpp_2m_sde")
SCHEDULES = ("model", "karras", "exponential", "uniform")
ETA_KINDS = ("euler", "dpmpp_2s", "dpmpp_sde", "dpmpp_2m_sde")
TWO_STAGE = ("heun", "dpm2", "dpmpp_2s", "dpmpp_sde")
M64 = (1 << 64) - 1


# ---- schedules ---------------------------------------------------------------------------------------------------------------
def model_sigmas(alphas) -> np.ndarray:
    a = np.asarray(alphas, np.float32).astype(np.float64)
    return np.sqrt((1.0 - a) / a)


def sigma_to_t(alphas, sigma: float) -> float:
    """k-diffusion's DiscreteSchedule.sigma_to_t (quantize=False)"""
    ls = np.log(model_sigmas(alphas))
    dists = math.log(sigma) - ls
    low = int(min(max(np.cumsum(dists >= 0).argmax(), 0), len(ls) - 2))
    w = (ls[low] - math.log(sigma)) / (ls[low] - ls[low + 1])
    return low + min(max(w, 0.0), 1.0)


def sigmas(schedule, alphas, n, rho=7.0, sigma_min=None, sigma_max=None):
    """the steps + 1 sigmas of n steps, the last 0"""
    S = model_sigmas(alphas)
    total = len(S)
    smin, smax = sigma_min or S[0], sigma_max or S[-1]
    if schedule == "model":
        out = [S[t] for t in range(total - 1, -1, -(total // n))]
    elif schedule == "karras":
        ramp = np.linspace(0.0, 1.0, n) if n > 1 else np.zeros(1)
        out = (smax ** (1 / rho) + ramp * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
    elif schedule == "exponential":
        out = np.exp(np.linspace(math.log(smax), math.log(smin), n)) if n > 1 else [smax]
    elif schedule == "uniform":
        t = np.linspace(total - 1, 0, n) if n > 1 else np.array([total - 1.0])
        lo = np.minimum(np.floor(t).astype(int), total - 2)
        w = t - lo
        out = np.exp((1 - w) * np.log(S[lo]) + w * np.log(S[lo + 1]))
    else:
        raise ValueError(schedule)
    return [float(v) for v in out] + [0.0]


def tail(sg, strength):
    """index of the first step an img2img call at `strength` runs: the last k = min(L, int(strength L)) of the L steps"""
    L = len(sg) - 1
    return L - min(L, int(strength * L))


# ---- step noise --------------------------------------------------------------------------------------------------------------
def noise_key(noise_seed: int, image_base: int, b: int, s: int, r: int = 0) -> int:
    """stream of draw r of image b at step s of the FULL schedule; uint64 wraparound"""
    return (noise_seed + image_base + b + ((s + 1) << 32) + (r << 62)) & M64


def step_noise(noise_seed: int, image_base: int, n: int, s: int, r: int, h: int, w: int) -> np.ndarray:
    return np.stack([normal_stream(noise_key(noise_seed, image_base, b, s, r), 4 * h * w).reshape(4, h, w) for b in range(n)])


# ---- the samplers, k-space -----------------------------------------------------------------------------------------------------
def anc(s, s2, eta):
    """get_ancestral_step -> (down, up)"""
    up = min(s2, eta * math.sqrt(s2 ** 2 * (s ** 2 - s2 ** 2) / s ** 2))
    return math.sqrt(s2 ** 2 - up ** 2), up


def _c(s):
    return 1.0 / math.sqrt(1.0 + s * s)


def sample_textbook(kind, eta, alphas, sg, first, x, predict, noise=None, blend=None):
    """Run `kind` over the steps first .. len(sg) - 2 of the schedule sg from the VP latent x at sg[first].  predict(x_vp, t, sigma) -> the CFG-combined e;
    noise(s, r) -> draw r of full-schedule step s (called only where its weight is not 0); blend(x_vp, a_end) -> the VP latent after the img2img mask blend,
    applied at the end of a step (history keeps the pre-blend quantities)."""
    def model(xk, s):                       # e at (x_k, sigma)
        return predict(xk * _c(s), sigma_to_t(alphas, s), s)

    xk = x / _c(sg[first])
    d_last, h_last = None, None
    for i in range(first, len(sg) - 1):
        s, s2 = sg[i], sg[i + 1]
        e1 = model(xk, s)
        D1 = xk - s * e1
        if s2 == 0.0:
            nx = D1
            if kind in ("dpmpp_2m", "dpmpp_2m_sde"):
                d_last = D1
        elif kind == "euler":
            dn, up = anc(s, s2, eta)
            nx = xk + e1 * (dn - s)
            if up != 0.0:
                nx = nx + up * noise(i, 0)
        elif kind == "dpmpp_2m":
            h = math.log(s) - math.log(s2)
            if d_last is None:
                dd = D1
            else:
                r = h_last / h
                dd = (1.0 + 1.0 / (2.0 * r)) * D1 - (1.0 / (2.0 * r)) * d_last
            nx = (s2 / s) * xk - math.expm1(-h) * dd
            d_last, h_last = D1, h
        elif kind == "heun":
            x2 = xk + e1 * (s2 - s)
            e2 = model(x2, s2)
            nx = xk + (e1 + e2) / 2.0 * (s2 - s)
        elif kind == "dpm2":
            sm = math.exp((math.log(s) + math.log(s2)) / 2.0)
            x2 = xk + e1 * (sm - s)
            e2 = model(x2, sm)
            nx = xk + e2 * (s2 - s)
        elif kind == "dpmpp_2s":
            dn, up = anc(s, s2, eta)
            t, tn = -math.log(s), -math.log(dn)
            sm = math.exp(-(t + 0.5 * (tn - t)))
            x2 = (sm / s) * xk - math.expm1(-0.5 * (tn - t)) * D1
            D2 = x2 - sm * model(x2, sm)
            nx = (dn / s) * xk - math.expm1(-(tn - t)) * D2
            if up != 0.0:
                nx = nx + up * noise(i, 0)
        elif kind == "dpmpp_sde":
            sm = math.exp((math.log(s) + math.log(s2)) / 2.0)          # r = 1/2
            d1, u1 = anc(s, sm, eta)
            x2 = (d1 / s) * xk - math.expm1(-(math.log(s) - math.log(d1))) * D1
            za = noise(i, 0) if u1 != 0.0 else None
            if za is not None:
                x2 = x2 + u1 * za
            D2 = x2 - sm * model(x2, sm)
            d2, u2 = anc(s, s2, eta)
            nx = (d2 / s) * xk - math.expm1(-(math.log(s) - math.log(d2))) * D2       # fac = 1 / (2 r) = 1: denoised_d = D2
            if u2 != 0.0:
                # W(s) - W(s') = (W(s) - W(s_m)) + (W(s_m) - W(s')): increments of variance s - s_m and s_m - s', the first one the draw stage 1 used
                al, be = math.sqrt((s - sm) / (s - s2)), math.sqrt((sm - s2) / (s - s2))
                nx = nx + u2 * (al * za + be * noise(i, 1))
        elif kind == "dpmpp_2m_sde":
            h = math.log(s) - math.log(s2)
            g = eta * h
            nx = (s2 / s) * math.exp(-g) * xk - math.expm1(-h - g) * D1
            if d_last is not None:
                r = h_last / h
                nx = nx + 0.5 * (-math.expm1(-h - g)) * (1.0 / r) * (D1 - d_last)      # midpoint
            if eta != 0.0:
                nx = nx + s2 * math.sqrt(-math.expm1(-2.0 * g)) * noise(i, 0)
            d_last, h_last = D1, h
        else:
            raise ValueError(kind)
        xk = nx
        if blend is not None:
            a_end = 1.0 / (1.0 + s2 * s2)
            xk = blend(xk * _c(s2), a_end) / _c(s2)
    return xk * _c(sg[-1])


def sample_plan(rows, x, predict, noise=None, blend=None):
    """The loop the kernel executes, on the table of sdmi_ksampler_plan [evaluations, 12] = step, stage, t, sigma, cx, ce, h1, cz, cz2, qx, qe, a_end"""
    q_last = None
    for step, stage, t, sigma, cx, ce, h1, cz, cz2, qx, qe, a_end in np.asarray(rows, np.float64).tolist():
        e = predict(x, t, sigma)
        q = qx * x + qe * e
        nx = cx * x + ce * e
        if q_last is not None:
            nx = nx + h1 * q_last
        else:
            assert h1 == 0.0, "a row reads history the call does not have"
        if cz != 0.0:
            nx = nx + cz * noise(int(step), 0)
        if cz2 != 0.0:
            nx = nx + cz2 * noise(int(step), 1)
        x, q_last = nx, q
        if blend is not None and a_end >= 0.0:
            x = blend(x, a_end)
    return x


def gain(rows) -> float:
    """sampler_ref.gain's rule on a plan of dpmpp_2m: the largest per-step 1-norm of the weights on the current and the earlier D, normalised by their sum"""
    g = 1.0
    for step, stage, t, sigma, cx, ce, h1, cz, cz2, qx, qe, a_end in np.asarray(rows, np.float64).tolist():
        w = [ce / qe, h1]
        g = max(g, sum(abs(v) for v in w) / abs(sum(w)))
    return g


# ---- the oracle's sampler driven in textbook form (GPU parity tests) -----------------------------------------------------------
def sample_latent(ora, context, uncond, scale, sg, first, x_start, kind, eta=0.0, noise_seed=0, image_base=0, mask=None, z0=None, eps=None, paired=False):
    """x_start [n,4,h,w] = the VP latent at sg[first] (txt2img: x_T; img2img: the re-noised z0); step noise from the numpy streams; mask blend toward
    sqrt(a_end) z0 + sqrt(1 - a_end) eps at the end of every step.  paired (the contexts have one length): both CFG halves in ONE oracle forward of 2n samples
    -- the UNet is per sample, so the same e, for half the passes over the weights."""
    import torch
    dt = ora.dtype
    x = torch.as_tensor(x_start).to(dt)
    context, uncond = torch.as_tensor(context).to(dt), torch.as_tensor(uncond).to(dt)
    n, _, h, w = x.shape
    predict = lambda x_, t, sigma: ora.forward_diffuser(x_, t, context, uncond, scale)                      # noqa: E731
    if paired:
        both = torch.cat([uncond.unsqueeze(0).repeat(n, 1, 1), context])

        def predict(x_, t, sigma):
            out = ora.unet.forward(torch.cat([x_, x_]), t, both)
            return out[:n] + (out[n:] - out[:n]) * scale
    noise = lambda s, r: torch.from_numpy(step_noise(noise_seed, image_base, n, s, r, h, w)).to(dt)       # noqa: E731
    blend = None
    if mask is not None:
        m = torch.as_tensor(mask).to(dt).reshape(n, 1, h, w)
        z0_, eps_ = torch.as_tensor(z0).to(dt), torch.as_tensor(eps).to(dt)
        blend = lambda x_, a: m * x_ + (1.0 - m) * (math.sqrt(a) * z0_ + math.sqrt(1.0 - a) * eps_)       # noqa: E731
    with torch.no_grad():
        return sample_textbook(kind, eta, ora.alphas, sg, first, x, predict, noise, blend)
