"""CPU restatement of the zero-terminal-SNR pieces (include/sdmi.h "CFG rescale and zero-terminal-SNR schedules"), independent of the
library: Algorithm 1 of Lin et al. ("Common Diffusion Noise Schedules and Sample Steps are Flawed") on sqrt(alphas_cumprod) in numpy f64, and the three samplers of
the sampler choice in the (x0, eps_hat) basis of a v-predicting model -- x0 = sqrt(a) x - sqrt(1 - a) v, eps_hat = sqrt(a) v + sqrt(1 - a) x -- in which nothing
is singular at a = 0.  Scalars are Python floats; x, v and z may be floats, numpy arrays or torch tensors."""
import math

import numpy as np

import sampler_ref as S


def rescale_zero_snr(alphas) -> np.ndarray:
    s = np.sqrt(np.asarray(alphas, np.float32).astype(np.float64))
    s0, sT = s[0], s[-1]
    s = (s - sT) * s0 / (s0 - sT)
    return (s * s).astype(np.float32)


def x0_eps(x, v, a):
    sc, sn = math.sqrt(a), math.sqrt(1.0 - a)
    return sc * x - sn * v, sc * v + sn * x


def _lam(a):
    return -math.inf if a == 0.0 else 0.5 * math.log(a / (1.0 - a))


def sample_x0_eps(kind, eta, alphas, ts, step, x, predict_v, noise=None, blend=None):
    """Run "ddim" (eta) / "dpmpp_2m" / "plms" over ts from x.  predict_v(x, t, cur) -> the guided v; noise(s) and blend(x, prev) as in
    sampler_ref.sample_textbook.  DDIM: Song et al. eq. 12 on (x0, eps_hat).  DPM-Solver++(2M): Lu et al.'s data-prediction update on the VP latent,
    x' = (sigma'/sigma) x - alpha' expm1(-h) D with sigma = sqrt(1 - a), alpha = sqrt(a), lambda = log(alpha / sigma); from a = 0 h is infinite (expm1(-h) = -1)
    and after such a step r = h_last / h is infinite: first order.  PLMS: Adams-Bashforth on eps_hat, the eta = 0 update with it."""
    total = len(alphas)
    cur_last, x0_last, e_hist = None, None, []
    for t, cur, prev in S.schedule(alphas, ts, step):
        x0, e = x0_eps(x, predict_v(x, t, cur), cur)
        sp, dn = math.sqrt(prev), math.sqrt(1.0 - prev)
        s = (total - 1 - t) // step
        if kind == "ddim":
            sigma = eta * math.sqrt((1.0 - prev) / (1.0 - cur)) * math.sqrt(1.0 - cur / prev)
            nx = sp * x0 + math.sqrt(1.0 - prev - sigma * sigma) * e
            if sigma != 0.0:
                nx = nx + sigma * noise(s)
        elif kind == "dpmpp_2m":
            if prev >= 1.0:
                nx = x0
            else:
                h = _lam(prev) - _lam(cur)
                D = x0
                if x0_last is not None and cur_last != 0.0 and cur != 0.0:
                    r = (_lam(cur) - _lam(cur_last)) / h
                    D = (1.0 + 1.0 / (2.0 * r)) * x0 - (1.0 / (2.0 * r)) * x0_last
                nx = (dn / math.sqrt(1.0 - cur)) * x - sp * math.expm1(-h) * D
            cur_last, x0_last = cur, x0
        elif kind == "plms":
            w = S.AB[min(3, len(e_hist))]
            ep = w[0] * e
            for k in range(1, len(w)):
                ep = ep + w[k] * e_hist[k - 1]
            # the eta = 0 update with eps' in place of eps_hat: x0' = x0 - (sn / sc)(eps' - eps_hat); with no history eps' = eps_hat and x0' = x0
            x0p = x0 if not e_hist else x0 - (math.sqrt(1.0 - cur) / math.sqrt(cur)) * (ep - e)
            nx = sp * x0p + dn * ep
            e_hist = [e] + e_hist[:2]
        else:
            raise ValueError(kind)
        x = nx if blend is None else blend(nx, prev)
    return x
