"""fp64 references of the operators at chosen outputs -- TEST INFRASTRUCTURE ONLY.

A full fp64 oracle of a megapixel convolution or a 16384-token attention takes minutes on the host.  Attention rows, convolution pixels and
Linear rows are independent of each other, so these helpers compute the reference only where a test checks it: for a convolution every output
channel and every k of the sampled pixels, for attention every key and every column of the sampled query rows.  Plain numpy / torch, fp64 throughout.
tests/test_sampled_ref_cpu.py pins every helper to the full oracle (oracle/sd_oracle.py) at the sampled positions, exactly.

Flat pixel p of an [n, c, ho, wo] output means (sample, y, x) = (p // (ho wo), p % (ho wo) // wo, p % wo) -- the row of the implicit GEMM.
"""
import numpy as np
import torch


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def out_hw(h, w, k, stride=1, ups=0):
    pad = 1 if k == 3 else 0
    return ((h << ups) + 2 * pad - k) // stride + 1, ((w << ups) + 2 * pad - k) // stride + 1


def _sample(m, picks, tile_heights, extra, seed):
    for tile_rows in tile_heights:
        n_tiles = (m + tile_rows - 1) // tile_rows
        for t in {0, n_tiles // 2, n_tiles - 1}:
            picks.append(np.array([tile_rows * t - 1, tile_rows * t, tile_rows * t + 1], dtype=np.int64))
    g = np.random.default_rng(seed)
    picks.append(g.integers(0, m, size=extra, dtype=np.int64))
    p = np.unique(np.concatenate(picks))
    p = p[(p >= 0) & (p < m)]
    want = min(m, 2048)
    if p.size < want:      # top up with further seeded positions (small outputs: everything)
        rest = np.setdiff1d(np.arange(m, dtype=np.int64), p)
        p = np.union1d(p, g.permutation(rest)[:want - p.size])
    return p


def sample_pixels(n, ho, wo, tile_rows=256, extra=1024, seed=0):
    """The sorted flat output pixels (GEMM rows) of an [n, ho, wo] output that a sampled check looks at.  The set is a condition, not a choice:
    the first and last pixel of every sample; every pixel of the four image borders of the first and last sample; the pixels 256 t - 1, 256 t
    and 256 t + 1 for the first, a middle and the last tile of tile_rows rows; `extra` seeded random pixels; at least min(M, 2048) pixels."""
    hw = ho * wo
    picks = [np.arange(n, dtype=np.int64) * hw, np.arange(n, dtype=np.int64) * hw + hw - 1]
    ys, xs = np.arange(ho, dtype=np.int64), np.arange(wo, dtype=np.int64)
    for s in {0, n - 1}:
        base = s * hw
        picks += [base + xs, base + (ho - 1) * wo + xs, base + ys * wo, base + ys * wo + wo - 1]
    return _sample(n * hw, picks, (tile_rows,), extra, seed)


def sample_rows(n, rows, tile_heights=(64, 128), extra=1024, seed=0):
    """sample_pixels for the query rows of an [n, rows, c] attention operand or the rows of a Linear layer (n = 1).  A sequence has no image
    borders beyond its first and last row; the tile rule is applied at both query-tile heights (64 and 128)."""
    picks = [np.arange(n, dtype=np.int64) * rows, np.arange(n, dtype=np.int64) * rows + rows - 1]
    return _sample(n * rows, picks, tile_heights, extra, seed)


def conv_at(x, w, b, pixels, stride=1, ups=0, temb=None, resid=None):
    """conv2d(nearest-2x^ups(x), w, zero padding 1 for 3x3 / 0 for 1x1, stride) + b + temb[sample] + resid at the given flat output pixels:
    [len(pixels), cout] in fp64.  x [n, cin, h, w]; w [cout, cin, k, k]; temb [cout] or [n, cout]; resid [n, cout, ho, wo]."""
    n, cin, h, wd = x.shape
    cout, _, k, _ = w.shape
    pad = 1 if k == 3 else 0
    ho, wo = out_hw(h, wd, k, stride, ups)
    hu, wu = h << ups, wd << ups
    pixels = np.asarray(pixels, dtype=np.int64)
    s, r = pixels // (ho * wo), pixels % (ho * wo)
    oy, ox = r // wo, r % wo
    patches = np.zeros((pixels.size, cin, k, k), dtype=np.float64)
    for ky in range(k):
        for kx in range(k):
            iy = oy * stride - pad + ky        # coordinates in the (upsampled) input
            ix = ox * stride - pad + kx
            ok = (iy >= 0) & (iy < hu) & (ix >= 0) & (ix < wu)
            sy, sx = np.clip(iy, 0, hu - 1) >> ups, np.clip(ix, 0, wu - 1) >> ups
            v = _f64(x[s, :, sy, sx])           # [P, cin]
            v[~ok] = 0.0
            patches[:, :, ky, kx] = v
    out = patches.reshape(pixels.size, cin * k * k) @ _f64(w).reshape(cout, cin * k * k).T
    if b is not None:
        out += _f64(b)[None, :]
    if temb is not None:
        t = _f64(temb)
        out += t[None, :] if t.ndim == 1 else t[s]
    if resid is not None:
        out += _f64(resid[s, :, oy, ox])
    return out


def at_pixels(y, pixels):
    """[len(pixels), c]: the values of an [n, c, h, w] tensor at flat pixels, in the layout conv_at / group_norm_at return"""
    n, c, h, w = y.shape
    pixels = np.asarray(pixels, dtype=np.int64)
    s, r = pixels // (h * w), pixels % (h * w)
    return y[s, :, r // w, r % w]


def linear_at(x, w, b, rows, resid=None):
    """(x @ w + b + resid)[rows] in fp64; x [rows_total, cin], w [cin, cout]"""
    rows = np.asarray(rows, dtype=np.int64)
    out = _f64(x[rows]) @ _f64(w)
    if b is not None:
        out += _f64(b)[None, :]
    if resid is not None:
        out += _f64(resid[rows])
    return out


def attention_at(q, k, v, rows, heads, kv_len=None):
    """qkv_attention (attention.rs:5-45) at flat query rows (sample * nq + row): [len(rows), c] in fp64, every key and every column.
    kv_len [n]: sample b attends to its first kv_len[b] keys only."""
    n, nq, c = q.shape
    nk = k.shape[1]
    d = c // heads
    scale = float(d) ** -0.25
    rows = np.asarray(rows, dtype=np.int64)
    out = np.empty((rows.size, c), dtype=np.float64)
    smp = rows // nq
    for b in np.unique(smp):
        sel = np.nonzero(smp == b)[0]
        live = nk if kv_len is None else int(kv_len[b])
        qs = _t64(q[b, rows[sel] % nq]) * scale
        ks = _t64(k[b, :live]) * scale
        vs = _t64(v[b, :live])
        for hd in range(heads):          # one head at a time: a [P, nk] score matrix, worked on in place
            cols = slice(hd * d, (hd + 1) * d)
            sc = qs[:, cols].contiguous() @ ks[:, cols].t().contiguous()
            sc -= sc.max(dim=1, keepdim=True).values
            sc.exp_()
            den = sc.sum(dim=1, keepdim=True)
            out[sel, cols] = ((sc @ vs[:, cols].contiguous()) / den).numpy()
    return out


def group_stats(x, groups):
    """(mean, biased variance) [n, groups] of an [n, c, h, w] tensor in fp64, two-pass, one group at a time (a whole > 2 GiB tensor is never widened)"""
    n, c, h, w = x.shape
    cg = c // groups
    mean = np.empty((n, groups), dtype=np.float64)
    var = np.empty((n, groups), dtype=np.float64)
    for s in range(n):
        for g in range(groups):
            u = _t64(x[s, g * cg:(g + 1) * cg])
            mean[s, g] = float(u.mean())
            u -= mean[s, g]
            var[s, g] = float((u * u).mean())
    return mean, var


def group_norm_at(x, gamma, beta, groups, eps, silu, pixels, stats=None):
    """GroupNorm (groupnorm/mod.rs:53-82, biased variance, sqrt(var + eps)) (+ SiLU): statistics over the whole tensor in fp64, the values at
    the given flat pixels as [len(pixels), c].  stats: group_stats(x, groups), where several calls share them."""
    n, c, h, w = x.shape
    cg = c // groups
    mean, var = group_stats(x, groups) if stats is None else stats
    pixels = np.asarray(pixels, dtype=np.int64)
    s = pixels // (h * w)
    v = _f64(at_pixels(x, pixels))                                       # [P, c]
    mu = np.repeat(mean[s], cg, axis=1)
    rs = np.repeat(1.0 / np.sqrt(var[s] + eps), cg, axis=1)
    y = (v - mu) * rs * _f64(gamma)[None, :] + _f64(beta)[None, :]
    if silu:
        y = y / (1.0 + np.exp(-y))
    return y
