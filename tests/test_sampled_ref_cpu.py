"""tests/sampled_ref.py against the full fp64 oracle (oracle/sd_oracle.py) on the small shapes of tests/test_ops_gpu.py: every helper must give the
oracle's value at the positions it samples, and sample_pixels must meet its condition.

"Equal" in fp64: on small-integer operands every product and partial sum is an integer below 2^53, so the convolution and Linear helpers must
match the oracle BIT FOR BIT whatever order either sums in; on the seeded real-valued operands of the GPU tests the two differ by their summation
order only, i.e. by a few fp64 ulps of the largest partial sum -- bound 1e-12 max(1, |ref|), seven orders below the tightest GPU bar (2e-5)."""
import math

import numpy as np
import pytest
import torch

from oracle import sd_oracle as O
import sampled_ref as S

ULPS = 1e-12

CONV_CASES = [
    # n, cin, h, w, cout, k, stride, ups: test_ops_gpu.CONV_CASES (with its stride-2 and upsample cases) + a stride-2 case on odd sizes
    (2, 320, 16, 16, 320, 3, 1, 0), (1, 4, 16, 16, 320, 3, 1, 0), (1, 320, 16, 16, 4, 3, 1, 0), (1, 128, 16, 16, 3, 3, 1, 0), (1, 4, 8, 8, 4, 1, 1, 0),
    (2, 320, 16, 16, 320, 3, 2, 0), (1, 640, 8, 8, 640, 3, 1, 1), (2, 640, 16, 16, 320, 1, 1, 0), (1, 960, 8, 8, 640, 3, 1, 0), (1, 2560, 8, 8, 1280, 3, 1, 0),
    (1, 256, 24, 40, 128, 3, 1, 0), (3, 64, 5, 7, 96, 3, 1, 0), (1, 128, 33, 31, 128, 3, 2, 0), (1, 64, 12, 20, 384, 3, 1, 1),
]
ATTN_CASES = [
    # n, nq, nk, c, heads: test_ops_gpu.ATTN_CASES up to 256 tokens
    (2, 256, 256, 320, 8), (2, 64, 64, 640, 8), (1, 256, 256, 1280, 8), (2, 256, 77, 320, 8), (2, 64, 2, 1280, 8), (1, 100, 37, 160, 4), (1, 4, 4, 640, 4),
    (1, 64, 64, 128, 1), (1, 256, 256, 512, 1),
]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _close(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.float64, what
    err = np.abs(got - ref).max()
    assert err <= ULPS * max(1.0, np.abs(ref).max()), f"{what}: {err:.3e}"


def _full_conv(x, wt, b, stride, ups, temb, resid):
    xin = O.upsample2x(_t(x)) if ups else _t(x)
    k = wt.shape[-1]
    ref = O.conv2d(xin, (_t(wt), None if b is None else _t(b)), stride=stride, padding=1 if k == 3 else 0).numpy()
    if temb is not None:
        ref = ref + np.asarray(temb, np.float64)[:, :, None, None]
    if resid is not None:
        ref = ref + np.asarray(resid, np.float64)
    return ref


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_at_equals_the_oracle(case):
    n, cin, h, w, cout, k, stride, ups = case
    g = np.random.default_rng(hash(case) % (2 ** 31))
    ho, wo = S.out_hw(h, w, k, stride, ups)
    pix = S.sample_pixels(n, ho, wo, extra=64, seed=1)
    # integers: exact in any summation order -> bit for bit
    x = g.integers(-8, 9, (n, cin, h, w)).astype(np.float32)
    wt = g.integers(-8, 9, (cout, cin, k, k)).astype(np.float32)
    b = g.integers(-8, 9, cout).astype(np.float32)
    temb = g.integers(-8, 9, (n, cout)).astype(np.float32)
    resid = g.integers(-8, 9, (n, cout, ho, wo)).astype(np.float32)
    ref = _full_conv(x, wt, b, stride, ups, temb, resid)
    got = S.conv_at(x, wt, b, pix, stride, ups, temb, resid)
    assert np.array_equal(got, S.at_pixels(ref, pix)), f"conv_at {case} (integers)"
    # the GPU tests' operands, with and without each term
    x = g.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (g.standard_normal((cout, cin, k, k)) / math.sqrt(cin * k * k)).astype(np.float32)
    b = g.standard_normal(cout).astype(np.float32)
    temb = g.standard_normal((n, cout)).astype(np.float32)
    resid = g.standard_normal((n, cout, ho, wo)).astype(np.float32)
    _close(S.conv_at(x, wt, b, pix, stride, ups, temb, resid), S.at_pixels(_full_conv(x, wt, b, stride, ups, temb, resid), pix), f"conv_at {case}")
    _close(S.conv_at(x, wt, None, pix, stride, ups), S.at_pixels(_full_conv(x, wt, None, stride, ups, None, None), pix), f"conv_at {case} bare")
    one = temb[0]          # one row for the batch
    _close(S.conv_at(x, wt, b, pix, stride, ups, one), S.at_pixels(_full_conv(x, wt, b, stride, ups, np.broadcast_to(one, (n, cout)), None), pix),
           f"conv_at {case} shared temb")


@pytest.mark.parametrize("rows,cin,cout", [(154, 768, 320), (20, 320, 1280), (512, 320, 2560), (1, 1280, 1280), (77, 64, 160)])
def test_linear_at_equals_the_oracle(rows, cin, cout):
    g = np.random.default_rng(rows * 3 + cout)
    rs = S.sample_rows(1, rows, extra=32, seed=2)
    x = g.integers(-8, 9, (rows, cin)).astype(np.float32)
    wt = g.integers(-8, 9, (cin, cout)).astype(np.float32)
    b = g.integers(-8, 9, cout).astype(np.float32)
    resid = g.integers(-8, 9, (rows, cout)).astype(np.float32)
    ref = O.linear(_t(x), _t(wt), _t(b)).numpy() + resid
    assert np.array_equal(S.linear_at(x, wt, b, rs, resid), ref[rs])
    x = g.standard_normal((rows, cin)).astype(np.float32)
    wt = (g.standard_normal((cin, cout)) / math.sqrt(cin)).astype(np.float32)
    _close(S.linear_at(x, wt, b, rs, resid), (O.linear(_t(x), _t(wt), _t(b)).numpy() + resid)[rs], f"linear_at ({rows},{cin},{cout})")
    _close(S.linear_at(x, wt, None, rs), O.linear(_t(x), _t(wt), None).numpy()[rs], f"linear_at ({rows},{cin},{cout}) bare")


@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_at_equals_the_oracle(case):
    n, nq, nk, c, heads = case
    g = np.random.default_rng(hash(case) % (2 ** 31))
    q = g.standard_normal((n, nq, c)).astype(np.float32)
    k = g.standard_normal((n, nk, c)).astype(np.float32)
    v = g.standard_normal((n, nk, c)).astype(np.float32)
    rs = S.sample_rows(n, nq, extra=32, seed=3)
    ref = O.qkv_attention(_t(q), _t(k), _t(v), None, heads).numpy().reshape(n * nq, c)
    _close(S.attention_at(q, k, v, rs, heads), ref[rs], f"attention_at {case}")
    if nk > 2:      # per-sample key counts: the oracle on each sample's own prefix
        kv_len = np.array([max(1, nk - 3 * (b + 1)) for b in range(n)])
        ref = np.concatenate([O.qkv_attention(_t(q[b:b + 1]), _t(k[b:b + 1, :kv_len[b]]), _t(v[b:b + 1, :kv_len[b]]), None, heads).numpy()[0] for b in range(n)])
        _close(S.attention_at(q, k, v, rs, heads, kv_len), ref[rs], f"attention_at {case} kv_len")


@pytest.mark.parametrize("shape", [(2, 320, 16, 16), (1, 128, 32, 32)])
@pytest.mark.parametrize("silu", [False, True])
def test_group_norm_at_equals_the_oracle(shape, silu):
    n, c, h, w = shape
    g = np.random.default_rng(c * 7 + h)
    x = (g.standard_normal(shape) * 1.7 + 0.9).astype(np.float32)
    gamma = (1 + 0.1 * g.standard_normal(c)).astype(np.float32)
    beta = (0.1 * g.standard_normal(c)).astype(np.float32)
    ref = O.group_norm(_t(x), _t(gamma), _t(beta), 32, 1e-5)
    if silu:
        ref = O.silu(ref)
    pix = S.sample_pixels(n, h, w, extra=64, seed=4)
    _close(S.group_norm_at(x, gamma, beta, 32, 1e-5, silu, pix), S.at_pixels(ref.numpy(), pix), f"group_norm_at {shape} silu={silu}")
    mean, var = S.group_stats(x, 32)
    xg = _t(x).reshape(n, 32, -1)
    _close(mean, xg.mean(dim=2).numpy(), "group mean")
    _close(var, xg.var(dim=2, unbiased=False).numpy(), "group variance")


# ---- the sampled set is a condition ---------------------------------------------------------------------------------------------------------------
def _condition(n, ho, wo, tile_rows, extra, seed, pix):
    hw, m = ho * wo, n * ho * wo
    have = set(pix.tolist())
    assert pix.ndim == 1 and np.all(np.diff(pix) > 0) and pix[0] >= 0 and pix[-1] < m, "sorted, distinct, in range"
    for s in range(n):
        assert s * hw in have and s * hw + hw - 1 in have, f"first / last pixel of sample {s}"
    for s in (0, n - 1):
        for x in range(wo):
            assert s * hw + x in have and s * hw + (ho - 1) * wo + x in have, f"top / bottom border of sample {s}"
        for y in range(ho):
            assert s * hw + y * wo in have and s * hw + y * wo + wo - 1 in have, f"left / right border of sample {s}"
    tiles = (m + tile_rows - 1) // tile_rows
    for t in (0, tiles // 2, tiles - 1):
        for p in (tile_rows * t - 1, tile_rows * t, tile_rows * t + 1):
            if 0 <= p < m:
                assert p in have, f"tile {t} boundary pixel {p}"
    rnd = np.random.default_rng(seed).integers(0, m, size=extra, dtype=np.int64)
    assert set(rnd.tolist()) <= have, "the seeded random pixels"
    assert pix.size >= min(m, 2048)


@pytest.mark.parametrize("n,ho,wo", [(1, 5, 7), (1, 15, 17), (1, 16, 16), (2, 8, 16), (1, 16, 17), (2, 72, 88), (3, 36, 44), (2, 9, 11), (1, 1, 1), (2, 1, 300), (1, 1024, 1024)])
@pytest.mark.parametrize("extra", [0, 1024])
def test_sample_pixels_meets_its_condition(n, ho, wo, extra):
    """M below one tile (35, 255), one tile exactly (256, n = 1 and n = 2), just above (272), many tiles, one-pixel and one-row images"""
    pix = S.sample_pixels(n, ho, wo, tile_rows=256, extra=extra, seed=11)
    _condition(n, ho, wo, 256, extra, 11, pix)
    assert np.array_equal(pix, S.sample_pixels(n, ho, wo, tile_rows=256, extra=extra, seed=11)), "seeded: the same set again"


@pytest.mark.parametrize("n,rows", [(1, 63), (1, 64), (1, 65), (2, 128), (2, 129), (2, 6336), (2, 16384), (1, 4)])
def test_sample_rows_meets_the_condition_at_both_tile_heights(n, rows):
    rs = S.sample_rows(n, rows, extra=256, seed=5)
    m = n * rows
    have = set(rs.tolist())
    assert np.all(np.diff(rs) > 0) and rs[0] >= 0 and rs[-1] < m
    for s in range(n):
        assert s * rows in have and s * rows + rows - 1 in have, f"first / last row of sample {s}"
    for th in (64, 128):
        tiles = (m + th - 1) // th
        for t in (0, tiles // 2, tiles - 1):
            for p in (th * t - 1, th * t, th * t + 1):
                assert not 0 <= p < m or p in have, f"tile height {th}: boundary row {p}"
    assert set(np.random.default_rng(5).integers(0, m, size=256, dtype=np.int64).tolist()) <= have
    assert rs.size >= min(m, 2048)
    assert rs.size <= 2048 + 256 + 64, "a sample, not everything"
