"""qkv_attention with a per-sample key count -- the CFG batch's cross attention, whose unconditional rows have Tu keys and conditional rows Tc, with K / V
padded to max(Tc, Tu) (Engine::sample_loop -> unet_prepare -> AttnParams::kv_len) -- through sdmi_op_qkv_attention_ragged, against the fp64 oracle on each
row's own keys.

Every kernel takes three things from its row's count: its tile count, the mask on its ragged last tile and the bounds of its key slices.  Here the keys behind
each row's count are NaN, so a kernel that lets one of them into the scores or into P V writes NaN (in the model they are finite projections of the zero
padding, which would only dilute the softmax).  Each call mixes 1 and 2 keys (empty key slices), tile - 1 / tile / tile + 1 for the kernel that runs, 77 and
the padded count, over k_attn.hip, k_attn_split.hip, k_attn_bf16.hip and the unfused GEMM path, their option forms and both grid regimes (4- and 8-wave
workgroups).  The bars are the operator bars of test_ops_gpu.py / test_bf16_gpu.py, per row.  Two identities hold bit for bit: with every count = nk the entry
IS sdmi_qkv_attention, and permuting the batch rows permutes the output.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import sd_oracle as O

pytestmark = pytest.mark.gpu

FP32_BAR = 2e-5                                 # test_ops_gpu.py RTOL
BF16_BAR, BF16_BAR_UNFUSED = 2 ** -7, 2 ** -6   # test_bf16_gpu.py: fused (q rounded once more at this boundary) / unfused (bf16 probabilities)
SDMI_ERR_INVALID, SDMI_ERR_UNSUPPORTED = -1, -5


def bf16_round(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _engine(precision):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    return StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=precision))


@pytest.fixture(scope="module")
def ops32():
    sd = _engine(0)
    yield sd
    sd.close()


@pytest.fixture(scope="module")
def ops16():
    sd = _engine(1)
    yield sd
    sd.close()


_DEFAULTS = {"attn_split": 1, "attn_kv_splits": 0, "attn_pack_tail": "default", "gemm_planes": "default", "attn_bf16": 1, "attn_bf16_variant": "default"}

# (query rows, heads) with 8 - 10 batch rows.  small: one query tile per (row, head) -- the 4-wave k_attn.hip / k_attn_split.hip workgroups (also with 8 key
# slices), the 2-wave k_attn_bf16.hip one, and automatic key slices (4 / 8 of them); medium: the 4-wave k_attn_bf16.hip workgroup; large: 2048 + 37 query rows --
# the 8-wave workgroups of all three kernels (k_attn_split.hip's non-log2 form at d = 80 has only the 4-wave one), and at d = 40 / 80 with <= 128 keys
# k_attn_bf16.hip's two-per-CU form (attn_bf16_variant bit 0)
GRIDS = {"small": (100, 2), "medium": (200, 16), "large": (2085, 4)}


def _counts(nk, tiles):
    """per-row key counts in 1 .. nk: 1, 2, tile - 1 / tile / tile + 1 for every key tile given, 77 and nk, filled up to 8 rows; in a fixed shuffled order"""
    want = [1, 2] + [t + e for t in tiles for e in (-1, 0, 1)] + [77, nk]
    counts = [x for x in dict.fromkeys(want) if 1 <= x <= nk]
    for x in (nk - 1, 3, 2 * tiles[0] + 1, 5, 6):
        if len(counts) < 8 and 1 <= x <= nk and x not in counts:
            counts.append(x)
    order = np.random.default_rng(1000 * len(counts) + nk).permutation(len(counts))
    return tuple(int(counts[i]) for i in order)


@functools.lru_cache(maxsize=2)
def _data(nq, nk, c, heads, counts, fmt):
    """q, k, v (finite); k, v with NaN behind every row's count; the fp64 oracle on each row's own keys.  fmt 'bf16': q / k / v on the bf16 grid."""
    n = len(counts)
    g = np.random.default_rng(zlib.crc32(repr((n, nq, nk, c, heads, fmt)).encode()))
    q = g.standard_normal((n, nq, c)).astype(np.float32)
    k = g.standard_normal((n, nk, c)).astype(np.float32)
    v = (g.standard_normal((n, nk, c)) * np.exp2(g.integers(-3, 4, (1, 1, c)))).astype(np.float32)   # a column mixed up with another shows
    if fmt == "bf16":
        q, k, v = bf16_round(q), bf16_round(k), bf16_round(v)
    kn, vn = k.copy(), v.copy()
    ref = np.empty((n, nq, c))
    for b, L in enumerate(counts):
        kn[b, L:] = np.nan
        vn[b, L:] = np.nan
        ref[b] = O.qkv_attention(_t(q[b:b + 1]), _t(k[b:b + 1, :L]), _t(v[b:b + 1, :L]), None, heads)[0].numpy()
    return q, k, v, kn, vn, ref


def _check_rows(got, ref, counts, what, bar):
    """bar x max(1, max|ref|) per row; prints the worst row"""
    got = np.asarray(got, np.float64)
    counts = np.asarray(counts)
    assert got.shape == ref.shape, what
    nan_rows = ~np.isfinite(got).all(axis=(1, 2))
    assert not nan_rows.any(), f"{what}: non-finite output in rows {np.flatnonzero(nan_rows).tolist()} (kv_len {counts[nan_rows].tolist()}): a key behind the row's count was read"
    err = np.abs(got - ref).max(axis=(1, 2))
    bound = bar * np.maximum(1.0, np.abs(ref).max(axis=(1, 2)))
    w = int(np.argmax(err / bound))
    print(f"{what}: worst row {w} (kv_len {counts[w]}): max|d| = {err[w]:.3e}, bar {bound[w]:.3e}")
    over = err > bound
    assert not over.any(), f"{what}: rows {np.flatnonzero(over).tolist()} (kv_len {counts[over].tolist()}) over the bar; worst row {w}: max|d| = {err[w]:.3e} > {bound[w]:.3e}"


def _ragged(sd, nq, nk, d, heads, counts, fmt, bar, what, **opts):
    """under the given engine options (restored afterwards): the ragged call against the oracle; with every count = nk and finite K / V, bit for bit the
    nullptr path (sdmi_qkv_attention); with the batch rows permuted, bit for bit the permuted output"""
    c = d * heads
    q, k, v, kn, vn, ref = _data(nq, nk, c, heads, counts, fmt)
    n = len(counts)
    kv = np.asarray(counts, np.int32)
    what = f"{what} n={n} nq={nq} nk={nk} d={d} heads={heads} {opts}"
    try:
        for key, val in opts.items():
            sd.set_option(key, val)
        got = sd.qkv_attention_ragged(q, kn, vn, kv, heads)
        _check_rows(got, ref, counts, what, bar)
        full = sd.qkv_attention_ragged(q, k, v, np.full(n, nk, np.int32), heads)
        np.testing.assert_array_equal(full, sd.qkv_attention(q, k, v, None, heads), err_msg=f"{what}: every kv_len = nk differs from sdmi_qkv_attention")
        perm = (np.arange(n) + 3) % n       # every row moves
        np.testing.assert_array_equal(sd.qkv_attention_ragged(q[perm], kn[perm], vn[perm], kv[perm], heads), got[perm],
                                      err_msg=f"{what}: permuting the batch rows changes a row's result")
    finally:
        for key in opts:
            sd.set_option(key, _DEFAULTS[key])


# ---- precision 0: k_attn_split.hip (d = 40 / 80, attn_split = 1) and k_attn.hip (attn_split = 0; d = 160 always), key slices, fp32 rows and bf16 planes -------------------
NK32 = 8 * 64 + 8       # 9 key tiles of 64 (17 of 32): rows with 1 or 2 keys leave all but their first key slice empty


def _tile32(d, split):
    """keys per tile of the fp32 kernel that runs (attn_f32_kv_tile)"""
    return 64 if split and d in (40, 80) else (32 if d > 96 else 64)


@pytest.mark.parametrize("kv_splits", [1, 0, 2, 3, 8, 16])
@pytest.mark.parametrize("grid", ["small", "large"])
@pytest.mark.parametrize("d,split", [(40, 1), (40, 0), (80, 1), (80, 0), (160, 0)])
def test_ragged_fp32(ops32, d, split, grid, kv_splits):
    """kv_splits 0 = the engine's rule (4 / 8 slices on the small grid, none on the large one); 16 = one slice per key tile (9, 17 at d = 160): more than 8, the
    merge launch's loop form"""
    nq, heads = GRIDS[grid]
    counts = _counts(NK32, (_tile32(d, split),))
    for planes in (0, 1):
        _ragged(ops32, nq, NK32, d, heads, counts, "f32", FP32_BAR, "fp32", attn_split=split, attn_kv_splits=kv_splits, gemm_planes=planes)


@pytest.mark.parametrize("kv_splits", [1, 8])
@pytest.mark.parametrize("grid", ["small", "large"])
@pytest.mark.parametrize("d,pack", [(40, 0), (40, 1), (40, 2), (40, 3), (80, 0), (80, 2)])
def test_ragged_fp32_split_pack_tail(ops32, d, pack, grid, kv_splits):
    """k_attn_split.hip's forms: bit 0 = d = 40's packed tail step / output tile, bit 1 = the log2-unit softmax with the row sum from a ones column
    (at d = 80 without it: the 4-wave-only form)"""
    nq, heads = GRIDS[grid]
    _ragged(ops32, nq, NK32, d, heads, _counts(NK32, (64,)), "f32", FP32_BAR, "fp32 split", attn_split=1, attn_pack_tail=pack, attn_kv_splits=kv_splits)


# ---- precision 1: k_attn_bf16.hip and its round-6 forms (attn_bf16_variant), bf16 storage widened onto k_attn.hip (attn_bf16 = 0) ---------------------------------------
# (d, attn_bf16, attn_bf16_variant): 0x100 forces a form whatever the grid -- bit 0: two 4-wave workgroups per CU (d = 40 / 80), bit 1 / 2: 64 query rows per wave
# on 8- / 4-wave workgroups (d = 40; 64-key tiles instead of 128)
BF16_FORMS = [(40, 1, "default"), (40, 1, 0), (40, 1, 0x101), (40, 1, 0x102), (40, 1, 0x104), (40, 0, "default"),
              (80, 1, "default"), (80, 1, 0), (80, 1, 0x101), (80, 0, "default"),
              (160, 1, "default"), (160, 1, 0), (160, 0, "default")]


# the key tiles of both kernels at each head dim: k_attn_bf16.hip walks 128 keys at d = 40 (64 in its two-block forms), 64 otherwise; k_attn.hip 64, 32 at d = 160
TILES16 = {40: (128, 64), 80: (64,), 160: (64, 32)}


@pytest.mark.parametrize("d,mfma16,variant", BF16_FORMS, ids=[f"d{d}-attn_bf16={m}-variant={v}" for d, m, v in BF16_FORMS])
@pytest.mark.parametrize("grid", ["small", "medium", "large"])
@pytest.mark.parametrize("nk", [128, 300])       # k_attn_bf16.hip picks its instance with short_ctx = nk <= 128 (the padded count)
def test_ragged_bf16(ops16, nk, grid, d, mfma16, variant):
    nq, heads = GRIDS[grid]
    _ragged(ops16, nq, nk, d, heads, _counts(nk, TILES16[d]), "bf16", BF16_BAR, "bf16", attn_bf16=mfma16, attn_bf16_variant=variant)


# ---- d = 64 (CLIP's head dim): the fused k_attn.hip instance at both precisions -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_splits", [1, 3])
def test_ragged_d64_fp32(ops32, kv_splits):
    counts = _counts(200, (64,))
    for planes in (0, 1):
        _ragged(ops32, 100, 200, 64, 1, counts, "f32", FP32_BAR, "fp32 d=64", attn_kv_splits=kv_splits, gemm_planes=planes)


def test_ragged_d64_bf16(ops16):
    _ragged(ops16, 100, 200, 64, 1, _counts(200, (64,)), "bf16", BF16_BAR, "bf16 d=64")


# ---- the unfused path (head dims without a fused instance: one (row, head) at a time, QK^T -> row softmax -> PV on the GEMM kernels) --------------------------------------
UNFUSED_COUNTS = {0: (96, 32, 256, 64, 224, 160, 128, 32), 1: (128, 64, 320, 192, 64, 256, 320, 128)}   # multiples of 32 (fp32) / 64 (bf16)


@pytest.mark.parametrize("d", [128, 512])
def test_ragged_unfused_fp32(ops32, d):
    counts = UNFUSED_COUNTS[0]
    _ragged(ops32, 100, max(counts), d, 1, counts, "f32", FP32_BAR, "fp32 unfused")


@pytest.mark.parametrize("d", [128, 512])
def test_ragged_unfused_bf16(ops16, d):
    counts = UNFUSED_COUNTS[1]
    _ragged(ops16, 100, max(counts), d, 1, counts, "bf16", BF16_BAR_UNFUSED, "bf16 unfused")


@pytest.mark.parametrize("precision,bad", [(0, 48), (1, 96)])
def test_ragged_unfused_rejects_other_counts(ops32, ops16, precision, bad):
    """the unfused path takes key counts that are multiples of 32 (64 at precision 1) only: anything else is SDMI_ERR_UNSUPPORTED, not a wrong result"""
    from stable_diffusion_burn_amd import SdmiError
    sd = ops16 if precision else ops32
    q, k, v, _, _, _ = _data(100, max(UNFUSED_COUNTS[precision]), 128, 1, UNFUSED_COUNTS[precision], "bf16" if precision else "f32")
    counts = np.array(UNFUSED_COUNTS[precision], np.int32)
    counts[3] = bad
    with pytest.raises(SdmiError) as ei:
        sd.qkv_attention_ragged(q, k, v, counts, 1)
    assert ei.value.status == SDMI_ERR_UNSUPPORTED, str(ei.value)


# ---- argument checks ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
def test_ragged_rejects_bad_kv_len(ops32, ops16, precision):
    """NULL kv_len and entries outside 1 .. nk are SDMI_ERR_INVALID (checked before anything is copied or launched); a kv_len of the wrong length never leaves Python"""
    from stable_diffusion_burn_amd import SdmiError
    sd = ops16 if precision else ops32
    n, nq, nk, heads = 3, 20, 40, 2
    g = np.random.default_rng(11)
    q = g.standard_normal((n, nq, 80)).astype(np.float32)
    k, v = (g.standard_normal((n, nk, 80)).astype(np.float32) for _ in range(2))
    for bad in (None, [5, 0, 7], [5, 7, nk + 1], [-3, 5, 7]):
        with pytest.raises(SdmiError) as ei:
            sd.qkv_attention_ragged(q, k, v, bad, heads)
        assert ei.value.status == SDMI_ERR_INVALID and "kv_len" in str(ei.value), f"kv_len={bad}: {ei.value}"
    with pytest.raises(ValueError):
        sd.qkv_attention_ragged(q, k, v, [5, 7], heads)
    got = sd.qkv_attention_ragged(q, k, v, [1, nk, 17], heads)        # and the engine goes on working
    assert np.isfinite(got).all()
