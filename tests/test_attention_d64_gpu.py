"""Head dim 64 on k_attn_split.hip and k_attn_bf16.hip (option attn_d64) -- the instances SD 2.x's UNet runs its attention on -- by the
method of tests/test_attention_ragged_gpu.py: per-sample key counts with NaN behind each row's count, the fp64 oracle on each row's own keys, that file's bars,
and its two bit-exact identities (all counts = nk IS qkv_attention; permuting the batch rows permutes the output).  Every case first reads the plan back
(sd.attention_plan) and asserts the kernel and wave count it is about.  Last: with attn_d64 = 0 the same context gives, bit for bit, what a context that never
heard of the option gives -- the gate leaks nothing.

At d = 64 both O^T tiles of k_attn_split.hip are full: its log2-unit softmax takes the row sum lane-locally instead of from a ones column of V (the form
attn_pack_tail bit 1 selects; without the bit the older softmax runs).  Both forms are run."""
import numpy as np
import pytest

from test_attention_ragged_gpu import BF16_BAR, FP32_BAR, GRIDS, _check_rows, _counts, _data, _ragged

pytestmark = pytest.mark.gpu

D = 64
NK32 = 8 * 64 + 8       # 9 key tiles of 64: rows with 1 or 2 keys leave all but their first key slice empty


def _engine(precision, d64):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=precision))
    if d64:
        sd.set_option("attn_d64", 1)
    return sd


@pytest.fixture(scope="module")
def e32():
    sd = _engine(0, True)
    yield sd
    sd.close()


@pytest.fixture(scope="module")
def e16():
    sd = _engine(1, True)
    yield sd
    sd.close()


def _plan(sd, n, heads, nq, nk, kernel, waves, kv_splits=None, **opts):
    """the plan of the call under the options the case runs with (restored by the caller's _ragged, which sets them again)"""
    try:
        for k, v in opts.items():
            sd.set_option(k, v)
        p = sd.attention_plan(n, heads, nq, nk, D)
    finally:
        for k in opts:
            sd.set_option(k, {"attn_kv_splits": 0, "attn_pack_tail": "default", "gemm_planes": "default"}[k])
    assert (p["kernel"], p["waves"]) == (kernel, waves), f"the case does not reach its instance: {p}"
    assert p["q_rows"] == 32 * waves and p["kv_tile"] == 64, p
    if kv_splits is not None:
        assert p["kv_splits"] == kv_splits, p
    return p


# ---- precision 0: k_attn_split.hip ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", [3, 0])
@pytest.mark.parametrize("kv_splits,slices", [(0, 4), (1, 1), (8, 8)])
def test_split_small_4_waves_and_key_slices(e32, kv_splits, slices, pack):
    """one query tile per (row, head): the 4-wave form; the automatic rule gives 4 key slices, 8 are forced (rows with 1 or 2 keys: empty slices), and the merge launch"""
    nq, heads = GRIDS["small"]
    counts = _counts(NK32, (64,))
    assert len(counts) == 8 and {1, 2, 63, 64, 65, 77, NK32} <= set(counts)
    _plan(e32, 8, heads, nq, NK32, "split", 4, slices, attn_kv_splits=kv_splits, attn_pack_tail=pack)
    for planes in (0, 1):
        _ragged(e32, nq, NK32, D, heads, counts, "f32", FP32_BAR, "fp32 d=64 split", attn_kv_splits=kv_splits, attn_pack_tail=pack, gemm_planes=planes)


@pytest.mark.parametrize("pack", [3, 0])
@pytest.mark.parametrize("nk", [NK32, 77])
def test_split_large_8_waves(e32, nk, pack):
    nq, heads = GRIDS["large"]
    counts = _counts(nk, (64,))
    _plan(e32, 8, heads, nq, nk, "split", 8, 1, attn_pack_tail=pack)
    for planes in (0, 1):
        _ragged(e32, nq, nk, D, heads, counts, "f32", FP32_BAR, "fp32 d=64 split", attn_pack_tail=pack, gemm_planes=planes)


def test_split_cross_small(e32):
    """a 77-key context on the 4-wave form: two key tiles, the second one 13 keys"""
    nq, heads = GRIDS["small"]
    _plan(e32, 8, heads, nq, 77, "split", 4, 1)
    _ragged(e32, nq, 77, D, heads, _counts(77, (64,)), "f32", FP32_BAR, "fp32 d=64 split cross")


@pytest.mark.parametrize("grid,nk,kv_splits", [("small", NK32, 0), ("small", NK32, 8), ("large", NK32, 0), ("large", 77, 0)])
def test_split_plane_output_equals_row_output(e32, grid, nk, kv_splits):
    """the three-plane output (what the UNet's transformer blocks take under gemm_planes) joined back against the fp32-row output of the same kernel"""
    nq, heads = GRIDS[grid]
    counts = _counts(nk, (64,))
    q, k, v, kn, vn, ref = _data(nq, nk, D * heads, heads, counts, "f32")
    kv = np.asarray(counts, np.int32)
    out = {}
    try:
        e32.set_option("attn_kv_splits", kv_splits)
        for planes in (0, 1):
            e32.set_option("gemm_planes", planes)
            assert e32.attention_plan(8, heads, nq, nk, D)["kernel"] == "split"
            out[planes] = e32.qkv_attention_ragged(q, kn, vn, kv, heads)
            _check_rows(out[planes], ref, counts, f"d=64 split {grid} nk={nk} slices={kv_splits} planes={planes}", FP32_BAR)
    finally:
        e32.set_option("gemm_planes", "default")
        e32.set_option("attn_kv_splits", 0)
    err = np.abs(out[1].astype(np.float64) - out[0]).max(axis=(1, 2))
    bound = FP32_BAR * np.maximum(1.0, np.abs(ref).max(axis=(1, 2)))
    print(f"plane output vs row output: worst {float((err / bound).max()):.3f} of the bar")
    assert (err <= bound).all()


def test_masked_and_unaligned_stay_on_the_flash_kernel(e32):
    assert e32.attention_plan(1, 16, 77, 77, D, has_mask=True)["kernel"] == "flash"
    assert e32.attention_plan(2, 2, 100, 200, 40)["kernel"] == "split"          # the other head dims are untouched
    try:
        e32.set_option("attn_split", 0)
        assert e32.attention_plan(8, 2, 100, NK32, D)["kernel"] == "flash"
    finally:
        e32.set_option("attn_split", 1)


# ---- precision 1: k_attn_bf16.hip --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [300, 77])
@pytest.mark.parametrize("grid,waves", [("small", 2), ("medium", 4), ("large", 8)])
def test_bf16_forms(e16, grid, waves, nk):
    nq, heads = GRIDS[grid]
    _plan(e16, 8, heads, nq, nk, "bf16", waves, 1)
    _ragged(e16, nq, nk, D, heads, _counts(nk, (64,)), "bf16", BF16_BAR, "bf16 d=64")


def test_bf16_widened_onto_the_flash_kernel_with_the_option_on(e16):
    """attn_bf16 = 0 under attn_d64 = 1: q still arrives pre-scaled (the option, not the kernel, decides), k_attn.hip takes it in log2 units"""
    nq, heads = GRIDS["medium"]
    try:
        e16.set_option("attn_bf16", 0)
        assert e16.attention_plan(8, heads, nq, 300, D)["kernel"] == "flash"
    finally:
        e16.set_option("attn_bf16", 1)
    _ragged(e16, nq, 300, D, heads, _counts(300, (64,)), "bf16", BF16_BAR, "bf16 d=64 widened", attn_bf16=0)


# ---- the gate leaks nothing ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
def test_option_off_is_a_context_without_it(e32, e16, precision):
    sd = e16 if precision else e32
    fresh = _engine(precision, False)
    try:
        for grid, nk in (("small", NK32), ("medium", 300), ("large", 77)):
            nq, heads = GRIDS[grid]
            counts = _counts(nk, (64,))
            q, k, v, kn, vn, _ = _data(nq, nk, D * heads, heads, counts, "bf16" if precision else "f32")
            kv = np.asarray(counts, np.int32)
            assert fresh.attention_plan(8, heads, nq, nk, D)["kernel"] == "flash"
            want = fresh.qkv_attention_ragged(q, kn, vn, kv, heads)
            want_full = fresh.qkv_attention(q, k, v, None, heads)
            on = sd.qkv_attention(q, k, v, None, heads)
            try:
                sd.set_option("attn_d64", 0)
                assert sd.attention_plan(8, heads, nq, nk, D) == fresh.attention_plan(8, heads, nq, nk, D)
                np.testing.assert_array_equal(sd.qkv_attention_ragged(q, kn, vn, kv, heads), want)
                np.testing.assert_array_equal(sd.qkv_attention(q, k, v, None, heads), want_full)
            finally:
                sd.set_option("attn_d64", 1)
            assert sd.attention_plan(8, heads, nq, nk, D)["kernel"] == ("bf16" if precision else "split")
            assert not np.array_equal(on, want_full), "the option changes no bit: the new instance did not run"
        np.testing.assert_array_equal(sd.qkv_attention(q, k, v, None, heads), on)      # and back on: the same bits as before
    finally:
        fresh.close()
