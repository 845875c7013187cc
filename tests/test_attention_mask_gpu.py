"""qkv_attention with an additive mask -- the eight masked instances of csrc/k_attn.hip (head dims 40, 64, 80, 160, each as a 4-wave and an
8-wave workgroup), reached through sdmi_qkv_attention with an arbitrary mask and mask_ld and, for CLIP, through clip.forward -- against
oracle.sd_oracle.qkv_attention in float64.

Bar: the operator bar of tests/test_ops_gpu.py, max|gpu - f64| <= 2e-5 * max(1, max|ref|), in every context: a masked call is fp32 in the
precision = 1 and precision = 2 contexts too (Engine::qkv_attention_dev).

What the masks are made of, and why.  A 0 / -inf mask (tests/test_ops_gpu.py::test_qkv_attention_causal_mask) is the same number in every unit,
and with mask_ld == nk, one sample and a pattern that depends on key <= row only, it cannot tell a wrong unit, stride, row or batch offset from
a right one.  So every mask here is DENSE: each entry an independent draw from [-8, 8], which a dropped or doubled log2(e), nk in place of
mask_ld, a row taken from another workgroup or a sample / head offset moves by orders of magnitude more than the bar.  Laid over it:
  oversized   [nq + 3, nk + 5], the margins filled with 1e3 -- reading them shows; the wrapper hands shape[1] down as mask_ld
  causal      -inf above the diagonal
  banded      row r keeps the 9 keys from (29 r + nk - 1) mod nk on: for many rows the first one or two key tiles are -inf altogether, so the
              running maximum is still -inf when the tile ends (the m_new == -inf guard) and the first live tile rescales from m_run = -inf
  checker     -inf on every second entry, single entries
  bigneg      -1e4 and float32's lowest on about 60 % of the entries -- what other front-ends write for "masked" -- only in rows that keep a key
              with |mask| <= 8 (asserted on the mask): a row whose every key sits at -1e4 loses ~ 5e-4 of its exponents to the fp32 rounding
              of score + mask, which no fp32 kernel could hold the bar against.  A condition on the inputs, not a tolerance
  dead        rows 3, 20, 70, nq - 1 and the whole 16-row wave block 32..47 have every key at -inf: softmax over nothing is 0 / 0, NaN in the
              reference and NaN here (l = 0, o * (1 / 0)); the outputs must be non-finite exactly where the oracle's are
The shapes are tests/attn_mask_cases.py; tests/test_attn_plan_cpu.py pins on a CPU that the planner sends each to the instance meant."""
import functools

import numpy as np
import pytest
import torch

import attn_mask_cases as A
from oracle import clip_oracle as CO
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

pytestmark = pytest.mark.gpu

RTOL = 2e-5   # tests/test_ops_gpu.py
KINDS = ("dense", "oversized", "causal", "banded", "checker", "bigneg", "dead")
OVERSIZED = ("oversized", "banded", "bigneg")


@pytest.fixture(scope="module")
def ops32():
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion(ModelConfig(32, 1, 32, 8, 8, 32))
    yield sd
    sd.close()


@pytest.fixture(scope="module", params=[1, 2])
def ops_reduced(request):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=request.param))
    yield request.param, sd
    sd.close()


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))   # a copy: the shared inputs are read-only


def make_mask(case, kind, g):
    nq, nk = case.nq, case.nk
    rows, keys = np.arange(nq)[:, None], np.arange(nk)[None, :]
    m = np.full((nq + 3, nk + 5) if kind in OVERSIZED else (nq, nk), 1e3, np.float32)
    live = m[:nq, :nk]
    live[...] = g.uniform(-8.0, 8.0, (nq, nk))
    if kind == "causal":
        live[np.broadcast_to(keys > rows, live.shape)] = -np.inf
    elif kind == "banded":
        first = (rows * 29 + nk - 1) % nk
        live[(keys < first) | (keys >= first + 9)] = -np.inf
        tile = A.KV_TILE[case.d]
        if nk > tile:       # some row meets its first live key in a later tile, some in the first
            dead_first = np.isinf(live[:, :tile]).all(axis=1)
            assert dead_first.any() and (nq == 1 or not dead_first.all())
            assert np.isinf(live[0, :tile * ((nk - 1) // tile)]).all()       # row 0: every tile but the last
    elif kind == "checker":
        assert nk >= 2
        live[np.broadcast_to((rows + keys) % 2 == 1, live.shape)] = -np.inf
    elif kind == "bigneg":
        hit = (g.random((nq, nk)) < 0.6) & (keys != (rows * 7) % nk)
        live[hit & ((rows + keys) % 2 == 0)] = -1e4
        live[hit & ((rows + keys) % 2 == 1)] = np.finfo(np.float32).min
        assert (np.abs(live) <= 8).any(axis=1).all(), "every row must keep a key with |mask| <= 8"
    elif kind == "dead":
        dead = sorted(r for r in {3, 20, 70, nq - 1} | set(range(32, 48)) if r < nq)
        live[dead, :] = -np.inf
    if kind != "dead":
        assert np.isfinite(live).any(axis=1).all()
    assert not np.isnan(m).any()
    return m


@functools.lru_cache(maxsize=16)
def _inputs(case, kind):
    """q, k, v as in test_qkv_attention_packed_tail_d40 (v's columns carry different magnitudes), the mask, and the float64 reference -- computed once and
    shared; nobody writes to them"""
    c = case.d * case.heads
    g = np.random.default_rng([case.d, case.n, case.heads, case.nq, case.nk, KINDS.index(kind)])
    q = (g.standard_normal((case.n, case.nq, c)) * 1.5).astype(np.float32)
    k = (g.standard_normal((case.n, case.nk, c)) * 1.5).astype(np.float32)
    v = (g.standard_normal((case.n, case.nk, c)) * np.exp2(g.integers(-4, 5, (1, 1, c))) + np.arange(c, dtype=np.float32) % 7).astype(np.float32)
    mask = make_mask(case, kind, g)
    ref = O.qkv_attention(_t(q), _t(k), _t(v), _t(mask), case.heads).numpy()
    if kind != "dead":
        assert np.isfinite(ref).all()
    else:
        assert not np.isfinite(ref).all()
    for a in (q, k, v, mask, ref):
        a.setflags(write=False)
    return q, k, v, mask, ref


def _check(got, ref, what):
    """the bar on every entry the oracle has a number for; non-finite exactly where the oracle is (NaN rows of a dead-row mask, nowhere otherwise)"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    ok = np.isfinite(ref)
    bad = np.isfinite(got) != ok
    assert not bad.any(), f"{what}: {int(bad.sum())} entries finite on one side only, first at {tuple(int(i) for i in np.argwhere(bad)[0])} (rows {sorted({int(r) for r in np.argwhere(bad)[:, 1]})[:8]})"
    err = np.where(ok, np.abs(got - np.where(ok, ref, 0.0)), 0.0)
    bound = RTOL * max(1.0, float(np.abs(ref[ok]).max()) if ok.any() else 1.0)
    idx = np.unravel_index(int(err.argmax()), err.shape)
    print(f"RATIO {what}: max|d| / bound = {err.max() / bound:.3f}")
    assert err.max() <= bound, f"{what}: max|d|={err.max():.3e} > {bound:.3e} at {idx} (got {got[idx]:.6f}, ref {ref[idx]:.6f}); mean|d|={err.mean():.3e}"


def _both_routes(ops32, case, kind):
    """the call with option gemm_planes at its default (where the channel count allows: the kernel's plane-writing epilogue, joined back) and at 0 (plain fp32
    stores): the join is exact, so the two agree bit for bit"""
    q, k, v, mask, ref = _inputs(case, kind)
    what = f"d{case.d} w{A.waves(case)} {A.case_id(case)} {kind}"
    try:
        got = ops32.qkv_attention(q, k, v, mask, case.heads)
        ops32.set_option("gemm_planes", 0)
        plain = ops32.qkv_attention(q, k, v, mask, case.heads)
    finally:
        ops32.set_option("gemm_planes", "default")
    np.testing.assert_array_equal(got, plain, err_msg=f"{what}: gemm_planes default vs 0")
    _check(got, ref, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", A.WAVE4, ids=A.case_id)
def test_masked_attention_4wave(ops32, case, kind):
    _both_routes(ops32, case, kind)


@pytest.mark.parametrize("kind", ["banded", "dead"])
@pytest.mark.parametrize("case", A.WAVE8, ids=A.case_id)
def test_masked_attention_8wave(ops32, case, kind):
    _both_routes(ops32, case, kind)


@pytest.mark.parametrize("case", A.REDUCED, ids=A.case_id)
def test_masked_attention_stays_fp32_in_reduced_precision(ops_reduced, case):
    """In a precision = 1 or 2 context the masked call must stay on the fp32 kernel (un-rounded fp32 inputs, the fp32 bar), while the same q, k, v without the
    mask go through bf16 storage -- further than the bar from the float64 reference, which shows the masked call took another route and that the context
    does not run fp32 throughout."""
    precision, ops = ops_reduced
    q, k, v, mask, ref = _inputs(case, "banded")
    _check(ops.qkv_attention(q, k, v, mask, case.heads), ref, f"d{case.d} w{A.waves(case)} {A.case_id(case)} banded precision={precision}")
    if precision == 1:
        plain = ops.qkv_attention(q, k, v, None, case.heads)
        ref0 = O.qkv_attention(_t(q), _t(k), _t(v), None, case.heads).numpy()
        assert np.isfinite(plain).all()
        assert np.abs(plain - ref0).max() > RTOL * max(1.0, np.abs(ref0).max())


def test_masked_attention_refusals(ops32):
    """A mask narrower than nk (the library: mask_ld < nk), a mask on a head dim without a fused kernel (the planner), and a mask with fewer than nq rows (the
    Python wrapper -- the library reads nq rows of mask_ld floats and cannot see where the array ends) each raise SdmiError, and the engine goes on working."""
    from stable_diffusion_burn_amd import SdmiError
    case = A.Case(40, 2, 2, 77, 77)
    q, k, v, mask, ref = _inputs(case, "dense")
    good = ops32.qkv_attention(q, k, v, mask, case.heads)
    _check(good, ref, "before the refusals")
    g = np.random.default_rng(128)
    q1, k1, v1 = (g.standard_normal((1, 64, 128)).astype(np.float32) for _ in range(3))
    refused = [
        ("narrow", lambda: ops32.qkv_attention(q, k, v, mask[:, :case.nk - 1], case.heads), -1),
        ("unfused", lambda: ops32.qkv_attention(q1, k1, v1, mask[:64, :64], 1), -5),
        ("short", lambda: ops32.qkv_attention(q, k, v, mask[:case.nq - 1], case.heads), -1),
        ("flat", lambda: ops32.qkv_attention(q, k, v, mask.reshape(-1), case.heads), -1),
    ]
    for what, call, status in refused:
        with pytest.raises(SdmiError) as e:
            call()
        assert e.value.status == status, (what, str(e.value))
        np.testing.assert_array_equal(ops32.qkv_attention(q, k, v, mask, case.heads), good, err_msg=f"after {what}")
    np.testing.assert_array_equal(ops32.qkv_attention(q1, k1, v1, None, 1).shape, q1.shape)    # d = 128 without a mask is served (unfused)


def test_clip_forward_8wave():
    """clip.forward end to end where its causal-mask attention is planned 8-wave: the tiny CLIP of tests/test_clip_gpu.py (one head of 64) at n = 384 chunks
    of T = 16 (tests/attn_mask_cases.py CLIP_TINY), against oracle/clip_oracle.py in float64 at that file's bar."""
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    from test_clip_gpu import MINI_VOCAB, TINY
    c = A.CLIP_TINY
    assert (TINY.n_state, TINY.n_head, TINY.n_ctx) == (c.d * c.heads, c.heads, c.nq) and c.nq == c.nk
    tokens = np.random.default_rng(384).integers(0, MINI_VOCAB, (c.n, c.nq)).astype(np.int32)
    ref = CO.CLIPOracle(syn.SyntheticWeights(), TINY, torch.float64).forward(tokens).numpy()
    sd = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, clip_layers=2, clip_heads=1, clip_vocab=MINI_VOCAB, clip_ctx=16))
    try:
        sd.load_weights(syn.SyntheticWeights(), vae_encoder=False)
        got = sd.clip.forward(tokens)
    finally:
        sd.close()
    assert np.isfinite(ref).all()
    _check(got, ref, f"d64 w8 clip tiny n={c.n} T={c.nq}")
