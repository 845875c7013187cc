"""qkv_attention at the full-width shapes of an SD 2.x UNet on a 64 x 64 latent -- 5, 10, 20 and 20 heads of width 64 over 4096, 1024, 256 and 64 tokens,
self attention and the 77-token context, CFG batch 2 -- on the d = 64 instances of k_attn_split.hip / k_attn_bf16.hip (option attn_d64), by the pattern of
tests/test_model_shapes_gpu.py: operands on the storage type's grid, the fp64 reference at sampled query rows (tests/sampled_ref.py), that file's bars, and the
route with the option off (k_attn.hip, the yardstick) within two bars of the new one at every element."""
import functools
import zlib

import numpy as np
import pytest

import model_shapes as M
import sampled_ref as S
from test_model_shapes_gpu import ATTN16_BAR, FP32_BAR, _check, _check_everywhere, _fmt, _grid

pytestmark = pytest.mark.gpu

D = 64
LEVELS = [(4096, 5), (1024, 10), (256, 20), (64, 20)]
SHAPES = [M.Attention(2, nq, nk, D * heads, heads) for nq, heads in LEVELS for nk in (nq, 77)]
PARAMS = [(p, a) for p in (0, 1) for a in SHAPES]


@pytest.fixture(scope="module")
def engines():
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=precision))
            made[precision].set_option("attn_d64", 1)
        return made[precision]
    yield get
    for sd in made.values():
        sd.close()


@functools.lru_cache(maxsize=2)
def _case(precision, a):
    g = np.random.default_rng(zlib.crc32(repr(("attention d64", tuple(a))).encode()))
    q, k, v = (_grid(g.standard_normal((a.n, s, a.c)), _fmt(precision), 2) for s in (a.nq, a.nk, a.nk))
    rs = S.sample_rows(a.n, a.nq, seed=a.nq + a.nk)
    return q, k, v, rs, S.attention_at(q, k, v, rs, a.heads)


@pytest.mark.parametrize("case", PARAMS, ids=lambda c: f"p{c[0]}-nq{c[1].nq}-nk{c[1].nk}-h{c[1].heads}")
def test_attention_sd2_shape(engines, case):
    precision, a = case
    sd = engines(precision)
    q, k, v, rs, ref = _case(precision, a)
    bar = FP32_BAR if precision == 0 else ATTN16_BAR
    what = f"precision {precision} attention {tuple(a)}"
    plan = sd.attention_plan(a.n, a.heads, a.nq, a.nk, D)
    assert plan["kernel"] == ("bf16" if precision else "split") and plan["kv_tile"] == 64 and plan["q_rows"] == 32 * plan["waves"], plan
    new = sd.qkv_attention(q, k, v, None, a.heads)
    _check(new.reshape(a.n * a.nq, a.c)[rs], ref, f"{what}, {plan}", bar)
    try:
        sd.set_option("attn_d64", 0)
        assert sd.attention_plan(a.n, a.heads, a.nq, a.nk, D)["kernel"] == "flash"
        old = sd.qkv_attention(q, k, v, None, a.heads)
    finally:
        sd.set_option("attn_d64", 1)
    _check(old.reshape(a.n * a.nq, a.c)[rs], ref, f"{what}, option off", bar)
    _check_everywhere(new, old, ref, what, bar)
