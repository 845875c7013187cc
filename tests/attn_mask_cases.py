"""The shapes of tests/test_attention_mask_gpu.py, one table for two readers: the GPU tests run them, and tests/test_attn_plan_cpu.py
replays the planner (csrc/attn_plan.cpp, host only) over the same list and compares with tests/golden/attn_plan_masked_cases.txt, so
that a shape which stopped reaching its k_attn.hip instance -- an "8-wave" case planned 4-wave, say -- fails on a CPU instead of
leaving a GPU test green and vacuous.

A case is (d_head, n, n_head, nq, nk); its channel count is d_head * n_head.  `waves` is what the planner's rule for k_attn.hip
(plan_flash: 8-wave workgroups of 128 query rows once 2 * ceil(nq / 128) * n * n_head >= 3 * 256, else 4-wave ones of 64) gives; a
masked call always has kv_splits = 1."""
from collections import namedtuple

Case = namedtuple("Case", "d n heads nq nk")

KV_TILE = {40: 64, 64: 64, 80: 64, 160: 32}   # keys per K / V tile of k_attn.hip (kAttnGeom, csrc/attn_plan.hpp)
ROWS_PER_WAVE = 16

# 4-wave instances: n = 2 and 2 heads (a batch or head offset wrongly applied to the shared mask shows); nq = 1, 77, 130 is one ragged
# workgroup, two, and three with 2 rows in the last; nk is below one tile, a ragged second tile, and a third tile of 2 keys
# (d = 160 walks 32-key tiles: 37 and 77 are a ragged second and third tile)
WAVE4 = [Case(d, 2, 2, nq, nk) for d in (40, 64, 80) for nq in (1, 77, 130) for nk in (2, 77, 130)] + \
        [Case(160, 2, 2, nq, nk) for nq in (1, 77, 130) for nk in (37, 77)]

# 8-wave instances: many samples rather than long sequences.  d = 64 is CLIP's own shape at 32 chunks of 77 tokens; d = 40 has two
# workgroups per (sample, head), the second with 2 live rows
WAVE8 = [Case(40, 48, 8, 130, 77), Case(64, 32, 12, 77, 77), Case(80, 48, 8, 100, 77), Case(160, 48, 8, 100, 77)]

# the reduced-precision contexts run one 4-wave case per head dim, and d = 64 in both forms; the same q, k, v without the mask go to
# the bf16 route there (listed in the fixture as "bf16" lines)
REDUCED = [Case(40, 2, 2, 130, 77), Case(64, 2, 2, 130, 77), Case(80, 2, 2, 130, 77), Case(160, 2, 2, 130, 77), Case(64, 32, 12, 77, 77)]

# the tiny CLIP of tests/test_clip_gpu.py (one head of 64) at n = 384 chunks of T = 16
CLIP_TINY = Case(64, 384, 1, 16, 16)

MASKED = WAVE4 + WAVE8 + [CLIP_TINY]          # REDUCED's masked calls are a subset of WAVE4 + WAVE8
UNMASKED_BF16 = REDUCED


def waves(c):
    """plan_flash's rule, restated"""
    return 8 if 2 * ((c.nq + 127) // 128) * c.n * c.heads >= 3 * 256 else 4


def case_id(c):
    return f"d{c.d}-n{c.n}-h{c.heads}-q{c.nq}-k{c.nk}"


def plan_header(c, masked):
    """the part of a fixture line before the colon, in tests/san/attn_plan_main.cpp's format"""
    return f"{'f32 mask' if masked else 'bf16'} d{c.d} n{c.n} h{c.heads} q{c.nq} k{c.nk}"
