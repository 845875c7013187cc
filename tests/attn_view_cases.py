"""The layouts, case table, data and reference of tests/test_attention_views_gpu.py, one module for two readers: the GPU tests run the table through
sdmi_op_qkv_attention_view, and tests/test_attention_views_cpu.py replays the planner and the view validator (csrc/attn_plan.cpp, host only) over the
same table, so that a row which stopped reaching the kernel form it names -- or a layout the entry would refuse -- fails on a CPU.

A LAYOUT says where the engine puts q, k, v and the result: a Slice is the columns [off, off + C) of a parent [n][rows][ld], ld elements between rows and
rows * ld between samples.  g is 16 bytes of the storage type (4 fp32 / 8 bf16 elements): the smallest gap the kernels' 16-byte loads allow.

A ROW of the table is (precision, kernel, workgroup form, shape, engine options); the shapes are those of tests/test_attention_ragged_gpu.py, so nothing
is new but the layout.  `kernel`, `waves` and `q_rows` are what sdmi_attention_plan must answer for the row under its options; `slices` the key-slice count
at the row's own nk and, where the row also runs as self attention (layout model_self: nk = nq), there."""
import functools
import zlib
from collections import namedtuple

import numpy as np

Slice = namedtuple("Slice", "ld off rows")
Layout = namedtuple("Layout", "name q k v packed out")


def gap(es):
    """elements in 16 bytes"""
    return 16 // es


def dense(nq, nk, c, es):
    """the identity: the entry must then BE sdmi_qkv_attention / sdmi_op_qkv_attention_ragged"""
    return Layout("dense", Slice(c, 0, nq), Slice(c, 0, nk), Slice(c, 0, nk), False, Slice(c, 0, nq))


def model_self(nq, nk, c, es):
    """the UNet's / CLIP's self-attention buffer exactly: one GEMM wrote [n][T][3C], q | k | v side by side, no padding anywhere; a dense result"""
    assert nq == nk
    return Layout("model_self", Slice(3 * c, 0, nq), Slice(3 * c, c, nq), Slice(3 * c, 2 * c, nq), True, Slice(c, 0, nq))


def packed_gaps(nq, nk, c, es):
    """one parent with a 16-byte gap in front of each slice and 5 rows of filler behind each sample: the batch stride is not rows_used * ld"""
    g = gap(es)
    ld, rows = 3 * c + 3 * g, max(nq, nk) + 5
    return Layout("packed_gaps", Slice(ld, g, rows), Slice(ld, c + 2 * g, rows), Slice(ld, 2 * c + 3 * g, rows), True, Slice(c + 2 * g, g, nq + 3))


def apart(nq, nk, c, es):
    """three parents and the output's: pairwise different row strides, offsets and rows per sample -- no two of the eight strides (four between rows, four
    between samples) are equal, so a kernel that took one for another moves data"""
    g = gap(es)
    return Layout("apart", Slice(c + g, 0, nq + 1), Slice(c + 2 * g, 2 * g, nk + 2), Slice(c + 3 * g, g, nk + 3), False, Slice(c + 4 * g, g, nq + 2))


LAYOUTS = {"dense": dense, "model_self": model_self, "packed_gaps": packed_gaps, "apart": apart}


def strides(lay):
    """the eight strides Engine::attention is handed"""
    return [s.ld for s in (lay.q, lay.k, lay.v, lay.out)] + [s.ld * s.rows for s in (lay.q, lay.k, lay.v, lay.out)]


# ---- numpy model of the scatter the entry makes (tests/test_attention_views_cpu.py: round trip, no overlap, filler everywhere else) ------------------------
def scatter(lay, q, k, v, fill=np.nan):
    """-> the parents {"q": .., "k": .., "v": ..} ([n][rows][ld]; one shared array when packed) with the operands in their slices and `fill` elsewhere"""
    n = q.shape[0]
    if lay.packed:
        par = np.full((n, lay.q.rows, lay.q.ld), fill, np.float32)
        parents = {"q": par, "k": par, "v": par}
    else:
        parents = {w: np.full((n, s.rows, s.ld), fill, np.float32) for w, s in (("q", lay.q), ("k", lay.k), ("v", lay.v))}
    for w, s, x in (("q", lay.q, q), ("k", lay.k, k), ("v", lay.v, v)):
        parents[w][:, :x.shape[1], s.off:s.off + x.shape[2]] = x
    return parents


def gather(lay, parents, nq, nk, c):
    return tuple(parents[w][:, :r, s.off:s.off + c].copy() for w, s, r in (("q", lay.q, nq), ("k", lay.k, nk), ("v", lay.v, nk)))


def cover(lay, n, nq, nk, c):
    """per parent, how many slices claim each cell (0: filler, 1: operand data, 2: an overlap)"""
    if lay.packed:
        cnt = np.zeros((n, lay.q.rows, lay.q.ld), np.int32)
        counts = {"q": cnt, "k": cnt, "v": cnt}
    else:
        counts = {w: np.zeros((n, s.rows, s.ld), np.int32) for w, s in (("q", lay.q), ("k", lay.k), ("v", lay.v))}
    for w, s, r in (("q", lay.q, nq), ("k", lay.k, nk), ("v", lay.v, nk)):
        counts[w][:, :r, s.off:s.off + c] += 1
    return counts


def out_slice(lay, parent, nq, c):
    return parent[:, :nq, lay.out.off:lay.out.off + c]


def prefill(lay, n, bf16):
    """the output parent before the call: a value that differs from cell to cell and that no attention result takes (below -1 where v is N(0, <= 8));
    on the bf16 grid where the parent is stored as bf16"""
    size = n * lay.out.rows * lay.out.ld
    a = -(2.0 + (np.arange(size, dtype=np.int64) % 65521).astype(np.float64) / 128.0)
    a = a.astype(np.float32).reshape(n, lay.out.rows, lay.out.ld)
    return bf16_round(a) if bf16 else a


def bf16_round(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


# ---- the case table -------------------------------------------------------------------------------------------------------------------------------------------
# opts: engine options of the row (restored to OPTION_DEFAULTS afterwards).  mask: None / "banded" (finite values, -inf above a shifted diagonal) / "causal".
# planes = 1: the plane-writing epilogue (out_planes = 1, a dense output, option gemm_planes = 1 for the dense entry); 0: rows, gemm_planes = 0.
# kv_len: the row runs with per-sample key counts (n = their number) under layout `apart` only.  layouts: the layouts the row runs under.
Row = namedtuple("Row", "id precision kernel waves q_rows slices d n heads nq nk opts mask planes kv_len layouts")

OPTION_DEFAULTS = {"attn_split": 1, "attn_kv_splits": 0, "attn_pack_tail": "default", "gemm_planes": "default", "attn_bf16": 1, "attn_bf16_variant": "default",
                   "attn_d64": 0}
PLAN_DEFAULTS = {"attn_split": 1, "attn_bf16": 1, "attn_bf16_variant": 7, "attn_pack_tail": 3, "attn_kv_splits": 0, "attn_kv_prefer8": 1, "attn_d64": 0}   # AttnPlanOpts

NK = 8 * 64 + 8                                            # test_attention_ragged_gpu.NK32: 9 key tiles of 64 (17 of 32)
GRIDS = {"small": (2, 100, 2), "large": (8, 2085, 4)}      # n, query rows, heads: 4-wave (2-wave bf16) forms / the 8-wave forms of all three kernels
FUSED = ("model_self", "packed_gaps", "apart")
ROWS_PER_WAVE = {"flash": 16, "split": 32, "bf16": 32}


def _fused(rid, precision, kernel, grid, d, waves, slices, opts=None, mask=None, planes=0, qr=1, layouts=FUSED):
    n, nq, heads = GRIDS[grid]
    return Row(f"{rid}-{grid}", precision, kernel, waves, ROWS_PER_WAVE[kernel] * waves * qr, slices, d, n, heads, nq, NK, opts or {}, mask, planes, False, layouts)


def _ragged(rid, precision, kernel, d, waves, slices, tiles, opts=None):
    """the small grid with the ragged test's key counts: 8 samples"""
    return Row(f"{rid}-kv_len", precision, kernel, waves, ROWS_PER_WAVE[kernel] * waves, slices, d, 8, 2, 100, NK, opts or {}, None, 0, tiles, ("apart",))


# precision 0.  slices = (at nk = NK, at nk = nq): the planner's rule -- on the small grid the automatic count fills the CUs (4 slices, 8 of d = 160's 32-key
# tiles) as long as a slice keeps two key tiles; as self attention over 100 keys there are 2 tiles (4 at d = 160)
FP32 = [
    # k_attn_split.hip: d = 40 with and without the packed tail / log2 softmax, d = 80, d = 64 behind attn_d64
    _fused("split-d40-pack3", 0, "split", "small", 40, 4, (4, 1), {"attn_split": 1, "attn_pack_tail": 3}),
    _fused("split-d40-pack3", 0, "split", "large", 40, 8, (1, 1), {"attn_split": 1, "attn_pack_tail": 3}),
    _fused("split-d40-pack0", 0, "split", "small", 40, 4, (4, 1), {"attn_split": 1, "attn_pack_tail": 0}),
    _fused("split-d40-pack0", 0, "split", "large", 40, 8, (1, 1), {"attn_split": 1, "attn_pack_tail": 0}),
    _fused("split-d80", 0, "split", "small", 80, 4, (4, 1), {"attn_split": 1}),
    _fused("split-d80", 0, "split", "large", 80, 8, (1, 1), {"attn_split": 1}),
    _fused("split-d64", 0, "split", "small", 64, 4, (4, 1), {"attn_d64": 1}),
    _fused("split-d64", 0, "split", "large", 64, 8, (1, 1), {"attn_d64": 1}),
    # k_attn.hip: attn_split = 0 at d = 40 / 80, always at d = 160
    _fused("flash-d40", 0, "flash", "small", 40, 4, (4, 1), {"attn_split": 0}),
    _fused("flash-d40", 0, "flash", "large", 40, 8, (1, 1), {"attn_split": 0}),
    _fused("flash-d80", 0, "flash", "small", 80, 4, (4, 1), {"attn_split": 0}),
    _fused("flash-d80", 0, "flash", "large", 80, 8, (1, 1), {"attn_split": 0}),
    _fused("flash-d160", 0, "flash", "small", 160, 4, (8, 2)),
    _fused("flash-d160", 0, "flash", "large", 160, 8, (1, 1)),
    # forced key slices: the partial results and the merge launch, which writes through out_ld (packed_gaps, apart)
    _fused("split-d40-slices3", 0, "split", "small", 40, 4, (3, 2), {"attn_kv_splits": 3}),
    _fused("split-d40-slices8", 0, "split", "large", 40, 8, (8, 8), {"attn_kv_splits": 8}),
    _fused("flash-d160-slices3", 0, "flash", "small", 160, 4, (3, 3), {"attn_kv_splits": 3}),
    _fused("flash-d40-slices8", 0, "flash", "small", 40, 4, (8, 2), {"attn_split": 0, "attn_kv_splits": 8}),
    # the plane-writing epilogue (a dense output, channel counts that are multiples of 32); gemm_planes = 0 is every other row
    _fused("split-d40-planes", 0, "split", "large", 40, 8, (1, 1), {"attn_split": 1}, planes=1),
    _fused("split-d80-planes", 0, "split", "small", 80, 4, (4, 1), {"attn_split": 1}, planes=1),
    _fused("flash-d160-planes", 0, "flash", "small", 160, 4, (8, 2), planes=1),
    # the HAS_MASK instance of k_attn.hip (a mask keeps d = 40 off k_attn_split.hip and the keys in one slice)
    _fused("flash-d40-mask", 0, "flash", "small", 40, 4, (1, 1), mask="banded"),
]
# CLIP's own layer: n = 2 chunks of T = 77 tokens, 768 channels in 12 heads, the causal mask, q | k | v out of one GEMM
CLIP = [Row(f"clip-p{p}", p, "flash", 4, 64, (1, 1), 64, 2, 12, 77, 77, {}, "causal", 0, False, ("model_self",)) for p in (0, 1)]
# the unfused path (QK^T -> row softmax -> PV on the GEMM kernels, one (sample, head) at a time): a_ld, b_ld, transpose2d's src_ld, the output's ldc
UNFUSED = [
    Row("unfused-d128", 0, "unfused", 0, 0, (1, 1), 128, 2, 1, 64, 64, {}, None, 0, False, ("apart", "model_self")),
    Row("unfused-d512", 0, "unfused", 0, 0, (1, 1), 512, 2, 1, 256, 256, {}, None, 0, False, ("apart", "model_self")),
    Row("unfused-d512-bf16", 1, "unfused", 0, 0, (1, 1), 512, 2, 1, 256, 256, {}, None, 0, False, ("apart", "model_self")),
]


def _bf16_rows():
    """k_attn_bf16.hip at d = 40 / 80 / 160 under attn_bf16_variant default (7), 1, 0x102, 0x104.  What each reaches at 520 (or nq) keys: the small grid's 4
    workgroups get the 2-wave form, the large grid's 288 workgroups of 256 rows the 8-wave one; bit 0 and the unforced bits 1 / 2 are forms for short contexts or
    grids that fill the chip, which these are not; 0x102 / 0x104 force d = 40's 64-rows-per-wave forms on 8 / 4 waves whatever the grid"""
    rows = []
    for d in (40, 80, 160):
        for variant in ("default", 1, 0x102, 0x104):
            for grid, waves in (("small", 2), ("large", 8)):
                w, qr = waves, 1
                if d == 40 and variant == 0x102:
                    w, qr = 8, 2
                if d == 40 and variant == 0x104:
                    w, qr = 4, 2
                name = variant if isinstance(variant, str) else hex(variant)
                rows.append(_fused(f"bf16-d{d}-variant-{name}", 1, "bf16", grid, d, w, (1, 1), {"attn_bf16_variant": variant}, qr=qr))
    return rows


BF16 = _bf16_rows()
# per-sample key counts (test_attention_ragged_gpu._counts: 1, 2, tile - 1 / tile / tile + 1, 77, nk; NaN behind each) under `apart`: one row per kernel
RAGGED = [
    _ragged("split-d40", 0, "split", 40, 4, (4, 1), (64,)),
    _ragged("flash-d160", 0, "flash", 160, 4, (8, 2), (32,)),
    _ragged("bf16-d80", 1, "bf16", 80, 2, (1, 1), (64,)),
    Row("unfused-d128-kv_len", 0, "unfused", 0, 0, (1, 1), 128, 8, 1, 100, 256, {}, None, 0, "unfused", ("apart",)),
    Row("unfused-d128-bf16-kv_len", 1, "unfused", 0, 0, (1, 1), 128, 8, 1, 100, 320, {}, None, 0, "unfused", ("apart",)),
]
ROWS = FP32 + CLIP + UNFUSED + BF16 + RAGGED
DENSE = ["split-d40-pack3-small", "flash-d160-small", "bf16-d80-variant-default-small", "unfused-d128", "split-d40-kv_len", "flash-d40-mask-small"]   # layout `dense`: one per kernel

BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def storage_bf16(row):
    """the storage type the call runs in: bf16 at precision >= 1, except under a mask (the masked kernels are fp32 at every precision)"""
    return row.precision >= 1 and row.mask is None


def elem_size(row):
    return 2 if storage_bf16(row) else 4


def shape(row, layout):
    """(nq, nk) of the row under a layout: model_self is self attention over the row's queries"""
    return (row.nq, row.nq) if layout == "model_self" else (row.nq, row.nk)


def expected_slices(row, layout):
    return row.slices[1 if layout == "model_self" and row.nq != row.nk else 0]


def layout_of(row, layout):
    nq, nk = shape(row, layout)
    lay = LAYOUTS[layout](nq, nk, row.d * row.heads, elem_size(row))
    if row.planes:      # the plane output is dense
        lay = lay._replace(out=Slice(row.d * row.heads, 0, nq))
    return lay


def cases():
    """every (row, layout) the GPU test runs, ordered so that cases sharing data and reference follow each other"""
    out = [(r, lay) for r in ROWS for lay in r.layouts] + [(BY_ID[i], "dense") for i in DENSE]
    return sorted(out, key=lambda rl: (rl[0].precision, rl[0].d * rl[0].heads, rl[0].n, shape(rl[0], rl[1]), str(rl[0].mask), str(rl[0].kv_len)))


def case_id(row, layout):
    return f"{row.id}-{layout}"


def kv_counts(row):
    """the row's per-sample key counts, or None"""
    if not row.kv_len:
        return None
    from test_attention_ragged_gpu import UNFUSED_COUNTS, _counts
    counts = UNFUSED_COUNTS[1 if row.precision else 0] if row.kv_len == "unfused" else _counts(row.nk, row.kv_len)
    assert len(counts) == row.n and max(counts) == row.nk
    return counts


def make_mask(kind, nq, nk):
    if kind is None:
        return None
    j, i = np.arange(nk)[None, :], np.arange(nq)[:, None]
    if kind == "causal":
        return np.where(j <= i, 0.0, -np.inf).astype(np.float32)
    g = np.random.default_rng(nq * 1000 + nk)
    m = (2.0 * g.standard_normal((nq, nk))).astype(np.float32)
    m[j > i + (nk - nq) + 3] = -np.inf       # every row keeps live keys
    return m


@functools.lru_cache(maxsize=2)
def data(n, nq, nk, c, heads, counts, fmt, mask_kind):
    """q, k, v as test_attention_ragged_gpu._data makes them (N(0, 1) q and k, v with per-column powers of two; fmt 'bf16': on the bf16 grid), kn / vn = k / v with NaN
    behind every sample's count, the mask, and oracle.sd_oracle.qkv_attention in float64 on each sample's own keys.  Read-only: shared between cases."""
    import torch
    from oracle import sd_oracle as O
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    g = np.random.default_rng(zlib.crc32(repr((n, nq, nk, c, heads, fmt)).encode()))
    q = g.standard_normal((n, nq, c)).astype(np.float32)
    k = g.standard_normal((n, nk, c)).astype(np.float32)
    v = (g.standard_normal((n, nk, c)) * np.exp2(g.integers(-3, 4, (1, 1, c)))).astype(np.float32)   # a column mixed up with another shows
    if fmt == "bf16":
        q, k, v = bf16_round(q), bf16_round(k), bf16_round(v)
    mask = make_mask(mask_kind, nq, nk)
    kn, vn = (k.copy(), v.copy()) if counts else (k, v)
    ref = np.empty((n, nq, c))
    for b in range(n):
        L = counts[b] if counts else nk
        if counts:
            kn[b, L:] = np.nan
            vn[b, L:] = np.nan
        ref[b] = O.qkv_attention(t(q[b:b + 1]), t(k[b:b + 1, :L]), t(v[b:b + 1, :L]), None if mask is None else t(mask), heads)[0].numpy()
    for a in (q, k, v, kn, vn, ref) + (() if mask is None else (mask,)):
        a.setflags(write=False)
    return q, k, v, kn, vn, mask, ref


def case_data(row, layout):
    nq, nk = shape(row, layout)
    return data(row.n, nq, nk, row.d * row.heads, row.heads, kv_counts(row), "bf16" if row.precision else "f32", row.mask)


# ---- what the entry must refuse (SDMI_ERR_INVALID on the host): (name, layout) at nq = 100, nk = 520, C = 80, for either element size -----------------------
def refusals(nq, nk, c, es):
    g = gap(es)
    ok = apart(nq, nk, c, es)
    pk = packed_gaps(nq, nk, c, es)
    return [
        ("q ld < off + n_state", ok._replace(q=ok.q._replace(off=2 * g))),
        ("k ld < n_state", ok._replace(k=Slice(c - g, 0, nk))),
        ("v negative off", ok._replace(v=ok.v._replace(off=-g))),
        ("q rows too small", ok._replace(q=ok.q._replace(rows=nq - 1))),
        ("k rows too small", ok._replace(k=ok.k._replace(rows=nk - 1))),
        ("v rows too small", ok._replace(v=ok.v._replace(rows=nk - 1))),
        ("packed q and k overlap", pk._replace(k=pk.k._replace(off=pk.q.off + c - g))),
        ("packed k and v overlap", pk._replace(v=pk.v._replace(off=pk.k.off))),
        ("packed with different ld", pk._replace(k=pk.k._replace(ld=pk.k.ld + g))),
        ("packed with different rows", pk._replace(v=pk.v._replace(rows=pk.v.rows + 1))),
        ("output leaves its parent", ok._replace(out=ok.out._replace(off=ok.out.ld - c + g))),
        ("output rows too small", ok._replace(out=ok.out._replace(rows=nq - 1))),
        ("q ld off a 16-byte multiple", ok._replace(q=ok.q._replace(ld=ok.q.ld + g // 2))),
        ("k off off a 16-byte multiple", ok._replace(k=ok.k._replace(off=g // 2))),
        ("v ld off a 16-byte multiple", ok._replace(v=ok.v._replace(ld=ok.v.ld + 1))),
        ("output off off a 16-byte multiple", ok._replace(out=ok.out._replace(off=g // 2))),
        ("output ld off a 16-byte multiple", ok._replace(out=ok.out._replace(ld=ok.out.ld + g // 2))),
    ]


PLANES_REFUSALS = ["strided plane output"]    # out_planes = 1 with layout `apart`'s output


# ---- lines for tests/san/attn_plan_main.cpp --views (tests/test_attention_views_cpu.py) ---------------------------------------------------------------------------
def plan_line(row, layout):
    nq, nk = shape(row, layout)
    o = dict(PLAN_DEFAULTS)
    for key, val in row.opts.items():
        if key in o and val != "default":
            o[key] = val
    return (f"plan {int(storage_bf16(row))} {int(row.mask is not None)} {row.planes} {row.d} {row.n} {row.heads} {nq} {nk} "
            f"{o['attn_split']} {o['attn_bf16']} {o['attn_bf16_variant']} {o['attn_pack_tail']} {o['attn_kv_splits']} {o['attn_kv_prefer8']} {o['attn_d64']}")


def view_line(lay, n, nq, nk, c, es, planes=0):
    s = " ".join(f"{x.ld} {x.off} {x.rows}" for x in (lay.q, lay.k, lay.v, lay.out))
    return f"view {int(es == 2)} {n} {nq} {nk} {c} {int(lay.packed)} {s} {planes}"
