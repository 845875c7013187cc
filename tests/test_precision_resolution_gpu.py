"""The low-order bf16 planes of the fp32 split arithmetic, on the device: k_gemm3x.hip (tiles 200 + x), k_gemm3p.hip (tiles 300 + x) and k_attn_split.hip under the
probes of tests/precision_probes.py -- inputs that resolve 2^-17 of a product, where the operator bars (2e-5 max|ref|) cannot tell a kernel that keeps six partial
products from one that keeps three.  tests/test_precision_probes_cpu.py proves on the CPU that every probe detects every mutation (a product deleted, the l plane shifted
by one k position or one row, V_m and V_l exchanged) and that each ratio bar lies 2 x below them.  The contract under test: include/sdmi.h ("fp32 semantics of
precision 0"), DESIGN.md section 4a.  Reference arithmetic: Burn's Conv2d / Linear (unet/mod.rs:397-729) and qkv_attention (attention.rs:5-45), plain fp32.

1. EXACT probes -- one-hot weights, every output ONE product that fp32 holds exactly; got == float32(fp64 reference), bit for bit.  Family A (x 24 bits, w +-2^e) needs
   x_m w_h and x_l w_h; B (x +-2^e, w 24 bits) needs x_h w_m, x_h w_l and the weight-plane packers, both b3_grouped layouts; C (12 x 11 bits) needs h m, m h and m m.
   One sample of 17 x 19 pixels (323 rows), cout 336; 1x1 at cin 32 (one k tile) and 64, 3x3 at cin 64 (stride 1, stride 2, upsample2x), weight sets that select every
   k position; Linear 323 x {32, 64} -> 336.  Tiles 200-205 x gemm3x_variant {0, 1, 2, 6} x splitk {1, 3}; tiles 300-308 x splitk {1, 3} x b3_grouped {0, 1}, with the
   phase form of the up-convolution and the auxiliary problem of op_conv2d_pair / op_linear_pair (24-bit operands in the shortcut's planes); tiles 0 and 103 (plain fp32)
   as controls: the probes are valid on the device.
2. DENSE probes -- rho = |got - ref64| / sum_k |a_k| |w_k| per output in units of u = 2^-24, rms (every K) and max (K <= 64) at most 3 x what the plain fp32
   evaluation of the same inputs reaches (fp64 products accumulated one by one in fp32, computed here).  CPU, plain fp32: rms 0.935 / 0.709 / 0.817 u, max 7.36 / 6.34 /
   7.02 u at K = 32 / 64 / 288; one low product deleted: rms >= 13.7 u and max >= 65 u at K <= 64, rms >= 8.0 u at K = 288.  Measured on an MI355X: MEASURED below.
3. ATTENTION -- k_attn_split.hip through qkv_attention, the form asserted by sdmi_attention_plan: d = 40 x attn_pack_tail 0 .. 3, d = 80 and 64 x {0, 2}, attn_kv_splits 1
   and 3, the 4-wave form (n 1, nq 300, nk 200 = three key tiles + 8, 4 heads) and the 8-wave form (n 4, 32 heads: 2 x 128 workgroups of 256 rows, the fewest that fill the
   256 CUs the planner counts); control attn_split = 0 (k_attn.hip).
   V planes: one-hot softmax rows, expected = row j*(i) of v, within 4 ulp of |v| (derived: 2 for the kept products' 2^-23, 1 for the accumulation, 1 for the
   normalisation), columns 32 .. 39 separately at d = 40.  BIT EQUALITY where the kernel's p is exactly 1: the log2-softmax forms (attn_pack_tail 2, 3) with one key
   slice -- there the dominant score is the reference maximum itself (delta = mt, s - delta = 0, exp2(0) = 1), every other exponential underflows, the row sum is 1
   and the planes are added smallest first (l, l + m, l + m + h: each representable).  Round 4's softmax (0, 1) forms exp2(fma(s, c, -fl(s c))), which is 1 + O(2^-17);
   the key-slice merge and k_attn.hip normalise once more.
   P planes: one-hot value columns (+-2^e, and 16-bit mantissas in the odd columns so that p_m v_m counts), relative error over the probabilities above 2^-20: rms at
   most 3 x the plain fp32 CPU evaluation's (oracle qkv_attention on float32), columns 32 .. 39 separately at d = 40; the max is printed, not asserted (it does not
   keep 2 x from every mutation: precision_probes.attention_stats).
   Q / K planes: keys that all score +30, each in two columns of its own; max and rms absolute error at most 3 x the plain fp32 CPU evaluation's.

Every case asserts, from the engine's own record (options record_shapes / dump_choices) or plan, that the forced tile / kernel form really ran.

MEASURED -- MI355X (profiles/precision_resolution_measured.txt has every line and the CPU figures they were judged against).
Exact probes: no mismatch on any tile, variant, split-K, layout or form.
Dense rho in u, (max, rms); every tile of k_gemm3x.hip and k_gemm3p.hip, every variant and both layouts give the same figures at the same split-K:
           split / plane tiles, splitk 1   splitk 3        tiles 0 / 103, splitk 1   splitk 3        plain fp32 on the CPU (the bar is 3 x)
  K = 32   2.37, 0.359                     the same        8.41, 0.929               the same        7.36, 0.935
  K = 64   4.46, 0.408                     2.11, 0.295     5.51, 0.729               5.51, 0.643     6.34, 0.709
  K = 288  6.60, 0.746                     3.58, 0.419     9.09, 0.937               4.55, 0.566     7.02, 0.817
Attention, V planes: bit-exact in 28 of the 36 forms (every asserted one; k_attn.hip too), 1 ulp on a quarter of the outputs at d = 40 with attn_pack_tail 0 / 1.
Attention, largest ratio to the plain fp32 CPU evaluation (the bar is 3): p rms 2.06 (d = 64, attn_pack_tail 2, 8 waves; plain 1.88e-7), p tail rms 1.86, p max 2.36
(not asserted), qk max 1.10 and qk rms 1.14 (both k_attn.hip, d = 64; plain 3.95e-6 / 6.70e-7); k_attn_split.hip is below the plain evaluation on the Q / K probe."""
import re

import numpy as np
import pytest

import precision_probes as P

pytestmark = pytest.mark.gpu

STILES = [200, 201, 202, 203, 204, 205]
PTILES = [300, 301, 302, 303, 304, 305, 306, 307, 308]
VARIANTS = [0, 1, 2, 6]          # bit 1: the scalar-subtraction split of S3SplitT; bit 0: the DMA in one block; bit 2: two LDS stages on the 128-row tiles
CONV_CASES = [(32, 1, 1, 0), (64, 1, 1, 0), (64, 3, 1, 0), (64, 3, 2, 0), (64, 3, 1, 1)]      # (cin, k, stride, ups)
COUT = 336
PAIR_COUT, PAIR_KAUX, FOLD_KMAIN = 96, 64, 128
_DEFAULTS = {"gemm_tile": "auto", "splitk": 0, "splitk_aux": 0, "gemm_planes": "default", "gemm3x_variant": "default", "ups_phase": "default", "b3_grouped": 1,
             "skip_slices": 1, "proj_out_fold": 2, "attn_split": 1, "attn_pack_tail": "default", "attn_kv_splits": 0, "attn_d64": "default"}
_LINE = re.compile(r"^(\d+),(\d+),(\d+) k(\d) s(\d) u(\d) W(\d+)( phase| pair| fold)? cfg=(\d+) splits=(\d+)(.*?) acc=\d+ x(\d+)$")


def _recorded(sd, tmp_path, fn, **opts):
    """fn() under the given engine options (restored afterwards) -> (result, the GEMM launches it made: dump_choices lines)"""
    path = tmp_path / "choices.txt"
    try:
        for k, v in opts.items():
            sd.set_option(k, v)
        sd.set_option("record_shapes", 1)
        try:
            out = fn()
        finally:
            sd.set_option("dump_choices", str(path))
    finally:
        sd.set_option("record_shapes", 0)
        for k in opts:
            sd.set_option(k, _DEFAULTS[k])
    return out, path.read_text().splitlines()


def _clamp(splits, kt_total):
    """gemm_plan.cpp clamp_splits: the slices a request for `splits` becomes over kt_total k tiles"""
    splits = max(1, min(splits, kt_total))
    per = -(-kt_total // splits)
    return -(-kt_total // per)


def _assert_ran(lines, tile, splitk, calls, kind=""):
    """every recorded launch ran on `tile` as the given kind ('' | ' phase' | ' pair' | ' fold') with the slices the request clamps to, and there were `calls` of them"""
    total = 0
    for ln in lines:
        m = _LINE.match(ln)
        assert m, f"unreadable record: {ln!r}"
        K, got_kind, cfg, splits, note, count = int(m.group(3)), m.group(8) or "", int(m.group(9)), int(m.group(10)), m.group(11), int(m.group(12))
        assert cfg == tile and got_kind == kind and "no planes" not in note, f"asked for tile {tile}{kind}: {ln}"
        if kind in ("", " phase"):
            kt = K // 72 if kind else K // 32          # a phase launch: K = 4 cin per phase, cin / 8 k tiles
            assert splits == _clamp(splitk, kt), f"asked for splitk {splitk} over {kt} k tiles: {ln}"
        else:
            assert splits >= 2 and " +aux K" in note, ln
        total += count
    assert total == calls, f"{calls} calls, {total} launches recorded on tile {tile}{kind}: {lines}"


def _exact(got, ref, what):
    frac = P.exact_mismatch(got, ref)
    if frac:
        bad = np.argwhere(~(got.astype(np.float32) == ref.astype(np.float32)))[0]
        i = tuple(bad)
        raise AssertionError(f"{what}: {100 * frac:.2f} % of the outputs are not the exactly representable product; first at {i}: got {got[i]!r}, want {np.float32(ref[i])!r}")


def _conv_calls(sd):
    """every exact convolution probe -> number of calls made (each checked)"""
    calls = 0
    for cin, k, stride, ups in CONV_CASES:
        for family in P.FAMILIES:
            for s in range(P.weight_sets(COUT, cin * k * k)):
                x, wt, ref = P.exact_conv_case(family, cin, k, stride, ups, s)
                _exact(sd.op_conv2d(x, wt, None, stride=stride, upsample2x=bool(ups)), ref, f"conv family {family} cin={cin} k={k} stride={stride} ups={ups} weight set {s}")
                calls += 1
    return calls


def _linear_calls(sd):
    calls = 0
    for cin in (32, 64):
        for family in P.FAMILIES:
            x, wt, ref = P.exact_linear_case(family, cin, 0)
            _exact(sd.op_linear(x, wt, None), ref, f"linear family {family} cin={cin}")
            calls += 1
    return calls


def _phase_calls(sd):
    """the up-convolution as four folded 2x2 phase convolutions: a one-hot 3x3 weight folds to itself"""
    calls = 0
    for family in P.FAMILIES:
        for s in range(P.weight_sets(COUT, 64 * 9)):
            x, wt, ref = P.exact_conv_case(family, 64, 3, 1, 1, s)
            _exact(sd.op_conv2d(x, wt, None, upsample2x=True), ref, f"phase conv family {family} weight set {s}")
            calls += 1
    return calls


def _pair_calls(sd, conv):
    calls = 0
    k_main = PAIR_COUT if conv else FOLD_KMAIN
    for family in P.FAMILIES:
        for s in range(P.weight_sets(PAIR_COUT // 2, PAIR_KAUX)):
            xm, xa, wm, wa, ref = P.exact_pair_case(family, k_main, PAIR_KAUX, s, conv, cout=PAIR_COUT)
            got = sd.op_conv2d_pair(xa, xm, wa, None, wm, None) if conv else sd.op_linear_pair(xm, xa, wm, None, wa, None)
            _exact(got, ref, f"{'conv' if conv else 'linear'} pair, auxiliary family {family}, weight set {s}")
            calls += 1
    return calls


# ---- 1. exact probes --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tile", STILES)
def test_exact_products_on_the_split_tiles(sd_ops, tmp_path, tile, splitk):
    """k_gemm3x.hip: weights as planes, activations split in the kernel (S3SplitT, both forms of the residual subtraction)"""
    for variant in VARIANTS:
        calls, lines = _recorded(sd_ops, tmp_path, lambda: _conv_calls(sd_ops) + _linear_calls(sd_ops), gemm_tile=tile, splitk=splitk, gemm3x_variant=variant)
        _assert_ran(lines, tile, splitk, calls)


@pytest.mark.parametrize("grouped", [0, 1])
@pytest.mark.parametrize("tile", PTILES)
def test_exact_products_on_the_plane_tiles(sd_ops, tmp_path, tile, grouped):
    """k_gemm3p.hip: both operands as planes (split3_rows_kernel in front of the launch; launch_pack_split3 in the row-major and the 16-row-group layout) -- convolutions,
    Linear, the phase form of the up-convolution, and the shortcut's slices of the paired launches"""
    for splitk, splitk_aux in ((1, 1), (3, 2)):
        base = dict(gemm_planes=2, gemm_tile=tile, splitk=splitk, b3_grouped=grouped)
        calls, lines = _recorded(sd_ops, tmp_path, lambda: _conv_calls(sd_ops) + _linear_calls(sd_ops), **base)
        _assert_ran(lines, tile, splitk, calls)
        calls, lines = _recorded(sd_ops, tmp_path, lambda: _phase_calls(sd_ops), ups_phase=1, **base)
        _assert_ran(lines, tile, splitk, calls, " phase")
        calls, lines = _recorded(sd_ops, tmp_path, lambda: _pair_calls(sd_ops, True), skip_slices=1, splitk_aux=splitk_aux, **base)
        _assert_ran(lines, tile, splitk, calls, " pair")
        calls, lines = _recorded(sd_ops, tmp_path, lambda: _pair_calls(sd_ops, False), proj_out_fold=1, splitk_aux=splitk_aux, **base)
        _assert_ran(lines, tile, splitk, calls, " fold")


@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tile", [0, 103])
def test_exact_products_on_the_fp32_controls(sd_ops, tmp_path, tile, splitk):
    """k_gemm2.hip (tile 0) and the fp32 matrix instruction (k_gemm2x.hip, tile 103): the probes hold on plain fp32, so a failure above is the planes'"""
    calls, lines = _recorded(sd_ops, tmp_path, lambda: _conv_calls(sd_ops) + _linear_calls(sd_ops), gemm_tile=tile, splitk=splitk)
    _assert_ran(lines, tile, splitk, calls)


# ---- 2. dense probes --------------------------------------------------------------------------------------------------------------------------------------------------
def _dense(sd, tmp_path, what, tile, splitk, **opts):
    """the three dense cases on one kernel configuration: rho printed, rms held at every K and max at K <= 64 against FACTOR x the plain fp32 evaluation"""
    def run():
        return [sd.op_conv2d(c["x"], c["wt"], None) for c in (P.dense_case(cin, k) for cin, k in P.DENSE_CASES)]
    outs, lines = _recorded(sd, tmp_path, run, gemm_tile=tile, splitk=splitk, **opts)
    _assert_ran(lines, tile, splitk, len(outs))
    failures = []
    for (cin, k), got in zip(P.DENSE_CASES, outs):
        c = P.dense_case(cin, k)
        (gmax, grms), (pmax, prms) = P.rho_stats(got, c["ref"], c["denom"]), c["plain"]
        print(f"RHO {what} K={c['K']}: max {gmax:.2f} u rms {grms:.3f} u (plain fp32 on the CPU: max {pmax:.2f} u rms {prms:.3f} u)")
        if grms > P.FACTOR * prms:
            failures.append(f"{what} K={c['K']}: rms rho {grms:.3f} u > {P.FACTOR:g} x {prms:.3f} u")
        if c["K"] <= 64 and gmax > P.FACTOR * pmax:
            failures.append(f"{what} K={c['K']}: max rho {gmax:.2f} u > {P.FACTOR:g} x {pmax:.2f} u")
    assert not failures, failures


@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tile", STILES)
def test_dense_componentwise_error_on_the_split_tiles(sd_ops, tmp_path, tile, splitk):
    for variant in VARIANTS:
        _dense(sd_ops, tmp_path, f"tile={tile} splitk={splitk} variant={variant}", tile, splitk, gemm3x_variant=variant)


@pytest.mark.parametrize("grouped", [0, 1])
@pytest.mark.parametrize("tile", PTILES)
def test_dense_componentwise_error_on_the_plane_tiles(sd_ops, tmp_path, tile, grouped):
    for splitk in (1, 3):
        _dense(sd_ops, tmp_path, f"tile={tile} splitk={splitk} b3_grouped={grouped}", tile, splitk, gemm_planes=2, b3_grouped=grouped)


@pytest.mark.parametrize("tile", [0, 103])
def test_dense_componentwise_error_on_the_fp32_controls(sd_ops, tmp_path, tile):
    for splitk in (1, 3):
        _dense(sd_ops, tmp_path, f"tile={tile} splitk={splitk} (fp32 control)", tile, splitk)


# ---- 3. attention -----------------------------------------------------------------------------------------------------------------------------------------------------
SHAPES = {4: (1, 300, 200, 4), 8: (4, 300, 200, 32)}          # waves -> n, nq, nk, heads
# (d, attn_pack_tail, waves): round 4's softmax (attn_pack_tail without bit 1) has no 8-wave d = 80 instance
FORMS = [(d, pt, w) for w in (4, 8) for d, pts in ((40, (0, 1, 2, 3)), (80, (0, 2)), (64, (0, 2))) for pt in pts if not (w == 8 and d == 80 and pt == 0)]


def _attention(sd, d, waves, kernel, kv_splits, exact_p, **opts):
    n, nq, nk, n_head = SHAPES[waves]
    what = f"d={d} {kernel} waves={waves} kv_splits={kv_splits} " + " ".join(f"{k}={v}" for k, v in opts.items())
    try:
        for k, v in opts.items():
            sd.set_option(k, v)
        plan = sd.attention_plan(n, n_head, nq, nk, d)
        tiles = -(-nk // plan["kv_tile"])
        assert (plan["kernel"], plan["waves"], plan["kv_splits"]) == (kernel, waves, min(kv_splits, tiles)), f"{what}: the plan is {plan}"
        outs = {}
        for kind in ("v", "p", "qk"):
            c = P.attention_case(kind, n, nq, nk, n_head, d)
            outs[kind] = sd.qkv_attention(c["q"], c["k"], c["v"], None, n_head)
    finally:
        for k in opts:
            sd.set_option(k, _DEFAULTS[k])
    failures = []
    # V planes
    c = P.attention_case("v", n, nq, nk, n_head, d)
    got = outs["v"]
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    ul = P.ulps(got, c["ref"])
    tail = float(ul.reshape(n, nq, n_head, d)[..., 32:].max()) if d == 40 else 0.0
    print(f"ATTN {what} V planes: max {ul.max():.2f} ulp" + (f", columns 32..39 {tail:.2f} ulp" if d == 40 else "") + f", {100 * float((ul > 0).mean()):.1f} % of the outputs inexact")
    if ul.max() > 4.0:
        failures.append(f"V planes: {ul.max():.1f} ulp > 4")
    if tail > 4.0:
        failures.append(f"V planes, columns 32..39: {tail:.1f} ulp > 4")
    if exact_p and ul.max() != 0.0:
        failures.append(f"V planes: p is exactly 1 in this form, yet {100 * float((ul > 0).mean()):.2f} % of the outputs are not row j* of v bit for bit (max {ul.max():.2f} ulp)")
    # P and Q / K planes
    for kind in ("p", "qk"):
        c = P.attention_case(kind, n, nq, nk, n_head, d)
        st = P.attention_stats(kind, outs[kind], c, n_head)
        print(f"ATTN {what} {'P' if kind == 'p' else 'Q/K'} planes: " + ", ".join(f"{k} {v:.3e} (plain fp32 on the CPU {c['plain'][k]:.3e})" for k, v in st.items()))
        for name, s in st.items():
            if name in P.ASSERTED and s > P.FACTOR * c["plain"][name]:
                failures.append(f"{name}: {s:.3e} > {P.FACTOR:g} x {c['plain'][name]:.3e}")
    assert not failures, f"{what}: {failures}"


@pytest.mark.parametrize("kv_splits", [1, 3])
@pytest.mark.parametrize("d,pack_tail,waves", FORMS)
def test_attention_planes_on_the_split_kernel(sd_ops, d, pack_tail, waves, kv_splits):
    _attention(sd_ops, d, waves, "split", kv_splits, exact_p=bool(pack_tail & 2) and kv_splits == 1,
               attn_split=1, attn_pack_tail=pack_tail, attn_kv_splits=kv_splits, **({"attn_d64": 1} if d == 64 else {}))


@pytest.mark.parametrize("kv_splits", [1, 3])
@pytest.mark.parametrize("d", [40, 80, 64])
def test_attention_probes_on_the_fp32_control(sd_ops, d, kv_splits):
    """k_attn.hip (fp32 matrix instruction): the probes and their bars hold on plain fp32"""
    _attention(sd_ops, d, 4, "flash", kv_splits, exact_p=False, attn_split=0, attn_kv_splits=kv_splits)
