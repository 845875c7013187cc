"""The probes of tests/precision_probes.py detect what they claim -- proved on the CPU with the six-product model (oracle/split_oracle.py's arithmetic) and its
mutations: each kept product deleted, the l plane shifted by one k position and by one row, V_m and V_l exchanged.  For every assertion that
tests/test_precision_resolution_gpu.py makes of a kernel:
  * the unmutated model passes it;
  * every mutation fails at least one of them -- which one is pinned here, product by product;
  * a ratio bar (3 x the plain fp32 evaluation) lies at least 2 x below every mutation it is meant to catch.
This is what keeps the GPU bars honest: a bar may only move while these still hold."""
import numpy as np
import pytest
import torch

import precision_probes as P
from oracle import sd_oracle as O
from oracle import split_oracle as S

# (cin, k, stride, ups): the convolution shapes of the exact probes (one sample of 17 x 19 pixels, cout = 336)
CONV_CASES = [(32, 1, 1, 0), (64, 1, 1, 0), (64, 3, 1, 0), (64, 3, 2, 0), (64, 3, 1, 1)]


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _mismatch_nonzero(got, ref):
    """fraction of the outputs with a non-zero reference (a tap inside the padding gives 0 whatever the planes hold) that differ from it"""
    live = ref != 0
    return float(np.mean(got.astype(np.float32)[live] != ref.astype(np.float32)[live]))


def test_operands_have_the_stated_bits_and_planes():
    g = np.random.default_rng(1)
    for bits in (1, 11, 12, 16, 24):
        x = P.odd_bits(g, (4000,), bits)
        m = np.abs(x.astype(np.float64))
        e = np.floor(np.log2(m))
        assert e.min() >= -12 and e.max() <= 12 and len(np.unique(e)) == 25
        mant = m / np.exp2(e - (bits - 1))
        assert np.array_equal(mant, np.round(mant)) and (mant.astype(np.int64) % 2 == 1).all() and (mant < 2 ** bits).all() and (mant >= 2 ** (bits - 1)).all()
        assert (x > 0).any() and (x < 0).any()
        h, mm, l = S.split3(x)
        assert np.array_equal(h.astype(np.float64) + mm + l, x.astype(np.float64))
        if bits == 24:
            assert (l != 0).mean() > 0.98 and (mm != 0).mean() > 0.98    # (a run of zero bits behind h lets m reach bit 0: l = 0, rarely)
        if bits in (11, 12):
            assert (mm != 0).all() and (l == 0).all()
        if bits == 1:
            assert (mm == 0).all() and (l == 0).all()


@pytest.mark.parametrize("case", CONV_CASES)
def test_one_hot_weight_sets_select_every_k_position_and_the_gather_is_the_convolution(case):
    cin, k, stride, ups = case
    K, cout = cin * k * k, 336
    sets = P.weight_sets(cout, K)
    seen = np.zeros(K, bool)
    for s in range(sets):
        pos = P.onehot_positions(cout, K, s)
        seen[pos] = True
        assert (pos[1:] != pos[:-1]).all()
        x, wt, ref = P.exact_conv_case("C", cin, k, stride, ups, s)
        assert (np.count_nonzero(wt.reshape(cout, -1), axis=1) == 1).all()
        xin = O.upsample2x(_t(x)) if ups else _t(x)
        conv = O.conv2d(xin, (_t(wt), None), stride=stride, padding=1 if k == 3 else 0).numpy()
        assert np.array_equal(conv, ref), "the gather is not the convolution"
        col = P.rows_to_nchw(P.im2col(x, k, stride, ups) @ wt.reshape(cout, -1).astype(np.float64).T, 1, *ref.shape[2:])
        assert np.array_equal(col, ref), "im2col is not the convolution"
    assert seen.all(), f"{(~seen).sum()} of {K} k positions are never selected"


@pytest.mark.parametrize("family", P.FAMILIES)
@pytest.mark.parametrize("case", CONV_CASES)
def test_exact_families_are_exact_under_six_products_and_lose_98_percent_without_a_needed_one(family, case):
    cin, k, stride, ups = case
    cout = 336
    x, wt, ref = P.exact_conv_case(family, cin, k, stride, ups, 0)
    a, w = P.im2col(x, k, stride, ups), wt.reshape(cout, -1)
    shape = (1,) + ref.shape[2:]
    got = P.rows_to_nchw(P.model_gemm(a, w), *shape)
    assert P.exact_mismatch(got, ref) == 0.0, f"family {family} is not exact under the six-product model"
    for pr in P.NEEDS[family]:
        bad = P.rows_to_nchw(P.model_gemm(a, w, P.Mutation(drop=pr)), *shape)
        frac = _mismatch_nonzero(bad, ref)
        print(f"family {family} {case} without {P.product_name(pr)}: {100 * frac:.1f} % of the outputs differ")
        assert frac > 0.98
        assert P.exact_mismatch(bad, ref) > 0.5


def test_every_gemm_mutation_fails_an_exact_family_and_which():
    """pins, product by product, the family that catches its loss (DESIGN.md section 4a names the same)"""
    cin, k, cout = 64, 3, 336
    caught = {}
    for family in P.FAMILIES:
        x, wt, ref = P.exact_conv_case(family, cin, k, 1, 0, 0)
        a, w = P.im2col(x, k), wt.reshape(cout, -1)
        for mu in P.gemm_mutations():
            bad = P.rows_to_nchw(P.model_gemm(a, w, mu), 1, 17, 19)
            if P.exact_mismatch(bad, ref) > 0.5:
                caught.setdefault(mu.name, []).append(family)
    print(caught)
    want = {"without a_h.w_l": ["B"], "without a_l.w_h": ["A"], "without a_m.w_m": ["C"], "without a_h.w_m": ["B", "C"], "without a_m.w_h": ["A", "C"],
            "without a_h.w_h": ["A", "B", "C"], "a_l shifted by one k": ["A"], "a_l shifted by one row": ["A"], "w_l shifted by one k": ["B"], "w_l shifted by one row": ["B"]}
    assert caught == want


@pytest.mark.parametrize("family", ["A", "B", "C"])
@pytest.mark.parametrize("conv", [True, False])
def test_pair_probes_put_one_product_in_every_output(family, conv):
    """a paired launch's probe: odd channels = one auxiliary product of the family, even channels = one main product of family C; exact under the model, and the
    auxiliary operands' low products are needed"""
    cout = 96
    seen = np.zeros(64, bool)
    for s in range(P.weight_sets(cout // 2, 64)):
        wa = P.exact_pair_case(family, 96 if conv else 128, 64, s, conv, cout=cout)[3]
        seen |= (wa.reshape(cout, 64) if conv else wa.T).any(axis=0)
    assert seen.all(), "a k position of the auxiliary problem is never selected"
    xm, xa, wm, wa, ref = P.exact_pair_case(family, 96 if conv else 128, 64, 0, conv, cout=cout)
    if conv:
        am, aa = P.im2col(xm, 3), P.im2col(xa, 1)
        bm, ba = wm.reshape(cout, -1), wa.reshape(cout, -1)
        back = lambda r: P.rows_to_nchw(r, 1, 17, 19)
    else:
        am, aa, bm, ba = xm, xa, wm.T, wa.T
        back = lambda r: r
    assert (np.count_nonzero(bm, axis=1) + np.count_nonzero(ba, axis=1) == 1).all()
    assert P.exact_mismatch(back(P.model_gemm(am, bm) + P.model_gemm(aa, ba)), ref) == 0.0
    for pr in P.NEEDS[family]:
        bad = back(P.model_gemm(am, bm) + P.model_gemm(aa, ba, P.Mutation(drop=pr)))
        odd = (bad.astype(np.float32) != ref.astype(np.float32))[:, 1::2]          # (channels are axis 1 of [n, cout, h, w] and of [rows, cout])
        assert odd.mean() > 0.95, f"auxiliary problem without {P.product_name(pr)}: {odd.mean()}"          # (48 channels: one weight with an empty plane is 2 %)


@pytest.mark.parametrize("cin,k", P.DENSE_CASES)
def test_dense_bar_passes_the_model_and_lies_2x_below_every_mutation(cin, k):
    """rho in units of 2^-24; the bar = 3 x plain fp32.  rms is asserted at every K, max at K <= 64 (at K = 288 the max statistic separates too thinly)."""
    c = P.dense_case(cin, k)
    K = c["K"]
    pmax, prms = c["plain"]
    bmax, brms = P.FACTOR * pmax, P.FACTOR * prms
    mmax, mrms = P.rho_stats(P.rows_to_nchw(P.model_gemm(c["a"], c["wm"]), *c["shape"]), c["ref"], c["denom"])
    print(f"K = {K}: plain fp32 rho max {pmax:.2f} u rms {prms:.3f} u; six-product model max {mmax:.3f} u rms {mrms:.4f} u; bar max {bmax:.1f} u rms {brms:.2f} u")
    assert mrms <= brms and mmax <= bmax
    assert prms <= brms / 3 * (1 + 1e-12) and pmax <= bmax / 3 * (1 + 1e-12)
    for mu in P.gemm_mutations():
        bad = P.rows_to_nchw(P.model_gemm(c["a"], c["wm"], mu), *c["shape"])
        xmax, xrms = P.rho_stats(bad, c["ref"], c["denom"])
        print(f"K = {K} {mu}: rho max {xmax:.1f} u rms {xrms:.2f} u ({xmax / bmax:.1f} x / {xrms / brms:.1f} x the bar)")
        assert xrms >= 2 * brms, f"K = {K} {mu}: rms {xrms:.2f} u is not 2 x the bar {brms:.2f} u"
        if K <= 64:
            assert xmax >= 2 * bmax, f"K = {K} {mu}: max {xmax:.1f} u is not 2 x the bar {bmax:.1f} u"


# ---- attention --------------------------------------------------------------------------------------------------------------------------------------------------------
ATTN = [(1, 70, 100, 2, 40), (1, 70, 100, 2, 64)]      # n, nq, nk, heads, d: small, more than one 64-key tile, ragged


def _verdicts(case_v, case_p, case_qk, n_head, d, qk_mu, pv_mu):
    """which assertions of the GPU test a model with these mutations fails -> (set of names, {name: statistic / bar})"""
    failed, ratio = set(), {}
    with np.errstate(under="ignore"):
        got = P.model_attention(case_v["q"], case_v["k"], case_v["v"], n_head, qk_mu, pv_mu)
    ul = P.ulps(got, case_v["ref"])
    ratio["v"] = float(ul.max()) / 4.0
    if not (np.isfinite(got).all() and ul.max() <= 4.0):
        failed.add("v")
    if d == 40:
        tail = ul.reshape(ul.shape[0], ul.shape[1], n_head, d)[..., 32:].max()
        ratio["v tail"] = float(tail) / 4.0
        if not tail <= 4.0:
            failed.add("v tail")
    for kind, case in (("p", case_p), ("qk", case_qk)):
        got = P.model_attention(case["q"], case["k"], case["v"], n_head, qk_mu, pv_mu)
        for name, s in P.attention_stats(kind, got, case, n_head).items():
            ratio[name] = s / (P.FACTOR * case["plain"][name])
            if name in P.ASSERTED and not s <= P.FACTOR * case["plain"][name]:
                failed.add(name)
    return failed, ratio


@pytest.mark.parametrize("shape", ATTN)
def test_attention_probes_pass_the_model_and_every_mutation_fails_one(shape):
    n, nq, nk, n_head, d = shape
    cases = [P.attention_case(kind, n, nq, nk, n_head, d) for kind in ("v", "p", "qk")]
    for kind, c in zip(("p", "qk"), cases[1:]):
        print(f"d = {d} {kind} probe, plain fp32 CPU evaluation: " + ", ".join(f"{k} {v:.3e}" for k, v in c["plain"].items()))
    failed, ratio = _verdicts(*cases, n_head, d, None, None)
    print(f"d = {d} six-product model: " + ", ".join(f"{k} {v:.3f}" for k, v in ratio.items()) + " (of the bar)")
    assert not failed, failed
    with np.errstate(under="ignore"):
        exact = P.model_attention(cases[0]["q"], cases[0]["k"], cases[0]["v"], n_head)
    assert np.array_equal(exact.astype(np.float64), cases[0]["ref"]), "one-hot softmax rows: the model's output is not row j* of v, bit for bit"
    # the probe each mutation must fail, by at least 2 x where the bar is a ratio
    for qk_mu, pv_mu in P.attention_mutations(d):
        mu = qk_mu or pv_mu
        failed, ratio = _verdicts(*cases, n_head, d, qk_mu, pv_mu)
        print(f"d = {d} {mu}: fails {sorted(failed)}; " + ", ".join(f"{k} {v:.1f}" for k, v in ratio.items()))
        if qk_mu is not None:
            must = {"qk max", "qk rms"}
        elif pv_mu.drop in ((0, 2), (0, 1)) or pv_mu.shift:          # p_h.v_l, p_h.v_m, a displaced V_l: the one-hot rows
            must = {"v"}
        elif pv_mu.drop == (0, 0):
            must = {"v", "p rms"}
        else:                                                         # p_l.v_h, p_m.v_h, p_m.v_m, V_m <-> V_l (which loses p_m.v_m): the one-hot value columns
            must = {"p rms"}
        if d == 40 and pv_mu is not None:                             # ... and columns 32 .. 39, the packed tail, on their own
            must = must | ({"v tail"} if "v" in must else set()) | ({"p tail rms"} if "p rms" in must else set())
        if pv_mu is not None and pv_mu.swap_ml_rows == slice(32, 40):
            must = {"p tail rms"}
        assert must <= failed, f"{mu}: expected to fail {sorted(must)}, failed {sorted(failed)}"
        for name in must:
            assert ratio[name] >= 2.0, f"{mu}: {name} is only {ratio[name]:.2f} x its bar"
