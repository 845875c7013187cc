"""Inputs and statistics that resolve the LOW-ORDER bf16 planes of the fp32 split arithmetic (csrc/k_gemm3x.hip, k_gemm3p.hip, k_attn_split.hip).

A max-norm bar of 2e-5 max|ref| cannot see whether the three smallest kept products (a_l w_h, a_h w_l, a_m w_m) exist: each is 2^-16 of ITS product and drowns in
a sum of thousands.  The probes here make each of them the whole answer, or measure the error against the size of the terms that were summed:

  exact probes      one-hot weights, so every output is ONE product, with operands whose product is exactly representable: got == float32(ref64), bit for bit.
                      family A   x 24 bits, w +-2^e      needs x_m w_h and x_l w_h
                      family B   x +-2^e,   w 24 bits    needs x_h w_m and x_h w_l (and the weight-plane packers)
                      family C   x 12 bits, w 11 bits    needs h m, m h and m m (the product has 23 bits; every partial sum is an integer < 2^24 in the common unit)
  dense probes      random GEMMs under the COMPONENTWISE statistic rho = |got - ref64| / sum_k |a_k| |w_k| in units of u = 2^-24, held against a plain fp32 evaluation
                    of the same inputs (fp32_sequential) -- a low product missing from only a part of the accumulation shows here.
  attention probes  one-hot softmax rows (V planes), one-hot value columns (P planes) and large common-mode scores (Q / K planes).

model_gemm / model_attention evaluate a probe with the six-product arithmetic of oracle/split_oracle.py and take a MUTATION (a product deleted, the l plane shifted by
one k position or one row, V_m and V_l exchanged): tests/test_precision_probes_cpu.py proves with them that every probe detects what it claims, which is what keeps
the bars of tests/test_precision_resolution_gpu.py honest.  Helper module (like the *_ref.py files): no test lives here.

Reference arithmetic: Burn's Conv2d / Linear (unet/mod.rs:397-729, autoencoder/mod.rs:516-604) and qkv_attention (attention.rs:5-45) -- plain fp32; the planes are this
project's own."""
import math
import zlib

import numpy as np

from oracle import split_oracle as S

U = 2.0 ** -24
# (activation plane, weight plane) of the six products the kernels keep, smallest first (h = 0, m = 1, l = 2): split_oracle.gemm_split's list
KEPT = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))
PLANE = "hml"
# the products each exact family cannot do without
NEEDS = {"A": ((1, 0), (2, 0)), "B": ((0, 1), (0, 2)), "C": ((0, 1), (1, 0), (1, 1))}
FAMILIES = ("A", "B", "C")


def product_name(pr):
    return f"a_{PLANE[pr[0]]}.w_{PLANE[pr[1]]}"


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------------------------
def odd_bits(g, shape, bits, binade=None):
    """fp32 numbers +-m 2^(e - bits + 1) with m an odd integer of exactly `bits` significant bits, random sign, and the binade e drawn from -12 .. 12 (or given,
    broadcast to the shape): |value| in [2^e, 2^(e + 1))."""
    assert 1 <= bits <= 24
    if bits == 1:
        m = np.ones(shape, np.int64)
    else:
        m = (1 << (bits - 1)) | (g.integers(0, 1 << (bits - 2), shape, dtype=np.int64) << 1) | 1
    e = g.integers(-12, 13, shape) if binade is None else np.broadcast_to(binade, shape)
    v = g.choice(np.array([-1.0, 1.0]), shape) * m * np.exp2((e - (bits - 1)).astype(np.float64))
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


FAMILY_BITS = {"A": (24, 1), "B": (1, 24), "C": (12, 11)}   # (activation bits, weight bits)


def family_operands(g, family, x_shape, w_count):
    """activations of x_shape (they differ per element) and w_count weight values of one exact family"""
    xb, wb = FAMILY_BITS[family]
    return odd_bits(g, x_shape, xb), odd_bits(g, (w_count,), wb)


# ---- one-hot weights ---------------------------------------------------------------------------------------------------------------------------------------------
def weight_sets(cout, K):
    """how many one-hot weight sets of cout channels it takes to select every one of K positions"""
    return -(-K // cout)


def onehot_positions(cout, K, set_index, seed=2024):
    """position (of K) of output channel c's only non-zero weight in weight set set_index: a fixed permutation of the K positions dealt out to the channels in turn,
    so neighbouring channels sit at unrelated positions and sets 0 .. weight_sets(cout, K) - 1 cover every position"""
    perm = np.random.default_rng(seed + 7919 * K).permutation(K)
    return perm[(np.arange(cout) + set_index * cout) % K]


def onehot_conv_weight(pos, val, cin, k):
    """[cout, cin, k, k] with weight[c].flat[pos[c]] = val[c]"""
    cout = len(pos)
    w = np.zeros((cout, cin * k * k), np.float32)
    w[np.arange(cout), pos] = val
    return w.reshape(cout, cin, k, k)


def onehot_linear_weight(pos, val, cin):
    """[cin, cout] (the reference's Linear layout) with weight[pos[c], c] = val[c]"""
    cout = len(pos)
    w = np.zeros((cin, cout), np.float32)
    w[pos, np.arange(cout)] = val
    return w


def conv_out_size(h, k, stride, ups):
    pad = 1 if k == 3 else 0
    return ((h << ups) + 2 * pad - k) // stride + 1


def onehot_conv_ref(x, pos, val, k, stride=1, ups=0):
    """float64 result of conv2d(upsample2x^ups(x), one-hot weight): out[n, c, oy, ox] = val[c] * x_padded[n, ci(c), oy stride + ky(c), ox stride + kx(c)] -- a gather, one
    product per output"""
    n, cin, h, w = x.shape
    xs = x.astype(np.float64)
    if ups:
        xs = xs.repeat(2, axis=2).repeat(2, axis=3)
    pad = 1 if k == 3 else 0
    xp = np.pad(xs, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    ho, wo = conv_out_size(h, k, stride, ups), conv_out_size(w, k, stride, ups)
    ci, ky, kx = np.unravel_index(pos, (cin, k, k))
    oy = np.arange(ho)[None, :, None] * stride + ky[:, None, None]
    ox = np.arange(wo)[None, None, :] * stride + kx[:, None, None]
    return xp[:, ci[:, None, None], oy, ox] * val.astype(np.float64)[None, :, None, None]


def im2col(x, k, stride=1, ups=0):
    """[n ho wo, cin k k] float64 rows of conv2d's GEMM, columns in the weight's (cin, ky, kx) order"""
    n, cin, h, w = x.shape
    xs = x.astype(np.float64)
    if ups:
        xs = xs.repeat(2, axis=2).repeat(2, axis=3)
    pad = 1 if k == 3 else 0
    xp = np.pad(xs, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    ho, wo = conv_out_size(h, k, stride, ups), conv_out_size(w, k, stride, ups)
    cols = np.empty((n, ho, wo, cin, k, k), np.float64)
    for ky in range(k):
        for kx in range(k):
            cols[:, :, :, :, ky, kx] = xp[:, :, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride].transpose(0, 2, 3, 1)
    return cols.reshape(n * ho * wo, cin * k * k)


def rows_to_nchw(rows, n, ho, wo):
    """[n ho wo, cout] -> [n, cout, ho, wo]"""
    return np.ascontiguousarray(rows.reshape(n, ho, wo, -1).transpose(0, 3, 1, 2))


def exact_mismatch(got, ref64):
    """fraction of the outputs that are not float32(ref64); +-0 are one value (an all-padding tap gives +-0 either way)"""
    got = np.asarray(got)
    ref = np.asarray(ref64, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref), "the probe's reference is not exactly representable in fp32"
    return float(np.mean(~(got.astype(np.float32) == r32)))          # (a NaN counts as a mismatch)


# ---- dense probes ------------------------------------------------------------------------------------------------------------------------------------------------
def dense_conv_inputs(g, n, cin, h, w, cout, k):
    """x normal with a per-channel binade in 2^-5 .. 2^5; weight normal / sqrt(K) with a per-row binade in 2^-3 .. 2^3"""
    x = (g.standard_normal((n, cin, h, w)) * np.exp2(g.integers(-5, 6, (1, cin, 1, 1)))).astype(np.float32)
    wt = (g.standard_normal((cout, cin, k, k)) / math.sqrt(cin * k * k) * np.exp2(g.integers(-3, 4, (cout, 1, 1, 1)))).astype(np.float32)
    return x, wt


def fp32_sequential(a, w):
    """a [M, K] @ w [N, K]^T as plain fp32 does it: every product formed exactly (float64 holds 48 bits), accumulated one after the other in fp32"""
    a = np.asarray(a, np.float64)
    w = np.asarray(w, np.float64)
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for kk in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a[:, kk:kk + 1] * w[None, :, kk]).astype(np.float32)
    return acc


def rho_stats(got, ref64, denom):
    """(max, rms) of rho = |got - ref64| / sum_k |a_k| |w_k| over the outputs, in units of u = 2^-24"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape == denom.shape, (got.shape, ref64.shape, denom.shape)
    assert np.isfinite(got).all(), "non-finite output"
    ok = denom > 0
    rho = np.abs(got - ref64)[ok] / denom[ok] / U
    return float(rho.max()), float(np.sqrt(np.mean(rho * rho)))


# ---- the six-product model and its mutations -----------------------------------------------------------------------------------------------------------------------
class Mutation:
    """What a wrong kernel would do.  drop: one (activation plane, weight plane) product left out; shift = (operand 'a' | 'w', axis 'k' | 'row'): that operand's l plane
    moved by one position along k, or by one row (an activation row is an output row, a weight row an output channel); swap_ml_rows: the rows of the weight operand
    (for P V, whose weight operand is V^T, the value columns) whose m and l planes are exchanged."""

    def __init__(self, drop=None, shift=None, swap_ml_rows=None, name=None):
        self.drop, self.shift, self.swap_ml_rows = drop, shift, swap_ml_rows
        self.name = name or (f"without {product_name(drop)}" if drop else f"{shift[0]}_l shifted by one {shift[1]}" if shift else "m and l planes exchanged")

    def __repr__(self):
        return self.name


def gemm_mutations():
    """each kept product deleted, one at a time; the l plane of either operand shifted by one k position, and by one row"""
    return [Mutation(drop=pr) for pr in KEPT] + [Mutation(shift=(op, ax)) for op in "aw" for ax in ("k", "row")]


def model_gemm(a, w, mutation=None):
    """a [M, K] @ w [N, K]^T as the split kernels form it: the six kept partial products (each exact), summed in float64 -- split_oracle.gemm_split with a mutation"""
    ap = [v.astype(np.float64) for v in S.split3(np.ascontiguousarray(a, np.float32))]
    wp = [v.astype(np.float64) for v in S.split3(np.ascontiguousarray(w, np.float32))]
    mu = mutation
    if mu is not None and mu.shift:
        planes = ap if mu.shift[0] == "a" else wp
        planes[2] = np.roll(planes[2], 1, axis=1 if mu.shift[1] == "k" else 0)
    if mu is not None and mu.swap_ml_rows is not None:
        m, l = wp[1].copy(), wp[2].copy()
        m[mu.swap_ml_rows], l[mu.swap_ml_rows] = wp[2][mu.swap_ml_rows], wp[1][mu.swap_ml_rows]
        wp[1], wp[2] = m, l
    out = np.zeros((ap[0].shape[0], wp[0].shape[0]), np.float64)
    for ia, iw in KEPT:
        if mu is not None and mu.drop == (ia, iw):
            continue
        out += ap[ia] @ wp[iw].T
    return out


# ---- attention ------------------------------------------------------------------------------------------------------------------------------------------------------
def heads(t, n_head):
    """[n, rows, c] -> [n, n_head, rows, d]"""
    n, rows, c = t.shape
    return t.reshape(n, rows, n_head, c // n_head).transpose(0, 2, 1, 3)


def unheads(t):
    """[n, n_head, rows, d] -> [n, rows, c]"""
    n, nh, rows, d = t.shape
    return np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(n, rows, nh * d)


def attention_ref64(q, k, v, n_head):
    """qkv_attention in float64 -> (output [n, nq, c], probabilities [n, n_head, nq, nk])"""
    d = q.shape[2] // n_head
    qh, kh, vh = (heads(np.asarray(t, np.float64), n_head) for t in (q, k, v))
    s = qh @ kh.transpose(0, 1, 3, 2) * d ** -0.5
    p = np.exp(s - s.max(axis=3, keepdims=True))
    p /= p.sum(axis=3, keepdims=True)
    return unheads(p @ vh), p


def model_attention(q, k, v, n_head, qk_mutation=None, pv_mutation=None):
    """qkv_attention as k_attn_split.hip forms it: S = Q K^T and O = P V by the six-product arithmetic (model_gemm; q is the activation operand of the first, the
    probabilities of the second), the softmax between them in fp32 (scores rounded to fp32, exponentials of s - max in fp32, unnormalised; the row sum in fp32, one
    division at the end).  A mutation's swap_ml_rows names value columns."""
    n, nq, c = q.shape
    d = c // n_head
    qh, kh, vh = (heads(np.ascontiguousarray(t, np.float32), n_head) for t in (q, k, v))
    out = np.empty((n, n_head, nq, d), np.float32)
    for b in range(n):
        for h in range(n_head):
            s = (model_gemm(qh[b, h], kh[b, h], qk_mutation) * d ** -0.5).astype(np.float32)
            e = np.exp(s - s.max(axis=1, keepdims=True)).astype(np.float32)
            o = model_gemm(e, np.ascontiguousarray(vh[b, h].T), pv_mutation).astype(np.float32)
            out[b, h] = o / e.sum(axis=1, keepdims=True, dtype=np.float32)
    return unheads(out)


def attention_mutations(d):
    """(qk_mutation, pv_mutation) pairs: each kept product of Q K^T and of P V deleted; the l plane of K and of V shifted by one column and by one key; and V_m / V_l
    exchanged -- in every column, and (d = 40) in columns 32 .. 39 alone.  Exchanged planes lose p_m.v_m (and keep the dropped p_m.v_l in its place) under the
    six kept products; the packed tail tile sums all nine products of its row groups, so there an exchange of two groups changes nothing and only a group that is
    missing or lands outside the three summed ones is an error -- which is the deletion of its products, above."""
    out = []
    for pr in KEPT:
        out.append((Mutation(drop=pr, name=f"Q K^T without q_{PLANE[pr[0]]}.k_{PLANE[pr[1]]}"), None))
        out.append((None, Mutation(drop=pr, name=f"P V without p_{PLANE[pr[0]]}.v_{PLANE[pr[1]]}")))
    out.append((Mutation(shift=("w", "k"), name="K_l shifted by one column"), None))
    out.append((Mutation(shift=("w", "row"), name="K_l shifted by one key"), None))
    out.append((None, Mutation(shift=("w", "k"), name="V_l shifted by one key")))        # (the w operand of P V is V^T: its k axis runs over the keys)
    out.append((None, Mutation(shift=("w", "row"), name="V_l shifted by one column")))
    out.append((None, Mutation(swap_ml_rows=slice(0, d), name="V_m and V_l exchanged")))
    if d == 40:
        out.append((None, Mutation(swap_ml_rows=slice(32, 40), name="V_m and V_l exchanged in columns 32..39")))
    return out


def dominant_key(nq, nk):
    """j*(i) = (7 i + 3) mod nk"""
    return (7 * np.arange(nq) + 3) % nk


MIN_LEAD = 150.0   # natural-log units: exp(-150) = 2^-216 underflows to 0 in fp32 also behind a reference maximum deferred by 2^8 (k_attn_split.hip, LG)


def v_plane_probe(g, n, nq, nk, n_head, d):
    """One-hot softmax rows.  Keys are random sign vectors, query i is T times key j*(i): its score leads every other key's by T (d - max other dot) / sqrt(d) >= MIN_LEAD
    (checked), so every other probability is 0 in fp32 and the output is row j*(i) of v.  v: 24-bit mantissas with a binade per column.  -> q, k, v, expected [n, nq, c]"""
    c = n_head * d
    jstar = dominant_key(nq, nk)
    kh = g.choice(np.array([-1.0, 1.0]), (n, n_head, nk, d))
    dots = kh[:, :, jstar, :] @ kh.transpose(0, 1, 3, 2)                       # [n, h, nq, nk]
    dots[:, :, np.arange(nq), jstar] = -np.inf
    gap = d - dots.max()
    assert gap > 0, "two keys coincide"
    T = 2.0 ** math.ceil(math.log2(MIN_LEAD * math.sqrt(d) / gap))
    assert T * gap / math.sqrt(d) >= MIN_LEAD
    qh = T * kh[:, :, jstar, :]
    q, k = unheads(qh).astype(np.float32), unheads(kh).astype(np.float32)
    v = odd_bits(g, (n, nk, c), 24, binade=g.integers(-6, 7, (1, 1, c)))
    return q, k, v, v[:, jstar, :].astype(np.float64)


def ulps(got, ref64):
    """|got - ref| in units of the fp32 spacing at |ref|"""
    ref32 = np.asarray(ref64).astype(np.float32)
    return np.abs(np.asarray(got, np.float64) - ref64) / np.spacing(np.abs(ref32)).astype(np.float64)


def kappa(n_head, d, nk):
    """the key that column c of head h selects in the P-plane probe: (11 (h d + c) + 5) mod nk"""
    return ((11 * np.arange(n_head * d) + 5) % nk).reshape(n_head, d)


def p_plane_probe(g, n, nq, nk, n_head, d):
    """Moderate random scores (standard normal q and k: standard deviation 1, |s| up to about 4) and v one-hot per column: v[kappa(c), c] = +-2^e in the even columns -- then out[i, c] = p(i, kappa(c)) 2^e
    needs p_m v_h and p_l v_h -- and a 16-bit odd mantissa times 2^e in the odd columns, where p_m v_m (2^-16 of the product) is needed too.  -> q, k, v"""
    c = n_head * d
    q = g.standard_normal((n, nq, c)).astype(np.float32)
    k = g.standard_normal((n, nk, c)).astype(np.float32)
    e = g.integers(-6, 7, c)
    val = np.where(np.arange(c) % 2 == 0, odd_bits(g, (c,), 1, binade=e), odd_bits(g, (c,), 16, binade=e))
    v = np.zeros((n, nk, c), np.float32)
    v[:, kappa(n_head, d, nk).reshape(-1), np.arange(c)] = val
    return q, k, v


def p_plane_live(ref_p, v, n_head):
    """[n, nq, c] mask of the outputs whose probability p(i, kappa(c)) exceeds 2^-20"""
    n, nk, c = v.shape
    kap = kappa(n_head, c // n_head, nk)
    live = unheads(np.stack([ref_p[:, h][:, :, kap[h]] for h in range(n_head)], axis=1)) > 2.0 ** -20      # [n, h, nq, d] -> [n, nq, c]
    assert live.mean() > 0.5
    return live


def p_plane_stats(got, ref_out, live, n_head, tail=False):
    """(max, rms) of |got - ref| / |ref| over the live outputs (p_plane_live); tail: over columns 32 .. 39 of every head (d = 40) alone"""
    c = got.shape[2]
    assert np.isfinite(got).all(), "non-finite output"
    if tail:
        live = live & (np.arange(c) % (c // n_head) >= 32)[None, None, :]
    rel = np.abs(np.asarray(got, np.float64) - ref_out)[live] / np.abs(ref_out[live])
    return float(rel.max()), float(np.sqrt(np.mean(rel * rel)))


def qk_plane_probe(g, n, nq, nk, n_head, d):
    """Large common-mode scores.  The keys come in pairs (2 t, 2 t + 1) and query i aims at pair t(i) = (5 i + 1) mod (nk / 2): its scores with the two keys of the pair
    are both about +30 (natural-log units) and differ by a few units (standard deviation 1.2).  v = 1 on the keys with j + c even, 0 on the others, so the output is a
    softmax weight between keys that all score +30: the +30 cancels, a score error of 2^-17 |q| |k| does not.
    Each key carries its +30 in TWO columns alone (amplitude +-9.7 at d = 40, varying by +-5 % per element) -- few, large terms, so that one missing 2^-16 term is
    not averaged away.  Every key has its own pair of columns, the two keys of a pair share none -- their errors do not cancel each other, whichever operand's low plane
    is lost -- and the query holds the four columns of its pair.  A key that shares one column with the query scores +15 and drops out; one that happens to hold a
    column of each of the pair's keys with the right signs scores +30 as well and joins the softmax, which the reference computes like everything else.  The column
    pairs go round every column of the head, columns 32 .. 39 included; the other columns of q and k hold noise of a tenth of the size.  Every value is a full 24-bit
    number.  -> q, k, v"""
    allp = np.array([(a, b) for a in range(d) for b in range(a + 1, d)])
    assert nk % 2 == 0 and nk <= len(allp) // 2
    c, pairs = n_head * d, nk // 2
    amp = math.sqrt(30.0 * math.sqrt(d) / 2.0)                                   # amp^2 . 2 / sqrt(d) = 30
    order = [tuple(pr) for pr in allp[g.permutation(len(allp))]]
    cols_of, fresh = [], set(range(d))
    for j in range(nk):          # the next unused column pair -- one with a column no key holds yet while there are such, and for an odd key one that shares none with key j - 1
        pick = next(i for i, pr in enumerate(order) if (not fresh or set(pr) & fresh) and (j % 2 == 0 or not set(pr) & set(cols_of[j - 1])))
        cols_of.append(order.pop(pick))
        fresh -= set(cols_of[-1])
    cols_of = np.array(cols_of)                                                  # [nk, 2]
    assert len(np.unique(cols_of)) == d, "a column carries no key's common mode"
    t_of = (5 * np.arange(nq) + 1) % pairs
    noise = lambda rows: 0.1 * amp * np.clip(g.standard_normal((rows, d)), -2.5, 2.5)
    big = lambda sg: amp * sg * (1 + 0.05 * g.uniform(-1, 1, sg.shape))
    rk, rq = np.arange(nk)[:, None], np.arange(nq)[:, None]
    qh = np.empty((n, n_head, nq, d))
    kh = np.empty((n, n_head, nk, d))
    for b in range(n):
        for h in range(n_head):
            sgn = g.choice(np.array([-1.0, 1.0]), (nk, 2))
            kh[b, h] = noise(nk)
            kh[b, h][rk, cols_of] = big(sgn)
            qh[b, h] = noise(nq)
            for key in (2 * t_of, 2 * t_of + 1):
                qh[b, h][rq, cols_of[key]] = big(sgn[key])
    q, k = unheads(qh).astype(np.float32), unheads(kh).astype(np.float32)
    v = ((np.arange(nk)[:, None] + np.arange(c)[None, :]) % 2 == 0).astype(np.float32)
    return q, k, np.ascontiguousarray(np.broadcast_to(v, (n, nk, c)))


def abs_stats(got, ref64):
    """(max, rms) of |got - ref64|"""
    assert np.isfinite(got).all(), "non-finite output"
    e = np.abs(np.asarray(got, np.float64) - ref64)
    return float(e.max()), float(np.sqrt(np.mean(e * e)))


# ---- cases: inputs, references and bars, computed once and left unchanged --------------------------------------------------------------------------------------------
FACTOR = 3.0          # a ratio bar = FACTOR x what the plain fp32 evaluation of the same inputs reaches
_CASES = {}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def exact_conv_case(family, cin, k, stride, ups, set_index, n=1, h=17, w=19, cout=336):
    """(x, weight, float64 reference) of one exact probe: the one-hot weight set set_index of a family on a convolution"""
    key = ("exact conv", family, cin, k, stride, ups, set_index, n, h, w, cout)
    if key not in _CASES:
        g = np.random.default_rng(_seed(key))
        x, val = family_operands(g, family, (n, cin, h, w), cout)
        pos = onehot_positions(cout, cin * k * k, set_index)
        wt = onehot_conv_weight(pos, val, cin, k)
        ref = onehot_conv_ref(x, pos, val, k, stride, ups)
        _frozen(x, wt, ref)
        _CASES[key] = (x, wt, ref)
    return _CASES[key]


def exact_linear_case(family, cin, set_index, rows=323, cout=336):
    """(x [rows, cin], weight [cin, cout], float64 reference) of one exact probe on a Linear layer"""
    key = ("exact linear", family, cin, set_index, rows, cout)
    if key not in _CASES:
        g = np.random.default_rng(_seed(key))
        x, val = family_operands(g, family, (rows, cin), cout)
        pos = onehot_positions(cout, cin, set_index)
        wt = onehot_linear_weight(pos, val, cin)
        ref = x.astype(np.float64)[:, pos] * val.astype(np.float64)[None, :]
        _frozen(x, wt, ref)
        _CASES[key] = (x, wt, ref)
    return _CASES[key]


def exact_pair_case(family, k_main, k_aux, set_index, conv, cout=112, n=1, h=17, w=19):
    """A paired launch (op_conv2d_pair: conv3x3(hh, w_main) + conv1x1(x, w_aux), k_main = cout; op_linear_pair: u @ w_main + hh @ w_aux) whose every output is still ONE
    product: the odd output channels take theirs from the AUXILIARY problem -- operands of the given family, so the 24-bit ones sit in the shortcut's planes -- and have
    no main weight; the even ones take a family C product from the main problem and have no auxiliary weight.  -> (main input, aux input, w_main, w_aux, float64 reference)"""
    key = ("exact pair", family, k_main, k_aux, set_index, conv, cout, n, h, w)
    if key not in _CASES:
        g = np.random.default_rng(_seed(key))
        odd = np.arange(cout) % 2 == 1

        def half(K, which):      # the positions of the channels that use this problem: weight sets 0 .. weight_sets(cout / 2, K) - 1 select every one of its K
            pos = np.zeros(cout, np.int64)
            pos[which] = onehot_positions(cout // 2, K, set_index)
            return pos
        if conv:
            xm, vm = family_operands(g, "C", (n, k_main, h, w), cout)
            xa, va = family_operands(g, family, (n, k_aux, h, w), cout)
            pm, pa = half(k_main * 9, ~odd), half(k_aux, odd)
            vm[odd], va[~odd] = 0.0, 0.0
            wm, wa = onehot_conv_weight(pm, vm, k_main, 3), onehot_conv_weight(pa, va, k_aux, 1)
            ref = onehot_conv_ref(xm, pm, vm, 3) + onehot_conv_ref(xa, pa, va, 1)
        else:
            rows = n * h * w
            xm, vm = family_operands(g, "C", (rows, k_main), cout)
            xa, va = family_operands(g, family, (rows, k_aux), cout)
            pm, pa = half(k_main, ~odd), half(k_aux, odd)
            vm[odd], va[~odd] = 0.0, 0.0
            wm, wa = onehot_linear_weight(pm, vm, k_main), onehot_linear_weight(pa, va, k_aux)
            ref = xm.astype(np.float64)[:, pm] * vm.astype(np.float64)[None, :] + xa.astype(np.float64)[:, pa] * va.astype(np.float64)[None, :]
        _frozen(xm, xa, wm, wa, ref)
        _CASES[key] = (xm, xa, wm, wa, ref)
    return _CASES[key]


DENSE_CASES = ((32, 1), (64, 1), (32, 3))          # (cin, k): K = 32, 64 and 288


def dense_case(cin, k, n=1, h=17, w=19, cout=336):
    """A dense probe: x, weight, the float64 reference and sum_k |a_k| |w_k| (both [n, cout, h, w]), the GEMM operands a [M, K] and wm [N, K], and the (max, rms) rho
    of the plain fp32 evaluation -- FACTOR times which is the bar"""
    key = ("dense", cin, k, n, h, w, cout)
    if key not in _CASES:
        g = np.random.default_rng(_seed(key))
        x, wt = dense_conv_inputs(g, n, cin, h, w, cout, k)
        a, wm = im2col(x, k), wt.reshape(cout, -1).astype(np.float64)
        ref = rows_to_nchw(a @ wm.T, n, h, w)
        denom = rows_to_nchw(np.abs(a) @ np.abs(wm).T, n, h, w)
        plain = rho_stats(rows_to_nchw(fp32_sequential(a, wm), n, h, w), ref, denom)
        _frozen(x, wt, a, wm, ref, denom)
        _CASES[key] = dict(x=x, wt=wt, a=a, wm=wm, ref=ref, denom=denom, plain=plain, K=cin * k * k, shape=(n, h, w))
    return _CASES[key]


def _fp32_attention(q, k, v, n_head):
    """the plain fp32 CPU evaluation: oracle.sd_oracle.qkv_attention on float32 tensors"""
    import torch

    from oracle import sd_oracle as O
    return O.qkv_attention(torch.tensor(q), torch.tensor(k), torch.tensor(v), None, n_head).numpy()


def attention_case(kind, n, nq, nk, n_head, d):
    """kind 'v': q, k, v and the expected rows (bar: 4 ulp, derived -- no reference evaluation); 'p' / 'qk': q, k, v, the float64 output, and the statistics (attention_stats) of
    the plain fp32 CPU evaluation -- FACTOR times which are the bars"""
    key = ("attention", kind, n, nq, nk, n_head, d)
    if key not in _CASES:
        g = np.random.default_rng(_seed(key))
        if kind == "v":
            q, k, v, want = v_plane_probe(g, n, nq, nk, n_head, d)
            _frozen(q, k, v, want)
            _CASES[key] = dict(q=q, k=k, v=v, ref=want)
        else:
            q, k, v = (p_plane_probe if kind == "p" else qk_plane_probe)(g, n, nq, nk, n_head, d)
            ref, prob = attention_ref64(q, k, v, n_head)
            case = dict(q=q, k=k, v=v, ref=ref)
            if kind == "p":
                case["live"] = p_plane_live(prob, v, n_head)
            case["plain"] = attention_stats(kind, _fp32_attention(q, k, v, n_head), case, n_head)
            _frozen(q, k, v, ref)
            _CASES[key] = case
    return _CASES[key]


def attention_stats(kind, got, case, n_head):
    """the statistics of a 'p' or 'qk' case, {name: value}.  Asserted against FACTOR x the plain evaluation's: 'qk max', 'qk rms', 'p rms' and, at d = 40, 'p tail rms'
    (columns 32 .. 39 alone).  'p max' is reported only: a missing p_l.v_h moves it to 1.8 x its bar at d = 64 (tests/test_precision_probes_cpu.py), not the 2 x a bar
    must keep from every mutation -- the largest relative error of the plain evaluation sits in its smallest probabilities, where a score error counts in full."""
    if kind == "qk":
        return dict(zip(("qk max", "qk rms"), abs_stats(got, case["ref"])))
    out = dict(zip(("p max", "p rms"), p_plane_stats(got, case["ref"], case["live"], n_head)))
    if got.shape[2] // n_head == 40:
        out["p tail rms"] = p_plane_stats(got, case["ref"], case["live"], n_head, tail=True)[1]
    return out


ASSERTED = ("qk max", "qk rms", "p rms", "p tail rms")
