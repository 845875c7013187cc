"""qkv_attention fed the way the model feeds it -- q, k and v as column slices of one packed [n][T][3C] buffer (the UNet's self attention, every CLIP layer) or of
buffers with strides of their own (cross attention's context K / V), the result written into a slice -- through sdmi_op_qkv_attention_view, which scatters the
dense operands into parents full of NaN and calls Engine::attention with the slices' bases, row strides and batch strides.

Every other operator-level attention test hands the kernels dense [n, rows, n_state] tensors: all four row strides equal, every batch stride = rows * ld.  A kernel
that took ldv for ldk, nk * ldk for k_bs or q_bs for o_bs passes all of them.  Here the layouts of tests/attn_view_cases.py (model_self: the model's buffer exactly;
packed_gaps: gaps between the slices and filler rows behind each sample; apart: eight pairwise different strides) run over that module's table: k_attn.hip,
k_attn_split.hip and k_attn_bf16.hip in their 4- (2-) and 8-wave forms, key slices and the merge launch, the plane-writing epilogue, the masked instance, CLIP's
own shape, per-sample key counts, and the unfused GEMM path (a_ld, b_ld, transpose2d's src_ld, ldc).

Per case, in this order:
 1. sdmi_attention_plan under the case's options names the kernel, wave count, query rows and key-slice count the table row states (asserted; the same table is
    replayed on the host-only planner by tests/test_attention_views_cpu.py);
 2. the result is finite: nothing outside a slice and no key behind a kv_len was read;
 3. the slice IS the dense entry's result (sdmi_qkv_attention / sdmi_op_qkv_attention_ragged, same context, same options), bit for bit: the plan takes no stride
    and the fused kernels' arithmetic does not depend on where a row starts, so any difference is an addressing bug.  On the unfused path this holds where option
    dump_choices records the same GEMM launches for both calls (as tests/test_views_gpu.py does it);
 4. the slice is within the operator bars of oracle.sd_oracle.qkv_attention in float64 on each sample's own keys: 2e-5 max(1, max|ref|) at fp32
    (test_ops_gpu.RTOL), 2^-7 at bf16 fused, 2^-6 at bf16 unfused (test_bf16_gpu.py), per sample;
 5. every cell of the output parent outside the slice -- margin columns, the extra rows of every sample -- still holds its prefill, bit for bit.
"""
import numpy as np
import pytest

import attn_view_cases as V

pytestmark = pytest.mark.gpu

FP32_BAR = 2e-5                                 # test_ops_gpu.py RTOL
BF16_BAR, BF16_BAR_UNFUSED = 2 ** -7, 2 ** -6   # test_bf16_gpu.py: fused / unfused (bf16 probabilities)
SDMI_ERR_INVALID = -1


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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _recorded(sd, tmp_path, name, fn):
    """fn() -> (result, the GEMM launches it made: dump_choices lines)"""
    path = tmp_path / name
    try:
        sd.set_option("record_shapes", 1)
        out = fn()
        sd.set_option("dump_choices", str(path))
    finally:
        sd.set_option("record_shapes", 0)
    return out, path.read_text().splitlines()


def _view_args(lay):
    return dict(q_view=tuple(lay.q), k_view=tuple(lay.k), v_view=tuple(lay.v), packed=lay.packed, out_off=lay.out.off)


def _check_rows(got, ref, counts, what, bar):
    """bar x max(1, max|ref|) per sample, as test_attention_ragged_gpu._check_rows; prints the worst sample"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref).max(axis=(1, 2))
    bound = bar * np.maximum(1.0, np.abs(ref).max(axis=(1, 2)))
    w = int(np.argmax(err / bound))
    print(f"{what}: worst sample {w}{'' if counts is None else f' (kv_len {counts[w]})'}: max|d| = {err[w]:.3e}, bar {bound[w]:.3e}")
    over = err > bound
    assert not over.any(), f"{what}: samples {np.flatnonzero(over).tolist()} over the bar; worst {w}: max|d| = {err[w]:.3e} > {bound[w]:.3e}"


def _run_case(sd, tmp_path, row, layout):
    nq, nk = V.shape(row, layout)
    c = row.d * row.heads
    lay = V.layout_of(row, layout)
    counts = V.kv_counts(row)
    kv = None if counts is None else np.asarray(counts, np.int32)
    what = V.case_id(row, layout)
    opts = dict(row.opts)
    if row.precision == 0:
        opts["gemm_planes"] = row.planes
    q, k, v, kn, vn, mask, ref = V.case_data(row, layout)
    pre = V.prefill(lay, row.n, V.storage_bf16(row))
    try:
        for key, val in opts.items():
            sd.set_option(key, val)
        # 1. the case reaches the form its row names
        plan = sd.attention_plan(row.n, row.heads, nq, nk, row.d, mask is not None)
        want = {"kernel": row.kernel, "waves": row.waves, "q_rows": row.q_rows, "kv_splits": V.expected_slices(row, layout)}
        assert {key: plan[key] for key in want} == want, f"{what}: the table row does not reach its form: planned {plan}, the table says {want}"
        dense_call = (lambda: sd.qkv_attention(q, k, v, mask, row.heads)) if kv is None else (lambda: sd.qkv_attention_ragged(q, kn, vn, kv, row.heads))
        view_call = lambda: sd.op_qkv_attention_view(q, kn, vn, mask, row.heads, kv, parent=pre, out_planes=row.planes, **_view_args(lay))
        if row.kernel == "unfused":
            dense, dense_gemms = _recorded(sd, tmp_path, "dense.txt", dense_call)
            got, view_gemms = _recorded(sd, tmp_path, "view.txt", view_call)
            assert dense_gemms and view_gemms, f"{what}: no GEMM launch recorded"
        else:
            dense, got = dense_call(), view_call()
            dense_gemms = view_gemms = None
    finally:
        for key in opts:
            sd.set_option(key, V.OPTION_DEFAULTS[key])
    assert got.shape == pre.shape
    sl = V.out_slice(lay, got, nq, c)
    # 2. finite
    bad = ~np.isfinite(sl).all(axis=(1, 2))
    assert not bad.any(), f"{what}: non-finite output in samples {np.flatnonzero(bad).tolist()}: a cell outside a slice, or a key behind a sample's count, was read"
    # 3. bit for bit the dense entry
    diff = _bits(sl) != _bits(dense)
    print(f"{what}: {int(diff.sum())} of {diff.size} elements differ from the dense entry" + (f"; max|d| = {np.abs(sl.astype(np.float64) - dense).max():.3e}" if diff.any() else ""))
    if dense_gemms is None or dense_gemms == view_gemms:
        where = np.argwhere(diff)[:5].tolist()
        assert not diff.any(), f"{what}: {int(diff.sum())} elements differ from the dense entry on the same operands (first at [sample, row, column] {where}): an addressing bug"
    else:
        print(f"{what}: the GEMM launches differ (dense {dense_gemms}, view {view_gemms}): the oracle bar only")
    # 4. the oracle
    bar = FP32_BAR if not V.storage_bf16(row) else BF16_BAR_UNFUSED if row.kernel == "unfused" else BF16_BAR
    _check_rows(sl, ref, counts, what, bar)
    # 5. nothing outside the slice was written
    outside = np.ones(pre.shape, bool)
    outside[:, :nq, lay.out.off:lay.out.off + c] = False
    touched = outside & (_bits(got) != _bits(pre))
    assert not touched.any(), f"{what}: {int(touched.sum())} cells outside the output slice were written (first at [sample, row, column] {np.argwhere(touched)[:5].tolist()})"


CASES = V.cases()


@pytest.mark.parametrize("row,layout", CASES, ids=[V.case_id(r, lay) for r, lay in CASES])
def test_attention_on_views(ops32, ops16, tmp_path, row, layout):
    _run_case(ops16 if row.precision else ops32, tmp_path, row, layout)


@pytest.mark.parametrize("precision", [0, 1])
def test_bad_attention_views_are_refused_before_anything_runs(ops32, ops16, tmp_path, precision):
    """every refusal of sdmi_op_qkv_attention_view is SDMI_ERR_INVALID from the host-side check, the parent comes back untouched, and the same context then
    passes an ordinary case"""
    from stable_diffusion_burn_amd import SdmiError
    sd = ops16 if precision else ops32
    n, nq, nk, heads, c, es = 2, 100, 520, 2, 80, 2 if precision else 4
    q, k, v, _, _, _, _ = V.data(n, nq, nk, c, heads, None, "bf16" if precision else "f32", None)
    cases = [(name, lay, 0) for name, lay in V.refusals(nq, nk, c, es)] + [(V.PLANES_REFUSALS[0], V.apart(nq, nk, c, es), 1)]
    for name, lay, planes in cases:
        pre = V.prefill(lay, n, bool(precision))
        with pytest.raises(SdmiError) as ei:
            sd.op_qkv_attention_view(q, k, v, None, heads, parent=pre, out_planes=planes, **_view_args(lay))
        assert ei.value.status == SDMI_ERR_INVALID and "attention view" in str(ei.value), f"{name}: {ei.value}"
        assert np.array_equal(_bits(ei.value.parent), _bits(pre)), name
    _run_case(sd, tmp_path, V.BY_ID["bf16-d40-variant-default-small" if precision else "split-d40-pack3-small"], "apart")
