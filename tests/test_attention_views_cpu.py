"""The table of tests/test_attention_views_gpu.py (tests/attn_view_cases.py), checked without a GPU.

1. The layouts in numpy: scattering q, k, v into their parents and gathering them again returns them, no two slices share a cell, every other cell holds the
   filler, and `apart` really has eight different strides.
2. The host-only planner and view validator (csrc/attn_plan.cpp), built with tests/san/attn_plan_main.cpp as tests/test_attn_plan_cpu.py builds it (g++ with the
   address and undefined-behaviour sanitizers, no HIP): every row of the table gets the kernel, workgroup form and key-slice count it names under its options,
   every layout it runs under passes check_attention_view, and every refusal case is refused with SDMI_ERR_INVALID.  The driver's own accept / refuse cases
   (view_selftest) run with test_attn_plan_cpu.py's fixture replay.
"""
import shutil
import subprocess

import numpy as np
import pytest

import attn_view_cases as V
from test_attn_plan_cpu import _build

SDMI_ERR_INVALID = -1
SHAPES = [(2, 100, 520, 80), (2, 100, 100, 80), (3, 77, 77, 768), (2, 7, 9, 64)]     # n, nq, nk, C


@pytest.mark.parametrize("es", [4, 2])
@pytest.mark.parametrize("name", list(V.LAYOUTS))
def test_layout_round_trip(name, es):
    for n, nq, nk, c in SHAPES:
        if name == "model_self" and nq != nk:
            continue
        lay = V.LAYOUTS[name](nq, nk, c, es)
        g = np.random.default_rng(n * nq + nk)
        q = g.standard_normal((n, nq, c)).astype(np.float32)
        k, v = (g.standard_normal((n, nk, c)).astype(np.float32) for _ in range(2))
        parents = V.scatter(lay, q, k, v, fill=np.nan)
        for got, want in zip(V.gather(lay, parents, nq, nk, c), (q, k, v)):
            np.testing.assert_array_equal(got, want)
        cover = V.cover(lay, n, nq, nk, c)
        for w in "qkv":
            assert cover[w].max() == 1, f"{name}: slices overlap in the parent of {w}"
            assert np.isnan(parents[w][cover[w] == 0]).all() and np.isfinite(parents[w][cover[w] == 1]).all(), f"{name}: {w}"
        assert (parents["q"] is parents["k"]) == lay.packed
        for s, rows in ((lay.q, nq), (lay.k, nk), (lay.v, nk), (lay.out, nq)):
            assert s.off >= 0 and s.off + c <= s.ld and s.rows >= rows and s.ld % V.gap(es) == 0 and s.off % V.gap(es) == 0
        pre = V.prefill(lay, n, es == 2)
        assert pre.shape == (n, lay.out.rows, lay.out.ld) and (pre < -1).all()
        if es == 2:
            np.testing.assert_array_equal(pre, V.bf16_round(pre))
        else:
            assert len(np.unique(pre)) == min(pre.size, 65521)


@pytest.mark.parametrize("es", [4, 2])
def test_layouts_are_what_they_claim(es):
    for n, nq, nk, c in SHAPES:
        g = V.gap(es)
        d = V.dense(nq, nk, c, es)
        assert V.strides(d) == [c, c, c, c, nq * c, nk * c, nk * c, nq * c] and not d.packed
        a = V.apart(nq, nk, c, es)
        assert len(set(V.strides(a))) == 8, (nq, nk, c, V.strides(a))
        assert len({a.q.off, a.k.off, a.v.off}) == 3 and len({a.q.rows, a.k.rows, a.v.rows}) == 3 and not a.packed
        p = V.packed_gaps(nq, nk, c, es)
        assert p.packed and p.q.ld == 3 * c + 3 * g and p.q.rows == max(nq, nk) + 5 and (p.q.off, p.k.off - p.q.off - c, p.v.off - p.k.off - c) == (g, g, g)
        if nq == nk:
            m = V.model_self(nq, nk, c, es)
            assert m.packed and (m.q, m.k, m.v) == (V.Slice(3 * c, 0, nq), V.Slice(3 * c, c, nq), V.Slice(3 * c, 2 * c, nq)) and m.out == V.Slice(c, 0, nq)


def test_table_covers_what_it_must():
    rows = V.ROWS
    reached = {(r.kernel, r.waves) for r in rows}
    assert {("flash", 4), ("flash", 8), ("split", 4), ("split", 8), ("bf16", 2), ("bf16", 8), ("bf16", 4), ("unfused", 0)} <= reached
    assert {r.d for r in rows if r.kernel == "split"} == {40, 64, 80} and {r.d for r in rows if r.kernel == "flash"} >= {40, 64, 80, 160}
    assert {r.d for r in rows if r.kernel == "bf16"} == {40, 80, 160}
    assert {r.opts.get("attn_bf16_variant") for r in rows if r.kernel == "bf16" and not r.kv_len} == {"default", 1, 0x102, 0x104}
    assert {r.opts.get("attn_kv_splits", 0) for r in rows if r.precision == 0} >= {0, 3, 8}
    assert {r.opts.get("attn_pack_tail") for r in rows if r.d == 40 and r.kernel == "split"} >= {0, 3}
    assert any(r.planes for r in rows) and any(r.mask == "banded" for r in rows) and {r.precision for r in rows if r.mask == "causal"} == {0, 1}
    assert {r.kernel for r in rows if r.kv_len} == {"flash", "split", "bf16", "unfused"} and {V.BY_ID[i].kernel for i in V.DENSE} == {"flash", "split", "bf16", "unfused"}
    # key slices with a strided output: the merge launch writes through out_ld
    assert any(V.expected_slices(r, lay) > 1 and V.layout_of(r, lay).out.ld != r.d * r.heads for r, lay in V.cases())
    for r in rows:
        if r.kernel != "unfused":
            assert set(r.layouts) == ({"apart"} if r.kv_len else {"model_self"} if r.nq == r.nk else set(V.FUSED)), r.id
        else:
            assert set(r.layouts) == ({"apart"} if r.kv_len else {"apart", "model_self"}), r.id
        assert r.n * r.nq * r.d * r.heads <= 8 * 2085 * 640
        assert not (r.planes and (r.d * r.heads) % 32)
    ids = [V.case_id(r, lay) for r, lay in V.cases()]
    assert len(ids) == len(set(ids))


def _ask(tmp_path, lines):
    exe = _build(tmp_path)
    path = tmp_path / "views.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), "--views", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_planner_sends_every_row_to_the_form_it_names(tmp_path):
    cases = V.cases()
    got = _ask(tmp_path, [V.plan_line(r, lay) for r, lay in cases])
    bad = []
    for (r, lay), line in zip(cases, got):
        want = f"{r.kernel} {r.waves} {r.q_rows} {V.expected_slices(r, lay)}"
        if line != want:
            bad.append(f"{V.case_id(r, lay)}: the table says {want}, the planner {line}")
    assert not bad, "\n".join(bad)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_validator_takes_the_layouts_and_refuses_the_refusals(tmp_path):
    lines, want, what = [], [], []
    for r, lay in V.cases():
        nq, nk = V.shape(r, lay)
        lines.append(V.view_line(V.layout_of(r, lay), r.n, nq, nk, r.d * r.heads, V.elem_size(r), r.planes))
        want.append("ok")
        what.append(V.case_id(r, lay))
    for es in (4, 2):
        for name, lay in V.refusals(100, 520, 80, es):
            lines.append(V.view_line(lay, 2, 100, 520, 80, es))
            want.append(f"E{SDMI_ERR_INVALID}")
            what.append(f"{name} (element size {es})")
        lines.append(V.view_line(V.apart(100, 520, 160, es), 2, 100, 520, 160, es, planes=1))
        want.append(f"E{SDMI_ERR_INVALID}")
        what.append(f"{V.PLANES_REFUSALS[0]} (element size {es})")
    got = _ask(tmp_path, lines)
    bad = [f"{w}: expected {a}, got {b}" for w, a, b in zip(what, want, got) if a != b]
    assert not bad, "\n".join(bad)
