"""Web-UI prompt encoding, the host side: sdmi_prompt_parse and sdmi_prompt_chunks through the C ABI against the pinned table of the
web UI's parser and against tests/prompt_ref.py, the same code under AddressSanitizer / UBSan in a stand-alone driver (tests/san/prompt_main.cpp, its own
process, nothing preloaded), and two facts about the oracle-side reference the GPU tests lean on.  No device is needed."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import prompt_ref as R

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "stable_diffusion_burn_amd" / "csrc"
MINI = ROOT / "tests" / "golden" / "mini_merges.txt"
MINI_VOCAB = 512 + 264 + 2
CTX = 16   # the tiny model of test_clip_gpu.py: L = 14 content positions


@pytest.fixture(scope="module")
def lib():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)
    from stable_diffusion_burn_amd import _capi
    return _capi.load_library()


@pytest.fixture(scope="module")
def tok(lib):
    from stable_diffusion_burn_amd import SimpleTokenizer
    return SimpleTokenizer(MINI)


def test_symbols_exported_and_bound(lib):
    from stable_diffusion_burn_amd import _capi
    for s in ("sdmi_prompt_parse", "sdmi_prompt_chunks", "sdmi_clip_forward_ex", "sdmi_embedding_add", "sdmi_embedding_load_safetensors", "sdmi_embedding_remove",
              "sdmi_embedding_list", "sdmi_encode_prompt"):
        assert s in _capi.SIGNATURES and getattr(lib, s).argtypes == _capi.SIGNATURES[s][1], s
    header = (ROOT / "include" / "sdmi.h").read_text()
    assert "sdmi_prompt_opts" in header and (ROOT / "ffi" / "sdmi.rs").read_text().count("fn sdmi_encode_prompt") == 1


@pytest.mark.parametrize("text,expect", R.PARSE_TABLE, ids=[repr(t) for t, _ in R.PARSE_TABLE])
def test_parse_table(lib, text, expect):
    """the web UI's own docstring cases and the other pinned ones, exact in f64"""
    from stable_diffusion_burn_amd import parse_prompt
    got = parse_prompt(text)
    assert got == [(t, float(w)) for t, w in expect]
    assert R.parse_prompt(text) == got


@pytest.mark.parametrize("text,offending", R.BAD_WEIGHTS)
def test_bad_weight_is_invalid(lib, text, offending):
    from stable_diffusion_burn_amd import SdmiError, parse_prompt
    with pytest.raises(SdmiError) as ei:
        parse_prompt(text)
    assert ei.value.status == -1 and f"'{offending}'" in str(ei.value)
    with pytest.raises(ValueError):
        R.parse_prompt(text)
    bare = text.replace("(", "")
    assert parse_prompt(bare) == R.parse_prompt(bare) == [(bare, 1.0)]   # without an open round span the same characters are text


def test_parse_fuzz_against_reference(lib):
    from stable_diffusion_burn_amd import SdmiError, parse_prompt
    strings = R.fuzz_strings()
    assert len(strings) == 2000 and set("".join(strings)) <= set(R.FUZZ_ALPHABET + "a")
    errors = 0
    for s in strings:
        try:
            ref = R.parse_prompt(s)
        except ValueError:
            ref = None
        try:
            got = parse_prompt(s)
        except SdmiError as e:
            assert e.status == -1
            got = None
        assert got == ref, repr(s)
        errors += ref is None
    assert 0 < errors < 200   # both outcomes occur


def test_parse_text_query_convention(lib):
    import ctypes as C
    need = C.c_size_t()
    assert lib.sdmi_prompt_parse(b"a (b)", None, 0, C.byref(need)) == 0 and need.value == len(b"1\ta \n1.1000000000000001\tb\n") + 1
    buf = C.create_string_buffer(4)
    assert lib.sdmi_prompt_parse(b"a (b)", buf, 4, C.byref(need)) == -1
    assert lib.sdmi_prompt_parse(None, None, 0, C.byref(need)) == -1


def _content(n):
    """a prompt of exactly n content tokens in the mini vocabulary ("a" is one token)"""
    return " ".join(["a"] * n)


CHUNK_CASES = {
    "empty": dict(text=""),
    "14 tokens": dict(text=_content(14)),
    "15 tokens": dict(text=_content(15)),
    "31 tokens": dict(text=_content(31)),
    "break": dict(text="a cat BREAK a (dog:2)"),
    "break twice": dict(text="a BREAK BREAK b"),
    "break last": dict(text="a BREAK"),
    "break after a full chunk": dict(text=_content(14) + " BREAK b"),
    "min_chunks": dict(text="a photo", min_chunks=3),
    "no emphasis": dict(text="a (photo:1.3) [of] BREAK \\(x", emphasis=False),
    "emphasis": dict(text="a (photo:1.3) [of] (((a))) (cat:-0.5) (b:0)"),
    "embedding first": dict(text="zx of a cat", embeddings=[("zx", 3)]),
    "embedding ends at 14": dict(text=_content(11) + " (zx:1.2) b", embeddings=[("zx", 3)]),
    "embedding spills": dict(text=_content(12) + " zx b", embeddings=[("zx", 3)]),
    "embedding of 14 after one token": dict(text="a zx", embeddings=[("q", 2), ("zx", 14)]),
    "longer name wins": dict(text="zx q zx", embeddings=[("zx", 2), ("zx q", 3)]),
    "longer name wins, listed first": dict(text="zx q zx", embeddings=[("zx q", 3), ("zx", 2)]),
    "no match inside a word": dict(text="cats cat", embeddings=[("cat", 2)]),
}


@pytest.mark.parametrize("case", CHUNK_CASES, ids=list(CHUNK_CASES))
def test_chunks_against_reference(tok, case):
    kw = dict(emphasis=True, min_chunks=1, embeddings=())
    kw.update(CHUNK_CASES[case])
    text = kw.pop("text")
    ids, w, rows = tok.prompt_chunks(text, CTX, **kw)
    rids, rw, rrows = R.prompt_chunks(tok.encode, MINI_VOCAB - 2, MINI_VOCAB - 1, text, CTX, **kw)
    np.testing.assert_array_equal(ids, rids)
    np.testing.assert_array_equal(w, rw)
    np.testing.assert_array_equal(rows, rrows)
    # start, end and padding positions: weight exactly 1, no bank row
    assert (ids[:, 0] == MINI_VOCAB - 2).all() and (ids[:, -1] == MINI_VOCAB - 1).all()
    for k in range(len(ids)):
        content = int((rows[k] >= 0).sum() + ((ids[k, 1:] != MINI_VOCAB - 1) & (rows[k, 1:] < 0)).sum())
        assert (w[k, 0] == 1.0) and (w[k, 1 + content:] == 1.0).all() and (rows[k, 1 + content:] == -1).all() and (ids[k, 1 + content:] == MINI_VOCAB - 1).all()


def test_chunk_counts_and_rows(tok):
    """the shapes the cases above are there for, spelled out (so that a reference wrong in the same way does not hide them)"""
    k = lambda text, **kw: tok.prompt_chunks(text, CTX, **kw)
    assert len(tok.encode("a")) == 1 and len(tok.encode("b")) == 1 and tok.encode("zx q")[:2] == tok.encode("zx") and tok.encode("cats")[0] != tok.encode("cat")[0]
    ids, w, rows = k("")
    assert ids.tolist() == [[MINI_VOCAB - 2] + [MINI_VOCAB - 1] * 15]
    assert [len(k(_content(n))[0]) for n in (14, 15, 28, 29, 31)] == [1, 2, 2, 3, 3]
    assert len(k("a BREAK BREAK b")[0]) == 3 and (k("a BREAK BREAK b")[0][1, 1:] == MINI_VOCAB - 1).all()
    assert len(k("a BREAK")[0]) == 1 and len(k("a cat BREAK a (dog:2)")[0]) == 2
    assert len(k("a photo", min_chunks=3)[0]) == 3 and len(k(_content(31), min_chunks=2)[0]) == 3
    assert k("a (b:2)")[1][0, :4].tolist() == [1.0, 1.0, 2.0, 1.0]
    assert k("zx of", embeddings=[("zx", 3)])[2][0, :5].tolist() == [-1, 0, 1, 2, -1]
    ids, w, rows = k(_content(11) + " (zx:1.2) b", embeddings=[("zx", 3)])
    assert len(ids) == 2 and rows[0, 12:15].tolist() == [0, 1, 2] and w[0, 12:15].tolist() == [np.float32(1.2)] * 3 and (ids[0, 12:] == MINI_VOCAB - 1).all()
    ids, w, rows = k(_content(12) + " zx b", embeddings=[("zx", 3)])
    assert (rows[0] == -1).all() and rows[1, 1:4].tolist() == [0, 1, 2] and ids[0, 13] == MINI_VOCAB - 1
    assert k("zx q zx", embeddings=[("zx", 2), ("zx q", 3)])[2][0, :7].tolist() == [-1, 2, 3, 4, 0, 1, -1]
    assert (k("cats", embeddings=[("cat", 2)])[2] == -1).all() and (k("cat", embeddings=[("cat", 2)])[2][0, 1:3] >= 0).all()


def test_chunk_errors(tok):
    from stable_diffusion_burn_amd import SdmiError
    for kw in (dict(embeddings=[("", 1)]), dict(embeddings=[("   ", 1)]), dict(embeddings=[("zx", 0)]), dict(embeddings=[("zx", 15)]), dict(min_chunks=-1)):
        with pytest.raises(SdmiError) as ei:
            tok.prompt_chunks("a", CTX, **kw)
        assert ei.value.status == -1, kw
    with pytest.raises(SdmiError):
        tok.prompt_chunks("a", 2)
    with pytest.raises(SdmiError):
        tok.prompt_chunks("(a:.)", CTX)
    assert len(tok.prompt_chunks("(a:.)", CTX, emphasis=False)[0]) == 1
    import ctypes as C
    n = C.c_int32(-7)
    st = tok._lib.sdmi_prompt_chunks(tok._tok, _content(31).encode(), CTX, 1, 1, None, None, 0, None, None, None, 0, C.byref(n))
    assert st == -1 and n.value == 3   # *n_chunks is always set


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_parser_and_chunker_under_sanitizers(tmp_path):
    cases = [(t, R.serialise(e)) for t, e in R.PARSE_TABLE] + [(t, "ERR") for t, _ in R.BAD_WEIGHTS]
    for s in R.fuzz_strings():
        try:
            cases.append((s, R.serialise(R.parse_prompt(s))))
        except ValueError:
            cases.append((s, "ERR"))
    cases += [(c["text"], R.serialise(R.parse_prompt(c["text"]))) for c in CHUNK_CASES.values()]
    (tmp_path / "cases.txt").write_text("".join(f"{t.encode().hex()}\n{e.encode().hex()}\n" for t, e in cases))
    exe = tmp_path / "prompt_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "san" / "prompt_main.cpp"), str(CSRC / "prompt.cpp"), str(CSRC / "tokenizer.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt"), str(MINI)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip() == f"{len(cases)} cases, 0 differ"


def test_oracle_emphasis_is_far_above_the_gpu_bars():
    """What the GPU tests compare with: on their inputs the weighting moves the output by more than 100 x the parity bar (2e-5 max(1, |ref|)), so a kernel that
    skipped it could not pass; with all weights 1 it is the identity; CLIP skip and a bank row move the output as far."""
    from oracle import clip_oracle as CO
    from stable_diffusion_burn_amd import synthetic as syn
    dims = CO.ClipDims(n_vocab=MINI_VOCAB, n_state=64, n_head=1, n_ctx=CTX, n_layer=2)
    clip = CO.CLIPOracle(syn.SyntheticWeights(), dims, torch.float64)
    tokens, w = R.emphasis_inputs(MINI_VOCAB, CTX)
    z = clip.forward(tokens)
    np.testing.assert_array_equal(R.clip_forward_ex(clip, tokens).numpy(), z.numpy())
    np.testing.assert_array_equal(R.reweight(z, np.ones_like(w)).numpy(), z.numpy())
    out = R.clip_forward_ex(clip, tokens, weights=w)
    bar = 2e-5 * max(1.0, float(z.abs().max()))
    np.testing.assert_array_equal(out[1].numpy(), z[1].numpy())          # the chunk whose weights are all 1
    for k in (0, 2):
        assert float((out[k] - z[k]).abs().max()) >= 100 * bar
        assert abs(float(out[k].sum()) - float(z[k].sum())) <= 1e-9 * float(z[k].abs().sum())   # the chunk keeps its sum: what the factor is for
    assert float((R.clip_forward_ex(clip, tokens, clip_skip=2) - z).abs().max()) >= 100 * bar
    bank = np.asarray(clip._table("token_embedding", MINI_VOCAB)[[5, 6]])
    rows = np.full(tokens.shape, -1, np.int32)
    rows[0, 1] = 1
    assert float((R.clip_forward_ex(clip, tokens, rows, bank) - z)[0].abs().max()) >= 100 * bar
    tok2 = tokens.copy()
    tok2[0, 1] = 6
    np.testing.assert_array_equal(R.clip_forward_ex(clip, tokens, rows, bank).numpy(), clip.forward(tok2).numpy())
    z32 = z.numpy().astype(np.float32)
    assert np.abs(R.reweight_f32_model(z32, w) - R.reweight(torch.from_numpy(z32).double(), w).numpy()).max() <= 4 * 2.0 ** -24 * np.abs(out.numpy()).max()
    assert (R.reweight_f32_model(z32, np.zeros_like(w)) == 0).all()
