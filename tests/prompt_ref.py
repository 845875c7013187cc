"""Plain-Python restatement of the web-UI prompt encoding -- TEST INFRASTRUCTURE ONLY.

parse_prompt is the A1111 web UI's parse_prompt_attention with its regular expressions restated over ASCII classes (the C++ parser works on bytes);
prompt_chunks is its chunker without the comma backtrack; clip_forward_ex drives the CLIP oracle's own pieces (CLIPOracle._table / .block, sd_oracle.layer_norm)
with bank rows, an early stop and the emphasis weighting.  Written from the rules, not from csrc/prompt.cpp: the two are compared case by case."""
import re

import numpy as np
import torch

_RE_ATTENTION = re.compile(r"""
\\\(|
\\\)|
\\\[|
\\]|
\\\\|
\\|
\(|
\[|
:\s*([+-]?[.\d]+)\s*\)|
\)|
]|
[^\\()\[\]:]+|
:
""", re.X | re.A)
_RE_BREAK = re.compile(r"\s*\bBREAK\b\s*", re.S | re.A)


def parse_prompt(text):
    """[(fragment, weight)]; ValueError for a weight that is no complete number"""
    res, round_brackets, square_brackets = [], [], []

    def multiply_range(start, m):
        for p in range(start, len(res)):
            res[p][1] *= m

    for m in _RE_ATTENTION.finditer(text):
        tok, weight = m.group(0), m.group(1)
        if tok.startswith("\\"):
            res.append([tok[1:], 1.0])
        elif tok == "(":
            round_brackets.append(len(res))
        elif tok == "[":
            square_brackets.append(len(res))
        elif weight is not None and round_brackets:
            multiply_range(round_brackets.pop(), float(weight))
        elif tok == ")" and round_brackets:
            multiply_range(round_brackets.pop(), 1.1)
        elif tok == "]" and square_brackets:
            multiply_range(square_brackets.pop(), 1 / 1.1)
        else:
            for i, part in enumerate(_RE_BREAK.split(tok)):
                if i > 0:
                    res.append(["BREAK", -1])
                res.append([part, 1.0])
    for pos in round_brackets:
        multiply_range(pos, 1.1)
    for pos in square_brackets:
        multiply_range(pos, 1 / 1.1)
    if not res:
        res = [["", 1.0]]
    i = 0
    while i + 1 < len(res):
        if res[i][1] == res[i + 1][1]:
            res[i][0] += res[i + 1][0]
            res.pop(i + 1)
        else:
            i += 1
    return [(t, float(w)) for t, w in res]


def prompt_chunks(encode, start_token, end_token, text, clip_ctx, emphasis=True, min_chunks=1, embeddings=()):
    """ids, weights (f32), emb_row (i32), each [k, clip_ctx].  encode: text -> ids; embeddings: [(name, n_vectors)]"""
    L = clip_ctx - 2
    names, first, rows = [], [], 0
    for name, v in embeddings:
        ids = encode(name) if name else []
        if not ids or v < 1 or v > L:
            raise ValueError(f"embedding {name!r}")
        names.append((ids, v))
        first.append(rows)
        rows += v
    chunks, cur = [], []

    def close():
        ids = [start_token] + [c[0] for c in cur] + [end_token] * (L + 1 - len(cur))
        w = [1.0] + [c[1] for c in cur] + [1.0] * (L + 1 - len(cur))
        r = [-1] + [c[2] for c in cur] + [-1] * (L + 1 - len(cur))
        chunks.append((ids, w, r))
        cur.clear()

    for frag, weight in (parse_prompt(text) if emphasis else [(text, 1.0)]):
        if emphasis and frag == "BREAK" and weight == -1:
            close()
            continue
        ids = encode(frag)
        pos = 0
        while pos < len(ids):
            if len(cur) == L:
                close()
            hit = None
            for e, (nids, v) in enumerate(names):
                if ids[pos:pos + len(nids)] == nids and (hit is None or len(nids) > len(names[hit][0])):
                    hit = e
            if hit is None:
                cur.append((ids[pos], weight, -1))
                pos += 1
                continue
            nids, v = names[hit]
            if len(cur) + v > L:
                close()
            cur.extend((end_token, weight, first[hit] + j) for j in range(v))
            pos += len(nids)
    if cur or not chunks:
        close()
    while len(chunks) < min_chunks:
        close()
    return (np.array([c[0] for c in chunks], np.int32), np.array([c[1] for c in chunks], np.float32), np.array([c[2] for c in chunks], np.int32))


def reweight(z, w):
    """emphasis weighting of z [n, T, C] by w [n, T], chunk by chunk, in the dtype of z: (z w) * (sum z / sum z w); a zero weighted sum gives the factor 1"""
    z = torch.as_tensor(z)
    zw = z * torch.as_tensor(np.asarray(w), dtype=z.dtype)[:, :, None]
    s, sw = z.sum(dim=(1, 2)), zw.sum(dim=(1, 2))
    r = torch.where(sw == 0, torch.ones_like(s), s / torch.where(sw == 0, torch.ones_like(sw), sw))
    return zw * r[:, None, None]


def reweight_f32_model(z32, w32):
    """what the device kernel computes from the fp32 z it has: fl32(z w) * fl32(sum z / sum fl32(z w)), both sums in f64 over the fp32 terms"""
    z32, w32 = np.asarray(z32, np.float32), np.asarray(w32, np.float32)
    zw = (z32 * w32[:, :, None]).astype(np.float32)
    s, sw = z32.astype(np.float64).sum(axis=(1, 2)), zw.astype(np.float64).sum(axis=(1, 2))
    r = np.where(sw == 0, 1.0, s / np.where(sw == 0, 1.0, sw)).astype(np.float32)
    return (zw * r[:, None, None]).astype(np.float32)


def clip_forward_ex(clip, tokens, emb_row=None, bank=None, weights=None, clip_skip=1):
    """the extended CLIP forward on a CLIPOracle, in its dtype: bank rows [rows, C] where emb_row >= 0, the first n_layer - clip_skip + 1 blocks, the final
    LayerNorm, then the weighting when weights are given"""
    from oracle import clip_oracle as CO
    from oracle import sd_oracle as O
    d = clip.d
    tokens = torch.as_tensor(np.asarray(tokens), dtype=torch.long)
    n, T = tokens.shape
    x = clip._table("token_embedding", d.n_vocab)[tokens]
    if emb_row is not None:
        rows = torch.as_tensor(np.asarray(emb_row), dtype=torch.long)
        b = torch.as_tensor(np.asarray(bank), dtype=clip.dtype)
        x = torch.where((rows >= 0)[:, :, None], b[rows.clamp(min=0)], x)
    x = x + clip._table("position_embedding", d.n_ctx)[:T][None]
    mask = CO.attn_decoder_mask(T, clip.dtype)
    if not 1 <= clip_skip <= d.n_layer:
        raise ValueError("clip_skip")
    for i in range(d.n_layer - clip_skip + 1):
        x = clip.block(f"{clip.root}/blocks/{i}", x, mask)
    z = O.layer_norm(x, *clip.P.norm(f"{clip.root}/layer_norm", d.n_state))
    return z if weights is None else reweight(z, weights)


# ---- inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------------
PARSE_TABLE = [
    ("normal text", [("normal text", 1.0)]),
    ("an (important) word", [("an ", 1.0), ("important", 1.1), (" word", 1.0)]),
    ("(unbalanced", [("unbalanced", 1.1)]),
    ("\\(literal\\]", [("(literal]", 1.0)]),
    ("(unnecessary)(parens)", [("unnecessaryparens", 1.1)]),
    ("a (((house:1.3)) [on] a (hill:0.5), sun, (((sky))).",
     [("a ", 1.0), ("house", 1.5730000000000004), (" ", 1.1), ("on", 1.0), (" a ", 1.1), ("hill", 0.55), (", sun, ", 1.1), ("sky", 1.4641000000000006), (".", 1.1)]),
    ("a cat BREAK a (dog:2)", [("a cat", 1.0), ("BREAK", -1), ("a ", 1.0), ("dog", 2.0)]),
    ("time 12:30 (x: 1.5 )", [("time 12:30 ", 1.0), ("x", 1.5)]),
    ("[a]]) b", [("a", 0.9090909090909091), ("]) b", 1.0)]),
    ("(a:1.2:3)", [("a:1.2", 3.0)]),
    ("(a:-0.5) [[b]]", [("a", -0.5), (" ", 1.0), ("b", 0.8264462809917354)]),
    ("a BREAK BREAK b", [("a", 1.0), ("BREAK", -1), ("", 1.0), ("BREAK", -1), ("b", 1.0)]),
    ("", [("", 1.0)]),
]
BAD_WEIGHTS = [("(y:.)", "."), ("(y:1.2.3)", "1.2.3"), ("((y: +. ))", "+.")]
FUZZ_ALPHABET = "()[]\\: .0123456789abBREAK"


def fuzz_strings(count=2000, seed=20240917):
    """random strings over FUZZ_ALPHABET, some with whole BREAK words and weights spliced in so that those paths are taken often"""
    import random
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        parts = []
        for _ in range(rng.randint(0, 24)):
            parts.append(rng.choice(FUZZ_ALPHABET) if rng.random() > 0.12 else rng.choice(["BREAK", " BREAK ", ":1.2)", ": .5 )", "(a", "\\"]))
        out.append("".join(parts))
    return out


def serialise(items):
    """the text sdmi_prompt_parse writes, before its escapes (the sanitizer driver compares with it)"""
    return "".join("%.17g\t%s\n" % (w, t) for t, w in items)


def emphasis_inputs(vocab, T, seed=5):
    """three chunks of tokens [3, T] and weights [3, T] for the weighting tests: chunk 0 has weights above and below 1, a negative one and a zero, chunk 1 has
    all weights 1 (it must keep its bits), chunk 2 other values.  Start, end and padding positions keep weight 1, as the chunker leaves them."""
    g = np.random.default_rng(seed)
    tokens = g.integers(0, vocab - 2, (3, T)).astype(np.int32)
    tokens[:, 0] = vocab - 2
    tokens[:, T - 4:] = vocab - 1
    w = np.ones((3, T), np.float32)
    w[0, 1:6] = [1.1, 1.3, 0.6, -0.5, 0.0]
    w[2, 2:7] = [1.21, 0.9090909, 2.0, 0.25, 1.1]
    return tokens, w
