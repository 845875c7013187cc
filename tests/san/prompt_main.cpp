// prompt_main.cpp -- sanitizer driver of the web-UI prompt parser and chunker (csrc/prompt.cpp, host only).  Built by tests/test_prompt_cpu.py with plain g++
// (-fsanitize=address,undefined) together with prompt.cpp and tokenizer.cpp.
//
//   prompt_main <cases> <merges file>
//
// <cases> holds two lines per case, both as hexadecimal bytes: the prompt, and what parse_prompt must give -- its items as "%.17g<TAB>fragment<LF>" one after
// the other, or the three bytes "ERR" for a prompt that must be refused with SDMI_ERR_INVALID.  Every prompt also goes through prompt_chunks (emphasis on and
// off, with and without embeddings) with the invariants of a chunk checked.  Exit 0 when every case is reproduced.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../stable_diffusion_burn_amd/csrc/error.hpp"
#include "../../stable_diffusion_burn_amd/csrc/prompt.hpp"

using namespace sdmi;

static std::string unhex(const std::string& h) {
    std::string s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s += (char)std::strtol(h.substr(i, 2).c_str(), nullptr, 16);
    return s;
}

static std::string parsed(const std::string& text) {
    try {
        std::string s;
        for (const PromptFragment& f : parse_prompt(text)) {
            char w[40];
            std::snprintf(w, sizeof w, "%.17g", f.weight);
            s += std::string(w) + "\t" + f.text + "\n";
        }
        return s;
    } catch (const Error& e) {
        return e.status == SDMI_ERR_INVALID ? "ERR" : "ERR?";
    }
}

static bool chunks_ok(const Tokenizer& tok, const std::string& text, int clip_ctx, bool emphasis, const std::vector<PromptEmbedding>& embs, int rows) {
    PromptChunks c;
    try {
        c = prompt_chunks(tok, text, clip_ctx, emphasis, 2, embs);
    } catch (const Error& e) {
        return e.status == SDMI_ERR_INVALID && emphasis;   // only a bad weight may refuse a prompt
    }
    const size_t n = (size_t)c.k * clip_ctx;
    if (c.k < 2 || c.ids.size() != n || c.weights.size() != n || c.emb_row.size() != n) return false;
    for (int k = 0; k < c.k; ++k) {
        const size_t o = (size_t)k * clip_ctx;
        if (c.ids[o] != tok.start_token() || c.weights[o] != 1.0f || c.emb_row[o] != -1) return false;
        if (c.ids[o + clip_ctx - 1] != tok.end_token() || c.weights[o + clip_ctx - 1] != 1.0f || c.emb_row[o + clip_ctx - 1] != -1) return false;
        for (int p = 0; p < clip_ctx; ++p)
            if (c.emb_row[o + p] < -1 || c.emb_row[o + p] >= rows || c.ids[o + p] < 0 || c.ids[o + p] >= tok.vocab_size()) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: prompt_main <cases> <merges file>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const Tokenizer tok(argv[2]);
    const std::vector<PromptEmbedding> embs = {{tok.encode("a"), 3}, {tok.encode("ab"), 1}, {tok.encode("b 1"), 14}};
    std::string hp, he;
    int cases = 0, differ = 0;
    while (std::getline(in, hp) && std::getline(in, he)) {
        const std::string text = unhex(hp), expect = unhex(he), got = parsed(text);
        ++cases;
        bool ok = got == expect;
        ok = chunks_ok(tok, text, 16, true, {}, 0) && ok;
        ok = chunks_ok(tok, text, 16, true, embs, 18) && ok;
        ok = chunks_ok(tok, text, 16, false, embs, 18) && ok;
        ok = chunks_ok(tok, text, 3, true, {}, 0) && ok;
        if (!ok && ++differ <= 5) std::fprintf(stderr, "case %d: prompt %s\n expected %s\n got      %s\n", cases, hp.c_str(), he.c_str(), got.c_str());
    }
    std::printf("%d cases, %d differ\n", cases, differ);
    return differ ? 1 : 0;
}
