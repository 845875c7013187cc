// prompt.cpp -- web-UI prompt parsing and chunking (prompt.hpp).  Host only, no HIP.
#include "prompt.hpp"

#include <cstdlib>
#include <cstring>

#include "error.hpp"

namespace sdmi {

namespace {

// the regular expressions of the web UI are restated over bytes: \s is ASCII white space, \w is [A-Za-z0-9_], \d is [0-9].  A byte of a multi-byte
// UTF-8 character is neither, so such characters are plain text.
inline bool is_space(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }
inline bool is_word(unsigned char c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; }
inline bool is_special(unsigned char c) { return c == '\\' || c == '(' || c == ')' || c == '[' || c == ']' || c == ':'; }

struct Parser {
    std::vector<PromptFragment> res;
    std::vector<size_t> round, square;

    void multiply_range(size_t start, double m) {
        for (size_t p = start; p < res.size(); ++p) res[p].weight *= m;
    }

    // text outside every token of the grammar: split at \s*\bBREAK\b\s*
    void plain(const std::string& t) {
        const size_t n = t.size();
        size_t start = 0, q = 0;
        bool first = true;
        auto emit = [&](const std::string& part) {
            if (!first) res.push_back({"BREAK", -1.0});
            res.push_back({part, 1.0});
            first = false;
        };
        while (q + 5 <= n) {
            if (std::memcmp(t.data() + q, "BREAK", 5) != 0 || (q > 0 && is_word((unsigned char)t[q - 1])) || (q + 5 < n && is_word((unsigned char)t[q + 5]))) {
                ++q;
                continue;
            }
            size_t left = q, right = q + 5;
            while (left > start && is_space((unsigned char)t[left - 1])) --left;
            while (right < n && is_space((unsigned char)t[right])) ++right;
            emit(t.substr(start, left - start));
            start = q = right;
        }
        emit(t.substr(start));
    }
};

}  // namespace

std::vector<PromptFragment> parse_prompt(const std::string& s) {
    Parser P;
    const size_t n = s.size();
    const double round_mul = 1.1, square_mul = 1 / 1.1;
    size_t i = 0;
    while (i < n) {
        const char c = s[i];
        if (c == '\\') {
            if (i + 1 < n && (s[i + 1] == '(' || s[i + 1] == ')' || s[i + 1] == '[' || s[i + 1] == ']' || s[i + 1] == '\\')) {
                P.res.push_back({std::string(1, s[i + 1]), 1.0});
                i += 2;
            } else {
                P.res.push_back({"", 1.0});   // a lone backslash is dropped
                i += 1;
            }
        } else if (c == '(') {
            P.round.push_back(P.res.size());
            ++i;
        } else if (c == '[') {
            P.square.push_back(P.res.size());
            ++i;
        } else if (c == ':') {
            // :\s*([+-]?[.\d]+)\s*\)
            size_t j = i + 1;
            while (j < n && is_space((unsigned char)s[j])) ++j;
            const size_t w0 = j;
            if (j < n && (s[j] == '+' || s[j] == '-')) ++j;
            const size_t d0 = j;
            while (j < n && (s[j] == '.' || (s[j] >= '0' && s[j] <= '9'))) ++j;
            const size_t w1 = j;
            while (j < n && is_space((unsigned char)s[j])) ++j;
            if (w1 > d0 && j < n && s[j] == ')') {
                if (!P.round.empty()) {
                    const std::string num = s.substr(w0, w1 - w0);
                    char* end = nullptr;
                    const double w = std::strtod(num.c_str(), &end);
                    if (end == num.c_str() || *end) throw Error(SDMI_ERR_INVALID, "parse_prompt: '" + num + "' is not a number (in '" + s.substr(i, j + 1 - i) + "')");
                    P.multiply_range(P.round.back(), w);
                    P.round.pop_back();
                } else {
                    P.plain(s.substr(i, j + 1 - i));
                }
                i = j + 1;
            } else {
                P.plain(":");
                ++i;
            }
        } else if (c == ')' && !P.round.empty()) {
            P.multiply_range(P.round.back(), round_mul);
            P.round.pop_back();
            ++i;
        } else if (c == ']' && !P.square.empty()) {
            P.multiply_range(P.square.back(), square_mul);
            P.square.pop_back();
            ++i;
        } else if (c == ')' || c == ']') {
            P.plain(std::string(1, c));
            ++i;
        } else {
            size_t j = i;
            while (j < n && !is_special((unsigned char)s[j])) ++j;
            P.plain(s.substr(i, j - i));
            i = j;
        }
    }
    for (size_t pos : P.round) P.multiply_range(pos, round_mul);
    for (size_t pos : P.square) P.multiply_range(pos, square_mul);
    std::vector<PromptFragment>& res = P.res;
    if (res.empty()) res.push_back({"", 1.0});
    // merge runs of equal weight.  A marker ("BREAK", -1) sits between two parts of its own token that carry minus its weight, so it never merges.
    std::vector<PromptFragment> out;
    out.reserve(res.size());
    for (PromptFragment& f : res) {
        if (!out.empty() && out.back().weight == f.weight) out.back().text += f.text;
        else out.push_back(std::move(f));
    }
    return out;
}

PromptChunks prompt_chunks(const Tokenizer& tok, const std::string& text, int clip_ctx, bool emphasis, int min_chunks,
                           const std::vector<PromptEmbedding>& embeddings, int pad_id) {
    if (clip_ctx < 3) throw Error(SDMI_ERR_INVALID, "prompt_chunks: clip_ctx must be at least 3");
    if (min_chunks < 0) throw Error(SDMI_ERR_INVALID, "prompt_chunks: min_chunks must not be negative");
    const int L = clip_ctx - 2;
    std::vector<int> first_row(embeddings.size());
    int rows = 0;
    for (size_t e = 0; e < embeddings.size(); ++e) {
        if (embeddings[e].ids.empty()) throw Error(SDMI_ERR_INVALID, "prompt_chunks: an embedding's name has no tokens");
        if (embeddings[e].n_vectors < 1 || embeddings[e].n_vectors > L)
            throw Error(SDMI_ERR_INVALID, "prompt_chunks: an embedding must have 1 .. clip_ctx - 2 = " + std::to_string(L) + " vectors, got " + std::to_string(embeddings[e].n_vectors));
        first_row[e] = rows;
        rows += embeddings[e].n_vectors;
    }
    std::vector<PromptFragment> parsed;
    if (emphasis) parsed = parse_prompt(text);
    else parsed.push_back({text, 1.0});

    PromptChunks out;
    const int32_t sot = tok.start_token(), eot = tok.end_token();
    std::vector<int32_t> c_ids, c_rows;
    std::vector<float> c_w;
    auto next_chunk = [&] {
        out.ids.push_back(sot); out.weights.push_back(1.0f); out.emb_row.push_back(-1);
        for (int p = 0; p < L + 1; ++p) {
            const bool content = p < (int)c_ids.size();
            out.ids.push_back(content ? c_ids[p] : (pad_id < 0 || p == (int)c_ids.size()) ? eot : pad_id);
            out.weights.push_back(content ? c_w[p] : 1.0f);
            out.emb_row.push_back(content ? c_rows[p] : -1);
        }
        ++out.k;
        c_ids.clear(); c_w.clear(); c_rows.clear();
    };
    for (const PromptFragment& f : parsed) {
        if (emphasis && f.is_break()) { next_chunk(); continue; }
        const std::vector<int32_t> ids = tok.encode(f.text);
        const float w = (float)f.weight;
        size_t pos = 0;
        while (pos < ids.size()) {
            if ((int)c_ids.size() == L) next_chunk();
            int best = -1;
            for (size_t e = 0; e < embeddings.size(); ++e) {
                const std::vector<int32_t>& name = embeddings[e].ids;
                if (name.size() > ids.size() - pos || (best >= 0 && name.size() <= embeddings[best].ids.size())) continue;
                if (std::equal(name.begin(), name.end(), ids.begin() + pos)) best = (int)e;
            }
            if (best < 0) {
                c_ids.push_back(ids[pos]); c_w.push_back(w); c_rows.push_back(-1);
                ++pos;
                continue;
            }
            const int v = embeddings[best].n_vectors;
            if ((int)c_ids.size() + v > L) next_chunk();
            for (int j = 0; j < v; ++j) { c_ids.push_back(eot); c_w.push_back(w); c_rows.push_back(first_row[best] + j); }
            pos += embeddings[best].ids.size();
        }
    }
    if (!c_ids.empty() || out.k == 0) next_chunk();
    while (out.k < min_chunks) next_chunk();
    return out;
}

}  // namespace sdmi
