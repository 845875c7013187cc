// prompt.hpp -- web-UI prompt encoding, the host side (include/sdmi.h "web-UI prompt encoding").  Host only, no HIP.
//
// parse_prompt is the A1111 web UI's parse_prompt_attention: emphasis brackets, explicit weights, escapes and BREAK markers -> (fragment, weight) pairs.
// prompt_chunks turns the pairs into padded clip_ctx-token chunks with per-position weights and textual-inversion rows, the input of
// Engine::clip_forward_dev's extended form.  Nothing here touches a device; tests/san/prompt_main.cpp builds it with plain g++.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "tokenizer.hpp"

namespace sdmi {

struct PromptFragment {
    std::string text;
    double weight;
    bool is_break() const { return weight == -1.0 && text == "BREAK"; }   // the marker is this exact pair; BREAK inside a span is ordinary text, as in the web UI
};

// Throws sdmi::Error (SDMI_ERR_INVALID) for a weight that is no complete number ("(y:.)", "(y:1.2.3)").
std::vector<PromptFragment> parse_prompt(const std::string& text);

// A textual-inversion embedding as the chunker sees it: the token ids of its name and how many vectors (content positions) it takes.
struct PromptEmbedding {
    std::vector<int32_t> ids;
    int n_vectors;
};

struct PromptChunks {
    int k = 0;                      // chunks
    std::vector<int32_t> ids;       // [k, clip_ctx]
    std::vector<float> weights;     // [k, clip_ctx]; start, end and padding positions 1.0
    std::vector<int32_t> emb_row;   // [k, clip_ctx]; -1: the token table's row
};

// embeddings: rows are numbered over the list in order (first_row(i) = sum of n_vectors before i).  SDMI_ERR_INVALID: clip_ctx < 3, min_chunks < 0,
// an embedding with no ids, n_vectors < 1 or n_vectors > clip_ctx - 2.
// pad_id: what fills a chunk BEHIND its first <|endoftext|>; < 0 = <|endoftext|> again (CLIP as SD v1 uses it), 0 = OpenCLIP's padding (SD 2.x)
PromptChunks prompt_chunks(const Tokenizer& tok, const std::string& text, int clip_ctx, bool emphasis, int min_chunks,
                           const std::vector<PromptEmbedding>& embeddings, int pad_id = -1);

}  // namespace sdmi
