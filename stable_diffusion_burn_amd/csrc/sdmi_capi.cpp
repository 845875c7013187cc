// sdmi_capi.cpp -- extern "C" boundary of libsdmi.so (see include/sdmi.h).
// Translates C arguments to Engine calls, C++ exceptions to sdmi_status codes,
// and stages host buffers through the device pool for the host-pointer API.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "capi_util.hpp"
#include "engine.hpp"
#include "ckpt_keys.hpp"
#include "mpk_reader.hpp"
#include "prompt.hpp"
#include "safetensors_reader.hpp"
#include "lora_keys.hpp"
#include "tokenizer.hpp"

namespace sdmi {
void write_png_rgb8(const std::string& path, const uint8_t* rgb, int width, int height);  // png_writer.cpp
}

struct sdmi_tokenizer {
    sdmi::Tokenizer tok;
};

static thread_local std::string g_last_error;

namespace sdmi {
void set_last_error(const std::string& msg) { g_last_error = msg; }
}

extern "C" {

int sdmi_default_config(sdmi_config* cfg) {
    if (!cfg) return SDMI_ERR_INVALID;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->device = 0;
    cfg->model_channels = 320;  // unet/mod.rs:41
    cfg->n_head = 8;            // unet/mod.rs:44
    cfg->ctx_dim = 768;         // unet/mod.rs:44
    cfg->latent_h = 64;         // stablediffusion/mod.rs:116
    cfg->latent_w = 64;
    cfg->vae_ch = 128;          // autoencoder/mod.rs:33-34
    cfg->max_batch = 0;
    cfg->precision = 0;
    cfg->clip_layers = 12;      // CLIPConfig::new(49408, 768, 12, 77, 12), stablediffusion/mod.rs:29
    cfg->clip_heads = 12;
    cfg->clip_vocab = 49408;
    cfg->clip_ctx = 77;
    cfg->unet_in_ch = 4;        // the latent alone (9: the SD v1 inpainting checkpoints)
    return SDMI_OK;
}

const char* sdmi_version(void) { return "sdmi 0.3 gfx950 fp32+bf16+mxfp8 (MI355X-native SD v1.4: CLIP, UNet DDIM/CFG loop, VAE; multi-GPU sharding)"; }

const char* sdmi_last_error(void) { return g_last_error.c_str(); }

int sdmi_create(sdmi_ctx** out, const sdmi_config* cfg) {
    if (!out || !cfg) { g_last_error = "sdmi_create: null argument"; return SDMI_ERR_INVALID; }
    *out = nullptr;
    return guarded([&] {
        Engine* e = new Engine(*cfg);
        *out = new sdmi_ctx{e};
    });
}

void sdmi_destroy(sdmi_ctx* ctx) {
    if (!ctx) return;
    delete ctx->engine;
    delete ctx;
}

int sdmi_synchronize(sdmi_ctx* ctx) { return guarded([&] { eng(ctx).sync(); }); }

int sdmi_set_stream(sdmi_ctx* ctx, void* hip_stream, int32_t enable) {
    return guarded([&] { eng(ctx).set_user_stream(reinterpret_cast<hipStream_t>(hip_stream), enable != 0); });
}

int sdmi_set_weight(sdmi_ctx* ctx, const char* name, const float* data, int32_t ndim, const int64_t* dims) {
    return guarded([&] { eng(ctx).set_weight(name, data, ndim, dims); });
}

int sdmi_weight_count(sdmi_ctx* ctx) {
    int n = 0;
    int st = guarded([&] { n = (int)eng(ctx).entries().size(); });
    return st == SDMI_OK ? n : st;
}

int sdmi_weight_info(sdmi_ctx* ctx, int32_t index, const char** name, int32_t* ndim, int64_t dims[4]) {
    return guarded([&] {
        const auto& es = eng(ctx).entries();
        if (index < 0 || index >= (int)es.size()) throw Error(SDMI_ERR_INVALID, "weight index out of range");
        if (name) *name = es[index].name.c_str();
        if (ndim) *ndim = es[index].ndim;
        if (dims) for (int i = 0; i < 4; ++i) dims[i] = es[index].dims[i];
    });
}

int sdmi_load_weights_dir(sdmi_ctx* ctx, const char* dump_dir) {
    return guarded([&] { eng(ctx).load_weights_dir(dump_dir); });
}

int sdmi_load_weights_mpk(sdmi_ctx* ctx, const char* mpk_path) {
    return guarded([&] { eng(ctx).load_weights_mpk(mpk_path); });
}

int sdmi_mpk_list(const char* mpk_path, char* out, size_t capacity, size_t* needed) {
    return guarded([&] {
        if (!mpk_path || !needed) throw Error(SDMI_ERR_INVALID, "mpk_list: null argument");
        sdmi::MpkFile f(mpk_path);
        std::string s = "# format=" + f.format() + " float=" + f.float_type() + "\n";
        for (const auto& t : f.tensors()) {
            s += t.name + "\t";
            for (size_t i = 0; i < t.shape.size(); ++i) s += (i ? "," : "") + std::to_string(t.shape[i]);
            s += "\t" + std::to_string(t.file_offset) + "\n";
        }
        *needed = s.size() + 1;
        if (out && capacity >= s.size() + 1) std::memcpy(out, s.c_str(), s.size() + 1);
        else if (out && capacity) throw Error(SDMI_ERR_INVALID, "mpk_list: capacity too small");
    });
}

int sdmi_load_weights_safetensors(sdmi_ctx* ctx, const char* path) {
    return guarded([&] { eng(ctx).load_weights_safetensors(path); });
}

// copies `s` + terminator to a caller's buffer by the query-then-fill convention of sdmi_mpk_list
static void text_out(const std::string& s, char* out, size_t capacity, size_t* needed, const char* what) {
    *needed = s.size() + 1;
    if (out && capacity >= s.size() + 1) std::memcpy(out, s.c_str(), s.size() + 1);
    else if (out && capacity) throw Error(SDMI_ERR_INVALID, std::string(what) + ": capacity too small");
}

// a key as one field of a tab-separated line: backslash and control characters as JSON escapes
static std::string listing_escape(const std::string& key) {
    std::string s;
    for (unsigned char ch : key) {
        if (ch == '\\') s += "\\\\";
        else if (ch == '\t') s += "\\t";
        else if (ch == '\n') s += "\\n";
        else if (ch < 0x20 || ch == 0x7f) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", ch); s += b; }
        else s += (char)ch;
    }
    return s;
}

int sdmi_safetensors_list(const char* path, char* out, size_t capacity, size_t* needed) {
    return guarded([&] {
        if (!path || !needed) throw Error(SDMI_ERR_INVALID, "safetensors_list: null argument");
        sdmi::SafetensorsFile f(path);
        std::string s;
        for (const auto& t : f.tensors()) {
            s += listing_escape(t.key) + "\t" + t.dtype + "\t";
            for (size_t i = 0; i < t.shape.size(); ++i) s += (i ? "," : "") + std::to_string(t.shape[i]);
            std::string dump;
            s += "\t" + std::to_string(t.file_offset) + "\t" + (sdmi::dump_name_of_checkpoint_key(t.key, &dump) ? dump : std::string("-")) + "\n";
        }
        text_out(s, out, capacity, needed, "safetensors_list");
    });
}

int sdmi_checkpoint_key(const char* dump_name, char* out, size_t capacity, size_t* needed, int32_t* transposed) {
    return guarded([&] {
        if (!dump_name || !needed) throw Error(SDMI_ERR_INVALID, "checkpoint_key: null argument");
        std::string key;
        bool tr = false;
        if (!sdmi::checkpoint_key(dump_name, &key, &tr)) throw Error(SDMI_ERR_INVALID, std::string("checkpoint_key: '") + dump_name + "' has no checkpoint source");
        if (transposed) *transposed = tr ? 1 : 0;
        text_out(key, out, capacity, needed, "checkpoint_key");
    });
}

int sdmi_checkpoint_key_ex(const char* dump_name, int32_t variant, char* out, size_t capacity, size_t* needed, int32_t* transposed, int32_t* slice) {
    return guarded([&] {
        if (!dump_name || !needed) throw Error(SDMI_ERR_INVALID, "checkpoint_key: null argument");
        if (variant != 0 && variant != 1) throw Error(SDMI_ERR_INVALID, "checkpoint_key: variant must be 0 (SD v1) or 1 (SD 2.x)");
        std::string key;
        bool tr = false;
        int sl = -1;
        if (!sdmi::checkpoint_key(dump_name, variant, &key, &tr, &sl)) throw Error(SDMI_ERR_INVALID, std::string("checkpoint_key: '") + dump_name + "' has no checkpoint source");
        if (transposed) *transposed = tr ? 1 : 0;
        if (slice) *slice = sl;
        text_out(key, out, capacity, needed, "checkpoint_key");
    });
}

int sdmi_safetensors_model_family(const char* path, int32_t* family) {
    return guarded([&] {
        if (!path || !family) throw Error(SDMI_ERR_INVALID, "safetensors_model_family: null argument");
        sdmi::SafetensorsFile f(path);
        *family = f.find(sdmi::kFamilyKeySd2) ? 2 : f.find(sdmi::kFamilyKeySd1) ? 1 : 0;
    });
}

int sdmi_default_alphas_cumprod(float* out, int32_t n) {
    return guarded([&] {
        if (!out || n < 1) throw Error(SDMI_ERR_INVALID, "default_alphas_cumprod: null output or n < 1");
        sdmi::default_alphas_cumprod(out, n);
    });
}

int sdmi_load_weights_packed(sdmi_ctx* ctx, const float* data, size_t n_floats, int32_t groups) {
    return guarded([&] { eng(ctx).load_weights_packed(data, n_floats, groups); });
}

int64_t sdmi_packed_size(sdmi_ctx* ctx, int32_t groups) {
    int64_t n = 0;
    int st = guarded([&] { n = (int64_t)eng(ctx).packed_size(groups); });
    return st == SDMI_OK ? n : st;
}

int sdmi_finalize_weights(sdmi_ctx* ctx) { return guarded([&] { eng(ctx).finalize_weights(); }); }

// ---- hot path, device pointers -----------------------------------------------------
int sdmi_sample_latent_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu,
                           double scale, size_t n_steps, const float* init_latent, float* latent_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!context || !uncond || !init_latent || !latent_out) throw Error(SDMI_ERR_INVALID, "sample_latent_dev: null pointer");
        Engine::Call call(e, /*dev_inputs=*/true);
        e.sample_latent_dev(context, n, T, uncond, Tu, scale, n_steps, init_latent, latent_out);
        call.finish();
    });
}

int sdmi_latent_to_image_dev(sdmi_ctx* ctx, const float* latent, int32_t n, uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!latent || !rgb_out) throw Error(SDMI_ERR_INVALID, "latent_to_image_dev: null pointer");
        Engine::Call call(e, /*dev_inputs=*/true);
        e.decode_latent_dev(latent, n, (float)(1.0 / 0.18215), nullptr, rgb_out);
        call.finish();
    });
}

int sdmi_sample_image_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu,
                          double scale, size_t n_steps, const float* init_latent, uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!context || !uncond || !init_latent || !rgb_out) throw Error(SDMI_ERR_INVALID, "sample_image_dev: null pointer");
        if (n <= 0) throw Error(SDMI_ERR_INVALID, "sample_image_dev: n must be positive");
        Engine::Call call(e, /*dev_inputs=*/true);
        Engine::Buf lat(&e, (size_t)n * 4 * e.latent_h() * e.latent_w() * sizeof(float));
        e.sample_latent_dev(context, n, T, uncond, Tu, scale, n_steps, init_latent, lat.f());
        e.decode_latent_dev(lat.f(), n, (float)(1.0 / 0.18215), nullptr, rgb_out);
        call.finish();
    });
}

int sdmi_img2img_latent_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale,
                            size_t n_steps, double strength, const float* z0, const float* mask, const float* noise, uint64_t seed,
                            float* latent_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!context || !uncond || !z0 || !latent_out) throw Error(SDMI_ERR_INVALID, "img2img_latent_dev: null pointer");
        Engine::Call call(e, /*dev_inputs=*/true);
        e.img2img_latent_dev(context, n, T, uncond, Tu, scale, n_steps, strength, z0, mask, noise, seed, latent_out);
        call.finish();
    });
}

int sdmi_img2img_image_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale,
                           size_t n_steps, double strength, const uint8_t* init_rgb, const float* mask, const float* noise, uint64_t seed,
                           uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!context || !uncond || !init_rgb || !rgb_out) throw Error(SDMI_ERR_INVALID, "img2img_image_dev: null pointer");
        if (n <= 0) throw Error(SDMI_ERR_INVALID, "img2img_image_dev: n must be positive");
        Engine::Call call(e, /*dev_inputs=*/true);
        Engine::Buf lat(&e, (size_t)n * 4 * e.latent_h() * e.latent_w() * sizeof(float));
        e.img2img_image_dev(context, n, T, uncond, Tu, scale, n_steps, strength, init_rgb, mask, noise, seed, lat.f());
        e.decode_latent_dev(lat.f(), n, (float)(1.0 / 0.18215), nullptr, rgb_out);
        call.finish();
    });
}

// ---- hot path, host pointers ---------------------------------------------------------
int sdmi_unet_forward(sdmi_ctx* ctx, const float* x, int32_t t, const float* context, int32_t n, int32_t T, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || T <= 0) throw Error(SDMI_ERR_INVALID, "unet_forward: n and T must be positive");
        const size_t lat = (size_t)n * 4 * e.latent_h() * e.latent_w() * sizeof(float);
        Engine::Call call(e);
        DevIn dx(e, x, lat), dc(e, context, (size_t)n * T * e.config().ctx_dim * sizeof(float));
        DevOut dout(e, out, lat);
        e.unet_forward_dev(dx.f(), t, dc.f(), n, T, dout.f());
        call.finish();
        dout.fetch();
    });
}

// ---- tokenizer + CLIP -----------------------------------------------------------------
int sdmi_tokenizer_create(sdmi_tokenizer** out, const char* merges_path) {
    if (!out || !merges_path) { g_last_error = "sdmi_tokenizer_create: null argument"; return SDMI_ERR_INVALID; }
    *out = nullptr;
    return guarded([&] { *out = new sdmi_tokenizer{sdmi::Tokenizer(merges_path)}; });
}

void sdmi_tokenizer_destroy(sdmi_tokenizer* tok) { delete tok; }

int sdmi_tokenizer_vocab_size(const sdmi_tokenizer* tok) { return tok ? tok->tok.vocab_size() : SDMI_ERR_INVALID; }

int sdmi_tokenizer_encode(const sdmi_tokenizer* tok, const char* text, int32_t* ids, int32_t capacity, int32_t* n_ids) {
    return guarded([&] {
        if (!tok || !text || !n_ids) throw Error(SDMI_ERR_INVALID, "tokenizer_encode: null argument");
        const std::vector<int32_t> v = tok->tok.encode(text);
        *n_ids = (int32_t)v.size();
        if ((int64_t)v.size() > capacity) throw Error(SDMI_ERR_INVALID, "tokenizer_encode: capacity too small");
        if (!v.empty() && !ids) throw Error(SDMI_ERR_INVALID, "tokenizer_encode: null output");
        std::copy(v.begin(), v.end(), ids);
    });
}

int sdmi_tokenizer_decode(const sdmi_tokenizer* tok, const int32_t* ids, int32_t n, char* out, int32_t capacity, int32_t* n_bytes) {
    return guarded([&] {
        if (!tok || !n_bytes || n < 0 || (n > 0 && !ids)) throw Error(SDMI_ERR_INVALID, "tokenizer_decode: bad argument");
        const std::string s = tok->tok.decode(ids, (size_t)n);
        *n_bytes = (int32_t)s.size();
        if ((int64_t)s.size() > capacity) throw Error(SDMI_ERR_INVALID, "tokenizer_decode: capacity too small");
        if (!s.empty() && !out) throw Error(SDMI_ERR_INVALID, "tokenizer_decode: null output");
        std::memcpy(out, s.data(), s.size());
    });
}

static void clip_forward_host(Engine& e, const int32_t* tokens, int n, int T, float* out) {
    if (!tokens || !out) throw Error(SDMI_ERR_INVALID, "clip_forward: null argument");
    if (n <= 0 || T <= 0) throw Error(SDMI_ERR_INVALID, "clip_forward: n and seq_len must be positive");
    const int vocab = e.config().clip_vocab;
    for (long long i = 0; i < (long long)n * T; ++i)   // the reference's embedding gather panics on an id outside the table
        if (tokens[i] < 0 || tokens[i] >= vocab) throw Error(SDMI_ERR_INVALID, "clip_forward: token id outside the vocabulary");
    Engine::Call call(e);
    DevIn dt(e, tokens, (size_t)n * T * sizeof(int32_t));
    DevOut dout(e, out, (size_t)n * T * e.config().ctx_dim * sizeof(float));
    e.clip_forward_dev(reinterpret_cast<const int32_t*>(dt.buf.p), n, T, dout.f());
    call.finish();
    dout.fetch();
}

int sdmi_clip_forward(sdmi_ctx* ctx, const int32_t* tokens, int32_t n, int32_t seq_len, float* out) {
    return guarded([&] { clip_forward_host(eng(ctx), tokens, n, seq_len, out); });
}

int sdmi_context(sdmi_ctx* ctx, const sdmi_tokenizer* tok, const char* text, float* out, int32_t capacity_tokens, int32_t* T) {
    return guarded([&] {
        if (!tok || !text || !T) throw Error(SDMI_ERR_INVALID, "context: null argument");
        Engine& e = eng(ctx);
        const std::vector<int32_t> ids = tok->tok.encode(std::string("<|startoftext|>") + text + "<|endoftext|>");  // mod.rs:200
        *T = (int32_t)ids.size();
        if ((int64_t)ids.size() > capacity_tokens) throw Error(SDMI_ERR_INVALID, "context: capacity_tokens too small");
        clip_forward_host(e, ids.data(), 1, (int)ids.size(), out);
    });
}

// ---- web-UI prompt encoding ---------------------------------------------------------------------------------------
int sdmi_prompt_parse(const char* text, char* out, size_t capacity, size_t* needed) {
    return guarded([&] {
        if (!text || !needed) throw Error(SDMI_ERR_INVALID, "prompt_parse: null argument");
        std::string s;
        for (const sdmi::PromptFragment& f : sdmi::parse_prompt(text)) {
            char w[40];
            std::snprintf(w, sizeof w, "%.17g", f.weight);
            s += std::string(w) + "\t" + listing_escape(f.text) + "\n";
        }
        text_out(s, out, capacity, needed, "prompt_parse");
    });
}

static void chunks_out(const sdmi::PromptChunks& c, int clip_ctx, int32_t* ids, float* weights, int32_t* emb_row, int32_t capacity_chunks, int32_t* n_chunks) {
    *n_chunks = c.k;
    if (c.k > capacity_chunks) throw Error(SDMI_ERR_INVALID, "prompt_chunks: capacity_chunks too small");
    if (!ids || !weights || !emb_row) throw Error(SDMI_ERR_INVALID, "prompt_chunks: null output");
    const size_t n = (size_t)c.k * clip_ctx;
    std::copy(c.ids.begin(), c.ids.begin() + n, ids);
    std::copy(c.weights.begin(), c.weights.begin() + n, weights);
    std::copy(c.emb_row.begin(), c.emb_row.begin() + n, emb_row);
}

int sdmi_prompt_chunks(const sdmi_tokenizer* tok, const char* text, int32_t clip_ctx, int32_t emphasis, int32_t min_chunks, const char* const* emb_names,
                       const int32_t* emb_vectors, int32_t n_emb, int32_t* ids, float* weights, int32_t* emb_row, int32_t capacity_chunks, int32_t* n_chunks) {
    return guarded([&] {
        if (!tok || !text || !n_chunks) throw Error(SDMI_ERR_INVALID, "prompt_chunks: null argument");
        if (n_emb < 0 || (n_emb > 0 && (!emb_names || !emb_vectors))) throw Error(SDMI_ERR_INVALID, "prompt_chunks: n_emb embeddings need their names and vector counts");
        std::vector<sdmi::PromptEmbedding> embs;
        for (int i = 0; i < n_emb; ++i) {
            if (!emb_names[i] || !*emb_names[i]) throw Error(SDMI_ERR_INVALID, "prompt_chunks: an embedding's name is empty");
            embs.push_back({tok->tok.encode(emb_names[i]), emb_vectors[i]});
        }
        const sdmi::PromptChunks c = sdmi::prompt_chunks(tok->tok, text, clip_ctx, emphasis != 0, min_chunks, embs);
        chunks_out(c, clip_ctx, ids, weights, emb_row, capacity_chunks, n_chunks);
    });
}

// tokens / emb_row / weights: host arrays [n, T].  The host decides what the device runs: rows only when some emb_row >= 0, the weighting launch only when
// some weight differs from 1 -- a call without either and with clip_skip = 1 is sdmi_clip_forward, launch for launch.
static void clip_forward_ex_host(Engine& e, const int32_t* tokens, const int32_t* emb_row, const float* weights, int n, int T, int clip_skip, float* out) {
    if (!tokens || !out) throw Error(SDMI_ERR_INVALID, "clip_forward: null argument");
    if (n <= 0 || T <= 0) throw Error(SDMI_ERR_INVALID, "clip_forward: n and seq_len must be positive");
    const long long M = (long long)n * T;
    const int vocab = e.config().clip_vocab, rows = e.embedding_rows();
    bool any_row = false, any_weight = false;
    for (long long i = 0; i < M; ++i) {
        if (tokens[i] < 0 || tokens[i] >= vocab) throw Error(SDMI_ERR_INVALID, "clip_forward: token id outside the vocabulary");
        if (emb_row) {
            if (emb_row[i] < -1 || emb_row[i] >= rows)
                throw Error(SDMI_ERR_INVALID, "clip_forward: embedding row " + std::to_string(emb_row[i]) + " outside the context's " + std::to_string(rows) + " rows");
            any_row |= emb_row[i] >= 0;
        }
        if (weights) any_weight |= !(weights[i] == 1.0f);
    }
    Engine::Call call(e);
    DevIn dt(e, tokens, (size_t)M * sizeof(int32_t));
    std::unique_ptr<DevIn> dr, dw;
    if (any_row) dr.reset(new DevIn(e, emb_row, (size_t)M * sizeof(int32_t)));
    if (any_weight) dw.reset(new DevIn(e, weights, (size_t)M * sizeof(float)));
    DevOut dout(e, out, (size_t)M * e.config().ctx_dim * sizeof(float));
    e.clip_forward_dev(reinterpret_cast<const int32_t*>(dt.buf.p), dr ? reinterpret_cast<const int32_t*>(dr->buf.p) : nullptr, dw ? dw->f() : nullptr, n, T,
                       clip_skip, dout.f());
    call.finish();
    dout.fetch();
}

int sdmi_clip_forward_ex(sdmi_ctx* ctx, const int32_t* tokens, const int32_t* emb_row, const float* weights, int32_t n, int32_t seq_len, int32_t clip_skip,
                         float* out) {
    return guarded([&] { clip_forward_ex_host(eng(ctx), tokens, emb_row, weights, n, seq_len, clip_skip, out); });
}

int sdmi_embedding_add(sdmi_ctx* ctx, const sdmi_tokenizer* tok, const char* name, const float* vectors, int32_t n_vectors) {
    return guarded([&] {
        if (!tok || !name) throw Error(SDMI_ERR_INVALID, "embedding_add: null argument");
        eng(ctx).embedding_add(name, tok->tok.encode(name), vectors, n_vectors);
    });
}

int sdmi_embedding_load_safetensors(sdmi_ctx* ctx, const sdmi_tokenizer* tok, const char* name, const char* path) {
    return guarded([&] {
        if (!tok || !name) throw Error(SDMI_ERR_INVALID, "embedding_load_safetensors: null argument");
        Engine& e = eng(ctx);
        Engine::Call call(e);
        e.embedding_load_safetensors(name, tok->tok.encode(name), path);
        call.finish();
    });
}

int sdmi_embedding_remove(sdmi_ctx* ctx, const char* name) {
    return guarded([&] {
        if (!name) throw Error(SDMI_ERR_INVALID, "embedding_remove: null argument");
        eng(ctx).embedding_remove(name);
    });
}

int sdmi_embedding_list(sdmi_ctx* ctx, char* out, size_t capacity, size_t* needed) {
    return guarded([&] {
        if (!needed) throw Error(SDMI_ERR_INVALID, "embedding_list: null argument");
        std::string s;
        for (const Engine::Embedding& em : eng(ctx).embeddings()) s += listing_escape(em.name) + "\t" + std::to_string(em.n_vectors) + "\n";
        text_out(s, out, capacity, needed, "embedding_list");
    });
}

int sdmi_encode_prompt(sdmi_ctx* ctx, const sdmi_tokenizer* tok, const char* text, const sdmi_prompt_opts* opts, float* out, int32_t capacity_tokens, int32_t* T) {
    return guarded([&] {
        if (!tok || !text || !T) throw Error(SDMI_ERR_INVALID, "encode_prompt: null argument");
        *T = 0;
        Engine& e = eng(ctx);
        sdmi_prompt_opts o{1, 1, 1, {0, 0, 0, 0, 0}};
        if (opts) o = *opts;
        for (int32_t r : o.reserved)
            if (r) throw Error(SDMI_ERR_INVALID, "encode_prompt: sdmi_prompt_opts.reserved must be zero");
        if (e.config().clip_layers <= 0 || !e.clip_ready()) throw Error(SDMI_ERR_STATE, "encode_prompt: CLIP weights are not loaded (clip/... tensors; clip_layers > 0 in the config)");
        std::vector<sdmi::PromptEmbedding> embs;
        for (const Engine::Embedding& em : e.embeddings()) embs.push_back({em.ids, em.n_vectors});
        const int cc = e.config().clip_ctx;
        const sdmi::PromptChunks c = sdmi::prompt_chunks(tok->tok, text, cc, o.emphasis != 0, o.min_chunks, embs, e.config().variant == 1 ? 0 : -1);
        if ((int64_t)c.k * cc > INT32_MAX) throw Error(SDMI_ERR_INVALID, "encode_prompt: too many chunks");
        *T = c.k * cc;
        if (*T > capacity_tokens) throw Error(SDMI_ERR_INVALID, "encode_prompt: capacity_tokens too small");
        clip_forward_ex_host(e, c.ids.data(), c.emb_row.data(), c.weights.data(), c.k, cc, o.clip_skip, out);
    });
}

int sdmi_encode_image(sdmi_ctx* ctx, const float* img, int32_t n, float* latent_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0) throw Error(SDMI_ERR_INVALID, "encode_image: n must be positive");
        const size_t lat = (size_t)n * 4 * e.latent_h() * e.latent_w() * sizeof(float);
        Engine::Call call(e);
        DevIn di(e, img, lat * 48);   // 3 * 64 / 4
        DevOut dout(e, latent_out, lat);
        e.encode_image_dev(di.f(), n, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_write_png(const char* path, const uint8_t* rgb, int32_t width, int32_t height) {
    return guarded([&] {
        if (!path) throw Error(SDMI_ERR_INVALID, "write_png: null path");
        sdmi::write_png_rgb8(path, rgb, width, height);
    });
}

static void make_init_latent(Engine& e, const float* init_latent, uint64_t seed, int n, int h, int w, Engine::Buf& dst) {
    const size_t per = (size_t)4 * h * w;
    if (init_latent) {
        SDMI_HIP(hipMemcpyAsync(dst.p, init_latent, n * per * sizeof(float), hipMemcpyHostToDevice, e.stream()));
    } else {
        for (int i = 0; i < n; ++i) SDMI_HIP(sdmi::launch_fill_normal(dst.f() + i * per, (long long)per, seed + (uint64_t)i, e.stream()));
    }
}

int sdmi_sample_latent(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu,
                       double scale, size_t n_steps, const float* init_latent, uint64_t seed, float* latent_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || T <= 0 || Tu <= 0) throw Error(SDMI_ERR_INVALID, "sample_latent: n, T, Tu must be positive");
        const int cd = e.config().ctx_dim;
        const size_t lat = (size_t)n * 4 * e.latent_h() * e.latent_w() * sizeof(float);
        Engine::Call call(e);
        DevIn dc(e, context, (size_t)n * T * cd * sizeof(float)), du(e, uncond, (size_t)Tu * cd * sizeof(float));
        Engine::Buf x0(&e, lat);
        make_init_latent(e, init_latent, seed, n, e.latent_h(), e.latent_w(), x0);
        DevOut dout(e, latent_out, lat);
        e.sample_latent_dev(dc.f(), n, T, du.f(), Tu, scale, n_steps, x0.f(), dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_img2img_timesteps(int32_t total, size_t n_steps, double strength, int32_t* timesteps, int32_t capacity, int32_t* count) {
    return guarded([&] {
        if (!count) throw Error(SDMI_ERR_INVALID, "img2img_timesteps: null count");
        if (total <= 0 || n_steps == 0 || n_steps > (size_t)total) throw Error(SDMI_ERR_INVALID, "img2img_timesteps: n_steps out of range");
        if (!(strength > 0.0 && strength <= 1.0)) throw Error(SDMI_ERR_INVALID, "img2img_timesteps: strength must satisfy 0 < strength <= 1");
        const size_t step = (size_t)total / n_steps;                         // sample_latent's schedule (stablediffusion/mod.rs:111,123)
        std::vector<int32_t> ts;
        for (long long t = (long long)total - 1; t >= 0; t -= (long long)step) ts.push_back((int32_t)t);
        const size_t L = ts.size(), k = std::min(L, (size_t)(strength * (double)L));
        if (k < 1) throw Error(SDMI_ERR_INVALID, "img2img_timesteps: strength * steps leaves no step");
        *count = (int32_t)k;
        if (capacity < (int32_t)k || !timesteps) throw Error(SDMI_ERR_INVALID, "img2img_timesteps: capacity too small");
        std::memcpy(timesteps, ts.data() + (L - k), k * sizeof(int32_t));
    });
}

// ---- sampler choice ----------------------------------------------------------------------------------
int sdmi_set_sampler(sdmi_ctx* ctx, const sdmi_sampler* sampler) {
    return guarded([&] { eng(ctx).set_sampler(sampler); });
}

// ---- ControlNet ------------------------------------------------------------------------------------------------
int sdmi_load_control_safetensors(sdmi_ctx* ctx, const char* path) {
    return guarded([&] { eng(ctx).load_control_safetensors(path); });
}

int sdmi_control_ready(sdmi_ctx* ctx) {
    int ready = 0;
    int st = guarded([&] { ready = eng(ctx).control_ready() ? 1 : 0; });
    return st == SDMI_OK ? ready : st;
}

int sdmi_set_control(sdmi_ctx* ctx, const sdmi_control* control) {
    return guarded([&] { eng(ctx).set_control(control); });
}

int sdmi_control_step_on(double start, double end, int32_t step, int32_t n_steps) {
    if (!(start >= 0.0 && start <= end && end <= 1.0) || step < 0 || n_steps < 1 || step >= n_steps) return SDMI_ERR_INVALID;
    return Engine::control_step_on(start, end, step, n_steps) ? 1 : 0;
}

// ---- FreeU -----------------------------------------------------------------------------------------------------------
int sdmi_set_freeu(sdmi_ctx* ctx, int32_t version, float b1, float b2, float s1, float s2, double start, double end) {
    return guarded([&] {
        Engine::FreeU f;
        f.version = version; f.b1 = b1; f.b2 = b2; f.s1 = s1; f.s2 = s2; f.start = start; f.end = end;
        Engine::check_freeu(f);   // the argument errors first: they need no context
        eng(ctx).set_freeu(f);
    });
}

int sdmi_get_freeu(sdmi_ctx* ctx, int32_t* version, float* b1, float* b2, float* s1, float* s2, double* start, double* end) {
    return guarded([&] {
        const Engine::FreeU& f = eng(ctx).freeu();
        if (version) *version = f.version;
        if (b1) *b1 = f.b1;
        if (b2) *b2 = f.b2;
        if (s1) *s1 = f.s1;
        if (s2) *s2 = f.s2;
        if (start) *start = f.start;
        if (end) *end = f.end;
    });
}

int sdmi_freeu_plan(const sdmi_config* cfg, int32_t latent_h, int32_t latent_w, int32_t* out) {
    return guarded([&] {
        if (!cfg || !out) throw Error(SDMI_ERR_INVALID, "freeu_plan: null pointer");
        int plan[60];
        Engine::freeu_plan(cfg->model_channels, latent_h, latent_w, plan);
        std::copy(plan, plan + 60, out);
    });
}

// ---- IP-Adapter ------------------------------------------------------------------------------------------------------
int sdmi_ip_adapter_load_safetensors(sdmi_ctx* ctx, const char* path) {
    return guarded([&] {
        Engine& e = eng(ctx);
        Engine::Call call(e);
        e.ip_load_safetensors(path);
        call.finish();
    });
}

int sdmi_ip_adapter_check_safetensors(const sdmi_config* cfg, const char* path, int32_t* D, int32_t* T) {
    return guarded([&] {
        if (!cfg || !path) throw Error(SDMI_ERR_INVALID, "ip_adapter_check_safetensors: null argument");
        int d = 0, t = 0;
        Engine::ip_check_safetensors(path, cfg->model_channels, cfg->ctx_dim, &d, &t);
        if (D) *D = d;
        if (T) *T = t;
    });
}

int sdmi_ip_adapter_set_weights(sdmi_ctx* ctx, const float* proj_w, const float* proj_b, const float* norm_g, const float* norm_b, int32_t D, int32_t T,
                                const float* const* wk, const float* const* wv) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!wk || !wv) throw Error(SDMI_ERR_INVALID, "ip_adapter: null pointer");
        Engine::IpTensor k[Engine::kIpLayers], v[Engine::kIpLayers];
        for (int i = 0; i < Engine::kIpLayers; ++i) { k[i] = {wk[i], 0}; v[i] = {wv[i], 0}; }
        Engine::Call call(e);
        e.ip_set_weights({proj_w, 0}, {proj_b, 0}, {norm_g, 0}, {norm_b, 0}, D, T, k, v);
        call.finish();
    });
}

int sdmi_ip_adapter_ready(sdmi_ctx* ctx) {
    int ready = 0;
    const int st = guarded([&] { ready = eng(ctx).ip_ready() ? 1 : 0; });
    return st == SDMI_OK ? ready : st;
}

int sdmi_ip_adapter_dims(sdmi_ctx* ctx, int32_t* D, int32_t* T) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!e.ip_ready()) throw Error(SDMI_ERR_STATE, "ip_adapter_dims: no adapter is loaded");
        if (D) *D = e.ip_embed_dim();
        if (T) *T = e.ip_tokens_per_image();
    });
}

int sdmi_ip_adapter_clear(sdmi_ctx* ctx) {
    return guarded([&] {
        Engine& e = eng(ctx);
        Engine::Call call(e);
        e.ip_clear();
        call.finish();
    });
}

int sdmi_ip_image_tokens(sdmi_ctx* ctx, const float* embeds, int32_t n, int32_t D, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!embeds || !out) throw Error(SDMI_ERR_INVALID, "ip_image_tokens: null pointer");
        if (!e.ip_ready()) throw Error(SDMI_ERR_STATE, "ip_image_tokens: no adapter is loaded");
        if (n < 1 || D != e.ip_embed_dim()) throw Error(SDMI_ERR_INVALID, "ip_image_tokens: embeds must be [n >= 1, D = " + std::to_string(e.ip_embed_dim()) + "]");
        Engine::Call call(e);
        DevIn de(e, embeds, (size_t)n * D * sizeof(float));
        DevOut dout(e, out, (size_t)n * e.ip_tokens_per_image() * e.config().ctx_dim * sizeof(float));
        e.ip_image_tokens_dev(de.f(), n, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_set_ip_adapter(sdmi_ctx* ctx, const sdmi_ip_adapter* adapter) {
    return guarded([&] {
        if (adapter) Engine::check_ip_adapter(*adapter);   // the argument errors first: they need no context
        Engine& e = eng(ctx);
        Engine::Call call(e);
        e.set_ip_adapter(adapter);
        call.finish();
    });
}

int sdmi_set_ip_adapter_file(sdmi_ctx* ctx, const char* embeds_path, float scale, double start, double end) {
    return guarded([&] {
        Engine& e = eng(ctx);
        Engine::Call call(e);
        e.set_ip_adapter_file(embeds_path, scale, start, end);
        call.finish();
    });
}

int sdmi_get_ip_adapter(sdmi_ctx* ctx, sdmi_ip_adapter* out) {
    int set = 0;
    const int st = guarded([&] { set = eng(ctx).get_ip_adapter(out) ? 1 : 0; });
    return st == SDMI_OK ? set : st;
}

int sdmi_ip_adapter_key(const sdmi_config* cfg, int32_t ctx_index, int32_t which, char* out, size_t capacity, size_t* needed, int32_t* j, int32_t* c) {
    return guarded([&] {
        if (!cfg || !needed) throw Error(SDMI_ERR_INVALID, "ip_adapter_key: null argument");
        if (cfg->model_channels < 1) throw Error(SDMI_ERR_INVALID, "ip_adapter_key: model_channels must be positive");
        const std::string key = Engine::ip_adapter_key(cfg->model_channels, ctx_index, which);
        int jj = 0, cc = 0;
        Engine::ip_adapter_layer(cfg->model_channels, ctx_index, &jj, &cc);
        if (j) *j = jj;
        if (c) *c = cc;
        text_out(key, out, capacity, needed, "ip_adapter_key");
    });
}

int64_t sdmi_ip_kv_size(sdmi_ctx* ctx, int32_t n, int32_t cfg_pair) {
    int64_t r = 0;
    const int st = guarded([&] {
        if (n < 1) throw Error(SDMI_ERR_INVALID, "ip_kv: n must be at least 1");
        r = (int64_t)eng(ctx).ip_kv_elems(cfg_pair ? 2 * n : n);
    });
    return st == SDMI_OK ? r : st;
}

int sdmi_ip_kv(sdmi_ctx* ctx, int32_t n, int32_t cfg_pair, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!out || n < 1) throw Error(SDMI_ERR_INVALID, "ip_kv: bad argument");
        Engine::Call call(e);
        DevOut dout(e, out, e.ip_kv_elems(cfg_pair ? 2 * n : n) * sizeof(float));
        e.ip_kv_dev(n, cfg_pair != 0, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_control_hint_embed(sdmi_ctx* ctx, const uint8_t* hint_rgb, int32_t n, int32_t hint_h, int32_t hint_w, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!hint_rgb || !out) throw Error(SDMI_ERR_INVALID, "control_hint_embed: null pointer");
        if (n < 1 || hint_h < 64 || hint_w < 64 || hint_h % 64 || hint_w % 64) throw Error(SDMI_ERR_INVALID, "control_hint_embed: n >= 1, hint_h / hint_w positive multiples of 64");
        if (!e.has_control()) throw Error(SDMI_ERR_STATE, "control_hint_embed: this context has no ControlNet (sdmi_config.control_hint_ch = 0)");
        Engine::Call call(e);
        DevIn dh(e, hint_rgb, (size_t)n * hint_h * hint_w * 3);
        DevOut dout(e, out, (size_t)n * e.config().model_channels * (hint_h / 8) * (hint_w / 8) * sizeof(float));
        e.control_hint_embed_dev(reinterpret_cast<const uint8_t*>(dh.buf.p), n, hint_h, hint_w, dout.f());
        call.finish();
        dout.fetch();
    });
}

int64_t sdmi_control_residuals_size(sdmi_ctx* ctx, int32_t n) {
    int64_t r = 0;
    int st = guarded([&] {
        Engine& e = eng(ctx);
        if (n < 1) throw Error(SDMI_ERR_INVALID, "control_residuals_size: n must be positive");
        if (!e.has_control()) throw Error(SDMI_ERR_STATE, "control_residuals_size: this context has no ControlNet (sdmi_config.control_hint_ch = 0)");
        r = (int64_t)e.control_residual_elems(n);
    });
    return st == SDMI_OK ? r : st;
}

int sdmi_control_residuals(sdmi_ctx* ctx, const float* x, int32_t t, const float* context, int32_t n, int32_t T, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || T <= 0) throw Error(SDMI_ERR_INVALID, "control_residuals: n and T must be positive");
        if (!e.has_control()) throw Error(SDMI_ERR_STATE, "control_residuals: this context has no ControlNet (sdmi_config.control_hint_ch = 0)");
        const size_t lat = (size_t)n * 4 * e.latent_h() * e.latent_w() * sizeof(float);
        Engine::Call call(e);
        DevIn dx(e, x, lat), dc(e, context, (size_t)n * T * e.config().ctx_dim * sizeof(float));
        DevOut dout(e, out, e.control_residual_elems(n) * sizeof(float));
        e.control_residuals_dev(dx.f(), t, dc.f(), n, T, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_get_sampler(sdmi_ctx* ctx, sdmi_sampler* out) {
    return guarded([&] {
        if (!out) throw Error(SDMI_ERR_INVALID, "get_sampler: null output");
        *out = eng(ctx).sampler();
    });
}

// ---- sigma-schedule samplers (ksampler.cpp) ----------------------------------------------------------------------------
int sdmi_set_ksampler(sdmi_ctx* ctx, const sdmi_ksampler* ksampler) {
    return guarded([&] { eng(ctx).set_ksampler(ksampler); });
}

int sdmi_get_ksampler(sdmi_ctx* ctx, sdmi_ksampler* out, int32_t* is_set) {
    return guarded([&] {
        if (!out || !is_set) throw Error(SDMI_ERR_INVALID, "get_ksampler: null output");
        Engine& e = eng(ctx);
        *is_set = e.ksampler_set() ? 1 : 0;
        *out = e.ksampler_set() ? e.ksampler() : sdmi_ksampler{};
    });
}

int sdmi_ksampler_sigmas(const sdmi_ksampler* ksampler, const float* alphas_cumprod, int32_t total, size_t n_steps, double* sigmas, int32_t capacity, int32_t* count) {
    return guarded([&] {
        if (!ksampler || !count) throw Error(SDMI_ERR_INVALID, "ksampler_sigmas: null pointer");
        const std::vector<double> sg = sdmi::ksampler_sigmas(*ksampler, alphas_cumprod, total, n_steps);
        *count = (int32_t)sg.size();
        if (!sigmas || capacity < (int32_t)sg.size()) throw Error(SDMI_ERR_INVALID, "ksampler_sigmas: capacity too small");
        std::memcpy(sigmas, sg.data(), sg.size() * sizeof(double));
    });
}

int sdmi_sigma_to_t(const float* alphas_cumprod, int32_t total, double sigma, double* t) {
    return guarded([&] {
        if (!t) throw Error(SDMI_ERR_INVALID, "sigma_to_t: null output");
        *t = sdmi::sigma_to_t(alphas_cumprod, total, sigma);
    });
}

int sdmi_ksampler_plan(const sdmi_ksampler* ksampler, const float* alphas_cumprod, int32_t total, size_t n_steps, double strength, double* rows, int32_t capacity,
                       int32_t* count) {
    return sdmi_ksampler_plan_ex(ksampler, alphas_cumprod, total, n_steps, strength, 0, rows, capacity, count);
}

int sdmi_ksampler_plan_ex(const sdmi_ksampler* ksampler, const float* alphas_cumprod, int32_t total, size_t n_steps, double strength, int32_t prediction, double* rows,
                          int32_t capacity, int32_t* count) {
    return guarded([&] {
        if (!ksampler || !count) throw Error(SDMI_ERR_INVALID, "ksampler_plan: null pointer");
        const std::vector<double> plan = sdmi::ksampler_plan(*ksampler, alphas_cumprod, total, n_steps, strength, nullptr, prediction);
        const size_t n = plan.size() / sdmi::KPLAN_COLS;
        *count = (int32_t)n;
        if (!rows || capacity < (int32_t)n) throw Error(SDMI_ERR_INVALID, "ksampler_plan: capacity too small");
        std::memcpy(rows, plan.data(), plan.size() * sizeof(double));
    });
}

// ---- latent size, resampling rule, hires fix ---------------------------------------------------------------
int sdmi_set_latent_size(sdmi_ctx* ctx, int32_t h, int32_t w) {
    return guarded([&] { eng(ctx).set_latent_size(h, w); });
}

int sdmi_get_latent_size(sdmi_ctx* ctx, int32_t* h, int32_t* w) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!h || !w) throw Error(SDMI_ERR_INVALID, "get_latent_size: null output");
        *h = e.latent_h();
        *w = e.latent_w();
    });
}

extern "C++" {
namespace {
// torch's cubic convolution pieces (ATen/native/UpSample.h): |x| <= 1 and 1 < |x| < 2
double cubic_near(double x, double A) { return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0; }
double cubic_far(double x, double A) { return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A; }
using TapRow = sdmi::ResizeRow;
// adds weight `wt` at input index `idx` clamped to [0, in): a clamped tap lands on the border index
void fold_tap(TapRow& r, int idx, int in, double wt) {
    idx = std::min(std::max(idx, 0), in - 1);
    if (r.w.empty()) r.first = idx;
    const int j = idx - r.first;       // indices arrive in ascending order
    if (j >= (int)r.w.size()) r.w.resize((size_t)j + 1, 0.0);
    r.w[(size_t)j] += wt;
}
// One output row of torch.nn.functional.interpolate's CPU kernels in float64 (align_corners = False); every rounding step that decides an index is theirs:
// the source index passes through float before floorf (UpSampleKernel.cpp, guard_index_and_lambda), the weights stay in double.
TapRow resize_row(int in, int out, int mode, bool aa, int o) {
    TapRow r;
    if (in == out) { r.first = o; r.w.assign(1, 1.0); return r; }
    const double scale = (double)in / (double)out;
    if (mode == 0) {
        // nearest-exact.  torch has TWO rules that differ where scale (o + 0.5) is an integer in exact arithmetic, and picks by the OUTPUT size of the whole call
        // (UpSampleKernel.cpp, _use_vectorized_kernel_cond_2d: out_h + out_w <= 128).  A table of one axis cannot see the other one: it follows the call on a
        // one-axis tensor [1,1,1,in] -> (1, out), i.e. the switch at out + 1 <= 128.
        int idx;
        if (out + 1 <= 128) {      // nearest_exact_idx: scale = in / out held in float, floorf((o + 0.5) * scale)
            const float fscale = (float)in / (float)out;
            idx = (int)std::floor((float)(((double)o + 0.5) * (double)fscale));
        } else {                   // the generic kernel: scale in double, floorf(scale (o + 0.5) - 0.5 + 0.5)
            idx = (int)std::floor((float)(scale * ((double)o + 0.5) - 0.5 + 0.5));
        }
        r.first = std::min(std::max(idx, 0), in - 1);
        r.w.assign(1, 1.0);
        return r;
    }
    if (!aa) {
        double real = scale * ((double)o + 0.5) - 0.5;
        if (mode == 1 && real < 0.0) real = 0.0;         // the linear kernel clamps the source index at 0; the cubic one does not
        const int i0 = std::min((int)std::floor((float)real), in - 1);
        const double t = std::min(std::max(real - (double)i0, 0.0), 1.0);
        if (mode == 1) {
            fold_tap(r, i0, in, 1.0 - t);
            fold_tap(r, i0 + 1, in, t);
        } else {
            const double A = -0.75;
            fold_tap(r, i0 - 1, in, cubic_far(t + 1.0, A));
            fold_tap(r, i0, in, cubic_near(t, A));
            fold_tap(r, i0 + 1, in, cubic_near(1.0 - t, A));
            fold_tap(r, i0 + 2, in, cubic_far(2.0 - t, A));
        }
        return r;
    }
    // antialiased (_compute_indices_min_size_weights_aa): the filter is stretched by the scale when shrinking and the row is normalised
    const double half = mode == 1 ? 1.0 : 2.0;
    const double support = scale >= 1.0 ? half * scale : half;
    const int max_size = (int)std::ceil(support) * 2 + 1;
    const double center = scale * ((double)o + 0.5), inv = scale >= 1.0 ? 1.0 / scale : 1.0;
    const long long xmin = std::max((long long)(center - support + 0.5), 0LL);
    long long xsize = std::min((long long)(center + support + 0.5), (long long)in) - xmin;
    xsize = std::min(std::max(xsize, 0LL), (long long)max_size);
    if (xsize < 1) throw Error(SDMI_ERR_STATE, "resize_weights: empty filter window");
    r.first = (int)xmin;
    r.w.resize((size_t)xsize);
    double total = 0.0;
    for (long long j = 0; j < xsize; ++j) {
        const double x = std::fabs(((double)(j + xmin) - center + 0.5) * inv);
        double wt;
        if (mode == 1) wt = x < 1.0 ? 1.0 - x : 0.0;
        else wt = x < 1.0 ? cubic_near(x, -0.5) : x < 2.0 ? cubic_far(x, -0.5) : 0.0;
        r.w[(size_t)j] = wt;
        total += wt;
    }
    if (total != 0.0) for (double& wt : r.w) wt /= total;
    return r;
}
}  // namespace

// the rows of one axis, each computed once: shared by sdmi_resize_weights and the engine (Engine::resize_nhwc4)
std::vector<sdmi::ResizeRow> sdmi::resize_rows(int in_size, int out_size, int mode, bool antialias) {
    if (in_size < 1 || out_size < 1) throw Error(SDMI_ERR_INVALID, "resize_weights: sizes must be positive");
    if (mode < 0 || mode > 2) throw Error(SDMI_ERR_INVALID, "resize_weights: mode must be 0 (nearest-exact), 1 (bilinear) or 2 (bicubic)");
    if (mode == 0 && antialias) throw Error(SDMI_ERR_INVALID, "resize_weights: antialias belongs to modes 1 and 2");
    std::vector<ResizeRow> rows((size_t)out_size);
    for (int o = 0; o < out_size; ++o) rows[(size_t)o] = resize_row(in_size, out_size, mode, antialias, o);
    return rows;
}
}  // extern "C++"

int sdmi_resize_weights(int32_t in_size, int32_t out_size, int32_t mode, int32_t antialias, int32_t* first, int32_t* count, double* taps,
                        int32_t capacity, int32_t* max_taps, int32_t* needed) {
    return guarded([&] {
        const bool query = !first && !count && !taps;
        if (!query && (!first || !count || !taps)) throw Error(SDMI_ERR_INVALID, "resize_weights: first, count and taps are given together or not at all");
        const std::vector<TapRow> rows = sdmi::resize_rows(in_size, out_size, mode, antialias != 0);
        size_t T = 0;
        for (const TapRow& r : rows) T = std::max(T, r.w.size());
        const long long need = (long long)out_size * (long long)T;
        if (need > INT32_MAX) throw Error(SDMI_ERR_INVALID, "resize_weights: table too large");
        if (max_taps) *max_taps = (int32_t)T;
        if (needed) *needed = (int32_t)need;
        if (query) return;
        if ((long long)capacity < need) throw Error(SDMI_ERR_INVALID, "resize_weights: capacity too small");
        for (int o = 0; o < out_size; ++o) {
            const TapRow& r = rows[(size_t)o];
            first[o] = r.first;
            count[o] = (int32_t)r.w.size();
            for (size_t j = 0; j < T; ++j) taps[(size_t)o * T + j] = j < r.w.size() ? r.w[j] : 0.0;
        }
    });
}

// the argument checks the hires entry points share; returns the byte sizes of the base (optional) and the final latent batch
static void hires_sizes(Engine& e, int n, int T, int Tu, const sdmi_hires* hr, size_t* base_bytes, size_t* final_bytes) {
    if (n <= 0 || T <= 0 || Tu <= 0) throw Error(SDMI_ERR_INVALID, "hires: n, T, Tu must be positive");
    Engine::check_hires(hr);
    if (base_bytes) *base_bytes = (size_t)n * 4 * hr->base_h * hr->base_w * sizeof(float);
    *final_bytes = (size_t)n * 4 * e.latent_h() * e.latent_w() * sizeof(float);
}

int sdmi_hires_latent_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                          const float* init_latent, const sdmi_hires* hires, const float* hires_noise, float* latent_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!context || !uncond || !init_latent || !latent_out) throw Error(SDMI_ERR_INVALID, "hires_latent_dev: null pointer");
        Engine::check_hires(hires);
        Engine::Call call(e, /*dev_inputs=*/true);
        e.hires_latent_dev(context, n, T, uncond, Tu, scale, n_steps, init_latent, *hires, hires_noise, latent_out);
        call.finish();
    });
}

int sdmi_hires_image_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                         const float* init_latent, const sdmi_hires* hires, const float* hires_noise, uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!context || !uncond || !init_latent || !rgb_out) throw Error(SDMI_ERR_INVALID, "hires_image_dev: null pointer");
        size_t lat = 0;
        hires_sizes(e, n, T, Tu, hires, nullptr, &lat);
        Engine::Call call(e, /*dev_inputs=*/true);
        Engine::Buf xl(&e, lat);
        e.hires_latent_dev(context, n, T, uncond, Tu, scale, n_steps, init_latent, *hires, hires_noise, xl.f());
        e.decode_latent_dev(xl.f(), n, (float)(1.0 / 0.18215), nullptr, rgb_out);
        call.finish();
    });
}

int sdmi_hires_latent(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                      const float* init_latent, uint64_t seed, const sdmi_hires* hires, const float* hires_noise, float* latent_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        size_t base = 0, lat = 0;
        hires_sizes(e, n, T, Tu, hires, &base, &lat);
        const int cd = e.config().ctx_dim;
        Engine::Call call(e);
        DevIn dc(e, context, (size_t)n * T * cd * sizeof(float)), du(e, uncond, (size_t)Tu * cd * sizeof(float));
        Engine::Buf x0(&e, base);
        make_init_latent(e, init_latent, seed, n, hires->base_h, hires->base_w, x0);
        auto dn = dev_in_opt(e, hires_noise, lat);
        DevOut dout(e, latent_out, lat);
        e.hires_latent_dev(dc.f(), n, T, du.f(), Tu, scale, n_steps, x0.f(), *hires, dn ? dn->f() : nullptr, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_hires_image(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                     const float* init_latent, uint64_t seed, const sdmi_hires* hires, const float* hires_noise, uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        size_t base = 0, lat = 0;
        hires_sizes(e, n, T, Tu, hires, &base, &lat);
        const int cd = e.config().ctx_dim;
        const size_t hw = (size_t)e.latent_h() * e.latent_w();
        Engine::Call call(e);
        DevIn dc(e, context, (size_t)n * T * cd * sizeof(float)), du(e, uncond, (size_t)Tu * cd * sizeof(float));
        Engine::Buf x0(&e, base), xl(&e, lat);
        make_init_latent(e, init_latent, seed, n, hires->base_h, hires->base_w, x0);
        auto dn = dev_in_opt(e, hires_noise, lat);
        DevOut dout(e, rgb_out, (size_t)n * 3 * 64 * hw);
        e.hires_latent_dev(dc.f(), n, T, du.f(), Tu, scale, n_steps, x0.f(), *hires, dn ? dn->f() : nullptr, xl.f());
        e.decode_latent_dev(xl.f(), n, (float)(1.0 / 0.18215), nullptr, reinterpret_cast<uint8_t*>(dout.buf.p));
        call.finish();
        dout.fetch();
    });
}

// ---- LoRA adapters -------------------------------------------------------------------------------------
static sdmi_lora& lora(sdmi_lora* a) {
    if (!a || !a->engine) throw Error(SDMI_ERR_INVALID, "null sdmi_lora");
    return *a;
}

int sdmi_lora_create(sdmi_ctx* ctx, sdmi_lora** out) {
    if (!out) { g_last_error = "sdmi_lora_create: null argument"; return SDMI_ERR_INVALID; }
    *out = nullptr;
    return guarded([&] { *out = eng(ctx).lora_create(); });
}

int sdmi_lora_add(sdmi_lora* a, const char* target, const float* down, const float* up, int32_t rank, float alpha) {
    return guarded([&] { lora(a).engine->lora_add(a, target, down, up, rank, alpha); });
}

int sdmi_lora_load_safetensors(sdmi_ctx* ctx, const char* path, int32_t which, int32_t flags, sdmi_lora** out, int32_t* n_targets, int32_t* n_skipped) {
    if (!out) { g_last_error = "sdmi_lora_load_safetensors: null argument"; return SDMI_ERR_INVALID; }
    *out = nullptr;
    if (n_targets) *n_targets = 0;
    if (n_skipped) *n_skipped = 0;
    return guarded([&] {
        int skipped = 0;
        sdmi_lora* a = eng(ctx).lora_load_safetensors(path, which, flags, &skipped);
        *out = a;
        if (n_targets) *n_targets = (int32_t)a->targets.size();
        if (n_skipped) *n_skipped = skipped;
    });
}

int sdmi_lora_factor_bytes(sdmi_lora* a, size_t* bytes) {
    return guarded([&] {
        if (!bytes) throw Error(SDMI_ERR_INVALID, "lora_factor_bytes: null argument");
        *bytes = lora(a).factor_bytes;
    });
}

int sdmi_lora_module_name(const char* dump_name, char* buf, size_t n) {
    return guarded([&] {
        if (!dump_name || !buf) throw Error(SDMI_ERR_INVALID, "lora_module_name: null argument");
        std::string name;
        if (!sdmi::lora_module_name(dump_name, &name)) throw Error(SDMI_ERR_INVALID, std::string("lora_module_name: '") + dump_name + "' is no conv / Linear weight of the UNet or the text encoder");
        if (n < name.size() + 1) throw Error(SDMI_ERR_INVALID, "lora_module_name: capacity too small");
        std::memcpy(buf, name.c_str(), name.size() + 1);
    });
}

int sdmi_lora_check_safetensors(const char* path, const char* const* names, const int32_t* ndims, const int64_t* dims, int32_t n_entries, int32_t which, int32_t flags,
                                int32_t* n_targets, int32_t* n_skipped) {
    return guarded([&] {
        if (!path || !names || !ndims || !dims || n_entries < 0) throw Error(SDMI_ERR_INVALID, "lora_check_safetensors: null argument");
        std::vector<sdmi::LoraEntryDesc> descs((size_t)n_entries);
        for (int32_t i = 0; i < n_entries; ++i) {
            if (!names[i]) throw Error(SDMI_ERR_INVALID, "lora_check_safetensors: null name");
            sdmi::LoraEntryDesc& d = descs[(size_t)i];
            d.name = names[i];
            d.kind = ndims[i] == 4 ? 0 : ndims[i] == 2 ? 1 : 2;
            for (int k = 0; k < 4; ++k) d.dims[k] = k < ndims[i] ? dims[4 * (size_t)i + k] : 1;
            d.padded = d.kind == 0 && Engine::padded_conv_cin(d.dims[1]) != d.dims[1];
        }
        sdmi::SafetensorsFile f(path);
        const sdmi::LoraFilePlan plan = sdmi::lora_plan_file(f.tensors(), descs, which, flags);
        if (n_targets) *n_targets = (int32_t)plan.targets.size();
        if (n_skipped) *n_skipped = (int32_t)plan.skipped.size();
    });
}

int sdmi_lora_set_scale(sdmi_lora* a, double scale) {
    return guarded([&] { lora(a).engine->lora_set_scale(a, scale); });
}

int sdmi_lora_get_scale(sdmi_lora* a, double* scale, int32_t* n_targets) {
    return guarded([&] {
        if (scale) *scale = lora(a).scale;
        if (n_targets) *n_targets = (int32_t)lora(a).targets.size();
    });
}

int sdmi_lora_destroy(sdmi_lora* a) {
    return guarded([&] { lora(a).engine->lora_destroy(a); });
}

int sdmi_lora_effective_weight(sdmi_ctx* ctx, const char* name, float* out, size_t n) {
    return guarded([&] { eng(ctx).effective_weight(name, out, n); });
}

// The one implementation of the three samplers' rules (include/sdmi.h "sampler choice"): everything in f64.  With sc = sqrt(cur),
// sn = sqrt(1 - cur), sp = sqrt(prev):  x0 = x / sc - (sn / sc) e.
int sdmi_sampler_coefs(const sdmi_sampler* sampler, const float* alphas_cumprod, int32_t total, const int32_t* ts, int32_t count,
                       int64_t step_size, double* coefs) {
    return sdmi_sampler_coefs_ex(sampler, alphas_cumprod, total, ts, count, step_size, 0, coefs);
}

// prediction = 1 (v): eps = sc v + sn x at the step's timestep, and the update is linear in x and in the model output -- the table is rewritten, nothing else changes
int sdmi_sampler_coefs_ex(const sdmi_sampler* sampler, const float* alphas_cumprod, int32_t total, const int32_t* ts, int32_t count,
                          int64_t step_size, int32_t prediction, double* coefs) {
    return guarded([&] {
        if (prediction != 0 && prediction != 1) throw Error(SDMI_ERR_INVALID, "sampler_coefs: prediction must be 0 (eps) or 1 (v)");
        if (!sampler || !alphas_cumprod || !ts || !coefs) throw Error(SDMI_ERR_INVALID, "sampler_coefs: null pointer");
        Engine::check_sampler(*sampler);
        if (total <= 0 || count <= 0 || step_size < 1) throw Error(SDMI_ERR_INVALID, "sampler_coefs: total, count and step_size must be positive");
        for (int32_t j = 0; j < count; ++j)
            if (ts[j] < 0 || ts[j] >= total) throw Error(SDMI_ERR_INVALID, "sampler_coefs: timestep outside [0, total)");
        if (prediction == 0)
            for (int32_t j = 0; j < total; ++j)
                if (alphas_cumprod[j] == 0.0f)
                    throw Error(SDMI_ERR_INVALID, "sampler_coefs: eps-prediction on a schedule that holds alphas_cumprod = 0 (zero terminal SNR): eps does not determine x0 there");
        auto lambda = [](double a) { return 0.5 * std::log(a / (1.0 - a)); };
        static const double AB[4][4] = {{1.0, 0.0, 0.0, 0.0}, {3.0 / 2, -1.0 / 2, 0.0, 0.0}, {23.0 / 12, -16.0 / 12, 5.0 / 12, 0.0},
                                        {55.0 / 24, -59.0 / 24, 37.0 / 24, -9.0 / 24}};
        for (int32_t j = 0; j < count; ++j) {
            const int64_t t = ts[j];
            const double cur = (double)alphas_cumprod[t];
            const double prev = t >= step_size ? (double)alphas_cumprod[t - step_size] : 1.0;
            const double sc = std::sqrt(cur), sn = std::sqrt(1.0 - cur), sp = std::sqrt(prev);
            double* k = coefs + (size_t)j * 8;
            for (int i = 0; i < 8; ++i) k[i] = 0.0;
            if (cur == 0.0) {
                // zero terminal SNR (v only, checked above): the eps basis is singular at a = 0 and v is not -- x0 = -v, eps = x.  The row is
                // written in v at once: x' = sp x0 + dir eps + sigma z.
                const double om = 1.0 - prev;
                if (sampler->kind == 0) {
                    const double sigma = sampler->eta * std::sqrt(om);
                    k[0] = std::sqrt(om - sigma * sigma);
                    k[1] = -sp;
                    k[5] = sigma;
                } else if (sampler->kind == 1) {
                    k[6] = 0.0; k[7] = -1.0;                    // q = x0 = -v
                    if (prev >= 1.0) { k[0] = 0.0; k[1] = -1.0; }
                    else { k[0] = std::sqrt(om); k[1] = -sp; }  // h = inf: first order whatever came before, no weight on the history
                } else {
                    k[0] = std::sqrt(om);
                    k[1] = -sp;
                    k[6] = 1.0; k[7] = 0.0;                     // q = eps = x: the model output has no part in it
                }
                continue;
            }
            if (sampler->kind == 0) {
                const double sigma = sampler->eta * std::sqrt((1.0 - prev) / (1.0 - cur)) * std::sqrt(1.0 - cur / prev);
                const double dir = std::sqrt(1.0 - prev - sigma * sigma);
                k[0] = sp / sc;
                k[1] = dir - sp * sn / sc;
                k[5] = sigma;                                   // exactly 0 where eta = 0 or prev = 1
            } else if (sampler->kind == 1) {
                const double qx = 1.0 / sc, qe = -sn / sc;      // q = x0
                k[6] = qx; k[7] = qe;
                if (prev >= 1.0) {                              // the limit h -> inf: x' = x0, the weight on x itself exactly 0
                    k[0] = qx; k[1] = qe;
                } else {
                    const double h = lambda(prev) - lambda(cur);
                    const double A = std::sqrt((1.0 - prev) / (1.0 - cur)), B = -sp * std::expm1(-h);
                    double w0 = 1.0, w1 = 0.0;
                    if (j > 0 && alphas_cumprod[ts[j - 1]] != 0.0f) {   // (behind a zero row lambda = -inf, r = +inf: first order, written out)
                        const double r = (lambda(cur) - lambda((double)alphas_cumprod[ts[j - 1]])) / h;
                        w0 = 1.0 + 1.0 / (2.0 * r);
                        w1 = -1.0 / (2.0 * r);
                    }
                    k[0] = A + B * w0 * qx;
                    k[1] = B * w0 * qe;
                    k[2] = B * w1;
                }
            } else {
                const double ce = std::sqrt(1.0 - prev) - sp * sn / sc;   // the eta = 0 update's weight on e, spread over e' = sum w e_-i
                const double* w = AB[j < 3 ? j : 3];
                k[0] = sp / sc;
                k[1] = ce * w[0]; k[2] = ce * w[1]; k[3] = ce * w[2]; k[4] = ce * w[3];
                k[7] = 1.0;                                     // q = e
            }
            if (prediction == 1) { k[0] += k[1] * sn; k[1] *= sc; k[6] += k[7] * sn; k[7] *= sc; }
        }
    });
}

int sdmi_set_prediction(sdmi_ctx* ctx, int32_t kind) {
    return guarded([&] { eng(ctx).set_prediction(kind); });
}

// ---- CFG rescale and zero-terminal-SNR schedules ---------------------------------------------------------------------
int sdmi_set_guidance_rescale(sdmi_ctx* ctx, double phi) {
    return guarded([&] { eng(ctx).set_guidance_rescale(phi); });
}

int sdmi_rescale_zero_snr(const float* in, float* out, int32_t n) {
    return guarded([&] { Engine::rescale_zero_snr(in, out, n); });
}

int sdmi_set_zero_snr(sdmi_ctx* ctx, int32_t on) {
    return guarded([&] { eng(ctx).set_zero_snr(on != 0); });
}

int sdmi_schedule(sdmi_ctx* ctx, float* out, int32_t capacity, int32_t* count) {
    return guarded([&] {
        const std::vector<float>& a = eng(ctx).alphas();
        if (!count) throw Error(SDMI_ERR_INVALID, "schedule: count is NULL");
        *count = (int32_t)a.size();
        if (!out) return;   // the size alone
        if (capacity < (int32_t)a.size()) throw Error(SDMI_ERR_INVALID, "schedule: capacity below the table's " + std::to_string(a.size()) + " entries");
        std::copy(a.begin(), a.end(), out);
    });
}

int sdmi_img2img_latent(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale,
                        size_t n_steps, double strength, const float* z0, const float* mask, const float* noise, uint64_t seed,
                        float* latent_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || T <= 0 || Tu <= 0) throw Error(SDMI_ERR_INVALID, "img2img_latent: n, T, Tu must be positive");
        const int cd = e.config().ctx_dim;
        const size_t hw = (size_t)e.latent_h() * e.latent_w(), lat = (size_t)n * 4 * hw * sizeof(float);
        Engine::Call call(e);
        DevIn dc(e, context, (size_t)n * T * cd * sizeof(float)), du(e, uncond, (size_t)Tu * cd * sizeof(float)), dz(e, z0, lat);
        auto dm = dev_in_opt(e, mask, (size_t)n * hw * sizeof(float));
        auto dn = dev_in_opt(e, noise, lat);
        DevOut dout(e, latent_out, lat);
        e.img2img_latent_dev(dc.f(), n, T, du.f(), Tu, scale, n_steps, strength, dz.f(), dm ? dm->f() : nullptr, dn ? dn->f() : nullptr, seed,
                             dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_img2img_image(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale,
                       size_t n_steps, double strength, const uint8_t* init_rgb, const float* mask, const float* noise, uint64_t seed,
                       uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || T <= 0 || Tu <= 0) throw Error(SDMI_ERR_INVALID, "img2img_image: n, T, Tu must be positive");
        const int cd = e.config().ctx_dim;
        const size_t hw = (size_t)e.latent_h() * e.latent_w(), lat = (size_t)n * 4 * hw * sizeof(float);
        Engine::Call call(e);
        DevIn dc(e, context, (size_t)n * T * cd * sizeof(float)), du(e, uncond, (size_t)Tu * cd * sizeof(float));
        DevIn drgb(e, init_rgb, (size_t)n * 3 * 64 * hw);
        auto dm = dev_in_opt(e, mask, (size_t)n * hw * sizeof(float));
        auto dn = dev_in_opt(e, noise, lat);
        Engine::Buf xl(&e, lat);
        DevOut dout(e, rgb_out, (size_t)n * 3 * 64 * hw);
        e.img2img_image_dev(dc.f(), n, T, du.f(), Tu, scale, n_steps, strength, reinterpret_cast<const uint8_t*>(drgb.buf.p),
                            dm ? dm->f() : nullptr, dn ? dn->f() : nullptr, seed, xl.f());
        e.decode_latent_dev(xl.f(), n, (float)(1.0 / 0.18215), nullptr, reinterpret_cast<uint8_t*>(dout.buf.p));
        call.finish();
        dout.fetch();
    });
}

// ---- conditioned UNet input and inpainting -----------------------------------------------------------------------------
int sdmi_inpaint_latent_mask(const uint8_t* mask_u8, int32_t n, int32_t h, int32_t w, float* out) {
    return guarded([&] {
        if (!mask_u8 || !out) throw Error(SDMI_ERR_INVALID, "inpaint_latent_mask: null pointer");
        if (n < 1 || h < 1 || w < 1) throw Error(SDMI_ERR_INVALID, "inpaint_latent_mask: n, h and w must be positive (the mask is n x [8h, 8w])");
        for (int64_t b = 0; b < n; ++b)
            for (int64_t y = 0; y < h; ++y)
                for (int64_t x = 0; x < w; ++x) out[(b * h + y) * w + x] = mask_u8[(b * 8 * h + 8 * y) * 8 * w + 8 * x] >= 128 ? 1.0f : 0.0f;
    });
}

int sdmi_unet_forward_cond(sdmi_ctx* ctx, const float* x, int32_t t, const float* context, const float* cond, int32_t n, int32_t T, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        e.check_cond("unet_forward_cond", true);
        if (!cond) throw Error(SDMI_ERR_INVALID, "unet_forward_cond: null cond");
        if (n <= 0 || T <= 0) throw Error(SDMI_ERR_INVALID, "unet_forward_cond: n and T must be positive");
        const size_t hw = (size_t)e.latent_h() * e.latent_w(), lat = (size_t)n * 4 * hw * sizeof(float);
        Engine::Call call(e);
        DevIn dx(e, x, lat), dc(e, context, (size_t)n * T * e.config().ctx_dim * sizeof(float)), dk(e, cond, (size_t)n * e.cond_ch() * hw * sizeof(float));
        DevOut dout(e, out, lat);
        e.unet_forward_dev(dx.f(), t, dc.f(), n, T, dout.f(), dk.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_img2img_latent_cond_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                                 double strength, const float* z0, const float* mask, const float* noise, uint64_t seed, const float* cond, float* latent_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        e.check_cond("img2img_latent_cond_dev", true);
        if (!cond) throw Error(SDMI_ERR_INVALID, "img2img_latent_cond_dev: null cond");
        if (!context || !uncond || !z0 || !latent_out) throw Error(SDMI_ERR_INVALID, "img2img_latent_cond_dev: null pointer");
        Engine::Call call(e, /*dev_inputs=*/true);
        e.img2img_latent_dev(context, n, T, uncond, Tu, scale, n_steps, strength, z0, mask, noise, seed, latent_out, cond);
        call.finish();
    });
}

int sdmi_img2img_latent_cond(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                             double strength, const float* z0, const float* mask, const float* noise, uint64_t seed, const float* cond, float* latent_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        e.check_cond("img2img_latent_cond", true);
        if (!cond) throw Error(SDMI_ERR_INVALID, "img2img_latent_cond: null cond");
        if (n <= 0 || T <= 0 || Tu <= 0) throw Error(SDMI_ERR_INVALID, "img2img_latent_cond: n, T, Tu must be positive");
        const int cd = e.config().ctx_dim;
        const size_t hw = (size_t)e.latent_h() * e.latent_w(), lat = (size_t)n * 4 * hw * sizeof(float);
        Engine::Call call(e);
        DevIn dc(e, context, (size_t)n * T * cd * sizeof(float)), du(e, uncond, (size_t)Tu * cd * sizeof(float)), dz(e, z0, lat);
        DevIn dk(e, cond, (size_t)n * e.cond_ch() * hw * sizeof(float));
        auto dm = dev_in_opt(e, mask, (size_t)n * hw * sizeof(float));
        auto dn = dev_in_opt(e, noise, lat);
        DevOut dout(e, latent_out, lat);
        e.img2img_latent_dev(dc.f(), n, T, du.f(), Tu, scale, n_steps, strength, dz.f(), dm ? dm->f() : nullptr, dn ? dn->f() : nullptr, seed, dout.f(), dk.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_inpaint_cond(sdmi_ctx* ctx, const uint8_t* init_rgb, const uint8_t* mask_u8, int32_t n, float* cond_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        e.check_inpaint("inpaint_cond");
        if (!init_rgb || !mask_u8 || !cond_out) throw Error(SDMI_ERR_INVALID, "inpaint_cond: null pointer");
        if (n <= 0) throw Error(SDMI_ERR_INVALID, "inpaint_cond: n must be positive");
        const size_t hw = (size_t)e.latent_h() * e.latent_w();
        Engine::Call call(e);
        DevIn drgb(e, init_rgb, (size_t)n * 3 * 64 * hw), dm(e, mask_u8, (size_t)n * 64 * hw);
        DevOut dout(e, cond_out, (size_t)n * 5 * hw * sizeof(float));
        e.inpaint_cond_dev(reinterpret_cast<const uint8_t*>(drgb.buf.p), reinterpret_cast<const uint8_t*>(dm.buf.p), n, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_inpaint_image_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps, double strength,
                           const uint8_t* init_rgb, const uint8_t* mask_u8, const sdmi_inpaint* opt, const float* noise, uint64_t seed, uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        e.check_inpaint("inpaint_image_dev");
        if (!context || !uncond || !init_rgb || !mask_u8 || !rgb_out) throw Error(SDMI_ERR_INVALID, "inpaint_image_dev: null pointer");
        Engine::Call call(e, /*dev_inputs=*/true);
        e.inpaint_image_dev(context, n, T, uncond, Tu, scale, n_steps, strength, init_rgb, mask_u8, opt, noise, seed, rgb_out);
        call.finish();
    });
}

int sdmi_inpaint_image(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps, double strength,
                       const uint8_t* init_rgb, const uint8_t* mask_u8, const sdmi_inpaint* opt, const float* noise, uint64_t seed, uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        e.check_inpaint("inpaint_image");
        if (!init_rgb || !mask_u8) throw Error(SDMI_ERR_INVALID, "inpaint_image: null pointer");
        if (n <= 0 || T <= 0 || Tu <= 0) throw Error(SDMI_ERR_INVALID, "inpaint_image: n, T, Tu must be positive");
        const int cd = e.config().ctx_dim;
        const size_t hw = (size_t)e.latent_h() * e.latent_w(), lat = (size_t)n * 4 * hw * sizeof(float);
        Engine::Call call(e);
        DevIn dc(e, context, (size_t)n * T * cd * sizeof(float)), du(e, uncond, (size_t)Tu * cd * sizeof(float));
        DevIn drgb(e, init_rgb, (size_t)n * 3 * 64 * hw), dm(e, mask_u8, (size_t)n * 64 * hw);
        auto dn = dev_in_opt(e, noise, lat);
        DevOut dout(e, rgb_out, (size_t)n * 3 * 64 * hw);
        e.inpaint_image_dev(dc.f(), n, T, du.f(), Tu, scale, n_steps, strength, reinterpret_cast<const uint8_t*>(drgb.buf.p), reinterpret_cast<const uint8_t*>(dm.buf.p),
                            opt, dn ? dn->f() : nullptr, seed, reinterpret_cast<uint8_t*>(dout.buf.p));
        call.finish();
        dout.fetch();
    });
}

int sdmi_decode_latent(sdmi_ctx* ctx, const float* latent, int32_t n, float* img_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0) throw Error(SDMI_ERR_INVALID, "decode_latent: n must be positive");
        const size_t hw = (size_t)e.latent_h() * e.latent_w();
        Engine::Call call(e);
        DevIn dl(e, latent, (size_t)n * 4 * hw * sizeof(float));
        DevOut dout(e, img_out, (size_t)n * 3 * 64 * hw * sizeof(float));
        e.decode_latent_dev(dl.f(), n, 1.0f, dout.f(), nullptr);
        call.finish();
        dout.fetch();
    });
}

int sdmi_latent_to_image(sdmi_ctx* ctx, const float* latent, int32_t n, uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0) throw Error(SDMI_ERR_INVALID, "latent_to_image: n must be positive");
        const size_t hw = (size_t)e.latent_h() * e.latent_w();
        Engine::Call call(e);
        DevIn dl(e, latent, (size_t)n * 4 * hw * sizeof(float));
        DevOut dout(e, rgb_out, (size_t)n * 3 * 64 * hw);
        e.decode_latent_dev(dl.f(), n, (float)(1.0 / 0.18215), nullptr, reinterpret_cast<uint8_t*>(dout.buf.p));
        call.finish();
        dout.fetch();
    });
}

int sdmi_sample_image(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu,
                      double scale, size_t n_steps, const float* init_latent, uint64_t seed, uint8_t* rgb_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || T <= 0 || Tu <= 0) throw Error(SDMI_ERR_INVALID, "sample_image: n, T, Tu must be positive");
        const int cd = e.config().ctx_dim;
        const size_t hw = (size_t)e.latent_h() * e.latent_w();
        const size_t lat = (size_t)n * 4 * hw * sizeof(float);
        Engine::Call call(e);
        DevIn dc(e, context, (size_t)n * T * cd * sizeof(float)), du(e, uncond, (size_t)Tu * cd * sizeof(float));
        Engine::Buf x0(&e, lat), xl(&e, lat);
        make_init_latent(e, init_latent, seed, n, e.latent_h(), e.latent_w(), x0);
        DevOut dout(e, rgb_out, (size_t)n * 3 * 64 * hw);
        e.sample_latent_dev(dc.f(), n, T, du.f(), Tu, scale, n_steps, x0.f(), xl.f());
        e.decode_latent_dev(xl.f(), n, (float)(1.0 / 0.18215), nullptr, reinterpret_cast<uint8_t*>(dout.buf.p));
        call.finish();
        dout.fetch();
    });
}

int sdmi_qkv_attention(sdmi_ctx* ctx, const float* q, const float* k, const float* v, const float* mask,
                       int32_t mask_ld, int32_t n, int32_t nq, int32_t nk, int32_t n_state, int32_t n_head, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || nq <= 0 || nk <= 0 || n_state <= 0) throw Error(SDMI_ERR_INVALID, "qkv_attention: bad shape");
        const size_t qb = (size_t)n * nq * n_state * sizeof(float), kb = (size_t)n * nk * n_state * sizeof(float);
        Engine::Call call(e);
        DevIn dq(e, q, qb), dk(e, k, kb), dv(e, v, kb);
        Engine::Buf dm(&e, mask ? (size_t)nq * mask_ld * sizeof(float) : 256);
        if (mask) SDMI_HIP(hipMemcpyAsync(dm.p, mask, (size_t)nq * mask_ld * sizeof(float), hipMemcpyHostToDevice, e.stream()));
        DevOut dout(e, out, qb);
        e.qkv_attention_dev(dq.f(), dk.f(), dv.f(), mask ? dm.f() : nullptr, mask_ld, n, nq, nk, n_state, n_head, dout.f());
        call.finish();
        dout.fetch();
    });
}

// ---- tuning / introspection --------------------------------------------------------------------
int sdmi_set_option(sdmi_ctx* ctx, const char* key, const char* value) {
    return guarded([&] {
        if (!key || !value) throw Error(SDMI_ERR_INVALID, "set_option: null argument");
        eng(ctx).set_option(key, value);
    });
}

int sdmi_last_call_stats(sdmi_ctx* ctx, double* gpu_ms, int64_t* n_kernels, double* flops) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (gpu_ms) *gpu_ms = e.last_ms;
        if (n_kernels) *n_kernels = e.last_kernels;
        if (flops) *flops = e.last_flops;
    });
}

int sdmi_profile_stats(sdmi_ctx* ctx, int32_t cls, double* ms, int64_t* launches, double* flops, double* bytes) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (cls < 0 || cls >= Engine::PC_COUNT) throw Error(SDMI_ERR_INVALID, "profile_stats: class out of range");
        e.prof_flush();
        if (ms) *ms = e.prof_[cls].ms;
        if (launches) *launches = e.prof_[cls].launches;
        if (flops) *flops = e.prof_[cls].flops;
        if (bytes) *bytes = e.prof_[cls].bytes;
    });
}

int sdmi_profile_overhead(sdmi_ctx* ctx, double* ms) {
    return guarded([&] {
        if (!ms) throw Error(SDMI_ERR_INVALID, "profile_overhead: null output");
        *ms = eng(ctx).prof_overhead_ms_;
    });
}

}  // extern "C"
