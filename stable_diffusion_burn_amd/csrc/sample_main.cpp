// sdmi_sample -- the C++ twin of the reference's `sample` binary (src/bin/sample/main.rs:36-125), same argv:
//
//   sdmi_sample <model_type(burn, dump or safetensors)> <model_name> <unconditional_guidance_scale> <n_diffusion_steps>
//               <prompt> <output_image_name> [device]
//
// It is a pure consumer of the C ABI (include/sdmi.h) -- the same calls the Rust shim (ffi/sdmi.rs) makes:
// tokenizer -> CLIP context -> sample_image -> PNG.  Differences from the reference, all forced:
//   * model_type "burn" reads the NamedMpkFileRecorder<FullPrecisionSettings> record "<model_name>.mpk" natively (the
//     recorder sets the extension itself, main.rs:27-34; layout assumptions: csrc/mpk_reader.hpp); "dump" is the npy tree
//     of python/dump.py (main.rs:94); "safetensors" (no reference counterpart) is an SD v1.x checkpoint in the CompVis layout, <model_name> its file;
//   * the usage line names the third model type, "safetensors"; every other message, and what "burn" and "dump" do, is unchanged;
//   * device is "hip", "hip:N" or "cuda[N]" (alias, index N); "cpu" / "mps" are refused -- there is no CPU path;
//   * the reference's noise is unseeded; here SDMI_SEED (default 0) seeds the device generator;
//   * the merges file is $SDMI_BPE_VOCAB, default "bpe_simple_vocab_16e6.txt" in the working directory (tokenizer.rs:91);
//   * SDMI_CONFIG="key=value,..." overrides model dimensions (tests use a small model).
//   * SDMI_PROMPT_STYLE=webui (no reference counterpart; unset: everything as above) encodes the prompt and the negative prompt with sdmi_encode_prompt --
//     chunks padded to clip_ctx tokens, emphasis, BREAK, no length limit.  In that mode only, SDMI_NEGATIVE_PROMPT (default "") replaces the empty prompt and
//     SDMI_CLIP_SKIP (default 1) is passed on; the negative prompt is brought to the prompt's chunk count.
//   * SDMI_LORA=<file>[:scale[:te_scale]] (no reference counterpart) attaches a kohya-ss / LyCORIS LoRA .safetensors file before the prompt is encoded
//     (sdmi_lora_load_safetensors): scale defaults to 1, te_scale -- the text encoder's -- to scale.  It sets the engine option keep_masters itself.  Only finite
//     decimal numbers are scales; a file name that itself ends in ":<number>" needs its scale spelled out ("name:2:1").
//   * SDMI_KSAMPLER=kind:schedule[:eta] (no reference counterpart; unset: the reference's DDIM) selects a sigma-schedule sampler (sdmi_set_ksampler) by name:
//     kind euler | dpmpp_2m | heun | dpm2 | dpmpp_2s | dpmpp_sde | dpmpp_2m_sde, schedule model | karras | exponential | uniform, eta 0 .. 1 (default 0); its step
//     noise is seeded by SDMI_SEED.
//   * SDMI_PREDICTION=v | eps (no reference counterpart; unset: eps) says what the checkpoint's UNet predicts (sdmi_set_prediction): v for SD 2.x's 768-v models.  An
//     SD 2.x checkpoint needs SDMI_CONFIG="variant=1,ctx_dim=1024,clip_layers=23,clip_heads=16" and, for OpenCLIP's padding, SDMI_PROMPT_STYLE=webui.
//   * SDMI_GUIDANCE_RESCALE=phi (0 .. 1; unset: 0, off) and SDMI_ZERO_SNR=1 (no reference counterpart): CFG rescale
//     (sdmi_set_guidance_rescale) and the schedule rescaled to zero terminal SNR (sdmi_set_zero_snr; needs SDMI_PREDICTION=v) -- what the 768-v models and most
//     v-prediction fine-tunes are sampled with (phi = 0.7).
//   * SDMI_IP_ADAPTER=<file>[:scale[:start:end]] with SDMI_IP_EMBEDS=<.safetensors holding "image_embeds" [n, D]> (no reference counterpart; DESIGN.md section 9m;
//     unset: off) loads an IP-Adapter (sdmi_ip_adapter_load_safetensors) and sets the caller's CLIP image embeddings as the image prompt (sdmi_set_ip_adapter_file).
//   * SDMI_FREEU=b1:b2:s1:s2[:version] (no reference counterpart; unset: off) switches FreeU on (sdmi_set_freeu) for every step: version 1
//     (the default) or 2 (ComfyUI's FreeU_V2).  The paper's values for SD 1.4 are 1.2:1.4:0.9:0.2, for SD 2.1 1.1:1.2:0.9:0.2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sdmi.h"

static void die(const char* what) {
    std::fprintf(stderr, "%s: %s\n", what, sdmi_last_error());
    std::exit(1);
}

static void apply_overrides(sdmi_config& cfg, const char* spec) {
    std::string s(spec);
    size_t pos = 0;
    while (pos < s.size()) {
        size_t end = s.find(',', pos);
        if (end == std::string::npos) end = s.size();
        const std::string kv = s.substr(pos, end - pos);
        pos = end + 1;
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) continue;
        const std::string k = kv.substr(0, eq);
        const int v = std::atoi(kv.c_str() + eq + 1);
        if (k == "model_channels") cfg.model_channels = v;
        else if (k == "n_head") cfg.n_head = v;
        else if (k == "ctx_dim") cfg.ctx_dim = v;
        else if (k == "latent_h") cfg.latent_h = v;
        else if (k == "latent_w") cfg.latent_w = v;
        else if (k == "vae_ch") cfg.vae_ch = v;
        else if (k == "precision") cfg.precision = v;
        else if (k == "clip_layers") cfg.clip_layers = v;
        else if (k == "clip_heads") cfg.clip_heads = v;
        else if (k == "clip_vocab") cfg.clip_vocab = v;
        else if (k == "clip_ctx") cfg.clip_ctx = v;
        else if (k == "variant") cfg.variant = v;
        else { std::fprintf(stderr, "SDMI_CONFIG: unknown key %s\n", k.c_str()); std::exit(1); }
    }
}

// a complete, finite decimal number ("0.8", "-1", "1e-1"): nothing strtod would also take -- "inf", "nan", hexadecimal floats -- counts as a scale
static bool decimal_scale(const char* s, double* v) {
    if (!*s || std::strspn(s, "0123456789+-.eE") != std::strlen(s)) return false;
    char* end = nullptr;
    *v = std::strtod(s, &end);
    return end != s && *end == '\0' && *v - *v == 0.0;
}

// "<file>[:scale[:te_scale]]": up to two trailing ':'-separated fields that are decimal numbers are scales, the rest is the path (which may hold ':' itself).
// A path whose own last field is a decimal number ("dir:2") is therefore written with its scale: "dir:2:1".
static std::string parse_lora_spec(const char* spec, double* scale, double* te_scale, bool* has_te) {
    std::string path(spec);
    double found[2];
    int n = 0;
    while (n < 2) {
        const size_t colon = path.rfind(':');
        double v;
        if (colon == std::string::npos || colon == 0 || !decimal_scale(path.c_str() + colon + 1, &v)) break;
        found[n++] = v;
        path.resize(colon);
    }
    *scale = n ? found[n - 1] : 1.0;
    *has_te = n == 2;
    *te_scale = n == 2 ? found[0] : *scale;
    return path;
}

// "kind:schedule[:eta]" by name; false for a name or a number that is none
static bool parse_ksampler_spec(const char* spec, sdmi_ksampler* k) {
    static const char* const kinds[] = {"euler", "dpmpp_2m", "heun", "dpm2", "dpmpp_2s", "dpmpp_sde", "dpmpp_2m_sde"};
    static const char* const schedules[] = {"model", "karras", "exponential", "uniform"};
    const std::string s(spec);
    const size_t c1 = s.find(':');
    if (c1 == std::string::npos) return false;
    const size_t c2 = s.find(':', c1 + 1);
    const std::string kind = s.substr(0, c1), sched = s.substr(c1 + 1, c2 == std::string::npos ? std::string::npos : c2 - c1 - 1);
    *k = sdmi_ksampler{};
    k->kind = k->schedule = -1;
    for (int i = 0; i < 7; ++i) if (kind == kinds[i]) k->kind = i;
    for (int i = 0; i < 4; ++i) if (sched == schedules[i]) k->schedule = i;
    if (k->kind < 0 || k->schedule < 0) return false;
    if (c2 != std::string::npos) {
        const std::string eta = s.substr(c2 + 1);
        char* end = nullptr;
        k->eta = std::strtod(eta.c_str(), &end);
        if (eta.empty() || *end) return false;
    }
    return true;
}

static void attach_lora(sdmi_ctx* ctx, const char* spec) {
    double scale, te_scale;
    bool has_te;
    const std::string path = parse_lora_spec(spec, &scale, &te_scale, &has_te);
    const int32_t which[2] = {has_te ? SDMI_LORA_UNET : (SDMI_LORA_UNET | SDMI_LORA_TE), SDMI_LORA_TE};
    const double scales[2] = {scale, te_scale};
    for (int i = 0; i < (has_te ? 2 : 1); ++i) {
        sdmi_lora* a = nullptr;   // owned by the context: freed by sdmi_destroy
        int32_t n = 0, skipped = 0;
        if (sdmi_lora_load_safetensors(ctx, path.c_str(), which[i], 0, &a, &n, &skipped) != SDMI_OK || sdmi_lora_set_scale(a, scales[i]) != SDMI_OK) die("Error loading LoRA");
        std::printf("LoRA %s: %d targets at scale %g\n", path.c_str(), (int)n, scales[i]);
    }
}

int main(int argc, char** argv) {
    if (argc != 7 && argc != 8) {
        std::fprintf(stderr, "Usage: %s <model_type(burn, dump or safetensors)> <model_name> <unconditional_guidance_scale> <n_diffusion_steps> <prompt> <output_image_name> [device(hip, hip:N)]\n", argv[0]);
        return 1;
    }
    const std::string model_type = argv[1], model_name = argv[2], prompt = argv[5], output = argv[6];
    char* endp = nullptr;
    const double scale = std::strtod(argv[3], &endp);
    if (endp == argv[3] || *endp) { std::fprintf(stderr, "Error: Invalid unconditional guidance scale.\n"); return 1; }
    const long long steps = std::strtoll(argv[4], &endp, 10);
    if (endp == argv[4] || *endp || steps < 0) { std::fprintf(stderr, "Error: Invalid number of diffusion steps.\n"); return 1; }

    sdmi_config cfg;
    sdmi_default_config(&cfg);
    if (argc == 8) {
        std::string d = argv[7];
        for (auto& c : d) c = (char)std::tolower((unsigned char)c);
        if (d.rfind("hip", 0) == 0 || d.rfind("cuda", 0) == 0) {
            const size_t digits = d.find_first_of("0123456789");
            cfg.device = digits == std::string::npos ? 0 : std::atoi(d.c_str() + digits);
        } else {
            std::fprintf(stderr, "Unknown device: %s (this build runs on MI355X only: hip or hip:N)\n", argv[7]);
            return 1;
        }
    }
    if (const char* o = std::getenv("SDMI_CONFIG")) apply_overrides(cfg, o);
    if (cfg.clip_layers <= 0) { std::fprintf(stderr, "Error: the sample binary needs the CLIP text encoder (clip_layers > 0)\n"); return 1; }

    // SDMI_KSAMPLER: a spec that names no sampler ends the run before anything is loaded
    sdmi_ksampler ksampler;
    const char* ks = std::getenv("SDMI_KSAMPLER");
    const bool has_ksampler = ks && *ks;
    if (has_ksampler) {
        if (!parse_ksampler_spec(ks, &ksampler)) { std::fprintf(stderr, "Error: SDMI_KSAMPLER must be kind:schedule[:eta], got '%s'\n", ks); return 1; }
        if (const char* sd = std::getenv("SDMI_SEED")) ksampler.noise_seed = std::strtoull(sd, nullptr, 10);
    }

    // SDMI_PREDICTION: likewise refused before anything is loaded
    int32_t prediction = 0;
    if (const char* pr = std::getenv("SDMI_PREDICTION")) {
        if (!std::strcmp(pr, "v")) prediction = 1;
        else if (*pr && std::strcmp(pr, "eps")) { std::fprintf(stderr, "Error: SDMI_PREDICTION must be v or eps, got '%s'\n", pr); return 1; }
    }
    // SDMI_GUIDANCE_RESCALE / SDMI_ZERO_SNR: likewise
    double guidance_rescale = 0.0;
    if (const char* gr = std::getenv("SDMI_GUIDANCE_RESCALE")) {
        char* end = nullptr;
        guidance_rescale = std::strtod(gr, &end);
        if (!*gr || *end || !(guidance_rescale >= 0.0 && guidance_rescale <= 1.0)) {
            std::fprintf(stderr, "Error: SDMI_GUIDANCE_RESCALE must be a number in [0, 1], got '%s'\n", gr);
            return 1;
        }
    }
    int32_t zero_snr = 0;
    if (const char* zs = std::getenv("SDMI_ZERO_SNR")) {
        if (!std::strcmp(zs, "1")) zero_snr = 1;
        else if (*zs && std::strcmp(zs, "0")) { std::fprintf(stderr, "Error: SDMI_ZERO_SNR must be 0 or 1, got '%s'\n", zs); return 1; }
    }
    // SDMI_FREEU: likewise
    int32_t freeu_version = 0;
    float freeu_p[4] = {1.f, 1.f, 1.f, 1.f};
    if (const char* fu = std::getenv("SDMI_FREEU")) {
        if (*fu) {
            double v[5] = {0, 0, 0, 0, 1};
            int got = 0;
            const char* q = fu;
            bool ok = true;
            while (ok && got < 5) {
                char* end = nullptr;
                v[got] = std::strtod(q, &end);
                if (end == q) { ok = false; break; }
                ++got;
                if (!*end) break;
                if (*end != ':') { ok = false; break; }
                q = end + 1;
                if (got == 5) ok = false;
            }
            if (!ok || got < 4 || !(v[4] == 1 || v[4] == 2)) {
                std::fprintf(stderr, "Error: SDMI_FREEU must be b1:b2:s1:s2[:version] with version 1 or 2, got '%s'\n", fu);
                return 1;
            }
            for (int i = 0; i < 4; ++i) freeu_p[i] = (float)v[i];
            freeu_version = (int32_t)v[4];
        }
    }
    // SDMI_IP_ADAPTER=<file>[:scale[:start:end]] + SDMI_IP_EMBEDS=<.safetensors holding "image_embeds" [n, D]>: an image prompt
    std::string ip_file;
    double ip_p[3] = {1.0, 0.0, 1.0};
    const char* ip_embeds = std::getenv("SDMI_IP_EMBEDS");
    if (const char* ia = std::getenv("SDMI_IP_ADAPTER")) {
        if (*ia) {
            std::vector<std::string> parts;
            std::string cur;
            for (const char* q = ia;; ++q) {
                if (*q == ':' || !*q) { parts.push_back(cur); cur.clear(); if (!*q) break; }
                else cur += *q;
            }
            bool ok = parts.size() == 1 || parts.size() == 2 || parts.size() == 4;
            ip_file = parts[0];
            for (size_t i = 1; ok && i < parts.size(); ++i) {
                char* end = nullptr;
                ip_p[i - 1] = std::strtod(parts[i].c_str(), &end);
                if (end == parts[i].c_str() || *end) ok = false;
            }
            if (!ok || ip_file.empty()) { std::fprintf(stderr, "Error: SDMI_IP_ADAPTER must be <file>[:scale[:start:end]], got '%s'\n", ia); return 1; }
            if (!ip_embeds || !*ip_embeds) { std::fprintf(stderr, "Error: SDMI_IP_ADAPTER needs SDMI_IP_EMBEDS=<.safetensors holding \"image_embeds\" [n, D]>\n"); return 1; }
        }
    }
    if (zero_snr && prediction != 1) { std::fprintf(stderr, "Error: SDMI_ZERO_SNR=1 needs SDMI_PREDICTION=v (eps does not determine x0 where alphas_cumprod is 0)\n"); return 1; }
    if (zero_snr && has_ksampler) { std::fprintf(stderr, "Error: SDMI_ZERO_SNR=1 excludes SDMI_KSAMPLER (sigma_max is infinite)\n"); return 1; }

    std::printf("Loading tokenizer...\n");
    const char* vocab = std::getenv("SDMI_BPE_VOCAB");
    sdmi_tokenizer* tok = nullptr;
    if (sdmi_tokenizer_create(&tok, vocab ? vocab : "bpe_simple_vocab_16e6.txt") != SDMI_OK) die("Error loading tokenizer");

    std::printf("Loading model...\n");
    sdmi_ctx* ctx = nullptr;
    if (sdmi_create(&ctx, &cfg) != SDMI_OK) die("Error creating device context");
    if (has_ksampler && sdmi_set_ksampler(ctx, &ksampler) != SDMI_OK) die("Error setting the k-sampler");   // sticky: set before the weights, refused at once
    if (sdmi_set_prediction(ctx, prediction) != SDMI_OK) die("Error setting the prediction kind");
    if (sdmi_set_guidance_rescale(ctx, guidance_rescale) != SDMI_OK) die("Error setting the guidance rescale");
    if (sdmi_set_zero_snr(ctx, zero_snr) != SDMI_OK) die("Error setting the zero-terminal-SNR schedule");
    if (freeu_version && sdmi_set_freeu(ctx, freeu_version, freeu_p[0], freeu_p[1], freeu_p[2], freeu_p[3], 0.0, 1.0) != SDMI_OK) die("Error setting FreeU");
    const char* lora = std::getenv("SDMI_LORA");
    if (lora && *lora && sdmi_set_option(ctx, "keep_masters", "1") != SDMI_OK) die("Error setting keep_masters");
    if (model_type == "burn") {
        std::string file = model_name;
        if (file.size() < 4 || file.compare(file.size() - 4, 4, ".mpk") != 0) file += ".mpk";   // FileRecorder::load sets the extension
        if (sdmi_load_weights_mpk(ctx, file.c_str()) != SDMI_OK || sdmi_finalize_weights(ctx) != SDMI_OK) die("Error loading model");
    } else if (model_type == "safetensors") {
        if (sdmi_load_weights_safetensors(ctx, model_name.c_str()) != SDMI_OK || sdmi_finalize_weights(ctx) != SDMI_OK) die("Error loading checkpoint");
    } else if (sdmi_load_weights_dir(ctx, model_name.c_str()) != SDMI_OK || sdmi_finalize_weights(ctx) != SDMI_OK) {
        die("Error loading model dump");
    }
    if (lora && *lora) attach_lora(ctx, lora);
    if (!ip_file.empty()) {
        if (sdmi_ip_adapter_load_safetensors(ctx, ip_file.c_str()) != SDMI_OK) die("Error loading the IP-Adapter");
        if (sdmi_set_ip_adapter_file(ctx, ip_embeds, (float)ip_p[0], ip_p[1], ip_p[2]) != SDMI_OK) die("Error setting the image prompt");
    }

    // sd.unconditional_context(&tokenizer); sd.context(&tokenizer, prompt)   (main.rs:100-101)
    const int cd = cfg.ctx_dim, cap = cfg.clip_ctx;
    std::vector<float> uncond((size_t)cap * cd), context((size_t)cap * cd);
    int32_t Tu = 0, T = 0;
    const char* style = std::getenv("SDMI_PROMPT_STYLE");
    if (style && std::strcmp(style, "webui") == 0) {
        const char* negative = std::getenv("SDMI_NEGATIVE_PROMPT");
        const char* skip = std::getenv("SDMI_CLIP_SKIP");
        sdmi_prompt_opts opts;
        std::memset(&opts, 0, sizeof opts);
        opts.emphasis = 1;
        opts.clip_skip = skip ? std::atoi(skip) : 1;
        opts.min_chunks = 1;
        if (sdmi_encode_prompt(ctx, tok, prompt.c_str(), &opts, context.data(), cap, &T) != SDMI_OK) {
            if (T <= cap) die("Error encoding the prompt");
            context.resize((size_t)T * cd);   // more than one chunk: *T says how many rows
            if (sdmi_encode_prompt(ctx, tok, prompt.c_str(), &opts, context.data(), T, &T) != SDMI_OK) die("Error encoding the prompt");
        }
        opts.min_chunks = T / cap;
        if (sdmi_encode_prompt(ctx, tok, negative ? negative : "", &opts, uncond.data(), cap, &Tu) != SDMI_OK) {
            if (Tu <= cap) die("Error encoding the negative prompt");
            uncond.resize((size_t)Tu * cd);
            if (sdmi_encode_prompt(ctx, tok, negative ? negative : "", &opts, uncond.data(), Tu, &Tu) != SDMI_OK) die("Error encoding the negative prompt");
        }
    } else if (style && *style) {
        std::fprintf(stderr, "SDMI_PROMPT_STYLE: unknown style %s (webui, or unset for the reference's rule)\n", style);
        return 1;
    } else {
        if (sdmi_context(ctx, tok, "", uncond.data(), cap, &Tu) != SDMI_OK) die("Error encoding the empty prompt");
        if (sdmi_context(ctx, tok, prompt.c_str(), context.data(), cap, &T) != SDMI_OK) die("Error encoding the prompt");
    }

    std::printf("Sampling image...\n");
    const int H = 8 * cfg.latent_h, W = 8 * cfg.latent_w;
    std::vector<uint8_t> rgb((size_t)H * W * 3);
    const char* seed_env = std::getenv("SDMI_SEED");
    const uint64_t seed = seed_env ? std::strtoull(seed_env, nullptr, 10) : 0;
    if (sdmi_sample_image(ctx, context.data(), 1, T, uncond.data(), Tu, scale, (size_t)steps, nullptr, seed, rgb.data()) != SDMI_OK)
        die("Error sampling image");

    // save_images (main.rs:118-125): "{basepath}{index}.png"
    const std::string path = output + "0.png";
    if (sdmi_write_png(path.c_str(), rgb.data(), W, H) != SDMI_OK) die("Error saving image");

    sdmi_destroy(ctx);
    sdmi_tokenizer_destroy(tok);
    return 0;
}
