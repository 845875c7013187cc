// ckpt_keys.cpp -- see ckpt_keys.hpp.  A recursive descent over the '/'-separated dump name; every function consumes the
// components of one module and appends that module's checkpoint path.
#include "ckpt_keys.hpp"

#include <cmath>
#include <map>
#include <vector>

namespace sdmi {

namespace {

enum Leaf { L_PLAIN, L_LINEAR, L_LINEAR_NOBIAS, L_TABLE };   // conv / norm: weight | bias as they are; Linear: weight transposed (the UNet attention's q / k / v: no bias); embedding: weight only

struct Walk {
    std::vector<std::string> t;
    size_t i = 0;
    std::string key;
    bool transposed = false;
    bool more() const { return i < t.size(); }
    const std::string& cur() const { return t[i]; }
    bool take(const char* s) {
        if (!more() || t[i] != s) return false;
        ++i;
        return true;
    }
};

// `s` == prefix + a decimal number in [lo, hi] without leading zeros
bool numbered(const std::string& s, const char* prefix, int lo, int hi, int* n) {
    size_t p = 0;
    while (prefix[p]) {
        if (p >= s.size() || s[p] != prefix[p]) return false;
        ++p;
    }
    if (p == s.size() || s.size() - p > 3 || (s[p] == '0' && s.size() - p > 1)) return false;
    int v = 0;
    for (; p < s.size(); ++p) {
        if (s[p] < '0' || s[p] > '9') return false;
        v = v * 10 + (s[p] - '0');
    }
    if (v < lo || v > hi) return false;
    *n = v;
    return true;
}

bool take_numbered(Walk& w, const char* prefix, int lo, int hi, int* n) {
    if (!w.more() || !numbered(w.cur(), prefix, lo, hi, n)) return false;
    ++w.i;
    return true;
}

// the last component: weight | bias of the module whose path is complete
bool leaf(Walk& w, Leaf kind) {
    if (w.i + 1 != w.t.size()) return false;
    const std::string& l = w.cur();
    if (l == "weight") {
        w.transposed = kind == L_LINEAR || kind == L_LINEAR_NOBIAS;
    } else if (l != "bias" || kind == L_TABLE || kind == L_LINEAR_NOBIAS) {
        return false;
    }
    w.key += "." + l;
    return true;
}

// one module out of a table of {dump directory, checkpoint path, leaf kind}
struct Rename { const char* dump; const char* ckpt; Leaf kind; };
template <size_t N>
bool renamed(Walk& w, const Rename (&table)[N]) {
    for (const Rename& r : table)
        if (w.take(r.dump)) {
            w.key += r.ckpt;
            return leaf(w, r.kind);
        }
    return false;
}

// ResBlock (python/unet.py: save_res_block)
bool res_block(Walk& w) {
    static const Rename k[] = {{"norm_in", ".in_layers.0", L_PLAIN},   {"conv_in", ".in_layers.2", L_PLAIN},   {"lin_embed", ".emb_layers.1", L_LINEAR},
                               {"norm_out", ".out_layers.0", L_PLAIN}, {"conv_out", ".out_layers.3", L_PLAIN}, {"skip_connection", ".skip_connection", L_PLAIN}};
    return renamed(w, k);
}

// CrossAttention (save_cross_attention)
bool cross_attention(Walk& w) {
    static const Rename k[] = {{"query", ".to_q", L_LINEAR_NOBIAS}, {"key", ".to_k", L_LINEAR_NOBIAS}, {"value", ".to_v", L_LINEAR_NOBIAS}, {"out", ".to_out.0", L_LINEAR}};
    return renamed(w, k);
}

// SpatialTransformer and its one BasicTransformerBlock (save_spatial_transformer, save_basic_transformer_block)
bool spatial_transformer(Walk& w) {
    if (w.take("transformer")) {
        w.key += ".transformer_blocks.0";
        if (w.take("attn1")) { w.key += ".attn1"; return cross_attention(w); }
        if (w.take("attn2")) { w.key += ".attn2"; return cross_attention(w); }
        if (w.take("mlp")) {
            if (w.take("geglu")) {
                static const Rename k[] = {{"proj", ".ff.net.0.proj", L_LINEAR}};
                return renamed(w, k);
            }
            static const Rename k[] = {{"lin", ".ff.net.2", L_LINEAR}};
            return renamed(w, k);
        }
        static const Rename k[] = {{"norm1", ".norm1", L_PLAIN}, {"norm2", ".norm2", L_PLAIN}, {"norm3", ".norm3", L_PLAIN}};
        return renamed(w, k);
    }
    static const Rename k[] = {{"norm", ".norm", L_PLAIN}, {"proj_in", ".proj_in", L_PLAIN}, {"proj_out", ".proj_out", L_PLAIN}};
    return renamed(w, k);
}

// [ResBlock, SpatialTransformer?, Upsample?]: "res" is element 0, "transformer" element 1, "upsample/conv" element `up_at`
bool res_group(Walk& w, bool has_transformer, int up_at) {
    if (w.take("res")) { w.key += ".0"; return res_block(w); }
    if (has_transformer && w.take("transformer")) { w.key += ".1"; return spatial_transformer(w); }
    if (up_at && w.take("upsample") && w.take("conv")) { w.key += "." + std::to_string(up_at) + ".conv"; return leaf(w, L_PLAIN); }
    return false;
}

// control = true: a ControlNet in the cldm layout -- the encoder half, the middle block and the time MLP under the UNet's own rules with another
// root, plus the three families the UNet does not have: the hint convolutions (input_hint_block: conv, SiLU, conv, ... -- convolution i is element 2i), the zero
// convolutions (zero_convs.<j> is a one-element sequential) and middle_block_out (likewise).  It has no output blocks and no head.
bool unet(Walk& w, bool control = false) {
    w.key = control ? "control_model" : "model.diffusion_model";
    int n = 0;
    if (control) {
        if (w.take("hint")) {
            if (!take_numbered(w, "c", 0, 7, &n)) return false;
            w.key += ".input_hint_block." + std::to_string(2 * n);
            return leaf(w, L_PLAIN);
        }
        if (w.take("zero_convs")) {
            if (!take_numbered(w, "", 0, 11, &n)) return false;
            w.key += ".zero_convs." + std::to_string(n) + ".0";
            return leaf(w, L_PLAIN);
        }
        if (w.take("middle_block_out")) { w.key += ".middle_block_out.0"; return leaf(w, L_PLAIN); }
    }
    if (w.take("input_blocks")) {   // save_unet_input_blocks: conv rt1 rt2 d1 rt3 rt4 d2 rt5 rt6 d3 r1 r2 = elements 0 .. 11
        w.key += ".input_blocks.";
        if (w.take("conv")) { w.key += "0.0"; return leaf(w, L_PLAIN); }
        if (take_numbered(w, "rt", 1, 6, &n)) { w.key += std::to_string(n + (n - 1) / 2); return res_group(w, true, 0); }
        if (take_numbered(w, "d", 1, 3, &n)) { w.key += std::to_string(3 * n) + ".0.op"; return leaf(w, L_PLAIN); }
        if (take_numbered(w, "r", 1, 2, &n)) { w.key += std::to_string(9 + n) + ".0"; return res_block(w); }
        return false;
    }
    if (w.take("middle_block")) {   // save_res_transformer_res
        w.key += ".middle_block";
        if (w.take("res1")) { w.key += ".0"; return res_block(w); }
        if (w.take("transformer")) { w.key += ".1"; return spatial_transformer(w); }
        if (w.take("res2")) { w.key += ".2"; return res_block(w); }
        return false;
    }
    if (!control && w.take("output_blocks")) {   // save_unet_output_blocks: r1 r2 ru rt1 rt2 rtu1 rt3 rt4 rtu2 rt5 rt6 rt7 = elements 0 .. 11
        w.key += ".output_blocks.";
        if (take_numbered(w, "rtu", 1, 2, &n)) { w.key += std::to_string(2 + 3 * n); return res_group(w, true, 2); }
        if (take_numbered(w, "rt", 1, 7, &n)) { w.key += std::to_string(2 + n + (n >= 3) + (n >= 5)); return res_group(w, true, 0); }
        if (w.take("ru")) { w.key += "2"; return res_group(w, false, 1); }
        if (take_numbered(w, "r", 1, 2, &n)) { w.key += std::to_string(n - 1) + ".0"; return res_block(w); }
        return false;
    }
    if (w.more() && (w.cur() == "lin1_time_embed" || w.cur() == "lin2_time_embed")) {   // the time MLP: a UNet's and a ControlNet's
        static const Rename kt[] = {{"lin1_time_embed", ".time_embed.0", L_LINEAR}, {"lin2_time_embed", ".time_embed.2", L_LINEAR}};
        return renamed(w, kt);
    }
    if (control) return false;   // no head
    static const Rename k[] = {{"norm_out", ".out.0", L_PLAIN}, {"conv_out", ".out.2", L_PLAIN}};
    return renamed(w, k);
}

// ResnetBlock (python/autoencoder.py: save_resnet_block)
bool resnet_block(Walk& w) {
    static const Rename k[] = {{"norm1", ".norm1", L_PLAIN}, {"conv1", ".conv1", L_PLAIN}, {"norm2", ".norm2", L_PLAIN}, {"conv2", ".conv2", L_PLAIN},
                               {"nin_shortcut", ".nin_shortcut", L_PLAIN}};
    return renamed(w, k);
}

bool vae_half(Walk& w, bool decoder) {
    int i = 0, j = 0;
    if (w.take("mid")) {   // save_mid
        w.key += ".mid";
        if (w.take("block_1")) { w.key += ".block_1"; return resnet_block(w); }
        if (w.take("block_2")) { w.key += ".block_2"; return resnet_block(w); }
        if (w.take("attn")) {
            w.key += ".attn_1";
            static const Rename k[] = {{"norm", ".norm", L_PLAIN}, {"q", ".q", L_PLAIN}, {"k", ".k", L_PLAIN}, {"v", ".v", L_PLAIN}, {"proj_out", ".proj_out", L_PLAIN}};
            return renamed(w, k);
        }
        return false;
    }
    if (w.take("blocks")) {
        if (!take_numbered(w, "", 0, 3, &i)) return false;
        // save_decoder walks decoder.up[::-1]: dump block i is up[3 - i]; save_encoder walks encoder.down in order
        w.key += decoder ? ".up." + std::to_string(3 - i) : ".down." + std::to_string(i);
        if (take_numbered(w, "res", 1, decoder ? 3 : 2, &j)) { w.key += ".block." + std::to_string(j - 1); return resnet_block(w); }
        if (decoder && w.take("upsampler")) { w.key += ".upsample.conv"; return leaf(w, L_PLAIN); }
        if (!decoder && w.take("downsampler") && w.take("conv")) { w.key += ".downsample.conv"; return leaf(w, L_PLAIN); }
        return false;
    }
    static const Rename k[] = {{"conv_in", ".conv_in", L_PLAIN}, {"norm_out", ".norm_out", L_PLAIN}, {"conv_out", ".conv_out", L_PLAIN}};
    return renamed(w, k);
}

bool autoencoder(Walk& w) {
    w.key = "first_stage_model";
    if (w.take("encoder")) { w.key += ".encoder"; return vae_half(w, false); }
    if (w.take("decoder")) { w.key += ".decoder"; return vae_half(w, true); }
    static const Rename k[] = {{"quant_conv", ".quant_conv", L_PLAIN}, {"post_quant_conv", ".post_quant_conv", L_PLAIN}};
    return renamed(w, k);
}

// python/clip.py: save_clip_text_transformer
bool clip(Walk& w) {
    w.key = "cond_stage_model.transformer.text_model";
    int i = 0;
    if (w.take("blocks")) {
        if (!take_numbered(w, "", 0, 999, &i)) return false;
        w.key += ".encoder.layers." + std::to_string(i);
        if (w.take("attn")) {
            w.key += ".self_attn";
            static const Rename k[] = {{"query", ".q_proj", L_LINEAR}, {"key", ".k_proj", L_LINEAR}, {"value", ".v_proj", L_LINEAR}, {"out", ".out_proj", L_LINEAR}};
            return renamed(w, k);
        }
        if (w.take("mlp")) {
            w.key += ".mlp";
            static const Rename k[] = {{"fc1", ".fc1", L_LINEAR}, {"fc2", ".fc2", L_LINEAR}};
            return renamed(w, k);
        }
        static const Rename k[] = {{"attn_ln", ".layer_norm1", L_PLAIN}, {"mlp_ln", ".layer_norm2", L_PLAIN}};
        return renamed(w, k);
    }
    static const Rename k[] = {{"token_embedding", ".embeddings.token_embedding", L_TABLE}, {"position_embedding", ".embeddings.position_embedding", L_TABLE},
                               {"layer_norm", ".final_layer_norm", L_PLAIN}};
    return renamed(w, k);
}

// SD 2.x: the OpenCLIP text tower as Stability's checkpoints name it (open_clip's TextTransformer under FrozenOpenCLIPEmbedder.model)
bool open_clip(Walk& w, int* slice) {
    w.key = "cond_stage_model.model";
    int i = 0;
    if (w.take("blocks")) {
        if (!take_numbered(w, "", 0, 999, &i)) return false;
        w.key += ".transformer.resblocks." + std::to_string(i);
        if (w.take("attn")) {
            w.key += ".attn";
            static const char* const part[3] = {"query", "key", "value"};
            for (int p = 0; p < 3; ++p)
                if (w.take(part[p])) {   // nn.MultiheadAttention's fused projection: rows [p C, (p + 1) C) of in_proj_weight / in_proj_bias
                    if (w.i + 1 != w.t.size() || (w.cur() != "weight" && w.cur() != "bias")) return false;
                    w.transposed = w.cur() == "weight";
                    w.key += w.cur() == "weight" ? ".in_proj_weight" : ".in_proj_bias";
                    *slice = p;
                    return true;
                }
            static const Rename k[] = {{"out", ".out_proj", L_LINEAR}};
            return renamed(w, k);
        }
        if (w.take("mlp")) {
            w.key += ".mlp";
            static const Rename k[] = {{"fc1", ".c_fc", L_LINEAR}, {"fc2", ".c_proj", L_LINEAR}};
            return renamed(w, k);
        }
        static const Rename k[] = {{"attn_ln", ".ln_1", L_PLAIN}, {"mlp_ln", ".ln_2", L_PLAIN}};
        return renamed(w, k);
    }
    if (w.take("position_embedding")) {   // a bare nn.Parameter: no ".weight"
        if (w.i + 1 != w.t.size() || w.cur() != "weight") return false;
        w.key += ".positional_embedding";
        return true;
    }
    static const Rename k[] = {{"token_embedding", ".token_embedding", L_TABLE}, {"layer_norm", ".ln_final", L_PLAIN}};
    return renamed(w, k);
}

}  // namespace

const char* const kFamilyKeySd1 = "cond_stage_model.transformer.text_model.final_layer_norm.weight";
const char* const kFamilyKeySd2 = "cond_stage_model.model.ln_final.weight";

bool checkpoint_key(const std::string& dump_name, std::string* key, bool* transposed) { return checkpoint_key(dump_name, 0, key, transposed, nullptr); }

bool checkpoint_key(const std::string& dump_name, int variant, std::string* key, bool* transposed, int* slice) {
    int sl = -1;
    Walk w;
    size_t start = 0;
    for (;;) {
        const size_t slash = dump_name.find('/', start);
        w.t.push_back(dump_name.substr(start, slash == std::string::npos ? std::string::npos : slash - start));
        if (w.t.back().empty()) return false;
        if (slash == std::string::npos) break;
        start = slash + 1;
    }
    bool ok = false;
    if (w.t.size() == 1 && w.t[0] == "alphas_cumprod") { w.key = "alphas_cumprod"; ok = true; }
    else if (w.take("unet")) ok = unet(w);
    else if (w.take("controlnet")) ok = unet(w, true);
    else if (w.take("autoencoder")) ok = autoencoder(w);
    else if (w.take("clip")) ok = variant == 1 ? open_clip(w, &sl) : clip(w);
    if (!ok) return false;
    if (key) *key = w.key;
    if (transposed) *transposed = w.transposed;
    if (slice) *slice = sl;
    return true;
}

namespace {

// checkpoint key -> dump name for every name the rules accept (CLIP: layer 0 stands for all layers).  The candidates are generated generously -- every
// module directory under every block name, with both leaves -- and checkpoint_key decides which of them exist.
const std::map<std::string, std::string>& reverse_map() {
    static const std::map<std::string, std::string> m = [] {
        std::map<std::string, std::string> r;
        auto both = [&](const std::string& mod) {
            for (const char* leaf_name : {"/weight", "/bias"}) {
                std::string key;
                bool tr;
                if (checkpoint_key(mod + leaf_name, &key, &tr)) r.emplace(key, mod + leaf_name);
            }
        };
        auto res = [&](const std::string& p) { for (const char* d : {"norm_in", "conv_in", "lin_embed", "norm_out", "conv_out", "skip_connection"}) both(p + "/" + d); };
        auto st = [&](const std::string& p) {
            for (const char* d : {"norm", "proj_in", "proj_out", "transformer/norm1", "transformer/norm2", "transformer/norm3", "transformer/mlp/geglu/proj", "transformer/mlp/lin"}) both(p + "/" + d);
            for (const char* a : {"attn1", "attn2"})
                for (const char* d : {"query", "key", "value", "out"}) both(p + "/transformer/" + a + "/" + d);
        };
        auto resnet = [&](const std::string& p) { for (const char* d : {"norm1", "conv1", "norm2", "conv2", "nin_shortcut"}) both(p + "/" + d); };
        std::string key;
        bool tr;
        if (checkpoint_key("alphas_cumprod", &key, &tr)) r.emplace(key, "alphas_cumprod");
        for (const char* d : {"lin1_time_embed", "lin2_time_embed", "norm_out", "conv_out", "input_blocks/conv"}) both(std::string("unet/") + d);
        for (const char* side : {"unet/input_blocks/", "unet/output_blocks/"})
            for (int i = 0; i <= 9; ++i) {
                const std::string n = std::to_string(i);
                for (const char* kind : {"rt", "rtu", "ru", "r", "d"}) {
                    const std::string b = std::string(side) + kind + (std::string(kind) == "ru" ? "" : n);
                    res(b); res(b + "/res"); st(b + "/transformer"); both(b + "/upsample/conv"); both(b);
                }
            }
        res("unet/middle_block/res1"); st("unet/middle_block/transformer"); res("unet/middle_block/res2");
        // a ControlNet (cldm layout): the encoder's names under another root + its three own families
        for (const char* d : {"lin1_time_embed", "lin2_time_embed", "input_blocks/conv", "middle_block_out"}) both(std::string("controlnet/") + d);
        for (int i = 0; i <= 9; ++i) {
            const std::string n = std::to_string(i);
            for (const char* kind : {"rt", "r", "d"}) {
                const std::string b = std::string("controlnet/input_blocks/") + kind + n;
                res(b); res(b + "/res"); st(b + "/transformer"); both(b);
            }
        }
        for (int i = 0; i <= 7; ++i) both("controlnet/hint/c" + std::to_string(i));
        for (int i = 0; i <= 11; ++i) both("controlnet/zero_convs/" + std::to_string(i));
        res("controlnet/middle_block/res1"); st("controlnet/middle_block/transformer"); res("controlnet/middle_block/res2");
        both("autoencoder/quant_conv"); both("autoencoder/post_quant_conv");
        for (const char* half : {"autoencoder/encoder", "autoencoder/decoder"}) {
            const std::string h = half;
            for (const char* d : {"conv_in", "norm_out", "conv_out", "mid/attn/norm", "mid/attn/q", "mid/attn/k", "mid/attn/v", "mid/attn/proj_out"}) both(h + "/" + d);
            resnet(h + "/mid/block_1"); resnet(h + "/mid/block_2");
            for (int i = 0; i <= 9; ++i) {
                const std::string b = h + "/blocks/" + std::to_string(i);
                for (int j = 0; j <= 9; ++j) resnet(b + "/res" + std::to_string(j));
                both(b + "/upsampler"); both(b + "/downsampler/conv");
            }
        }
        for (const char* d : {"token_embedding", "position_embedding", "layer_norm"}) both(std::string("clip/") + d);
        for (const char* d : {"attn/query", "attn/key", "attn/value", "attn/out", "attn_ln", "mlp/fc1", "mlp/fc2", "mlp_ln"}) both(std::string("clip/blocks/0/") + d);
        return r;
    }();
    return m;
}

}  // namespace

bool dump_name_of_checkpoint_key(const std::string& key, std::string* dump_name) {
    const auto& m = reverse_map();
    auto it = m.find(key);
    std::string name;
    if (it != m.end()) {
        name = it->second;
    } else {
        // a CLIP layer other than 0: look layer 0's name up, put the index back
        static const std::string prefix = "cond_stage_model.transformer.text_model.encoder.layers.";
        if (key.compare(0, prefix.size(), prefix) != 0) return false;
        const size_t dot = key.find('.', prefix.size());
        if (dot == std::string::npos) return false;
        const std::string index = key.substr(prefix.size(), dot - prefix.size());
        it = m.find(prefix + "0" + key.substr(dot));
        if (it == m.end()) return false;
        name = "clip/blocks/" + index + it->second.substr(std::string("clip/blocks/0").size());
    }
    std::string back;   // whatever the route, the answer is only given when the rules map it back to the key
    bool tr;
    if (!checkpoint_key(name, &back, &tr) || back != key) return false;
    if (dump_name) *dump_name = name;
    return true;
}

void default_alphas_cumprod(float* out, int n) {
    const double start = std::sqrt(0.00085), stop = std::sqrt(0.012);
    const double step = n > 1 ? (stop - start) / (double)(n - 1) : 0.0;
    double prod = 1.0;
    for (int i = 0; i < n; ++i) {
        // numpy.linspace: arange(n) * step + start, the last point set to `stop`; the product is rounded before the sum (no fused multiply-add)
        volatile double scaled = (double)i * step;
        const double root = (i == n - 1 && n > 1) ? stop : scaled + start;
        volatile double beta = root * root;
        prod *= 1.0 - beta;
        out[i] = (float)prod;
    }
}

}  // namespace sdmi
