// lora_keys.cpp -- see lora_keys.hpp.  The renaming works on the '.'-separated CompVis key of an entry (ckpt_keys.cpp makes it from the dump name); the file plan
// works on the header of a mapped .safetensors file and touches tensor data only to read a module's alpha.
#include "lora_keys.hpp"

#include <cmath>
#include <cstring>

#include "ckpt_keys.hpp"
#include "error.hpp"

namespace sdmi {

namespace {

std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> t;
    size_t start = 0;
    for (;;) {
        const size_t p = s.find(sep, start);
        t.push_back(s.substr(start, p == std::string::npos ? std::string::npos : p - start));
        if (p == std::string::npos) break;
        start = p + 1;
    }
    return t;
}

std::string join(const std::vector<std::string>& t, size_t from) {
    std::string s;
    for (size_t i = from; i < t.size(); ++i) s += (i > from ? "." : "") + t[i];
    return s;
}

// a decimal number without leading zeros, at most three digits
bool index_of(const std::string& s, int* v) {
    if (s.empty() || s.size() > 3 || (s[0] == '0' && s.size() > 1)) return false;
    int n = 0;
    for (char ch : s) {
        if (ch < '0' || ch > '9') return false;
        n = n * 10 + (ch - '0');
    }
    *v = n;
    return true;
}

bool starts_with(const std::string& s, const char* prefix) { return s.compare(0, std::strlen(prefix), prefix) == 0; }

std::string underscored(std::string s) {
    for (char& ch : s)
        if (ch == '.') ch = '_';
    return s;
}

// the conv / Linear modules inside a ResBlock
bool res_module(const std::string& compvis, std::string* diffusers) {
    static const char* const k[][2] = {{"in_layers.2", "conv1"}, {"emb_layers.1", "time_emb_proj"}, {"out_layers.3", "conv2"}, {"skip_connection", "conv_shortcut"}};
    for (const auto& r : k)
        if (compvis == r[0]) { *diffusers = r[1]; return true; }
    return false;
}

// the conv / Linear modules inside a SpatialTransformer: the same names on both sides
bool transformer_module(const std::string& m) {
    static const char* const k[] = {"proj_in", "proj_out", "transformer_blocks.0.ff.net.0.proj", "transformer_blocks.0.ff.net.2"};
    for (const char* s : k)
        if (m == s) return true;
    for (const char* a : {"attn1", "attn2"})
        for (const char* p : {"to_q", "to_k", "to_v", "to_out.0"})
            if (m == std::string("transformer_blocks.0.") + a + "." + p) return true;
    return false;
}

// CompVis module path of the UNet ("input_blocks.1.1.proj_in") -> diffusers module path ("down_blocks.0.attentions.0.proj_in"): SD v1, 4 levels, 2 ResBlocks per level
bool unet_diffusers_path(const std::string& compvis, std::string* out) {
    const std::vector<std::string> t = split(compvis, '.');
    int n = 0, m = 0;
    std::string sub;
    if (t[0] == "time_embed" && t.size() == 2) {
        if (t[1] == "0") { *out = "time_embedding.linear_1"; return true; }
        if (t[1] == "2") { *out = "time_embedding.linear_2"; return true; }
        return false;
    }
    if (t[0] == "out" && t.size() == 2 && t[1] == "2") { *out = "conv_out"; return true; }
    if (t[0] == "middle_block" && t.size() >= 3 && index_of(t[1], &m)) {
        const std::string rest = join(t, 2);
        if (m == 1 && transformer_module(rest)) { *out = "mid_block.attentions.0." + rest; return true; }
        if ((m == 0 || m == 2) && res_module(rest, &sub)) { *out = std::string("mid_block.resnets.") + (m == 0 ? "0." : "1.") + sub; return true; }
        return false;
    }
    if (t[0] == "input_blocks" && t.size() >= 3 && index_of(t[1], &n) && index_of(t[2], &m) && n <= 11) {
        const std::string rest = join(t, 3);
        if (n == 0) {
            if (m == 0 && rest.empty()) { *out = "conv_in"; return true; }
            return false;
        }
        const int i = (n - 1) / 3, j = (n - 1) % 3;
        const std::string level = "down_blocks." + std::to_string(i);
        if (j == 2) {
            if (m == 0 && rest == "op") { *out = level + ".downsamplers.0.conv"; return true; }
            return false;
        }
        if (m == 0 && res_module(rest, &sub)) { *out = level + ".resnets." + std::to_string(j) + "." + sub; return true; }
        if (m == 1 && i < 3 && transformer_module(rest)) { *out = level + ".attentions." + std::to_string(j) + "." + rest; return true; }
        return false;
    }
    if (t[0] == "output_blocks" && t.size() >= 4 && index_of(t[1], &n) && index_of(t[2], &m) && n <= 11) {
        const std::string rest = join(t, 3);
        const int i = n / 3, j = n % 3;
        const std::string level = "up_blocks." + std::to_string(i);
        if (m == 0 && res_module(rest, &sub)) { *out = level + ".resnets." + std::to_string(j) + "." + sub; return true; }
        if (rest == "conv") {
            if (j == 2 && i < 3 && m == (i == 0 ? 1 : 2)) { *out = level + ".upsamplers.0.conv"; return true; }
            return false;
        }
        if (m == 1 && i > 0 && transformer_module(rest)) { *out = level + ".attentions." + std::to_string(j) + "." + rest; return true; }
        return false;
    }
    return false;
}

// "text_model.encoder.layers.<n>.self_attn.q_proj" ...: the Linear layers of the text encoder (the same path on both sides)
bool te_module(const std::string& path) {
    const std::vector<std::string> t = split(path, '.');
    int n = 0;
    if (t.size() != 6 || t[0] != "text_model" || t[1] != "encoder" || t[2] != "layers" || !index_of(t[3], &n)) return false;
    if (t[4] == "self_attn") return t[5] == "q_proj" || t[5] == "k_proj" || t[5] == "v_proj" || t[5] == "out_proj";
    if (t[4] == "mlp") return t[5] == "fc1" || t[5] == "fc2";
    return false;
}

const char kUnetRoot[] = "model.diffusion_model.", kTeRoot[] = "cond_stage_model.transformer.", kWeight[] = ".weight";

}  // namespace

bool lora_module_name(const std::string& dump_name, std::string* kohya, std::string* compvis) {
    std::string key;
    bool transposed = false;
    if (!checkpoint_key(dump_name, &key, &transposed)) return false;
    const size_t nw = sizeof(kWeight) - 1;
    if (key.size() <= nw || key.compare(key.size() - nw, nw, kWeight) != 0) return false;
    key.resize(key.size() - nw);
    if (starts_with(key, kUnetRoot)) {
        const std::string path = key.substr(sizeof(kUnetRoot) - 1);
        std::string diffusers;
        if (path.empty() || !unet_diffusers_path(path, &diffusers)) return false;
        if (kohya) *kohya = "lora_unet_" + underscored(diffusers);
        if (compvis) *compvis = "lora_unet_" + underscored(path);
        return true;
    }
    if (starts_with(key, kTeRoot)) {
        const std::string path = key.substr(sizeof(kTeRoot) - 1);
        if (!te_module(path)) return false;
        if (kohya) *kohya = "lora_te_" + underscored(path);
        if (compvis) *compvis = "lora_te_" + underscored(path);
        return true;
    }
    return false;
}

LoraKeyTable::LoraKeyTable(const std::vector<LoraEntryDesc>& entries) : n_entries_(entries.size()) {
    for (size_t i = 0; i < entries.size(); ++i) {
        if (entries[i].kind != 0 && entries[i].kind != 1) continue;
        std::string kohya, compvis;
        if (!lora_module_name(entries[i].name, &kohya, &compvis)) continue;
        index_.emplace(kohya, (int)i);
        index_.emplace(compvis, (int)i);
    }
}

int LoraKeyTable::find(const std::string& module) const {
    auto it = index_.find(module);
    return it == index_.end() ? -1 : it->second;
}

namespace {

int factor_dtype(const std::string& d) { return d == "F32" ? 0 : d == "F16" ? 1 : d == "BF16" ? 2 : -1; }

// a module's alpha: one element of any float dtype, widened exactly
bool scalar_value(const StTensor& t, double* v) {
    if (t.count != 1 || !t.data) return false;
    if (t.dtype == "F64") { std::memcpy(v, t.data, 8); return true; }
    if (t.dtype == "F32") { float f; std::memcpy(&f, t.data, 4); *v = f; return true; }
    uint16_t h;
    if (t.dtype == "BF16") {
        std::memcpy(&h, t.data, 2);
        const uint32_t bits = (uint32_t)h << 16;
        float f;
        std::memcpy(&f, &bits, 4);
        *v = f;
        return true;
    }
    if (t.dtype == "F16") {
        std::memcpy(&h, t.data, 2);
        const int ex = (h >> 10) & 31, man = h & 0x3ff;
        double m;
        if (ex == 0) m = std::ldexp((double)man, -24);
        else if (ex == 31) m = man ? NAN : INFINITY;
        else m = std::ldexp((double)(man | 0x400), ex - 25);
        *v = (h & 0x8000) ? -m : m;
        return true;
    }
    return false;
}

std::string shape_text(const std::vector<int64_t>& s) {
    std::string r = "[";
    for (size_t i = 0; i < s.size(); ++i) r += (i ? "," : "") + std::to_string(s[i]);
    return r + "]";
}

enum Suffix { S_DOWN, S_UP, S_ALPHA, S_W1A, S_W1B, S_W2A, S_W2B, S_COUNT };
const char* const kSuffix[S_COUNT] = {"lora_down.weight", "lora_up.weight", "alpha", "hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b"};

struct Module {
    std::string name;
    const StTensor* part[S_COUNT] = {};
};

// a "down" factor: [r, n_in], or the 4-D spelling [r, cin, kh, kw] (a Linear counts as cin = in, k = 1)
bool down_shape_ok(const StTensor& t, const LoraEntryDesc& e, int64_t n_in, int64_t* rank) {
    const auto& s = t.shape;
    if (s.size() == 2) { *rank = s[0]; return s[1] == n_in; }
    if (s.size() != 4) return false;
    *rank = s[0];
    if (e.kind == 0) return s[1] == e.dims[1] && s[2] == e.dims[2] && s[3] == e.dims[3];
    return s[1] == n_in && s[2] == 1 && s[3] == 1;
}

// an "up" factor: [n_out, r] or [n_out, r, 1, 1]
bool up_shape_ok(const StTensor& t, int64_t n_out, int64_t rank) {
    const auto& s = t.shape;
    if (s.size() != 2 && s.size() != 4) return false;
    if (s.size() == 4 && (s[2] != 1 || s[3] != 1)) return false;
    return s[0] == n_out && s[1] == rank;
}

}  // namespace

LoraFilePlan lora_plan_file(const std::vector<StTensor>& tensors, const std::vector<LoraEntryDesc>& entries, int which, int flags) {
    const char* fn = "lora_load_safetensors: ";
    if (!(which & (kLoraUnet | kLoraTe)) || (which & ~(kLoraUnet | kLoraTe)))
        throw Error(SDMI_ERR_INVALID, std::string(fn) + "which must be SDMI_LORA_UNET, SDMI_LORA_TE or both");
    if (flags & ~kLoraSkipUnknown) throw Error(SDMI_ERR_INVALID, std::string(fn) + "unknown flag");

    // 1. every key is "<module>.<kind>": group by module in header order; a kind that is not built refuses the file, whichever half it is in
    std::vector<Module> modules;
    std::map<std::string, size_t> by_name;
    for (const StTensor& t : tensors) {
        const size_t dot = t.key.find('.');
        const std::string module = t.key.substr(0, dot), kind = dot == std::string::npos ? std::string() : t.key.substr(dot + 1);
        int s = -1;
        for (int i = 0; i < S_COUNT; ++i)
            if (kind == kSuffix[i]) s = i;
        if (s < 0) {
            const char* what = "is no key of a LoRA / LoCon / LoHa module";
            if (kind == "lora_mid.weight" || kind == "hada_t1" || kind == "hada_t2") what = "is a Tucker core: Tucker-decomposed convolutions are not supported";
            else if (starts_with(kind, "lokr_")) what = "is a LoKr factor: LoKr is not supported";
            else if (kind == "dora_scale") what = "is a DoRA magnitude: DoRA is not supported";
            else if (kind == "diff" || kind == "diff_b") what = "is a full-rank difference: not supported";
            throw Error(SDMI_ERR_UNSUPPORTED, std::string(fn) + "'" + t.key + "' " + what);
        }
        auto it = by_name.find(module);
        if (it == by_name.end()) {
            it = by_name.emplace(module, modules.size()).first;
            modules.emplace_back();
            modules.back().name = module;
        }
        modules[it->second].part[s] = &t;
    }

    // 2. module -> entry, then every check the entry's dims allow
    const LoraKeyTable table(entries);
    LoraFilePlan plan;
    std::map<int, std::string> taken;
    for (const Module& m : modules) {
        const bool is_unet = starts_with(m.name, "lora_unet_"), is_te = starts_with(m.name, "lora_te_");
        if ((is_unet && !(which & kLoraUnet)) || (is_te && !(which & kLoraTe))) continue;
        const StTensor* first = nullptr;
        for (const StTensor* p : m.part)
            if (p && (!first || p->file_offset < first->file_offset)) first = p;
        const int ei = table.find(m.name);
        if (ei < 0) {
            if (flags & kLoraSkipUnknown) { plan.skipped.push_back(m.name); continue; }
            throw Error(SDMI_ERR_UNSUPPORTED, std::string(fn) + "'" + first->key + "': no conv / Linear weight of this model is named '" + m.name +
                                                  "' (SDMI_LORA_SKIP_UNKNOWN passes such modules over)");
        }
        const LoraEntryDesc& e = entries[ei];
        const bool lora = m.part[S_DOWN] || m.part[S_UP], hada = m.part[S_W1A] || m.part[S_W1B] || m.part[S_W2A] || m.part[S_W2B];
        LoraFileTarget tg{};
        tg.entry = ei;
        tg.module = m.name;
        if (lora && hada) throw Error(SDMI_ERR_WEIGHTS, std::string(fn) + "module '" + m.name + "' has both LoRA and LoHa factors");
        if (lora) {
            tg.kind = 0;
            tg.f[0] = m.part[S_DOWN]; tg.f[1] = m.part[S_UP];
            if (!tg.f[0] || !tg.f[1])
                throw Error(SDMI_ERR_WEIGHTS, std::string(fn) + "module '" + m.name + "' has no '" + m.name + "." + kSuffix[tg.f[0] ? S_UP : S_DOWN] + "'");
        } else if (hada) {
            tg.kind = 1;
            const int order[4] = {S_W1B, S_W1A, S_W2B, S_W2A};
            for (int i = 0; i < 4; ++i) {
                tg.f[i] = m.part[order[i]];
                if (!tg.f[i]) throw Error(SDMI_ERR_WEIGHTS, std::string(fn) + "module '" + m.name + "' has no '" + m.name + "." + kSuffix[order[i]] + "'");
            }
        } else {
            throw Error(SDMI_ERR_WEIGHTS, std::string(fn) + "module '" + m.name + "' has no factors ('" + first->key + "' alone)");
        }
        const int nf = tg.kind == 1 ? 4 : 2;
        tg.dtype = factor_dtype(tg.f[0]->dtype);
        for (int i = 0; i < nf; ++i) {
            const int dt = factor_dtype(tg.f[i]->dtype);
            if (dt < 0) throw Error(SDMI_ERR_UNSUPPORTED, std::string(fn) + "'" + tg.f[i]->key + "' has dtype " + tg.f[i]->dtype + "; F32, F16 and BF16 are supported");
            if (dt != tg.dtype) throw Error(SDMI_ERR_UNSUPPORTED, std::string(fn) + "'" + tg.f[i]->key + "' has dtype " + tg.f[i]->dtype + ", the module's other factors " + tg.f[0]->dtype);
        }
        if (e.padded)
            throw Error(SDMI_ERR_UNSUPPORTED, std::string(fn) + "'" + first->key + "': '" + e.name + "' is the " + std::to_string(e.dims[1]) + "-channel conv_in, packed in a padded form");
        const int64_t n_in = e.kind == 0 ? e.dims[1] * e.dims[2] * e.dims[3] : e.dims[0], n_out = e.kind == 0 ? e.dims[0] : e.dims[1];
        int64_t rank = 0;
        for (int i = 0; i < nf; i += 2) {
            int64_t r = 0;
            if (!down_shape_ok(*tg.f[i], e, n_in, &r) || r < 1 || (i && r != rank))
                throw Error(SDMI_ERR_WEIGHTS, std::string(fn) + "'" + tg.f[i]->key + "' has shape " + shape_text(tg.f[i]->shape) + "; '" + e.name + "' takes [r, " +
                                                  std::to_string(n_in) + "]" + (e.kind == 0 ? " or [r, cin, k, k]" : "") + (i ? " with the rank of the first pair" : ""));
            rank = r;
            if (!up_shape_ok(*tg.f[i + 1], n_out, rank))
                throw Error(SDMI_ERR_WEIGHTS, std::string(fn) + "'" + tg.f[i + 1]->key + "' has shape " + shape_text(tg.f[i + 1]->shape) + "; '" + e.name + "' at rank " +
                                                  std::to_string(rank) + " takes [" + std::to_string(n_out) + ", " + std::to_string(rank) + "]");
        }
        if (rank > 256) throw Error(SDMI_ERR_UNSUPPORTED, std::string(fn) + "'" + tg.f[0]->key + "' has rank " + std::to_string(rank) + "; ranks 1 .. 256 are supported");
        tg.rank = (int)rank;
        tg.alpha = (double)rank;
        if (const StTensor* a = m.part[S_ALPHA]) {
            if (!scalar_value(*a, &tg.alpha) || !std::isfinite(tg.alpha))
                throw Error(SDMI_ERR_WEIGHTS, std::string(fn) + "'" + a->key + "' must be one finite number (F32, F16, BF16 or F64); it is " + a->dtype + " " + shape_text(a->shape));
        }
        auto dup = taken.emplace(ei, m.name);
        if (!dup.second)
            throw Error(SDMI_ERR_WEIGHTS, std::string(fn) + "modules '" + dup.first->second + "' and '" + m.name + "' both name '" + e.name + "'");
        plan.targets.push_back(tg);
    }
    return plan;
}

}  // namespace sdmi
