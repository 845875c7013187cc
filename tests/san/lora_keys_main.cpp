// lora_keys_main.cpp -- sanitizer driver of the kohya-ss LoRA name map and file plan (csrc/lora_keys.cpp, host only).  Built by tests/test_lora_file_cpu.py with plain
// g++ (-fsanitize=address,undefined) together with lora_keys.cpp, ckpt_keys.cpp and safetensors_reader.cpp.
//
//   lora_keys_main <table>
//
// <table> is tests/golden/kohya_lora_keys.txt: "dump name<TAB>kohya module<TAB>CompVis-style module" per line.  Every line goes through lora_module_name and, in both
// spellings, through a LoraKeyTable made from all lines; then malformed module names (every prefix and suffix of every name, byte substitutions, long and empty
// strings) and malformed dump names go through the same entry points, and fabricated tensor lists -- well-formed LoRA / LoHa modules, every refused key kind, wrong
// shapes, keys without a module -- through lora_plan_file with the status of each checked.  Exit 0 when everything is as expected.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../stable_diffusion_burn_amd/csrc/error.hpp"
#include "../../stable_diffusion_burn_amd/csrc/lora_keys.hpp"

using namespace sdmi;

static int g_bad = 0;
static void expect(bool ok, const std::string& what) {
    if (!ok && ++g_bad <= 10) std::fprintf(stderr, "FAILED: %s\n", what.c_str());
}

static std::vector<unsigned char> g_bytes(64, 0);   // data of every fabricated tensor: zeros (alpha = 0.0 in any dtype)

static StTensor tensor(const std::string& key, const std::string& dtype, std::vector<int64_t> shape) {
    StTensor t;
    t.key = key; t.dtype = dtype; t.shape = shape;
    t.count = 1;
    for (int64_t d : shape) t.count *= (size_t)d;
    t.nbytes = t.count * safetensors_dtype_size(dtype);
    t.data = g_bytes.data();   // only an alpha's single element is ever read
    t.file_offset = 0;
    return t;
}

// the status lora_plan_file ends with (0: accepted) and, when accepted, the number of targets / skips
static int plan_status(const std::vector<StTensor>& ts, const std::vector<LoraEntryDesc>& entries, int which, int flags, size_t* n_targets = nullptr, size_t* n_skipped = nullptr,
                       std::string* message = nullptr) {
    try {
        const LoraFilePlan p = lora_plan_file(ts, entries, which, flags);
        if (n_targets) *n_targets = p.targets.size();
        if (n_skipped) *n_skipped = p.skipped.size();
        return 0;
    } catch (const Error& e) {
        if (message) *message = e.what();
        return e.status;
    }
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: lora_keys_main <table>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<LoraEntryDesc> entries;
    std::vector<std::string> kohya, compvis;
    std::string line;
    while (std::getline(in, line)) {
        const size_t a = line.find('\t'), b = line.find('\t', a + 1);
        if (a == std::string::npos || b == std::string::npos) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        LoraEntryDesc e{};
        e.name = line.substr(0, a);
        e.kind = 1;
        e.dims[0] = 8; e.dims[1] = 12; e.dims[2] = e.dims[3] = 1;   // every entry a Linear [8, 12]: the map does not look at dims
        entries.push_back(e);
        kohya.push_back(line.substr(a + 1, b - a - 1));
        compvis.push_back(line.substr(b + 1));
    }
    long checks = 0;

    // 1. the table, forwards and backwards
    const LoraKeyTable table(entries);
    for (size_t i = 0; i < entries.size(); ++i) {
        std::string k, c;
        expect(lora_module_name(entries[i].name, &k, &c) && k == kohya[i] && c == compvis[i], "lora_module_name(" + entries[i].name + ")");
        expect(table.find(kohya[i]) == (int)i && table.find(compvis[i]) == (int)i, "table.find of " + kohya[i]);
        checks += 3;
    }

    // 2. malformed module names: nothing but a complete name of the table resolves
    for (size_t i = 0; i < kohya.size(); ++i) {
        const std::string& m = kohya[i];
        for (size_t n = 0; n < m.size(); ++n) {
            const std::string pre = m.substr(0, n), suf = m.substr(n + 1);
            const int a = table.find(pre), b = table.find(suf);
            expect(a < 0 || kohya[a] == pre || compvis[a] == pre, "prefix " + pre);
            expect(b < 0 || kohya[b] == suf || compvis[b] == suf, "suffix " + suf);
            checks += 2;
        }
        for (size_t n = 0; n < m.size(); n += 7) {
            std::string x = m;
            x[n] = x[n] == '_' ? '.' : '_';
            const int a = table.find(x);
            expect(a < 0 || kohya[a] == x || compvis[a] == x, "substitution " + x);
            x[n] = (char)0xff;
            expect(table.find(x) < 0, "byte 0xff in a name");
            checks += 2;
        }
    }
    for (const std::string& m : {std::string(), std::string("lora_unet_"), std::string("lora_te_"), std::string(1 << 16, '_'), std::string("lora_unet_") + std::string(4096, '9'),
                                 std::string("lora_te1_text_model_encoder_layers_0_mlp_fc1"), std::string("lora_unet_down_blocks_0_attentions_0_transformer_blocks_1_attn1_to_q"),
                                 std::string("lora_unet_input_blocks_12_1_proj_in"), std::string("lora_unet_down_blocks_4_resnets_0_conv1")}) {
        expect(table.find(m) < 0, "a name of no entry resolves: " + m.substr(0, 60));
        ++checks;
    }
    // ... and malformed dump names: never a module name, never a crash
    for (const std::string& d : {std::string(), std::string("/"), std::string("unet"), std::string("unet/"), std::string("unet//weight"), std::string("unet/input_blocks/rt1/res/conv_in/bias"),
                                 std::string("unet/input_blocks/rt1/res/norm_in/weight"), std::string("unet/input_blocks/rt9/res/conv_in/weight"), std::string("clip/token_embedding/weight"),
                                 std::string("clip/blocks/1000/mlp/fc1/weight"), std::string("clip/blocks/-1/mlp/fc1/weight"), std::string("autoencoder/decoder/conv_in/weight"),
                                 std::string("controlnet/input_blocks/rt1/res/conv_in/weight"), std::string(1 << 16, '/'), std::string("unet/") + std::string(1 << 16, 'x') + "/weight"}) {
        std::string k;
        expect(!lora_module_name(d, &k, nullptr), "a module name for dump name " + d.substr(0, 60));
        ++checks;
    }
    for (size_t i = 0; i < entries.size(); i += 5)
        for (size_t n = 0; n < entries[i].name.size(); ++n) {
            std::string k;
            expect(!lora_module_name(entries[i].name.substr(0, n), &k, nullptr), "a module name for a truncated dump name");
            ++checks;
        }

    // 3. the file plan on fabricated tensor lists
    const std::string q = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q", fc = "lora_te_text_model_encoder_layers_0_mlp_fc1";
    const int both = kLoraUnet | kLoraTe;
    size_t nt = 0, ns = 0;
    std::vector<StTensor> ok = {tensor(q + ".lora_down.weight", "F16", {4, 8}), tensor(q + ".lora_up.weight", "F16", {12, 4}), tensor(q + ".alpha", "F16", {}),
                                tensor(fc + ".hada_w1_a", "BF16", {12, 3}), tensor(fc + ".hada_w1_b", "BF16", {3, 8}), tensor(fc + ".hada_w2_a", "BF16", {12, 3}),
                                tensor(fc + ".hada_w2_b", "BF16", {3, 8}), tensor(fc + ".alpha", "F64", {1})};
    expect(plan_status(ok, entries, both, 0, &nt, &ns) == 0 && nt == 2 && ns == 0, "a well-formed LoRA + LoHa list");
    expect(plan_status(ok, entries, kLoraUnet, 0, &nt, &ns) == 0 && nt == 1, "which = unet");
    expect(plan_status(ok, entries, kLoraTe, 0, &nt, &ns) == 0 && nt == 1, "which = te");
    expect(plan_status(ok, entries, 0, 0) == SDMI_ERR_INVALID && plan_status(ok, entries, 4, 0) == SDMI_ERR_INVALID && plan_status(ok, entries, both, 2) == SDMI_ERR_INVALID, "which / flags");
    checks += 4;
    for (const char* kind : {"lora_mid.weight", "hada_t1", "hada_t2", "lokr_w1", "lokr_w2_a", "lokr_t2", "dora_scale", "diff", "diff_b", "lora_A.weight", "", "weight", "lora_down"}) {
        std::vector<StTensor> ts = ok;
        ts.push_back(tensor(q + (*kind ? "." : "") + kind, "F16", {4, 4}));
        std::string msg;
        expect(plan_status(ts, entries, both, kLoraSkipUnknown, nullptr, nullptr, &msg) == SDMI_ERR_UNSUPPORTED && msg.find(ts.back().key) != std::string::npos, std::string("refused key kind ") + kind);
        ++checks;
    }
    struct Case { const char* what; std::vector<StTensor> ts; int flags; int status; };
    const std::vector<Case> cases = {
        {"down of another width", {tensor(q + ".lora_down.weight", "F32", {4, 9}), tensor(q + ".lora_up.weight", "F32", {12, 4})}, 0, SDMI_ERR_WEIGHTS},
        {"up of another rank", {tensor(q + ".lora_down.weight", "F32", {4, 8}), tensor(q + ".lora_up.weight", "F32", {12, 5})}, 0, SDMI_ERR_WEIGHTS},
        {"up alone", {tensor(q + ".lora_up.weight", "F32", {12, 4})}, 0, SDMI_ERR_WEIGHTS},
        {"alpha alone", {tensor(q + ".alpha", "F32", {})}, 0, SDMI_ERR_WEIGHTS},
        {"alpha of two elements", {tensor(q + ".lora_down.weight", "F32", {4, 8}), tensor(q + ".lora_up.weight", "F32", {12, 4}), tensor(q + ".alpha", "F32", {2})}, 0, SDMI_ERR_WEIGHTS},
        {"an integer alpha", {tensor(q + ".lora_down.weight", "F32", {4, 8}), tensor(q + ".lora_up.weight", "F32", {12, 4}), tensor(q + ".alpha", "I64", {})}, 0, SDMI_ERR_WEIGHTS},
        {"three LoHa factors", {tensor(q + ".hada_w1_a", "F32", {12, 3}), tensor(q + ".hada_w1_b", "F32", {3, 8}), tensor(q + ".hada_w2_a", "F32", {12, 3})}, 0, SDMI_ERR_WEIGHTS},
        {"LoHa ranks that differ", {tensor(q + ".hada_w1_a", "F32", {12, 3}), tensor(q + ".hada_w1_b", "F32", {3, 8}), tensor(q + ".hada_w2_a", "F32", {12, 2}), tensor(q + ".hada_w2_b", "F32", {2, 8})}, 0, SDMI_ERR_WEIGHTS},
        {"LoRA and LoHa factors in one module", {tensor(q + ".lora_down.weight", "F32", {4, 8}), tensor(q + ".lora_up.weight", "F32", {12, 4}), tensor(q + ".hada_w1_a", "F32", {12, 3})}, 0, SDMI_ERR_WEIGHTS},
        {"rank 0", {tensor(q + ".lora_down.weight", "F32", {0, 8}), tensor(q + ".lora_up.weight", "F32", {12, 0})}, 0, SDMI_ERR_WEIGHTS},
        {"rank 257", {tensor(q + ".lora_down.weight", "F32", {257, 8}), tensor(q + ".lora_up.weight", "F32", {12, 257})}, 0, SDMI_ERR_UNSUPPORTED},
        {"F64 factors", {tensor(q + ".lora_down.weight", "F64", {4, 8}), tensor(q + ".lora_up.weight", "F64", {12, 4})}, 0, SDMI_ERR_UNSUPPORTED},
        {"factors of two dtypes", {tensor(q + ".lora_down.weight", "F16", {4, 8}), tensor(q + ".lora_up.weight", "F32", {12, 4})}, 0, SDMI_ERR_UNSUPPORTED},
        {"an unknown module", {tensor("lora_unet_nope.lora_down.weight", "F32", {4, 8}), tensor("lora_unet_nope.lora_up.weight", "F32", {12, 4})}, 0, SDMI_ERR_UNSUPPORTED},
        {"an unknown module, skipped", {tensor("lora_unet_nope.lora_down.weight", "F32", {4, 8}), tensor("lora_unet_nope.lora_up.weight", "F32", {12, 4})}, kLoraSkipUnknown, 0},
        {"a 5-D factor", {tensor(q + ".lora_down.weight", "F32", {4, 8, 1, 1, 1}), tensor(q + ".lora_up.weight", "F32", {12, 4})}, 0, SDMI_ERR_WEIGHTS},
        {"a scalar factor", {tensor(q + ".lora_down.weight", "F32", {}), tensor(q + ".lora_up.weight", "F32", {12, 4})}, 0, SDMI_ERR_WEIGHTS},
        {"the 4-D spelling of a Linear", {tensor(q + ".lora_down.weight", "F32", {4, 8, 1, 1}), tensor(q + ".lora_up.weight", "F32", {12, 4, 1, 1})}, 0, 0},
        {"no tensors", {}, 0, 0},
    };
    for (const Case& c : cases) {
        expect(plan_status(c.ts, entries, both, c.flags) == c.status, c.what);
        ++checks;
    }
    {   // both spellings of one entry in one file
        const std::string q2 = "lora_unet_input_blocks_1_1_transformer_blocks_0_attn1_to_q";
        std::vector<StTensor> ts = {tensor(q + ".lora_down.weight", "F32", {4, 8}), tensor(q + ".lora_up.weight", "F32", {12, 4}), tensor(q2 + ".lora_down.weight", "F32", {4, 8}),
                                    tensor(q2 + ".lora_up.weight", "F32", {12, 4})};
        expect(plan_status(ts, entries, both, 0) == SDMI_ERR_WEIGHTS, "two modules naming one entry");
        ++checks;
    }
    {   // a conv entry: both spellings of its down factor, and the padded conv_in
        std::vector<LoraEntryDesc> es = entries;
        const int ci = table.find("lora_unet_conv_in"), c1 = table.find("lora_unet_down_blocks_0_resnets_0_conv1");
        expect(ci >= 0 && c1 >= 0, "conv entries of the table");
        if (ci >= 0 && c1 >= 0) {
            es[ci].kind = 0; es[ci].dims[0] = 8; es[ci].dims[1] = 9; es[ci].dims[2] = es[ci].dims[3] = 3; es[ci].padded = true;
            es[c1].kind = 0; es[c1].dims[0] = 8; es[c1].dims[1] = 5; es[c1].dims[2] = es[c1].dims[3] = 3;
            const std::string m = "lora_unet_down_blocks_0_resnets_0_conv1";
            expect(plan_status({tensor(m + ".lora_down.weight", "F16", {3, 5, 3, 3}), tensor(m + ".lora_up.weight", "F16", {8, 3, 1, 1})}, es, both, 0) == 0, "LoCon, 4-D");
            expect(plan_status({tensor(m + ".lora_down.weight", "F16", {3, 45}), tensor(m + ".lora_up.weight", "F16", {8, 3})}, es, both, 0) == 0, "LoCon, 2-D");
            expect(plan_status({tensor(m + ".lora_down.weight", "F16", {3, 5, 1, 9}), tensor(m + ".lora_up.weight", "F16", {8, 3})}, es, both, 0) == SDMI_ERR_WEIGHTS, "LoCon, a kernel of another shape");
            expect(plan_status({tensor(m + ".hada_w1_a", "F16", {8, 3}), tensor(m + ".hada_w1_b", "F16", {3, 45}), tensor(m + ".hada_w2_a", "F16", {8, 3}), tensor(m + ".hada_w2_b", "F16", {3, 5, 3, 3})}, es, both, 0) == 0,
                   "LoHa on a conv");
            expect(plan_status({tensor("lora_unet_conv_in.lora_down.weight", "F16", {2, 9, 3, 3}), tensor("lora_unet_conv_in.lora_up.weight", "F16", {8, 2, 1, 1})}, es, both, kLoraSkipUnknown) ==
                       SDMI_ERR_UNSUPPORTED, "a padded conv_in");
            checks += 5;
        }
    }
    std::printf("%ld checks, %d failed\n", checks, g_bad);
    return g_bad ? 1 : 0;
}
