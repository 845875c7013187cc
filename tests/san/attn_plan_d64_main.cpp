// attn_plan_d64_main.cpp -- the attention planner (csrc/attn_plan.cpp, host-only) with option attn_d64 given per case: tests/test_sd2_cpu.py builds it with plain
// g++ (no HIP) next to tests/san/attn_plan_main.cpp, whose enumeration and fixture stay as they are.
//
//   attn_plan_d64 <cases>    one case per line of <cases>: "attn_d64 bf16 mask aligned d n h q k" (nine integers).  Per case one output line:
//                            the line tests/golden/attn_plan_choices.txt would hold for it -- one token per option variant in attn_plan_main.cpp's order, equal
//                            neighbours folded -- with attn_d64 set in every variant, then " | kernel waves q_rows kv_tile kv_splits" of the plan under the
//                            default options + attn_d64 (kernel: U, F, S, B; E<status> alone for a refusal)
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../stable_diffusion_burn_amd/csrc/attn_plan.hpp"
#include "../../stable_diffusion_burn_amd/csrc/error.hpp"

using namespace sdmi;

static std::vector<AttnPlanOpts> variants(bool bf16, int d64) {   // attn_plan_main.cpp's, + attn_d64
    std::vector<AttnPlanOpts> v;
    if (!bf16) {
        for (int split : {1, 0})
            for (int kv : {0, 1, 2, 8, 1000})
                for (int p8 : {1, 0})
                    for (int pack : {3, 2, 1, 0}) {
                        AttnPlanOpts o;
                        o.attn_split = split; o.attn_kv_splits = kv; o.attn_kv_prefer8 = p8; o.attn_pack_tail = pack; o.attn_d64 = d64;
                        v.push_back(o);
                    }
    } else {
        for (int on : {1, 0})
            for (int var : {7, 0, 1, 2, 4, 6, 0x101, 0x102, 0x104, 0x106}) {
                AttnPlanOpts o;
                o.attn_bf16 = on; o.attn_bf16_variant = var; o.attn_d64 = d64;
                v.push_back(o);
            }
    }
    return v;
}

static const char* letter(AttnKernel k) { return k == AttnKernel::Unfused ? "U" : k == AttnKernel::Flash ? "F" : k == AttnKernel::Split ? "S" : "B"; }

static std::string token(const AttnPlanIn& in, const AttnPlanOpts& o) {
    try {
        const AttnPlan a = plan_attention(in, o);
        const std::string w = std::to_string(a.waves);
        std::string t;
        switch (a.kernel) {
            case AttnKernel::Unfused: return "U";
            case AttnKernel::Flash: t = "F" + w; break;
            case AttnKernel::Split: t = "S" + w + (a.pk ? "p" : "") + (a.lg ? "l" : ""); break;
            case AttnKernel::Bf16: t = "B" + w + (a.wpe == 1 && a.qr == 1 ? "" : "." + std::to_string(a.wpe) + "." + std::to_string(a.qr)); break;
        }
        if (a.kv_splits > 1) t += "/" + std::to_string(a.kv_splits);
        return t;
    } catch (const Error& e) {
        return "E" + std::to_string(e.status);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: attn_plan_d64 <cases>\n"); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string ln;
    while (std::getline(f, ln)) {
        if (ln.empty() || ln[0] == '#') continue;
        std::istringstream is(ln);
        int d64, bf16, mask, aligned, d, n, h, q, k;
        if (!(is >> d64 >> bf16 >> mask >> aligned >> d >> n >> h >> q >> k)) { std::fprintf(stderr, "no case: %s\n", ln.c_str()); return 2; }
        AttnPlanIn in{};
        in.n = n; in.n_head = h; in.nq = q; in.nk = k; in.d_head = d; in.bf16 = bf16; in.has_mask = mask != 0; in.planes_out = false; in.rows_aligned = aligned != 0;
        std::ostringstream os;
        os << (bf16 ? "bf16" : "f32") << " d" << d << " n" << n << " h" << h << " q" << q << " k" << k << ":";
        std::string prev;
        int count = 0;
        auto flush = [&] {
            if (!count) return;
            os << " " << prev;
            if (count > 1) os << "*" << count;
        };
        for (const AttnPlanOpts& o : variants(bf16 != 0, d64)) {
            const std::string t = token(in, o);
            if (t == prev) { ++count; continue; }
            flush();
            prev = t; count = 1;
        }
        flush();
        AttnPlanOpts def;
        def.attn_d64 = d64;
        try {
            const AttnPlan a = plan_attention(in, def);
            os << " | " << letter(a.kernel) << " " << a.waves << " " << a.q_rows << " " << a.kv_tile << " " << a.kv_splits;
        } catch (const Error& e) {
            os << " | E" << e.status;
        }
        std::puts(os.str().c_str());
    }
    return 0;
}
