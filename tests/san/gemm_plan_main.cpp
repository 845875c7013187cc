// gemm_plan_main.cpp -- replays the GEMM planner (csrc/gemm_plan.cpp, host-only) over a fixed list of cases and compares what it
// decides with tests/golden/gemm_plan_choices.txt, line by line.  Built by tests/test_gemm_plan_cpu.py with plain g++ (no HIP).
//
//   gemm_plan <fixture>      exit 0 when every line is reproduced, 1 with the first differing lines otherwise
//   gemm_plan                prints the lines (how the fixture was written -- by the code BEFORE the planner was rewritten)
//
// The fixture holds results only, in the order this file enumerates the cases; a token is cfg (one K slice), cfg/splits, or
// E<status> for an sdmi::Error.  So the enumeration below must not change unless the fixture is regenerated from a trusted planner.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../stable_diffusion_burn_amd/csrc/error.hpp"
#include "../../stable_diffusion_burn_amd/csrc/gemm_plan.hpp"

using namespace sdmi;

static std::string tok(int cfg, int splits) {
    char b[32];
    if (splits == 1) std::snprintf(b, sizeof b, " %d", cfg);
    else std::snprintf(b, sizeof b, " %d/%d", cfg, splits);
    return b;
}

// a case of the full plan: "geglu=1 gp=2 ..." over the defaults
struct Variant {
    int geglu = 0, out = 0, ap = 0, wp = 1;   // GEGLU form, out_mode, activations arrive as planes, weight planes present
    GemmPlanOpts o;
    int fc = -1, fs = 0;                      // caller-forced tile / split count
    explicit Variant(const char* spec) {
        std::istringstream ss(spec);
        std::string kv;
        while (ss >> kv) {
            const size_t eq = kv.find('=');
            const std::string k = kv.substr(0, eq);
            const int v = std::atoi(kv.c_str() + eq + 1);
            int* dst = k == "geglu" ? &geglu : k == "out" ? &out : k == "ap" ? &ap : k == "wp" ? &wp : k == "fc" ? &fc : k == "fs" ? &fs
                     : k == "gp" ? &o.gemm_planes : k == "c3" ? &o.conv3_reuse : k == "x32" ? &o.gemm_x32 : k == "f32s" ? &o.gemm_f32s
                     : k == "bf16x" ? &o.gemm_bf16x : k == "ft" ? &o.force_tile : k == "os" ? &o.force_splits : nullptr;
            if (!dst) { std::fprintf(stderr, "bad variant key %s\n", k.c_str()); std::exit(2); }
            *dst = v;
        }
    }
};

static const char* const kVarF32[] = {
    "", "gp=0", "gp=2", "geglu=1", "geglu=2", "gp=2 geglu=1", "gp=2 geglu=2", "ap=1", "ap=1 geglu=1", "ap=1 geglu=2", "ap=1 gp=2",
    "wp=0", "wp=0 ap=1", "wp=0 gp=2", "out=2", "out=2 os=3", "x32=0", "f32s=0", "x32=0 f32s=0", "f32s=0 gp=2",
    "ft=3", "ft=10", "ft=102", "ft=104", "ft=203", "ft=206", "ft=304", "ft=309", "ft=203 wp=0", "fc=203 wp=0", "ft=304 gp=0", "ft=203 gp=2",
    "ft=201 gp=2 geglu=1", "ft=202 gp=2 geglu=1", "ap=1 ft=203", "ap=1 fc=203", "ap=1 ft=308", "ap=1 fc=308 fs=1 geglu=2", "ft=102 out=2", "fc=102 out=2",
    "os=1", "os=3", "os=1000", "fs=3", "os=3 fs=1", "ap=1 os=3"};
static const char* const kVarF32Conv3[] = {"", "gp=2", "ap=1", "ft=102", "ft=203"};
static const char* const kVarBf16[] = {
    "", "bf16x=0", "c3=0", "geglu=1", "out=1", "ft=3", "ft=101", "ft=104", "ft=106", "ft=203", "fc=101", "os=1", "os=3", "os=1000", "fs=3", "c3=0 os=3", "ft=100"};

// the facts Engine::launch_gemm derives for a stride-1 layer [M pixels, K = Cin * taps] -> N
static bool make_in(int M, int N, int K, bool conv3, bool bf16, const Variant& v, GemmPlanIn* in) {
    GemmPlanIn p{};
    p.M = M; p.N = N; p.K = K; p.bf16 = bf16; p.geglu = v.geglu; p.out_mode = v.out;
    p.Cin = conv3 ? K / 9 : K;
    if (bf16 && p.Cin % 64) return false;   // (the engine refuses these before it plans)
    p.kt_total = (K + (bf16 ? 64 : 32) - 1) / (bf16 ? 64 : 32);
    p.KH = p.KW = conv3 ? 3 : 1; p.stride = 1; p.pad = conv3 ? 1 : 0; p.ups = 0;
    p.Hs = 1; p.Ws = M;
    if (conv3)
        for (int w : {128, 64, 32, 16})
            if (M % (w * w) == 0) { p.Hs = p.Ws = w; break; }
    p.Ho = p.Hs; p.Wo = p.Ws;
    p.zero_page = true;
    p.x32_ok = !bf16 && p.Cin % 32 == 0 && v.out == 0;
    p.s_ok = p.x32_ok && v.wp && (unsigned long long)N * (v.geglu ? 2 : 1) * (unsigned long long)p.kt_total * 192ull < 0xFFFFFF00ull;
    p.p_ok = p.s_ok && (unsigned long long)M * (unsigned long long)(p.Cin * 6) < 0xFFFFFF00ull;
    p.from_planes = !bf16 && v.ap;
    p.force_cfg = v.fc; p.force_splits = v.fs;
    *in = p;
    return true;
}

static std::string run(const GemmPlanIn& in, const GemmPlanOpts& o, const GemmTuning& t) {
    try {
        const GemmPlan g = plan_gemm(in, o, t);
        if (g.cfg != g.tile.cfg() || g.kt_per_split != (in.kt_total + g.splits - 1) / g.splits) return " BAD";
        return tok(g.cfg, g.splits);
    } catch (const Error& e) {
        return " E" + std::to_string(e.status);
    }
}

static const int kM[] = {1, 2, 16, 64, 77, 154, 256, 1024, 1232, 2464, 4096, 8192, 16384, 32768, 65536, 131072, 262144};
static const int kN[] = {3, 4, 8, 64, 128, 256, 320, 512, 640, 768, 1280, 2560, 5120, 10240};
static const int kKt[] = {1, 2, 3, 4, 5, 8, 9, 10, 16, 20, 24, 30, 36, 40, 45, 60, 72, 80, 90, 120, 144, 160, 180, 270, 360, 540};

// (i) the cost model alone: empty tables, every kernel family applicable
static void cost_section(std::ostream& os, const char* name, bool bf16, bool planes, int geglu, const char* opts, int every) {
    const GemmTuning none;
    const Variant v(opts);
    os << "# cost " << name << "\n";
    long long idx = 0;
    for (int M : kM)
        for (int N : kN) {
            os << M << " " << N << ":";
            for (int kt : kKt) {
                if (idx++ % every) continue;
                GemmPlanIn p{};
                p.M = M; p.N = N; p.kt_total = kt; p.K = kt * (bf16 ? 64 : 32); p.bf16 = bf16; p.geglu = geglu;
                p.Cin = p.K; p.KH = p.KW = 1; p.stride = 1; p.Hs = p.Ho = 1; p.Ws = p.Wo = M; p.zero_page = true;
                p.x32_ok = p.s_ok = p.p_ok = !bf16;
                p.from_planes = planes;
                os << run(p, v.o, none);
            }
            os << "\n";
        }
}

// (ii) the full plan on the measured shapes
static void plan_section(std::ostream& os, const GemmTuning& t) {
    os << "# plan fp32\n";
    std::map<std::string, int> keys;
    for (auto* m : {&t.f32, &t.mfma, &t.planes}) for (auto& kv : *m) keys[kv.first] = 0;
    auto lines = [&](const std::map<std::string, int>& ks, bool bf16) {
        for (auto& kv : ks) {
            int M, N, K;
            if (std::sscanf(kv.first.c_str(), "%d,%d,%d", &M, &N, &K) != 3) std::exit(2);
            for (int conv3 = 0; conv3 < 2; ++conv3) {
                if (conv3 && K % 9) continue;
                os << kv.first << (conv3 ? " k3:" : " k1:");
                auto each = [&](const char* const* vs, size_t n) {
                    for (size_t i = 0; i < n; ++i) {
                        const Variant v(vs[i]);
                        GemmPlanIn in;
                        if (!make_in(M, N, K, conv3, bf16, v, &in)) { os << " -"; continue; }
                        os << run(in, v.o, t);
                    }
                };
                if (bf16) each(kVarBf16, sizeof kVarBf16 / sizeof *kVarBf16);
                else if (conv3) each(kVarF32Conv3, sizeof kVarF32Conv3 / sizeof *kVarF32Conv3);
                else each(kVarF32, sizeof kVarF32 / sizeof *kVarF32);
                os << "\n";
            }
        }
    };
    lines(keys, false);
    os << "# plan bf16\n";
    keys.clear();
    for (auto& kv : t.bf16) keys[kv.first] = 0;
    lines(keys, true);
}

static void fp8_section(std::ostream& os) {
    os << "# fp8\n";
    for (int M : {64, 1024, 4096, 8192, 65536})
        for (int N : {320, 640, 1280, 2560}) {
            os << M << " " << N << ":";
            for (int kt : {1, 3, 8, 23, 90, 180})
                for (int tile : {-1, 0, 1, 2, 3})
                    for (int fs : {0, 3, 1000}) {
                        if (fs && tile >= 0) continue;
                        try {
                            int per = 0;
                            const TileChoice c = plan_gemm_fp8(M, N, kt, tile, fs, &per);
                            os << (per == (kt + c.splits - 1) / c.splits ? tok(c.cfg, c.splits) : " BAD");
                        } catch (const Error& e) { os << " E" << e.status; }
                    }
            os << "\n";
        }
}

static void geglu_section(std::ostream& os, const GemmTuning& t) {
    os << "# geglu\n";
    for (long long rows : {1024ll, 4096ll, 16384ll, 65536ll})
        for (int hidden : {1280, 2560, 5120}) {
            os << rows << " " << hidden << ":";
            for (int cin : {320, 640, 1280})
                for (const char* s : {"", "ft=308", "ft=304", "ft=203", "os=3", "os=1"}) os << " " << plan_geglu_plane_tile(rows, hidden, cin, Variant(s).o, t);
            for (int fuse = 1; fuse <= 6; ++fuse)
                for (int f32s = 0; f32s < 2; ++f32s) os << " " << plan_geglu_paired_tile(rows, hidden, fuse, f32s != 0);
            os << "\n";
        }
}

int main(int argc, char** argv) {
    std::ostringstream os;
    cost_section(os, "fp32", false, false, 0, "", 1);
    cost_section(os, "bf16", true, false, 0, "bf16x=1", 1);
    cost_section(os, "planes", false, true, 0, "", 1);
    cost_section(os, "planes-even", false, true, 1, "", 1);
    cost_section(os, "fp32-mfma4", false, false, 0, "x32=0 f32s=0", 1);
    cost_section(os, "bf16-4wave", true, false, 0, "bf16x=0", 4);
    GemmTuning t;
    t.load_builtin();
    plan_section(os, t);
    fp8_section(os);
    geglu_section(os, t);
    // options tune / tune_bf16 / tune_clear: where an entry lands, and what is refused
    os << "# tune\n";
    for (const char* s : {"1,2,3=3,2", "1,2,3=104,1", "1,2,3=205,4", "1,2,3=308,1", "1,2,3=309,1", "1,2,3=10,1", "1,2,3=3,0", "1,2,3", "1,2,3=x"})
        for (int b16 = 0; b16 < 2; ++b16) {
            GemmTuning u;
            try { u.set(s, b16 != 0); os << " " << u.f32.size() << u.mfma.size() << u.planes.size() << u.bf16.size(); } catch (const Error& e) { os << " E" << e.status; }
        }
    os << "\n";
    const std::string got = os.str();
    if (argc < 2) { std::fputs(got.c_str(), stdout); return 0; }
    std::ifstream f(argv[1]);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::istringstream g(got);
    std::string a, b;
    int line = 0, bad = 0;
    for (;;) {
        const bool ha = (bool)std::getline(f, a), hb = (bool)std::getline(g, b);
        if (!ha && !hb) break;
        ++line;
        if (ha != hb || a != b) {
            if (++bad <= 5) std::fprintf(stderr, "line %d differs:\n  fixture: %s\n  planner: %s\n", line, ha ? a.c_str() : "<end>", hb ? b.c_str() : "<end>");
        }
    }
    std::printf("%d lines, %d differ\n", line, bad);
    return bad ? 1 : 0;
}
