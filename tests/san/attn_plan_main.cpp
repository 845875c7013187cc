// attn_plan_main.cpp -- replays the attention planner (csrc/attn_plan.cpp, host-only) over a fixed list of cases and compares what it
// decides with tests/golden/attn_plan_choices.txt, line by line.  Built by tests/test_attn_plan_cpu.py with plain g++ (no HIP).
//
//   attn_plan <fixture>      exit 0 when every line is reproduced, 1 with the first differing lines otherwise
//   attn_plan                prints the lines (how the fixture was written -- by the code BEFORE the planner was restructured)
//   attn_plan --replay <f>   plans the cases a fixture NAMES: every line of <f> that is no comment is parsed back into its case
//                            ("f32|bf16 [mask] [planes] [unaligned] d<D> n<N> h<H> q<NQ> k<NK>:", the words setting has_mask, planes_out and
//                            !rows_aligned), planned under every option variant and compared with the line.  No grid, no form census:
//                            tests/golden/attn_plan_masked_cases.txt, the shapes of tests/test_attention_mask_gpu.py
//   attn_plan --views <f>    answers the lines of <f>, one line of output each (tests/test_attention_views_cpu.py writes them from tests/attn_view_cases.py):
//                            "plan <bf16> <mask> <planes> <d> <n> <heads> <nq> <nk> <attn_split> <attn_bf16> <attn_bf16_variant> <attn_pack_tail> <attn_kv_splits>
//                            <attn_kv_prefer8> <attn_d64>" -> "<kernel> <waves> <q_rows> <kv_splits>" (kernel: unfused / flash / split / bf16) or "E<status>";
//                            "view <bf16> <n> <nq> <nk> <n_state> <packed> <ld off rows of q, k, v, out> <out_planes>" -> "ok" or "E<status>" (check_attention_view)
//
// Every run without --replay / --views first puts check_attention_view through its own accept and refuse cases (view_selftest below).
//
// One line per (storage, d, n, heads, nq, nk), one token per option variant in the order of variants() below; equal neighbours are
// folded into "token*count".  A token is
//   F<waves>                k_attn.hip
//   S<waves>[p][l]          k_attn_split.hip, template flags PK / LG
//   B<waves>[.<wpe>.<qr>]   k_attn_bf16.hip (.1.1 left out)
//   U                       the unfused path
// followed by /<slices> when there is more than one key slice, or E<status> for an sdmi::Error.  The "# geometry" section lists query
// rows per workgroup and keys per tile of every (kernel, d, waves, qr) that occurred.  The fixture holds results only, so the
// enumeration below must not change unless the fixture is regenerated from a trusted planner.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../../stable_diffusion_burn_amd/csrc/attn_plan.hpp"
#include "../../stable_diffusion_burn_amd/csrc/error.hpp"

using namespace sdmi;

static std::set<std::string> g_forms;                // every instantiation / slice rule that occurred: condition (b)
static std::map<std::string, std::string> g_geom;    // (kernel, d, waves, qr) -> "q_rows kv_tile"
static int g_refused = 0;                            // condition (a)

static std::vector<AttnPlanOpts> variants(bool bf16) {
    std::vector<AttnPlanOpts> v;
    if (!bf16) {
        for (int split : {1, 0})
            for (int kv : {0, 1, 2, 8, 1000})
                for (int p8 : {1, 0})
                    for (int pack : {3, 2, 1, 0}) {
                        AttnPlanOpts o;
                        o.attn_split = split; o.attn_kv_splits = kv; o.attn_kv_prefer8 = p8; o.attn_pack_tail = pack;
                        v.push_back(o);
                    }
    } else {
        for (int on : {1, 0})
            for (int var : {7, 0, 1, 2, 4, 6, 0x101, 0x102, 0x104, 0x106}) {
                AttnPlanOpts o;
                o.attn_bf16 = on; o.attn_bf16_variant = var;
                v.push_back(o);
            }
    }
    return v;
}

static std::string run(const AttnPlanIn& in, const AttnPlanOpts& o) {
    try {
        const AttnPlan a = plan_attention(in, o);
        const std::string where = in.bf16 ? "bf16" : in.has_mask ? "f32 mask" : "f32";
        const std::string d = " d" + std::to_string(in.d_head), w = std::to_string(a.waves);
        std::string t;
        switch (a.kernel) {
            case AttnKernel::Unfused: return "U";
            case AttnKernel::Flash: t = "F" + w; break;
            case AttnKernel::Split: t = "S" + w + (a.pk ? "p" : "") + (a.lg ? "l" : ""); break;
            case AttnKernel::Bf16: t = "B" + w + (a.wpe == 1 && a.qr == 1 ? "" : "." + std::to_string(a.wpe) + "." + std::to_string(a.qr)); break;
        }
        g_forms.insert(t + d + " " + where);
        const std::string key = t.substr(0, 1) + d + " w" + w + " qr" + std::to_string(a.qr);
        const std::string geom = std::to_string(a.q_rows) + " " + std::to_string(a.kv_tile);
        if (g_geom.count(key) && g_geom[key] != geom) return "BAD";
        g_geom[key] = geom;
        if (!in.bf16 && !in.has_mask && o.attn_kv_splits == 0 && (a.kv_splits == 1 || a.kv_splits == 4 || a.kv_splits == 8))   // the automatic slice counts the model reaches
            g_forms.insert("auto" + std::to_string(a.kv_splits) + (a.kv_splits != 8 ? "" : o.attn_kv_prefer8 ? " prefer8=1" : " prefer8=0"));
        if (a.kv_splits > 1) t += "/" + std::to_string(a.kv_splits);
        return t;
    } catch (const Error& e) {
        ++g_refused;
        return "E" + std::to_string(e.status);
    }
}

static AttnPlanIn make_in(bool bf16, int d, int n, int heads, int nq, int nk, bool mask = false, bool planes = false, bool aligned = true) {
    AttnPlanIn p{};
    p.n = n; p.n_head = heads; p.nq = nq; p.nk = nk; p.d_head = d; p.bf16 = bf16; p.has_mask = mask; p.planes_out = planes; p.rows_aligned = aligned;
    return p;
}

static void line(std::ostream& os, const AttnPlanIn& in, const char* note = "") {
    os << (in.bf16 ? "bf16" : "f32") << note << " d" << in.d_head << " n" << in.n << " h" << in.n_head << " q" << in.nq << " k" << in.nk << ":";
    std::string prev;
    int count = 0;
    auto flush = [&] {
        if (!count) return;
        os << " " << prev;
        if (count > 1) os << "*" << count;
    };
    for (const AttnPlanOpts& o : variants(in.bf16 != 0)) {
        const std::string t = run(in, o);
        if (t == prev) { ++count; continue; }
        flush();
        prev = t; count = 1;
    }
    flush();
    os << "\n";
}

// --replay: the fixture names its cases, see the head of this file
static int replay(const char* path) {
    std::ifstream f(path);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string a;
    int ln = 0, cases = 0, bad = 0;
    while (std::getline(f, a)) {
        ++ln;
        if (a.empty() || a[0] == '#') continue;
        std::istringstream hs(a.substr(0, a.find(':')));
        std::string w, note;
        bool bf16 = false, mask = false, planes = false, aligned = true, ok = (bool)(hs >> w) && (w == "f32" || w == "bf16") && a.find(':') != std::string::npos;
        bf16 = w == "bf16";
        int val[5] = {0, 0, 0, 0, 0}, seen = 0;   // d n h q k, in this order
        while (ok && hs >> w) {
            if (w == "mask") mask = true;
            else if (w == "planes") planes = true;
            else if (w == "unaligned") aligned = false;
            else if (seen < 5 && w.size() > 1 && w[0] == "dnhqk"[seen] && w.find_first_not_of("0123456789", 1) == std::string::npos && w.size() < 9) { val[seen++] = std::atoi(w.c_str() + 1); continue; }
            else ok = false;
            if (seen) ok = false;   // the words come before the numbers
            note += " " + w;
        }
        if (!ok || seen != 5) { std::fprintf(stderr, "line %d is no case: %s\n", ln, a.c_str()); return 2; }
        std::ostringstream os;
        line(os, make_in(bf16, val[0], val[1], val[2], val[3], val[4], mask, planes, aligned), note.c_str());
        ++cases;
        if (os.str() != a + "\n" && ++bad <= 5) std::fprintf(stderr, "line %d differs:\n  fixture: %s\n  planner: %s", ln, a.c_str(), os.str().c_str());
    }
    std::printf("%d cases, %d differ\n", cases, bad);
    return bad ? 1 : 0;
}

// --views: see the head of this file
static int views(const char* path) {
    std::ifstream f(path);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string a;
    int ln = 0;
    while (std::getline(f, a)) {
        ++ln;
        if (a.empty() || a[0] == '#') continue;
        std::istringstream is(a);
        std::string kind;
        is >> kind;
        std::vector<int> x;
        for (int t; is >> t;) x.push_back(t);
        try {
            if (kind == "plan" && x.size() == 15) {
                const AttnPlanIn in = make_in(x[0] != 0, x[3], x[4], x[5], x[6], x[7], x[1] != 0, x[2] != 0);
                AttnPlanOpts o;
                o.attn_split = x[8]; o.attn_bf16 = x[9]; o.attn_bf16_variant = x[10]; o.attn_pack_tail = x[11]; o.attn_kv_splits = x[12]; o.attn_kv_prefer8 = x[13]; o.attn_d64 = x[14];
                const AttnPlan p = plan_attention(in, o);
                static const char* names[] = {"unfused", "flash", "split", "bf16"};
                std::printf("%s %d %d %d\n", names[(int)p.kernel], p.waves, p.q_rows, p.kv_splits);
            } else if (kind == "view" && x.size() == 19) {
                AttnViewIn v{};
                v.bf16 = x[0]; v.n = x[1]; v.nq = x[2]; v.nk = x[3]; v.n_state = x[4]; v.packed = x[5] != 0;
                v.q = {x[6], x[7], x[8]}; v.k = {x[9], x[10], x[11]}; v.v = {x[12], x[13], x[14]}; v.out = {x[15], x[16], x[17]}; v.out_planes = x[18] != 0;
                check_attention_view(v);
                std::printf("ok\n");
            } else {
                std::fprintf(stderr, "line %d is no case: %s\n", ln, a.c_str());
                return 2;
            }
        } catch (const Error& e) {
            std::printf("E%d\n", e.status);
        }
    }
    return 0;
}

// check_attention_view on views it must take and views it must refuse (SDMI_ERR_INVALID), at both element sizes: the model's packed [n][T][3C] buffer, gaps
// and filler rows, three parents with different strides; every way a slice can leave its parent, overlap a neighbour or miss a 16-byte boundary
static int view_selftest() {
    int bad = 0;
    auto expect = [&](const AttnViewIn& v, bool ok, const char* what) {
        int st = 0;
        try { check_attention_view(v); } catch (const Error& e) { st = e.status; }
        if ((st == 0) != ok || (!ok && st != SDMI_ERR_INVALID)) { std::fprintf(stderr, "check_attention_view: %s (bf16=%d): status %d\n", what, v.bf16, st); ++bad; }
    };
    for (int bf16 = 0; bf16 < 2; ++bf16) {
        const int g = bf16 ? 8 : 4, c = 80, nq = 100, nk = 520;
        AttnViewIn self{};
        self.n = 2; self.nq = nq; self.nk = nq; self.n_state = c; self.bf16 = bf16; self.packed = true;
        self.q = {3 * c, 0, nq}; self.k = {3 * c, c, nq}; self.v = {3 * c, 2 * c, nq}; self.out = {c, 0, nq};
        expect(self, true, "the model's packed buffer");
        AttnViewIn planes = self;
        planes.out_planes = true;
        expect(planes, true, "the model's packed buffer, plane output");
        AttnViewIn pk = self;
        pk.nk = nk;
        pk.q = {3 * c + 3 * g, g, nk + 5}; pk.k = {3 * c + 3 * g, c + 2 * g, nk + 5}; pk.v = {3 * c + 3 * g, 2 * c + 3 * g, nk + 5}; pk.out = {c + 2 * g, g, nq + 3};
        expect(pk, true, "packed with gaps");
        AttnViewIn ap = pk;
        ap.packed = false;
        ap.q = {c + g, 0, nq + 1}; ap.k = {c + 2 * g, 2 * g, nk + 2}; ap.v = {c + 3 * g, g, nk + 3}; ap.out = {c + 4 * g, g, nq + 2};
        expect(ap, true, "three parents");
        AttnViewIn same = ap;       // slices of different parents may share columns
        same.k = same.v;
        expect(same, true, "three parents, equal slices");
        AttnViewIn t;
        t = ap; t.q.off = 2 * g; expect(t, false, "q: ld < off + n_state");
        t = ap; t.k.ld = c - g; expect(t, false, "k: ld < n_state");
        t = ap; t.v.off = -g; expect(t, false, "v: negative off");
        t = ap; t.q.rows = nq - 1; expect(t, false, "q: rows < nq");
        t = ap; t.k.rows = nk - 1; expect(t, false, "k: rows < nk");
        t = ap; t.v.rows = 0; expect(t, false, "v: no rows");
        t = ap; t.out.off = t.out.ld - c + g; expect(t, false, "out: leaves its parent");
        t = ap; t.out.rows = nq - 1; expect(t, false, "out: rows < nq");
        t = ap; t.q.ld += g / 2; expect(t, false, "q: ld off 16 bytes");
        t = ap; t.k.off = g / 2; expect(t, false, "k: off off 16 bytes");
        t = ap; t.v.ld += 1; expect(t, false, "v: ld off 16 bytes");
        t = ap; t.out.off = g / 2; expect(t, false, "out: off off 16 bytes");
        t = ap; t.out.ld += g / 2; expect(t, false, "out: ld off 16 bytes");
        t = ap; t.out_planes = true; expect(t, false, "a strided plane output");
        t = pk; t.k.off = t.q.off + c - g; expect(t, false, "packed: q and k overlap");
        t = pk; t.v.off = t.k.off; expect(t, false, "packed: k and v coincide");
        t = pk; t.k.ld += g; expect(t, false, "packed: different ld");
        t = pk; t.v.rows += 1; expect(t, false, "packed: different rows");
        t = ap; t.n = 0; expect(t, false, "no samples");
        t = ap; t.q.ld = 0x7FFFFFF8; t.q.off = 0x7FFFFFF0; expect(t, false, "off + n_state past INT_MAX");
    }
    if (bad) std::fprintf(stderr, "%d view cases went wrong\n", bad);
    return bad;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--replay") return replay(argv[2]);
    if (argc == 3 && std::string(argv[1]) == "--views") return views(argv[2]);
    if (view_selftest()) return 2;
    std::ostringstream os;
    os << "# written by the planner's first form, Engine::attention's and the launchers' rules moved out verbatim; never regenerated since\n";
    for (int bf16 = 0; bf16 < 2; ++bf16) {
        os << (bf16 ? "# grid bf16\n" : "# grid fp32\n");
        for (int d : {40, 64, 80, 160})
            for (int n : {1, 2, 4, 16})
                for (int heads : {1, 8})
                    for (int nq : {64, 256, 1024, 2085, 4096})
                        for (int nk : {77, 128, 129, nq}) line(os, make_in(bf16 != 0, d, n, heads, nq, nk));
    }
    os << "# masked fp32\n";
    line(os, make_in(false, 64, 1, 12, 77, 77, true));   // CLIP
    for (int d : {40, 64, 80, 160}) {
        line(os, make_in(false, d, 2, 8, 64, 77, true));
        line(os, make_in(false, d, 2, 8, 4096, 77, true));
        line(os, make_in(false, d, 16, 8, 1024, 1024, true));
    }
    os << "# planes out\n";
    for (int d : {40, 64, 80, 160})
        for (int n : {1, 2})
            for (int nq : {64, 1024, 4096})
                for (int nk : {77, nq}) line(os, make_in(false, d, n, 8, nq, nk, false, true));
    line(os, make_in(false, 40, 1, 4, 1024, 1024, false, true));
    os << "# row strides not 16-byte aligned\n";
    for (int bf16 = 0; bf16 < 2; ++bf16)
        for (int d : {40, 80})
            for (int nq : {64, 4096}) line(os, make_in(bf16 != 0, d, 2, 8, nq, nq, false, false, false), " unaligned");
    os << "# unfused\n";
    for (int bf16 = 0; bf16 < 2; ++bf16)
        for (int n : {1, 2})
            for (int nq : {1024, 4096}) line(os, make_in(bf16 != 0, 512, n, 1, nq, nq));
    if (g_refused) { std::fprintf(stderr, "%d cases of the grid were refused\n", g_refused); return 2; }   // (a)

    os << "# refusals\n";
    line(os, make_in(true, 40, 2, 8, 1024, 77, true), " mask");
    line(os, make_in(true, 64, 1, 12, 77, 77, true), " mask");
    line(os, make_in(false, 48, 2, 8, 1024, 1024));
    line(os, make_in(true, 48, 2, 8, 1024, 1024));
    line(os, make_in(false, 512, 1, 1, 1024, 1024, true), " mask");
    line(os, make_in(true, 96, 1, 1, 1024, 1024));
    line(os, make_in(true, 40, 2, 8, 1024, 1024, false, true), " planes");
    line(os, make_in(false, 40, 2, 1, 1024, 1024, false, true), " planes");
    line(os, make_in(false, 80, 2, 1, 1024, 77, false, true), " planes");
    line(os, make_in(false, 512, 1, 1, 1024, 1024, false, true), " planes");
    line(os, make_in(true, 512, 1, 1, 1024, 1024, false, true), " planes");

    os << "# geometry: kernel, d, waves, query blocks per wave: query rows per workgroup, keys per tile\n";
    for (auto& kv : g_geom) os << kv.first << ": " << kv.second << "\n";

    // (b) every instantiated kernel and every automatic slice count occurs
    std::vector<std::string> need = {"auto1", "auto4", "auto8 prefer8=1", "auto8 prefer8=0"};
    for (int d : {40, 64, 80, 160})
        for (const char* w : {"F4", "F8"})
            for (const char* where : {"f32", "f32 mask", "bf16"}) need.push_back(std::string(w) + " d" + std::to_string(d) + " " + where);
    for (const char* f : {"S4", "S4p", "S4l", "S4pl", "S8", "S8p", "S8l", "S8pl"}) need.push_back(std::string(f) + " d40 f32");
    for (const char* f : {"S4", "S4l", "S8l"}) need.push_back(std::string(f) + " d80 f32");
    for (int d : {40, 80, 160})
        for (const char* f : {"B2", "B4", "B8"}) need.push_back(std::string(f) + " d" + std::to_string(d) + " bf16");
    for (const char* f : {"B4.2.2 d40", "B8.2.2 d40", "B4.2.1 d40", "B4.2.1 d80"}) need.push_back(std::string(f) + " bf16");
    int missing = 0;
    for (const std::string& f : need)
        if (!g_forms.count(f)) { std::fprintf(stderr, "form never planned: %s\n", f.c_str()); ++missing; }
    if (missing || need.size() != g_forms.size()) {
        for (const std::string& f : g_forms)
            if (std::find(need.begin(), need.end(), f) == need.end()) std::fprintf(stderr, "form without an instantiation: %s\n", f.c_str());
        return 2;
    }

    const std::string got = os.str();
    if (argc < 2) { std::fputs(got.c_str(), stdout); return 0; }
    std::ifstream f(argv[1]);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::istringstream g(got);
    std::string a, b;
    int ln = 0, bad = 0;
    for (;;) {
        const bool ha = (bool)std::getline(f, a), hb = (bool)std::getline(g, b);
        if (!ha && !hb) break;
        ++ln;
        if (ha != hb || a != b) {
            if (++bad <= 5) std::fprintf(stderr, "line %d differs:\n  fixture: %s\n  planner: %s\n", ln, ha ? a.c_str() : "<end>", hb ? b.c_str() : "<end>");
        }
    }
    std::printf("%d lines, %d differ\n", ln, bad);
    return bad ? 1 : 0;
}
