// linear_pair_plan_main.cpp -- runs the pair planner (csrc/gemm_plan.cpp plan_gemm_pair, host-only) over Linear main problems: the batch-1 model's four transformer
// tails (mlp_lin K = 4C on the folded weight + proj_out K = C on extra slices; Engine::linear_pair) and a shape sweep, and checks what it promises.  Built by
// tests/test_linear_pair_plan_cpu.py with plain g++ (no HIP) under -fsanitize=address,undefined.
//
//   linear_pair_plan         one line per model pair ("pair M,N,Kmain+Kaux cfg=.. kt=.. main=.. aux=.. rounds=../..", or "... none"), then "<n> cases, <bad> bad";
//                            exit 1 when a promise is broken (the first ones on stderr)
//
// Promises, as for a ResBlock's pair (gemm_pair_plan_main.cpp): no slice is empty and the slices cover every k tile of their problem exactly once; the tile is plan_gemm's
// for the main launch; a planned pair needs no more rounds of 256 workgroups than the main launch alone, no slice is shorter than four k tiles (unless the main problem
// is) or than the main launch's slices today, and kt is the smallest such; a "0" row means no pair, a measured row is taken as written; forced slice counts are met
// through the shared kt.
#include <algorithm>
#include <cstdio>
#include <string>

#include "../../stable_diffusion_burn_amd/csrc/error.hpp"
#include "../../stable_diffusion_burn_amd/csrc/gemm_plan.hpp"

using namespace sdmi;

static int g_cases = 0, g_bad = 0;

static void bad(const char* what, int M, int N, int K, int ka, int fm, int fa) {
    if (++g_bad <= 10) std::fprintf(stderr, "BROKEN: %s at M=%d N=%d K=%d Kaux=%d forced=(%d,%d)\n", what, M, N, K, ka, fm, fa);
}

// a Linear layer K -> N over M rows as Engine::linear_gemm lays it out (one image of 1 x M pixels, one tap), activations as planes
static GemmPlanIn linear_in(int M, int N, int K) {
    GemmPlanIn in{};
    in.M = M; in.N = N; in.K = K; in.kt_total = K / 32;
    in.x32_ok = in.s_ok = in.p_ok = in.from_planes = true;
    in.KH = in.KW = 1; in.stride = 1; in.pad = 0; in.ups = 0; in.Cin = K; in.Hs = in.Ho = 1; in.Ws = in.Wo = M;
    in.zero_page = true;
    return in;
}

static long long rounds(const GemmTileId& id, int M, int N, int slices) {
    const GemmTileInfo& ti = id.info();
    const long long tiles = (long long)((M + ti.bm - 1) / ti.bm) * ((N + ti.bn - 1) / ti.bn);
    return (tiles * slices + 255) / 256;
}

static GemmPairPlan check(const GemmPlanIn& in, int ka, const GemmPlanOpts& o, const GemmTuning& t, int fm, int fa, bool table_row) {
    ++g_cases;
    const int kta = ka / 32;
    const GemmPlan g = plan_gemm(in, o, t);
    const GemmPairPlan p = plan_gemm_pair(in, ka, kta, o, t, fm, fa);
    if (!p.pair) {
        if (fm > 0 || fa > 0) bad("a forced request did not pair", in.M, in.N, in.K, ka, fm, fa);
        return p;
    }
    const int kt = p.kt_per_split;
    if (kt < 1) { bad("kt_per_split < 1", in.M, in.N, in.K, ka, fm, fa); return p; }
    if (p.splits_main != (in.kt_total + kt - 1) / kt || p.splits_aux != (kta + kt - 1) / kt) bad("slice counts do not cover the k tiles", in.M, in.N, in.K, ka, fm, fa);
    if (p.splits_main < 1 || p.splits_aux < 1 || (p.splits_main - 1) * kt >= in.kt_total || (p.splits_aux - 1) * kt >= kta) bad("an empty slice", in.M, in.N, in.K, ka, fm, fa);
    if (p.tile.family != kFamP || !p.tile.in_range(false) || p.cfg != p.tile.cfg()) bad("not a plane tile", in.M, in.N, in.K, ka, fm, fa);
    if (!table_row && (p.tile.family != g.tile.family || p.tile.index != g.tile.index)) bad("the tile is not plan_gemm's", in.M, in.N, in.K, ka, fm, fa);
    if (fm > 0 || fa > 0) {
        const int sm = std::max(1, std::min(fm, in.kt_total)), sa = std::max(1, std::min(fa, kta));
        if (p.splits_main > sm || p.splits_aux > sa) bad("more slices than requested", in.M, in.N, in.K, ka, fm, fa);
        if (kt != std::max((in.kt_total + sm - 1) / sm, (kta + sa - 1) / sa)) bad("forced kt", in.M, in.N, in.K, ka, fm, fa);
    } else if (!table_row) {
        if (g.splits <= 1) bad("paired a launch that is not split today", in.M, in.N, in.K, ka, fm, fa);
        if (rounds(p.tile, in.M, in.N, p.splits_main + p.splits_aux) > rounds(g.tile, in.M, in.N, g.splits)) bad("more rounds than the main launch alone", in.M, in.N, in.K, ka, fm, fa);
        const int floor_kt = std::max(std::min(4, in.kt_total), g.kt_per_split);
        if (kt < floor_kt) bad("a slice shorter than four k tiles or than the main launch's slices today", in.M, in.N, in.K, ka, fm, fa);
        if (kt > floor_kt) {   // the smallest such kt: one less would need another round
            const int c = kt - 1;
            if (rounds(p.tile, in.M, in.N, (in.kt_total + c - 1) / c + (kta + c - 1) / c) <= rounds(g.tile, in.M, in.N, g.splits)) bad("kt is not the smallest", in.M, in.N, in.K, ka, fm, fa);
        }
    }
    return p;
}

int main() {
    try {
        GemmTuning t;
        t.load_builtin();
        const GemmPlanOpts o;
        // the batch-1 model's transformer tails (two CFG samples): (rows, C); main K = 4 C, auxiliary K = C
        static const int kPairs[4][2] = {{8192, 320}, {2048, 640}, {512, 1280}, {128, 1280}};
        for (const auto& s : kPairs) {
            const GemmPlanIn in = linear_in(s[0], s[1], 4 * s[1]);
            const int ka = s[1];
            char key[80];
            std::snprintf(key, sizeof key, "%d,%d,%d+%d", in.M, in.N, in.K, ka);
            const bool row = t.pairs.count(key) != 0;
            const GemmPlan g = plan_gemm(in, o, t);
            if (g.tile.family != kFamP || g.splits <= 1) bad("mlp_lin is not a split plane launch today", in.M, in.N, in.K, ka, 0, 0);
            const GemmPairPlan p = check(in, ka, o, t, 0, 0, row);
            if (row && (t.pairs[key].splits > 0) != p.pair) bad("the table row was not honoured", in.M, in.N, in.K, ka, 0, 0);
            if (row && p.pair && (p.kt_per_split != std::min(t.pairs[key].splits, in.kt_total) || p.cfg != t.pairs[key].cfg)) bad("the table row's kt / tile", in.M, in.N, in.K, ka, 0, 0);
            if (p.pair)
                std::printf("pair %s cfg=%d kt=%d main=%d aux=%d rounds=%lld/%lld%s\n", key, p.cfg, p.kt_per_split, p.splits_main, p.splits_aux,
                            rounds(p.tile, in.M, in.N, p.splits_main + p.splits_aux), rounds(g.tile, in.M, in.N, g.splits), row ? " (table)" : "");
            else
                std::printf("pair %s none (mlp_lin cfg=%d splits=%d)%s\n", key, g.cfg, g.splits, row ? " (table)" : "");
            // without its row the shape is planned: every promise holds and it pairs (mlp_lin is split at every level)
            GemmTuning t0 = t;
            t0.pairs.erase(key);
            if (!check(in, ka, o, t0, 0, 0, false).pair) bad("the planner does not pair a model tail", in.M, in.N, in.K, ka, 0, 0);
            // "do not pair" and a measured kt, from the table
            GemmTuning t2 = t;
            t2.pairs[key] = TileChoice{g.cfg, 0};
            ++g_cases;
            if (plan_gemm_pair(in, ka, ka / 32, o, t2).pair) bad("a 0 row paired", in.M, in.N, in.K, ka, 0, 0);
            t2.set(std::string(key) + "=" + std::to_string(g.cfg) + ",7", false);
            const GemmPairPlan p7 = check(in, ka, o, t2, 0, 0, true);
            if (!p7.pair || p7.kt_per_split != 7 || p7.cfg != g.cfg) bad("a table row with kt 7 was not taken", in.M, in.N, in.K, ka, 0, 0);
        }
        // sweep of Linear mains: planned and forced
        for (int M : {1, 8, 32, 100, 128, 300, 512, 2048, 8192, 32768})
            for (int N : {32, 96, 160, 320, 640, 1280})
                for (int K : {128, 640, 1280, 5120})
                    for (int ka : {32, 160, 320, 1280}) {
                        const GemmPlanIn in = linear_in(M, N, K);
                        char key[80];
                        std::snprintf(key, sizeof key, "%d,%d,%d+%d", M, N, K, ka);
                        const bool row = t.pairs.count(key) != 0;
                        check(in, ka, o, t, 0, 0, row);
                        for (int fm : {1, 2, 3, 1000})
                            for (int fa : {1, 2, 1000}) check(in, ka, o, t, fm, fa, false);
                        for (int tile : {300, 304, 305, 307}) {   // option gemm_tile
                            GemmPlanOpts of;
                            of.force_tile = tile;
                            const GemmPairPlan p = check(in, ka, of, t, 3, 1, false);
                            if (p.pair && p.cfg != tile) bad("the forced tile was not taken", M, N, K, ka, 3, 1);
                        }
                    }
        // what must not pair: bf16 storage, fp32 input (no planes)
        {
            GemmPlanIn in = linear_in(2048, 640, 2560);
            ++g_cases;
            in.from_planes = false;
            if (plan_gemm_pair(in, 640, 20, o, t).pair) bad("paired without activation planes", in.M, in.N, in.K, 640, 0, 0);
            in.from_planes = true; in.bf16 = 1;
            if (plan_gemm_pair(in, 640, 20, o, t).pair) bad("paired a bf16 launch", in.M, in.N, in.K, 640, 0, 0);
        }
    } catch (const Error& e) {
        std::fprintf(stderr, "sdmi::Error %d: %s\n", e.status, e.what());
        return 2;
    }
    std::printf("%d cases, %d bad\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
