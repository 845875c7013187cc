// ups_phase_plan_main.cpp -- runs the phase planner (csrc/gemm_plan.cpp plan_ups_phase, host-only) over the up-convolutions of the model at the headline size and at
// two other latent sizes, plus a sweep, and checks what it promises.  Built by tests/test_upsample_phase_cpu.py with plain g++ (no HIP) under
// -fsanitize=address,undefined.
//
//   ups_phase_plan       one line per model layer and option value ("phase <mode> NB,C,Hs,Ws take cfg=.. splits=.. kt=.. tiles=.." or "... decline"), then
//                        "<n> cases, <bad> bad"; exit 1 when a promise is broken (the first ones on stderr)
//
// Promises.  A taken plan: a plane tile; the phase shape (M / 4 rows, K = 4 Cin, Cin / 8 k tiles); no K slice is empty and the slices cover every k tile once;
// the M tiles are counted per phase (4 x ceil(M / 4 / bm)), so none straddles two phases.  Declined ("today's plan": the engine then runs plan_gemm, which this
// planner does not touch): ups_phase = 0, a stale fold, a forced tile of another family, gemm_planes = 0, gemm_f32s = 0, a layer that is not an up-convolution; with
// ups_phase = 2 also: fp32 input, any forced tile, fewer than kUpsPhaseMinRows rows per phase, a "0" row of the table.  ups_phase = 1 honours a forced plane tile
// and a forced split count (clamped to the k tiles).
#include <algorithm>
#include <cstdio>
#include <string>

#include "../../stable_diffusion_burn_amd/csrc/error.hpp"
#include "../../stable_diffusion_burn_amd/csrc/gemm_plan.hpp"

using namespace sdmi;

static int g_cases = 0, g_bad = 0;

static void bad(const char* what, int nb, int c, int hs, int ws) {
    if (++g_bad <= 10) std::fprintf(stderr, "BROKEN: %s at NB=%d C=%d Hs=%d Ws=%d\n", what, nb, c, hs, ws);
}

// the 3x3 convolution of an Upsample layer, C -> C channels, over the nearest-2x of an [nb, hs, ws] source; activations as planes
static GemmPlanIn up_in(int nb, int c, int hs, int ws) {
    GemmPlanIn in{};
    in.M = nb * 2 * hs * 2 * ws; in.N = c; in.K = 9 * c; in.kt_total = in.K / 32;
    in.x32_ok = in.s_ok = in.p_ok = in.from_planes = true;
    in.KH = in.KW = 3; in.stride = 1; in.pad = 1; in.ups = 1; in.Cin = c; in.Hs = hs; in.Ws = ws; in.Ho = 2 * hs; in.Wo = 2 * ws;
    in.zero_page = true;
    return in;
}

static UpsPhasePlan check(const GemmPlanIn& in, int nb, bool fresh, int mode, const GemmPlanOpts& o, const GemmTuning& t) {
    ++g_cases;
    const UpsPhasePlan p = plan_ups_phase(in, fresh, mode, o, t);
    const int c = in.Cin, hs = in.Hs, ws = in.Ws;
    if (!p.take) return p;
    if (mode == 0) bad("taken with ups_phase = 0", nb, c, hs, ws);
    if (!fresh) bad("taken with a stale fold", nb, c, hs, ws);
    if (p.tile.family != kFamP || !p.tile.in_range(false) || p.cfg != p.tile.cfg()) { bad("not a plane tile", nb, c, hs, ws); return p; }
    if (p.M != nb * hs * ws || p.K != 4 * c || p.kt_total != c / 8) bad("not the phase shape", nb, c, hs, ws);
    const int kt = p.kt_per_split;
    if (kt < 1 || p.splits < 1) { bad("kt_per_split / splits < 1", nb, c, hs, ws); return p; }
    if (p.splits != (p.kt_total + kt - 1) / kt) bad("the slices do not cover the k tiles once", nb, c, hs, ws);
    if ((p.splits - 1) * kt >= p.kt_total) bad("an empty K slice", nb, c, hs, ws);
    return p;
}

// M tiles of a taken plan: ceil(rows of a phase / bm) per phase -- tile t belongs to phase t / per_phase and starts at row (t % per_phase) bm of it
static long long m_tiles(const UpsPhasePlan& p) {
    const int bm = p.tile.info().bm;
    const long long per_phase = (p.M + bm - 1) / bm;
    for (long long t = 0; t < 4 * per_phase; ++t) {
        const long long ph = t / per_phase, m0 = (t - ph * per_phase) * bm;
        if (ph > 3 || m0 >= p.M) return -1;      // a tile past the four phases, or one that starts beyond its phase's rows
    }
    return 4 * per_phase;
}

int main() {
    try {
        GemmTuning t;
        t.load_builtin();
        const GemmPlanOpts o;
        // (NB, C, Hs, Ws): UNet 8->16, 16->32, 32->64 (two CFG samples) and VAE 64->128, 128->256, 256->512 at the 64 x 64 latent; then at 72 x 88 and 40 x 40
        static const int kLayers[18][4] = {{2, 1280, 8, 8},  {2, 1280, 16, 16}, {2, 640, 32, 32}, {1, 512, 64, 64}, {1, 512, 128, 128}, {1, 256, 256, 256},
                                           {2, 1280, 9, 11}, {2, 1280, 18, 22}, {2, 640, 36, 44}, {1, 512, 72, 88}, {1, 512, 144, 176}, {1, 256, 288, 352},
                                           {2, 1280, 5, 5},  {2, 1280, 10, 10}, {2, 640, 20, 20}, {1, 512, 40, 40}, {1, 512, 80, 80},   {1, 256, 160, 160}};
        for (const auto& s : kLayers) {
            const GemmPlanIn in = up_in(s[0], s[1], s[2], s[3]);
            for (int mode : {2, 1}) {
                const UpsPhasePlan p = check(in, s[0], true, mode, o, t);
                if (mode == 1 && !p.take) bad("ups_phase = 1 declined a supported layer", s[0], s[1], s[2], s[3]);
                if (p.take) {
                    const long long mt = m_tiles(p);
                    if (mt < 0) bad("an M tile straddles two phases", s[0], s[1], s[2], s[3]);
                    std::printf("phase %d %d,%d,%d,%d take cfg=%d splits=%d kt=%d tiles=%lld\n", mode, s[0], s[1], s[2], s[3], p.cfg, p.splits, p.kt_per_split,
                                mt * ((in.N + p.tile.info().bn - 1) / p.tile.info().bn));
                } else
                    std::printf("phase %d %d,%d,%d,%d decline\n", mode, s[0], s[1], s[2], s[3]);
            }
            // today's plan: the A/B arm, a stale fold, forced tiles of the other families, the plane kernels switched off, fp32 input under the default
            if (check(in, s[0], true, 0, o, t).take) bad("ups_phase = 0", s[0], s[1], s[2], s[3]);
            for (int mode : {1, 2}) {
                if (check(in, s[0], false, mode, o, t).take) bad("a stale fold", s[0], s[1], s[2], s[3]);
                for (int tile : {0, 5, 100, 103, 200, 205}) {
                    GemmPlanOpts of;
                    of.force_tile = tile;
                    if (check(in, s[0], true, mode, of, t).take) bad("a forced non-plane tile", s[0], s[1], s[2], s[3]);
                }
                GemmPlanOpts op; op.gemm_planes = 0;
                if (check(in, s[0], true, mode, op, t).take) bad("gemm_planes = 0", s[0], s[1], s[2], s[3]);
                GemmPlanOpts os; os.gemm_f32s = 0;
                if (check(in, s[0], true, mode, os, t).take) bad("gemm_f32s = 0", s[0], s[1], s[2], s[3]);
            }
            GemmPlanIn f32 = in;
            f32.from_planes = false;
            if (check(f32, s[0], true, 2, o, t).take) bad("ups_phase = 2 took an fp32 input", s[0], s[1], s[2], s[3]);
            // forced plane tiles / split counts: honoured by ups_phase = 1, a reason to decline for ups_phase = 2
            for (int tile = 300; tile <= 308; ++tile)
                for (int sk : {0, 1, 2, 3, 7, 1000}) {
                    GemmPlanOpts of;
                    of.force_tile = tile; of.force_splits = sk;
                    if (check(in, s[0], true, 2, of, t).take) bad("ups_phase = 2 took a forced tile", s[0], s[1], s[2], s[3]);
                    const UpsPhasePlan p = check(in, s[0], true, 1, of, t);
                    if (!p.take || p.cfg != tile) bad("ups_phase = 1: the forced plane tile was not taken", s[0], s[1], s[2], s[3]);
                    if (p.take && sk > 0) {
                        const int want = std::max(1, std::min(sk, p.kt_total)), per = (p.kt_total + want - 1) / want;
                        if (p.kt_per_split != per || p.splits > want) bad("ups_phase = 1: the forced split count", s[0], s[1], s[2], s[3]);
                    }
                    if (p.take && m_tiles(p) < 0) bad("an M tile straddles two phases", s[0], s[1], s[2], s[3]);
                }
            // a "0" row declines under the default and a measured row is taken as written
            {
                const std::string key = "ph:" + std::to_string(in.M / 4) + "," + std::to_string(in.N) + "," + std::to_string(4 * in.Cin);
                GemmTuning t2 = t;
                t2.set(key + "=304,0", false);
                if (check(in, s[0], true, 2, o, t2).take) bad("a 0 row was taken", s[0], s[1], s[2], s[3]);
                t2.set(key + "=304,2", false);
                const UpsPhasePlan p = check(in, s[0], true, 2, o, t2);
                if (!p.take || p.cfg != 304 || p.splits != 2) bad("a measured row was not taken as written", s[0], s[1], s[2], s[3]);
            }
        }
        // fewer than kUpsPhaseMinRows rows per phase: taken by default only where the table holds a measured row (the headline's 8 -> 16 level)
        for (const auto& s : kLayers) {
            const GemmPlanIn in = up_in(s[0], s[1], s[2], s[3]);
            const std::string key = std::to_string(in.M / 4) + "," + std::to_string(in.N) + "," + std::to_string(4 * in.Cin);
            ++g_cases;
            if (in.M / 4 < kUpsPhaseMinRows && !t.phases.count(key) && plan_ups_phase(in, true, 2, o, t).take) bad("a small level without a measured row was taken by default", s[0], s[1], s[2], s[3]);
            if (t.phases.count(key) && t.phases[key].splits > 0) {
                const UpsPhasePlan p = plan_ups_phase(in, true, 2, o, t);
                if (!p.take || p.cfg != t.phases[key].cfg || p.splits != t.phases[key].splits) bad("a built-in table row was not taken as written", s[0], s[1], s[2], s[3]);
            }
        }
        // sweep: odd sizes, one pixel, many rows
        for (int nb : {1, 2, 3})
            for (int c : {32, 64, 96, 160, 320, 1280})
                for (int hs : {1, 3, 5, 16, 33})
                    for (int ws : {1, 2, 7, 16, 40})
                        for (int mode : {1, 2}) {
                            const UpsPhasePlan p = check(up_in(nb, c, hs, ws), nb, true, mode, o, t);
                            if (p.take && m_tiles(p) < 0) bad("an M tile straddles two phases", nb, c, hs, ws);
                        }
        // not an up-convolution: no upsample, stride 2, 1x1, bf16 storage
        {
            GemmPlanIn in = up_in(2, 640, 32, 32);
            g_cases += 4;
            GemmPlanIn a = in; a.ups = 0;
            if (plan_ups_phase(a, true, 1, o, t).take) bad("ups = 0", 2, 640, 32, 32);
            a = in; a.stride = 2;
            if (plan_ups_phase(a, true, 1, o, t).take) bad("stride 2", 2, 640, 32, 32);
            a = in; a.KH = a.KW = 1; a.pad = 0;
            if (plan_ups_phase(a, true, 1, o, t).take) bad("1x1", 2, 640, 32, 32);
            a = in; a.bf16 = 1;
            if (plan_ups_phase(a, true, 1, o, t).take) bad("bf16", 2, 640, 32, 32);
        }
    } catch (const Error& e) {
        std::fprintf(stderr, "sdmi::Error %d: %s\n", e.status, e.what());
        return 2;
    }
    std::printf("%d cases, %d bad\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
