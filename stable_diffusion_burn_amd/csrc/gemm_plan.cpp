// gemm_plan.cpp -- tile / split-K choice of every GEMM launch (see gemm_plan.hpp).  Host-only.
#include "gemm_plan.hpp"

#include <algorithm>
#include <cstdio>

#include "error.hpp"

namespace sdmi {

// tuning/gfx950_{fp32,fp32_mfma,fp32_planes,bf16}.txt as build.py compiles them in; a row without a key ends a table
struct TuneRow { const char* key; int cfg, splits; };
static const TuneRow kTuneRows[] = {
#include "tuning_table.inc"
    {nullptr, 0, 0},
#include "tuning_table_mfma.inc"
    {nullptr, 0, 0},
#include "tuning_table_planes.inc"
    {nullptr, 0, 0},
#include "tuning_table_bf16.inc"
    {nullptr, 0, 0}};

// tuning/gfx950_fp32_pairs.txt: "M,N,Kmain+Kaux" -> (cfg, k tiles per slice)
static const TuneRow kPairRows[] = {
#include "tuning_table_pairs.inc"
    {nullptr, 0, 0}};

// tuning/gfx950_fp32_phases.txt: the phase shape "M/4,N,4Cin" of an up-convolution -> (plane tile, split count; 0 = keep the K = 9 Cin launch)
static const TuneRow kPhaseRows[] = {
#include "tuning_table_phases.inc"
    {nullptr, 0, 0}};

// ---- cost model of the five MFMA families ------------------------------------------------------------------------------
// Cycles per CU: (rounds of workgroups on 256 CUs) x (k loop of one workgroup / tile efficiency + per-workgroup overhead)
// + split-K reduce launch and slab traffic.  A k tile of a bm x bn block is bm * bn * flop / rate cycles: fp32 MFMA 32 * 2 flop at
// 256 flop/clk/CU; bf16 64 * 2 at 4096; the three-plane kernels six bf16 MFMAs per 16x16x32 block = 384 at 4096.  The efficiencies are
// measured ones (tools/autotune.py).  The overhead is the prologue and epilogue of a workgroup: a constant for the 4-wave kernels (two
// workgroups per CU hide each other's), DMA prologue latency + the output tile's store for the 8-wave ones (one workgroup per CU).
// Choices are made by `t < best` on doubles: the shape of the expression below is pinned by tests/golden/gemm_plan_choices.txt.
// n: tiles considered (the kernel-row tiles of k_gemm_bf16t.hip are an upgrade, not a choice); flop, rate: per k-tile element;
// overhead per workgroup = wg + bm * bn * area_num / area_den
struct CostRow { int bf16; GemmFamily family; int n; double eff[kNumGemmTiles]; double flop, rate, wg, area_num, area_den; };
static const CostRow kCost[] = {
    {0, kFam4, kNumGemmTiles, {0.85, 0.75, 0.60, 0.90, 0.75, 0.85, 0.75, 0.85, 0.65, 0.75}, 64.0, 256.0, 3000.0, 0.0, 1.0},
    {0, kFamX, kNumGemmTilesX, {0.90, 0.90, 0.88, 0.90}, 64.0, 256.0, 8000.0, 4.0, 10.0},
    {0, kFamS, kNumGemmTilesS, {0.55, 0.55, 0.52, 0.52, 0.46, 0.44}, 384.0, 4096.0, 8000.0, 4.0, 10.0},
    {0, kFamP, kNumGemmTilesP, {0.62, 0.60, 0.60, 0.52, 0.50, 0.34, 0.40, 0.50, 0.40}, 384.0, 4096.0, 8000.0, 4.0, 10.0},
    {1, kFam4, kNumGemmTiles, {0.31, 0.22, 0.16, 0.22, 0.20, 0.20, 0.22, 0.26, 0.15, 0.28}, 128.0, 4096.0, 3000.0, 0.0, 1.0},
    {1, kFamX, kNumGemmTilesX, {0.54, 0.46, 0.38, 0.48}, 128.0, 4096.0, 6000.0, 2.0, 20.0}};
static const int kSplitOpts[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48};

// the cheapest (tile, split count) among the families of `families` (bit per GemmFamily); pairs_only: tiles with geglu_pairs; phases: the launch holds that many
// problems of the shape, each with its own M tiles (plan_ups_phase)
static TileChoice cost_model(int bf16, unsigned families, int M, int N, int kt_total, bool pairs_only, int phases = 1) {
    const int n_cu = 256;
    double best = 1e300;
    TileChoice bc{0, 1};
    for (const CostRow& r : kCost) {
        if (r.bf16 != bf16 || !(families >> r.family & 1)) continue;
        for (int c = 0; c < r.n; ++c) {
            const GemmTileInfo& ti = kGemmFamilies[r.family].tiles[c];
            if (pairs_only && !ti.geglu_pairs) continue;
            const int bm = ti.bm, bn = ti.bn;
            const long long tiles = (long long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) * phases;
            const double overhead = r.wg + bm * bn * r.area_num / r.area_den;
            for (int s : kSplitOpts) {
                if (s > 1 && kt_total / s < 4) break;
                const int kt_per = (kt_total + s - 1) / s;
                const long long wgs = tiles * ((kt_total + kt_per - 1) / kt_per);
                const double per_cu = (double)((wgs + n_cu - 1) / n_cu);
                double t = per_cu * ((double)bm * bn * kt_per * r.flop / r.rate / r.eff[c] + overhead);
                if (s > 1) t += 8000.0 + (double)M * phases * N * 4.0 * (s + 1) / (5.0e12 / 2.4e9);  // reduce launch + slab traffic
                if (t < best) { best = t; bc = {kGemmFamilies[r.family].base + c, s}; }
            }
        }
    }
    return bc;
}

// at most kt_total slices, none of them empty
static int clamp_splits(int splits, int kt_total, int* kt_per_split) {
    splits = std::max(1, std::min(splits, kt_total));
    *kt_per_split = (kt_total + splits - 1) / splits;
    return (kt_total + *kt_per_split - 1) / *kt_per_split;
}

static const TileChoice* find(const std::map<std::string, TileChoice>& m, const char* key) {
    const auto it = m.find(key);
    return it == m.end() ? nullptr : &it->second;
}

// the plane tile of a shape whose activations arrive as planes: measured, else modelled; pairs_only as cost_model
static TileChoice plane_choice(const GemmTuning& t, const char* key, int M, int N, int kt_total, bool pairs_only) {
    if (const TileChoice* tc = find(t.planes, key)) {
        const GemmTileId id = gemm_tile_id(tc->cfg);
        if (!(pairs_only && id.family == kFamP && id.in_range(false) && !id.info().geglu_pairs)) return *tc;
    }
    return cost_model(0, 1u << kFamP, M, N, kt_total, pairs_only);
}

void GemmTuning::load_builtin() {
    std::map<std::string, TileChoice>* const tables[] = {&f32, &mfma, &planes, &bf16};
    int t = 0;
    for (const TuneRow& r : kTuneRows)
        if (r.key) (*tables[t])[r.key] = TileChoice{r.cfg, r.splits};
        else ++t;
    for (const TuneRow& r : kPairRows)
        if (r.key) pairs[r.key] = TileChoice{r.cfg, r.splits};
    for (const TuneRow& r : kPhaseRows)
        if (r.key) phases[r.key] = TileChoice{r.cfg, r.splits};
}

void GemmTuning::set(const std::string& value, bool b16) {
    const size_t eq = value.find('=');
    if (eq == std::string::npos) throw Error(SDMI_ERR_INVALID, "tune expects M,N,K=cfg,splits");
    TileChoice tc{0, 1};
    if (!b16 && value.find('+') < eq) {   // a pair row: plane tiles, k tiles per slice (0: do not pair)
        if (std::sscanf(value.c_str() + eq + 1, "%d,%d", &tc.cfg, &tc.splits) != 2 || tc.splits < 0 || gemm_tile_id(tc.cfg).family != kFamP || !gemm_tile_id(tc.cfg).in_range(false))
            throw Error(SDMI_ERR_INVALID, "tune: a pair row is M,N,Kmain+Kaux=cfg,kt_per_split with a plane tile (300 + x)");
        pairs[value.substr(0, eq)] = tc;
        return;
    }
    if (!b16 && value.compare(0, 3, "ph:") == 0) {   // a row of the phase table (plan_ups_phase): the phase shape, a plane tile, splits = 0: decline the shape
        if (std::sscanf(value.c_str() + eq + 1, "%d,%d", &tc.cfg, &tc.splits) != 2 || tc.splits < 0 || gemm_tile_id(tc.cfg).family != kFamP || !gemm_tile_id(tc.cfg).in_range(false))
            throw Error(SDMI_ERR_INVALID, "tune: a phase row is ph:M/4,N,4Cin=cfg,splits with a plane tile (300 + x)");
        phases[value.substr(3, eq - 3)] = tc;
        return;
    }
    if (std::sscanf(value.c_str() + eq + 1, "%d,%d", &tc.cfg, &tc.splits) != 2 || tc.cfg < 0 || tc.splits < 1 || !gemm_tile_id(tc.cfg).in_range(b16))
        throw Error(SDMI_ERR_INVALID, "tune: bad value");
    // plane tiles have their own table: what a GEMM whose input arrives as planes chooses from
    (b16 ? bf16 : (gemm_tile_id(tc.cfg).family == kFamP ? planes : f32))[value.substr(0, eq)] = tc;
}

GemmPlan plan_gemm(const GemmPlanIn& in, const GemmPlanOpts& o, const GemmTuning& t) {
    if (in.from_planes && !in.p_ok)
        throw Error(in.s_ok ? SDMI_ERR_UNSUPPORTED : SDMI_ERR_STATE,
                    in.s_ok ? "fp32 GEMM: an activation tensor stored as bf16 planes (6 bytes per element) reaches 4 GiB (32-bit piece offsets): lower the batch (at 64x64x960 the CFG "
                              "batch 2n must stay <= 182) or set option gemm_planes=0"
                            : "gemm: activation planes given for a layer the plane kernel does not take");
    // does the family's kernel take this layer / may it be chosen for it?  (4-wave kernels and bf16 storage: every layer)
    auto applicable = [&](int f) { return f == kFam4 || in.bf16 || (f == kFamP ? in.p_ok : f == kFamS ? in.s_ok : in.x32_ok); };
    auto enabled = [&](int f) { return f == kFam4 || (in.bf16 ? o.gemm_bf16x != 0 : f == kFamX ? o.gemm_x32 != 0 : f == kFamS ? o.gemm_f32s != 0 : true); };
    auto usable = [&](const TileChoice* tc) { return tc && applicable(gemm_tile_id(tc->cfg).family) && enabled(gemm_tile_id(tc->cfg).family); };
    char key[64];
    std::snprintf(key, sizeof key, "%d,%d,%d", in.M, in.N, in.K);
    // 1. measured tables (per storage type; then the one measured without the split kernels), else the cost model
    const TileChoice* const t1 = find(in.bf16 ? t.bf16 : t.f32, key);
    const TileChoice* const t2 = in.bf16 ? nullptr : find(t.mfma, key);
    TileChoice tc;
    if (in.from_planes) tc = plane_choice(t, key, in.M, in.N, in.kt_total, in.geglu != 0);
    else if (usable(t1)) tc = *t1;
    else if (usable(t2)) tc = *t2;
    else {
        unsigned fams = 0;
        for (int f : {kFam4, kFamX, kFamS})
            if (applicable(f) && enabled(f)) fams |= 1u << f;
        tc = cost_model(in.bf16, fams, in.M, in.N, in.kt_total, false);
    }
    // 2. overrides: option gemm_tile (where the tile applies), option splitk, the caller.  A forced tile runs as it is (no step 5).
    bool tile_forced = false;
    if (o.force_tile >= 0 && (in.from_planes ? gemm_tile_id(o.force_tile).family == kFamP : applicable(gemm_tile_id(o.force_tile).family))) { tc.cfg = o.force_tile; tile_forced = true; }
    if (o.force_splits > 0) tc.splits = o.force_splits;
    if (in.force_cfg >= 0) { tc.cfg = in.force_cfg; tile_forced = true; }
    GemmTileId tile = gemm_tile_id(tc.cfg);
    // 3. gemm_planes = 2 (A/B switch, tests): every launch that chose a k_gemm3x.hip tile runs on the k_gemm3p.hip tile nearest in shape
    if (!in.bf16 && !in.from_planes && in.p_ok && o.gemm_planes == 2 && tile.family == kFamS && tile.in_range(false)) {
        const GemmTileId twin{kFamP, tile.info().p_twin};
        if (!in.geglu || twin.info().geglu_pairs) tile = twin;
    }
    if (in.from_planes && tile.family != kFamP) throw Error(SDMI_ERR_STATE, "gemm: activation planes need a plane tile (300 + x)");
    // 4. split count
    if (in.force_splits > 0) tc.splits = in.force_splits;
    if (!in.bf16 && in.out_mode == 2) tc.splits = 1;  // fp32 kernel emitting bf16: no split-K path
    GemmPlan g{};
    g.splits = clamp_splits(tc.splits, in.kt_total, &g.kt_per_split);
    // 5. bf16 3x3 / stride-1 convolutions on the 256 x 320 / 256 x 256 tiles: the form that stages a kernel row's activations once for its three taps
    if (in.bf16 && o.conv3_reuse && !tile_forced && tile.family == kFamX && tile.index < kNumGemmTilesT && conv_gemm_bf16t_supported(in, g.kt_per_split))
        tile.index += kNumGemmTilesX;
    if (tile.family != kFam4 && (!tile.in_range(in.bf16) || !applicable(tile.family)))
        throw Error(SDMI_ERR_INVALID, "gemm: large-tile kernel index out of range or not applicable to this layer");
    g.tile = tile; g.cfg = tile.cfg(); g.tile_forced = tile_forced;
    return g;
}

GemmPairPlan plan_gemm_pair(const GemmPlanIn& main, int k_aux, int kt_aux, const GemmPlanOpts& o, const GemmTuning& t, int force_main, int force_aux) {
    GemmPairPlan pp{};
    if (main.bf16 || !main.from_planes || main.geglu || main.out_mode != 0 || kt_aux <= 0 || main.kt_total <= 0) return pp;
    const GemmPlan g = plan_gemm(main, o, t);
    if (g.tile.family != kFamP) return pp;
    pp.tile = g.tile; pp.cfg = g.cfg;
    const int ktm = main.kt_total;
    auto slices = [](int kt_total, int kt) { return (kt_total + kt - 1) / kt; };
    int kt = 0;
    if (force_main > 0 || force_aux > 0) {
        const int sm = std::max(1, std::min(force_main, ktm)), sa = std::max(1, std::min(force_aux, kt_aux));
        kt = std::max(slices(ktm, sm), slices(kt_aux, sa));
    } else {
        char key[80];
        std::snprintf(key, sizeof key, "%d,%d,%d+%d", main.M, main.N, main.K, k_aux);
        const TileChoice* const row = g.tile_forced ? nullptr : find(t.pairs, key);
        if (row) {
            if (row->splits <= 0) return pp;
            const GemmTileId id = gemm_tile_id(row->cfg);
            if (id.family != kFamP || !id.in_range(false)) throw Error(SDMI_ERR_INVALID, "pairs table: not a plane tile");
            pp.tile = id; pp.cfg = id.cfg();
            kt = std::min(row->splits, std::max(ktm, kt_aux));
        } else {
            if (g.splits <= 1) return pp;
            const GemmTileInfo& ti = g.tile.info();
            const long long tiles = (long long)((main.M + ti.bm - 1) / ti.bm) * ((main.N + ti.bn - 1) / ti.bn);
            const long long rounds_today = (tiles * g.splits + 255) / 256;
            // never finer than the main launch is cut today: that count is the measured (or modelled) balance of k-loop length against slab traffic
            for (int c = std::max(std::min(4, ktm), g.kt_per_split); c <= ktm; ++c)
                if ((tiles * (slices(ktm, c) + slices(kt_aux, c)) + 255) / 256 <= rounds_today) { kt = c; break; }
            if (!kt) return pp;
        }
    }
    pp.kt_per_split = kt;
    pp.splits_main = slices(ktm, kt);
    pp.splits_aux = slices(kt_aux, kt);
    pp.pair = true;
    return pp;
}

UpsPhasePlan plan_ups_phase(const GemmPlanIn& layer, bool fold_fresh, int ups_phase, const GemmPlanOpts& o, const GemmTuning& t) {
    UpsPhasePlan pp{};
    if (ups_phase == 0 || !fold_fresh) return pp;
    if (layer.bf16 || layer.geglu || layer.out_mode != 0 || layer.KH != 3 || layer.KW != 3 || layer.stride != 1 || layer.pad != 1 || layer.ups != 1) return pp;
    if (!layer.p_ok || !o.gemm_planes || !o.gemm_f32s || layer.Cin % 32 || layer.Ho != 2 * layer.Hs || layer.Wo != 2 * layer.Ws || layer.M % 4) return pp;
    const int forced = layer.force_cfg >= 0 ? layer.force_cfg : o.force_tile;
    if (forced >= 0 && gemm_tile_id(forced).family != kFamP) return pp;
    if (ups_phase != 1 && (!layer.from_planes || forced >= 0)) return pp;
    pp.M = layer.M / 4; pp.K = 4 * layer.Cin; pp.kt_total = layer.Cin / 8;
    char key[64];
    std::snprintf(key, sizeof key, "%d,%d,%d", pp.M, layer.N, pp.K);
    TileChoice tc;
    if (const TileChoice* row = find(t.phases, key)) {
        if (row->splits <= 0 && ups_phase != 1) return pp;
        tc = *row;
        if (tc.splits <= 0) tc.splits = 1;
    } else {
        if (ups_phase != 1 && pp.M < kUpsPhaseMinRows) return pp;
        tc = cost_model(0, 1u << kFamP, pp.M, layer.N, pp.kt_total, false, 4);
    }
    if (forced >= 0) tc.cfg = forced;
    if (o.force_splits > 0) tc.splits = o.force_splits;
    if (layer.force_splits > 0) tc.splits = layer.force_splits;
    const GemmTileId tile = gemm_tile_id(tc.cfg);
    if (tile.family != kFamP || !tile.in_range(false)) throw Error(SDMI_ERR_INVALID, "gemm: a phase launch needs a plane tile (300 + x)");
    pp.tile = tile; pp.cfg = tile.cfg();
    pp.splits = clamp_splits(tc.splits, pp.kt_total, &pp.kt_per_split);
    pp.take = true;
    return pp;
}

// Rounds of workgroups on 256 CUs x the time of one tile at the rate each tile shape sustains when the chip is full
// (tools/bench_gemm_fp8.py on MI355X: 256x320 2.4, 256x256 2.1, 256x128 1.7 PFLOP/s); K is split only when the tiles would
// leave half of the chip or more idle
TileChoice plan_gemm_fp8(int M, int N, int kt_total, int fp8_tile, int force_splits, int* kt_per_split) {
    static const double kRate[kNumGemmTilesQ] = {2400.0, 2100.0, 1700.0};
    if (fp8_tile >= kNumGemmTilesQ) throw Error(SDMI_ERR_INVALID, "fp8_tile out of range");
    double best = 1e300;
    TileChoice bc{fp8_tile, 1};
    for (int c = std::max(fp8_tile, 0); c < (fp8_tile < 0 ? kNumGemmTilesQ : fp8_tile + 1); ++c) {
        const int bm = kTilesQ[c].bm, bn = kTilesQ[c].bn;
        const long long tiles = (long long)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
        int s = 1;
        // (<= 128: half a round of tiles is split too: M = 8192, N = 1280 on 256 x 320 tiles is 128 workgroups; K = 11520: 167.5 -> 143.0 us, K = 23040: 314 -> 240, profiles/r06q_fp8_shapes.txt)
        if (tiles <= 128) s = (int)std::max<long long>(1, std::min<long long>(kt_total / 4, (256 + tiles - 1) / tiles));
        const double rounds = (double)((tiles * s + 255) / 256);
        const double t = rounds * (double)bm * bn / kRate[c] / s + (s > 1 ? 0.15 * (double)bm * bn / kRate[c] : 0.0);
        if (t < best) { best = t; bc = {c, s}; }
    }
    if (force_splits > 0) bc.splits = force_splits;
    bc.splits = clamp_splits(bc.splits, kt_total, kt_per_split);
    return bc;
}

// The tile is the one the unfused projection [rows, 2 hidden] would take (same tile count: 80 outputs = 160 weight rows per tile); it must
// run without split-K and have an even number of wave columns
int plan_geglu_plane_tile(long long rows, int hidden, int cin, const GemmPlanOpts& o, const GemmTuning& t) {
    char key[64];
    std::snprintf(key, sizeof key, "%lld,%d,%d", rows, 2 * hidden, cin);
    const TileChoice tc = plane_choice(t, key, (int)rows, 2 * hidden, (cin + 31) / 32, false);
    const bool forced = o.force_tile >= 0 && gemm_tile_id(o.force_tile).family == kFamP;
    const GemmTileId id = gemm_tile_id(forced ? o.force_tile : tc.cfg);
    const bool wave_cols = !id.in_range(false) || id.info().geglu_wave_cols;   // (an index out of range is plan_gemm's to report)
    return id.family == kFamP && wave_cols && (tc.splits == 1 || forced) && o.force_splits <= 1 ? id.cfg() : -1;
}

int plan_geglu_paired_tile(long long rows, int hidden, int fuse, bool f32s) {
    const long long mt = (rows + 255) / 256;
    const long long t256 = mt * ((hidden + 127) / 128), t128 = mt * ((hidden + 63) / 64);   // tiles with 256x256 / 256x128
    // measured (--opt geglu_fuse=0/1): at batch 1 the 256-wide tiles quantise badly against 256 CUs (320 tiles = two rounds) and the
    // fused form LOSES 2.6 % end to end in fp32; with >= 4 rounds it wins ~1 % (bf16, batch 8)
    int cfg = -1;
    if (t256 >= 1024 || fuse == 3) cfg = GemmTileId{kFamX, 1}.cfg();        // 256x256
    else if (t128 >= 1024 || fuse == 2) cfg = GemmTileId{kFamX, 2}.cfg();   // 256x128
    // precision = 0 with the split kernels: geglu_fuse = 4 / 5 / 6 force their tiles with geglu_pairs, 128x256s / 256x128s / 128x128s
    // (measured at batch 1: 3.56 / 3.58 / 3.54 img/s against 3.66 unfused)
    if (f32s && fuse >= 4 && fuse <= 6) cfg = GemmTileId{kFamS, fuse == 4 ? 3 : fuse == 5 ? 2 : 5}.cfg();
    return cfg;
}

}  // namespace sdmi
