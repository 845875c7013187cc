// gemm_tiles.hpp -- every tile of the GEMM kernel families in one table (host-only: no HIP include, so the planner and its
// CPU test build with a plain C++ compiler).  A tile is named outside the engine by one number, `cfg` (option gemm_tile,
// tuning/*.txt, the cfg= of dump_choices): the family's base + the index in the family's list.
#pragma once

namespace sdmi {

// BM x BN per workgroup; what the GEGLU epilogues and the gemm_planes=2 switch need to know about a tile
struct GemmTileInfo {
    int bm, bn;
    const char* name;
    bool geglu_pairs = false;      // GEGLU with value / gate in paired fragments (ConvGemm::geglu == 1): an even fragment count per wave
    bool geglu_wave_cols = false;  // GEGLU with value / gate split by wave column (geglu == 2): an even number of wave columns
    int p_twin = -1;               // k_gemm3x.hip tile: index of the k_gemm3p.hip tile nearest in shape
};

enum GemmFamily { kFam4 = 0, kFamX = 1, kFamS = 2, kFamP = 3, kNumGemmFamilies = 4 };

constexpr int kNumGemmTiles = 10, kNumGemmTilesX = 4, kNumGemmTilesT = 2, kNumGemmTilesS = 6, kNumGemmTilesP = 9, kNumGemmTilesQ = 3;
constexpr int kNumGemmTilesXB = kNumGemmTilesX + kNumGemmTilesT;   // bf16 large tiles as one list: k_gemm_bf16x.hip, then k_gemm_bf16t.hip

// 4-wave kernels, 256 threads (k_gemm2.hip fp32, k_gemm_bf16.hip)
inline constexpr GemmTileInfo kTiles4[kNumGemmTiles] = {
    {128, 128, "128x128"}, {128, 64, "128x64"},  // 0: wave 64x64; 1: wave 64x32
    {64, 64, "64x64"}, {256, 128, "256x128"},    // 2: wave 32x32; 3: wave 128x64
    {128, 80, "128x80"}, {256, 80, "256x80"},    // 4: wave 32x80 (N = 320 -> 4 column tiles); 5: wave 64x80
    {64, 128, "64x128"}, {128, 160, "128x160"},  // 6: wave 32x64; 7: wave 64x80 (2x2 waves)
    {64, 80, "64x80"}, {64, 160, "64x160"}};     // 8: wave 16x80 (M = 8192, N = 320 -> 512 tiles, no split-K); 9: wave 32x80 (2x2 waves)
// 8-wave LDS-DMA kernels (k_gemm2x.hip fp32, k_gemm_bf16x.hip); behind them the kernel-row tiles of k_gemm_bf16t.hip (bf16 only)
inline constexpr GemmTileInfo kTilesX[kNumGemmTilesXB] = {
    {256, 320, "256x320x"}, {256, 256, "256x256x"}, {256, 128, "256x128x"}, {128, 320, "128x320x"}, {256, 320, "256x320t"}, {256, 256, "256x256t"}};
// fp32 as three bf16 planes, weights only (k_gemm3x.hip)
inline constexpr GemmTileInfo kTilesS[kNumGemmTilesS] = {
    {256, 160, "256x160s", false, false, 0}, {128, 320, "128x320s", false, false, 3}, {256, 128, "256x128s", true, false, 1},
    {128, 256, "128x256s", true, false, 2},  {128, 160, "128x160s", false, false, 3}, {128, 128, "128x128s", true, false, 4}};
// ... activations as planes too (k_gemm3p.hip)
inline constexpr GemmTileInfo kTilesP[kNumGemmTilesP] = {
    {256, 160, "256x160p", false, true}, {256, 128, "256x128p", true, true}, {128, 256, "128x256p", true, true},
    {128, 160, "128x160p", false, true}, {128, 128, "128x128p", true, true}, {64, 64, "64x64p", true, true},
    {64, 128, "64x128p", true, true},    {64, 320, "64x320p", false, true},  {128, 64, "128x64p", true, false}};
// MXFP8 (k_fp8.hip): option fp8_tile, not part of the cfg numbering
inline constexpr GemmTileInfo kTilesQ[kNumGemmTilesQ] = {{256, 320, "256x320q"}, {256, 256, "256x256q"}, {256, 128, "256x128q"}};

// base: cfg of the family's tile 0; count: tiles by storage type (0 fp32, 1 bf16), 0 = the family has no kernel for it
struct GemmFamilyInfo { int base; int count[2]; const char* name; const GemmTileInfo* tiles; };
inline constexpr GemmFamilyInfo kGemmFamilies[kNumGemmFamilies] = {
    {0, {kNumGemmTiles, kNumGemmTiles}, "4-wave", kTiles4},
    {100, {kNumGemmTilesX, kNumGemmTilesXB}, "large", kTilesX},
    {200, {kNumGemmTilesS, 0}, "split", kTilesS},
    {300, {kNumGemmTilesP, 0}, "planes", kTilesP}};

// cfg <-> {family, index}: the one place that knows the numbering.  An index past the family's count decodes as it is (the caller reports it).
struct GemmTileId {
    int family, index;
    int cfg() const { return kGemmFamilies[family].base + index; }
    bool in_range(bool bf16) const { return index < kGemmFamilies[family].count[bf16]; }
    const GemmTileInfo& info() const { return kGemmFamilies[family].tiles[index]; }
};
inline GemmTileId gemm_tile_id(int cfg) {
    const int f = cfg >= kGemmFamilies[kFamP].base ? kFamP : cfg / 100;
    return {f, cfg - kGemmFamilies[f].base};
}

inline const GemmTileInfo& gemm_tile_info(int c) { return kTiles4[c]; }
inline const GemmTileInfo& gemm_tile_info_x(int c) { return kTilesX[c]; }
inline const GemmTileInfo& gemm_tile_info_t(int c) { return kTilesX[kNumGemmTilesX + c]; }

// what k_gemm_bf16t.hip takes: a 3x3 / stride-1 / pad-1 convolution without upsampling over images whose width is 16, 32, 64 or 128 and whose pixel count is a
// multiple of the 256-row tile (so a tile lies inside one image), bf16 storage, k slices of whole kernel rows, no GEGLU pairing.  P: ConvGemm or GemmPlanIn.
template <class P>
bool conv_gemm_bf16t_supported(const P& p, int kt_per_split) {
    if (p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad != 1 || p.ups != 0 || p.geglu) return false;
    if ((p.Cin % 64) || !p.zero_page) return false;
    if (p.Ws != 16 && p.Ws != 32 && p.Ws != 64 && p.Ws != 128) return false;
    if (p.Ho != p.Hs || p.Wo != p.Ws || (p.Hs * p.Ws) % 256 || p.M % 256) return false;
    return kt_per_split % 3 == 0;
}

}  // namespace sdmi
