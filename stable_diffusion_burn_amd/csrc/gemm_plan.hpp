// gemm_plan.hpp -- which tile and how many K slices a GEMM launch gets: a pure function of the layer's shape, the options and
// the measured tables.  Host-only (no HIP, like error.hpp and tokenizer.cpp), so tests/test_gemm_plan_cpu.py replays it on a CPU.
// The K-reduction order, and with it the bits of the result, follows from this choice: see DESIGN.md "Determinism".
#pragma once
#include <map>
#include <string>

#include "gemm_tiles.hpp"

namespace sdmi {

struct TileChoice { int cfg; int splits; };

// what Engine::launch_gemm knows about a launch before it picks a kernel
struct GemmPlanIn {
    int M, N, K, kt_total;
    int bf16;          // storage type: 0 fp32, 1 bf16
    int geglu;         // ConvGemm::geglu
    int out_mode;      // ConvGemm::out_mode
    bool x32_ok, s_ok, p_ok;   // fp32: k_gemm2x.hip / k_gemm3x.hip / k_gemm3p.hip takes the layer (Engine::launch_gemm)
    bool from_planes;          // the activations arrive as planes
    int force_cfg = -1, force_splits = 0;   // the caller's choice (Engine::gemm_geglu)
    // the convolution, as conv_gemm_bf16t_supported reads it
    int KH, KW, stride, pad, ups, Cin, Hs, Ws, Ho, Wo;
    bool zero_page;
};

struct GemmPlanOpts {
    int force_tile = -1, force_splits = 0;   // options gemm_tile (-1 auto), splitk (0 auto)
    int gemm_x32 = 1;      // precision = 0: 1 = large-tile LDS-DMA fp32 GEMM (k_gemm2x.hip) where measured / modelled faster
    int gemm_f32s = 1;     // precision = 0: 1 = fp32 GEMMs on the bf16 matrix pipe (three-way operand split, k_gemm3x.hip) where faster
    int gemm_planes = 1;   // precision = 0: k_gemm3p.hip (activations as bf16 planes too, no split in the k loop): 0 never, 1 every launch that would take a k_gemm3x.hip tile,
                           // 2 = A/B switch (tests): every launch that chose a k_gemm3x.hip tile runs on the nearest k_gemm3p.hip tile, its fp32 input converted by split3_rows_kernel in front of it
    int gemm_bf16x = 1;    // precision = 1: 1 = large-tile LDS-DMA GEMM where the cost model prefers it; 0 = never
    int conv3_reuse = 1;   // precision >= 1: 1 = 3x3 / stride-1 convolutions that chose the 256 x 320 / 256 x 256 tile run on k_gemm_bf16t.hip (one staged activation tile per kernel row)
};

// measured per-shape choices, "M,N,K" -> (cfg, splits): tuning/gfx950_*.txt compiled in, then options tune / tune_bf16 / tune_clear
struct GemmTuning {
    std::map<std::string, TileChoice> f32;     // fp32 kernels
    std::map<std::string, TileChoice> mfma;    // fp32 shapes measured with the fp32-MFMA kernels only (gemm_f32s=0)
    std::map<std::string, TileChoice> planes;  // fp32 shapes whose activations arrive as planes: k_gemm3p.hip tiles only
    std::map<std::string, TileChoice> bf16;    // bf16 kernels
    void load_builtin();
    void set(const std::string& value, bool b16);   // "M,N,K=cfg,splits"
    void clear() { f32.clear(); mfma.clear(); planes.clear(); bf16.clear(); }
};

struct GemmPlan { GemmTileId tile; int cfg, splits, kt_per_split; bool tile_forced; };   // cfg = tile.cfg(); tile_forced: by option gemm_tile or by the caller

GemmPlan plan_gemm(const GemmPlanIn& in, const GemmPlanOpts& o, const GemmTuning& t);   // throws Error
// MXFP8 (k_fp8.hip): tile index (fp8_tile >= 0 forces it) and split count
TileChoice plan_gemm_fp8(int M, int N, int kt_total, int fp8_tile, int force_splits, int* kt_per_split);
// the plane tile the GEGLU projection [rows, 2 hidden] takes with the gate split by wave column in its epilogue, or -1 (unfused)
int plan_geglu_plane_tile(long long rows, int hidden, int cin, const GemmPlanOpts& o, const GemmTuning& t);
// the large tile for the GEGLU projection with paired fragments (option geglu_fuse = fuse), or -1; f32s: fp32 with weight planes and gemm_f32s
int plan_geglu_paired_tile(long long rows, int hidden, int fuse, bool f32s);

}  // namespace sdmi
