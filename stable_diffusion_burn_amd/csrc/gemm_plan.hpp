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
    // paired launches (plan_gemm_pair), "M,N,Kmain+Kaux" -> (cfg, k tiles per slice; 0 = do not pair): tuning/gfx950_fp32_pairs.txt.  TileChoice::splits holds the k tiles.
    std::map<std::string, TileChoice> pairs;
    void load_builtin();
    void set(const std::string& value, bool b16);   // "M,N,K=cfg,splits"; "M,N,Kmain+Kaux=cfg,kt_per_split" goes to pairs
    // phase launches of up-convolutions (plan_ups_phase), the PHASE shape "M/4,N,4Cin" -> (plane tile, splits; 0 = do not take): tuning/gfx950_fp32_phases.txt.  A map of
    // its own, so a phase shape cannot collide with a plain shape of `planes`; option tune writes it through the key "ph:M/4,N,4Cin"
    std::map<std::string, TileChoice> phases;
    void clear() { f32.clear(); mfma.clear(); planes.clear(); bf16.clear(); pairs.clear(); phases.clear(); }
};

struct GemmPlan { GemmTileId tile; int cfg, splits, kt_per_split; bool tile_forced; };   // cfg = tile.cfg(); tile_forced: by option gemm_tile or by the caller

GemmPlan plan_gemm(const GemmPlanIn& in, const GemmPlanOpts& o, const GemmTuning& t);   // throws Error

// A split-K plane launch that carries a second, 1x1 problem over the same rows and columns on extra slices (kernels.hpp, ConvGemm::z_aux): slices [0, splits_main) hold
// the main problem's k tiles, [splits_main, splits_main + splits_aux) the auxiliary one's, kt_per_split tiles each (the last of either may be short; none is empty).
struct GemmPairPlan { bool pair; GemmTileId tile; int cfg, kt_per_split, splits_main, splits_aux; };
// main: the launch as plan_gemm would see it alone (from_planes).  The tile is plan_gemm's.  kt_per_split is the smallest one -- not below the k tiles a slice of the main
// launch holds today (the measured or modelled balance of k-loop length against slab traffic), nor below four (the cost model's floor for a slice) -- with which
// tiles x (main + auxiliary slices) needs no more rounds of 256 workgroups than the main launch alone needs today: the auxiliary k tiles join a k loop that already
// runs and never add a round.  pair = false ("run the two launches"): the main launch is not on a plane tile or not split today (the reduce
// would be a new dependent phase), no such kt exists, or the pairs table says 0 for the shape.  A table row's cfg / kt are taken as measured.
// force_main / force_aux > 0 (tests, with option gemm_tile for the tile): requested slice counts.  Both problems share kt_per_split, so the request is met as
// kt = max(ceil(kt_main / force_main), ceil(kt_aux / force_aux)) and the counts that follow from it; it pairs whatever today's split count is.
GemmPairPlan plan_gemm_pair(const GemmPlanIn& main, int k_aux, int kt_aux, const GemmPlanOpts& o, const GemmTuning& t, int force_main = 0, int force_aux = 0);   // throws Error
// conv3x3(nearest_2x(x)) as four folded 2x2 phase convolutions in one plane launch (kernels.hpp, ConvGemm::phases).  `layer`: the up-convolution as plan_gemm would see
// it (M = NB 2Hs 2Ws rows, K = 9 Cin).  The phase shape is 4 x [M / 4, N, 4 Cin], kt = Cin / 8 k tiles; M, K, kt_per_split of the plan are the phase shape's.
// take = false ("run today's launch") when
//   * ups_phase = 0, the fold is not fresh, the layer is not 3x3 / stride 1 / pad 1 / ups 1 in fp32 with plain output, or the plane kernel does not take it (p_ok,
//     gemm_planes = 0, gemm_f32s = 0, a forced tile of another family);
//   * ups_phase = 2 (default) and: the activations do not arrive as planes, a tile is forced (option gemm_tile or the caller), the phase table says splits = 0 for
//     the shape, or -- without a row -- a phase has fewer than kUpsPhaseMinRows rows: one M tile per phase then streams the 16 Cin N folded weights where today's
//     launch streams 9 Cin N, and launches that small run at the weight stream's rate, not the matrix pipe's.
// ups_phase = 1 (tests): wherever supported; option gemm_tile = 30x and option splitk are honoured.
// Tile and split count: the phase table (GemmTuning::phases, keyed by the phase shape in a map of its own: no collision with a plain "M,N,K" row), else the cost model
// over the plane tiles with 4 x the M tiles.  No slice is empty (clamp as plan_gemm).
constexpr int kUpsPhaseMinRows = 256;
struct UpsPhasePlan { bool take; GemmTileId tile; int cfg, splits, kt_per_split, M, K, kt_total; };
UpsPhasePlan plan_ups_phase(const GemmPlanIn& layer, bool fold_fresh, int ups_phase, const GemmPlanOpts& o, const GemmTuning& t);
// MXFP8 (k_fp8.hip): tile index (fp8_tile >= 0 forces it) and split count
TileChoice plan_gemm_fp8(int M, int N, int kt_total, int fp8_tile, int force_splits, int* kt_per_split);
// the plane tile the GEGLU projection [rows, 2 hidden] takes with the gate split by wave column in its epilogue, or -1 (unfused)
int plan_geglu_plane_tile(long long rows, int hidden, int cin, const GemmPlanOpts& o, const GemmTuning& t);
// the large tile for the GEGLU projection with paired fragments (option geglu_fuse = fuse), or -1; f32s: fp32 with weight planes and gemm_f32s
int plan_geglu_paired_tile(long long rows, int hidden, int fuse, bool f32s);

}  // namespace sdmi
