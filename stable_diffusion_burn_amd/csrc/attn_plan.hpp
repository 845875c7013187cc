// attn_plan.hpp -- which kernel, which workgroup form and how many key slices an attention call gets: a pure function of the call's
// shape and the options.  Host-only (no HIP, like gemm_plan.hpp), so tests/test_attn_plan_cpu.py replays it on a CPU.
// The slice count fixes the order in which the fp32 kernels' partial results are merged, and with it the bits of the result: see
// DESIGN.md "Determinism".  The launchers (kernels.hpp) only map a plan to its template instantiation.
#pragma once

namespace sdmi {

enum class AttnKernel {
    Unfused,   // QK^T -> row softmax -> PV on the GEMM kernels, one (sample, head) at a time (the VAE's single 512-wide head)
    Flash,     // k_attn.hip: fp32 matrix instructions; fp32 storage, or bf16 storage widened when staged
    Split,     // k_attn_split.hip: fp32 storage on the bf16 matrix pipe, three-way split operands
    Bf16,      // k_attn_bf16.hip: bf16 storage, bf16 matrix instructions
};

// The geometry of every instantiated (kernel, head dim, query blocks per wave): query rows a wave owns and keys per K / V tile.  static_asserts in the three .hip
// files tie kv_tile to Attn2Cfg / AttnSpCfg / AttnBfCfg and rows_per_wave to the kernels' row mapping; their launchers refuse a plan made for another form.
struct AttnGeom { AttnKernel kernel; int d_head, qr, rows_per_wave, kv_tile; };
inline constexpr AttnGeom kAttnGeom[] = {
    {AttnKernel::Flash, 40, 1, 16, 64}, {AttnKernel::Flash, 64, 1, 16, 64}, {AttnKernel::Flash, 80, 1, 16, 64}, {AttnKernel::Flash, 160, 1, 16, 32},   // 64: CLIP (768 / 12)
    {AttnKernel::Split, 40, 1, 32, 64}, {AttnKernel::Split, 64, 1, 32, 64}, {AttnKernel::Split, 80, 1, 32, 64},   // 64: SD 2.x's UNet, behind option attn_d64
    {AttnKernel::Bf16, 40, 1, 32, 128}, {AttnKernel::Bf16, 40, 2, 64, 64},   // d = 40 is softmax-bound: fewer / longer iterations; with two query blocks per wave 64 keys fit the registers
    {AttnKernel::Bf16, 64, 1, 32, 64}, {AttnKernel::Bf16, 80, 1, 32, 64}, {AttnKernel::Bf16, 160, 1, 32, 64},     // 64: behind option attn_d64
};
constexpr const AttnGeom* attn_geom(AttnKernel k, int d_head, int qr = 1) {
    for (const AttnGeom& g : kAttnGeom)
        if (g.kernel == k && g.d_head == d_head && g.qr == qr) return &g;
    return nullptr;
}
// the head dims with a fused kernel (every one of them has a k_attn.hip instance) ...
constexpr bool attn_supported_head_dim(int d) { return attn_geom(AttnKernel::Flash, d) != nullptr; }
// ... and those k_attn_bf16.hip serves.  Bf16 q tensors of these head dims arrive multiplied by attn_bf16_q_scale (kernels.hpp), whichever kernel runs.
// d = 64 has instances of k_attn_split.hip and k_attn_bf16.hip that only option attn_d64 opens (AttnPlanOpts): without it d = 64 is what it was before they existed,
// k_attn.hip at every precision and no pre-scaled query.
constexpr bool attn_bf16_head_dim(int d, int attn_d64 = 0) { return attn_geom(AttnKernel::Bf16, d) != nullptr && (d != 64 || attn_d64); }
constexpr bool attn_split_head_dim(int d, int attn_d64 = 0) { return attn_geom(AttnKernel::Split, d) != nullptr && (d != 64 || attn_d64); }

struct AttnPlanIn {
    int n, n_head, nq;
    int nk;              // the padded key count (per-sample counts do not enter the plan)
    int d_head;
    int bf16;            // storage type: 0 fp32, 1 bf16
    bool has_mask;       // additive mask
    bool planes_out;     // the output is written as three bf16 planes
    bool rows_aligned;   // the row strides of q, k, v and o are multiples of 16 bytes
};

struct AttnPlanOpts {
    int attn_split = 1;          // precision = 0: 1 = d_head 40 / 80 on k_attn_split.hip
    int attn_bf16 = 1;           // precision = 1: 1 = k_attn_bf16.hip, 0 = bf16 storage widened onto k_attn.hip
    int attn_bf16_variant = 7;   // k_attn_bf16.hip: bit 0 = 4-wave workgroups, two per CU; bit 1 / 2 = 64 query rows per wave (d = 40) on 8- / 4-wave workgroups;
                                 // 0x100 = whatever the grid (tests)
    int attn_pack_tail = 3;      // k_attn_split.hip: bit 0 = d = 40's columns 32..39 as a packed k step / packed output tile (PK); bit 1 = scores in log2 units with the
                                 // reference maximum as accumulator input and the row sum from a ones column (LG) (A/B, tests)
    int attn_kv_splits = 0;      // fp32, no mask: key slices + merge launch where the query-tile grid leaves CUs idle: 0 = automatic, 1 = never, S = forced
    int attn_kv_prefer8 = 1;     // ... and, for k_attn_split.hip, as many slices as let its 8-wave form fill the chip (A/B switch)
    int attn_d64 = 0;            // d_head 64: 0 = on k_attn.hip as before; 1 = on k_attn_split.hip (fp32, no mask, aligned rows) and k_attn_bf16.hip (bf16) wherever they
                                 // take the call (tests, A/B); 2 = the same, except the fp32 calls measured slower there (attn_plan.cpp: d64_stays_on_flash).  The engine's
                                 // default is 2 on an SD 2.x context (sdmi_config.variant = 1), whose UNet has 64-wide heads at every level
};

struct AttnPlan {
    AttnKernel kernel;
    int waves;       // per workgroup (0: unfused)
    bool pk, lg;     // k_attn_split.hip: template flags PK / LG
    int wpe, qr;     // k_attn_bf16.hip: workgroups per CU the register budget is cut for / 32-row query blocks per wave
    int q_rows;      // query rows per workgroup
    int kv_tile;     // keys per K / V tile: the unit kv_splits cuts
    int kv_splits;   // key slices (grid z); > 1: the kernel writes partials and launch_attention_combine merges them in slice order
};

AttnPlan plan_attention(const AttnPlanIn& in, const AttnPlanOpts& o);   // throws Error

// Where an attention call's operands and result lie inside wider parent buffers (tests: sdmi_op_qkv_attention_view, which feeds Engine::attention the way the
// model does -- q, k, v as column slices of one packed [n][rows][3C] buffer, or of buffers of their own -- instead of dense [n][rows][C] tensors).  A slice is the
// columns [off, off + n_state) of a parent [n][rows][ld]: ld elements between rows, rows * ld between samples.
struct AttnViewSlice { int ld, off, rows; };
struct AttnViewIn {
    int n, nq, nk, n_state;
    int bf16;               // storage type of the parents: 0 fp32, 1 bf16
    AttnViewSlice q, k, v;
    bool packed;            // q, k and v are slices of ONE parent (equal ld and rows, disjoint columns)
    AttnViewSlice out;      // the output slice: nq rows per sample
    bool out_planes;        // the result leaves as three bf16 planes (Engine::attention's o3), joined back: a dense output only
};
// SDMI_ERR_INVALID (thrown) for a view no launch may see: a slice that leaves its parent (ld < off + n_state, rows below the operand's), packed slices that
// overlap or disagree about their parent, a strided plane output, and any ld or off that is no multiple of 16 bytes -- the kernels load 16 bytes at a time
// and plan_attention knows of the row strides only rows_aligned.  Host-only, like the planner.
void check_attention_view(const AttnViewIn& v);

}  // namespace sdmi
