// attn_plan.cpp -- kernel, workgroup form and key-slice count of every attention call (see attn_plan.hpp).  Host-only.
// Every threshold below is pinned by tests/golden/attn_plan_choices.txt.
#include "attn_plan.hpp"

#include <algorithm>
#include <string>

#include "error.hpp"

namespace sdmi {

static const int kCUs = 256;

// workgroups of `rows` query rows the call makes (one key slice)
static long long workgroups(const AttnPlanIn& p, int rows) { return (long long)((p.nq + rows - 1) / rows) * p.n * p.n_head; }

static AttnPlan form(const AttnPlanIn& p, AttnKernel k, int waves, int kv_splits = 1, int wpe = 1, int qr = 1) {
    const AttnGeom& g = *attn_geom(k, p.d_head, qr);
    AttnPlan a{};
    a.kernel = k; a.waves = waves; a.wpe = wpe; a.qr = qr;
    a.q_rows = g.rows_per_wave * waves; a.kv_tile = g.kv_tile; a.kv_splits = kv_splits;
    return a;
}

// Key slices (fp32, no mask): at batch 1 the 32 x 32 level's self attention is 128 workgroups and the 16 x 16 level's 64 -- most CUs idle while each workgroup
// walks every key.  S slices of the keys run as S x the workgroups (grid z) and a merge launch combines them in slice order.  S = what fills the CUs with 4-wave
// workgroups, at least two K / V tiles per slice, at most 8; option attn_kv_splits: 0 = this rule, 1 = never, S = forced (at most one slice per tile).
static int plan_kv_splits(const AttnPlanIn& p, const AttnPlanOpts& o, bool on_split) {
    if (p.bf16 || p.has_mask || o.attn_kv_splits == 1) return 1;
    const AttnGeom& g = *attn_geom(on_split ? AttnKernel::Split : AttnKernel::Flash, p.d_head);
    const int tiles = (p.nk + g.kv_tile - 1) / g.kv_tile;
    if (o.attn_kv_splits > 1) return std::min(o.attn_kv_splits, std::max(1, tiles));
    const long long most = std::min(tiles / 2, 8);
    const long long wgs4 = workgroups(p, 4 * g.rows_per_wave);
    long long s = std::min<long long>(wgs4 > 0 && wgs4 <= kCUs / 2 ? kCUs / wgs4 : 1, most);
    if (on_split && o.attn_kv_prefer8) {   // k_attn_split.hip: enough slices that the 8-wave form fills the chip beat fewer slices of the 4-wave form
        const long long wgs8 = workgroups(p, 8 * g.rows_per_wave);
        const long long s8 = std::min<long long>(wgs8 < kCUs ? (kCUs + wgs8 - 1) / wgs8 : 1, most);
        if (s8 >= 2 && wgs8 * s8 >= kCUs) s = s8;
    }
    return (int)std::max<long long>(1, s);
}

// attn_d64 = 2, fp32: the d = 64 calls that stay on k_attn.hip because the interleaved A/B measured k_attn_split.hip slower there (profiles/r13a_attn_d64_ab.txt, 216
// shapes).  k_attn_split.hip wins wherever k_attn.hip needs more than one round of workgroups or walks a long key loop (1.1 - 2.0 x); it loses 2 - 8 % in the
// latency-bound regime -- k_attn.hip's 64-row workgroups, key slices included, fit the CUs in ONE round and each walks a handful of key tiles: a 128-row workgroup then
// is a longer serial chain (3.6 against 3.2 us per 64-key tile, measured) and nothing is left for it to overlap.  Two measured constants: a tile of k_attn_split.hip
// costs 9/8 of one of k_attn.hip's, a merge launch 15/8.  At nq <= 64 both kernels run one partly filled query tile: equal within 1.5 %, the call goes to the new instance.
static bool d64_stays_on_flash(const AttnPlanIn& p, const AttnPlanOpts& o) {
    if (p.nq <= 64) return false;
    const int tiles = (p.nk + 63) / 64;
    const int sf = plan_kv_splits(p, o, false), ss = plan_kv_splits(p, o, true);
    if (workgroups(p, 64) * sf > kCUs) return false;
    const int tf = (tiles + sf - 1) / sf, ts = (tiles + ss - 1) / ss;
    return 8 * tf + (sf > 1 ? 15 : 0) <= 9 * ts + (ss > 1 ? 15 : 0);
}

// k_attn.hip: 8-wave workgroups once they still fill the chip (>= 1.5 workgroups per CU), else 4-wave
static AttnPlan plan_flash(const AttnPlanIn& p, int kv_splits) {
    return form(p, AttnKernel::Flash, 2 * workgroups(p, 128) >= 3 * kCUs ? 8 : 4, kv_splits);
}

// k_attn_split.hip: the widest workgroup that still gives every CU a workgroup, key slices included.  PK is a d = 40 form; without LG (round 4's softmax, the A/B
// form) d = 80 has no 8-wave instance.
static AttnPlan plan_split(const AttnPlanIn& p, const AttnPlanOpts& o, int kv_splits) {
    const bool pk = p.d_head == 40 && (o.attn_pack_tail & 1), lg = (o.attn_pack_tail & 2) != 0;
    const bool w8 = workgroups(p, 256) * kv_splits >= kCUs && (lg || p.d_head != 80);
    AttnPlan a = form(p, AttnKernel::Split, w8 ? 8 : 4, kv_splits);
    a.pk = pk; a.lg = lg;
    return a;
}

// k_attn_bf16.hip.  Option attn_bf16_variant allows the round 6 forms (0x100, tests: the form whatever the grid size):
//   bit 1  d = 40, self attention: 64 query rows per wave on 8-wave workgroups;
//   bit 2  d = 40, a context of at most two 64-key tiles: the same on 4-wave workgroups, two per CU;
//   bit 0  d = 80 (and d = 40 without bits 1 / 2): 4-wave workgroups, two per CU -- no gain on the self attentions, so short contexts only.
// Otherwise the widest workgroup that still gives every CU a workgroup.
static AttnPlan plan_bf16(const AttnPlanIn& p, const AttnPlanOpts& o) {
    const int v = o.attn_bf16_variant, d = p.d_head;
    const bool force = (v & 0x100) != 0, short_ctx = p.nk <= 128;
    auto fills = [&](int rows, int per_cu) { return workgroups(p, rows) >= per_cu * kCUs; };
    if (d == 40) {
        if ((v & 4) && (force ? !(v & 2) : short_ctx && fills(256, 2))) return form(p, AttnKernel::Bf16, 4, 1, 2, 2);
        if ((v & 2) && (force || (!short_ctx && fills(512, 1)))) return form(p, AttnKernel::Bf16, 8, 1, 2, 2);
    }
    if ((d == 40 || d == 80) && (v & 1) && (force || (short_ctx && fills(128, 2)))) return form(p, AttnKernel::Bf16, 4, 1, 2);
    for (int waves : {8, 4})
        if (fills(32 * waves, 1)) return form(p, AttnKernel::Bf16, waves);
    return form(p, AttnKernel::Bf16, 2);
}

AttnPlan plan_attention(const AttnPlanIn& p, const AttnPlanOpts& o) {
    const int d = p.d_head;
    const bool fused = attn_supported_head_dim(d);
    if (p.planes_out && (p.bf16 || !fused || (p.n_head * d) % 32)) throw Error(SDMI_ERR_STATE, "attention: plane output needs a fused fp32 kernel");
    if (!fused) {
        if (p.has_mask) throw Error(SDMI_ERR_UNSUPPORTED, "attention: additive mask is only supported for head dims 40/80/160");
        if (d % 32) throw Error(SDMI_ERR_UNSUPPORTED, "attention: head dim must be 40/80/160 or a multiple of 32");
        if (p.bf16 && (d % 64)) throw Error(SDMI_ERR_UNSUPPORTED, "bf16 attention (unfused path): head dim must be a multiple of 64");
        AttnPlan a{};
        a.kernel = AttnKernel::Unfused; a.kv_splits = 1;
        return a;
    }
    if (p.bf16 && p.has_mask) throw Error(SDMI_ERR_UNSUPPORTED, "attention: additive mask is fp32-only");
    if (p.bf16 && o.attn_bf16 && attn_bf16_head_dim(d, o.attn_d64)) return plan_bf16(p, o);
    const bool on_split = !p.bf16 && !p.has_mask && o.attn_split && p.rows_aligned && attn_split_head_dim(d, o.attn_d64) && !(d == 64 && o.attn_d64 == 2 && d64_stays_on_flash(p, o));
    const int kv_splits = plan_kv_splits(p, o, on_split);
    return on_split ? plan_split(p, o, kv_splits) : plan_flash(p, kv_splits);
}

void check_attention_view(const AttnViewIn& v) {
    if (v.n <= 0 || v.nq <= 0 || v.nk <= 0 || v.n_state <= 0) throw Error(SDMI_ERR_INVALID, "attention view: bad shape");
    const int unit = v.bf16 ? 8 : 4;   // elements in 16 bytes
    auto slice = [&](const AttnViewSlice& s, int need_rows, const char* what) {
        if (s.off < 0 || s.ld <= 0 || (long long)s.off + v.n_state > s.ld) throw Error(SDMI_ERR_INVALID, std::string("attention view: ") + what + " leaves its parent (need 0 <= off, off + n_state <= ld)");
        if (s.rows < need_rows) throw Error(SDMI_ERR_INVALID, std::string("attention view: ") + what + " has fewer parent rows than the operand");
        if (s.ld % unit || s.off % unit) throw Error(SDMI_ERR_INVALID, std::string("attention view: ") + what + ": ld and off must be multiples of 16 bytes");
    };
    slice(v.q, v.nq, "q");
    slice(v.k, v.nk, "k");
    slice(v.v, v.nk, "v");
    slice(v.out, v.nq, "the output");
    if (v.packed) {
        if (v.q.ld != v.k.ld || v.q.ld != v.v.ld || v.q.rows != v.k.rows || v.q.rows != v.v.rows) throw Error(SDMI_ERR_INVALID, "attention view: packed q, k and v share one parent (equal ld and rows)");
        auto apart = [&](const AttnViewSlice& a, const AttnViewSlice& b) { return a.off + v.n_state <= b.off || b.off + v.n_state <= a.off; };
        if (!apart(v.q, v.k) || !apart(v.q, v.v) || !apart(v.k, v.v)) throw Error(SDMI_ERR_INVALID, "attention view: packed slices overlap");
    }
    if (v.out_planes && (v.out.ld != v.n_state || v.out.off || v.out.rows != v.nq)) throw Error(SDMI_ERR_INVALID, "attention view: the plane output is dense (out_ld = n_state, out_off = 0, out_rows = nq)");
}

}  // namespace sdmi
