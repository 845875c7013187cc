// sdmi_capi_ops.cpp -- the operator-level, bench and introspection entry points of the C ABI (sdmi_op_*, sdmi_bench_*, sdmi_attention_plan; include/sdmi.h):
// host arrays staged through the device pool around the Engine members of engine_ops.cpp.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "capi_util.hpp"

namespace {
// x [n,c,h,w] -> the host image of its parent: NHWC rows ld wide, x at columns [off, off + c), `fill` elsewhere
std::vector<float> view_parent(const float* x, int n, int c, int h, int w, int ld, int off, float fill) {
    if (!x) throw Error(SDMI_ERR_INVALID, "null input pointer");
    const size_t hw = (size_t)h * w;
    std::vector<float> img((size_t)n * hw * ld, fill);
    for (int b = 0; b < n; ++b)
        for (int j = 0; j < c; ++j) {
            const float* src = x + ((size_t)b * c + j) * hw;
            float* dst = img.data() + (size_t)b * hw * ld + off + j;
            for (size_t i = 0; i < hw; ++i) dst[i * ld] = src[i];
        }
    return img;
}
// its inverse: columns [off, off + c) of the parent image -> x [n,c,h,w].  written (may be null): the SDMI_ERR_STATE message where a column next to them is no NaN any more
void view_unparent(const std::vector<float>& img, float* x, int n, int c, int h, int w, int ld, int off, const char* written) {
    const size_t hw = (size_t)h * w;
    for (size_t r = 0; written && r < n * hw; ++r)
        for (int j = 0; j < ld; ++j)
            if ((j < off || j >= off + c) && !std::isnan(img[r * ld + j])) throw Error(SDMI_ERR_STATE, written);
    for (int b = 0; b < n; ++b)
        for (int j = 0; j < c; ++j)
            for (size_t i = 0; i < hw; ++i) x[((size_t)b * c + j) * hw + i] = img[((size_t)b * hw + i) * ld + off + j];
}
void need_view(const sdmi_op_view* v, int cin, int cout) {
    if (!v) throw Error(SDMI_ERR_INVALID, "null view");
    Engine::check_view(*v, cin, cout);
}
// the optional bias [c] of a wrapper on the device, null without one: through stage_epi (epi: option op_misalign acts on it) or in a plain pool buffer
const float* stage_bias(Engine& e, std::unique_ptr<Engine::Buf>& holder, const float* bias, int c, bool epi) {
    if (epi) return bias ? e.stage_epi(holder, bias, 1, c, c, 0) : nullptr;
    holder.reset(new Engine::Buf(&e, (size_t)c * sizeof(float)));
    if (bias) SDMI_HIP(hipMemcpyAsync(holder->p, bias, (size_t)c * sizeof(float), hipMemcpyHostToDevice, e.stream()));
    return bias ? holder->f() : nullptr;
}
// a normalisation wrapper: x / out of `elems` floats, gamma / beta [c]; run(engine, x, gamma, beta, out) on the device copies
template <class F>
int norm_op(sdmi_ctx* ctx, bool shape_ok, const char* bad_shape, const float* x, const float* gamma, const float* beta, size_t elems, int c, float* out, F&& run) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!shape_ok) throw Error(SDMI_ERR_INVALID, bad_shape);
        Engine::Call call(e);
        DevIn dx(e, x, elems * sizeof(float)), dg(e, gamma, c * sizeof(float)), db(e, beta, c * sizeof(float));
        DevOut dout(e, out, elems * sizeof(float));
        run(e, dx.f(), dg.f(), db.f(), dout.f());
        call.finish();
        dout.fetch();
    });
}
}  // namespace

extern "C" {

int sdmi_op_qkv_attention_ragged(sdmi_ctx* ctx, const float* q, const float* k, const float* v, const int32_t* kv_len,
                                 int32_t n, int32_t nq, int32_t nk, int32_t n_state, int32_t n_head, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || nq <= 0 || nk <= 0 || n_state <= 0) throw Error(SDMI_ERR_INVALID, "qkv_attention_ragged: bad shape");
        if (!kv_len) throw Error(SDMI_ERR_INVALID, "qkv_attention_ragged: kv_len is NULL");
        for (int32_t b = 0; b < n; ++b)
            if (kv_len[b] < 1 || kv_len[b] > nk) throw Error(SDMI_ERR_INVALID, "qkv_attention_ragged: kv_len[" + std::to_string(b) + "] = " + std::to_string(kv_len[b]) + " outside 1 .. nk");
        const size_t qb = (size_t)n * nq * n_state * sizeof(float), kb = (size_t)n * nk * n_state * sizeof(float);
        Engine::Call call(e);
        DevIn dq(e, q, qb), dk(e, k, kb), dv(e, v, kb);
        DevOut dout(e, out, qb);
        e.qkv_attention_dev(dq.f(), dk.f(), dv.f(), nullptr, 0, n, nq, nk, n_state, n_head, dout.f(), kv_len);
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_qkv_attention_view(sdmi_ctx* ctx, const float* q, const float* k, const float* v, const float* mask, int32_t mask_ld, const int32_t* kv_len,
                               int32_t n, int32_t nq, int32_t nk, int32_t n_state, int32_t n_head, sdmi_attn_view view, float* parent) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!q || !k || !v || !parent) throw Error(SDMI_ERR_INVALID, "qkv_attention_view: null pointer");
        e.check_qkv_attention_view(view, mask != nullptr, mask_ld, kv_len, n, nq, nk, n_state, n_head);   // every refusal before anything is allocated or launched
        const size_t qb = (size_t)n * nq * n_state * sizeof(float), kb = (size_t)n * nk * n_state * sizeof(float);
        const size_t pbytes = (size_t)n * view.out_rows * view.out_ld * sizeof(float);
        Engine::Call call(e);
        DevIn dq(e, q, qb), dk(e, k, kb), dv(e, v, kb);
        Engine::Buf dm(&e, mask ? (size_t)nq * mask_ld * sizeof(float) : 256);
        if (mask) SDMI_HIP(hipMemcpyAsync(dm.p, mask, (size_t)nq * mask_ld * sizeof(float), hipMemcpyHostToDevice, e.stream()));
        DevOut dout(e, parent, pbytes);
        SDMI_HIP(hipMemcpyAsync(dout.buf.p, parent, pbytes, hipMemcpyHostToDevice, e.stream()));
        e.op_qkv_attention_view(dq.f(), dk.f(), dv.f(), mask ? dm.f() : nullptr, mask_ld, kv_len, n, nq, nk, n_state, n_head, view, dout.f());
        call.finish();
        dout.fetch();
    });
}

// ---- operator-level entry points -----------------------------------------------------------
int sdmi_op_group_norm(sdmi_ctx* ctx, const float* x, const float* gamma, const float* beta, int32_t n, int32_t c,
                       int32_t h, int32_t w, int32_t n_group, float eps, int32_t fuse_silu, float* out) {
    return norm_op(ctx, n > 0 && c > 0 && h > 0 && w > 0, "group_norm: bad shape", x, gamma, beta, (size_t)n * c * h * w, c, out,
                   [&](Engine& e, const float* dx, const float* dg, const float* db, float* dout) { e.op_group_norm(dx, dg, db, n, c, h, w, n_group, eps, fuse_silu != 0, dout); });
}

int sdmi_op_group_norm_fp8(sdmi_ctx* ctx, const float* x, const float* gamma, const float* beta, int32_t n, int32_t c, int32_t h,
                           int32_t w, int32_t n_group, float eps, int32_t fuse_silu, float* out) {
    return norm_op(ctx, n > 0 && c > 0 && h > 0 && w > 0, "group_norm_fp8: bad shape", x, gamma, beta, (size_t)n * c * h * w, c, out,
                   [&](Engine& e, const float* dx, const float* dg, const float* db, float* dout) { e.op_group_norm_fp8(dx, dg, db, n, c, h, w, n_group, eps, fuse_silu != 0, dout); });
}

int sdmi_op_layer_norm(sdmi_ctx* ctx, const float* x, const float* gamma, const float* beta, int32_t rows, int32_t c,
                       float eps, float* out) {
    return norm_op(ctx, rows > 0 && c > 0, "layer_norm: bad shape", x, gamma, beta, (size_t)rows * c, c, out,
                   [&](Engine& e, const float* dx, const float* dg, const float* db, float* dout) { e.op_layer_norm(dx, dg, db, rows, c, eps, dout); });
}

int sdmi_op_conv2d(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, int32_t n, int32_t cin,
                   int32_t h, int32_t w, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t upsample2x,
                   float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || cin <= 0 || h <= 0 || w <= 0 || cout <= 0 || stride <= 0) throw Error(SDMI_ERR_INVALID, "conv2d: bad shape");
        const int ups = upsample2x ? 1 : 0;
        int ho, wo;
        Engine::conv_out_hw(h, w, k, stride, pad, ups, &ho, &wo);
        Engine::Call call(e);
        DevIn dx(e, x, (size_t)n * cin * h * w * sizeof(float)), dw(e, weight, (size_t)cout * cin * k * k * sizeof(float));
        std::unique_ptr<Engine::Buf> db;
        const float* bias_d = stage_bias(e, db, bias, cout, false);
        DevOut dout(e, out, (size_t)n * cout * ho * wo * sizeof(float));
        e.op_conv2d(dx.f(), dw.f(), bias_d, n, cin, h, w, cout, k, stride, pad, ups, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_conv2d_epilogue(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, const float* temb, int32_t temb_stride,
                            const float* resid, int32_t resid_ld, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k, int32_t stride,
                            int32_t pad, int32_t upsample2x, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || cin <= 0 || h <= 0 || w <= 0 || cout <= 0 || stride <= 0 || temb_stride < 0 || resid_ld < 0) throw Error(SDMI_ERR_INVALID, "conv2d_epilogue: bad shape");
        const int ups = upsample2x ? 1 : 0;
        int ho, wo;
        Engine::conv_out_hw(h, w, k, stride, pad, ups, &ho, &wo);
        Engine::Call call(e);
        DevIn dx(e, x, (size_t)n * cin * h * w * sizeof(float)), dw(e, weight, (size_t)cout * cin * k * k * sizeof(float));
        std::unique_ptr<Engine::Buf> db;
        const float* bias_d = stage_bias(e, db, bias, cout, true);
        Engine::EpiOps epi;
        epi.temb = temb; epi.temb_stride = temb_stride; epi.resid = resid; epi.resid_ld = resid_ld;
        DevOut dout(e, out, (size_t)n * cout * ho * wo * sizeof(float));
        e.op_conv2d(dx.f(), dw.f(), bias_d, n, cin, h, w, cout, k, stride, pad, ups, dout.f(), &epi);
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_conv2d_pair(sdmi_ctx* ctx, const float* x, const float* h, const float* w_skip, const float* b_skip, const float* w_out, const float* b_out, int32_t n,
                        int32_t cin_x, int32_t cout, int32_t hh, int32_t ww, float* out, float* out_planes) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || cin_x <= 0 || cout <= 0 || hh <= 0 || ww <= 0) throw Error(SDMI_ERR_INVALID, "conv2d_pair: bad shape");
        const size_t px = (size_t)n * hh * ww;
        Engine::Call call(e);
        DevIn dx(e, x, px * cin_x * sizeof(float)), dh(e, h, px * cout * sizeof(float));
        DevIn dws(e, w_skip, (size_t)cout * cin_x * sizeof(float)), dwo(e, w_out, (size_t)cout * cout * 9 * sizeof(float));
        std::unique_ptr<Engine::Buf> dbs, dbo;
        const float* bs = stage_bias(e, dbs, b_skip, cout, true);
        const float* bo = stage_bias(e, dbo, b_out, cout, true);
        DevOut dout(e, out, px * cout * sizeof(float));
        std::unique_ptr<DevOut> dout3;
        if (out_planes) dout3.reset(new DevOut(e, out_planes, px * cout * sizeof(float)));
        e.op_conv2d_pair(dx.f(), dh.f(), dws.f(), bs, dwo.f(), bo, n, cin_x, cout, hh, ww, dout.f(), dout3 ? dout3->f() : nullptr);
        call.finish();
        dout.fetch();
        if (dout3) dout3->fetch();
    });
}

int sdmi_op_linear_epilogue(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, const float* resid, int32_t resid_ld, int32_t rows,
                            int32_t cin, int32_t cout, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (rows <= 0 || cin <= 0 || cout <= 0 || resid_ld < 0) throw Error(SDMI_ERR_INVALID, "linear_epilogue: bad shape");
        Engine::Call call(e);
        DevIn dx(e, x, (size_t)rows * cin * sizeof(float)), dw(e, weight, (size_t)cin * cout * sizeof(float));
        std::unique_ptr<Engine::Buf> db;
        const float* bias_d = stage_bias(e, db, bias, cout, true);
        Engine::EpiOps epi;
        epi.resid = resid; epi.resid_ld = resid_ld;
        DevOut dout(e, out, (size_t)rows * cout * sizeof(float));
        e.op_linear(dx.f(), dw.f(), bias_d, rows, cin, cout, dout.f(), &epi);
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_linear_pair(sdmi_ctx* ctx, const float* u, const float* h, const float* w_main, const float* b_main, const float* w_aux, const float* b_aux,
                        const float* resid, int32_t resid_ld, int32_t rows, int32_t k_main, int32_t k_aux, int32_t cout, int32_t out_ld, float* out, float* out_planes) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (rows <= 0 || k_main <= 0 || k_aux <= 0 || cout <= 0 || resid_ld < 0 || out_ld < 0 || (resid_ld && resid_ld < cout) || (out_ld && out_ld < cout))
            throw Error(SDMI_ERR_INVALID, "linear_pair: bad shape");
        if (!out && !out_planes) throw Error(SDMI_ERR_INVALID, "linear_pair: no output pointer");
        Engine::Call call(e);
        DevIn du(e, u, (size_t)rows * k_main * sizeof(float)), dh(e, h, (size_t)rows * k_aux * sizeof(float));
        DevIn dwm(e, w_main, (size_t)k_main * cout * sizeof(float)), dwa(e, w_aux, (size_t)k_aux * cout * sizeof(float));
        std::unique_ptr<Engine::Buf> dbm, dba, dr;
        const float* bm = stage_bias(e, dbm, b_main, cout, true);
        const float* ba = stage_bias(e, dba, b_aux, cout, true);
        const float* r = resid ? e.stage_epi(dr, resid, rows, cout, resid_ld ? resid_ld : cout, 0) : nullptr;
        std::unique_ptr<DevOut> dout, dout3;
        if (out) dout.reset(new DevOut(e, out, (size_t)rows * cout * sizeof(float)));
        if (out_planes) dout3.reset(new DevOut(e, out_planes, (size_t)rows * cout * sizeof(float)));
        e.op_linear_pair(du.f(), dh.f(), dwm.f(), bm, dwa.f(), ba, r, resid_ld, rows, k_main, k_aux, cout, out_ld, dout ? dout->f() : nullptr, dout3 ? dout3->f() : nullptr);
        call.finish();
        if (dout) dout->fetch();
        if (dout3) dout3->fetch();
    });
}

int sdmi_op_linear_fold(sdmi_ctx* ctx, const float* w_lin, const float* b_lin, const float* w_proj, int32_t k_main, int32_t cmid, int32_t cout, float* wf, float* bf) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (k_main <= 0 || cmid <= 0 || cout <= 0) throw Error(SDMI_ERR_INVALID, "linear_fold: bad shape");
        Engine::Call call(e);
        DevIn dl(e, w_lin, (size_t)k_main * cmid * sizeof(float)), dp(e, w_proj, (size_t)cout * cmid * sizeof(float));
        std::unique_ptr<DevIn> db;
        if (b_lin) db.reset(new DevIn(e, b_lin, (size_t)cmid * sizeof(float)));
        DevOut dwf(e, wf, (size_t)cout * k_main * sizeof(float)), dbf(e, bf, (size_t)cout * sizeof(float));
        e.op_linear_fold(dl.f(), db ? db->f() : nullptr, dp.f(), k_main, cmid, cout, dwf.f(), dbf.f());
        call.finish();
        dwf.fetch();
        dbf.fetch();
    });
}

// ---- the operators on channel-slice views ---------------------------------------------------------------------------------
int sdmi_op_conv2d_view(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, const float* temb, int32_t temb_stride,
                        const float* resid, int32_t resid_ld, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k, int32_t stride,
                        int32_t pad, int32_t upsample2x, const sdmi_op_view* view, float* parent, float* parent_planes) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || cin <= 0 || h <= 0 || w <= 0 || cout <= 0 || stride <= 0 || k <= 0 || pad < 0 || temb_stride < 0 || resid_ld < 0) throw Error(SDMI_ERR_INVALID, "conv2d_view: bad shape");
        need_view(view, cin, cout);
        const int ups = upsample2x ? 1 : 0;
        int ho, wo;
        Engine::conv_out_hw(h, w, k, stride, pad, ups, &ho, &wo);
        if (ho <= 0 || wo <= 0) throw Error(SDMI_ERR_INVALID, "conv2d_view: empty output");
        const bool both = view->out_planes == 3 && e.config().precision == 0;
        if (both && !parent_planes) throw Error(SDMI_ERR_INVALID, "conv2d_view: out_planes = 3 returns two copies of the parent");
        const std::vector<float> xp = view_parent(x, n, cin, h, w, view->in_ld, view->in_off, view->in_fill);
        const size_t pbytes = (size_t)n * ho * wo * view->out_ld * sizeof(float);
        Engine::Call call(e);
        DevIn dx(e, xp.data(), xp.size() * sizeof(float)), dw(e, weight, (size_t)cout * cin * k * k * sizeof(float));
        std::unique_ptr<Engine::Buf> db;
        const float* bias_d = stage_bias(e, db, bias, cout, true);
        Engine::EpiOps epi;
        epi.temb = temb; epi.temb_stride = temb_stride; epi.resid = resid; epi.resid_ld = resid_ld;
        DevIn dpre(e, parent, pbytes);
        DevOut dout(e, parent, pbytes);
        SDMI_HIP(hipMemcpyAsync(dout.buf.p, dpre.buf.p, pbytes, hipMemcpyDeviceToDevice, e.stream()));
        std::unique_ptr<DevOut> dout3;
        if (both) dout3.reset(new DevOut(e, parent_planes, pbytes));
        try {
            e.op_conv2d_view(dx.f(), dw.f(), bias_d, n, cin, h, w, cout, k, stride, pad, ups, *view, &epi, dout.f(), both ? dout3->f() : nullptr);
        } catch (...) {
            try { dout.fetch(); } catch (...) {}     // what a refused launch left of the parent
            throw;
        }
        call.finish();
        dout.fetch();
        if (both) dout3->fetch();
    });
}

int sdmi_op_linear_view(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, const float* resid, int32_t resid_ld, int32_t rows,
                        int32_t cin, int32_t cout, const sdmi_op_view* view, float* parent) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (rows <= 0 || cin <= 0 || cout <= 0 || resid_ld < 0) throw Error(SDMI_ERR_INVALID, "linear_view: bad shape");
        need_view(view, cin, cout);
        const size_t pbytes = (size_t)rows * view->out_ld * sizeof(float);
        Engine::Call call(e);
        DevIn dx(e, x, (size_t)rows * cin * sizeof(float)), dw(e, weight, (size_t)cin * cout * sizeof(float));
        std::unique_ptr<Engine::Buf> db;
        const float* bias_d = stage_bias(e, db, bias, cout, true);
        Engine::EpiOps epi;
        epi.resid = resid; epi.resid_ld = resid_ld;
        DevIn dpre(e, parent, pbytes);
        DevOut dout(e, parent, pbytes);
        SDMI_HIP(hipMemcpyAsync(dout.buf.p, dpre.buf.p, pbytes, hipMemcpyDeviceToDevice, e.stream()));
        try {
            e.op_linear_view(dx.f(), dw.f(), bias_d, rows, cin, cout, *view, &epi, dout.f());
        } catch (...) {
            try { dout.fetch(); } catch (...) {}
            throw;
        }
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_group_norm_view(sdmi_ctx* ctx, const float* x, const float* gamma, const float* beta, int32_t n, int32_t c, int32_t h, int32_t w,
                            int32_t n_group, float eps, int32_t fuse_silu, const sdmi_op_view* view, int32_t form, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || c <= 0 || h <= 0 || w <= 0) throw Error(SDMI_ERR_INVALID, "group_norm_view: bad shape");
        need_view(view, c, c);
        const std::vector<float> xp = view_parent(x, n, c, h, w, view->in_ld, view->in_off, view->in_fill);
        Engine::Call call(e);
        DevIn dx(e, xp.data(), xp.size() * sizeof(float)), dg(e, gamma, c * sizeof(float)), db(e, beta, c * sizeof(float));
        DevOut dout(e, out, (size_t)n * c * h * w * sizeof(float));
        e.op_group_norm_view(dx.f(), dg.f(), db.f(), n, c, h, w, n_group, eps, fuse_silu != 0, *view, form, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_cat_chain(sdmi_ctx* ctx, const float* x, const float* w_x, const float* b_x, const float* w_skip, const float* b_skip, const float* gamma,
                      const float* beta, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cx, int32_t cskip, float eps, int32_t fuse_silu,
                      int32_t dense, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || cin <= 0 || h <= 0 || w <= 0 || cx <= 0 || cskip <= 0) throw Error(SDMI_ERR_INVALID, "cat_chain: bad shape");
        const int ctot = cx + cskip;
        Engine::Call call(e);
        DevIn dx(e, x, (size_t)n * cin * h * w * sizeof(float)), dwx(e, w_x, (size_t)cx * cin * 9 * sizeof(float)), dws(e, w_skip, (size_t)cskip * cin * 9 * sizeof(float));
        DevIn dbx(e, b_x, cx * sizeof(float)), dbs(e, b_skip, cskip * sizeof(float)), dg(e, gamma, ctot * sizeof(float)), db(e, beta, ctot * sizeof(float));
        DevOut dout(e, out, (size_t)n * ctot * h * w * sizeof(float));
        e.op_cat_chain(dx.f(), dwx.f(), dbx.f(), dws.f(), dbs.f(), dg.f(), db.f(), n, cin, h, w, cx, cskip, eps, fuse_silu != 0, dense != 0, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_geglu_forward(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, int32_t rows, int32_t cin,
                          int32_t hidden, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (rows <= 0 || cin <= 0 || hidden <= 0 || cin % 32) throw Error(SDMI_ERR_INVALID, "geglu_forward: bad shape");
        Engine::Call call(e);
        DevIn dx(e, x, (size_t)rows * cin * sizeof(float)), dw(e, weight, (size_t)cin * 2 * hidden * sizeof(float));
        std::unique_ptr<Engine::Buf> db;
        const float* bias_d = stage_bias(e, db, bias, 2 * hidden, false);
        DevOut dout(e, out, (size_t)rows * hidden * sizeof(float));
        e.op_geglu_forward(dx.f(), dw.f(), bias_d, rows, cin, hidden, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_linear(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, int32_t rows, int32_t cin,
                   int32_t cout, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (rows <= 0 || cin <= 0 || cout <= 0) throw Error(SDMI_ERR_INVALID, "linear: bad shape");
        Engine::Call call(e);
        DevIn dx(e, x, (size_t)rows * cin * sizeof(float)), dw(e, weight, (size_t)cin * cout * sizeof(float));
        std::unique_ptr<Engine::Buf> db;
        const float* bias_d = stage_bias(e, db, bias, cout, false);
        DevOut dout(e, out, (size_t)rows * cout * sizeof(float));
        e.op_linear(dx.f(), dw.f(), bias_d, rows, cin, cout, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_geglu(sdmi_ctx* ctx, const float* proj, int32_t rows, int32_t hidden, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (rows <= 0 || hidden <= 0 || hidden % 4) throw Error(SDMI_ERR_INVALID, "geglu: bad shape");
        Engine::Call call(e);
        DevIn dp(e, proj, (size_t)rows * 2 * hidden * sizeof(float));
        DevOut dout(e, out, (size_t)rows * hidden * sizeof(float));
        e.op_geglu(dp.f(), rows, hidden, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_timestep_embedding(sdmi_ctx* ctx, int32_t t, int32_t dim, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (dim <= 0 || dim % 2) throw Error(SDMI_ERR_INVALID, "timestep_embedding: dim must be even");
        Engine::Call call(e);
        DevOut dout(e, out, (size_t)dim * sizeof(float));
        e.op_timestep_embedding(t, dim, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_timestep_embedding_f(sdmi_ctx* ctx, double t, int32_t dim, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (dim <= 0 || dim % 2) throw Error(SDMI_ERR_INVALID, "timestep_embedding: dim must be even");
        if (!std::isfinite(t)) throw Error(SDMI_ERR_INVALID, "timestep_embedding: t must be finite");
        Engine::Call call(e);
        DevOut dout(e, out, (size_t)dim * sizeof(float));
        e.op_timestep_embedding_f(t, dim, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_freeu(sdmi_ctx* ctx, const float* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t cx, int32_t version, float b, float s, float* y,
                  float* y_from_planes) {
    bool planes = false;
    const int st = guarded([&] {
        Engine& e = eng(ctx);
        if (!x || !y) throw Error(SDMI_ERR_INVALID, "op_freeu: null pointer");
        if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || cx <= 0 || cx >= c) throw Error(SDMI_ERR_INVALID, "op_freeu: bad shape");
        // rows one granule wider than the tensor, the columns next to it NaN: whatever is written there shows
        const int ld = c + (e.config().precision ? 64 : 32);
        const std::vector<float> xp = view_parent(x, n, c, h, w, ld, 0, std::nanf(""));
        const size_t pbytes = xp.size() * sizeof(float);
        std::vector<float> yp(xp.size()), yp3(y_from_planes ? xp.size() : 0);
        Engine::Call call(e);
        DevIn dpre(e, xp.data(), pbytes);
        DevOut dout(e, yp.data(), pbytes);
        SDMI_HIP(hipMemcpyAsync(dout.buf.p, dpre.buf.p, pbytes, hipMemcpyDeviceToDevice, e.stream()));
        std::unique_ptr<DevOut> dout3;
        if (y_from_planes) dout3.reset(new DevOut(e, yp3.data(), pbytes));
        planes = e.op_freeu(dout.f(), n, c, h, w, ld, cx, version, b, s, dout3 ? dout3->f() : nullptr);
        call.finish();
        dout.fetch();
        if (planes && dout3) dout3->fetch();
        view_unparent(yp, y, n, c, h, w, ld, 0, "op_freeu: a column next to the tensor was written (fp32 / bf16)");
        if (planes && y_from_planes) view_unparent(yp3, y_from_planes, n, c, h, w, ld, 0, "op_freeu: a column next to the tensor was written (planes)");
    });
    return st != SDMI_OK ? st : (planes ? 1 : 0);
}

int sdmi_op_ip_attention(sdmi_ctx* ctx, const float* q, const float* k_ip, const float* v_ip, const float* o_text, const float* scale, int32_t n, int32_t nq,
                         int32_t T_ip, int32_t n_state, int32_t n_head, int32_t planes, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!q || !k_ip || !v_ip || !o_text || !scale || !out) throw Error(SDMI_ERR_INVALID, "op_ip_attention: null pointer");
        if (n < 1 || nq < 1 || T_ip < 1 || n_state < 1 || n_head < 1) throw Error(SDMI_ERR_INVALID, "op_ip_attention: bad shape");
        if (T_ip > 64) throw Error(SDMI_ERR_UNSUPPORTED, "op_ip_attention: more than 64 image tokens");
        const size_t qb = (size_t)n * nq * n_state * sizeof(float), kb = (size_t)n * T_ip * n_state * sizeof(float);
        Engine::Call call(e);
        DevIn dq(e, q, qb), dk(e, k_ip, kb), dv(e, v_ip, kb), dot(e, o_text, qb), ds(e, scale, (size_t)n * sizeof(float));
        DevOut dout(e, out, qb);
        e.op_ip_attention(dq.f(), dk.f(), dv.f(), dot.f(), ds.f(), n, nq, T_ip, n_state, n_head, planes != 0, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_resize(sdmi_ctx* ctx, const float* x, int32_t n, int32_t h, int32_t w, int32_t out_h, int32_t out_w, int32_t mode, int32_t antialias,
                   float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0) throw Error(SDMI_ERR_INVALID, "resize: sizes must be positive");
        Engine::Call call(e);
        DevIn dx(e, x, (size_t)n * 4 * h * w * sizeof(float));
        DevOut dout(e, out, (size_t)n * 4 * out_h * out_w * sizeof(float));
        e.op_resize(dx.f(), n, h, w, out_h, out_w, mode, antialias, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_unpack_tensor(sdmi_ctx* ctx, const void* raw, int32_t dtype, int32_t ndim, const int64_t* dims, int32_t transform, float* out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (!dims || ndim < 1 || ndim > 4) throw Error(SDMI_ERR_INVALID, "unpack_tensor: ndim must be 1 .. 4");
        if (dtype < 0 || dtype > 2) throw Error(SDMI_ERR_INVALID, "unpack_tensor: dtype must be 0 (F32), 1 (F16) or 2 (BF16)");
        size_t count = 1;
        for (int i = 0; i < ndim; ++i) {
            if (dims[i] < 1 || dims[i] > (int64_t)1 << 30 || count > ((size_t)1 << 34) / (size_t)dims[i]) throw Error(SDMI_ERR_INVALID, "unpack_tensor: dimensions must be positive (at most 2^34 elements)");
            count *= (size_t)dims[i];
        }
        if (transform < 0 || transform > 2 || (transform == 1 && ndim != 2) || (transform == 2 && (ndim != 4 || dims[1] >= 32 || dims[1] % 4 == 0)))
            throw Error(SDMI_ERR_INVALID, "unpack_tensor: transform 0 (copy), 1 (a 2-D tensor transposed) or 2 (a [cout,cin,kh,kw] conv, cin < 32 and no multiple of 4, padded to the next multiple of 4 input channels)");
        const size_t n_out = transform == 2 ? count / (size_t)dims[1] * (size_t)((dims[1] + 3) / 4 * 4) : count;
        Engine::Call call(e);
        DevIn dx(e, raw, count * (dtype == 0 ? 4 : 2));
        DevOut dout(e, out, n_out * sizeof(float));
        e.op_unpack_tensor(dx.buf.p, dtype, ndim, dims, transform, dout.f());
        call.finish();
        dout.fetch();
    });
}

int sdmi_op_sampler_step(sdmi_ctx* ctx, const float* eps, const float* latent, int32_t n, int32_t h, int32_t w, double scale, double rescale, const double* row,
                         int32_t depth, int32_t n_hist, const float* q_hist, uint64_t noise_key, uint64_t noise_key2, const float* mask, const float* z0,
                         const float* e0, double blend_prev, double blend_dir, float* latent_out, float* q_out) {
    return guarded([&] {
        Engine& e = eng(ctx);
        if (n <= 0 || h <= 0 || w <= 0) throw Error(SDMI_ERR_INVALID, "sampler_step: bad shape");
        if (!eps || !latent || !row || !latent_out) throw Error(SDMI_ERR_INVALID, "sampler_step: null pointer");
        if (depth != 0 && depth != 1 && depth != 3) throw Error(SDMI_ERR_INVALID, "sampler_step: depth must be 0, 1 or 3");
        if (n_hist < 0 || n_hist > depth || (n_hist && !q_hist) || (depth && !q_out)) throw Error(SDMI_ERR_INVALID, "sampler_step: history does not fit depth");
        if (!(rescale >= 0.0 && rescale <= 1.0)) throw Error(SDMI_ERR_INVALID, "sampler_step: rescale must satisfy 0 <= rescale <= 1");
        if ((!mask) != (!z0) || (!mask) != (!e0)) throw Error(SDMI_ERR_INVALID, "sampler_step: mask, z0 and e0 come together");
        if (row[6] != 0.0 && (depth != 1 || row[5] == 0.0)) throw Error(SDMI_ERR_INVALID, "sampler_step: cz2 needs depth 1 and cz != 0");
        sdmi::SamplerStep c{};
        c.scale = (float)scale;
        c.cx = (float)row[0]; c.ce = (float)row[1]; c.h[0] = (float)row[2]; c.h[1] = (float)row[3]; c.h[2] = (float)row[4];
        c.cz = (float)row[5]; c.cz2 = (float)row[6]; c.qx = (float)row[7]; c.qe = (float)row[8];
        c.blend_prev = (float)blend_prev; c.blend_dir = (float)blend_dir;
        c.n_hist = n_hist;
        const size_t hw = (size_t)h * w, lat = (size_t)n * 4 * hw * sizeof(float);
        Engine::Call call(e);
        DevIn de(e, eps, 2 * lat), dl(e, latent, lat);
        auto dq = dev_in_opt(e, n_hist ? q_hist : nullptr, (size_t)n_hist * lat);
        auto dm = dev_in_opt(e, mask, (size_t)n * hw * sizeof(float));
        auto dz = dev_in_opt(e, z0, lat);
        auto dn = dev_in_opt(e, e0, lat);
        DevOut dout(e, latent_out, lat);
        std::unique_ptr<DevOut> dqo;
        if (depth) dqo.reset(new DevOut(e, q_out, lat));
        e.op_sampler_step(de.f(), dl.f(), n, h, w, c, (float)rescale, depth, dq ? dq->f() : nullptr, noise_key, noise_key2, dm ? dm->f() : nullptr,
                          dz ? dz->f() : nullptr, dn ? dn->f() : nullptr, dout.f(), dqo ? dqo->f() : nullptr);
        call.finish();
        dout.fetch();
        if (dqo) dqo->fetch();
    });
}

int sdmi_bench_conv(sdmi_ctx* ctx, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k,
                    int32_t stride, int32_t upsample2x, int32_t tile_cfg, int32_t splitk, int32_t iters, double* ms_out) {
    return guarded([&] {
        if (!ms_out) throw Error(SDMI_ERR_INVALID, "bench_conv: null output");
        *ms_out = eng(ctx).bench_conv(n, cin, h, w, cout, k, stride, upsample2x ? 1 : 0, tile_cfg, splitk, iters);
    });
}

int sdmi_bench_attention(sdmi_ctx* ctx, int32_t n, int32_t nq, int32_t nk, int32_t n_state, int32_t n_head,
                         int32_t iters, double* ms_out) {
    return guarded([&] {
        if (!ms_out) throw Error(SDMI_ERR_INVALID, "bench_attention: null output");
        *ms_out = eng(ctx).bench_attention(n, nq, nk, n_state, n_head, iters);
    });
}

int sdmi_attention_plan(sdmi_ctx* ctx, int32_t n, int32_t n_head, int32_t nq, int32_t nk, int32_t d_head, int32_t has_mask, sdmi_attn_plan* out) {
    return guarded([&] {
        if (!out) throw Error(SDMI_ERR_INVALID, "attention_plan: null output");
        const sdmi::AttnPlan a = eng(ctx).attention_plan(n, n_head, nq, nk, d_head, has_mask != 0);
        *out = sdmi_attn_plan{};
        out->kernel = a.kernel == sdmi::AttnKernel::Unfused ? 0 : a.kernel == sdmi::AttnKernel::Flash ? 1 : a.kernel == sdmi::AttnKernel::Split ? 2 : 3;
        out->waves = a.waves; out->q_rows = a.q_rows; out->kv_tile = a.kv_tile; out->kv_splits = a.kv_splits;
    });
}

}  // extern "C"
