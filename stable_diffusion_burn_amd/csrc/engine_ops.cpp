// engine_ops.cpp -- the operator-level test and bench entry points of Engine (sdmi_op_*, sdmi_bench_*, sdmi_attention_plan): device pointers, reference
// layouts.  They stage one operator the way the model runs it -- the storage types, packed weights, views and options of the route -- around the primitives of
// engine.cpp.  See engine.hpp.
#include "engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

namespace sdmi {

// =============================================================================
// what the entry points share
// =============================================================================
// runs f when the scope ends, however it ends
template <class F> struct AtExit { F f; ~AtExit() { f(); } };
template <class F> AtExit(F) -> AtExit<F>;

Engine::OpRoute Engine::conv_route(int cin, int cout, int k, int stride, int ups, bool f32, bool refuse) const {
    if (f32) return {false, 0, 0, 0};   // option op_f32 (tests): fp32 weight, input and output at every precision -- what the ControlNet hint convolutions run
    // precision = 2 mirrors the model's ResBlock convs: MXFP8 input, MXFP8 weight, bf16 output
    if (fp8_ && opt_fp8_convs_ && k == 3 && stride == 1 && !ups && cin % 32 == 0 && cout % 8 == 0) return {true, 1, 1, 1};
    // precision = 1 mirrors the model: Cin % 64 == 0 -> bf16 kernel, Cin < 32 -> fp32 kernel emitting bf16, <= 4 output channels (eps / RGB heads) -> fp32 output
    const int wdt = (bf16_ && cin % 64 == 0) ? 1 : 0;
    if (refuse && bf16_ && !wdt && cin >= 32) throw Error(SDMI_ERR_UNSUPPORTED, "bf16 conv2d: Cin must be a multiple of 64 (or < 32)");
    return {false, wdt, wdt, (bf16_ && cout > 4) ? 1 : 0};
}

Engine::OpRoute Engine::lin_route(int cin, int cout) const {
    const bool q8 = fp8_ && opt_fp8_ops_ && cin % 32 == 0 && cout % 8 == 0;   // option fp8_ops (tests): the Linear layer as the fp8_linear path runs it
    const int dt = (q8 || (bf16_ && cin % 64 == 0)) ? 1 : 0;
    return {q8, dt, dt, dt};
}

// wt [cout][cin][k][k] -> the packed weight of the route: MXFP8 with its scales, bf16, or fp32 with its planes (TempSplit) and, for an up-convolution, its phase
// weights as rebuild_folds derives the model's (TempUpFold)
struct Engine::OpConvW {
    ConvW w;
    OpConvW(Engine* e, const float* wt, const float* bias, int cin, int cout, int k, int stride, int ups, const OpRoute& r) {
        w.cin = cin; w.cout = cout; w.k = k; w.dt = r.wdt; w.bias = const_cast<float*>(bias);
        if (r.q8) {
            const int cp = (cin + 127) / 128 * 128;
            bt_.reset(new Buf(e, (size_t)cout * cp * 9)); bs_.reset(new Buf(e, (size_t)cout * cp * 9 / 32));
            SDMI_HIP(launch_pack_conv_weight_fp8(wt, bt_->p, bs_->p, cout, cin, 3, 3, e->stream_));
            w.bt8 = bt_->f(); w.bs8 = bs_->f();
            return;
        }
        bt_.reset(new Buf(e, (size_t)cout * cin * k * k * 4));
        if (w.dt) SDMI_HIP(launch_pack_conv_weight_bf16(wt, bt_->p, cout, cin, k, k, e->stream_));
        else SDMI_HIP(launch_pack_conv_weight(wt, bt_->f(), cout, cin, k, k, e->stream_));
        split_.reset(new TempSplit(e, bt_->f(), w.dt ? 0 : cout, (long long)cin * k * k));
        w.bt = bt_->f();
        fold_.reset(new TempUpFold(e, w, stride, ups));
    }
    OpConvW(const OpConvW&) = delete;
    OpConvW& operator=(const OpConvW&) = delete;
private:
    std::unique_ptr<Buf> bt_, bs_;
    std::unique_ptr<TempSplit> split_;
    std::unique_ptr<TempUpFold> fold_;
};

// wt [cin][cout] -> bt [cout][cin] packed for the route: the MXFP8 pair, bf16, or fp32 with its planes
struct Engine::OpLinW {
    LinW w;
    OpLinW(Engine* e, const float* wt, const float* bias, int cin, int cout, const OpRoute& r) {
        w.cin = cin; w.cout = cout; w.dt = r.wdt; w.bias = const_cast<float*>(bias);
        if (r.q8) {
            const size_t kp = (size_t)(cin + 127) / 128 * 128;
            bt_.reset(new Buf(e, (size_t)cout * kp)); bs_.reset(new Buf(e, (size_t)cout * kp / 32));
            SDMI_HIP(launch_pack_linear_weight_fp8(wt, bt_->p, bs_->p, cin, cout, e->stream_));
            w.bt8 = bt_->f(); w.bs8 = bs_->f();
            return;
        }
        bt_.reset(new Buf(e, (size_t)cin * cout * 4));
        w.bt = bt_->f();
        if (w.dt) SDMI_HIP(launch_pack_linear_weight_bf16(wt, bt_->p, cin, cout, e->stream_));
        else {
            SDMI_HIP(launch_pack_linear_weight(wt, bt_->f(), cin, cout, e->stream_));
            split_.reset(new TempSplit(e, bt_->f(), cout, cin));
        }
    }
    OpLinW(const OpLinW&) = delete;
    OpLinW& operator=(const OpLinW&) = delete;
private:
    std::unique_ptr<Buf> bt_, bs_;
    std::unique_ptr<TempSplit> split_;
};

// n x h x w rows of ld elements, as unet_run allocates the input of an output block: bf16 (dt 1), or at dt 0 fp32 (planes 0 / 1), planes only (2) or both (3);
// filled from the caller's image img [rows][ld] fp32 on the device
struct Engine::OpParent {
    Engine* e; Act a;
    OpParent(Engine* e_, int n, int h, int w, int ld, int dt, int planes, const float* img) : e(e_) {
        a = (!dt && planes > 1) ? e->new_act3(n, h, w, ld, planes) : e->new_act(n, h, w, ld, dt);
        if (dt) SDMI_HIP(launch_f32_to_bf16(img, a.p, a.rows() * ld, e->stream_));
        else {
            if (a.p) SDMI_HIP(hipMemcpyAsync(a.p, img, a.bytes(), hipMemcpyDeviceToDevice, e->stream_));
            if (a.p3) SDMI_HIP(launch_split3_rows(img, a.p3, a.rows(), ld, ld, a.ld3, e->stream_));
        }
    }
    Act slice(int off, int c) const { return Engine::slice(a, off, c); }
    // the WHOLE parent goes back: the caller judges the columns next to the slice (after a refused launch too: what it left behind).  yp: the fp32 / bf16 copy, or
    // the joined planes where they are the only copy; yp3 (may be null): the joined planes next to an fp32 copy
    void give_back(float* yp, float* yp3) const {
        if (a.dt) SDMI_HIP(launch_nhwc_bf16_to_nchw_f32(a.p, yp, (int)a.rows(), a.c, 1, 1, e->stream_));
        else {
            if (a.p) SDMI_HIP(hipMemcpyAsync(yp, a.p, a.bytes(), hipMemcpyDeviceToDevice, e->stream_));
            float* joined = a.p ? yp3 : yp;
            if (a.p3 && joined) SDMI_HIP(launch_join3_rows(a.p3, joined, a.rows(), a.c, a.ld3, a.c, e->stream_));
        }
    }
    void release() { e->release(a); }
};

Act Engine::act_from_nchw(const float* x, int n, int c, int h, int w, int dt) {
    Act a = new_act(n, h, w, c, dt);
    if (dt) SDMI_HIP(launch_nchw_f32_to_nhwc_bf16(x, a.p, n, c, h, w, 1.0f, stream_));
    else SDMI_HIP(launch_nchw_to_nhwc(x, a.p, n, c, h, w, 1.0f, stream_));
    return a;
}

void Engine::act_to_nchw(const Act& a, float* out) {
    if (a.dt) SDMI_HIP(launch_nhwc_bf16_to_nchw_f32(a.p, out, a.n, a.c, a.h, a.w, stream_));
    else SDMI_HIP(launch_nhwc_to_nchw(a.p, out, a.n, a.c, a.h, a.w, stream_));
}

void Engine::rows_to_f32(const void* bf16_rows, float* out, long long rows, int c) {
    SDMI_HIP(launch_nhwc_bf16_to_nchw_f32(bf16_rows, out, (int)rows, c, 1, 1, stream_));
}

// per-sample key counts: a device copy for the kernels, the host array for the unfused path's per-sample loop (as unet_prepare keeps them)
const int* Engine::kv_len_to_dev(std::unique_ptr<Buf>& b, const int* kv_len_host, int n) {
    if (!kv_len_host) return nullptr;
    b.reset(new Buf(this, (size_t)n * sizeof(int)));
    SDMI_HIP(hipMemcpyAsync(b->p, kv_len_host, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream_));
    return reinterpret_cast<const int*>(b->p);
}

// precision >= 1: the boundary is fp32, the kernel sees bf16 tensors
void Engine::qkv_to_bf16(const float*& q, const float*& k, const float*& v, long long qe, long long ke, int dh, std::unique_ptr<Buf> (&bufs)[3]) {
    bufs[0].reset(new Buf(this, qe * 2)); bufs[1].reset(new Buf(this, ke * 2)); bufs[2].reset(new Buf(this, ke * 2));
    if (q_prescaled(1, dh)) SDMI_HIP(launch_f32_to_bf16_scaled(q, bufs[0]->p, qe, attn_bf16_q_scale(dh), stream_));   // Engine::attention's q convention
    else SDMI_HIP(launch_f32_to_bf16(q, bufs[0]->p, qe, stream_));
    SDMI_HIP(launch_f32_to_bf16(k, bufs[1]->p, ke, stream_));
    SDMI_HIP(launch_f32_to_bf16(v, bufs[2]->p, ke, stream_));
    q = bufs[0]->f(); k = bufs[1]->f(); v = bufs[2]->f();
}

// the conversion kernel on its own (tests: sdmi_op_unpack_tensor); raw / out: device pointers
void Engine::op_unpack_tensor(const void* raw, int dtype, int ndim, const int64_t* dims, int transform, float* out) {
    long long d0, d1;
    if (transform == 1) { d0 = dims[0]; d1 = dims[1]; }
    else if (transform == 2) { d0 = dims[0]; d1 = dims[2] * dims[3]; }
    else { d0 = 1; for (int i = 0; i < ndim; ++i) d0 *= dims[i]; d1 = 1; }
    SDMI_LAUNCH(launch_unpack_tensor(raw, dtype, transform, d0, d1, out, stream_, transform == 2 ? (int)dims[1] : 3));
}

bool Engine::op_freeu(float* parent, int n, int c, int h, int w, int ld, int cx, int version, float b, float s, float* parent3) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || cx <= 0 || cx >= c || ld < c) throw Error(SDMI_ERR_INVALID, "op_freeu: bad shape");
    FreeU f; f.version = version; f.b1 = f.b2 = b; f.s1 = f.s2 = s;
    check_freeu(f);
    if (version < 1) throw Error(SDMI_ERR_INVALID, "op_freeu: version must be 1 or 2");
    const int g = freeu_granule(), dt = edt();
    if (cx % (2 * g) || (c - cx) % g || (ld * (dt ? 2 : 4)) % 16) throw Error(SDMI_ERR_UNSUPPORTED, "op_freeu: cx / 2 and c - cx must be multiples of " + std::to_string(g));
    if (!freeu_filter_size_ok(h, w)) throw Error(SDMI_ERR_UNSUPPORTED, "op_freeu: the size is beyond what the filter kernel's tables hold");
    const bool planes = !dt && plane_gemm(c, c) && ld % 32 == 0;   // (cx and c - cx are multiples of 32 here)
    OpParent par(this, n, h, w, ld, dt, planes ? 3 : 0, parent);   // the cat is its first c columns
    const Act cat = par.slice(0, c);
    Act catv = cat; catv.view = false;   // (slice refuses a view of a view; the cuts below are taken on the same rows)
    const Act* cats[1] = {&catv};
    freeu_filter(cats, &cx, &s, 1);
    freeu_backbone(catv, cx, b, version);
    par.give_back(parent, parent3);
    par.release();
    return planes;
}

void Engine::op_resize(const float* x_nchw, int n, int h, int w, int oh, int ow, int mode, int antialias, float* out_nchw) {
    if (n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) throw Error(SDMI_ERR_INVALID, "resize: sizes must be positive");
    Buf xin(this, (size_t)n * h * w * 16), xout(this, (size_t)n * oh * ow * 16);
    SDMI_LAUNCH(launch_nchw_to_nhwc(x_nchw, xin.f(), n, 4, h, w, 1.0f, stream_));
    resize_nhwc4(xin.f(), n, h, w, oh, ow, mode, antialias, xout.f());
    SDMI_LAUNCH(launch_nhwc_to_nchw(xout.f(), out_nchw, n, 4, oh, ow, stream_));
}

void Engine::op_sampler_step(const float* eps, const float* latent, int n, int h, int w, const SamplerStep& c, float rescale, int depth, const float* q_hist,
                             uint64_t noise_key, uint64_t noise_key2, const float* mask, const float* z0, const float* e0, float* latent_out, float* q_out) {
    const size_t img = (size_t)h * w * 16, half = (size_t)n * img;
    const long long per_half = (long long)n * h * w * 4;
    Buf de(this, 2 * half), dl(this, half), du(this, 2 * half), dq(this, 3 * half), dqo(this, half), dz(this, half), dn(this, half);
    auto to_nhwc = [&](const float* src, float* dst, int images) {
        SDMI_LAUNCH(launch_nchw_to_nhwc(src, dst, images, 4, h, w, 1.0f, stream_));
    };
    to_nhwc(eps, de.f(), 2 * n);
    to_nhwc(latent, dl.f(), n);
    const float* q_prev[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < c.n_hist; ++k) {
        to_nhwc(q_hist + (size_t)k * per_half, dq.f() + (size_t)k * per_half, n);
        q_prev[k] = dq.f() + (size_t)k * per_half;
    }
    if (mask) { to_nhwc(z0, dz.f(), n); to_nhwc(e0, dn.f(), n); }
    SDMI_LAUNCH(launch_sampler_step(de.f(), dl.f(), du.f(), per_half, (long long)h * w, c, rescale, depth, q_prev, depth ? dqo.f() : nullptr, noise_key, noise_key2,
                                    mask, mask ? dz.f() : nullptr, mask ? dn.f() : nullptr, stream_));
    SDMI_LAUNCH(launch_nhwc_to_nchw(dl.f(), latent_out, n, 4, h, w, stream_));
    if (depth) SDMI_LAUNCH(launch_nhwc_to_nchw(dqo.f(), q_out, n, 4, h, w, stream_));
}

void Engine::qkv_attention_dev(const float* q, const float* k, const float* v, const float* mask, int mask_ld, int n,
                               int nq, int nk, int n_state, int n_head, float* out, const int* kv_len_host) {
    if (n <= 0 || nq <= 0 || nk <= 0 || n_head <= 0 || n_state % n_head) throw Error(SDMI_ERR_INVALID, "qkv_attention: bad shape");
    if (mask && mask_ld < nk) throw Error(SDMI_ERR_INVALID, "qkv_attention: mask_ld < nk");
    if (kv_len_host)
        for (int b = 0; b < n; ++b)
            if (kv_len_host[b] < 1 || kv_len_host[b] > nk) throw Error(SDMI_ERR_INVALID, "qkv_attention: kv_len entries must lie in 1 .. nk");
    std::unique_ptr<Buf> kl, qkv[3];
    const int* kv_len_dev = kv_len_to_dev(kl, kv_len_host, n);
    const long long q_bs = (long long)nq * n_state, k_bs = (long long)nk * n_state;
    const int dh = n_state / n_head;
    auto run = [&](float* o, int dt, void* o3) {   // q, k, v: dense, fp32 or already converted
        Attn at;
        at.q = attn_rows(rows_view(q, (long long)n * nq, n_state, dt), nq);
        at.k = attn_rows(rows_view(k, (long long)n * nk, n_state, dt), nk);
        at.v = attn_rows(rows_view(v, (long long)n * nk, n_state, dt), nk);
        at.o = attn_rows(rows_view(o, (long long)n * nq, n_state, dt), nq); at.o3 = o3;
        at.n = n; at.nq = nq; at.nk = nk; at.n_head = n_head; at.d_head = dh;
        at.kv_len_dev = kv_len_dev; at.kv_len_host = kv_len_host;
        at.mask = mask; at.mask_ld = dt ? 0 : mask_ld; at.dt = dt; at.q_log2 = q_prescaled(dt, dh);
        attention(at);
    };
    if (bf16_ && !mask) {
        qkv_to_bf16(q, k, v, n * q_bs, n * k_bs, dh, qkv);
        Buf oh(this, n * q_bs * 2);
        run(oh.f(), 1, nullptr);
        rows_to_f32(oh.p, out, (long long)n * nq, n_state);
    } else if (plane_gemm(n_state, n_state) && attn_supported_head_dim(dh)) {   // option gemm_planes: the kernels' plane-writing epilogue, joined back
        Buf o3(this, (size_t)n * nq * (n_state / 32) * 192);
        run(nullptr, 0, o3.p);
        SDMI_HIP(launch_join3_rows(o3.p, out, (long long)n * nq, n_state, (long long)(n_state / 32) * 192, n_state, stream_));
    } else {
        run(out, 0, nullptr);
    }
}

void Engine::check_qkv_attention_view(const sdmi_attn_view& view, bool has_mask, int mask_ld, const int* kv_len_host, int n, int nq, int nk, int n_state,
                                      int n_head) const {
    if (n <= 0 || nq <= 0 || nk <= 0 || n_state <= 0 || n_head <= 0 || n_state % n_head) throw Error(SDMI_ERR_INVALID, "qkv_attention_view: bad shape");
    if (has_mask && mask_ld < nk) throw Error(SDMI_ERR_INVALID, "qkv_attention_view: mask_ld < nk");
    if (has_mask && kv_len_host) throw Error(SDMI_ERR_INVALID, "qkv_attention_view: a mask or kv_len, not both");
    if (kv_len_host)
        for (int b = 0; b < n; ++b)
            if (kv_len_host[b] < 1 || kv_len_host[b] > nk) throw Error(SDMI_ERR_INVALID, "qkv_attention_view: kv_len entries must lie in 1 .. nk");
    AttnViewIn in{};
    in.n = n; in.nq = nq; in.nk = nk; in.n_state = n_state; in.bf16 = (bf16_ && !has_mask) ? 1 : 0;
    in.q = {view.q_ld, view.q_off, view.q_rows}; in.k = {view.k_ld, view.k_off, view.k_rows}; in.v = {view.v_ld, view.v_off, view.v_rows};
    in.packed = view.packed != 0; in.out = {view.out_ld, view.out_off, view.out_rows}; in.out_planes = view.out_planes != 0;
    check_attention_view(in);
}

// The operands take qkv_attention_dev's way to the device (the same conversions in the same order on the dense tensors), then are copied row by row into
// parents full of in_fill; attention() gets the slices' bases, row strides and batch strides.
void Engine::op_qkv_attention_view(const float* q, const float* k, const float* v, const float* mask, int mask_ld, const int* kv_len_host, int n, int nq, int nk,
                                   int n_state, int n_head, const sdmi_attn_view& view, float* parent) {
    check_qkv_attention_view(view, mask != nullptr, mask_ld, kv_len_host, n, nq, nk, n_state, n_head);
    const int dt = (bf16_ && !mask) ? 1 : 0, dh = n_state / n_head;
    const size_t es = dt ? 2 : 4;
    std::unique_ptr<Buf> kl, qkv[3];
    const int* kv_len_dev = kv_len_to_dev(kl, kv_len_host, n);
    if (dt) qkv_to_bf16(q, k, v, (long long)n * nq * n_state, (long long)n * nk * n_state, dh, qkv);   // precision >= 1: as qkv_attention_dev converts them
    // in_fill in the parents' storage type (bf16: round to nearest even, a NaN stays one)
    uint32_t fill32;
    std::memcpy(&fill32, &view.in_fill, 4);
    const uint16_t fill16 = (fill32 & 0x7FFFFFFFu) > 0x7F800000u ? (uint16_t)((fill32 >> 16) | 0x40) : (uint16_t)((fill32 + 0x7FFFu + ((fill32 >> 16) & 1u)) >> 16);
    auto new_parent = [&](int ld, int rows) {
        const size_t elems = (size_t)n * rows * ld;
        std::unique_ptr<Buf> b(new Buf(this, elems * es));
        if (dt) SDMI_HIP(hipMemsetD16Async(b->p, fill16, elems, stream_));
        else SDMI_HIP(hipMemsetD32Async(b->p, (int)fill32, elems, stream_));
        return b;
    };
    auto scatter = [&](const float* dense, int used, Buf& par, int ld, int off, int rows) {   // -> the slice's base
        float* base = adv(par.f(), off, dt);
        for (int b = 0; b < n; ++b)
            SDMI_HIP(hipMemcpy2DAsync(adv(base, (long long)b * rows * ld, dt), (size_t)ld * es, adv(dense, (long long)b * used * n_state, dt), (size_t)n_state * es,
                                      (size_t)n_state * es, (size_t)used, hipMemcpyDeviceToDevice, stream_));
        return base;
    };
    std::unique_ptr<Buf> pq = new_parent(view.q_ld, view.q_rows), pk, pv;
    if (!view.packed) { pk = new_parent(view.k_ld, view.k_rows); pv = new_parent(view.v_ld, view.v_rows); }
    const float* qs = scatter(q, nq, *pq, view.q_ld, view.q_off, view.q_rows);
    const float* ks = scatter(k, nk, view.packed ? *pq : *pk, view.k_ld, view.k_off, view.k_rows);
    const float* vs = scatter(v, nk, view.packed ? *pq : *pv, view.v_ld, view.v_off, view.v_rows);
    const long long q_bs = (long long)view.q_rows * view.q_ld, k_bs = (long long)view.k_rows * view.k_ld, v_bs = (long long)view.v_rows * view.v_ld;
    const long long o_bs = (long long)view.out_rows * view.out_ld;
    auto run = [&](float* o, int mld, void* o3) {
        Attn at;
        at.q = AttnOperand{qs, view.q_ld, q_bs}; at.k = AttnOperand{ks, view.k_ld, k_bs}; at.v = AttnOperand{vs, view.v_ld, v_bs};
        at.o = AttnOperand{o, view.out_ld, o_bs}; at.o3 = o3;
        at.n = n; at.nq = nq; at.nk = nk; at.n_head = n_head; at.d_head = dh;
        at.kv_len_dev = kv_len_dev; at.kv_len_host = kv_len_host;
        at.mask = mask; at.mask_ld = mld; at.dt = dt; at.q_log2 = q_prescaled(dt, dh);
        attention(at);
    };
    if (view.out_planes) {   // the kernels' plane-writing epilogue, joined back (dense: check_attention_view); what cannot write planes is plan_attention's to refuse
        Buf o3(this, (size_t)n * nq * (n_state / 32) * 192 + 256);
        run(nullptr, mask_ld, o3.p);
        SDMI_HIP(launch_join3_rows(o3.p, parent, (long long)n * nq, n_state, (long long)(n_state / 32) * 192, n_state, stream_));
    } else if (dt) {
        OpParent y(this, n, view.out_rows, 1, view.out_ld, 1, 0, parent);
        run(y.slice(view.out_off, n_state).p, 0, nullptr);
        y.give_back(parent, nullptr);
        y.release();
    } else {
        run(parent + view.out_off, mask_ld, nullptr);
    }
}

// =============================================================================
// operator-level entry points (device pointers, reference layouts)
// =============================================================================
void Engine::op_group_norm(const float* x, const float* gamma, const float* beta, int n, int c, int h, int w,
                           int groups, float eps, bool silu, float* out) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || groups <= 0 || c % groups || c % 4) throw Error(SDMI_ERR_INVALID, "group_norm: bad shape");
    const int dt = (bf16_ && c % 8 == 0) ? 1 : 0;
    Act a = act_from_nchw(x, n, c, h, w, dt), b = new_act(n, h, w, c, dt);
    if (dt) {
        Buf part(this, gn_partials_bytes_bf16(n, h * w, c, gn_tune_));
        SDMI_HIP(launch_group_norm_bf16(a.p, b.p, gamma, beta, n, h * w, c, c, groups, eps, silu, part.p, stream_, gn_tune_));
    } else {
        Buf part(this, gn_partials_bytes(n, h * w, c, opt_gn32_min_wgs_));
        if (plane_gemm(c, c)) {   // option gemm_planes: the plane-writing form of the kernel, joined back to fp32 (exact)
            Buf y3(this, (size_t)n * h * w * (c / 32) * 192);
            SDMI_HIP(launch_group_norm_planes(a.p, y3.p, gamma, beta, n, h * w, c, c, groups, eps, silu, part.p, stream_, opt_gn32_min_wgs_));
            SDMI_HIP(launch_join3_rows(y3.p, b.p, (long long)n * h * w, c, (long long)(c / 32) * 192, c, stream_));
        } else {
            SDMI_HIP(launch_group_norm(a.p, b.p, gamma, beta, n, h * w, c, c, groups, eps, silu, part.p, stream_, opt_gn32_min_wgs_));
        }
    }
    act_to_nchw(b, out);
    release(a); release(b);
}

// GroupNorm(+SiLU) with MXFP8 output (precision = 2), returned dequantised: out [n,c,h,w] fp32
void Engine::op_group_norm_fp8(const float* x, const float* gamma, const float* beta, int n, int c, int h, int w, int groups, float eps,
                               bool silu, float* out) {
    if (!fp8_) throw Error(SDMI_ERR_STATE, "group_norm_fp8 needs a precision = 2 context");
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || groups <= 0 || c % groups || c % 32) throw Error(SDMI_ERR_INVALID, "group_norm_fp8: bad shape");
    Act a = act_from_nchw(x, n, c, h, w, 1);
    ActQ q = new_actq(n, h, w, c);
    Buf part(this, gn_partials_bytes_bf16(n, h * w, c, gn_tune_));
    SDMI_HIP(launch_group_norm_fp8(a.p, q.q, q.s, gamma, beta, n, h * w, c, c, groups, eps, silu, part.p, stream_, &gn_tune_));
    Act d = new_act(n, h, w, c, 0);
    SDMI_HIP(launch_dequant_fp8(q.q, q.s, d.p, d.rows(), c, stream_));
    act_to_nchw(d, out);
    release(a); release(q); release(d);
}

void Engine::op_layer_norm(const float* x, const float* gamma, const float* beta, int rows, int c, float eps, float* out) {
    if (rows <= 0 || c <= 0) throw Error(SDMI_ERR_INVALID, "layer_norm: bad shape");
    if (fp8_ && opt_fp8_ops_ && c % 32 == 0) {   // option fp8_ops (tests): the quantising LayerNorm of the fp8_linear path, dequantised
        Buf xh(this, (size_t)rows * c * 2);
        SDMI_HIP(launch_f32_to_bf16(x, xh.p, (long long)rows * c, stream_));
        ActQ q = new_rowsq(rows, c);
        SDMI_HIP(launch_layer_norm_fp8(xh.p, q.q, q.s, gamma, beta, rows, c, eps, stream_));
        SDMI_HIP(launch_dequant_fp8(q.q, q.s, out, rows, c, stream_));
        release(q);
        return;
    }
    if (bf16_ && c % 8 == 0) {
        Buf xh(this, (size_t)rows * c * 2), yh(this, (size_t)rows * c * 2);
        SDMI_HIP(launch_f32_to_bf16(x, xh.p, (long long)rows * c, stream_));
        SDMI_HIP(launch_layer_norm_bf16(xh.p, yh.p, gamma, beta, rows, c, eps, stream_));
        rows_to_f32(yh.p, out, rows, c);
        return;
    }
    if (plane_gemm(c, c)) {
        Buf y3(this, (size_t)rows * (c / 32) * 192);
        SDMI_HIP(launch_layer_norm_planes(x, y3.p, gamma, beta, rows, c, eps, stream_));
        SDMI_HIP(launch_join3_rows(y3.p, out, rows, c, (long long)(c / 32) * 192, c, stream_));
        return;
    }
    SDMI_HIP(launch_layer_norm(x, out, gamma, beta, rows, c, eps, stream_));
}

const float* Engine::stage_epi(std::unique_ptr<Buf>& b, const float* host, long long rows, int c, int ld, int dt, long long nchw_hw) {
    if (ld < c) throw Error(SDMI_ERR_INVALID, "epilogue operand: row stride below the channel count");
    const size_t es = dt ? 2 : 4, bytes = (size_t)rows * ld * es;
    std::vector<unsigned char> img(bytes);
    for (long long r = 0; r < rows; ++r)
        for (int j = 0; j < ld; ++j) {
            const float v = j >= c ? std::nanf("") : nchw_hw ? host[((r / nchw_hw) * c + j) * nchw_hw + r % nchw_hw] : host[r * c + j];
            unsigned char* d = img.data() + ((size_t)r * ld + j) * es;
            if (dt) {
                uint32_t u;
                std::memcpy(&u, &v, 4);
                const uint16_t hb = std::isnan(v) ? (uint16_t)0x7FC0 : (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
                std::memcpy(d, &hb, 2);
            } else std::memcpy(d, &v, 4);
        }
    b.reset(new Buf(this, bytes + 16));
    unsigned char* dst = static_cast<unsigned char*>(b->p) + (opt_op_misalign_ ? es : 0);
    SDMI_HIP(hipMemcpyAsync(dst, img.data(), bytes, hipMemcpyHostToDevice, stream_));
    SDMI_HIP(hipStreamSynchronize(stream_));     // (img is a local)
    return reinterpret_cast<const float*>(dst);
}

void Engine::op_conv_run(const OpRoute& r, const float* wt, const float* bias, int k, int stride, int ups, const EpiOps* epi, const Act& xs, Act& ys, const Act* self_resid) {
    const int cout = ys.c;
    // the caller's time-embedding row (fp32, as the model's) and residual (in the output's storage type, rows ho x wo pixels): epi != null
    std::unique_ptr<Buf> tb, rb;
    const float* temb = (epi && epi->temb) ? stage_epi(tb, epi->temb, epi->temb_stride ? ys.n : 1, cout, epi->temb_stride ? epi->temb_stride : cout, 0) : nullptr;
    Act res;
    if (epi && epi->resid) {
        if (!ys.p) throw Error(SDMI_ERR_INVALID, "view: a residual needs the output as fp32");
        res = ys;
        res.view = true; res.p3 = nullptr;
        res.ld = epi->resid_ld ? epi->resid_ld : cout;
        res.p = const_cast<float*>(stage_epi(rb, epi->resid, ys.rows(), cout, res.ld, ys.dt, (long long)ys.h * ys.w));
    }
    const Act* resid = res.p ? &res : self_resid;
    OpConvW w(this, wt, bias, xs.c, cout, k, stride, ups, r);
    if (r.q8) {
        ActQ q = new_actq(xs.n, xs.h, xs.w, xs.c);
        if (xs.dt) quantize(xs, q);   // a bf16 slice -> MXFP8, as res_block's shortcut and conv_raw do
        else SDMI_HIP(launch_quantize_fp8(xs.p, q.q, q.s, xs.rows(), xs.c, stream_));   // the fp32 argument (the model gets its MXFP8 input from the fused GroupNorm)
        conv_fp8(w.w, q, ys, temb, resid, 1, 0, epi ? epi->temb_stride : 0);
        release(q);
    } else {
        conv(w.w, xs, ys, stride, ups, temb, epi ? epi->temb_stride : 0, resid);
    }
}

void Engine::op_conv2d(const float* x, const float* wt, const float* bias, int n, int cin, int h, int wd, int cout,
                       int k, int stride, int pad, int ups, float* out, const EpiOps* epi) {
    if (!(k == 1 || k == 3) || pad != (k == 3 ? 1 : 0) || !(stride == 1 || stride == 2))
        throw Error(SDMI_ERR_UNSUPPORTED, "conv2d: only 3x3 pad 1 / 1x1 pad 0, stride 1|2 are on the hot path");
    if (!(cin % 32 == 0 || (cin < 32 && cin % 4 == 0))) throw Error(SDMI_ERR_UNSUPPORTED, "conv2d: Cin must be a multiple of 32, or < 32 and a multiple of 4");
    if (epi && epi->temb_stride && epi->temb_stride < cout) throw Error(SDMI_ERR_INVALID, "conv2d: temb_stride below cout");
    const OpRoute r = conv_route(cin, cout, k, stride, ups, opt_op_f32_ != 0);
    int ho, wo;
    conv_out_hw(h, wd, k, stride, pad, ups, &ho, &wo);
    Act a = act_from_nchw(x, n, cin, h, wd, r.q8 ? 0 : r.xdt);   // (MXFP8: quantised from the fp32 argument)
    Act y = new_act(n, ho, wo, cout, r.ydt);
    // option op_resid (tests): out = conv(x) + x through the GEMM's residual epilogue, where the shapes allow it
    const bool with_resid = !r.q8 && opt_op_resid_ && cin == cout && stride == 1 && !ups && a.dt == y.dt;
    op_conv_run(r, wt, bias, k, stride, ups, epi, a, y, with_resid ? &a : nullptr);
    act_to_nchw(y, out);
    release(a); release(y);
}

// conv3x3(h, w_out) + b_out + conv1x1(x, w_skip) + b_skip as Engine::res_block computes the tail of a ResBlock with a shortcut: both inputs as planes, option skip_slices
// = 1 -> conv_pair (an error where it declines: no quiet other path), 0 -> the two launches.  out / out3 [n,cout,h,w]; out3 (may be null): the result also written
// as planes by the same launch and joined back (exact).
void Engine::op_conv2d_pair(const float* x, const float* hp, const float* w_skip, const float* b_skip, const float* w_out, const float* b_out, int n, int cin_x, int cout,
                            int h, int wd, float* out, float* out3) {
    if (n <= 0 || h <= 0 || wd <= 0 || cin_x <= 0 || cout <= 0) throw Error(SDMI_ERR_INVALID, "conv2d_pair: bad shape");
    if (bf16_ || !plane_gemm(cin_x, cout) || !plane_gemm(cout, cout)) throw Error(SDMI_ERR_UNSUPPORTED, "conv2d_pair: the fp32 plane kernels only (channels in multiples of 32)");
    const OpRoute r{false, 0, 0, 0};
    OpConvW w_o(this, w_out, b_out, cout, cout, 3, 1, 0, r), w_s(this, w_skip, b_skip, cin_x, cout, 1, 1, 0, r);
    Act ax = new_act3(n, h, wd, cin_x, 3), ah = new_act3(n, h, wd, cout, 3);
    SDMI_HIP(launch_nchw_to_nhwc(x, ax.p, n, cin_x, h, wd, 1.0f, stream_));
    SDMI_HIP(launch_nchw_to_nhwc(hp, ah.p, n, cout, h, wd, 1.0f, stream_));
    SDMI_HIP(launch_split3_rows(ax.p, ax.p3, ax.rows(), cin_x, cin_x, ax.ld3, stream_));
    SDMI_HIP(launch_split3_rows(ah.p, ah.p3, ah.rows(), cout, cout, ah.ld3, stream_));
    Act y = new_act3(n, h, wd, cout, out3 ? 3 : 1);
    if (opt_skip_slices_) {
        if (!conv_pair(w_o.w, ah, w_s.w, ax, y)) throw Error(SDMI_ERR_UNSUPPORTED, "conv2d_pair: this shape / these options do not pair (skip_slices=0 runs the two launches)");
    } else {
        Act sk = y; sk.p3 = nullptr; sk.view = true;
        conv(w_s.w, ax, sk, 1, 0, nullptr, 0, nullptr);
        conv(w_o.w, ah, y, 1, 0, nullptr, 0, &sk);
    }
    SDMI_HIP(launch_nhwc_to_nchw(y.p, out, n, cout, h, wd, stream_));
    if (out3) {
        Act j = new_act(n, h, wd, cout);
        SDMI_HIP(launch_join3_rows(y.p3, j.p, y.rows(), cout, y.ld3, cout, stream_));
        SDMI_HIP(launch_nhwc_to_nchw(j.p, out3, n, cout, h, wd, stream_));
        release(j);
    }
    release(ax); release(ah); release(y);
}

void Engine::op_linear_run(const OpRoute& r, const float* x, const float* wt, const float* bias, int rows, int cin, int cout, float* C, int ldc, const float* resid, int ldr,
                           bool self_resid) {
    std::unique_ptr<Buf> xh;
    auto x_bf16 = [&] {
        xh.reset(new Buf(this, (size_t)rows * cin * 2));
        SDMI_HIP(launch_f32_to_bf16(x, xh->p, (long long)rows * cin, stream_));
        return xh->f();
    };
    if (r.q8) {
        const Act xa = rows_view(x_bf16(), rows, cin, 1), ra = rows_view(resid, rows, cout, 1, ldr);
        OpLinW w(this, wt, bias, cin, cout, r);
        ActQ q = new_rowsq(rows, cin);
        quantize(xa, q);
        linear(w.w, q, rows_view(C, rows, cout, 1, ldc), resid ? &ra : nullptr);
        release(q);
        return;
    }
    OpLinW w(this, wt, bias, cin, cout, r);
    const Act xa = rows_view(r.xdt ? x_bf16() : x, rows, cin, r.xdt);
    const Act ra = resid ? rows_view(resid, rows, cout, r.xdt, ldr) : xa;
    linear(w.w, xa, rows_view(C, rows, cout, r.xdt, ldc), (resid || self_resid) ? &ra : nullptr);
}

void Engine::op_linear(const float* x, const float* wt, const float* bias, int rows, int cin, int cout, float* out, const EpiOps* epi) {
    const OpRoute r = lin_route(cin, cout);
    // the caller's residual (epi != null) in the storage type of the route: bf16 for the bf16 / MXFP8 kernels, fp32 otherwise
    const int rld = (epi && epi->resid) ? (epi->resid_ld ? epi->resid_ld : cout) : 0;
    std::unique_ptr<Buf> rb;
    const float* resid = rld ? stage_epi(rb, epi->resid, rows, cout, rld, r.ydt) : nullptr;
    const bool with_resid = opt_op_resid_ && cin == cout;   // option op_resid (tests): out = x W + b + x through the residual epilogue
    if (r.ydt) {
        Buf yh(this, (size_t)rows * cout * 2);
        op_linear_run(r, x, wt, bias, rows, cin, cout, yh.f(), cout, resid, rld, with_resid);
        rows_to_f32(yh.p, out, rows, cout);
    } else {
        op_linear_run(r, x, wt, bias, rows, cin, cout, out, cout, resid, rld, with_resid);
    }
}

// ---- the same operators on channel-slice views (tests: sdmi_op_*_view) -------------------------------------------------------------------------------
void Engine::check_view(const sdmi_op_view& v, int cin, int cout) {
    if (v.in_ld < cin || v.in_off < 0 || v.in_off + cin > v.in_ld || v.out_ld < cout || v.out_off < 0 || v.out_off + cout > v.out_ld ||
        v.in_planes < 0 || v.in_planes > 3 || v.out_planes < 0 || v.out_planes > 3)
        throw Error(SDMI_ERR_INVALID, "view: need 0 <= off, off + c <= ld and planes in 0 .. 3");
}

void Engine::op_conv2d_view(const float* xp, const float* wt, const float* bias, int n, int cin, int h, int wd, int cout, int k, int stride, int pad, int ups,
                            const sdmi_op_view& v, const EpiOps* epi, float* yp, float* yp3) {
    check_view(v, cin, cout);
    if (!(k == 1 || k == 3) || pad != (k == 3 ? 1 : 0) || !(stride == 1 || stride == 2))
        throw Error(SDMI_ERR_UNSUPPORTED, "conv2d: only 3x3 pad 1 / 1x1 pad 0, stride 1|2 are on the hot path");
    if (!(cin % 32 == 0 || (cin < 32 && cin % 4 == 0))) throw Error(SDMI_ERR_UNSUPPORTED, "conv2d: Cin must be a multiple of 32, or < 32 and a multiple of 4");
    if (epi && epi->temb_stride && epi->temb_stride < cout) throw Error(SDMI_ERR_INVALID, "conv2d: temb_stride below cout");
    const OpRoute r = conv_route(cin, cout, k, stride, ups);
    int ho, wo;
    conv_out_hw(h, wd, k, stride, pad, ups, &ho, &wo);
    if ((r.xdt && v.in_planes > 1) || (r.ydt && v.out_planes > 1)) throw Error(SDMI_ERR_INVALID, "view: planes are an fp32 format");
    OpParent a(this, n, h, wd, v.in_ld, r.xdt, v.in_planes, xp), y(this, n, ho, wo, v.out_ld, r.ydt, v.out_planes, yp);
    try {
        Act xs = a.slice(v.in_off, cin), ys = y.slice(v.out_off, cout);
        op_conv_run(r, wt, bias, k, stride, ups, epi, xs, ys, nullptr);
    } catch (...) {
        try { y.give_back(yp, yp3); } catch (...) {}
        throw;
    }
    y.give_back(yp, yp3);
    a.release(); y.release();
}

void Engine::op_linear_view(const float* x, const float* wt, const float* bias, int rows, int cin, int cout, const sdmi_op_view& v, const EpiOps* epi, float* yp) {
    check_view(v, cin, cout);
    if (v.in_ld != cin || v.in_off || v.in_planes > 1 || v.out_planes > 1)
        throw Error(SDMI_ERR_UNSUPPORTED, "linear view: Engine::gemm reads dense rows and writes fp32 / bf16 slices only");
    const int rld = (epi && epi->resid) ? (epi->resid_ld ? epi->resid_ld : cout) : 0;
    const OpRoute r = lin_route(cin, cout);
    OpParent y(this, 1, 1, rows, v.out_ld, r.ydt, 0, yp);
    try {
        Act ys = y.slice(v.out_off, cout);
        std::unique_ptr<Buf> rb;
        const float* resid = rld ? stage_epi(rb, epi->resid, rows, cout, rld, r.ydt) : nullptr;
        op_linear_run(r, x, wt, bias, rows, cin, cout, ys.p, ys.stride(), resid, rld, false);
    } catch (...) {
        try { y.give_back(yp, nullptr); } catch (...) {}
        throw;
    }
    y.give_back(yp, nullptr);
    y.release();
}

void Engine::op_group_norm_view(const float* xp, const float* gamma, const float* beta, int n, int c, int h, int w, int groups, float eps, bool silu,
                                const sdmi_op_view& v, int form, float* out) {
    check_view(v, c, c);
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || c % 32 || form < 0 || form > 2) throw Error(SDMI_ERR_INVALID, "group_norm view: bad shape");
    if (groups != 32) throw Error(SDMI_ERR_UNSUPPORTED, "group_norm view: Engine::group_norm normalises 32 groups");
    if ((form == 1 && bf16_) || (form == 2 && !fp8_)) throw Error(SDMI_ERR_STATE, "group_norm view: planes need precision 0, MXFP8 output precision 2");
    const int dt = bf16_ ? 1 : 0;
    if (dt && v.in_planes > 1) throw Error(SDMI_ERR_INVALID, "view: planes are an fp32 format");
    OpParent a(this, n, h, w, v.in_ld, dt, v.in_planes > 1 ? 3 : 0, xp);
    Act xs = a.slice(v.in_off, c);
    NormW nw; nw.gamma = const_cast<float*>(gamma); nw.beta = const_cast<float*>(beta); nw.c = c; nw.eps = eps;
    if (form == 2) {
        ActQ q = new_actq(n, h, w, c);
        group_norm_fp8(nw, xs, q, silu);
        Act d = new_act(n, h, w, c, 0);
        SDMI_HIP(launch_dequant_fp8(q.q, q.s, d.p, d.rows(), c, stream_));
        act_to_nchw(d, out);
        release(q); release(d);
    } else if (form == 1) {
        Act b3 = new_act3(n, h, w, c, 2), b = new_act(n, h, w, c, 0);
        group_norm(nw, xs, b3, silu);
        SDMI_HIP(launch_join3_rows(b3.p3, b.p, b.rows(), c, b3.ld3, c, stream_));
        act_to_nchw(b, out);
        release(b3); release(b);
    } else {
        Act b = new_act(n, h, w, c, dt);
        group_norm(nw, xs, b, silu);
        act_to_nchw(b, out);
        release(b);
    }
    a.release();
}

void Engine::op_cat_chain(const float* x, const float* w_x, const float* b_x, const float* w_skip, const float* b_skip, const float* gamma, const float* beta,
                          int n, int cin, int h, int wd, int cx, int cskip, float eps, bool silu, bool dense, float* out) {
    if (n <= 0 || h <= 0 || wd <= 0 || cin <= 0 || cx <= 0 || cskip <= 0 || (cx + cskip) % 32) throw Error(SDMI_ERR_INVALID, "cat_chain: bad shape");
    const int dt = bf16_ ? 1 : 0, ctot = cx + cskip;
    if (cin % (dt ? 64 : 32) || cx % 8 || cskip % 8) throw Error(SDMI_ERR_UNSUPPORTED, "cat_chain: Cin must be a multiple of 32 (bf16: 64), the halves of 8");
    Act a = act_from_nchw(x, n, cin, h, wd, dt);
    const OpRoute r{false, dt, dt, dt};
    auto run = [&](const float* wt, const float* bias, int cout, Act& y) {
        OpConvW w(this, wt, bias, cin, cout, 3, 1, 0, r);
        conv(w.w, a, y, 1, 0, nullptr, 0, nullptr);
    };
    Act cat = new_act(n, h, wd, ctot, dt);
    if (dense) {
        Act yx = new_act(n, h, wd, cx, dt), ys = new_act(n, h, wd, cskip, dt);
        run(w_skip, b_skip, cskip, ys);
        run(w_x, b_x, cx, yx);
        // (the kernel moves 16-byte pieces: a bf16 row of c channels is c / 2 floats)
        SDMI_HIP(launch_concat_channels(yx.p, ys.p, cat.p, cat.rows(), dt ? cx / 2 : cx, dt ? cskip / 2 : cskip, stream_));
        release(yx); release(ys);
    } else {
        Act ys = slice(cat, cx, cskip), yx = slice(cat, 0, cx);   // the input block's half first, then the block below's: unet_run's order
        run(w_skip, b_skip, cskip, ys);
        run(w_x, b_x, cx, yx);
    }
    NormW nw; nw.gamma = const_cast<float*>(gamma); nw.beta = const_cast<float*>(beta); nw.c = ctot; nw.eps = eps;
    Act g = new_act(n, h, wd, ctot, dt);
    group_norm(nw, cat, g, silu);
    act_to_nchw(g, out);
    release(a); release(cat); release(g);
}

void Engine::op_geglu_forward(const float* x, const float* wt, const float* bias, int rows, int cin, int hidden, float* out) {
    const int dt = (bf16_ && cin % 64 == 0 && hidden % 8 == 0) ? 1 : 0;
    OpLinW w(this, wt, bias, cin, 2 * hidden, OpRoute{false, dt, dt, dt});
    if (dt) {
        Buf xh(this, (size_t)rows * cin * 2), yh(this, (size_t)rows * hidden * 2);
        SDMI_HIP(launch_f32_to_bf16(x, xh.p, (long long)rows * cin, stream_));
        gemm_geglu(w.w, rows_view(xh.p, rows, cin, 1), rows_view(yh.p, rows, hidden, 1));
        rows_to_f32(yh.p, out, rows, hidden);
        return;
    }
    if (opt_geglu_fuse_ >= 7 && plane_gemm(cin, hidden) && hidden % 32 == 0) {
        // tests: the model's plane form -- x as planes in, the gated result as planes out (joined back exactly) -- through the plane GEMM's fused gate;
        // geglu_fuse = 7: the tile the table / cost model picks, 8: also the fp32 result from the same launch (both outputs of the epilogue)
        Buf x3(this, (size_t)rows * (cin / 32) * 192), o3(this, (size_t)rows * (hidden / 32) * 192);
        SDMI_HIP(launch_split3_rows(x, x3.p, rows, cin, cin, (long long)(cin / 32) * 192, stream_));
        if (opt_geglu_fuse_ == 8) {
            Buf o32(this, (size_t)rows * hidden * 4);
            gemm_geglu(w.w, rows_view(nullptr, rows, cin, 0, 0, x3.p), rows_view(o32.p, rows, hidden, 0, 0, o3.p));
            SDMI_HIP(hipMemcpyAsync(out, o32.p, (size_t)rows * hidden * 4, hipMemcpyDeviceToDevice, stream_));   // the fp32 output of a launch that writes both
        } else {
            gemm_geglu(w.w, rows_view(nullptr, rows, cin, 0, 0, x3.p), rows_view(nullptr, rows, hidden, 0, 0, o3.p));
            SDMI_HIP(launch_join3_rows(o3.p, out, rows, hidden, (long long)(hidden / 32) * 192, hidden, stream_));
        }
        return;
    }
    gemm_geglu(w.w, rows_view(x, rows, cin, 0), rows_view(out, rows, hidden, 0));
}

// out = u x w_main + b_main + h x w_aux + b_aux + resid as Engine::spatial_transformer computes the tail of a transformer block: both inputs as planes, option
// proj_out_fold = 1 -> linear_pair (an error where it declines: no quiet other path), 0 -> two launches (the auxiliary Linear with the residual, then the main one with
// that as its residual).  The result is kept at rows out_ld floats (planes: out_ld / 32 * 192 bytes) apart and returned dense.
void Engine::op_linear_pair(const float* u, const float* h, const float* w_main, const float* b_main, const float* w_aux, const float* b_aux, const float* resid, int resid_ld,
                            int rows, int k_main, int k_aux, int cout, int out_ld, float* out, float* out3) {
    if (rows <= 0 || k_main <= 0 || k_aux <= 0 || cout <= 0) throw Error(SDMI_ERR_INVALID, "linear_pair: bad shape");
    if (bf16_ || !plane_gemm(k_main, cout) || !plane_gemm(k_aux, cout)) throw Error(SDMI_ERR_UNSUPPORTED, "linear_pair: the fp32 plane kernels only (in_features in multiples of 32)");
    if (!out_ld) out_ld = cout;
    if (out_ld < cout || (!out && !out3)) throw Error(SDMI_ERR_INVALID, "linear_pair: out_ld below cout, or no output asked for");
    if (out3 && (cout % 32 || out_ld % 32)) throw Error(SDMI_ERR_UNSUPPORTED, "linear_pair: a plane output needs cout and out_ld in multiples of 32");
    const OpRoute r{false, 0, 0, 0};
    OpLinW wm(this, w_main, b_main, k_main, cout, r), wa(this, w_aux, b_aux, k_aux, cout, r);
    const int u_ld = k_main / 32 * 192, h_ld = k_aux / 32 * 192, ld3 = out_ld / 32 * 192;
    Buf u3(this, (size_t)rows * u_ld), h3(this, (size_t)rows * h_ld);
    SDMI_HIP(launch_split3_rows(u, u3.p, rows, k_main, k_main, u_ld, stream_));
    SDMI_HIP(launch_split3_rows(h, h3.p, rows, k_aux, k_aux, h_ld, stream_));
    std::unique_ptr<Buf> y, y3;
    if (out) y.reset(new Buf(this, (size_t)rows * out_ld * 4));
    if (out3) y3.reset(new Buf(this, (size_t)rows * ld3));
    if (opt_proj_out_fold_) {
        const LinearPair lp{u3.p, u_ld, wm.w.bt, b_main, k_main, h3.p, h_ld, wa.w.bt, b_aux, k_aux, rows, cout, resid, resid_ld ? resid_ld : cout,
                            y ? y->f() : nullptr, out_ld, y3 ? y3->p : nullptr, ld3};
        if (!linear_pair(lp)) throw Error(SDMI_ERR_UNSUPPORTED, "linear_pair: this shape / these options do not pair (proj_out_fold=0 runs the two launches)");
    } else {
        if (out_ld != cout) throw Error(SDMI_ERR_UNSUPPORTED, "linear_pair: the two launches keep the result dense (out_ld = cout)");
        Buf t(this, (size_t)rows * cout * 4);
        const Act ta = rows_view(t.p, rows, cout, 0), ra = rows_view(resid, rows, cout, 0, resid_ld);
        linear(wa.w, rows_view(nullptr, rows, k_aux, 0, 0, h3.p), ta, resid ? &ra : nullptr);
        linear(wm.w, rows_view(nullptr, rows, k_main, 0, 0, u3.p), rows_view(y ? y->p : nullptr, rows, cout, 0, 0, y3 ? y3->p : nullptr), &ta);
    }
    if (y) SDMI_HIP(hipMemcpy2DAsync(out, (size_t)cout * 4, y->p, (size_t)out_ld * 4, (size_t)cout * 4, (size_t)rows, hipMemcpyDeviceToDevice, stream_));
    if (y3) SDMI_HIP(launch_join3_rows(y3->p, out3, rows, cout, ld3, cout, stream_));
}

void Engine::op_linear_fold(const float* w_lin, const float* b_lin, const float* w_proj, int k_main, int cmid, int cout, float* wf, float* bf) {
    if (k_main <= 0 || cmid <= 0 || cout <= 0) throw Error(SDMI_ERR_INVALID, "linear_fold: bad shape");
    if (!(cmid % 32 == 0 || (cmid < 32 && cmid % 4 == 0))) throw Error(SDMI_ERR_UNSUPPORTED, "linear_fold: the inner width must be a multiple of 32, or < 32 and a multiple of 4");
    Buf bt_l(this, (size_t)cmid * k_main * 4), bt_p(this, (size_t)cout * cmid * 4);
    SDMI_HIP(launch_pack_linear_weight(w_lin, bt_l.f(), k_main, cmid, stream_));     // [cmid][k_main]
    SDMI_HIP(launch_pack_conv_weight(w_proj, bt_p.f(), cout, cmid, 1, 1, stream_));   // [cout][cmid]
    fold_weights(bt_p.f(), bt_l.f(), b_lin, cout, cmid, k_main, wf, bf);
}

void Engine::op_geglu(const float* proj, int rows, int hidden, float* out) {
    if (fp8_ && opt_fp8_ops_ && hidden % 32 == 0) {   // option fp8_ops (tests): the quantising gate of the fp8_linear path, dequantised
        Buf ph(this, (size_t)rows * 2 * hidden * 2);
        SDMI_HIP(launch_f32_to_bf16(proj, ph.p, (long long)rows * 2 * hidden, stream_));
        ActQ q = new_rowsq(rows, hidden);
        SDMI_HIP(launch_geglu_fp8(ph.p, q.q, q.s, rows, hidden, stream_));
        SDMI_HIP(launch_dequant_fp8(q.q, q.s, out, rows, hidden, stream_));
        release(q);
        return;
    }
    if (bf16_ && hidden % 8 == 0) {
        Buf ph(this, (size_t)rows * 2 * hidden * 2), oh(this, (size_t)rows * hidden * 2);
        SDMI_HIP(launch_f32_to_bf16(proj, ph.p, (long long)rows * 2 * hidden, stream_));
        SDMI_HIP(launch_geglu_bf16(ph.p, oh.p, rows, hidden, stream_));
        rows_to_f32(oh.p, out, rows, hidden);
        return;
    }
    if (plane_gemm(hidden, hidden)) {
        Buf y3(this, (size_t)rows * (hidden / 32) * 192);
        SDMI_HIP(launch_geglu_planes(proj, y3.p, rows, hidden, stream_));
        SDMI_HIP(launch_join3_rows(y3.p, out, rows, hidden, (long long)(hidden / 32) * 192, hidden, stream_));
        return;
    }
    SDMI_HIP(launch_geglu(proj, out, rows, hidden, stream_));
}

void Engine::op_timestep_embedding_f(double t, int dim, float* out) {
    const float tf = (float)t;
    Buf td(this, sizeof(float));
    SDMI_HIP(hipMemcpyAsync(td.p, &tf, sizeof(float), hipMemcpyHostToDevice, stream_));
    SDMI_HIP(hipStreamSynchronize(stream_));
    { ProfScope ps_o(this, PC_OTHER); SDMI_HIP(launch_timestep_embedding_f((const float*)td.p, 1, dim, out, stream_)); }   // (profiled, not counted: as ever)
    SDMI_HIP(hipStreamSynchronize(stream_));
}

void Engine::op_timestep_embedding(int t, int dim, float* out) {
    Buf td(this, sizeof(int));
    SDMI_HIP(hipMemcpyAsync(td.p, &t, sizeof(int), hipMemcpyHostToDevice, stream_));
    SDMI_HIP(hipStreamSynchronize(stream_));
    { ProfScope ps_o(this, PC_OTHER); SDMI_HIP(launch_timestep_embedding((const int*)td.p, 1, dim, out, stream_)); }       // (profiled, not counted: as ever)
    SDMI_HIP(hipStreamSynchronize(stream_));
}

// option gemm_probe: what the diagnostic instantiation of a plane GEMM stored (24 words per workgroup: kernels.hpp ConvGemm::probe), summarised on stderr
void Engine::probe_report(void* pb_dev, size_t kMaxBlocks, int n, int cin, int h, int w, int cout, int k, int tile_cfg, int splitk) {
    std::vector<unsigned long long> hb(kMaxBlocks * 24);
    SDMI_HIP(hipMemcpyAsync(hb.data(), pb_dev, hb.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_));
    SDMI_HIP(hipStreamSynchronize(stream_));
    std::vector<double> pro, loop, epi, tot, wait_frac, mhz;
    unsigned long long first = ~0ull, last = 0, last_start = 0;
    for (size_t b = 0; b < kMaxBlocks; ++b) {
        const unsigned long long* d = &hb[24 * b];
        if (!d[0] || !d[3]) continue;
        pro.push_back((d[1] - d[0]) * 0.01); loop.push_back((d[2] - d[1]) * 0.01); epi.push_back((d[3] - d[2]) * 0.01); tot.push_back((d[3] - d[0]) * 0.01);
        first = std::min(first, d[0]); last = std::max(last, d[3]); last_start = std::max(last_start, d[0]);
        for (int wv = 0; wv < 8; ++wv)
            if (d[4 + 2 * wv]) {
                wait_frac.push_back((double)d[5 + 2 * wv] / (double)d[4 + 2 * wv]);
                if (d[2] > d[1]) mhz.push_back((double)d[4 + 2 * wv] / ((d[2] - d[1]) * 0.01));
            }
    }
    auto q = [](std::vector<double>& v, double f) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[std::min(v.size() - 1, (size_t)(f * v.size()))]; };
    std::fprintf(stderr, "gemm_probe n=%d cin=%d %dx%d cout=%d k=%d tile=%d splitk=%d cold=%d: %zu workgroups; us min/median/max: first tile %.2f/%.2f/%.2f, "
                         "k loop %.2f/%.2f/%.2f, epilogue %.2f/%.2f/%.2f, workgroup %.2f/%.2f/%.2f; first entry -> last entry %.2f, first entry -> last exit %.2f; "
                         "per wave: share of the k loop waiting at the per-tile barrier %.3f/%.3f/%.3f, shader clock in the k loop %.0f/%.0f/%.0f MHz\n",
                 n, cin, h, w, cout, k, tile_cfg, splitk, opt_bench_cold_, tot.size(), q(pro, 0), q(pro, 0.5), q(pro, 1), q(loop, 0), q(loop, 0.5), q(loop, 1),
                 q(epi, 0), q(epi, 0.5), q(epi, 1), q(tot, 0), q(tot, 0.5), q(tot, 1), (last_start - first) * 0.01, (last - first) * 0.01,
                 q(wait_frac, 0), q(wait_frac, 0.5), q(wait_frac, 1), q(mhz, 0), q(mhz, 0.5), q(mhz, 1));
}

// puts an option back when the scope ends, however it ends
struct OptRestore { int& opt; const int saved = opt; ~OptRestore() { opt = saved; } };

double Engine::bench_conv(int n, int cin, int h, int w, int cout, int k, int stride, int ups, int tile_cfg, int splitk,
                          int iters) {
    SDMI_HIP(hipSetDevice(cfg_.device));
    const OpRoute r = conv_route(cin, cout, k, stride, ups, false, false);
    int ho, wo;
    conv_out_hw(h, w, k, stride, k == 3 ? 1 : 0, ups, &ho, &wo);
    if (r.q8) {
        // precision = 2: time the MXFP8 kernel on a pre-quantised activation (what the fused GroupNorm hands it)
        Act x32 = new_act(n, h, w, cin, 0), y = new_act(n, h, w, cout, 1);
        Buf w32(this, (size_t)cout * cin * 9 * 4), bias(this, (size_t)cout * 4);
        SDMI_HIP(launch_fill_normal(x32.p, (long long)x32.rows() * cin, 11, stream_));
        SDMI_HIP(launch_fill_normal(w32.f(), (long long)cout * cin * 9, 12, stream_));
        SDMI_HIP(launch_fill_normal(bias.f(), cout, 13, stream_));
        ActQ q = new_actq(n, h, w, cin);
        SDMI_HIP(launch_quantize_fp8(x32.p, q.q, q.s, x32.rows(), cin, stream_));
        const OpConvW packed(this, w32.f(), bias.f(), cin, cout, 3, 1, 0, r);
        const ConvW& cw = packed.w;
        const OptRestore r1{opt_fp8_tile_}, r2{gopt_.force_splits};
        opt_fp8_tile_ = tile_cfg; gopt_.force_splits = splitk;
        const AtExit done{[&] { release(x32); release(y); release(q); }};
        float ms = 0;
        conv_fp8(cw, q, y, nullptr, nullptr);
        SDMI_HIP(hipEventRecord(ev0_, stream_));
        for (int i = 0; i < iters; ++i) conv_fp8(cw, q, y, nullptr, nullptr);
        SDMI_HIP(hipEventRecord(ev1_, stream_));
        SDMI_HIP(hipEventSynchronize(ev1_));
        SDMI_HIP(hipEventElapsedTime(&ms, ev0_, ev1_));
        return (double)ms / std::max(1, iters);
    }
    const int wdt = r.wdt;
    Act a = new_act(n, h, w, cin, wdt), y = new_act(n, ho, wo, cout, r.ydt);
    const AtExit done{[&] { release(a); release(y); }};
    Buf bt(this, (size_t)cout * cin * k * k * 4), bias(this, (size_t)cout * 4);
    {
        Buf tmp(this, std::max((size_t)a.rows() * cin, (size_t)cout * cin * k * k) * 4);
        SDMI_HIP(launch_fill_normal(wdt ? tmp.f() : a.p, (long long)a.rows() * cin, 11, stream_));
        if (wdt) SDMI_HIP(launch_f32_to_bf16(tmp.f(), a.p, (long long)a.rows() * cin, stream_));
        SDMI_HIP(launch_fill_normal(wdt ? tmp.f() : bt.f(), (long long)cout * cin * k * k, 12, stream_));
        if (wdt) SDMI_HIP(launch_f32_to_bf16(tmp.f(), bt.p, (long long)cout * cin * k * k, stream_));
        SDMI_HIP(hipStreamSynchronize(stream_));
    }
    SDMI_HIP(launch_fill_normal(bias.f(), cout, 13, stream_));
    TempSplit planes(this, bt.f(), wdt ? 0 : cout, (long long)cin * k * k);
    const bool plane_tile = tile_cfg >= 0 && gemm_tile_id(tile_cfg).family == kFamP;
    if (!wdt && plane_tile && cin % 32 == 0) {   // plane tiles are timed on planes their producer would have written
        a.p3 = pool_.alloc(a.bytes3()); a.ld3 = (cin / 32) * 192;
        SDMI_HIP(launch_split3_rows(a.p, a.p3, a.rows(), cin, cin, a.ld3, stream_));
    }
    ConvW cw; cw.cin = cin; cw.cout = cout; cw.k = k; cw.bt = bt.f(); cw.bias = bias.f(); cw.dt = wdt;
    TempUpFold up_fold(this, cw, stride, ups);   // (option ups_phase = 1 times the phase launch of an up-convolution on the forced plane tile / split count)
    const OptRestore r1{gopt_.force_tile}, r2{gopt_.force_splits}, r3{gopt_.gemm_planes};
    gopt_.force_tile = tile_cfg; gopt_.force_splits = splitk;
    if (plane_tile && !gopt_.gemm_planes) gopt_.gemm_planes = 2;
    float ms = 0;
    conv(cw, a, y, stride, ups, nullptr, 0, nullptr);  // warm-up
    if (opt_bench_cold_) {
        // what the layer costs INSIDE the model: its weights come from HBM (5 GB of planes per UNet forward pass through the 256 MB
        // Infinity Cache between two uses), its activations from the L2s / Infinity Cache of the kernel that wrote them.  Between
        // timed launches a 512 MB fill evicts the weights, then the activation tensor is re-written (split3_rows / a copy).
        const size_t flush_bytes = (size_t)512 << 20;
        Buf flush(this, flush_bytes);
        Buf a_copy(this, a.bytes());
        SDMI_HIP(hipMemcpyAsync(a_copy.p, a.p, a.bytes(), hipMemcpyDeviceToDevice, stream_));
        for (int i = 0; i < iters; ++i) {
            SDMI_HIP(hipMemsetAsync(flush.p, i, flush_bytes, stream_));
            SDMI_HIP(hipMemcpyAsync(a.p, a_copy.p, a.bytes(), hipMemcpyDeviceToDevice, stream_));
            if (a.p3) SDMI_HIP(launch_split3_rows(a.p, a.p3, a.rows(), cin, cin, a.ld3, stream_));
            SDMI_HIP(hipEventRecord(ev0_, stream_));
            conv(cw, a, y, stride, ups, nullptr, 0, nullptr);
            SDMI_HIP(hipEventRecord(ev1_, stream_));
            SDMI_HIP(hipEventSynchronize(ev1_));
            float t = 0;
            SDMI_HIP(hipEventElapsedTime(&t, ev0_, ev1_));
            ms += t;
        }
    } else {
        SDMI_HIP(hipEventRecord(ev0_, stream_));
        for (int i = 0; i < iters; ++i) conv(cw, a, y, stride, ups, nullptr, 0, nullptr);
        SDMI_HIP(hipEventRecord(ev1_, stream_));
        SDMI_HIP(hipEventSynchronize(ev1_));
        SDMI_HIP(hipEventElapsedTime(&ms, ev0_, ev1_));
    }
    if (opt_gemm_probe_ && a.p3) {
        // diagnostic: one more launch in which every workgroup of the plane GEMM stamps its phases (ConvGemm::probe; 100 MHz clock)
        constexpr size_t kMaxBlocks = kGemmProbeBlocks;
        Buf pb(this, kMaxBlocks * 24 * sizeof(unsigned long long));
        SDMI_HIP(hipMemsetAsync(pb.p, 0, kMaxBlocks * 24 * sizeof(unsigned long long), stream_));
        if (opt_bench_cold_) {
            Buf flush(this, (size_t)512 << 20);
            SDMI_HIP(hipMemsetAsync(flush.p, 1, (size_t)512 << 20, stream_));
            SDMI_HIP(launch_split3_rows(a.p, a.p3, a.rows(), cin, cin, a.ld3, stream_));
        }
        probe_buf_ = static_cast<unsigned long long*>(pb.p);
        try { conv(cw, a, y, stride, ups, nullptr, 0, nullptr); } catch (...) { probe_buf_ = nullptr; throw; }
        probe_buf_ = nullptr;
        probe_report(pb.p, kMaxBlocks, n, cin, h, w, cout, k, tile_cfg, splitk);
    }
    return (double)ms / std::max(1, iters);
}

// sdmi_attention_plan: the AttnPlanIn of qkv_attention_dev (dense rows, bf16 storage on a bf16 context unless masked, plane output under gemm_planes), planned
// under the current options.  No device call.
AttnPlan Engine::attention_plan(int n, int n_head, int nq, int nk, int d_head, bool has_mask) const {
    if (n <= 0 || nq <= 0 || nk <= 0 || n_head <= 0 || d_head <= 0) throw Error(SDMI_ERR_INVALID, "attention_plan: bad shape");
    const int n_state = n_head * d_head;
    AttnPlanIn in{};
    in.n = n; in.n_head = n_head; in.nq = nq; in.nk = nk; in.d_head = d_head; in.has_mask = has_mask;
    in.bf16 = (bf16_ && !has_mask) ? 1 : 0;
    in.planes_out = !in.bf16 && plane_gemm(n_state, n_state) && attn_supported_head_dim(d_head);
    in.rows_aligned = !(n_state & (in.bf16 ? 7 : 3));
    return plan_attention(in, aopt_);
}

double Engine::bench_attention(int n, int nq, int nk, int n_state, int n_head, int iters) {
    SDMI_HIP(hipSetDevice(cfg_.device));
    if (n <= 0 || nq <= 0 || nk <= 0 || n_head <= 0 || n_state % n_head) throw Error(SDMI_ERR_INVALID, "bench_attention: bad shape");
    const long long qe = (long long)n * nq * n_state, ke = (long long)n * nk * n_state;
    Buf q(this, qe * 4), k(this, ke * 4), v(this, ke * 4), o(this, qe * 4);
    SDMI_HIP(launch_fill_normal(q.f(), qe, 21, stream_));
    SDMI_HIP(launch_fill_normal(k.f(), ke, 22, stream_));
    SDMI_HIP(launch_fill_normal(v.f(), ke, 23, stream_));
    const int dt = edt();
    Buf qh(this, dt ? qe * 2 : 256), kh(this, dt ? ke * 2 : 256), vh(this, dt ? ke * 2 : 256);
    if (dt) {
        const int dh = n_state / n_head;
        SDMI_HIP(launch_f32_to_bf16_scaled(q.f(), qh.p, qe, q_prescaled(dt, dh) ? attn_bf16_q_scale(dh) : 1.f, stream_));
        SDMI_HIP(launch_f32_to_bf16(k.f(), kh.p, ke, stream_));
        SDMI_HIP(launch_f32_to_bf16(v.f(), vh.p, ke, stream_));
    }
    const float* qp = dt ? qh.f() : q.f(); const float* kp = dt ? kh.f() : k.f(); const float* vp = dt ? vh.f() : v.f();
    Attn at;
    at.q = attn_rows(rows_view(qp, (long long)n * nq, n_state, dt), nq);
    at.k = attn_rows(rows_view(kp, (long long)n * nk, n_state, dt), nk);
    at.v = attn_rows(rows_view(vp, (long long)n * nk, n_state, dt), nk);
    at.o = attn_rows(rows_view(o.p, (long long)n * nq, n_state, dt), nq);
    at.n = n; at.nq = nq; at.nk = nk; at.n_head = n_head; at.d_head = n_state / n_head; at.dt = dt; at.q_log2 = q_prescaled(dt, at.d_head);
    auto run = [&] { attention(at); };
    run();
    float ms = 0;
    SDMI_HIP(hipEventRecord(ev0_, stream_));
    for (int i = 0; i < iters; ++i) run();
    SDMI_HIP(hipEventRecord(ev1_, stream_));
    SDMI_HIP(hipEventSynchronize(ev1_));
    SDMI_HIP(hipEventElapsedTime(&ms, ev0_, ev1_));
    return (double)ms / std::max(1, iters);
}

void Engine::op_ip_attention(const float* q, const float* k_ip, const float* v_ip, const float* o_text, const float* s, int n, int nq, int T, int n_state, int n_head,
                             bool planes, float* out) {
    if (n < 1 || nq < 1 || n_head < 1 || n_state < 1 || n_state % n_head) throw Error(SDMI_ERR_INVALID, "op_ip_attention: bad shape");
    if (T < 1) throw Error(SDMI_ERR_INVALID, "op_ip_attention: T_ip must be at least 1");
    if (T > kIpMaxTokens) throw Error(SDMI_ERR_UNSUPPORTED, "op_ip_attention: more than 64 image tokens");
    const int d = n_state / n_head, dt = edt();
    if (!ip_attention_head_dim(d)) throw Error(SDMI_ERR_UNSUPPORTED, "op_ip_attention: head width " + std::to_string(d) + " (40, 64, 80, 160 are served)");
    if (planes && (dt || n_state % 32)) throw Error(SDMI_ERR_INVALID, "op_ip_attention: planes are the fp32 engine's format and need n_state % 32 == 0");
    const long long qe = (long long)n * nq * n_state;
    IpAttnParams p{};
    p.k = k_ip; p.v = v_ip; p.s = s;
    p.n = n; p.nq = nq; p.T = T; p.n_head = n_head; p.d_head = d;
    p.ldq = n_state; p.q_bs = (long long)nq * n_state; p.ldo3 = (n_state / 32) * 192;
    p.bf16 = dt; p.q_log2 = q_prescaled(dt, d) ? 1 : 0; p.scale = (float)std::pow((double)d, -0.25);
    const double fl = 4.0 * n * n_head * (double)nq * T * d;
    auto run = [&] {
        ProfScope ps(this, PC_ATTENTION, fl, 0);
        SDMI_LAUNCH_IN(ps, fl, launch_ip_attention(p, stream_));
    };
    if (dt) {
        Buf qh(this, qe * 2), oh(this, qe * 2), yh(this, qe * 2);
        SDMI_HIP(launch_f32_to_bf16_scaled(q, qh.p, qe, p.q_log2 ? attn_bf16_q_scale(d) : 1.f, stream_));   // Engine::attention's q convention
        SDMI_HIP(launch_f32_to_bf16(o_text, oh.p, qe, stream_));
        p.q = qh.p; p.o_text = oh.p; p.o = yh.p; p.form = 1;
        run();
        rows_to_f32(yh.p, out, n * nq, n_state);
    } else if (planes) {
        Buf o3(this, (size_t)n * nq * p.ldo3);
        SDMI_HIP(launch_split3_rows(o_text, o3.p, (long long)n * nq, n_state, n_state, p.ldo3, stream_));
        p.q = q; p.o_text = o3.p; p.o = o3.p; p.form = 2;
        run();
        SDMI_HIP(launch_join3_rows(o3.p, out, (long long)n * nq, n_state, p.ldo3, n_state, stream_));
    } else {
        p.q = q; p.o_text = o_text; p.o = out; p.form = 0;
        run();
    }
}

}  // namespace sdmi
