// engine.cpp -- see engine.hpp.  Reference citations are relative to
// Gadersd/stable-diffusion-burn (src/model/...).
#include "engine.hpp"
#include "ckpt_keys.hpp"
#include "lora_keys.hpp"
#include "mpk_reader.hpp"
#include "safetensors_reader.hpp"

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

namespace sdmi {

// =============================================================================
// DevPool
// =============================================================================
static constexpr size_t kAlign = 256;
static constexpr size_t kSlabMin = (size_t)1 << 30;  // 1 GiB

DevPool::~DevPool() {
    for (auto& s : slabs_) (void)hipFree(s.base);
}

void* DevPool::alloc(size_t bytes) {
    if (bytes == 0) bytes = kAlign;
    bytes = (bytes + kAlign - 1) / kAlign * kAlign;
    for (int pass = 0; pass < 2; ++pass) {
        for (size_t si = 0; si < slabs_.size(); ++si) {
            auto& fl = slabs_[si].free_list;
            for (size_t i = 0; i < fl.size(); ++i) {
                if (fl[i].size >= bytes) {
                    void* p = slabs_[si].base + fl[i].off;
                    if (fl[i].size == bytes) fl.erase(fl.begin() + i);
                    else { fl[i].off += bytes; fl[i].size -= bytes; }
                    live_[p] = Live{(int)si, bytes, ++serial_};
                    in_use_ += bytes;
                    high_ = std::max(high_, in_use_);
                    if (fill_ >= 0) {
                        hipError_t e = hipMemsetAsync(p, fill_, bytes, stream_);
                        if (e != hipSuccess) { free(p); throw Error(SDMI_ERR_HIP, std::string("DevPool: hipMemsetAsync failed: ") + hipGetErrorString(e)); }
                        note_fill(bytes);
                    }
                    return p;
                }
            }
        }
        // no fit: new slab
        size_t sz = std::max(bytes, kSlabMin);
        char* base = nullptr;
        hipError_t e = hipMalloc((void**)&base, sz);
        if (e != hipSuccess && sz > bytes) { sz = bytes; e = hipMalloc((void**)&base, sz); }
        if (e != hipSuccess)
            throw Error(SDMI_ERR_HIP, std::string("DevPool: hipMalloc(") + std::to_string(sz) + ") failed: " + hipGetErrorString(e));
        Slab s; s.base = base; s.size = sz; s.free_list.push_back({0, sz});
        slabs_.push_back(std::move(s));
        reserved_ += sz;
    }
    throw Error(SDMI_ERR_HIP, "DevPool: allocation failed");
}

void DevPool::free(void* p) {
    if (!p) return;
    auto it = live_.find(p);
    if (it == live_.end()) throw Error(SDMI_ERR_STATE, "DevPool: free of unknown pointer");
    const int si = it->second.slab;
    const size_t size = it->second.size;
    live_.erase(it);
    in_use_ -= size;
    auto& sl = slabs_[si];
    const size_t off = (char*)p - sl.base;
    auto& fl = sl.free_list;
    size_t pos = 0;
    while (pos < fl.size() && fl[pos].off < off) ++pos;
    fl.insert(fl.begin() + pos, {off, size});
    if (pos + 1 < fl.size() && fl[pos].off + fl[pos].size == fl[pos + 1].off) {
        fl[pos].size += fl[pos + 1].size;
        fl.erase(fl.begin() + pos + 1);
    }
    if (pos > 0 && fl[pos - 1].off + fl[pos - 1].size == fl[pos].off) {
        fl[pos - 1].size += fl[pos].size;
        fl.erase(fl.begin() + pos);
    }
}

size_t DevPool::free_since(unsigned long long mark) {
    std::vector<void*> victims;
    for (auto& kv : live_)
        if (kv.second.serial > mark) victims.push_back(kv.first);
    for (void* p : victims) free(p);
    return victims.size();
}

// =============================================================================
// per-class kernel timing (HIP events on the engine stream)
// =============================================================================
hipEvent_t Engine::prof_event() {
    if (!prof_free_.empty()) { hipEvent_t e = prof_free_.back(); prof_free_.pop_back(); return e; }
    hipEvent_t e;
    SDMI_HIP(hipEventCreate(&e));
    return e;
}

Engine::ProfScope::ProfScope(Engine* e_, int cls_, double flops_, double bytes_, int n_launch_) : e(e_), cls(cls_), flops(flops_), bytes(bytes_), n_launch(n_launch_) {
    if (!e->profiling_) return;
    a = e->prof_event();
    b = e->prof_event();
    (void)hipEventRecord(a, e->stream_);
}

Engine::ProfScope::~ProfScope() {
    if (!a) return;
    (void)hipEventRecord(b, e->stream_);
    e->prof_pending_.push_back({cls, a, b, flops, bytes, n_launch, tag});
    if (e->prof_pending_.size() >= 2048) {
        try { e->prof_flush(); } catch (...) {}
    }
}

void Engine::ProfScope::set_tag(const char* fmt, ...) {
    if (!a || !e->prof_tagging_) return;
    char buf[192];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    auto it = e->prof_tag_ids_.find(buf);
    if (it == e->prof_tag_ids_.end()) {
        it = e->prof_tag_ids_.emplace(buf, (int)e->prof_tag_names_.size()).first;
        e->prof_tag_names_.push_back(buf);
    }
    tag = it->second;
}

// What an (a, b) event pair reads with NOTHING between its two records: the pair's own cost on the stream, which would otherwise be
// booked as kernel time on every launch (round 2: the classes summed to 7 % more than the step).  Median of 64 empty pairs, taken with the
// stream otherwise idle when profiling is switched on, and subtracted from every sample.
void Engine::prof_calibrate() {
    SDMI_HIP(hipStreamSynchronize(stream_));
    std::vector<float> t;
    for (int i = 0; i < 64; ++i) {
        hipEvent_t a = prof_event(), b = prof_event();
        SDMI_HIP(hipEventRecord(a, stream_));
        SDMI_HIP(hipEventRecord(b, stream_));
        SDMI_HIP(hipEventSynchronize(b));
        float ms = 0;
        if (hipEventElapsedTime(&ms, a, b) == hipSuccess) t.push_back(ms);
        prof_free_.push_back(a);
        prof_free_.push_back(b);
    }
    std::sort(t.begin(), t.end());
    // An empty pair reads the cost of TWO back-to-back event records (4.6 us on MI355X); a pair around a kernel adds about half of that
    // to the kernel's duration -- rocprofv3's kernel trace of the same run is the yardstick: round 2, 46.0 us by raw events against 43.4 us
    // by rocprofv3 per split-GEMM launch; round 3, 43.4 against 41.1 (profiles/README.md).  So half the empty-pair reading is subtracted.
    prof_overhead_ms_ = t.empty() ? 0.0 : 0.5 * (double)t[t.size() / 2];
}

void Engine::prof_flush() {
    if (prof_pending_.empty()) return;
    SDMI_HIP(hipStreamSynchronize(stream_));
    for (auto& p : prof_pending_) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            ms = (float)std::max(0.0, (double)ms - prof_overhead_ms_);
            prof_[p.cls].ms += ms;
            prof_[p.cls].launches += p.n_launch;
            prof_[p.cls].flops += p.flops;
            prof_[p.cls].bytes += p.bytes;
            if (p.tag >= 0) {
                ProfStat& t = prof_tags_[prof_tag_names_[p.tag]];
                t.ms += ms; t.launches += p.n_launch; t.flops += p.flops; t.bytes += p.bytes;
            }
        }
        prof_free_.push_back(p.a);
        prof_free_.push_back(p.b);
    }
    prof_pending_.clear();
}

// =============================================================================
// roctx ranges
// =============================================================================
namespace {
struct Roctx {
    void* lib = nullptr;
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    bool tried = false;
} g_roctx;
}  // namespace

void Engine::roctx_enable(bool on) {
    if (on && !g_roctx.tried) {
        g_roctx.tried = true;
        for (const char* name : {"libroctx64.so.4", "libroctx64.so", "librocprofiler-sdk-roctx.so.1", "/opt/rocm/lib/libroctx64.so"}) {
            g_roctx.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (g_roctx.lib) break;
        }
        if (g_roctx.lib) {
            g_roctx.push = reinterpret_cast<int (*)(const char*)>(dlsym(g_roctx.lib, "roctxRangePushA"));
            g_roctx.pop = reinterpret_cast<int (*)()>(dlsym(g_roctx.lib, "roctxRangePop"));
        }
    }
    if (on && (!g_roctx.push || !g_roctx.pop)) throw Error(SDMI_ERR_UNSUPPORTED, "roctx: libroctx64 (roctxRangePushA / roctxRangePop) not found");
    roctx_on_ = on;
}
void Engine::roctx_push(const char* name) { if (g_roctx.push) (void)g_roctx.push(name); }
void Engine::roctx_pop() { if (g_roctx.pop) (void)g_roctx.pop(); }

// =============================================================================
// construction / model definition
// =============================================================================
Engine::Engine(const sdmi_config& cfg) : cfg_(cfg) {
    if (cfg.precision < 0 || cfg.precision > 2) throw Error(SDMI_ERR_UNSUPPORTED, "precision must be 0 (fp32), 1 (bf16) or 2 (bf16 + MXFP8 ResBlock convolutions)");
    bf16_ = cfg.precision >= 1;
    fp8_ = cfg.precision == 2;
    if (bf16_ && (cfg.model_channels % 64 || cfg.vae_ch % 64 || cfg.ctx_dim % 64))
        throw Error(SDMI_ERR_UNSUPPORTED, "precision=1 (bf16) needs model_channels, vae_ch and ctx_dim to be multiples of 64");
    if (cfg.model_channels % 32 || cfg.model_channels <= 0) throw Error(SDMI_ERR_INVALID, "model_channels must be a positive multiple of 32");
    if (cfg.vae_ch % 32 || cfg.vae_ch <= 0) throw Error(SDMI_ERR_INVALID, "vae_ch must be a positive multiple of 32");
    if (cfg.variant != 0 && cfg.variant != 1) throw Error(SDMI_ERR_INVALID, "variant must be 0 (SD v1) or 1 (SD 2.x)");
    if (cfg.variant == 1 && cfg.model_channels % 64) throw Error(SDMI_ERR_INVALID, "variant = 1 (SD 2.x): model_channels must be a multiple of 64, the head width");
    if (cfg.variant == 0 && (cfg.n_head <= 0 || cfg.model_channels % cfg.n_head)) throw Error(SDMI_ERR_INVALID, "n_head must divide model_channels");
    if (cfg.ctx_dim % 32 || cfg.ctx_dim <= 0) throw Error(SDMI_ERR_INVALID, "ctx_dim must be a positive multiple of 32");
    if (cfg_.unet_in_ch == 0) cfg_.unet_in_ch = 4;   // a zeroed field: the latent alone
    if (cfg_.unet_in_ch < 4 || cfg_.unet_in_ch > 12) throw Error(SDMI_ERR_INVALID, "unet_in_ch must be 4 (the latent alone) or 5 .. 12 (the latent + conditioning channels)");
    if (cfg_.control_hint_ch != 0 && cfg_.control_hint_ch != 3) throw Error(SDMI_ERR_INVALID, "control_hint_ch must be 0 (no ControlNet) or 3 (an RGB hint)");
    if (cfg_.control_hint_ch != 0 && cfg_.unet_in_ch != 4)
        throw Error(SDMI_ERR_UNSUPPORTED, "control_hint_ch != 0 needs unet_in_ch = 4: the control encoder's first convolution takes the 4 latent channels");
    if (cfg_.control_hint_ch != 0 && cfg_.variant == 1) throw Error(SDMI_ERR_UNSUPPORTED, "control_hint_ch != 0 is not supported on a variant = 1 (SD 2.x) context");
    aopt_.attn_d64 = cfg_.variant == 1 ? 2 : 0;   // before build_model: the query weights' pre-scale follows it (q_prescaled)
    check_latent_size(cfg.latent_h, cfg.latent_w);
    lat_h_ = cfg.latent_h;
    lat_w_ = cfg.latent_w;
    int ndev = 0;
    SDMI_HIP(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw Error(SDMI_ERR_HIP, "no HIP device visible: libsdmi has no CPU fallback");
    if (cfg.device < 0 || cfg.device >= ndev) throw Error(SDMI_ERR_INVALID, "device ordinal out of range");
    SDMI_HIP(hipSetDevice(cfg.device));
    hipDeviceProp_t prop;
    SDMI_HIP(hipGetDeviceProperties(&prop, cfg.device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        throw Error(SDMI_ERR_UNSUPPORTED, std::string("libsdmi is built for gfx950 (MI355X) only; device is ") + prop.gcnArchName);
    try {
    SDMI_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    pool_.set_stream(stream_);
    SDMI_HIP(hipEventCreate(&ev0_));
    SDMI_HIP(hipEventCreate(&ev1_));
    SDMI_HIP(hipEventCreateWithFlags(&ev_user_, hipEventDisableTiming));
    SDMI_HIP(hipMalloc(&zero_page_, 256));
    weight_allocs_.push_back(zero_page_);
    SDMI_HIP(hipMemsetAsync(zero_page_, 0, 256, stream_));
    SDMI_HIP(hipStreamSynchronize(stream_));
    tuning_.load_builtin();   // measured per-shape tile choices (tools/autotune.py -> tuning/gfx950_*.txt)
    build_model();
    } catch (...) {   // the destructor does not run for a half-built object
        destroy();
        throw;
    }
}

Engine::~Engine() { destroy(); }

void Engine::check_latent_size(int h, int w) {
    if (h % 8 || w % 8 || h <= 0 || w <= 0) throw Error(SDMI_ERR_INVALID, "latent_h/latent_w must be positive multiples of 8");
}

void Engine::destroy() noexcept {
    (void)hipSetDevice(cfg_.device);
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (sdmi_lora* a : loras_) {
        for (void* p : a->allocs) (void)hipFree(p);
        delete a;
    }
    loras_.clear();
    if (emb_bank_) (void)hipFree(emb_bank_);
    emb_bank_ = nullptr; emb_rows_ = 0; embeddings_.clear();
    if (ctrl_.hint_dev) (void)hipFree(ctrl_.hint_dev);   // a control still set: its hint pictures
    ctrl_ = Control{};
    if (ip_.tokens) (void)hipFree(ip_.tokens);
    if (ip_.neg) (void)hipFree(ip_.neg);
    ip_ = IpState{};
    for (void* p : ipw_.allocs) (void)hipFree(p);
    ipw_ = IpWeights{};
    for (void* p : weight_allocs_) (void)hipFree(p);
    for (auto& p : prof_pending_) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (hipEvent_t e : prof_free_) (void)hipEventDestroy(e);
    if (ev0_) (void)hipEventDestroy(ev0_);
    if (ev1_) (void)hipEventDestroy(ev1_);
    if (ev_user_) (void)hipEventDestroy(ev_user_);
    if (stream_) (void)hipStreamDestroy(stream_);
    weight_allocs_.clear(); prof_pending_.clear(); prof_free_.clear();
    ev0_ = ev1_ = ev_user_ = nullptr; stream_ = nullptr;
}

void Engine::add_entry(const std::string& name, int kind, std::initializer_list<int64_t> dims, float** dst, int wdt) {
    WeightEntry e;
    e.name = name; e.kind = kind; e.ndim = (int)dims.size(); e.dst = dst; e.wdt = wdt; e.group = cur_group_;
    int i = 0;
    for (int k = 0; k < 4; ++k) e.dims[k] = 1;
    for (auto d : dims) e.dims[i++] = d;
    entry_index_[name] = (int)entries_.size();
    entries_.push_back(e);
}

void Engine::add_meta(const std::string& name, int n, float e0, float e1, float* store) {
    MetaEntry m{name, n, {e0, e1}, store};
    meta_index_[name] = (int)meta_.size();
    meta_.push_back(m);
}

// The structs build_model() fills live in members / vectors whose storage is fixed
// before any entry is added (entries_ keeps float** into them).
void Engine::build_model() {
    const int mc = cfg_.model_channels, ed = 4 * mc, cd = cfg_.ctx_dim;
    const int c1 = mc, c2 = 2 * mc, c4 = 4 * mc;
    auto add = [](Engine* e, const std::string& n, int kind, std::initializer_list<int64_t> d, float** dst, int wdt = 0) { e->add_entry(n, kind, d, dst, wdt); };
    // precision = 1: weights of every layer with Cin % 64 == 0 are packed as bf16; the three Cin = 4
    // layers and the time-embedding MLPs (M = n_steps rows, once per call) stay fp32
    // stride / pad: what the engine applies to this layer; checked against the dump's metadata files (load_conv2d, load.rs:118-160)
    // keep_f32 (the ControlNet hint convolutions): fp32 weight, input and output at every precision, like the time MLPs -- they run once per call
    auto conv = [&](ConvW& w, const std::string& path, int cin, int cout, int k, int stride = 1, int pad = -1, bool keep_f32 = false) {
        w.cin = cin < 32 ? (cin + 3) / 4 * 4 : cin; w.cout = cout; w.k = k;   // what the layer reads: padded_cin of its weight (9 -> 12: a conditioned UNet's conv_in)
        w.dt = (bf16_ && cin % 64 == 0 && !keep_f32) ? 1 : 0;
        if (bf16_ && !w.dt && cin >= 32 && !keep_f32) throw Error(SDMI_ERR_UNSUPPORTED, "bf16: conv Cin must be a multiple of 64 (or < 32)");
        add(this, path + "/weight", 0, {cout, cin, k, k}, &w.bt, w.dt);
        add(this, path + "/bias", 2, {cout}, &w.bias);
        if (pad < 0) pad = k == 3 ? 1 : 0;
        add_meta(path + "/stride", 2, (float)stride, (float)stride, nullptr);
        add_meta(path + "/padding", 2, (float)pad, (float)pad, nullptr);
        add_meta(path + "/dilation", 2, 1.f, 1.f, nullptr);
        add_meta(path + "/kernel_size", 2, (float)k, (float)k, nullptr);
        add_meta(path + "/n_group", 1, 1.f, 0.f, nullptr);
    };
    auto lin = [&](LinW& w, const std::string& path, int cin, int cout, bool bias, bool keep_f32 = false) {
        w.cin = cin; w.cout = cout;
        w.dt = (bf16_ && !keep_f32) ? 1 : 0;
        if (w.dt && cin % 64) throw Error(SDMI_ERR_UNSUPPORTED, "bf16: linear in_features must be a multiple of 64");
        add(this, path + "/weight", 1, {cin, cout}, &w.bt, w.dt);
        if (bias) add(this, path + "/bias", 2, {cout}, &w.bias);
    };
    auto norm = [&](NormW& w, const std::string& path, int c, bool group_norm = true) {
        w.c = c;
        add(this, path + "/weight", 2, {c}, &w.gamma);
        add(this, path + "/bias", 2, {c}, &w.beta);
        add_meta(path + "/eps", 1, 0.f, 0.f, &w.eps);
        if (group_norm) {
            add_meta(path + "/n_group", 1, 32.f, 0.f, nullptr);   // GroupNormConfig::new(32, ..) everywhere (unet/mod.rs:692, autoencoder/mod.rs:483)
            add_meta(path + "/n_channel", 1, (float)c, 0.f, nullptr);
        }
    };
    // precision = 2: these convs (fed by a GroupNorm + SiLU, Cin % 32 == 0, Cout % 8 == 0) also get an MXFP8 copy of their weight
    auto fp8_copy = [&](ConvW& w, const std::string& weight_name) {
        if (!fp8_ || w.cin % 32 || w.cout % 8 || !w.dt) return;
        WeightEntry& e = entries_[entry_index_.at(weight_name)];
        e.dst8 = &w.bt8;
        e.dsts = &w.bs8;
    };
    // ... and (option fp8_linear) the Linear layers of the transformer blocks
    auto fp8_copy_lin = [&](LinW& w, const std::string& weight_name) {
        if (!fp8_ || w.cin % 32 || w.cout % 8 || !w.dt) return;
        WeightEntry& e = entries_[entry_index_.at(weight_name)];
        e.dst8 = &w.bt8;
        e.dsts = &w.bs8;
    };
    auto res = [&](ResW& r, const std::string& path, int cin, int cout, bool unet) {
        r.cin = cin; r.cout = cout; r.has_embed = unet; r.has_skip = cin != cout;
        if (unet) {  // ResBlock, unet/mod.rs:679-734; names unet/load.rs:20-25
            norm(r.norm_in, path + "/norm_in", cin);
            conv(r.conv_in, path + "/conv_in", cin, cout, 3);
            lin(r.lin_embed, path + "/lin_embed", ed, cout, true, /*keep_f32=*/true);
            norm(r.norm_out, path + "/norm_out", cout);
            conv(r.conv_out, path + "/conv_out", cout, cout, 3);
            if (r.has_skip) conv(r.skip, path + "/skip_connection", cin, cout, 1);
            fp8_copy(r.conv_in, path + "/conv_in/weight");
            fp8_copy(r.conv_out, path + "/conv_out/weight");
            if (r.has_skip) fp8_copy(r.skip, path + "/skip_connection/weight");
        } else {  // ResnetBlock, autoencoder/mod.rs:472-528; names autoencoder/load.rs:39-45
            norm(r.norm_in, path + "/norm1", cin);
            conv(r.conv_in, path + "/conv1", cin, cout, 3);
            norm(r.norm_out, path + "/norm2", cout);
            conv(r.conv_out, path + "/conv2", cout, cout, 3);
            if (r.has_skip) conv(r.skip, path + "/nin_shortcut", cin, cout, 1);
            fp8_copy(r.conv_in, path + "/conv1/weight");
            fp8_copy(r.conv_out, path + "/conv2/weight");
            // (the decoder's 1x1 shortcuts and up-convolutions stay bf16 under fp8_linear too: measured on MI355X, MXFP8 there moves the decoded
            // RGB from 2.1e-2 to 9.8e-2 relative RMS of the exact decode and saves 0.4 ms per image)
        }
    };
    auto mha = [&](MhaW& m, const std::string& path, int c, int cctx) {  // unet/mod.rs:603-653
        if (c == cctx) {
            // self-attention: query/key/value weights are packed into ONE [3c][c] buffer so the three
            // projections of unet/mod.rs:645-647 run as a single GEMM with N = 3c
            void* p = persistent_alloc((size_t)3 * c * c * esz());
            weight_allocs_.push_back(p);
            m.q.bt = reinterpret_cast<float*>(p);
            if (!bf16_) {   // and its bf16 planes (k_gemm3x.hip), same 1.5x offset rule as the arenas
                void* pl = persistent_alloc((size_t)3 * c * c * 6);
                weight_allocs_.push_back(pl);
                split_regions_.push_back(SplitRegion{reinterpret_cast<char*>(p), (size_t)3 * c * c * 4, reinterpret_cast<char*>(pl)});
            }
            m.q.fused = 3;
            m.k.bt = adv(m.q.bt, (long long)c * c, edt());
            m.v.bt = adv(m.q.bt, (long long)2 * c * c, edt());
            if (fp8_ && c % 32 == 0) {   // the packed [3c][Kp] MXFP8 copy + its scales: one N = 3c GEMM as well
                const size_t kp = (size_t)(c + 127) / 128 * 128;
                void* q8 = persistent_alloc((size_t)3 * c * kp);
                weight_allocs_.push_back(q8);
                void* s8 = persistent_alloc((size_t)3 * c * kp / 32);
                weight_allocs_.push_back(s8);
                m.q.bt8 = reinterpret_cast<float*>(q8);
                m.k.bt8 = reinterpret_cast<float*>((char*)q8 + (size_t)c * kp);
                m.v.bt8 = reinterpret_cast<float*>((char*)q8 + (size_t)2 * c * kp);
                m.q.bs8 = reinterpret_cast<float*>(s8);
                m.k.bs8 = reinterpret_cast<float*>((char*)s8 + (size_t)c * kp / 32);
                m.v.bs8 = reinterpret_cast<float*>((char*)s8 + (size_t)2 * c * kp / 32);
            }
        }
        lin(m.q, path + "/query", c, c, false);
        // precision >= 1: the bf16 attention kernel takes q in log2 units -- d_head^-0.5 log2(e) is folded into the query weight here, in
        // fp32, before its only rounding (attention.rs:15-26 applies d_head^-0.25 to q and to k)
        const int heads = unet_heads(c);
        if (q_prescaled(m.q.dt, c / heads)) entries_[entry_index_.at(path + "/query/weight")].pre_scale = attn_bf16_q_scale(c / heads);
        if (m.q.dt && c / heads == 64) q64_entries_.push_back(entry_index_.at(path + "/query/weight"));   // option attn_d64 decides their pre-scale
        lin(m.k, path + "/key", cctx, c, false);
        lin(m.v, path + "/value", cctx, c, false);
        lin(m.out, path + "/out", c, c, true);
        fp8_copy_lin(m.q, path + "/query/weight");
        if (c == cctx) { fp8_copy_lin(m.k, path + "/key/weight"); fp8_copy_lin(m.v, path + "/value/weight"); }   // (cross-attention K / V: hoisted, once per call, bf16)
        fp8_copy_lin(m.out, path + "/out/weight");
        add_meta(path + "/n_head", 1, (float)heads, 0.f, nullptr);
    };
    auto spatial = [&](SpatialW& s, const std::string& path, int c) {  // unet/mod.rs:436-527
        s.c = c;
        norm(s.norm, path + "/norm", c);
        conv(s.proj_in, path + "/proj_in", c, c, 1);
        const std::string t = path + "/transformer";
        norm(s.ln1, t + "/norm1", c, false);
        mha(s.attn1, t + "/attn1", c, c);
        norm(s.ln2, t + "/norm2", c, false);
        mha(s.attn2, t + "/attn2", c, cd);
        norm(s.ln3, t + "/norm3", c, false);
        lin(s.geglu_proj, t + "/mlp/geglu/proj", c, 8 * c, true);
        lin(s.mlp_lin, t + "/mlp/lin", 4 * c, c, true);
        conv(s.proj_out, path + "/proj_out", c, c, 1);
        fp8_copy(s.proj_in, path + "/proj_in/weight");
        fp8_copy(s.proj_out, path + "/proj_out/weight");
        fp8_copy_lin(s.geglu_proj, t + "/mlp/geglu/proj/weight");
        fp8_copy_lin(s.mlp_lin, t + "/mlp/lin/weight");
        // the entries the folded weights are derived from (rebuild_folds); idx_st ties them to the block
        s.fold_entries[0] = entry_index_.at(t + "/mlp/lin/weight");
        s.fold_entries[1] = entry_index_.at(t + "/mlp/lin/bias");
        s.fold_entries[2] = entry_index_.at(path + "/proj_out/weight");
    };

    add(this, "alphas_cumprod", 3, {1000}, nullptr);
    add_meta("n_steps", 1, 1000.f, 0.f, nullptr);   // stablediffusion/load.rs:20

    // ---- UNet (unet/mod.rs:36-92) ------------------------------------------------
    lin(lin1_time_, "unet/lin1_time_embed", mc, ed, true, /*keep_f32=*/true);
    lin(lin2_time_, "unet/lin2_time_embed", ed, ed, true, /*keep_f32=*/true);
    struct Spec { BlockKind kind; const char* name; int cin, cout; };
    const Spec in_spec[12] = {
        {BK_CONV, "conv", cfg_.unet_in_ch, c1},   {BK_RES_ST, "rt1", c1, c1}, {BK_RES_ST, "rt2", c1, c1}, {BK_DOWN, "d1", c1, c1},
        {BK_RES_ST, "rt3", c1, c2}, {BK_RES_ST, "rt4", c2, c2}, {BK_DOWN, "d2", c2, c2},    {BK_RES_ST, "rt5", c2, c4},
        {BK_RES_ST, "rt6", c4, c4}, {BK_DOWN, "d3", c4, c4},    {BK_RES, "r1", c4, c4},     {BK_RES, "r2", c4, c4}};
    const Spec out_spec[12] = {
        {BK_RES, "r1", 2 * c4, c4},        {BK_RES, "r2", 2 * c4, c4},        {BK_RES_UP, "ru", 2 * c4, c4},
        {BK_RES_ST, "rt1", 2 * c4, c4},    {BK_RES_ST, "rt2", 2 * c4, c4},    {BK_RES_ST_UP, "rtu1", c4 + c2, c4},
        {BK_RES_ST, "rt3", c4 + c2, c2},   {BK_RES_ST, "rt4", 2 * c2, c2},    {BK_RES_ST_UP, "rtu2", c2 + c1, c2},
        {BK_RES_ST, "rt5", c2 + c1, c1},   {BK_RES_ST, "rt6", 2 * c1, c1},    {BK_RES_ST, "rt7", 2 * c1, c1}};
    in_blocks_.resize(12);
    out_blocks_.resize(12);
    auto def_block = [&](UBlock& b, const Spec& s, const std::string& root) {
        b.kind = s.kind; b.cin = s.cin; b.cout = s.cout;
        const std::string path = root + "/" + s.name;
        switch (s.kind) {
            case BK_CONV: conv(b.conv, path, s.cin, s.cout, 3); break;
            case BK_DOWN: conv(b.conv, path, s.cin, s.cout, 3, 2); fp8_copy(b.conv, path + "/weight"); break;  // load_downsample: path itself (unet/load.rs:138-143); stride 2, pad 1 (unet/mod.rs:413-418)
            case BK_RES: res(b.res, path, s.cin, s.cout, true); break;
            default:
                res(b.res, path + "/res", s.cin, s.cout, true);
                if (s.kind == BK_RES_ST || s.kind == BK_RES_ST_UP) spatial(b.st, path + "/transformer", s.cout);
                if (s.kind == BK_RES_UP || s.kind == BK_RES_ST_UP) { conv(b.up, path + "/upsample/conv", s.cout, s.cout, 3); fp8_copy(b.up, path + "/upsample/conv/weight"); }
        }
    };
    // an up-convolution: its phase weights are derived from its weight entry (rebuild_folds)
    auto reg_up = [&](ConvW& w, const std::string& weight_name) {
        w.up_entry = entry_index_.at(weight_name);
        entries_[(size_t)w.up_entry].fold_up = (int)up_list_.size();
        up_list_.push_back(&w);
    };
    for (int i = 0; i < 12; ++i) def_block(in_blocks_[i], in_spec[i], "unet/input_blocks");
    res(mid_res1_, "unet/middle_block/res1", c4, c4, true);
    spatial(mid_st_, "unet/middle_block/transformer", c4);
    res(mid_res2_, "unet/middle_block/res2", c4, c4, true);
    for (int i = 0; i < 12; ++i) def_block(out_blocks_[i], out_spec[i], "unet/output_blocks");
    for (int i = 0; i < 12; ++i)
        if (out_spec[i].kind == BK_RES_UP || out_spec[i].kind == BK_RES_ST_UP) reg_up(out_blocks_[i].up, std::string("unet/output_blocks/") + out_spec[i].name + "/upsample/conv/weight");
    norm(unet_norm_out_, "unet/norm_out", c1);
    conv(unet_conv_out_, "unet/conv_out", c1, 4, 3);

    // index ResBlocks / SpatialTransformers for the hoisted per-call tables
    auto idx_res = [&](ResW& r) { r.temb_index = (int)res_list_.size(); res_list_.push_back(&r); };
    auto idx_st = [&](SpatialW& s) {
        s.ctx_index = (int)st_list_.size();
        st_list_.push_back(&s);
        for (int i : s.fold_entries) entries_[(size_t)i].fold_st = s.ctx_index;
    };
    auto idx_block = [&](UBlock& b) {
        if (b.kind == BK_CONV || b.kind == BK_DOWN) return;
        idx_res(b.res);
        if (b.kind == BK_RES_ST || b.kind == BK_RES_ST_UP) idx_st(b.st);
    };
    for (auto& b : in_blocks_) idx_block(b);
    idx_res(mid_res1_); idx_st(mid_st_); idx_res(mid_res2_);
    for (auto& b : out_blocks_) idx_block(b);
    n_res_unet_ = res_list_.size();
    n_st_unet_ = st_list_.size();

    // ---- VAE decoder (autoencoder/mod.rs:30-36,154-191) ------------------------------
    const int vc = cfg_.vae_ch;
    const int dch[4][2] = {{4 * vc, 4 * vc}, {4 * vc, 4 * vc}, {4 * vc, 2 * vc}, {2 * vc, vc}};
    conv(post_quant_, "autoencoder/post_quant_conv", 4, 4, 1);
    conv(dec_conv_in_, "autoencoder/decoder/conv_in", 4, 4 * vc, 3);
    res(dec_mid1_, "autoencoder/decoder/mid/block_1", 4 * vc, 4 * vc, false);
    dec_attn_.c = 4 * vc;
    norm(dec_attn_.norm, "autoencoder/decoder/mid/attn/norm", 4 * vc);
    conv(dec_attn_.q, "autoencoder/decoder/mid/attn/q", 4 * vc, 4 * vc, 1);
    conv(dec_attn_.k, "autoencoder/decoder/mid/attn/k", 4 * vc, 4 * vc, 1);
    conv(dec_attn_.v, "autoencoder/decoder/mid/attn/v", 4 * vc, 4 * vc, 1);
    conv(dec_attn_.proj_out, "autoencoder/decoder/mid/attn/proj_out", 4 * vc, 4 * vc, 1);
    res(dec_mid2_, "autoencoder/decoder/mid/block_2", 4 * vc, 4 * vc, false);
    for (int i = 0; i < 4; ++i) {
        DecBlockW& b = dec_blocks_[i];
        b.cin = dch[i][0]; b.cout = dch[i][1]; b.has_up = i != 3;
        const std::string bp = "autoencoder/decoder/blocks/" + std::to_string(i);
        res(b.res[0], bp + "/res1", b.cin, b.cout, false);
        res(b.res[1], bp + "/res2", b.cout, b.cout, false);
        res(b.res[2], bp + "/res3", b.cout, b.cout, false);
        if (b.has_up) { conv(b.upsampler, bp + "/upsampler", b.cout, b.cout, 3); reg_up(b.upsampler, bp + "/upsampler/weight"); }
    }
    norm(dec_norm_out_, "autoencoder/decoder/norm_out", vc);
    conv(dec_conv_out_, "autoencoder/decoder/conv_out", vc, 3, 3);

    // ---- CLIP text encoder (clip/mod.rs:18-45; dump names clip/load.rs:14-91) -- SURVEY 8f rank 2 -------------
    // An optional weight group: the sampling path takes the text embedding as an input, so a context without
    // CLIP weights is complete; sdmi_clip_forward / sdmi_context need the whole group.  Always fp32.
    if (cfg_.clip_layers > 0) {
        const int cs = cd, L = cfg_.clip_layers, H = cfg_.clip_heads;
        if (H <= 0 || cs % H || !attn_supported_head_dim(cs / H) || cfg_.clip_vocab <= 0 || cfg_.clip_ctx <= 0 || cs % 32)
            throw Error(SDMI_ERR_UNSUPPORTED, "CLIP: ctx_dim / clip_heads must be one of the fused attention head dims (40, 64, 80, 160)");
        cur_group_ = 1;
        add(this, "clip/token_embedding/weight", 2, {cfg_.clip_vocab, cs}, &clip_tok_);
        add(this, "clip/position_embedding/weight", 2, {cfg_.clip_ctx, cs}, &clip_pos_);
        clip_blocks_.resize(L);
        for (int i = 0; i < L; ++i) {
            ClipBlockW& b = clip_blocks_[i];
            const std::string bp = "clip/blocks/" + std::to_string(i);
            void* w = persistent_alloc((size_t)3 * cs * cs * sizeof(float));
            weight_allocs_.push_back(w);
            void* bias = persistent_alloc((size_t)3 * cs * sizeof(float));
            weight_allocs_.push_back(bias);
            b.q.bt = reinterpret_cast<float*>(w); b.k.bt = b.q.bt + (size_t)cs * cs; b.v.bt = b.q.bt + (size_t)2 * cs * cs;
            b.q.bias = reinterpret_cast<float*>(bias); b.k.bias = b.q.bias + cs; b.v.bias = b.q.bias + 2 * cs;
            b.q.fused = 3;
            norm(b.attn_ln, bp + "/attn_ln", cs, false);
            lin(b.q, bp + "/attn/query", cs, cs, true, true);   // MultiHeadSelfAttention: all four Linears carry a bias
            lin(b.k, bp + "/attn/key", cs, cs, true, true);
            lin(b.v, bp + "/attn/value", cs, cs, true, true);
            lin(b.out, bp + "/attn/out", cs, cs, true, true);
            norm(b.mlp_ln, bp + "/mlp_ln", cs, false);
            lin(b.fc1, bp + "/mlp/fc1", cs, 4 * cs, true, true);
            lin(b.fc2, bp + "/mlp/fc2", 4 * cs, cs, true, true);
        }
        norm(clip_ln_, "clip/layer_norm", cs, false);
        cur_group_ = 0;
    }

    // ---- VAE encoder (autoencoder/mod.rs:30-32,76-144,220-265; names autoencoder/load.rs:120-190) -- SURVEY 8f rank 4
    // Optional weight group: txt2img never encodes; sdmi_encode_image and sdmi_img2img_image need the whole group.
    {
        cur_group_ = 2;
        const int ech[4][2] = {{vc, vc}, {vc, 2 * vc}, {2 * vc, 4 * vc}, {4 * vc, 4 * vc}};
        enc_conv_in_.cin = 4; enc_conv_in_.cout = vc; enc_conv_in_.k = 3; enc_conv_in_.dt = 0;   // RGB + one zero channel
        add(this, "autoencoder/encoder/conv_in/weight", 0, {vc, 3, 3, 3}, &enc_conv_in_.bt);
        add(this, "autoencoder/encoder/conv_in/bias", 2, {vc}, &enc_conv_in_.bias);
        for (int i = 0; i < 4; ++i) {
            EncBlockW& b = enc_blocks_[i];
            b.cin = ech[i][0]; b.cout = ech[i][1]; b.has_down = i != 3;
            const std::string bp = "autoencoder/encoder/blocks/" + std::to_string(i);
            res(b.res[0], bp + "/res1", b.cin, b.cout, false);
            res(b.res[1], bp + "/res2", b.cout, b.cout, false);
            if (b.has_down) conv(b.down, bp + "/downsampler/conv", b.cout, b.cout, 3, 2, 0);   // load_padded_conv2d: "{path}/conv", saved with padding (0, 0) (python/save.py:73-76)
        }
        res(enc_mid1_, "autoencoder/encoder/mid/block_1", 4 * vc, 4 * vc, false);
        enc_attn_.c = 4 * vc;
        norm(enc_attn_.norm, "autoencoder/encoder/mid/attn/norm", 4 * vc);
        conv(enc_attn_.q, "autoencoder/encoder/mid/attn/q", 4 * vc, 4 * vc, 1);
        conv(enc_attn_.k, "autoencoder/encoder/mid/attn/k", 4 * vc, 4 * vc, 1);
        conv(enc_attn_.v, "autoencoder/encoder/mid/attn/v", 4 * vc, 4 * vc, 1);
        conv(enc_attn_.proj_out, "autoencoder/encoder/mid/attn/proj_out", 4 * vc, 4 * vc, 1);
        res(enc_mid2_, "autoencoder/encoder/mid/block_2", 4 * vc, 4 * vc, false);
        norm(enc_norm_out_, "autoencoder/encoder/norm_out", 4 * vc);
        conv(enc_conv_out_, "autoencoder/encoder/conv_out", 4 * vc, 8, 3);
        conv(quant_conv_, "autoencoder/quant_conv", 8, 8, 1);
        cur_group_ = 0;
    }

    // ---- ControlNet (cldm.py ControlNet): no reference counterpart -------------------------------------------------
    // Optional weight group 3: a second copy of the UNet's time MLP, encoder and middle block under the root "controlnet" -- the same lambdas, hence the same dump
    // naming, storage types and MXFP8 copies as their UNet twins -- plus the hint convolutions (fp32 at every precision; the widths 16 / 32 / 96 / 256 are
    // ControlNet's constants), one zero convolution per input block and middle_block_out.  Its ResBlocks and transformers follow the UNet's in res_list_ / st_list_.
    if (cfg_.control_hint_ch) {
        cur_group_ = 3;
        lin(ctl_lin1_time_, "controlnet/lin1_time_embed", mc, ed, true, /*keep_f32=*/true);
        lin(ctl_lin2_time_, "controlnet/lin2_time_embed", ed, ed, true, /*keep_f32=*/true);
        ctl_blocks_.resize(12);
        for (int i = 0; i < 12; ++i) {
            Spec sp = in_spec[i];
            if (i == 0) sp.cin = 4;
            def_block(ctl_blocks_[i], sp, "controlnet/input_blocks");
        }
        res(ctl_mid_res1_, "controlnet/middle_block/res1", c4, c4, true);
        spatial(ctl_mid_st_, "controlnet/middle_block/transformer", c4);
        res(ctl_mid_res2_, "controlnet/middle_block/res2", c4, c4, true);
        const int hch[9] = {cfg_.control_hint_ch, 16, 16, 32, 32, 96, 96, 256, mc};
        for (int i = 0; i < 8; ++i)
            conv(ctl_hint_[i], "controlnet/hint/c" + std::to_string(i), hch[i], hch[i + 1], 3, (i == 2 || i == 4 || i == 6) ? 2 : 1, 1, /*keep_f32=*/true);
        for (int j = 0; j < 12; ++j) conv(ctl_zero_[j], "controlnet/zero_convs/" + std::to_string(j), in_spec[j].cout, in_spec[j].cout, 1);
        conv(ctl_mid_out_, "controlnet/middle_block_out", c4, c4, 1);
        for (auto& b : ctl_blocks_) idx_block(b);
        idx_res(ctl_mid_res1_); idx_st(ctl_mid_st_); idx_res(ctl_mid_res2_);
        cur_group_ = 0;
    }
}

// =============================================================================
// weights
// =============================================================================
// Loading is batched: every tensor goes host -> pinned ring -> (device staging ->) packing kernel -> its slot of
// ONE device arena per weight group, all asynchronous on the engine's stream; the callers synchronise once
// (load_weights_dir / load_weights_packed) or per tensor (set_weight, whose source may be freed on return).
// The reference builds ~1100 Burn tensors one file at a time (stablediffusion/load.rs:16-33, model/load.rs:30-46).
static constexpr size_t kStageBytes = (size_t)160 << 20;   // >= the largest tensor (CLIP token table, 152 MB)

struct Engine::Stager {
    char* pinned[2] = {nullptr, nullptr};
    char* dev[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    size_t used = 0;
    int cur = 0;
    ~Stager() {
        for (int i = 0; i < 2; ++i) {
            if (done[i]) { (void)hipEventSynchronize(done[i]); (void)hipEventDestroy(done[i]); }
            if (pinned[i]) (void)hipHostFree(pinned[i]);
            if (dev[i]) (void)hipFree(dev[i]);
        }
    }
};

void Engine::stager_release() { stager_.reset(); }

// `bytes` of pinned host memory (256-byte aligned) the caller fills; valid until the matching commit
char* Engine::stage_reserve(size_t bytes, size_t* offset, int* half) {
    if (bytes > kStageBytes) throw Error(SDMI_ERR_UNSUPPORTED, "weight tensor larger than the staging buffer");
    if (!stager_) {
        stager_.reset(new Stager());
        for (int i = 0; i < 2; ++i) {
            SDMI_HIP(hipHostMalloc((void**)&stager_->pinned[i], kStageBytes, hipHostMallocDefault));
            SDMI_HIP(hipMalloc((void**)&stager_->dev[i], kStageBytes));
            SDMI_HIP(hipEventCreateWithFlags(&stager_->done[i], hipEventDisableTiming));
        }
    }
    Stager& st = *stager_;
    const size_t need = (bytes + 255) / 256 * 256;
    if (st.used + need > kStageBytes) {   // this half is full: mark it in flight, move to the other one
        SDMI_HIP(hipEventRecord(st.done[st.cur], stream_));
        st.busy[st.cur] = true;
        st.cur ^= 1;
        st.used = 0;
        if (st.busy[st.cur]) { SDMI_HIP(hipEventSynchronize(st.done[st.cur])); st.busy[st.cur] = false; }
    }
    *offset = st.used;
    *half = st.cur;
    st.used += need;
    return st.pinned[st.cur] + *offset;
}

void* Engine::persistent_alloc(size_t bytes, bool weight_buffer) {
    void* p = nullptr;
    SDMI_HIP(hipMalloc(&p, bytes));
    if (pool_.fill() >= 0) {
        hipError_t e = hipMemsetAsync(p, pool_.fill(), bytes, stream_);
        if (e == hipSuccess && !weight_buffer) e = hipStreamSynchronize(stream_);
        if (e != hipSuccess) { (void)hipFree(p); SDMI_HIP(e); }
        pool_.note_fill(bytes);
    }
    if (weight_buffer) persistent_blocks_.push_back({p, bytes});
    return p;
}

void Engine::ensure_arena(int group) {
    if (arena_done_[group]) return;
    size_t total = 0;
    for (auto& e : entries_) {
        if (e.group != group || e.kind == 3 || *e.dst) continue;
        const size_t count = stage_elems(e);   // (a conv_in with padded input channels: the padded count)
        total += (count * (e.wdt ? 2 : 4) + 255) / 256 * 256;
    }
    if (total) {
        char* base = static_cast<char*>(persistent_alloc(total));
        weight_allocs_.push_back(base);
        arena_base_[group] = base;
        arena_bytes_[group] = total;
        if (!bf16_) {
            split_base_[group] = static_cast<char*>(persistent_alloc(total / 2 * 3));
            weight_allocs_.push_back(split_base_[group]);
        }
        size_t off = 0;
        for (auto& e : entries_) {
            if (e.group != group || e.kind == 3 || *e.dst) continue;
            const size_t count = stage_elems(e);
            *e.dst = reinterpret_cast<float*>(base + off);
            off += (count * (e.wdt ? 2 : 4) + 255) / 256 * 256;
        }
    }
    if (opt_keep_masters_) {   // the fp32 masters of every conv / Linear tensor of the group (the packed q | k | v members included), same slot rule
        size_t mtotal = 0;
        for (auto& e : entries_)
            if (e.group == group && e.kind <= 1) mtotal += (stage_elems(e) * sizeof(float) + 255) / 256 * 256;
        if (mtotal) {
            char* mbase = static_cast<char*>(persistent_alloc(mtotal));
            weight_allocs_.push_back(mbase);
            size_t off = 0;
            for (auto& e : entries_) {
                if (e.group != group || e.kind > 1) continue;
                e.master = reinterpret_cast<float*>(mbase + off);
                off += (stage_elems(e) * sizeof(float) + 255) / 256 * 256;
            }
        }
    }
    arena_done_[group] = true;
}

Engine::TempSplit::TempSplit(Engine* e_, const float* bt_, long long rows, long long K) : e(e_), bt(bt_) {
    if (e->bf16_ || K % 32 || rows <= 0) return;
    planes = e->pool_.alloc((size_t)rows * K * 6);
    hipError_t err = launch_pack_split3(bt, planes, rows, (int)K, e->stream_, e->b3_grouped(rows));
    if (err != hipSuccess) { e->pool_.free(planes); planes = nullptr; SDMI_HIP(err); }
    const int slot = e->temp_split_bt_[0] ? 1 : 0;   // (two at a time: op_conv2d_pair's weights)
    e->temp_split_bt_[slot] = bt;
    e->temp_split_planes_[slot] = planes;
}
Engine::TempSplit::~TempSplit() {
    if (!planes) return;
    const int slot = e->temp_split_planes_[0] == planes ? 0 : 1;
    e->temp_split_bt_[slot] = nullptr;
    e->temp_split_planes_[slot] = nullptr;
    e->pool_.free(planes);
}

const void* Engine::split_planes(const float* bt) const {
    for (int slot = 0; slot < 2; ++slot)
        if (bt && bt == temp_split_bt_[slot]) return temp_split_planes_[slot];
    const char* b = reinterpret_cast<const char*>(bt);
    for (int g = 0; g < kGroups; ++g)
        if (split_base_[g] && b >= arena_base_[g] && b < arena_base_[g] + arena_bytes_[g]) return split_base_[g] + (size_t)(b - arena_base_[g]) / 2 * 3;
    for (const SplitRegion& r : split_regions_)    // the packed q | k | v weights of the self-attentions (own allocations)
        if (b >= r.base && b < r.base + r.bytes) return r.planes + (size_t)(b - r.base) / 2 * 3;
    return nullptr;
}

static size_t entry_count(const WeightEntry& e) {
    size_t count = 1;
    for (int i = 0; i < e.ndim; ++i) count *= (size_t)e.dims[i];
    return count;
}

// THE rule for a convolution's stored input channels: Cin < 32 is kept as one channel slice, which the GEMM kernels read in 16-byte pieces, so it is zero-padded
// up to the next multiple of 4 (the RGB conv_in of the VAE encoder 3 -> 4, the 9-channel conv_in of an inpainting UNet 9 -> 12; 4 and 8 stay).
int64_t Engine::padded_conv_cin(int64_t cin) { return cin < 32 ? (cin + 3) / 4 * 4 : cin; }

int Engine::padded_cin(const WeightEntry& e) {
    return e.kind == 0 ? (int)padded_conv_cin(e.dims[1]) : (int)e.dims[1];
}

size_t Engine::stage_elems(const WeightEntry& e) {
    const size_t count = entry_count(e);
    return e.kind == 0 ? count / (size_t)e.dims[1] * (size_t)padded_cin(e) : count;
}

void Engine::pack_entry(WeightEntry& e, float* stage) {
    const size_t n_stage = stage_elems(e);
    fold_touch(e);
    if (e.pre_scale != 1.f) SDMI_HIP(launch_scale_f32(stage, (long long)n_stage, e.pre_scale, stream_));
    hipError_t err;
    if (e.kind == 0) {
        const int cout = (int)e.dims[0], cin = padded_cin(e), k = (int)e.dims[2];
        if (!(cin % 32 == 0 || (cin < 32 && cin % 4 == 0))) throw Error(SDMI_ERR_UNSUPPORTED, "conv Cin must be a multiple of 32, or < 32 and a multiple of 4");
        err = e.wdt ? launch_pack_conv_weight_bf16(stage, *e.dst, cout, cin, k, k, stream_)
                    : launch_pack_conv_weight(stage, *e.dst, cout, cin, k, k, stream_);
        if (err == hipSuccess && e.dst8) {
            const size_t kp = (size_t)((cin + 127) / 128 * 128) * k * k;
            if (!*e.dst8) {
                void* q = persistent_alloc((size_t)cout * kp);
                weight_allocs_.push_back(q);
                void* sc = persistent_alloc((size_t)cout * kp / 32);
                weight_allocs_.push_back(sc);
                *e.dst8 = reinterpret_cast<float*>(q);
                *e.dsts = reinterpret_cast<float*>(sc);
            }
            err = launch_pack_conv_weight_fp8(stage, *e.dst8, *e.dsts, cout, cin, k, k, stream_);
        }
    } else {
        err = e.wdt ? launch_pack_linear_weight_bf16(stage, *e.dst, (int)e.dims[0], (int)e.dims[1], stream_)
                    : launch_pack_linear_weight(stage, *e.dst, (int)e.dims[0], (int)e.dims[1], stream_);
        if (err == hipSuccess && e.dst8) {
            const int cin = (int)e.dims[0], cout = (int)e.dims[1];
            const size_t kp = (size_t)(cin + 127) / 128 * 128;
            if (!*e.dst8) {
                void* q = persistent_alloc((size_t)cout * kp);
                weight_allocs_.push_back(q);
                void* sc = persistent_alloc((size_t)cout * kp / 32);
                weight_allocs_.push_back(sc);
                *e.dst8 = reinterpret_cast<float*>(q);
                *e.dsts = reinterpret_cast<float*>(sc);
            }
            err = launch_pack_linear_weight_fp8(stage, *e.dst8, *e.dsts, cin, cout, stream_);
        }
    }
    SDMI_HIP(err);
    if (!e.wdt) {   // the bf16 planes of the packed fp32 rows (k_gemm3x.hip)
        const long long rows = e.kind == 0 ? e.dims[0] : e.dims[1];
        const long long K = e.kind == 0 ? (long long)padded_cin(e) * e.dims[2] * e.dims[3] : e.dims[0];
        void* planes = const_cast<void*>(split_planes(*e.dst));
        if (planes && K % 32 == 0) SDMI_HIP(launch_pack_split3(*e.dst, planes, rows, (int)K, stream_, b3_grouped(rows)));
    }
}

// Enqueues the upload + packing of one tensor whose fp32 values (reference layout) the caller has written to the
// pinned block (half, offset) returned by stage_reserve.
void Engine::stage_commit(WeightEntry& e, size_t offset, int half) {
    Stager& st = *stager_;
    const size_t count = entry_count(e);
    const float* host = reinterpret_cast<const float*>(st.pinned[half] + offset);
    if (e.kind == 3) {
        alphas_loaded_.assign(host, host + count);
        refresh_schedule();
        e.set = true;
        return;
    }
    ensure_arena(e.group);
    if (e.kind == 2) {
        fold_touch(e);
        SDMI_HIP(hipMemcpyAsync(*e.dst, host, count * sizeof(float), hipMemcpyHostToDevice, stream_));
    } else {
        float* stage = reinterpret_cast<float*>(st.dev[half] + offset);
        const size_t n_stage = stage_elems(e);   // (a padded conv_in: padded on the host by the caller of stage_commit)
        SDMI_HIP(hipMemcpyAsync(stage, host, n_stage * sizeof(float), hipMemcpyHostToDevice, stream_));
        if (e.master) SDMI_HIP(hipMemcpyAsync(e.master, stage, n_stage * sizeof(float), hipMemcpyDeviceToDevice, stream_));
        pack_entry(e, stage);
    }
    e.set = true;
    if (e.group != 3) finalized_ = false;   // (a ControlNet tensor may arrive behind finalize_weights: control_ready() counts)
}

// copies one tensor into the pinned ring (zero-padding the input channels of a conv_in that is stored padded: padded_cin) and commits it
void Engine::upload_weight(WeightEntry& e, const float* data) {
    const size_t count = entry_count(e);
    size_t off; int half;
    if (e.kind == 0 && padded_cin(e) != e.dims[1]) {
        const int cout = (int)e.dims[0], T = (int)(e.dims[2] * e.dims[3]), cin = (int)e.dims[1], pc = padded_cin(e);
        float* dst = reinterpret_cast<float*>(stage_reserve((size_t)cout * pc * T * sizeof(float), &off, &half));
        std::memset(dst, 0, (size_t)cout * pc * T * sizeof(float));
        for (int o = 0; o < cout; ++o) std::memcpy(dst + (size_t)o * pc * T, data + (size_t)o * cin * T, (size_t)cin * T * sizeof(float));
    } else {
        char* dst = stage_reserve(count * sizeof(float), &off, &half);
        std::memcpy(dst, data, count * sizeof(float));
    }
    stage_commit(e, off, half);
}

// Module metadata the reference's loaders read next to the tensors (python/save.py:23-68): a norm's `eps` is honoured
// (groupnorm/load.rs:19, load.rs:load_layer_norm), everything else must equal what this engine is built for.
bool Engine::set_meta(const std::string& name, const float* values, size_t n) {
    auto it = meta_index_.find(name);
    if (it == meta_index_.end()) return false;
    MetaEntry& m = meta_[it->second];
    if ((int)n != m.n) throw Error(SDMI_ERR_WEIGHTS, "'" + name + "' holds " + std::to_string(n) + " values, expected " + std::to_string(m.n));
    if (m.store) {
        if (!(values[0] > 0.f) || values[0] > 1.f) throw Error(SDMI_ERR_WEIGHTS, "'" + name + "': eps out of range");
        *m.store = values[0];
        return true;
    }
    for (int i = 0; i < m.n; ++i)
        if (values[i] != m.expect[i]) {
            std::ostringstream os;
            os << "'" << name << "' = " << values[i] << " but this engine is built for " << m.expect[i]
               << " (the reference's loaders honour the file; a dump with different hyper-parameters needs a matching sdmi_config)";
            throw Error(SDMI_ERR_WEIGHTS, os.str());
        }
    return true;
}

void Engine::set_weight(const char* name, const float* data, int ndim, const int64_t* dims) {
    if (!name || !data || !dims) throw Error(SDMI_ERR_INVALID, "set_weight: null argument");
    if (meta_index_.count(name)) {
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= (size_t)dims[i];
        set_meta(name, data, n);
        return;
    }
    auto it = entry_index_.find(name);
    if (it == entry_index_.end()) throw Error(SDMI_ERR_WEIGHTS, std::string("set_weight: unknown tensor '") + name + "'");
    WeightEntry& e = entries_[it->second];
    bool ok = ndim == e.ndim;
    for (int i = 0; ok && i < ndim; ++i) ok = dims[i] == e.dims[i];
    if (!ok) {
        std::ostringstream os;
        os << "set_weight: '" << name << "' expects shape [";
        for (int i = 0; i < e.ndim; ++i) os << (i ? "," : "") << e.dims[i];
        os << "], got [";
        for (int i = 0; i < ndim; ++i) os << (i ? "," : "") << dims[i];
        os << "]";
        throw Error(SDMI_ERR_WEIGHTS, os.str());
    }
    // a tensor under an active adapter is refused here, before anything is staged (the bulk loaders refuse at their start: lora_refuse_bulk_load)
    if (e.master && lora_active_on(it->second))
        throw Error(SDMI_ERR_STATE, std::string("set_weight: '") + name + "' carries a LoRA adapter with a non-zero scale: set its scale to 0 first");
    SDMI_HIP(hipSetDevice(cfg_.device));
    upload_weight(e, data);   // data is copied into the pinned ring before this returns: the caller may free it
    // a ControlNet tensor behind finalize_weights leaves finalized_ alone, so no later finalize releases the pinned ring: the tensor that completes the group does
    if (e.group == 3 && finalized_ && control_ready()) {
        rebuild_folds();
        SDMI_HIP(hipStreamSynchronize(stream_));
        stager_release();
    }
}

size_t Engine::packed_size(int groups) const {
    size_t n = 0;
    for (auto& e : entries_)
        if (groups & (1 << e.group)) n += entry_count(e);
    return n;
}

void Engine::load_weights_packed(const float* data, size_t n_floats, int groups) {
    if (!data) throw Error(SDMI_ERR_INVALID, "load_weights_packed: null pointer");
    if (groups <= 0 || groups > 7) throw Error(SDMI_ERR_INVALID, "load_weights_packed: groups is a bit mask of 1 (hot path), 2 (CLIP), 4 (VAE encoder)");
    lora_refuse_bulk_load("load_weights_packed");
    if (n_floats != packed_size(groups)) throw Error(SDMI_ERR_WEIGHTS, "load_weights_packed: expected " + std::to_string(packed_size(groups)) + " floats, got " + std::to_string(n_floats));
    SDMI_HIP(hipSetDevice(cfg_.device));
    size_t off = 0;
    for (auto& e : entries_) {
        if (!(groups & (1 << e.group))) continue;
        upload_weight(e, data + off);
        off += entry_count(e);
    }
    SDMI_HIP(hipStreamSynchronize(stream_));
    stager_release();
}

// load_stable_diffusion_model_file (src/bin/sample/main.rs:27-34): the Burn record, read natively (mpk_reader.hpp for the
// assumed layout).  Tensors the configured model does not have (e.g. clip/... with clip_layers = 0) are skipped.
void Engine::load_weights_mpk(const char* path) {
    if (!path) throw Error(SDMI_ERR_INVALID, "load_weights_mpk: null path");
    SDMI_HIP(hipSetDevice(cfg_.device));
    lora_refuse_bulk_load("load_weights_mpk");
    MpkFile f(path);
    size_t used = 0;
    for (const MpkTensor& t : f.tensors()) {
        auto it = entry_index_.find(t.name);
        if (it == entry_index_.end()) continue;
        WeightEntry& e = entries_[it->second];
        bool ok = (int)t.shape.size() == e.ndim;
        for (int i = 0; ok && i < e.ndim; ++i) ok = t.shape[i] == e.dims[i];
        if (!ok) {
            std::ostringstream os;
            os << "load_weights_mpk: '" << t.name << "' has shape [";
            for (size_t i = 0; i < t.shape.size(); ++i) os << (i ? "," : "") << t.shape[i];
            os << "], the configured model expects [";
            for (int i = 0; i < e.ndim; ++i) os << (i ? "," : "") << e.dims[i];
            os << "]";
            throw Error(SDMI_ERR_WEIGHTS, os.str());
        }
        upload_weight(e, reinterpret_cast<const float*>(t.data));   // memcpy into the pinned ring: any alignment
        ++used;
    }
    if (!used) throw Error(SDMI_ERR_WEIGHTS, std::string("load_weights_mpk: no tensor of ") + path + " matches the configured model");
    SDMI_HIP(hipStreamSynchronize(stream_));
    stager_release();
}

// An SD v1.x checkpoint in the CompVis layout, one .safetensors file.  Every weight entry is looked up under the key
// checkpoint_key derives from its dump name; the tensor's RAW bytes go mapping -> pinned ring -> device as they are (half the bytes for F16 / BF16), and ONE
// launch of k_unpack.hip writes the fp32 tensor in the reference's layout -- into a stage buffer for the consumers of stage_commit (conv / Linear: master copy,
// pre_scale, pack_entry as for every other loader), or straight into the arena slot (norms, biases, embedding tables).  Everything about the file is checked
// before the first tensor is staged, so a refused file leaves the context as it was.  Keys the model has no entry for (model_ema.*, position_ids, ...) are skipped.
static int unpack_dtype(const std::string& d) { return d == "F32" ? 0 : d == "F16" ? 1 : d == "BF16" ? 2 : -1; }

static float raw_to_f32(const unsigned char* p, const std::string& dtype, size_t i) {   // host twin of k_unpack.hip's conversions, + F64 (alphas_cumprod)
    if (dtype == "F64") { double v; std::memcpy(&v, p + 8 * i, 8); return (float)v; }
    uint32_t bits;
    if (dtype == "F32") {
        std::memcpy(&bits, p + 4 * i, 4);
    } else {
        uint16_t h;
        std::memcpy(&h, p + 2 * i, 2);
        if (dtype == "BF16") {
            bits = (uint32_t)h << 16;
        } else {
            const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, ex = (h >> 10) & 31u;
            uint32_t man = h & 0x3ffu;
            if (ex == 0) {
                if (man == 0) bits = sign;
                else { uint32_t s = 0; while (!(man & 0x400u)) { man <<= 1; ++s; } bits = sign | ((113u - s) << 23) | ((man & 0x3ffu) << 13); }
            } else {
                bits = sign | ((ex == 31 ? 255u : ex + 112u) << 23) | (man << 13);
            }
        }
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

static std::string shape_str(const int64_t* d, size_t n) {
    std::string s = "[";
    for (size_t i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string(d[i]);
    return s + "]";
}

void Engine::load_weights_safetensors(const char* path) { load_safetensors_groups(path, false); }

// A ControlNet in the cldm layout ("control_model.…") -> weight group 3, by the same route.  Every tensor of the group must be in the file.
void Engine::load_control_safetensors(const char* path) {
    if (!has_control()) throw Error(SDMI_ERR_STATE, "load_control_safetensors: this context has no ControlNet (sdmi_config.control_hint_ch = 0)");
    load_safetensors_groups(path, true);
}

void Engine::load_safetensors_groups(const char* path, bool control) {
    const std::string fn_name = control ? "load_control_safetensors" : "load_weights_safetensors";
    if (!path) throw Error(SDMI_ERR_INVALID, fn_name + ": null path");
    SDMI_HIP(hipSetDevice(cfg_.device));
    lora_refuse_bulk_load(fn_name.c_str());
    SafetensorsFile f(path);
    // data / nbytes: the bytes the entry is made from -- the key's whole tensor, or (variant = 1: the text encoder's fused attn.in_proj_*) one of its three row
    // blocks, a view of the mapping: no host copy, the same widen-and-transpose launch
    struct Job { WeightEntry* e; const StTensor* t; int dtype; int transform; const unsigned char* data; size_t nbytes; };
    std::vector<Job> jobs;
    if (!control) {   // a file of the other model family: refused here, before anything is looked up or staged
        const char* other = cfg_.variant == 1 ? kFamilyKeySd1 : kFamilyKeySd2;
        if (f.find(other))
            throw Error(SDMI_ERR_WEIGHTS, fn_name + ": " + path + " holds '" + other + "': " + (cfg_.variant == 1 ? "an SD v1 checkpoint, and this context is SD 2.x (variant = 1)"
                                                                                                              : "an SD 2.x checkpoint, and this context is SD v1 (variant = 0)"));
    }
    const StTensor* alphas = nullptr;
    WeightEntry* alphas_entry = nullptr;
    for (auto& e : entries_) {
        if ((e.group == 3) != control) continue;   // a ControlNet comes in a file of its own (load_control_safetensors)
        std::string key;
        bool transposed = false;
        int slice = -1;
        if (!checkpoint_key(e.name, cfg_.variant, &key, &transposed, &slice)) throw Error(SDMI_ERR_STATE, fn_name + ": no checkpoint key rule for '" + e.name + "'");
        const StTensor* t = f.find(key);
        if (e.kind == 3) { alphas = t; alphas_entry = &e; continue; }   // optional: the LDM schedule is computed when the file has none
        if (!t) {
            if (e.group == 0 || control)
                throw Error(SDMI_ERR_WEIGHTS, std::string(fn_name + ": ") + path + " has no tensor '" + key + "' (the source of '" + e.name + "')");
            continue;   // CLIP / VAE encoder: all or nothing, decided by finalize_weights (a ControlNet: by this loader, above)
        }
        const int dt = unpack_dtype(t->dtype);
        if (dt < 0) throw Error(SDMI_ERR_UNSUPPORTED, fn_name + ": '" + key + "' has dtype " + t->dtype + "; F32, F16 and BF16 are supported");
        if (transposed && (e.kind != 1 || e.ndim != 2)) throw Error(SDMI_ERR_STATE, fn_name + ": '" + e.name + "' is not a Linear weight");
        int64_t want[4];
        for (int i = 0; i < e.ndim; ++i) want[i] = e.dims[i];
        if (transposed) std::swap(want[0], want[1]);   // torch's [out, in]
        if (slice >= 0) want[0] *= 3;                  // the fused [3C, C] / [3C]: this entry is rows [slice C, (slice + 1) C)
        bool ok = (int)t->shape.size() == e.ndim;
        for (int i = 0; ok && i < e.ndim; ++i) ok = t->shape[i] == want[i];
        // SD 2.x: the transformers' proj_in / proj_out are Linear layers, [C, C] in the file -- the bytes of the [C, C, 1, 1] convolution weight
        if (!ok && cfg_.variant == 1 && e.kind == 0 && e.ndim == 4 && e.dims[2] == 1 && e.dims[3] == 1 && t->shape.size() == 2)
            ok = t->shape[0] == e.dims[0] && t->shape[1] == e.dims[1];
        if (!ok)
            throw Error(SDMI_ERR_WEIGHTS, fn_name + ": '" + key + "' has shape " + shape_str(t->shape.data(), t->shape.size()) +
                                              ", the configured model expects " + shape_str(want, (size_t)e.ndim) + " ('" + e.name + "')");
        const size_t part = slice >= 0 ? t->nbytes / 3 : t->nbytes;
        jobs.push_back(Job{&e, t, dt, transposed ? 1 : (e.kind == 0 && padded_cin(e) != e.dims[1]) ? 2 : 0, t->data + (slice >= 0 ? (size_t)slice * part : 0), part});
    }
    if (jobs.empty()) throw Error(SDMI_ERR_WEIGHTS, std::string(fn_name + ": no tensor of ") + path + " matches the configured model");
    std::vector<float> schedule;
    if (alphas_entry) {
        const size_t n = entry_count(*alphas_entry);
        schedule.resize(n);
        if (alphas) {
            if (alphas->dtype != "F64" && unpack_dtype(alphas->dtype) < 0)
                throw Error(SDMI_ERR_UNSUPPORTED, fn_name + ": 'alphas_cumprod' has dtype " + alphas->dtype);
            if (alphas->shape.size() != 1 || (size_t)alphas->shape[0] != n)
                throw Error(SDMI_ERR_WEIGHTS, fn_name + ": 'alphas_cumprod' has shape " + shape_str(alphas->shape.data(), alphas->shape.size()) +
                                                  ", expected [" + std::to_string(n) + "]");
            for (size_t i = 0; i < n; ++i) schedule[i] = raw_to_f32(alphas->data, alphas->dtype, i);
        } else {
            default_alphas_cumprod(schedule.data(), (int)n);
        }
    }

    // The raw bytes go through the ring, so its limit applies to the file's bytes alone, as for every other loader.  The fp32 result of a conv / Linear tensor
    // goes to ONE device buffer of this call, sized for the largest of them (118 MB for SD v1.4's 2560 -> 1280 3x3 convolutions) and shared by all: the stream
    // orders tensor k's packing in front of tensor k + 1's conversion.  It is freed with the stager, so a load leaves nothing resident behind.
    size_t conv_bytes = 0;
    for (const Job& j : jobs)
        if (j.e->kind <= 1) conv_bytes = std::max(conv_bytes, stage_elems(*j.e) * sizeof(float));
    struct DevTemp {
        void* p = nullptr;
        ~DevTemp() { if (p) (void)hipFree(p); }
    } conv_stage;
    if (conv_bytes) SDMI_HIP(hipMalloc(&conv_stage.p, conv_bytes));
    struct Drain {   // the temporary outlives everything enqueued on it, also on the way out of an error
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{stream_};
    for (const Job& j : jobs) {
        WeightEntry& e = *j.e;
        ensure_arena(e.group);
        size_t off; int half;
        char* pinned = stage_reserve(j.nbytes, &off, &half);
        std::memcpy(pinned, j.data, j.nbytes);   // any file alignment
        char* dev = stager_->dev[half] + off;
        SDMI_HIP(hipMemcpyAsync(dev, pinned, j.nbytes, hipMemcpyHostToDevice, stream_));
        float* out = e.kind <= 1 ? static_cast<float*>(conv_stage.p) : *e.dst;
        fold_touch(e);
        long long d0, d1;
        if (j.transform == 1) { d0 = e.dims[1]; d1 = e.dims[0]; }
        else if (j.transform == 2) { d0 = e.dims[0]; d1 = e.dims[2] * e.dims[3]; }
        else { d0 = (long long)entry_count(e); d1 = 1; }
        {
            ProfScope ps_o(this, PC_OTHER, 0, (double)j.nbytes + (double)(e.kind <= 1 ? stage_elems(e) : entry_count(e)) * 4);
            ps_o.set_tag("unpack %s t%d %lldx%lld", j.t->dtype.c_str(), j.transform, d0, d1);
            SDMI_LAUNCH_IN(ps_o, 0, launch_unpack_tensor(dev, j.dtype, j.transform, d0, d1, out, stream_, (int)e.dims[1]));
        }
        if (e.kind <= 1) {
            if (e.master) SDMI_HIP(hipMemcpyAsync(e.master, out, stage_elems(e) * sizeof(float), hipMemcpyDeviceToDevice, stream_));
            pack_entry(e, out);
        }
        e.set = true;
        if (e.group != 3) finalized_ = false;
    }
    if (alphas_entry) { alphas_loaded_ = schedule; refresh_schedule(); alphas_entry->set = true; }
    if (control && finalized_) rebuild_folds();   // a ControlNet loaded behind finalize_weights: its folds are built here (the UNet's: by finalize_weights)
    SDMI_HIP(hipStreamSynchronize(stream_));
    if (profiling_) prof_flush();
    stager_release();
}

bool Engine::control_ready() const {
    bool any = false;
    for (auto& e : entries_)
        if (e.group == 3) { any = true; if (!e.set) return false; }
    return any;
}

void Engine::finalize_weights() {
    int total[kGroups] = {0, 0, 0, 0}, set[kGroups] = {0, 0, 0, 0};
    const WeightEntry* missing[kGroups] = {nullptr, nullptr, nullptr, nullptr};
    for (auto& e : entries_) {
        ++total[e.group];
        if (e.set) ++set[e.group];
        else if (!missing[e.group]) missing[e.group] = &e;
    }
    if (missing[0]) throw Error(SDMI_ERR_WEIGHTS, "finalize_weights: tensor '" + missing[0]->name + "' was never set");
    static const char* const kGroupName[kGroups] = {"", "CLIP", "VAE encoder", "ControlNet"};
    for (int g = 1; g < kGroups; ++g)
        if (set[g] && missing[g])
            throw Error(SDMI_ERR_WEIGHTS, std::string("finalize_weights: ") + kGroupName[g] + " weights are partially set; missing '" + missing[g]->name + "'");
    rebuild_folds();                           // the one thing derived from more than one entry (see "LoRA adapters" below)
    SDMI_HIP(hipStreamSynchronize(stream_));   // every packing kernel has run
    stager_release();
    clip_ready_ = total[1] > 0 && set[1] == total[1];
    enc_ready_ = total[2] > 0 && set[2] == total[2];
    finalized_ = true;
}

// =============================================================================
// LoRA adapters (include/sdmi.h "LoRA adapters")
// =============================================================================
// A merge rewrites packed weights outside any sampling call: W0 (the fp32 master, option keep_masters) + the deltas of the adapters active on a tensor go
// through launch_lora_merge into a pool buffer, and pack_entry -- the loader's own routine -- packs that buffer.  finalized_ / clip_ready_ / enc_ready_ are
// not touched, the pinned ring (released by finalize_weights) is not used.  ONE kind of device tensor is derived from more than one entry: the folded weights of
// a fp32 engine's transformer blocks (SpatialW::fold_bt / fold_bias = proj_out x mlp_lin, built by rebuild_folds at the end of finalize_weights).  pack_entry and
// every other write of one of the three entries clears SpatialW::fold_fresh (fold_touch), a block whose fold is not fresh runs its two launches and never the stale
// product, and lora_set_scale re-derives the stale folds behind its re-packs, outside any sampling call -- so the packed weights, the folds, get_scale and
// effective_weight agree whenever a call can run.  Everything else is per entry (the packed q | k | v regions are three entries' slots side by side, each with its
// own planes / MXFP8 rows): re-packing the entry is all there is to re-derive.

// out = the product of two packed fp32 weights in fp64, rounded once (k_gemm.hip fold_matmul_f64_kernel)
void Engine::fold_weights(const float* proj_bt, const float* lin_bt, const float* lin_bias, int cout, int cmid, int k_main, float* wf, float* bf) {
    ProfScope ps(this, PC_OTHER, 2.0 * cout * (double)cmid * k_main, ((double)cout * cmid + (double)cmid * k_main + (double)cout * k_main) * 4.0);
    ps.set_tag("fold %d,%d,%d", cout, k_main, cmid);
    SDMI_HIP(launch_fold_matmul_f64(proj_bt, lin_bt, wf, cout, cmid, k_main, cmid, k_main, k_main, stream_));
    if (lin_bias) SDMI_HIP(launch_fold_matmul_f64(proj_bt, lin_bias, bf, cout, cmid, 1, cmid, 1, 1, stream_));
    else SDMI_HIP(hipMemsetAsync(bf, 0, (size_t)cout * sizeof(float), stream_));
}

void Engine::rebuild_folds() {
    if (bf16_) return;
    for (SpatialW* s : st_list_) {
        if (s->fold_fresh || s->fold_entries[0] < 0) continue;
        bool ready = true;
        for (int i : s->fold_entries) ready = ready && entries_[(size_t)i].set;
        const int C = s->c;
        if (!ready || C % 32 || !split_planes(s->proj_out.bt) || !split_planes(s->mlp_lin.bt)) continue;
        const size_t w_bytes = (size_t)C * 4 * C * sizeof(float);
        if (!s->fold_bt) {   // Wf | bf in one allocation, the planes of Wf in a second: a split region, like the packed q | k | v weights
            char* base = static_cast<char*>(persistent_alloc(w_bytes + (size_t)C * sizeof(float)));
            weight_allocs_.push_back(base);
            char* planes = static_cast<char*>(persistent_alloc(w_bytes / 2 * 3));
            weight_allocs_.push_back(planes);
            split_regions_.push_back(SplitRegion{base, w_bytes, planes});
            s->fold_bt = reinterpret_cast<float*>(base);
            s->fold_bias = reinterpret_cast<float*>(base + w_bytes);
        }
        fold_weights(s->proj_out.bt, s->mlp_lin.bt, s->mlp_lin.bias, C, C, 4 * C, s->fold_bt, s->fold_bias);
        SDMI_HIP(launch_pack_split3(s->fold_bt, const_cast<void*>(split_planes(s->fold_bt)), C, 4 * C, stream_, b3_grouped(C)));
        s->fold_fresh = true;
    }
    // the phase weights of the up-convolutions (ConvW::up3): derived from ONE entry each, but not by pack_entry -- they live here so that one rule covers both kinds of
    // derived tensor (stale after any write of the entry, re-derived at finalize_weights and behind lora_set_scale, never run stale)
    for (ConvW* w : up_list_) {
        if (w->up_fresh || w->up_entry < 0 || !entries_[(size_t)w->up_entry].set || !opt_ups_phase_ || !up_fold_supported(w->cin, w->cout) || !split_planes(w->bt)) continue;
        if (!w->up3) {
            w->up3 = persistent_alloc((size_t)w->cout * w->cin * 96);
            weight_allocs_.push_back(w->up3);
        }
        build_up_fold(w->bt, w->up3, w->cout, w->cin);
        w->up_fresh = true;
    }
}

// what the plane kernel's phase mode reads: fp32 weights with planes, whole 32-channel slices, 32-bit piece offsets within a phase image
bool Engine::up_fold_supported(int cin, int cout) const {
    return !bf16_ && cin % 32 == 0 && cout >= 32 && (unsigned long long)cout * (unsigned long long)(cin / 8) * 192ull < 0xFFFFFF00ull;
}

void Engine::build_up_fold(const float* bt, void* up3, int cout, int cin) {
    // the fp32 image of a phase [cout][4 cin] is needed only until its planes exist: one pool buffer, reused by the four phases (stream order)
    Buf img(this, (size_t)4 * cout * cin * sizeof(float));
    ProfScope ps(this, PC_OTHER, 0, ((double)9 + 16 + 16 + 24) * cout * cin * 4.0);
    ps.set_tag("fold ups_phase %d,%d", cout, cin);
    for (int ph = 0; ph < 4; ++ph) {
        SDMI_HIP(launch_fold_ups_phase_f64(bt, img.f(), cout, cin, ph, 1, stream_));
        // each image is a weight of cout rows in the layout b3_grouped(cout) names -- the rule the launch reads the layout by
        SDMI_HIP(launch_pack_split3(img.f(), static_cast<char*>(up3) + (size_t)ph * cout * cin * 24, cout, 4 * cin, stream_, b3_grouped(cout)));
    }
}

Engine::TempUpFold::TempUpFold(Engine* e_, ConvW& w, int stride, int ups) : e(e_) {
    if (!e->opt_ups_phase_ || w.dt || w.k != 3 || stride != 1 || ups != 1 || !e->up_fold_supported(w.cin, w.cout) || !e->split_planes(w.bt)) return;
    up3 = e->pool_.alloc((size_t)w.cout * w.cin * 96);
    try { e->build_up_fold(w.bt, up3, w.cout, w.cin); } catch (...) { e->pool_.free(up3); up3 = nullptr; throw; }
    w.up3 = up3; w.up_fresh = true;
}
Engine::TempUpFold::~TempUpFold() { if (up3) e->pool_.free(up3); }
bool Engine::lora_owned(const sdmi_lora* a) const { return a && std::find(loras_.begin(), loras_.end(), a) != loras_.end(); }

bool Engine::lora_active_on(int entry) const {
    for (const sdmi_lora* a : loras_) {
        if (a->scale == 0) continue;
        for (const LoraTarget& t : a->targets)
            if (t.entry == entry) return true;
    }
    return false;
}

// a bulk load replaces every master: refused as a whole, before the first tensor is staged, while any adapter is merged in
void Engine::lora_refuse_bulk_load(const char* what) const {
    for (const sdmi_lora* a : loras_)
        if (a->scale != 0 && !a->targets.empty())
            throw Error(SDMI_ERR_STATE, std::string(what) + ": a LoRA adapter with a non-zero scale is attached: set its scale to 0 first");
}

sdmi_lora* Engine::lora_create() {
    if (!finalized_) throw Error(SDMI_ERR_STATE, "lora_create: weights not finalized");
    if (!opt_keep_masters_) throw Error(SDMI_ERR_STATE, "lora_create: the context keeps no fp32 master weights (option keep_masters=1, set before the weights are loaded)");
    sdmi_lora* a = new sdmi_lora{};
    a->engine = this;
    loras_.push_back(a);
    return a;
}

void Engine::lora_add(sdmi_lora* a, const char* target, const float* down, const float* up, int rank, float alpha) {
    if (!lora_owned(a)) throw Error(SDMI_ERR_INVALID, "lora_add: not an adapter of this context");
    if (!target || !down || !up) throw Error(SDMI_ERR_INVALID, "lora_add: null argument");
    if (a->scale != 0) throw Error(SDMI_ERR_STATE, "lora_add: targets are added while the adapter's scale is 0");
    auto it = entry_index_.find(target);
    if (it == entry_index_.end()) throw Error(SDMI_ERR_INVALID, std::string("lora_add: unknown tensor '") + target + "'");
    const WeightEntry& e = entries_[it->second];
    if (e.kind > 1) throw Error(SDMI_ERR_INVALID, std::string("lora_add: '") + target + "' is not a conv or Linear weight");
    if (e.kind == 0 && padded_cin(e) != e.dims[1])
        throw Error(SDMI_ERR_UNSUPPORTED, std::string("lora_add: '") + target + "' is the " + std::to_string(e.dims[1]) + "-channel conv_in, packed in a padded form");
    if (rank < 1 || rank > 256) throw Error(SDMI_ERR_INVALID, "lora_add: rank must be 1 .. 256");
    if (!std::isfinite(alpha)) throw Error(SDMI_ERR_INVALID, "lora_add: alpha is not finite");
    for (const LoraTarget& t : a->targets)
        if (t.entry == it->second) throw Error(SDMI_ERR_INVALID, std::string("lora_add: the adapter already has '") + target + "'");
    if (!e.master || !e.set) throw Error(SDMI_ERR_STATE, std::string("lora_add: '") + target + "' is not loaded");
    // Linear [in, out]: down [rank][in], up [out][rank]; conv [cout][cin][k][k]: down [rank][cin k k], up [cout][rank]
    const size_t n_in = e.kind == 0 ? (size_t)(e.dims[1] * e.dims[2] * e.dims[3]) : (size_t)e.dims[0];
    const size_t n_out = e.kind == 0 ? (size_t)e.dims[0] : (size_t)e.dims[1];
    SDMI_HIP(hipSetDevice(cfg_.device));
    // the copies below run on the null stream, which nothing orders behind the engine's: a fill of this buffer is complete before they start
    float* dev = static_cast<float*>(persistent_alloc((size_t)rank * (n_in + n_out) * sizeof(float), /*weight_buffer=*/false));
    hipError_t err = hipMemcpy(dev, down, (size_t)rank * n_in * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dev + (size_t)rank * n_in, up, (size_t)rank * n_out * sizeof(float), hipMemcpyHostToDevice);
    if (err != hipSuccess) { (void)hipFree(dev); SDMI_HIP(err); }
    a->allocs.push_back(dev);
    a->targets.push_back(LoraTarget{it->second, rank, (double)alpha, dev, dev + (size_t)rank * n_in});
}

sdmi_lora* Engine::lora_load_safetensors(const char* path, int which, int flags, int* n_skipped) {
    if (!path) throw Error(SDMI_ERR_INVALID, "lora_load_safetensors: null path");
    if (!finalized_) throw Error(SDMI_ERR_STATE, "lora_load_safetensors: weights not finalized");
    if (!opt_keep_masters_) throw Error(SDMI_ERR_STATE, "lora_load_safetensors: the context keeps no fp32 master weights (option keep_masters=1, set before the weights are loaded)");
    SDMI_HIP(hipSetDevice(cfg_.device));   // the allocations and copies below go to this context's device, whatever the calling thread used last
    SafetensorsFile f(path);
    std::vector<LoraEntryDesc> descs(entries_.size());
    for (size_t i = 0; i < entries_.size(); ++i) {
        const WeightEntry& e = entries_[i];
        descs[i].name = e.name; descs[i].kind = e.kind;
        for (int k = 0; k < 4; ++k) descs[i].dims[k] = k < e.ndim ? e.dims[k] : 1;
        descs[i].padded = e.kind == 0 && padded_cin(e) != e.dims[1];
    }
    LoraFilePlan plan = lora_plan_file(f.tensors(), descs, which, flags);
    // a weight group that was never loaded (a context without the text encoder's weights) is no target either
    std::vector<LoraFileTarget> targets;
    for (const LoraFileTarget& t : plan.targets) {
        const WeightEntry& e = entries_[t.entry];
        if (e.master && e.set) { targets.push_back(t); continue; }
        if (!(flags & kLoraSkipUnknown)) throw Error(SDMI_ERR_STATE, std::string("lora_load_safetensors: '") + e.name + "' (module '" + t.module + "') is not loaded");
        plan.skipped.push_back(t.module);
    }
    if (n_skipped) *n_skipped = (int)plan.skipped.size();
    // nothing below depends on the file's contents any more: only an allocation or a copy can fail, and then the adapter goes as a whole
    sdmi_lora* a = lora_create();
    try {
        for (const LoraFileTarget& t : targets) {
            const int nf = t.kind == 1 ? 4 : 2;
            size_t off[4], bytes = 0;   // each factor's raw bytes at a 16-byte aligned offset of one allocation
            for (int i = 0; i < nf; ++i) { off[i] = bytes; bytes += (t.f[i]->nbytes + 15) / 16 * 16; }
            char* dev = static_cast<char*>(persistent_alloc(bytes, /*weight_buffer=*/false));
            a->allocs.push_back(dev);
            a->factor_bytes += bytes;
            for (int i = 0; i < nf; ++i) SDMI_HIP(hipMemcpy(dev + off[i], t.f[i]->data, t.f[i]->nbytes, hipMemcpyHostToDevice));
            LoraTarget lt{t.entry, t.rank, t.alpha, dev + off[0], dev + off[1], t.dtype, t.kind};
            if (t.kind == 1) { lt.down2 = dev + off[2]; lt.up2 = dev + off[3]; }
            a->targets.push_back(lt);
        }
    } catch (...) {
        try { lora_destroy(a); } catch (...) {}
        throw;
    }
    return a;
}

void Engine::lora_compose(int entry, float* dst) {
    const WeightEntry& e = entries_[entry];
    const size_t n = stage_elems(e);
    LoraMerge m{};
    m.R = (int)e.dims[0];   // conv: cout rows of cin k k; Linear: in rows of out
    m.Cc = (int)(n / (size_t)m.R);
    m.W0 = e.master; m.W = dst;
    bool any = false;
    auto flush = [&] {
        {
            ProfScope ps(this, PC_OTHER, 0, 2.0 * (double)n * sizeof(float));   // the master read + the result written; the factors are a few per cent of that
            ps.set_tag("lora_merge %s%s %dx%d terms %d", m.t[0].dtype == 0 ? "F32" : m.t[0].dtype == 1 ? "F16" : "BF16", m.t[0].kind ? " loha" : "", m.R, m.Cc, m.n_terms);
            SDMI_HIP(launch_lora_merge(m, stream_));
        }
        m.W0 = dst;   // more than kLoraMaxTerms active adapters on one tensor: the next launch continues the sum in place
        m.n_terms = 0;
        any = true;
    };
    for (const sdmi_lora* a : loras_)
        for (const LoraTarget& t : a->targets) {
            if (t.entry != entry) continue;
            const float coef = (float)(a->scale * t.alpha / (double)t.rank);
            if (coef == 0.f) continue;
            // a launch takes terms of one factor dtype and one kind: a change continues the sum in place, like a ninth term
            if (m.n_terms && (m.t[0].dtype != t.dtype || m.t[0].kind != t.kind)) flush();
            LoraTerm& lt = m.t[m.n_terms++];
            lt = LoraTerm{};
            lt.rank = t.rank; lt.coef = coef; lt.dtype = t.dtype; lt.kind = t.kind;
            if (e.kind == 0) {   // rows = cout: P = up [cout][rank], Q = down [rank][Cc]
                lt.P = t.up; lt.p_rs = t.rank; lt.p_js = 1;
                lt.Q = t.down; lt.q_js = m.Cc; lt.q_cs = 1;
            } else {             // rows = in: P(i, j) = down[j][i], Q(j, o) = up[o][j]
                lt.P = t.down; lt.p_rs = 1; lt.p_js = m.R;
                lt.Q = t.up; lt.q_js = 1; lt.q_cs = t.rank;
            }
            if (t.kind == 1) {   // LoHa: the second pair, stored the same way
                lt.P2 = e.kind == 0 ? t.up2 : t.down2; lt.Q2 = e.kind == 0 ? t.down2 : t.up2;
                lt.p2_rs = lt.p_rs; lt.p2_js = lt.p_js; lt.q2_js = lt.q_js; lt.q2_cs = lt.q_cs;
            }
            if (m.n_terms == kLoraMaxTerms) flush();
        }
    if (m.n_terms) flush();
    // no active adapter: W0 itself -- not a merge with zero coefficients, which would turn -0.0 into +0.0
    if (!any) SDMI_HIP(hipMemcpyAsync(dst, e.master, n * sizeof(float), hipMemcpyDeviceToDevice, stream_));
}

void Engine::lora_repack(int entry) {
    WeightEntry& e = entries_[entry];
    Buf stage(this, stage_elems(e) * sizeof(float));
    lora_compose(entry, stage.f());
    pack_entry(e, stage.f());
}

void Engine::lora_set_scale(sdmi_lora* a, double scale) {
    if (!lora_owned(a)) throw Error(SDMI_ERR_INVALID, "lora_set_scale: not an adapter of this context");
    if (!std::isfinite(scale)) throw Error(SDMI_ERR_INVALID, "lora_set_scale: scale is not finite");
    if (scale == a->scale) return;
    SDMI_HIP(hipSetDevice(cfg_.device));
    const double old = a->scale;
    a->scale = scale;
    size_t done = 0;
    try {
        for (; done < a->targets.size(); ++done) lora_repack(a->targets[done].entry);
        rebuild_folds();   // the folds the re-packs left stale
        SDMI_HIP(hipStreamSynchronize(stream_));
    } catch (...) {
        // back to the old scale: the targets already re-packed (and the one that failed) are re-packed at it, so that the packed weights, get_scale and
        // effective_weight agree again.  Best effort: after a HIP error the context is usually lost anyway, and the first error is the one reported.
        a->scale = old;
        for (size_t i = 0; i <= done && i < a->targets.size(); ++i) {
            try { lora_repack(a->targets[i].entry); } catch (...) {}
        }
        try { rebuild_folds(); } catch (...) {}   // (a fold that cannot be rebuilt stays stale: its block runs the two launches)
        (void)hipStreamSynchronize(stream_);
        throw;
    }
}

void Engine::lora_destroy(sdmi_lora* a) {
    if (!lora_owned(a)) throw Error(SDMI_ERR_INVALID, "lora_destroy: not an adapter of this context");
    lora_set_scale(a, 0.0);
    SDMI_HIP(hipSetDevice(cfg_.device));
    for (void* p : a->allocs) (void)hipFree(p);
    loras_.erase(std::find(loras_.begin(), loras_.end(), a));
    delete a;
}

void Engine::effective_weight(const char* name, float* out, size_t n) {
    if (!name || !out) throw Error(SDMI_ERR_INVALID, "effective_weight: null argument");
    auto it = entry_index_.find(name);
    if (it == entry_index_.end()) throw Error(SDMI_ERR_INVALID, std::string("effective_weight: unknown tensor '") + name + "'");
    const WeightEntry& e = entries_[it->second];
    if (e.kind > 1) throw Error(SDMI_ERR_INVALID, std::string("effective_weight: '") + name + "' is not a conv or Linear weight");
    if (n != entry_count(e)) throw Error(SDMI_ERR_INVALID, std::string("effective_weight: '") + name + "' has " + std::to_string(entry_count(e)) + " elements");
    if (!opt_keep_masters_) throw Error(SDMI_ERR_STATE, "effective_weight: the context keeps no fp32 master weights (option keep_masters=1)");
    if (!e.master || !e.set) throw Error(SDMI_ERR_STATE, std::string("effective_weight: '") + name + "' is not loaded");
    SDMI_HIP(hipSetDevice(cfg_.device));
    const size_t ns = stage_elems(e);
    Buf stage(this, ns * sizeof(float));
    lora_compose(it->second, stage.f());
    if (ns == n) {
        SDMI_HIP(hipMemcpyAsync(out, stage.p, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
        SDMI_HIP(hipStreamSynchronize(stream_));
    } else {   // a padded conv_in: drop the zero input channels
        std::vector<float> padded(ns);
        SDMI_HIP(hipMemcpyAsync(padded.data(), stage.p, ns * sizeof(float), hipMemcpyDeviceToHost, stream_));
        SDMI_HIP(hipStreamSynchronize(stream_));
        const size_t T = (size_t)(e.dims[2] * e.dims[3]), cin = (size_t)e.dims[1], pc = (size_t)padded_cin(e);
        for (size_t o = 0; o < (size_t)e.dims[0]; ++o) std::memcpy(out + o * cin * T, padded.data() + o * pc * T, cin * T * sizeof(float));
    }
}

// npy-dump reader: src/model/load.rs:17-28 -- a 1-D float32 .npy whose first D
// values are the shape and whose remaining values are the row-major data.
// Returns the number of floats in the file; `sink(n)` supplies the destination for them.
template <class Sink>
static size_t read_npy_f32(const std::string& path, Sink&& sink) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Error(SDMI_ERR_IO, "cannot open " + path);
    char magic[8];
    f.read(magic, 8);
    if (!f || std::memcmp(magic, "\x93NUMPY", 6) != 0) throw Error(SDMI_ERR_IO, "not an npy file: " + path);
    uint32_t hlen = 0;
    if (magic[6] == 1) { uint16_t h16; f.read((char*)&h16, 2); hlen = h16; }
    else { f.read((char*)&hlen, 4); }
    std::string header(hlen, ' ');
    f.read(&header[0], hlen);
    if (header.find("'<f4'") == std::string::npos && header.find("\"<f4\"") == std::string::npos)
        throw Error(SDMI_ERR_IO, "npy dtype is not <f4: " + path);
    if (header.find("'fortran_order': True") != std::string::npos) throw Error(SDMI_ERR_IO, "fortran-order npy: " + path);
    const std::streampos start = f.tellg();
    f.seekg(0, std::ios::end);
    const size_t n = (size_t)(f.tellg() - start) / sizeof(float);
    f.seekg(start);
    float* dst = sink(n);
    f.read((char*)dst, (std::streamsize)(n * sizeof(float)));
    if (!f) throw Error(SDMI_ERR_IO, "short read: " + path);
    return n;
}

void Engine::load_weights_dir(const char* dir) {
    if (!dir) throw Error(SDMI_ERR_INVALID, "load_weights_dir: null path");
    SDMI_HIP(hipSetDevice(cfg_.device));
    lora_refuse_bulk_load("load_weights_dir");
    // the CLIP subtree is read when it exists (load_stable_diffusion always has it, stablediffusion/load.rs:24)
    const bool have_clip = std::ifstream(std::string(dir) + "/clip/token_embedding/weight.npy").good();
    const bool have_enc = std::ifstream(std::string(dir) + "/autoencoder/encoder/conv_in/weight.npy").good();
    const bool have_ctl = std::ifstream(std::string(dir) + "/controlnet/lin1_time_embed/weight.npy").good();
    for (auto& m : meta_) {   // optional per-module metadata files
        const std::string path = std::string(dir) + "/" + m.name + ".npy";
        if (!std::ifstream(path).good()) continue;
        std::vector<float> raw;
        read_npy_f32(path, [&](size_t n) { raw.resize(n); return raw.data(); });
        // save_scalar writes [1.0, s]; save_tensor of a 2-vector writes [2.0, a, b] (python/save.py:6-15)
        if (raw.size() != (size_t)m.n + 1 || raw[0] != (float)m.n) throw Error(SDMI_ERR_WEIGHTS, "malformed metadata file " + path);
        set_meta(m.name, raw.data() + 1, (size_t)m.n);
    }
    for (auto& e : entries_) {
        if ((e.group == 1 && !have_clip) || (e.group == 2 && !have_enc) || (e.group == 3 && !have_ctl)) continue;
        const std::string path = std::string(dir) + "/" + e.name + ".npy";
        const size_t count = entry_count(e);
        if (e.kind == 0 && padded_cin(e) != e.dims[1]) {   // rare (a padded conv_in): through the padding path
            std::vector<float> raw;
            read_npy_f32(path, [&](size_t n) { raw.resize(n); return raw.data(); });
            if (raw.size() != count + (size_t)e.ndim) throw Error(SDMI_ERR_WEIGHTS, "shape prefix does not match payload in " + path);
            for (int i = 0; i < e.ndim; ++i)
                if ((int64_t)raw[i] != e.dims[i]) throw Error(SDMI_ERR_WEIGHTS, "unexpected shape in " + path);
            upload_weight(e, raw.data() + e.ndim);
            continue;
        }
        // the file's floats land in the pinned ring directly: [dims.., values..]; the values start ndim floats in
        size_t off = 0; int half = 0;
        char* base = nullptr;
        const size_t n = read_npy_f32(path, [&](size_t nf) {
            if (nf != count + (size_t)e.ndim) throw Error(SDMI_ERR_WEIGHTS, "shape prefix does not match payload in " + path);
            base = stage_reserve((nf + 64) * sizeof(float), &off, &half);
            // keep the VALUES 256-byte aligned for the H2D copy: the prefix sits right before them
            return reinterpret_cast<float*>(base + 256) - e.ndim;
        });
        (void)n;
        const float* pre = reinterpret_cast<const float*>(base + 256) - e.ndim;
        for (int i = 0; i < e.ndim; ++i)
            if ((int64_t)pre[i] != e.dims[i]) {
                std::ostringstream os;
                os << "unexpected shape in " << path << ": dim " << i << " is " << pre[i] << ", expected " << e.dims[i];
                throw Error(SDMI_ERR_WEIGHTS, os.str());
            }
        stage_commit(e, off + 256, half);
    }
    SDMI_HIP(hipStreamSynchronize(stream_));
    stager_release();
}

// =============================================================================
// primitive ops
// =============================================================================
Act Engine::new_act(int n, int h, int w, int c, int dt) {
    Act a; a.n = n; a.h = h; a.w = w; a.c = c; a.dt = dt < 0 ? edt() : dt;
    a.p = reinterpret_cast<float*>(pool_.alloc(a.bytes()));
    return a;
}
Act Engine::new_act3(int n, int h, int w, int c, int what) {
    if ((what & 2) && (c % 32 || bf16_)) throw Error(SDMI_ERR_STATE, "new_act3: planes need fp32 storage and c % 32 == 0");
    Act a; a.n = n; a.h = h; a.w = w; a.c = c; a.dt = 0;
    if (what & 1) a.p = reinterpret_cast<float*>(pool_.alloc(a.bytes()));
    if (what & 2) { a.p3 = pool_.alloc(a.bytes3()); a.ld3 = (c / 32) * 192; }
    return a;
}
void Engine::release(Act& a) {
    if (!a.view) {
        if (a.p) pool_.free(a.p);
        if (a.p3) pool_.free(a.p3);
    }
    a.p = nullptr; a.p3 = nullptr;
}

Act Engine::slice(const Act& parent, int c_off, int c) {
    if (c_off < 0 || c <= 0 || c_off + c > parent.c || parent.view) throw Error(SDMI_ERR_STATE, "slice: bad channel range");
    // every kernel that reads or writes a view takes its 16-byte forms from the strides alone (vec_ok, the GroupNorm / quantiser loads, the DMA gather): the cut keeps the base on 16 bytes
    if (((size_t)c_off * (parent.dt ? 2 : 4)) % 16) throw Error(SDMI_ERR_STATE, "slice: the cut must start on a 16-byte boundary");
    Act a = parent;
    a.p = parent.p ? adv(parent.p, c_off, parent.dt) : nullptr;
    if (parent.p3) {
        if (c_off % 32 || c % 32) throw Error(SDMI_ERR_STATE, "slice: plane tensors are cut at multiples of 32 channels");
        a.p3 = (char*)parent.p3 + (size_t)(c_off / 32) * 192;
    }
    a.c = c; a.ld = parent.stride(); a.view = true;
    return a;
}

void Engine::sync() { SDMI_HIP(hipStreamSynchronize(stream_)); }

void Engine::begin_call(bool dev_inputs) {
    SDMI_HIP(hipSetDevice(cfg_.device));
    n_kernels_ = 0; flops_ = 0;
    call_mark_ = pool_.serial();
    call_dev_ = dev_inputs;
    if (dev_inputs) {
        // the engine's stream is non-blocking: nothing orders it behind the stream that produced the caller's device
        // buffers unless we do
        if (has_user_stream_) {
            SDMI_HIP(hipEventRecord(ev_user_, user_stream_));
            SDMI_HIP(hipStreamWaitEvent(stream_, ev_user_, 0));
        } else {
            SDMI_HIP(hipDeviceSynchronize());
        }
    }
    SDMI_HIP(hipEventRecord(ev0_, stream_));
}
void Engine::end_call() {
    SDMI_HIP(hipEventRecord(ev1_, stream_));
    if (call_dev_ && has_user_stream_) SDMI_HIP(hipStreamWaitEvent(user_stream_, ev1_, 0));  // later work on the caller's stream sees the outputs
    SDMI_HIP(hipEventSynchronize(ev1_));
    float ms = 0;
    SDMI_HIP(hipEventElapsedTime(&ms, ev0_, ev1_));
    last_ms = ms; last_kernels = n_kernels_; last_flops = flops_;
}
void Engine::abort_call() noexcept {
    // a throw inside a forward pass leaves raw activations and the per-call UNet tables allocated: wait for what was
    // enqueued, then hand every block this call took back to the pool
    (void)hipStreamSynchronize(stream_);
    try {
        us_ = UNetState{};
        ip_live_ = false;
        pool_.free_since(call_mark_);
    } catch (...) {}
}

void Engine::set_option(const std::string& key, const std::string& value) {
    if (key == "gemm_tile") gopt_.force_tile = (value == "auto") ? -1 : std::stoi(value);
    else if (key == "splitk") gopt_.force_splits = std::stoi(value);
    else if (key == "splitk_aux") opt_splitk_aux_ = std::stoi(value);
    else if (key == "skip_slices") opt_skip_slices_ = std::stoi(value);
    else if (key == "proj_out_fold") opt_proj_out_fold_ = std::stoi(value);
    else if (key == "roctx") roctx_enable(std::stoi(value) != 0);
    else if (key == "fp8_convs") opt_fp8_convs_ = std::stoi(value);
    else if (key == "fp8_min_rows") opt_fp8_min_rows_ = std::stoi(value);
    else if (key == "fp8_linear") opt_fp8_linear_ = std::stoi(value);
    else if (key == "fp8_ops") opt_fp8_ops_ = std::stoi(value);
    else if (key == "op_resid") opt_op_resid_ = std::stoi(value);
    else if (key == "op_misalign") opt_op_misalign_ = std::stoi(value);
    else if (key == "op_f32") opt_op_f32_ = std::stoi(value);
    else if (key == "pool_fill") {   // tests: -1 = off, 0 .. 255 = the byte every pool block and persistent allocation made from now on is filled with (DevPool::set_fill)
        const int b = std::stoi(value);
        if (b < -1 || b > 255) throw Error(SDMI_ERR_INVALID, "pool_fill: -1 (off) or a byte 0 .. 255");
        pool_.set_fill(b);
        // the constructor allocated the fused q | k | v weight buffers before any option could be set: while no weight is loaded they hold nothing, fill them as well
        if (b >= 0 && std::none_of(entries_.begin(), entries_.end(), [](const WeightEntry& w) { return w.set; })) {
            SDMI_HIP(hipSetDevice(cfg_.device));
            for (const PersistentBlock& pb : persistent_blocks_) {
                SDMI_HIP(hipMemsetAsync(pb.p, b, pb.bytes, stream_));
                pool_.note_fill(pb.bytes);
            }
        }
    }
    else if (key == "dump_pool_fills") {   // "blocks bytes" filled since this option was last written (or the context was created)
        std::ofstream f(value);
        if (!f) throw Error(SDMI_ERR_IO, "dump_pool_fills: cannot write " + value);
        unsigned long long blocks = 0, bytes = 0;
        pool_.take_fill_counts(&blocks, &bytes);
        f << blocks << " " << bytes << "\n";
    }
    else if (key == "cfg_share") opt_cfg_share_ = std::stoi(value);
    else if (key == "attn_kv_splits") aopt_.attn_kv_splits = std::stoi(value);
    else if (key == "attn_kv_prefer8") aopt_.attn_kv_prefer8 = std::stoi(value);
    else if (key == "b3_grouped") {
        if (!entries_.empty() && std::any_of(entries_.begin(), entries_.end(), [](const WeightEntry& w) { return w.set; }))
            throw Error(SDMI_ERR_STATE, "b3_grouped selects the layout the weight planes are packed in: set it before the first weight is loaded");
        opt_b3_grouped_ = std::stoi(value);
    }
    else if (key == "keep_masters") {
        if (std::any_of(entries_.begin(), entries_.end(), [](const WeightEntry& w) { return w.set; }) || arena_done_[0] || arena_done_[1] || arena_done_[2] || arena_done_[3])
            throw Error(SDMI_ERR_STATE, "keep_masters decides what the weight arenas hold: set it before the first weight is loaded");
        opt_keep_masters_ = std::stoi(value) != 0;
    }
    else if (key == "attn_pack_tail") aopt_.attn_pack_tail = (value == "default") ? AttnPlanOpts().attn_pack_tail : std::stoi(value);
    else if (key == "gn32_min_wgs") opt_gn32_min_wgs_ = (opt_gn32_min_wgs_ & ~0xFFFF) | (std::stoi(value) & 0xFFFF);
    else if (key == "gn32_stats_min_wgs") opt_gn32_min_wgs_ = (opt_gn32_min_wgs_ & 0xFFFF) | ((std::stoi(value) + 1) << 16);   // the statistics pass cut differently from the apply pass (-1: the same)
    else if (key == "gn_target_wgs") gn_tune_.target_wgs = std::stoi(value);
    else if (key == "gn_max_threads") gn_tune_.max_threads = std::stoi(value);
    else if (key == "gn_unroll") gn_tune_.unroll = std::stoi(value);
    else if (key == "fp8_tile") opt_fp8_tile_ = (value == "auto") ? -1 : std::stoi(value);
    else if (key == "resid_acc") opt_resid_acc_ = std::stoi(value);
    else if (key == "attn_bf16") aopt_.attn_bf16 = std::stoi(value);
    else if (key == "attn_bf16_variant") aopt_.attn_bf16_variant = (value == "default") ? AttnPlanOpts().attn_bf16_variant : std::stoi(value, nullptr, 0);
    else if (key == "attn_split") aopt_.attn_split = std::stoi(value);
    else if (key == "attn_d64") {   // d_head = 64 on k_attn_split.hip / k_attn_bf16.hip: 0 never, 1 wherever they take the call, 2 where measured faster; "default": 2 on an SD 2.x context
        const int v = (value == "default") ? (cfg_.variant == 1 ? 2 : 0) : std::stoi(value);
        if (v < 0 || v > 2) throw Error(SDMI_ERR_INVALID, "attn_d64: 0 (never), 1 (wherever supported) or 2 (where measured faster)");
        if ((v != 0) != (aopt_.attn_d64 != 0) && !q64_entries_.empty()) {   // a bf16 UNet with 64-wide heads: the option decides whether its query weights are packed pre-scaled
            for (int i : q64_entries_)
                if (entries_[(size_t)i].set) throw Error(SDMI_ERR_STATE, "attn_d64 decides the scale the 64-wide heads' query weights are packed with: set it before they are loaded");
            for (int i : q64_entries_) entries_[(size_t)i].pre_scale = v ? attn_bf16_q_scale(64) : 1.f;
        }
        aopt_.attn_d64 = v;
    }
    else if (key == "gemm_bf16x") gopt_.gemm_bf16x = std::stoi(value);
    else if (key == "gemm_x32") gopt_.gemm_x32 = std::stoi(value);
    else if (key == "gemm_f32s") gopt_.gemm_f32s = std::stoi(value);
    else if (key == "bench_cold") opt_bench_cold_ = std::stoi(value);
    else if (key == "gemm_probe") opt_gemm_probe_ = std::stoi(value);
    else if (key == "conv3_reuse") gopt_.conv3_reuse = std::stoi(value);
    else if (key == "gemm_planes") gopt_.gemm_planes = (value == "default") ? GemmPlanOpts().gemm_planes : std::stoi(value);
    else if (key == "gemm3x_variant") opt_gemm3x_variant_ = (value == "default") ? kGemm3xVariantDefault : std::stoi(value);
    else if (key == "gemm_bf16x_variant") opt_gemm_bf16x_variant_ = (value == "default") ? kGemmBf16xVariantDefault : std::stoi(value);
    else if (key == "geglu_fuse") opt_geglu_fuse_ = std::stoi(value);
    else if (key == "ups_phase") {
        const int v = (value == "default") ? 2 : std::stoi(value);
        if (v < 0 || v > 2) throw Error(SDMI_ERR_INVALID, "ups_phase: 0 (never), 1 (wherever supported) or 2 (where the planner takes it)");
        opt_ups_phase_ = v;
        if (v && finalized_) {   // switched on behind finalize_weights: the phase weights that were never built
            SDMI_HIP(hipSetDevice(cfg_.device));
            rebuild_folds();
            SDMI_HIP(hipStreamSynchronize(stream_));
        }
    }
    else if (key == "record_shapes") { record_shapes_ = std::stoi(value) != 0; if (record_shapes_) { shape_counts_.clear(); choice_counts_.clear(); } }
    else if (key == "dump_shapes") {
        std::ofstream f(value);
        if (!f) throw Error(SDMI_ERR_IO, "dump_shapes: cannot write " + value);
        for (auto& kv : shape_counts_) f << kv.first << " " << kv.second << "\n";
    }
    else if (key == "dump_choices") {
        std::ofstream f(value);
        if (!f) throw Error(SDMI_ERR_IO, "dump_choices: cannot write " + value);
        for (auto& kv : choice_counts_) f << kv.first << " x" << kv.second << "\n";
    }
    else if (key == "profile") { prof_flush(); profiling_ = std::stoi(value) != 0; prof_tagging_ = std::stoi(value) >= 2; if (profiling_) prof_calibrate(); }
    else if (key == "dump_profile_tags") {   // profile=2: "ms launches flops bytes<TAB>tag" per line
        prof_flush();
        std::ofstream f(value);
        if (!f) throw Error(SDMI_ERR_IO, "dump_profile_tags: cannot write " + value);
        for (auto& kv : prof_tags_) f << kv.second.ms << " " << kv.second.launches << " " << kv.second.flops << " " << kv.second.bytes << "\t" << kv.first << "\n";
    }
    else if (key == "profile_reset") prof_reset();
    else if (key == "tune" || key == "tune_bf16") tuning_.set(value, key == "tune_bf16");   // "M,N,K=cfg,splits"
    else if (key == "tune_clear") tuning_.clear();
    else throw Error(SDMI_ERR_INVALID, "unknown option '" + key + "'");
}

// ConvGemm::resid_acc for a launch of a kernel that can take it (`eligible`: large-tile bf16 / MXFP8, no split-K): every 16-byte bias / time-embedding load and
// 8-byte residual load of gemm_acc_init_bf16 -- edge tiles included -- must be aligned, so besides the strides the base addresses are checked; a launch
// that fails a condition leaves its bit unset and adds that term in the epilogue
void Engine::set_resid_acc(ConvGemm& p, bool eligible, bool resid_ok) const {
    p.resid_acc = 0;
    if (!eligible || (p.N % 8) || (p.ldc % 8)) return;
    if ((opt_resid_acc_ & 1) && p.resid && resid_ok && (p.ldr % 4) == 0 && ((uintptr_t)p.resid & 7) == 0) p.resid_acc |= 1;
    if ((opt_resid_acc_ & 2) && (p.bias || p.rowvec) && (p.rowvec_stride % 4) == 0 && (((uintptr_t)p.bias | (uintptr_t)p.rowvec) & 15) == 0) p.resid_acc |= 2;
}

// option dump_choices (with record_shapes): which kernel / tile / split-K each (M, N, K) got
void Engine::record_choice(const ConvGemm& p, const char* kind, int cfg, const char* note) {
    if (!record_shapes_) return;
    char ck[128];
    std::snprintf(ck, sizeof ck, "%d,%d,%d k%d s%d u%d W%d%s cfg=%d splits=%d%s acc=%d", p.M, p.N, p.K, p.KH, p.stride, p.ups, p.Ws, kind, cfg, p.splits, note, p.resid_acc);
    ++choice_counts_[ck];
}

// The launch of a planned GEMM (p.splits set), profiled and counted: the kernel, and behind a split-K launch the reduce over its slabs.
// `what` / cfg name the launch in the profile tags; reduce_tag: 0 = the reduce carries none.
void Engine::run_gemm(ConvGemm& p, const GemmRun& r) {
    if (p.splits == 1) {
        p.slabs = nullptr; p.slab_stride = 0;
        ProfScope ps(this, r.pc, r.flops, r.bytes);
        ps.set_tag("%s %d,%d,%d k%d%s%s%s cfg=%d splits=1", r.what, p.M, p.N, p.K, p.KH, p.geglu ? " geglu" : "", p.resid ? " resid" : "", p.rowvec ? " rowvec" : "", r.cfg);
        SDMI_LAUNCH_IN(ps, r.flops, r.launch(p, r.index, stream_));
        return;
    }
    p.slab_stride = (long long)p.M * p.N;
    Buf slab(this, (size_t)p.splits * p.slab_stride * sizeof(float));
    p.slabs = slab.f();
    {
        ProfScope ps(this, r.pc, r.flops, r.bytes);
        ps.set_tag("%s %d,%d,%d k%d%s cfg=%d splits=%d", r.what, p.M, p.N, p.K, p.KH, p.geglu ? " geglu" : "", r.cfg, p.splits);
        SDMI_LAUNCH_IN(ps, r.flops, r.launch(p, r.index, stream_));
    }
    ProfScope ps(this, PC_SPLITK_REDUCE, 0, (double)(p.splits + 1) * p.slab_stride * 4.0);
    if (r.reduce_tag) ps.set_tag("reduce %d,%d,%d k%d cfg=%d splits=%d", p.M, p.N, p.K, p.KH, r.cfg, p.splits);
    SDMI_LAUNCH_IN(ps, 0, r.bf16_reduce ? launch_splitk_reduce_bf16(p, stream_) : launch_splitk_reduce(p, stream_));
}

// what the planner (gemm_plan.hpp) is told about a launch; p.kt_total, p.Bt3 and the shape are set
GemmPlanIn Engine::gemm_plan_in(const ConvGemm& p, int in_dt, int force_cfg, int force_splits) const {
    GemmPlanIn in{};
    in.M = p.M; in.N = p.N; in.K = p.K; in.kt_total = p.kt_total; in.bf16 = in_dt; in.geglu = p.geglu; in.out_mode = p.out_mode; in.force_cfg = force_cfg; in.force_splits = force_splits;
    in.KH = p.KH; in.KW = p.KW; in.stride = p.stride; in.pad = p.pad; in.ups = p.ups; in.Cin = p.Cin; in.Hs = p.Hs; in.Ws = p.Ws; in.Ho = p.Ho; in.Wo = p.Wo;
    in.zero_page = zero_page_ != nullptr;
    in.x32_ok = !in_dt && p.CS == 32 && p.Cin % 32 == 0 && p.out_mode == 0;   // what k_gemm2x.hip handles
    // k_gemm3x.hip: the same layers, when the weight has its bf16 planes (weights in the arenas; not e.g. the K / V operands of
    // the unfused VAE attention) and the 32-bit piece offsets reach
    in.s_ok = in.x32_ok && p.Bt3 && (unsigned long long)p.N * (p.geglu ? 2 : 1) * (unsigned long long)p.kt_total * 192ull < 0xFFFFFF00ull;
    // k_gemm3p.hip: the same layers with the activations as planes too -- written by their producer (p.A3) or, for a tensor that
    // arrives as fp32, by split3_rows_kernel right here
    in.p_ok = in.s_ok && (unsigned long long)p.NB * p.Hs * p.Ws * (unsigned long long)(p.A3 ? p.a3_ld : p.Cin * 6) < 0xFFFFFF00ull;
    // the activations arrive as planes (their producer wrote them): the GEMM runs on a plane tile -- from the plane table or the cost model
    in.from_planes = !in_dt && p.A3 != nullptr;
    return in;
}

// Which tile and how many K slices: plan_gemm (gemm_plan.cpp).  Here: the facts it plans from, the temporary buffers, the launch.
void Engine::launch_gemm(ConvGemm& p, int in_dt, int force_cfg, int force_splits) {
    const int kt_elems = in_dt ? 64 : 32;  // a k tile is 128 bytes of K per row in both storage types
    p.kt_total = (p.K + kt_elems - 1) / kt_elems;
    if (in_dt && (p.Cin % 64)) throw Error(SDMI_ERR_UNSUPPORTED, "bf16 GEMM: K slices must be multiples of 64");
    if (record_shapes_) {
        char sk[96];
        std::snprintf(sk, sizeof sk, "%d,%d,%d,%d,%d,%d,%d,%d", p.NB, p.Cin, p.Hs, p.Ws, p.N, p.KH, p.stride, p.ups);
        ++shape_counts_[sk];
    }
    p.Bt3 = in_dt ? nullptr : split_planes(p.Bt);
    p.b3_grouped = b3_grouped((long long)p.N * (p.geglu ? 2 : 1)) ? 1 : 0;   // the layout the planes of a weight with that many rows were packed in
    p.variant = in_dt ? opt_gemm_bf16x_variant_ : opt_gemm3x_variant_;
    p.zero_page = zero_page_;
    p.probe = probe_buf_;
    const GemmPlanIn in = gemm_plan_in(p, in_dt, force_cfg, force_splits);
    if (!in.from_planes && !p.A) throw Error(SDMI_ERR_STATE, "gemm: no activations");
    const GemmPlan g = plan_gemm(in, gopt_, tuning_);
    p.kt_per_split = g.kt_per_split; p.splits = g.splits;
    const bool w_planes = g.tile.family >= kFamS, a_planes = g.tile.family == kFamP;   // the operands the kernel reads as three bf16 planes
    const double flops = 2.0 * p.M * (double)p.N * p.K * (p.geglu ? 2.0 : 1.0);
    // raw buffer loads: the range check needs 32-bit extents
    const unsigned long long es = in_dt ? 2ull : 4ull;
    const unsigned long long a_ext = ((unsigned long long)p.NB * p.Hs * p.Ws - 1) * (unsigned long long)p.a_ld * es + (unsigned long long)p.Cin * es;
    const unsigned long long b_ext = ((unsigned long long)p.N * (p.geglu ? 2 : 1) - 1) * (unsigned long long)p.b_ld * es + (unsigned long long)p.K * es;
    if (a_ext >= 0xFFFFFFE0ull || b_ext >= 0xFFFFFFE0ull) throw Error(SDMI_ERR_UNSUPPORTED, "GEMM: operand larger than 4 GiB (the buffer-load range check needs 32-bit extents)");
    p.a_bytes = (unsigned)a_ext;
    p.b_bytes = (unsigned)b_ext;
    // the output as planes (p.C3): written by the epilogue of the split / plane kernels and by the split-K reduce kernel on their 16-byte
    // path; otherwise (old kernels, odd strides, GEGLU epilogue) converted from an fp32 result right behind the launch
    void* const c3_want = in_dt ? nullptr : p.C3;
    const int ldc3_want = p.ldc3;
    const bool vec_out = (p.N % 4 == 0) && (!p.C || p.ldc % 4 == 0) && (!p.resid || p.ldr % 4 == 0);
    const bool c3_native = c3_want && w_planes && vec_out && (!p.geglu || (p.geglu == 2 && a_planes));
    std::unique_ptr<Buf> c_tmp;
    if (!c3_native) {
        p.C3 = nullptr;
        if (c3_want && !p.C) {
            c_tmp.reset(new Buf(this, (size_t)p.M * p.N * sizeof(float)));
            p.C = c_tmp->f(); p.ldc = p.N;
        }
    }
    if (!p.C) p.ldc = p.N;
    std::unique_ptr<Buf> a3_tmp;
    if (a_planes && !p.A3) {   // the source is fp32: split it once for this launch (a producer that writes planes itself saves this pass)
        const long long rows = (long long)p.NB * p.Hs * p.Ws;
        p.a3_ld = (p.Cin / 32) * 192;
        a3_tmp.reset(new Buf(this, (size_t)rows * p.a3_ld));
        ProfScope ps(this, PC_SPLIT_ROWS, 0, (double)rows * p.Cin * 10.0);
        SDMI_LAUNCH_IN(ps, 0, launch_split3_rows(p.A, a3_tmp->p, rows, p.Cin, p.a_ld, p.a3_ld, stream_));
        p.A3 = a3_tmp->p;
    }
    // the large-tile bf16 kernels take the residual as the accumulators' initial value (k_gemm_bf16_epi.hpp gemm_acc_init_bf16) where their 8-byte loads apply
    // (option resid_acc: bit 0 = the residual, bit 1 = bias + time-embedding row; launches without split-K only -- the split-K combine adds them otherwise)
    set_resid_acc(p, in_dt && g.tile.family == kFamX && g.splits == 1, !p.geglu);
    record_choice(p, "", g.cfg, p.Bt3 || in_dt ? "" : " (no planes)");
    // ALGORITHMIC bytes of the launch in the formats the tensors are stored in: the source activations once, the weights once, the result once (bf16 2 B, fp32 4 B,
    // planes 6 B per element; split-K slabs and im2col / tile re-reads are not algorithmic) -- what the PMC byte counters of profiles/pmc_summary.json are held against
    const double a_es = in_dt ? 2.0 : (a_planes ? 6.0 : 4.0), w_es = in_dt ? 2.0 : (w_planes ? 6.0 : 4.0);
    const double c_es = in_dt ? (p.out_mode == 1 ? 4.0 : 2.0) : (p.out_mode == 2 ? 2.0 : ((p.C ? 4.0 : 0.0) + (c3_native ? 6.0 : 0.0)));
    const double gemm_bytes = (double)p.NB * p.Hs * p.Ws * p.Cin * a_es + (double)p.N * (p.geglu ? 2.0 : 1.0) * p.K * w_es + (double)p.M * p.N * c_es;
    // kernel by storage type and family (bf16: plan_gemm lets only the first two through)
    static const GemmLauncher kLaunchers[2][kNumGemmFamilies] = {{launch_conv_gemm2, launch_conv_gemm2x, launch_conv_gemm3x, launch_conv_gemm3p},
                                                                 {launch_conv_gemm_bf16, launch_conv_gemm_bf16_large, nullptr, nullptr}};
    // (k_gemm3x.hip / k_gemm3p.hip launches are timed as their own class)
    run_gemm(p, GemmRun{kLaunchers[in_dt ? 1 : 0][g.tile.family], g.tile.index, "gemm", g.cfg, w_planes ? PC_CONV_SPLIT : PC_CONV_GEMM, in_dt != 0, true, flops, gemm_bytes});
    if (c3_want && !c3_native) {
        ProfScope ps(this, PC_SPLIT_ROWS, 0, (double)p.M * p.N * 10.0);
        SDMI_LAUNCH_IN(ps, 0, launch_split3_rows(p.C, c3_want, p.M, p.N, p.ldc, ldc3_want, stream_));
    }
}

void Engine::conv(const ConvW& w, const Act& x, Act& y, int stride, int ups, const float* rowvec, int rowvec_stride,
                  const Act* resid, bool pad_br) {
    if (x.c != w.cin) throw Error(SDMI_ERR_INVALID, "conv: input channels mismatch");
    // pad_br: rows / columns past the bottom / right edge read as zero through the kernels' range check, so the
    // asymmetric padding is pad = 0 plus one more output row / column than a symmetric pad-0 conv has
    const int pad = pad_br ? 0 : (w.k == 3 ? 1 : 0);
    const int hin = x.h << ups, win = x.w << ups;
    const int extra = pad_br ? 1 : 0;
    const int ho = (hin + 2 * pad + extra - w.k) / stride + 1, wo = (win + 2 * pad + extra - w.k) / stride + 1;
    if (y.n != x.n || y.h != ho || y.w != wo || y.c != w.cout) throw Error(SDMI_ERR_INVALID, "conv: output shape mismatch");
    if (ups == 1 && stride == 1 && w.k == 3 && !pad_br && conv_ups_phase(w, x, y, rowvec, resid)) return;   // four folded 2x2 phase convolutions instead
    ConvGemm p{};
    // (an fp32 -> bf16 layer -- Cin < 32 at precision >= 1 -- adds its residual in fp32, in front of the rounding: k_gemm2.hip's epilogue)
    const int resid_dt = (!x.dt && y.dt) ? 0 : y.dt;
    if (resid && !x.dt && y.dt && (w.cout % 4 || y.stride() % 4 || resid->stride() % 4))   // (only that kernel's 16-byte epilogue rounds to bf16)
        throw Error(SDMI_ERR_STATE, "conv: a residual on an fp32 -> bf16 layer needs cout and the row strides to be multiples of 4");
    if (resid && (resid->rows() != y.rows() || resid->c != y.c || resid->dt != resid_dt)) throw Error(SDMI_ERR_STATE, "conv: residual shape / type mismatch");
    p.A = x.p; p.Bt = w.bt; p.C = y.p; p.bias = w.bias; p.rowvec = rowvec; p.resid = resid ? resid->p : nullptr;
    if (resid && !resid->p) throw Error(SDMI_ERR_STATE, "conv: the residual must exist as fp32");
    if (!x.dt && plane_gemm(w.cin, w.cout) && split_planes(w.bt)) { p.A3 = x.p3; p.a3_ld = x.ld3; }   // planes in, where the plane kernel takes the layer
    if (!x.p && !p.A3) throw Error(SDMI_ERR_STATE, "conv: the input exists only as planes, which this layer cannot read");
    p.C3 = y.p3; p.ldc3 = y.ld3;
    p.M = x.n * ho * wo; p.N = w.cout; p.K = w.cin * w.k * w.k;
    p.NB = x.n; p.Hs = x.h; p.Ws = x.w; p.Cin = w.cin; p.Ho = ho; p.Wo = wo;
    p.KH = w.k; p.KW = w.k; p.stride = stride; p.pad = pad; p.ups = ups;
    p.ldc = y.stride(); p.ldr = resid ? resid->stride() : y.stride(); p.a_ld = x.stride(); p.b_ld = p.K; p.rowvec_stride = rowvec_stride;
    p.CS = std::min(32, w.cin);
    if (!y.p && !y.p3) throw Error(SDMI_ERR_STATE, "conv: no output buffer");
    if (x.dt != w.dt) throw Error(SDMI_ERR_STATE, "conv: activation / weight storage types disagree");
    p.out_mode = x.dt ? (y.dt ? 0 : 1) : (y.dt ? 2 : 0);
    launch_gemm(p, x.dt);
}

// y = conv3x3(nearest_2x(x), w) + bias as ONE plane launch over the SOURCE grid: four 2x2 convolutions, one per output pixel phase, with the weights folded at load
// (ConvW::up3, rebuild_folds; kernels.hpp ConvGemm::phases).  Of the nine taps of an output pixel only four distinct source pixels are read, so the K = 9 cin launch
// multiplies duplicated activations in 5/9 of its matrix instructions; this one executes 2 . 4 . (M / 4) . N . 4 cin flops.  Returns false -- nothing launched, the
// caller runs the K = 9 cin launch -- when the option, the layer, the fold's freshness, the buffers or the planner (plan_ups_phase) do not allow it.  ups_phase = 1
// (tests) with a time-embedding row or a residual is an error: a phase launch carries the bias only, and a forced arm has no quiet other path.
bool Engine::conv_ups_phase(const ConvW& w, const Act& x, Act& y, const float* rowvec, const Act* resid) {
    if (!opt_ups_phase_ || bf16_ || x.dt || y.dt || w.dt || w.k != 3 || !w.up3 || !w.up_fresh || probe_buf_) return false;
    if (x.c != w.cin || !plane_gemm(w.cin, w.cout) || !up_fold_supported(w.cin, w.cout) || (!x.p3 && !x.p) || (!y.p && !y.p3)) return false;
    ConvGemm p{};
    p.A = x.p; p.Bt = w.bt; p.bias = w.bias;
    p.Bt3 = split_planes(w.bt);
    if (!p.Bt3) return false;
    p.A3 = x.p3; p.a3_ld = x.ld3;
    p.C = y.p; p.C3 = y.p3; p.ldc3 = y.ld3;
    p.M = (int)y.rows(); p.N = w.cout; p.K = w.cin * 9;            // the layer, as the planner and the records see it
    p.NB = x.n; p.Hs = x.h; p.Ws = x.w; p.Cin = w.cin; p.Ho = 2 * x.h; p.Wo = 2 * x.w;
    p.KH = 3; p.KW = 3; p.stride = 1; p.pad = 1; p.ups = 1;
    p.ldc = y.p ? y.stride() : p.N; p.ldr = p.ldc; p.a_ld = x.stride(); p.b_ld = p.K; p.CS = 32;
    p.kt_total = p.K / 32;
    p.variant = opt_gemm3x_variant_;
    p.zero_page = zero_page_;
    const GemmPlanIn in = gemm_plan_in(p, 0, -1, 0);
    const UpsPhasePlan g = plan_ups_phase(in, w.up_fresh, opt_ups_phase_, gopt_, tuning_);
    if (!g.take) return false;
    // the native plane output of launch_gemm: 16-byte stores
    if ((p.N % 4) || (p.C && p.ldc % 4)) { if (p.C3 || opt_ups_phase_ != 1) return false; }
    if (rowvec || resid) {
        if (opt_ups_phase_ != 1) return false;
        throw Error(SDMI_ERR_INVALID, "conv: ups_phase=1 with a time-embedding row or a residual: a phase launch carries the bias only");
    }
    if (record_shapes_) {
        char sk[96];
        std::snprintf(sk, sizeof sk, "%d,%d,%d,%d,%d,%d,%d,%d", p.NB, p.Cin, p.Hs, p.Ws, p.N, 3, 1, 1);
        ++shape_counts_[sk];
        p.splits = g.splits;
        record_choice(p, " phase", g.cfg, "");
    }
    std::unique_ptr<Buf> a3_tmp;
    if (!p.A3) {   // ups_phase = 1 on an fp32 source: split once for this launch, as launch_gemm does for a plane tile
        const long long rows = (long long)p.NB * p.Hs * p.Ws;
        p.a3_ld = (p.Cin / 32) * 192;
        a3_tmp.reset(new Buf(this, (size_t)rows * p.a3_ld));
        ProfScope ps(this, PC_SPLIT_ROWS, 0, (double)rows * p.Cin * 10.0);
        SDMI_LAUNCH_IN(ps, 0, launch_split3_rows(p.A, a3_tmp->p, rows, p.Cin, p.a_ld, p.a3_ld, stream_));
        p.A3 = a3_tmp->p;
    }
    // from here on the struct describes the phase launch: M = the rows of one phase, K = 4 cin
    p.Bt3 = w.up3; p.phases = 4; p.phase_stride = (long long)w.cout * w.cin * 24;
    p.b3_grouped = b3_grouped(p.N) ? 1 : 0;
    p.M = g.M; p.K = g.K; p.kt_total = g.kt_total; p.b_ld = p.K;
    p.kt_per_split = g.kt_per_split; p.splits = g.splits;
    const double flops = 2.0 * 4.0 * p.M * (double)p.N * p.K;      // executed
    const double bytes = (double)p.M * p.Cin * 6.0 + 4.0 * p.N * (double)p.K * 6.0 + 4.0 * p.M * (double)p.N * ((p.C ? 4.0 : 0.0) + (p.C3 ? 6.0 : 0.0));
    std::unique_ptr<Buf> slab;
    if (p.splits > 1) {
        p.slab_stride = 4ll * p.M * p.N;
        slab.reset(new Buf(this, (size_t)p.splits * p.slab_stride * sizeof(float)));
        p.slabs = slab->f();
    }
    {
        ProfScope ps(this, PC_CONV_SPLIT, flops, bytes);
        ps.set_tag("gemm 4x%d,%d,%d k3 phase cfg=%d splits=%d", p.M, p.N, p.K, g.cfg, p.splits);
        SDMI_LAUNCH_IN(ps, flops, launch_conv_gemm3p(p, g.tile.index, stream_));
    }
    if (p.splits > 1) {
        ProfScope ps(this, PC_SPLITK_REDUCE, 0, (double)(p.splits + 1) * p.slab_stride * 4.0);
        ps.set_tag("reduce 4x%d,%d,%d k3 phase cfg=%d splits=%d", p.M, p.N, p.K, g.cfg, p.splits);
        SDMI_LAUNCH_IN(ps, 0, launch_splitk_reduce(p, stream_));
    }
    return true;
}

// y = conv3x3(h, w_out) + conv1x1(x, w_skip) as ONE split-K plane launch + its reduce: the 1x1 shortcut of a ResBlock runs on extra K slices of conv_out's grid
// (ConvGemm::z_aux) and the reduce sums all slabs and adds both biases.  Against the two-launch path the shortcut's GEMM launch, its reduce where it is split and the
// write + read of its result as conv_out's residual are gone, and its matrix work joins a k loop that already runs.  Returns false -- nothing launched, the caller
// runs the two launches -- when the layers, the buffers or the planner (plan_gemm_pair: "do not pair") do not allow it.
bool Engine::conv_pair(const ConvW& w_out, const Act& h, const ConvW& w_skip, const Act& x, Act& y) {
    if (bf16_ || h.dt || x.dt || y.dt || w_out.dt || w_skip.dt || w_out.k != 3 || w_skip.k != 1 || probe_buf_) return false;
    if (h.c != w_out.cin || x.c != w_skip.cin || w_out.cout != w_skip.cout || y.c != w_out.cout) return false;
    if (h.n != x.n || h.h != x.h || h.w != x.w || y.n != h.n || y.h != h.h || y.w != h.w) return false;
    if (!plane_gemm(w_out.cin, w_out.cout) || !plane_gemm(w_skip.cin, w_skip.cout) || !h.p3 || !x.p3 || (!y.p && !y.p3)) return false;
    if (gopt_.force_splits > 0 && opt_splitk_aux_ <= 0) return false;   // option splitk alone forces the slices of ordinary launches: those run
    ConvGemm p{};
    p.Bt = w_out.bt; p.bias = w_out.bias; p.bias_aux = w_skip.bias;
    p.Bt3 = split_planes(w_out.bt); p.Bt3_aux = split_planes(w_skip.bt);
    if (!p.Bt3 || !p.Bt3_aux) return false;
    p.A3 = h.p3; p.a3_ld = h.ld3; p.A3_aux = x.p3; p.a3_ld_aux = x.ld3;
    p.C = y.p; p.C3 = y.p3; p.ldc3 = y.ld3;
    p.M = (int)h.rows(); p.N = w_out.cout; p.K = w_out.cin * 9;
    p.NB = h.n; p.Hs = h.h; p.Ws = h.w; p.Cin = w_out.cin; p.Ho = h.h; p.Wo = h.w;
    p.KH = 3; p.KW = 3; p.stride = 1; p.pad = 1; p.ups = 0;
    p.ldc = y.p ? y.stride() : p.N; p.ldr = p.ldc; p.a_ld = h.stride(); p.b_ld = p.K; p.CS = 32;
    p.kt_total = p.K / 32; p.Cin_aux = w_skip.cin; p.kt_total_aux = w_skip.cin / 32;
    p.b3_grouped = b3_grouped(p.N) ? 1 : 0;
    p.variant = opt_gemm3x_variant_;
    p.zero_page = zero_page_;
    // the output conditions of launch_gemm's native plane output, on the reduce's 16-byte path (the only one that writes planes or adds two biases at once)
    if (!splitk_reduce_vec(p, false) || ((uintptr_t)p.bias_aux & 15) || (p.C3 && (p.N % 32 || p.ldc3 % 192))) return false;
    const GemmPlanIn in = gemm_plan_in(p, 0, -1, 0);
    if (!in.p_ok) return false;
    if ((unsigned long long)p.N * (unsigned long long)p.kt_total_aux * 192ull >= 0xFFFFFF00ull || (unsigned long long)p.NB * p.Hs * p.Ws * (unsigned long long)p.a3_ld_aux >= 0xFFFFFF00ull) return false;
    const GemmPairPlan g = plan_gemm_pair(in, w_skip.cin, p.kt_total_aux, gopt_, tuning_, opt_splitk_aux_ > 0 ? std::max(gopt_.force_splits, 1) : 0, std::max(opt_splitk_aux_, 0));
    if (!g.pair) return false;
    p.kt_per_split = g.kt_per_split; p.splits = g.splits_main + g.splits_aux; p.z_aux = g.splits_main;
    if (record_shapes_) {
        char note[48];
        std::snprintf(note, sizeof note, " +aux K%d z%d", w_skip.cin, p.z_aux);
        record_choice(p, " pair", g.cfg, note);
    }
    p.slab_stride = (long long)p.M * p.N;
    Buf slab(this, (size_t)p.splits * p.slab_stride * sizeof(float));
    p.slabs = slab.f();
    const double flops = 2.0 * p.M * (double)p.N * ((double)p.K + w_skip.cin);
    const double bytes = (double)p.M * (w_out.cin + w_skip.cin) * 6.0 + (double)p.N * (p.K + w_skip.cin) * 6.0 + (double)p.M * p.N * ((p.C ? 4.0 : 0.0) + (p.C3 ? 6.0 : 0.0));
    {
        ProfScope ps(this, PC_CONV_SPLIT, flops, bytes);
        ps.set_tag("gemm %d,%d,%d+%d k3+1 cfg=%d splits=%d+%d", p.M, p.N, p.K, w_skip.cin, g.cfg, g.splits_main, g.splits_aux);
        SDMI_LAUNCH_IN(ps, flops, launch_conv_gemm3p(p, g.tile.index, stream_));
    }
    ProfScope ps(this, PC_SPLITK_REDUCE, 0, (double)(p.splits + 1) * p.slab_stride * 4.0);
    ps.set_tag("reduce %d,%d,%d+%d k3+1 cfg=%d splits=%d+%d", p.M, p.N, p.K, w_skip.cin, g.cfg, g.splits_main, g.splits_aux);
    SDMI_LAUNCH_IN(ps, 0, launch_splitk_reduce(p, stream_));
    return true;
}

// the ConvGemm of a Linear layer: [rows, cin] x [cout, cin]^T as a 1x1 convolution over one image of 1 x rows pixels
static ConvGemm linear_gemm(const float* A, int rows, const float* bt, const float* bias, int cin, int cout, float* C, int ldc, const float* resid, int ldr) {
    ConvGemm p{};
    p.A = A; p.Bt = bt; p.C = C; p.bias = bias; p.resid = resid;
    p.M = rows; p.N = cout; p.K = cin;
    p.NB = 1; p.Hs = 1; p.Ws = rows; p.Cin = cin; p.Ho = 1; p.Wo = rows;
    p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0; p.ups = 0;
    p.ldc = ldc; p.ldr = ldr; p.a_ld = cin; p.b_ld = cin; p.rowvec_stride = 0; p.CS = 32;
    return p;
}

// conv_pair with a Linear main problem: y = u x bt^T + bias + h x bt_aux^T + bias_aux + resid as ONE split-K plane launch + its reduce.  The transformer block's
// tail (spatial_transformer, option proj_out_fold): with bt = proj_out x mlp_lin folded at load (rebuild_folds), u the gated MLP hidden state, h the hidden state in
// front of the MLP and resid the block input, this is proj_out(h + mlp_lin(u)) + x -- proj_out's launch, its reduce where it is split and the write + read of the
// planes between the two layers are gone.  The residual is the reduce's to add (bias + bias_aux, then the residual: k_gemm.hip).
bool Engine::linear_pair(const LinearPair& a, bool plan_only) {
    if (bf16_ || probe_buf_ || a.rows <= 0 || a.cout <= 0 || a.k_main <= 0 || a.k_aux <= 0) return false;
    if (!plane_gemm(a.k_main, a.cout) || !plane_gemm(a.k_aux, a.cout) || !a.u3 || !a.h3 || (!a.C && !a.C3)) return false;
    if (gopt_.force_splits > 0 && opt_splitk_aux_ <= 0) return false;   // option splitk alone forces the slices of ordinary launches: those run
    const int ldc = a.C ? a.ldc : a.cout;
    ConvGemm p = linear_gemm(nullptr, a.rows, a.bt, a.bias, a.k_main, a.cout, a.C, ldc, a.resid, a.resid ? a.ldr : ldc);
    p.bias_aux = a.bias_aux;
    p.Bt3 = split_planes(a.bt); p.Bt3_aux = split_planes(a.bt_aux);
    if (!p.Bt3 || !p.Bt3_aux) return false;
    p.A3 = a.u3; p.a3_ld = a.u3_ld; p.A3_aux = a.h3; p.a3_ld_aux = a.h3_ld;
    p.C3 = a.C3; p.ldc3 = a.ldc3;
    p.kt_total = a.k_main / 32; p.Cin_aux = a.k_aux; p.kt_total_aux = a.k_aux / 32;
    p.b3_grouped = b3_grouped(p.N) ? 1 : 0;
    p.variant = opt_gemm3x_variant_;
    p.zero_page = zero_page_;
    if (p.a3_ld < p.kt_total * 192 || p.a3_ld % 192 || p.a3_ld_aux < p.kt_total_aux * 192 || p.a3_ld_aux % 192) return false;
    // the output conditions of launch_gemm's native plane output, on the reduce's 16-byte path (the only one that writes planes or adds two biases at once)
    if (!splitk_reduce_vec(p, false) || ((uintptr_t)p.bias_aux & 15) || (p.C3 && (p.N % 32 || p.ldc3 % 192 || p.ldc3 < p.N / 32 * 192))) return false;
    const GemmPlanIn in = gemm_plan_in(p, 0, -1, 0);
    if (!in.p_ok) return false;
    if ((unsigned long long)p.N * (unsigned long long)p.kt_total_aux * 192ull >= 0xFFFFFF00ull || (unsigned long long)a.rows * (unsigned long long)p.a3_ld_aux >= 0xFFFFFF00ull) return false;
    if (a.measured_only) {
        char key[80];
        std::snprintf(key, sizeof key, "%d,%d,%d+%d", p.M, p.N, p.K, a.k_aux);
        if (!tuning_.pairs.count(key)) return false;
    }
    const GemmPairPlan g = plan_gemm_pair(in, a.k_aux, p.kt_total_aux, gopt_, tuning_, opt_splitk_aux_ > 0 ? std::max(gopt_.force_splits, 1) : 0, std::max(opt_splitk_aux_, 0));
    if (!g.pair) return false;
    if (plan_only) return true;
    p.kt_per_split = g.kt_per_split; p.splits = g.splits_main + g.splits_aux; p.z_aux = g.splits_main;
    if (record_shapes_) {
        char note[48];
        std::snprintf(note, sizeof note, " +aux K%d z%d", a.k_aux, p.z_aux);
        record_choice(p, " fold", g.cfg, note);   // (" pair" names a ResBlock's: conv_pair)
    }
    p.slab_stride = (long long)p.M * p.N;
    Buf slab(this, (size_t)p.splits * p.slab_stride * sizeof(float));
    p.slabs = slab.f();
    const double flops = 2.0 * p.M * (double)p.N * ((double)p.K + a.k_aux);
    const double bytes = (double)p.M * (a.k_main + a.k_aux) * 6.0 + (double)p.N * (p.K + a.k_aux) * 6.0 + (double)p.M * p.N * ((p.C ? 4.0 : 0.0) + (p.C3 ? 6.0 : 0.0) + (p.resid ? 4.0 : 0.0));
    {
        ProfScope ps(this, PC_CONV_SPLIT, flops, bytes);
        ps.set_tag("gemm %d,%d,%d+%d k1+1%s cfg=%d splits=%d+%d", p.M, p.N, p.K, a.k_aux, p.resid ? " resid" : "", g.cfg, g.splits_main, g.splits_aux);
        SDMI_LAUNCH_IN(ps, flops, launch_conv_gemm3p(p, g.tile.index, stream_));
    }
    ProfScope ps(this, PC_SPLITK_REDUCE, 0, (double)(p.splits + 1) * p.slab_stride * 4.0);
    ps.set_tag("reduce %d,%d,%d+%d k1+1 cfg=%d splits=%d+%d", p.M, p.N, p.K, a.k_aux, g.cfg, g.splits_main, g.splits_aux);
    SDMI_LAUNCH_IN(ps, 0, launch_splitk_reduce(p, stream_));
    return true;
}

// what linear() and its MXFP8 form check alike: the shapes of x (c channels), y and resid against the weight
static void check_linear(const LinW& w, long long rows, int c, const Act& y, const Act* resid) {
    if (c != w.cin || y.rows() != rows || (y.c != w.cout && (w.fused < 2 || y.c != w.fused * w.cout)))
        throw Error(SDMI_ERR_STATE, "linear: the tensors do not have the weight's shape");
    if (resid && (resid->rows() != rows || resid->c != y.c || resid->dt != y.dt || !resid->p)) throw Error(SDMI_ERR_STATE, "linear: the residual does not have the output's shape and type");
}

void Engine::linear(const LinW& w, const Act& x, const Act& y, const Act* resid) {
    check_linear(w, x.rows(), x.c, y, resid);
    if (x.dt != y.dt || x.stride() != x.c) throw Error(SDMI_ERR_STATE, "linear: dense input rows of the output's storage type expected");
    if (w.cin % 32) throw Error(SDMI_ERR_UNSUPPORTED, "linear: in_features must be a multiple of 32");
    ConvGemm p = linear_gemm(x.p, (int)x.rows(), w.bt, w.bias, w.cin, y.c, y.p, y.stride(), resid ? resid->p : nullptr, resid ? resid->stride() : 0);
    p.A3 = x.p3; p.a3_ld = (w.cin / 32) * 192;      // dense planes in ...
    p.C3 = y.p3; p.ldc3 = (y.c / 32) * 192;         // ... and out
    if (y.p3 && (y.c % 32 || y.ld3 != p.ldc3)) throw Error(SDMI_ERR_STATE, "linear: plane output needs out_features % 32 == 0 and dense planes");
    launch_gemm(p, x.dt);
}

void Engine::gemm_geglu(const LinW& w, const Act& x, const Act& y) {
    const int dt = x.dt, cin = w.cin, hidden = w.cout / 2;
    const long long rows = x.rows();
    if (x.c != cin || y.c != hidden || w.cout != 2 * hidden || y.rows() != rows || y.dt != dt || x.stride() != cin || y.stride() != hidden)
        throw Error(SDMI_ERR_STATE, "geglu: dense tensors of the projection's shape expected");
    if (dt && (x.p3 || y.p3)) throw Error(SDMI_ERR_STATE, "geglu: planes are an fp32-engine format");
    if (x.p3 && !dt && opt_geglu_fuse_ && hidden % 32 == 0 && cin % 32 == 0 && split_planes(w.bt)) {
        // the gate in the plane GEMM's epilogue -- value / gate rows split by WAVE column, so the tiles with an odd fragment count per wave (256 x 160: the batch-1 model's) qualify
        const int cfg = plan_geglu_plane_tile(rows, hidden, cin, gopt_, tuning_);
        if (cfg >= 0) {
            ConvGemm p = linear_gemm(x.p, (int)rows, w.bt, w.bias, cin, hidden, y.p, hidden, nullptr, hidden);
            p.A3 = x.p3; p.a3_ld = (cin / 32) * 192;
            p.C3 = y.p3; p.ldc3 = (hidden / 32) * 192;
            p.geglu = 2;
            launch_gemm(p, 0, cfg, 1);
            return;
        }
    }
    if (x.p3 || y.p3) {   // plane form: projection on a plane tile, gate kernel writing planes (the MLP's second Linear reads them)
        Act proj = new_rows(rows, 2 * hidden, 1, 0);
        linear(w, x, proj);
        {
            ProfScope ps(this, PC_GEGLU, 0, (double)rows * hidden * (8.0 + (y.p3 ? 6.0 : 4.0)));
            if (y.p3) SDMI_LAUNCH_IN(ps, 0, launch_geglu_planes(proj.p, y.p3, rows, hidden, stream_));
            // (both asked for -- op_geglu_forward with geglu_fuse = 8: the fused launch above writes both, so must this form; the model asks for one)
            if (y.p) SDMI_LAUNCH_IN(ps, 0, launch_geglu(proj.p, y.p, rows, hidden, stream_));
        }
        release(proj);
        return;
    }
    // the fused form needs a large-tile kernel with an even fragment count per wave (256x256 or 256x128 tiles, no split-K)
    const bool eligible = opt_geglu_fuse_ && hidden % 8 == 0 && cin % (dt ? 64 : 32) == 0 && (dt ? gopt_.gemm_bf16x : gopt_.gemm_x32);
    const int cfg = eligible ? plan_geglu_paired_tile(rows, hidden, opt_geglu_fuse_, !dt && gopt_.gemm_f32s && split_planes(w.bt)) : -1;
    if (cfg >= 0) {
        ConvGemm p = linear_gemm(x.p, (int)rows, w.bt, w.bias, cin, hidden, y.p, hidden, nullptr, hidden);
        p.geglu = 1;
        launch_gemm(p, dt, cfg, 1);
        return;
    }
    Act proj = new_rows(rows, 2 * hidden, 1, dt);
    linear(w, x, proj);
    {
        ProfScope ps(this, PC_GEGLU, 0, (double)rows * hidden * (dt ? 6.0 : 12.0));
        if (dt) SDMI_LAUNCH_IN(ps, 0, launch_geglu_bf16(proj.p, y.p, rows, hidden, stream_));
        else SDMI_LAUNCH_IN(ps, 0, launch_geglu(proj.p, y.p, rows, hidden, stream_));
    }
    release(proj);
}

void Engine::group_norm(const NormW& w, const Act& x, Act& y, bool silu) {
    const int hw = x.h * x.w;
    if (x.dt != y.dt) throw Error(SDMI_ERR_STATE, "group_norm: in/out storage types disagree");
    Buf part(this, x.dt ? gn_partials_bytes_bf16(x.n, hw, x.c, gn_tune_) : gn_partials_bytes(x.n, hw, x.c, opt_gn32_min_wgs_));
    ProfScope ps(this, PC_GROUP_NORM, 0, 2.0 * (double)x.bytes(), 2);  // algorithmic: one read + one write; two launches (statistics, apply)
    ps.set_tag("group_norm n%d hw%d c%d%s", x.n, hw, x.c, silu ? " silu" : "");
    if (y.view) throw Error(SDMI_ERR_STATE, "group_norm: output must be dense");
    if (!x.p) throw Error(SDMI_ERR_STATE, "group_norm: the input must exist as fp32");
    if (y.p3 && !y.p) {   // the consumer is a plane GEMM: the normalised tensor is written as three bf16 planes only
        if (x.dt) throw Error(SDMI_ERR_STATE, "group_norm: planes are an fp32-engine format");
        SDMI_LAUNCH_IN(ps, 0, launch_group_norm_planes(x.p, y.p3, w.gamma, w.beta, x.n, hw, x.c, x.stride(), 32, w.eps, silu, part.p, stream_, opt_gn32_min_wgs_));
    }
    else if (x.dt) SDMI_LAUNCH_IN(ps, 0, launch_group_norm_bf16(x.p, y.p, w.gamma, w.beta, x.n, hw, x.c, x.stride(), 32, w.eps, silu, part.p, stream_, gn_tune_));
    else SDMI_LAUNCH_IN(ps, 0, launch_group_norm(x.p, y.p, w.gamma, w.beta, x.n, hw, x.c, x.stride(), 32, w.eps, silu, part.p, stream_, opt_gn32_min_wgs_));
    count_kernel();   // each launcher enqueues two kernels: statistics, apply
}

void Engine::layer_norm(const NormW& w, const Act& x, const Act& y) {
    const long long rows = x.rows();
    const int dt = x.dt;
    if (x.c != w.c || y.c != w.c || y.rows() != rows || y.dt != dt || !x.p || x.stride() != w.c || y.stride() != w.c || (y.p != nullptr) == (y.p3 != nullptr))
        throw Error(SDMI_ERR_STATE, "layer_norm: dense rows of the norm's width and one storage type expected, the output in one form");
    ProfScope ps(this, PC_LAYER_NORM, 0, 2.0 * (double)rows * w.c * (dt ? 2.0 : 4.0));
    ps.set_tag("layer_norm rows%lld c%d", rows, w.c);
    if (y.p3) {
        if (dt) throw Error(SDMI_ERR_STATE, "layer_norm: planes are an fp32-engine format");
        SDMI_LAUNCH_IN(ps, 0, launch_layer_norm_planes(x.p, y.p3, w.gamma, w.beta, (int)rows, w.c, w.eps, stream_));
    } else if (dt) SDMI_LAUNCH_IN(ps, 0, launch_layer_norm_bf16(x.p, y.p, w.gamma, w.beta, (int)rows, w.c, w.eps, stream_));
    else SDMI_LAUNCH_IN(ps, 0, launch_layer_norm(x.p, y.p, w.gamma, w.beta, (int)rows, w.c, w.eps, stream_));
}

// qkv_attention (attention.rs:5-45).  Head dims with a fused instance use the flash
// kernel; others (the VAE's single 512-wide head) run QK^T -> row softmax -> PV on
// the GEMM kernel, one (batch, head) at a time.
void Engine::attention(const Attn& a) {
    const int dt = a.dt < 0 ? edt() : a.dt, n = a.n, nq = a.nq, nk = a.nk, n_head = a.n_head, d_head = a.d_head;
    const bool q_log2 = a.q_log2;
    if (nq <= 0 || nk <= 0) throw Error(SDMI_ERR_INVALID, "attention: empty sequence");
    AttnPlanIn in{};
    in.n = n; in.n_head = n_head; in.nq = nq; in.nk = nk; in.d_head = d_head; in.bf16 = dt; in.has_mask = a.mask != nullptr; in.planes_out = a.o3 != nullptr;
    in.rows_aligned = !((a.q.ld | a.k.ld | a.v.ld | a.o.ld) & (dt ? 7 : 3));
    const AttnPlan plan = plan_attention(in, aopt_);   // kernel, workgroup form, key slices (attn_plan.cpp); refuses what no kernel serves
    // q_log2 (stated by the caller, Engine::q_prescaled): q arrives in log2 units (attn_bf16_q_scale: folded into the query weights at load, applied by
    // qkv_attention_dev's conversion); the bf16 kernel needs no scale, the widened fp32 kernel (attn_bf16=0) gets scale^2 = ln 2
    if (q_log2 != q_prescaled(dt, d_head)) throw Error(SDMI_ERR_STATE, "attention: the caller's statement about the query's scale does not match the storage type / head dim");
    const float scale = q_log2 ? 0.83255461115769775635f : (float)std::pow((double)d_head, -0.25);
    if (plan.kernel != AttnKernel::Unfused) {
        AttnParams p{};
        p.q = a.q.p; p.k = a.k.p; p.v = a.v.p; p.o = const_cast<float*>(a.o.p); p.kv_len = a.kv_len_dev; p.mask = a.mask; p.mask_ld = a.mask_ld;
        p.n = n; p.n_head = n_head; p.nq = nq; p.nk = nk; p.d_head = d_head;
        p.ldq = a.q.ld; p.ldk = a.k.ld; p.ldv = a.v.ld; p.ldo = a.o.ld;
        p.q_bs = a.q.bs; p.k_bs = a.k.bs; p.v_bs = a.v.bs; p.o_bs = a.o.bs; p.scale = scale;
        p.bf16 = dt;
        p.q_log2 = q_log2 ? 1 : 0;
        p.o3 = a.o3; p.ldo3 = (n_head * d_head / 32) * 192;
        const double fl = 4.0 * n * n_head * (double)nq * nk * d_head;
        const int kv_splits = plan.kv_splits;
        std::unique_ptr<Buf> part_o, part_ml;
        if (kv_splits > 1) {
            part_o.reset(new Buf(this, (size_t)kv_splits * n * nq * n_head * d_head * sizeof(float)));
            part_ml.reset(new Buf(this, (size_t)kv_splits * n * n_head * nq * 2 * sizeof(float)));
            p.kv_splits = kv_splits; p.part_o = part_o->f(); p.part_ml = part_ml->f();
        }
        ProfScope ps(this, PC_ATTENTION, fl, 0, kv_splits > 1 ? 2 : 1);
        ps.set_tag("attention n%d nq%d nk%d h%d d%d slices=%d", n, nq, nk, n_head, d_head, kv_splits);
        if (plan.kernel == AttnKernel::Bf16) SDMI_LAUNCH_IN(ps, fl, launch_attention_bf16(p, plan, stream_));
        else if (plan.kernel == AttnKernel::Split) SDMI_LAUNCH_IN(ps, fl, launch_attention_split(p, plan, stream_));
        else SDMI_LAUNCH_IN(ps, fl, launch_attention(p, plan, stream_));
        if (kv_splits > 1) SDMI_LAUNCH_IN(ps, 0, launch_attention_combine(p, stream_));
        return;
    }
    const int* kv_len_host = a.kv_len_host;
    const int ldq = a.q.ld, ldk = a.k.ld, ldv = a.v.ld, ldo = a.o.ld;
    for (int b = 0; b < n; ++b)   // every sample's key count before the first launch
        if ((kv_len_host ? kv_len_host[b] : nk) % (dt ? 64 : 32)) throw Error(SDMI_ERR_UNSUPPORTED, "attention (unfused path): key count must be a multiple of 32 (64 for bf16)");
    for (int b = 0; b < n; ++b) {
        const int nkb = kv_len_host ? kv_len_host[b] : nk;
        Buf s(this, (size_t)nq * nkb * sizeof(float));            // scores stay fp32 in both precisions
        Buf pb(this, dt ? (size_t)nq * nkb * 2 : 256);             // bf16 probabilities (precision = 1)
        Buf vt(this, (size_t)d_head * nkb * (dt ? 2 : 4));
        for (int h = 0; h < n_head; ++h) {
            const float* qb = adv(a.q.p, b * a.q.bs + h * d_head, dt);
            const float* kb = adv(a.k.p, b * a.k.bs + h * d_head, dt);
            const float* vb = adv(a.v.p, b * a.v.bs + h * d_head, dt);
            float* ob = adv(a.o.p, b * a.o.bs + h * d_head, dt);
            ConvGemm g{};
            g.A = qb; g.Bt = kb; g.C = s.f();
            g.M = nq; g.N = nkb; g.K = d_head; g.NB = 1; g.Hs = 1; g.Ws = nq; g.Cin = d_head; g.Ho = 1; g.Wo = nq;
            g.KH = g.KW = 1; g.stride = 1; g.ldc = nkb; g.ldr = nkb; g.a_ld = ldq; g.b_ld = ldk; g.CS = 32;
            g.out_mode = dt ? 1 : 0;
            launch_gemm(g, dt);
            if (dt) SDMI_LAUNCH(launch_softmax_rows_f32_to_bf16(s.f(), pb.p, nq, nkb, scale * scale, stream_));
            else SDMI_LAUNCH(launch_softmax_rows(s.f(), nq, nkb, scale * scale, stream_));
            if (dt) SDMI_LAUNCH(launch_transpose2d_bf16(vb, vt.p, nkb, d_head, ldv, stream_));
            else SDMI_LAUNCH(launch_transpose2d(vb, vt.f(), nkb, d_head, ldv, stream_));
            ConvGemm g2{};
            g2.A = dt ? pb.f() : s.f(); g2.Bt = vt.f(); g2.C = ob;
            g2.M = nq; g2.N = d_head; g2.K = nkb; g2.NB = 1; g2.Hs = 1; g2.Ws = nq; g2.Cin = nkb; g2.Ho = 1; g2.Wo = nq;
            g2.KH = g2.KW = 1; g2.stride = 1; g2.ldc = ldo; g2.ldr = ldo; g2.a_ld = nkb; g2.b_ld = nkb; g2.CS = 32;
            launch_gemm(g2, dt);
        }
    }
}

// =============================================================================
// composite blocks
// =============================================================================
// ResBlock::forward (unet/mod.rs:713-733) / ResnetBlock::forward (autoencoder/mod.rs:514-527)
void Engine::res_block(const ResW& w, const Act& x, Act& y, int step) {
    Range rng(this, "ResBlock");
    Act h2 = new_act(x.n, x.h, x.w, w.cout);
    const float* rowvec = nullptr;
    if (w.has_embed) rowvec = us_.temb.at(w.temb_index) + (size_t)step * w.cout;  // shared by the batch (one timestep)
    if (use_fp8(w.conv_in, x)) {   // precision = 2: the normalisation writes MXFP8, the conv runs on the MX-scaled matrix instruction
        ActQ q1 = new_actq(x.n, x.h, x.w, x.c);
        group_norm_fp8(w.norm_in, x, q1, true);
        conv_fp8(w.conv_in, q1, h2, rowvec, nullptr);
        release(q1);
    } else {
        // the normalised tensors have one consumer, a 3x3 convolution: on the fp32 engine they exist only as bf16 planes (k_gemm3p.hip)
        Act h1 = plane_gemm(x.c, w.cout) ? new_act3(x.n, x.h, x.w, x.c, 2) : new_act(x.n, x.h, x.w, x.c);
        group_norm(w.norm_in, x, h1, true);
        conv(w.conv_in, h1, h2, 1, 0, rowvec, 0, nullptr);
        release(h1);
    }
    // fp32 engine, option skip_slices: the 1x1 shortcut rides on extra K slices of conv_out's split-K launch (conv_pair) -- no launch, reduce or
    // residual buffer of its own.  Where conv_pair declines (x without planes, conv_out not split, a "0" row of the pairs table ...) the two launches below run.
    Act h3{};
    if (w.has_skip && opt_skip_slices_ && !bf16_ && !fp8_ && plane_gemm(w.cout, w.cout) && plane_gemm(x.c, w.cout) && x.p3) {
        h3 = new_act3(x.n, x.h, x.w, w.cout, 2);
        group_norm(w.norm_out, h2, h3, true);   // (independent of the shortcut: where conv_pair declines, the launches below find it done)
        release(h2);
        if (conv_pair(w.conv_out, h3, w.skip, x, y)) {
            release(h3);
            return;
        }
    }
    // the shortcut's result is the residual of conv_out: it goes through y's fp32 buffer, or through a temporary when y exists as planes only
    Act sk{};
    if (w.has_skip) {
        if (y.p) { sk = y; sk.p3 = nullptr; sk.view = true; }
        else sk = new_act(y.n, y.h, y.w, y.c);
        if (use_fp8_wide(w.skip.bt8, x.rows()) && x.dt == 1 && x.c % 32 == 0) {
            ActQ xq = new_actq(x.n, x.h, x.w, x.c);
            quantize(x, xq);
            conv_fp8(w.skip, xq, sk, nullptr, nullptr);
            release(xq);
        } else {
            conv(w.skip, x, sk, 1, 0, nullptr, 0, nullptr);
        }
    }
    const Act* resid = w.has_skip ? &sk : &x;
    if (use_fp8(w.conv_out, h2)) {
        ActQ q3 = new_actq(x.n, x.h, x.w, w.cout);
        group_norm_fp8(w.norm_out, h2, q3, true);
        release(h2);
        conv_fp8(w.conv_out, q3, y, nullptr, resid);
        release(q3);
    } else {
        if (!h3.p3) {
            h3 = plane_gemm(w.cout, w.cout) ? new_act3(x.n, x.h, x.w, w.cout, 2) : new_act(x.n, x.h, x.w, w.cout);
            group_norm(w.norm_out, h2, h3, true);
            release(h2);
        }
        conv(w.conv_out, h3, y, 1, 0, nullptr, 0, resid);
        release(h3);
    }
    if (w.has_skip) release(sk);
}

// ---- precision = 2: MXFP8 GroupNorm output + 3x3 convolution (k_fp8.hip) ------------------------------------------------
bool Engine::use_fp8(const ConvW& w, const Act& x) const {
    return fp8_ && opt_fp8_convs_ && w.bt8 && x.dt == 1 && x.rows() >= opt_fp8_min_rows_;
}

ActQ Engine::new_actq(int n, int h, int w, int c) {
    ActQ a; a.n = n; a.h = h; a.w = w; a.c = c; a.cp = (c + 127) / 128 * 128;
    a.q = pool_.alloc((size_t)a.rows() * a.cp);
    a.s = pool_.alloc((size_t)a.rows() * (a.cp / 32));
    return a;
}
void Engine::release(ActQ& a) {
    if (a.q) pool_.free(a.q);
    if (a.s) pool_.free(a.s);
    a.q = a.s = nullptr;
}

void Engine::group_norm_fp8(const NormW& w, const Act& x, ActQ& y, bool silu) {
    const int hw = x.h * x.w;
    if (x.dt != 1 || y.c != x.c) throw Error(SDMI_ERR_STATE, "group_norm_fp8: bf16 input of matching width expected");
    Buf part(this, gn_partials_bytes_bf16(x.n, hw, x.c, gn_tune_));
    ProfScope ps(this, PC_GROUP_NORM, 0, (double)x.bytes() + (double)x.rows() * (y.cp + y.cp / 32), 2);
    SDMI_LAUNCH_IN(ps, 0, launch_group_norm_fp8(x.p, y.q, y.s, w.gamma, w.beta, x.n, hw, x.c, x.stride(), 32, w.eps, silu, part.p, stream_, &gn_tune_));
    count_kernel();   // statistics + apply
}

void Engine::conv_fp8(const ConvW& w, const ActQ& x, Act& y, const float* rowvec, const Act* resid, int stride, int ups, int rowvec_stride) {
    if (x.c != w.cin || (w.k != 3 && w.k != 1) || !w.bt8) throw Error(SDMI_ERR_STATE, "conv_fp8: not an MXFP8-packed convolution");
    const int pad = w.k == 3 ? 1 : 0;
    const int hin = x.h << ups, win = x.w << ups;
    const int ho = (hin + 2 * pad - w.k) / stride + 1, wo = (win + 2 * pad - w.k) / stride + 1;
    if (y.n != x.n || y.h != ho || y.w != wo || y.c != w.cout || y.dt != 1) throw Error(SDMI_ERR_INVALID, "conv_fp8: output shape / type mismatch");
    if (resid && (resid->rows() != y.rows() || resid->c != y.c || resid->dt != 1)) throw Error(SDMI_ERR_STATE, "conv_fp8: residual shape / type mismatch");
    ConvGemm p{};
    p.A = reinterpret_cast<const float*>(x.q); p.Bt = w.bt8; p.C = y.p; p.bias = w.bias; p.rowvec = rowvec; p.resid = resid ? resid->p : nullptr;
    p.a_scale = x.s; p.b_scale = w.bs8;
    p.M = x.n * ho * wo; p.N = w.cout; p.K = x.cp * w.k * w.k;
    p.NB = x.n; p.Hs = x.h; p.Ws = x.w; p.Cin = x.cp; p.Ho = ho; p.Wo = wo;
    p.KH = w.k; p.KW = w.k; p.stride = stride; p.pad = pad; p.ups = ups;
    p.ldc = y.stride(); p.ldr = resid ? resid->stride() : y.stride(); p.a_ld = x.cp; p.b_ld = p.K; p.rowvec_stride = rowvec_stride; p.CS = 128;
    launch_fp8(p, 2.0 * p.M * (double)p.N * w.cin * w.k * w.k);   // algorithmic (unpadded) work
}

// y (bf16) = x W^T + bias (+ resid): a Linear layer on MXFP8 operands
void Engine::linear(const LinW& w, const ActQ& x, const Act& y, const Act* resid) {
    check_linear(w, x.rows(), x.c, y, resid);
    if (!w.bt8 || y.dt != 1 || !y.p) throw Error(SDMI_ERR_STATE, "linear: not an MXFP8-packed Linear layer with a bf16 output");
    ConvGemm p = linear_gemm(reinterpret_cast<const float*>(x.q), (int)x.rows(), w.bt8, w.bias, x.cp, y.c, y.p, y.stride(), resid ? resid->p : nullptr, resid ? resid->stride() : 0);
    p.a_scale = x.s; p.b_scale = w.bs8; p.CS = 128;
    launch_fp8(p, 2.0 * p.M * (double)p.N * w.cin);
}

void Engine::launch_fp8(ConvGemm& p, double flops) {
    p.out_mode = 0;
    p.variant = opt_gemm_bf16x_variant_;
    p.zero_page = zero_page_;
    p.kt_total = p.K / 128;
    if ((unsigned long long)p.NB * p.Hs * p.Ws * (unsigned long long)p.a_ld >= 0xFFFFFFE0ull || (unsigned long long)p.N * p.K >= 0xFFFFFFE0ull) throw Error(SDMI_ERR_UNSUPPORTED, "fp8 GEMM: operand larger than 4 GiB");
    const TileChoice tc = plan_gemm_fp8(p.M, p.N, p.kt_total, opt_fp8_tile_, gopt_.force_splits, &p.kt_per_split);
    p.splits = tc.splits;
    set_resid_acc(p, tc.splits == 1, true);   // (as Engine::launch_gemm)
    record_choice(p, " fp8", tc.cfg, "");   // the MXFP8 launches are listed with their own tag, so a test can pin WHICH layers run on fp8 operands
    // algorithmic bytes: e4m3 operands + one E8M0 scale byte per 32 elements, bf16 result
    const double fp8_bytes = ((double)p.NB * p.Hs * p.Ws * p.a_ld + (double)p.N * p.K) * (1.0 + 1.0 / 32.0) + (double)p.M * p.N * 2.0;
    run_gemm(p, GemmRun{launch_conv_gemm_fp8x, tc.cfg, "gemm_fp8", tc.cfg, PC_CONV_FP8, true, false, flops, fp8_bytes});
}

// a convolution whose input is a raw (not normalised) activation -- the down / up convolutions (unet/mod.rs:397,425; autoencoder/mod.rs:319):
// precision = 2 with option fp8_linear quantises the input in front of it, everything else is conv()
void Engine::conv_raw(const ConvW& w, const Act& x, Act& y, int stride, int ups) {
    if (use_fp8_wide(w.bt8, y.rows()) && x.dt == 1 && y.dt == 1 && x.p && x.c % 32 == 0) {
        ActQ xq = new_actq(x.n, x.h, x.w, x.c);
        quantize(x, xq);
        conv_fp8(w, xq, y, nullptr, nullptr, stride, ups);
        release(xq);
        return;
    }
    conv(w, x, y, stride, ups, nullptr, 0, nullptr);
}

void Engine::quantize(const Act& x, ActQ& y) {
    if (x.dt != 1 || !x.p || y.c != x.c || y.rows() != x.rows()) throw Error(SDMI_ERR_STATE, "quantize: bf16 input of matching shape expected");
    ProfScope ps(this, PC_OTHER, 0, (double)x.rows() * (x.c * 2.0 + y.cp * 1.03));
    SDMI_LAUNCH_IN(ps, 0, launch_quantize_bf16_fp8(x.p, y.q, y.s, x.rows(), x.c, x.stride(), stream_));
}

void Engine::layer_norm(const NormW& w, const Act& x, ActQ& y) {
    const long long rows = x.rows();
    if (y.c != w.c || y.rows() != rows || x.c != w.c || x.dt != 1 || !x.p || x.stride() != w.c) throw Error(SDMI_ERR_STATE, "layer_norm (MXFP8 out): dense bf16 rows of the norm's width expected");
    ProfScope ps(this, PC_LAYER_NORM, 0, (double)rows * (w.c * 2.0 + y.cp * 1.03));
    SDMI_LAUNCH_IN(ps, 0, launch_layer_norm_fp8(x.p, y.q, y.s, w.gamma, w.beta, (int)rows, w.c, w.eps, stream_));
}

// SpatialTransformer::forward (unet/mod.rs:462-480) + TransformerBlock (:522-526) +
// MultiHeadAttention (:642-652) + MLP/GEGLU (:552-591).  NHWC makes the reference's
// two NCHW<->token transposes disappear.
void Engine::spatial_transformer(const SpatialW& w, const Act& x, Act& y) {
    Range rng(this, "SpatialTransformer");
    // y.n == 2 x.n: the shared prefix of a CFG pair (unet_run): x holds ONE copy of the two halves' identical input; everything in front of the cross attention --
    // the first place the text context enters -- is computed once and duplicated there
    if (y.n != x.n && y.n != 2 * x.n) throw Error(SDMI_ERR_STATE, "spatial_transformer: batch mismatch");
    auto duplicate = [&](const Act& src) {   // [n] -> [2n] (dense, same type): both halves = src
        Act d2 = new_act(2 * src.n, src.h, src.w, src.c);
        ProfScope ps_o(this, PC_OTHER, 0, 3.0 * (double)src.bytes());
        SDMI_LAUNCH_IN(ps_o, 0, launch_repeat_rows(src.p, d2.p, 2, (long long)(src.bytes() / 4), stream_));
        return d2;
    };
    const int C = w.c, hw = x.h * x.w;
    const int heads = unet_heads(C), d = C / heads;
    // both attentions of the block: n samples of hw queries against nk keys -> o (fp32 / bf16 rows, or planes)
    auto attend = [&](Attn& at, int n, int nk, const Act& o) {
        at.o = attn_rows(o, hw); at.o3 = o.p3;
        at.n = n; at.nq = hw; at.nk = nk; at.n_head = heads; at.d_head = d; at.q_log2 = q_prescaled(edt(), d);
        attention(at);
    };
    auto cross_attend = [&](const Act& q, const Act& o) {   // against the hoisted K / V of the text context
        Attn at;
        const long long ctx_rows = (long long)y.n * us_.t_max;
        at.k = attn_rows(rows_view(us_.kc.at(w.ctx_index), ctx_rows, C, edt()), us_.t_max);
        at.v = attn_rows(rows_view(us_.vc.at(w.ctx_index), ctx_rows, C, edt()), us_.t_max);
        at.q = attn_rows(q, hw); at.kv_len_dev = us_.kv_len_dev; at.kv_len_host = us_.kv_len_host.data();
        attend(at, y.n, us_.t_max, o);
    };
    if (y.n != x.n && use_fp8_wide(w.proj_in.bt8, y.rows()) && x.dt == 1 && y.dt == 1) {   // option fp8_linear: no shared form -- duplicate first
        Act x2 = duplicate(x);
        spatial_transformer(w, x2, y);
        release(x2);
        return;
    }
    const int nb = y.n, n1 = x.n;            // n1: samples of the part in front of the cross attention
    const bool share = nb != n1;
    const long long M = (long long)nb * hw, M1 = (long long)n1 * hw;
    if (use_fp8_wide(w.proj_in.bt8, M) && w.attn1.q.bt8 && w.attn1.out.bt8 && w.attn2.q.bt8 && w.attn2.out.bt8 && w.geglu_proj.bt8 && w.mlp_lin.bt8 &&
        w.proj_out.bt8 && x.dt == 1 && y.dt == 1) {
        // precision = 2, option fp8_linear: every GEMM of the block on MXFP8 operands.  Their inputs are quantised by the kernel that
        // produces them (GroupNorm, LayerNorm, the GEGLU gate) or by quantize() (attention outputs, the hidden state in front of proj_out);
        // the residual stream h, q / k / v and the attention itself stay bf16 (why attention is not fp8).
        ActQ gq = new_actq(x.n, x.h, x.w, C);
        group_norm_fp8(w.norm, x, gq, false);
        Act h = new_act(x.n, x.h, x.w, C);
        conv_fp8(w.proj_in, gq, h, nullptr, nullptr);
        release(gq);
        {
            ActQ lnq = new_rowsq(M, C), aq = new_rowsq(M, C);
            Act q = new_rows(M, C), a = new_rows(M, C);
            layer_norm(w.ln1, h, lnq);
            {
                Act qkv = new_rows(M, 3 * C);
                linear(w.attn1.q, lnq, qkv);      // q | k | v: the packed [3C][Kp] weight
                Attn at;
                attn_packed_qkv(qkv, hw, at); attend(at, nb, hw, a);
                release(qkv);
            }
            quantize(a, aq);
            linear(w.attn1.out, aq, h, &h);
            layer_norm(w.ln2, h, lnq);
            linear(w.attn2.q, lnq, q);
            cross_attend(q, a);
            ip_attention(w, q, a, nb, hw, heads, d);   // IP-Adapter: + the image term, in front of the quantisation
            quantize(a, aq);
            linear(w.attn2.out, aq, h, &h);
            layer_norm(w.ln3, h, lnq);
            {
                Act proj = new_rows(M, 8 * C);
                linear(w.geglu_proj, lnq, proj);
                ActQ uq = new_rowsq(M, 4 * C);
                {
                    ProfScope ps(this, PC_GEGLU, 0, (double)M * (8.0 * C * 2.0 + 4.0 * C * 1.03));
                    SDMI_LAUNCH_IN(ps, 0, launch_geglu_fp8(proj.p, uq.q, uq.s, M, 4 * C, stream_));
                }
                linear(w.mlp_lin, uq, h, &h);
                release(uq);
                release(proj);
            }
            release(lnq); release(aq);
            release(a); release(q);
        }
        ActQ hq = new_actq(x.n, x.h, x.w, C);
        quantize(h, hq);
        release(h);
        conv_fp8(w.proj_out, hq, y, nullptr, &x);
        release(hq);
        return;
    }
    // fp32 engine: every tensor whose only consumer is a GEMM (the normalised activations, the attention outputs, the gated MLP
    // hidden state, the block's last hidden state) is written by its producer as three bf16 planes -- what k_gemm3p.hip reads
    const bool pl = plane_gemm(C, C) && attn_supported_head_dim(d);
    Act g = pl ? new_act3(x.n, x.h, x.w, C, 2) : new_act(x.n, x.h, x.w, C);
    group_norm(w.norm, x, g, false);
    Act h = new_act(x.n, x.h, x.w, C);
    conv(w.proj_in, g, h, 1, 0, nullptr, 0, nullptr);
    release(g);
    Act hp{};                                                 // (pl) the hidden state after the MLP as planes: read by proj_out only
    Act x2{};                                                 // shared prefix: the block input once per half (proj_out's residual)
    bool folded = false;                                      // mlp_lin + proj_out ran as one paired launch (option proj_out_fold)
    {
        // the row tensors of the block: planes only where their one consumer is a plane GEMM (pl), the storage type otherwise
        const int form = pl ? 2 : 1;
        const size_t row3 = (size_t)(C / 32) * 192;
        Act ln = new_rows(M, C, form), q = new_rows(M, C), a = new_rows(M, C, form);
        const Act ln1 = top(ln, M1), a1 = top(a, M1);   // in front of the cross attention: n1 samples
        // self attention: q, k, v in one GEMM (N = 3C) on the packed [3C][C] weight
        layer_norm(w.ln1, h, ln1);
        {
            Act qkv = new_rows(M1, 3 * C);
            linear(w.attn1.q, ln1, qkv);
            Attn at;
            attn_packed_qkv(qkv, hw, at); attend(at, n1, hw, a1);
            release(qkv);
        }
        linear(w.attn1.out, a1, h, &h);
        if (share) {   // from here on the halves differ: the hidden state and the block input, once per half
            Act h2 = duplicate(h);
            release(h);
            h = h2;
            x2 = duplicate(x);
        }
        layer_norm(w.ln2, h, ln);
        linear(w.attn2.q, ln, q);
        cross_attend(q, a);
        ip_attention(w, q, a, nb, hw, heads, d);   // IP-Adapter: + the image term (planes: read-modify-write)
        // Option proj_out_fold: y = x + proj_out(h + mlp_lin(u)) has no nonlinearity between its two layers, so with Wf = proj_out x mlp_lin folded at load
        // (rebuild_folds) it is y = x + Wf u + proj_out h + (bf + b_proj): ONE paired launch (linear_pair) whose extra K slices carry proj_out h.  h is then needed
        // as planes: the cross attention's output projection writes them next to its fp32 result.  A block whose fold is not fresh, or whose shape the planner does
        // not pair, runs the two launches.
        const Act& xr = share ? x2 : x;
        Act h3{};
        if (pl && opt_proj_out_fold_ && w.fold_fresh) h3 = new_rows(M, C, 2);
        LinearPair lp{h3.p3 /* (for the plan: any plane buffer) */, (int)(4 * row3), w.fold_bt, w.fold_bias, 4 * C, h3.p3, (int)row3, w.proj_out.bt, w.proj_out.bias, C,
                      (int)M, C, xr.p, xr.stride(), y.p, y.stride(), y.p3, y.ld3, opt_proj_out_fold_ == 2};
        const bool fold = h3.p3 && xr.p && !xr.dt && !y.dt && xr.rows() == M && xr.c == C && y.rows() == M && y.c == C && linear_pair(lp, /*plan_only=*/true);
        Act hh = h;   // the hidden state as attn2.out writes it, a view: fp32 and, for the pair, the planes h3 next to it
        hh.view = true; hh.p3 = fold ? h3.p3 : nullptr; hh.ld3 = h3.ld3;
        linear(w.attn2.out, a, hh, &h);
        // GEGLU MLP
        layer_norm(w.ln3, h, ln);
        {
            Act u = new_rows(M, 4 * C, form);
            gemm_geglu(w.geglu_proj, ln, u);
            lp.u3 = u.p3;
            if (fold && linear_pair(lp)) folded = true;
            else if (pl) {
                hp = new_act3(nb, x.h, x.w, C, 2);
                linear(w.mlp_lin, u, hp, &h);   // h + mlp -> planes only
            }
            else linear(w.mlp_lin, u, h, &h);
            release(u);
        }
        if (h3.p3) release(h3);
        release(a); release(q); release(ln);
    }
    const Act& xr = share ? x2 : x;
    if (pl && !folded) { conv(w.proj_out, hp, y, 1, 0, nullptr, 0, &xr); release(hp); }
    else if (!folded) conv(w.proj_out, h, y, 1, 0, nullptr, 0, &xr);
    release(h);
    if (share) release(x2);
}

// ConvSelfAttentionBlock::forward (autoencoder/mod.rs:563-607)
void Engine::vae_attn(const VaeAttnW& w, const Act& x, Act& y) {
    Range rng(this, "ConvSelfAttentionBlock");
    const int C = w.c, hw = x.h * x.w;
    Act g = new_act(x.n, x.h, x.w, C);
    group_norm(w.norm, x, g, false);
    Act q = new_act(x.n, x.h, x.w, C), k = new_act(x.n, x.h, x.w, C), v = new_act(x.n, x.h, x.w, C);
    conv(w.q, g, q, 1, 0, nullptr, 0, nullptr);
    conv(w.k, g, k, 1, 0, nullptr, 0, nullptr);
    conv(w.v, g, v, 1, 0, nullptr, 0, nullptr);
    release(g);
    Act a = new_act(x.n, x.h, x.w, C);
    Attn at;
    at.q = attn_rows(q, hw); at.k = attn_rows(k, hw); at.v = attn_rows(v, hw); at.o = attn_rows(a, hw); at.n = x.n; at.nq = hw; at.nk = hw; at.n_head = 1; at.d_head = C;
    attention(at);
    release(q); release(k); release(v);
    conv(w.proj_out, a, y, 1, 0, nullptr, 0, &x);
    release(a);
}

// =============================================================================
// UNet driver
// =============================================================================
void Engine::unet_release() {
    for (void* p : us_.owned) pool_.free(p);
    us_ = UNetState{};
    ip_live_ = false;
}

// Hoists everything that does not depend on the latent out of the step loop:
// the time-embedding MLP for every timestep (unet/mod.rs:115-118), each ResBlock's
// Linear(SiLU(emb)) (unet/mod.rs:718-719) and each cross-attention's K/V projection
// of the text context (unet/mod.rs:646-647), which the reference recomputes in all
// 2*n_steps forwards.
void Engine::unet_prepare(const float* ctx_packed, int nb, int t_max, const int* kv_len_host,
                          const std::vector<int>& ts, int n_images, bool window, bool force_control) {
    unet_prepare_rows(ctx_packed, nb, t_max, kv_len_host, ts.data(), nullptr, (int)ts.size(), n_images, window, force_control);
}

void Engine::unet_prepare(const float* ctx_packed, int nb, int t_max, const int* kv_len_host, const std::vector<double>& tf, const std::vector<int>& eval_step,
                          int call_steps, int n_images) {
    if (tf.empty() || eval_step.size() != tf.size() || call_steps < 1) throw Error(SDMI_ERR_STATE, "unet_prepare: bad evaluation plan");
    std::vector<float> t32(tf.size());
    for (size_t i = 0; i < tf.size(); ++i) t32[i] = (float)tf[i];   // THE narrowing of the evaluation times
    unet_prepare_rows(ctx_packed, nb, t_max, kv_len_host, nullptr, t32.data(), (int)t32.size(), n_images, /*window=*/true, /*force_control=*/false);
    us_.eval_step = eval_step;
    us_.call_steps = call_steps;
}

// ti: S integer timesteps, or null and tf: S fractional ones -- one row of every per-step table each
void Engine::unet_prepare_rows(const float* ctx_packed, int nb, int t_max, const int* kv_len_host, const int* ti, const float* tf, int S, int n_images, bool window,
                               bool force_control) {
    unet_release();
    // a controlled call (sticky state, sdmi_set_control): strength 0 is the plain call, launch for launch (force_control: control_residuals_dev, which ignores the strength)
    const bool ctrl = ctrl_.set && (ctrl_.strength != 0.0 || force_control) && n_images > 0;
    if (ctrl) {
        if (!control_ready()) throw Error(SDMI_ERR_STATE, "control: the ControlNet weights (controlnet/...) are no longer complete");
        if (ctrl_.hint_h != 8 * lat_h_ || ctrl_.hint_w != 8 * lat_w_)
            throw Error(SDMI_ERR_INVALID, "control: the hint is " + std::to_string(ctrl_.hint_h) + " x " + std::to_string(ctrl_.hint_w) + " but the latent size in force, " +
                                              std::to_string(lat_h_) + " x " + std::to_string(lat_w_) + ", needs " + std::to_string(8 * lat_h_) + " x " + std::to_string(8 * lat_w_));
        if (ctrl_.n_hint != 1 && ctrl_.n_hint != n_images)
            throw Error(SDMI_ERR_INVALID, "control: the call has n = " + std::to_string(n_images) + " images but the control was set with n_hint = " + std::to_string(ctrl_.n_hint));
    }
    const int mc = cfg_.model_channels, ed = 4 * mc, cd = cfg_.ctx_dim;
    us_.nb = nb; us_.t_max = t_max; us_.steps = S;
    us_.window = window;
    us_.kv_len_host.assign(kv_len_host, kv_len_host + nb);
    auto own = [&](size_t bytes) { void* p = pool_.alloc(bytes); us_.owned.push_back(p); return p; };
    us_.kv_len_dev = (int*)own(nb * sizeof(int));
    static_assert(sizeof(int) == sizeof(float), "one buffer serves both forms of the timesteps");
    int* t_dev = (int*)own(S * sizeof(int));
    SDMI_HIP(hipMemcpyAsync(us_.kv_len_dev, us_.kv_len_host.data(), nb * sizeof(int), hipMemcpyHostToDevice, stream_));
    SDMI_HIP(hipMemcpyAsync(t_dev, ti ? (const void*)ti : (const void*)tf, S * sizeof(int), hipMemcpyHostToDevice, stream_));
    SDMI_HIP(hipStreamSynchronize(stream_));  // host vectors may go away; once per call, outside the step loop

    // the time embedding and everything made from it are fp32 at every precision
    Buf te_buf(this, (size_t)S * mc * 4), e1_buf(this, (size_t)S * ed * 4), e2_buf(this, (size_t)S * ed * 4);
    const Act te = rows_view(te_buf.p, S, mc, 0), e1 = rows_view(e1_buf.p, S, ed, 0), e2 = rows_view(e2_buf.p, S, ed, 0);
    SDMI_LAUNCH(ti ? launch_timestep_embedding(t_dev, S, mc, te.p, stream_) : launch_timestep_embedding_f(reinterpret_cast<const float*>(t_dev), S, mc, te.p, stream_));
    auto time_mlp = [&](const LinW& l1, const LinW& l2) {   // e2 = SiLU(emb), shared by all ResBlocks
        linear(l1, te, e1);
        SDMI_LAUNCH(launch_silu(e1.p, e1.p, (long long)S * ed, stream_));
        linear(l2, e1, e2);
        SDMI_LAUNCH(launch_silu(e2.p, e2.p, (long long)S * ed, stream_));
    };
    auto embed_rows = [&](size_t i) {   // ResBlock i's Linear(SiLU(emb)) for every step
        const ResW& r = *res_list_[i];
        us_.temb[i] = (float*)own((size_t)S * r.cout * 4);
        linear(r.lin_embed, e2, rows_view(us_.temb[i], S, r.cout, 0));
    };
    time_mlp(lin1_time_, lin2_time_);
    // (the ControlNet's blocks follow the UNet's in res_list_ / st_list_: their rows exist in a controlled call only)
    const size_t n_res = ctrl ? res_list_.size() : n_res_unet_, n_st = ctrl ? st_list_.size() : n_st_unet_;
    us_.temb.resize(n_res);
    for (size_t i = 0; i < n_res_unet_; ++i) embed_rows(i);
    if (ctrl) {   // the ControlNet has a time MLP of its own (cldm.py: self.time_embed)
        time_mlp(ctl_lin1_time_, ctl_lin2_time_);
        for (size_t i = n_res_unet_; i < n_res; ++i) embed_rows(i);
    }
    us_.kc.resize(n_st);
    us_.vc.resize(n_st);
    const long long ctx_rows = (long long)nb * t_max;
    Act ctx = rows_view(ctx_packed, ctx_rows, cd, 0);  // text context in the engine's storage type
    Buf ctx_h(this, bf16_ ? (size_t)ctx_rows * cd * 2 : 256);
    if (bf16_) {
        SDMI_LAUNCH(launch_f32_to_bf16(ctx_packed, ctx_h.p, ctx_rows * cd, stream_));
        ctx = rows_view(ctx_h.p, ctx_rows, cd, 1);
    }
    for (size_t i = 0; i < n_st; ++i) {
        const SpatialW& s = *st_list_[i];
        us_.kc[i] = (float*)own((size_t)ctx_rows * s.c * esz());
        us_.vc[i] = (float*)own((size_t)ctx_rows * s.c * esz());
        linear(s.attn2.k, ctx, rows_view(us_.kc[i], ctx_rows, s.c, edt()));
        linear(s.attn2.v, ctx, rows_view(us_.vc[i], ctx_rows, s.c, edt()));
    }
    // an adapted call (IP-Adapter): K_ip / V_ip of the nb batch rows are made by the first step inside the window (unet_run), so a call without one runs the plain launches
    us_.ip_want = ip_.set && ip_.scale != 0.f && n_images > 0;
    us_.n_images = n_images;
    if (ctrl) {
        // the hint embedding, once per call: n_hint pictures through the eight hint convolutions, then laid out as the residual of the control encoder's first
        // convolution -- one block of h w rows per batch row, image i of either CFG half reading hint i mod n_hint (device copies, no launch)
        Act emb = control_hint_embed(ctrl_.hint_dev, ctrl_.n_hint, ctrl_.hint_h, ctrl_.hint_w);
        const size_t per = (size_t)lat_h_ * lat_w_ * mc;
        us_.hint_rows = (float*)own((size_t)nb * per * 4);
        for (int b = 0; b < nb; ++b)
            SDMI_HIP(hipMemcpyAsync(us_.hint_rows + (size_t)b * per, emb.p + (size_t)((b % n_images) % ctrl_.n_hint) * per, per * 4, hipMemcpyDeviceToDevice, stream_));
        release(emb);
        us_.ctrl = true;
        us_.ctrl_window = window;
    }
}

// ---- ControlNet (include/sdmi.h "ControlNet") ------------------------------------------------------------------------
void Engine::check_control(const sdmi_control& c) {
    if (!c.hint_rgb) throw Error(SDMI_ERR_INVALID, "control: null hint");
    if (c.n_hint < 1) throw Error(SDMI_ERR_INVALID, "control: n_hint must be at least 1");
    if (c.hint_h < 64 || c.hint_w < 64 || c.hint_h % 64 || c.hint_w % 64) throw Error(SDMI_ERR_INVALID, "control: hint_h / hint_w must be 8 x a latent size (positive multiples of 64)");
    if (!std::isfinite(c.strength)) throw Error(SDMI_ERR_INVALID, "control: strength must be finite");
    if ((unsigned long long)c.n_hint * (unsigned long long)c.hint_h * (unsigned long long)c.hint_w * 3ull > (1ull << 32))
        throw Error(SDMI_ERR_UNSUPPORTED, "control: more than 4 GiB of hint pictures");
    if (!(c.start >= 0.0 && c.start <= c.end && c.end <= 1.0)) throw Error(SDMI_ERR_INVALID, "control: the step window must satisfy 0 <= start <= end <= 1");
}

void Engine::set_control(const sdmi_control* c) {
    if (!has_control()) throw Error(SDMI_ERR_STATE, "set_control: this context has no ControlNet (sdmi_config.control_hint_ch = 0)");
    SDMI_HIP(hipSetDevice(cfg_.device));
    if (!c) {
        SDMI_HIP(hipStreamSynchronize(stream_));
        if (ctrl_.hint_dev) (void)hipFree(ctrl_.hint_dev);
        ctrl_ = Control{};
        return;
    }
    if (!control_ready()) throw Error(SDMI_ERR_STATE, "set_control: the ControlNet weights (controlnet/...) are not loaded");
    check_control(*c);
    const size_t bytes = (size_t)c->n_hint * c->hint_h * c->hint_w * 3;
    uint8_t* d = nullptr;
    SDMI_HIP(hipMalloc((void**)&d, bytes));
    hipError_t err = hipMemcpy(d, c->hint_rgb, bytes, hipMemcpyHostToDevice);
    if (err != hipSuccess) { (void)hipFree(d); SDMI_HIP(err); }
    SDMI_HIP(hipStreamSynchronize(stream_));
    if (ctrl_.hint_dev) (void)hipFree(ctrl_.hint_dev);
    ctrl_.set = true; ctrl_.hint_dev = d; ctrl_.hint_bytes = bytes;
    ctrl_.n_hint = c->n_hint; ctrl_.hint_h = c->hint_h; ctrl_.hint_w = c->hint_w;
    ctrl_.strength = c->strength; ctrl_.start = c->start; ctrl_.end = c->end;
}

// input_hint_block (cldm.py): eight 3x3 convolutions, SiLU after all but the last, fp32 at every precision.  u8 -> v / 255 with a zero 4th channel first.
// ---- FreeU (include/sdmi.h "FreeU") ------------------------------------------------------------------------------------
// THE block rule: keyed on the channel count of the backbone tensor entering output block i, as ComfyUI's FreeU nodes ship it (not on the resolution)
void Engine::freeu_plan(int model_channels, int latent_h, int latent_w, int (&out)[60]) {
    if (model_channels < 1) throw Error(SDMI_ERR_INVALID, "freeu_plan: model_channels must be positive");
    check_latent_size(latent_h, latent_w);
    const int c1 = model_channels, c2 = 2 * c1, c4 = 4 * c1;
    const int cx[12] = {c4, c4, c4, c4, c4, c4, c4, c2, c2, c2, c1, c1};          // what the block below (or the middle block) hands up
    const int cskip[12] = {c4, c4, c4, c4, c4, c2, c2, c2, c1, c1, c1, c1};       // what input block 11 - i saved
    for (int i = 0; i < 12; ++i) {
        const int level = 3 - i / 3;   // down-convolutions between the latent and the block's input (stride 2, pad 1: the size is halved, rounded up)
        int h = latent_h, w = latent_w;
        for (int l = 0; l < level; ++l) { h = (h + 1) / 2; w = (w + 1) / 2; }
        int* o = out + 5 * i;
        o[0] = cx[i] == c4 ? 1 : cx[i] == c2 ? 2 : 0;
        o[1] = cx[i]; o[2] = cskip[i]; o[3] = h; o[4] = w;
    }
}

void Engine::check_freeu(const FreeU& f) {
    if (f.version < 0 || f.version > 2) throw Error(SDMI_ERR_INVALID, "freeu: version must be 0 (off), 1 or 2");
    if (!f.version) return;
    for (float v : {f.b1, f.b2, f.s1, f.s2})
        if (!std::isfinite(v)) throw Error(SDMI_ERR_INVALID, "freeu: b1, b2, s1, s2 must be finite");
    if (!(f.b1 > 0.f && f.b2 > 0.f)) throw Error(SDMI_ERR_INVALID, "freeu: b1 and b2 must be positive");
    if (!(f.s1 >= 0.f && f.s2 >= 0.f)) throw Error(SDMI_ERR_INVALID, "freeu: s1 and s2 must not be negative");
    if (!(f.start >= 0.0 && f.start <= f.end && f.end <= 1.0)) throw Error(SDMI_ERR_INVALID, "freeu: the step window must satisfy 0 <= start <= end <= 1");
}

void Engine::set_freeu(const FreeU& f) {
    check_freeu(f);
    if (!f.version) { freeu_ = FreeU{}; return; }
    int plan[60];
    freeu_plan(cfg_.model_channels, lat_h_, lat_w_, plan);
    const int g = freeu_granule();
    for (int i = 0; i < 12; ++i)
        if (plan[5 * i] && (plan[5 * i + 1] % (2 * g) || plan[5 * i + 2] % g))
            throw Error(SDMI_ERR_UNSUPPORTED, "freeu: output block " + std::to_string(i) + " joins " + std::to_string(plan[5 * i + 1]) + " backbone and " + std::to_string(plan[5 * i + 2]) +
                                                  " skip channels; the kernels take half the former and the latter in multiples of " + std::to_string(g));
    freeu_ = f;
}

void Engine::freeu_filter(const Act* const* cats, const int* cx, const float* s, int n_cats) {
    FreeuFilter ff{};
    ff.dt = edt();
    double bytes = 0;
    int planes = 0;
    for (int i = 0; i < n_cats; ++i) {
        if (s[i] == 1.0f) continue;
        if (ff.n_seg == kFreeuMaxSegs) throw Error(SDMI_ERR_STATE, "freeu: more filtered skips than the segment table holds");
        const Act hs = slice(*cats[i], cx[i], cats[i]->c - cx[i]);
        if (!hs.p || hs.dt != edt() || hs.c % freeu_granule()) throw Error(SDMI_ERR_STATE, "freeu: a skip does not have the form the filter takes");
        FreeuSeg& g = ff.seg[ff.n_seg++];
        g.y = hs.p; g.y3 = hs.p3; g.n = hs.n; g.h = hs.h; g.w = hs.w; g.c = hs.c; g.ld = hs.stride(); g.ld3 = hs.ld3; g.k = s[i] - 1.0f;
        planes += g.y3 ? 1 : 0;
        bytes += (double)hs.rows() * hs.c * (edt() ? 6.0 : (g.y3 ? 18.0 : 12.0));   // read twice (the second time from L2), written once in every form
    }
    if (!ff.n_seg) return;
    if (record_shapes_) ++choice_counts_["freeu_filter segs=" + std::to_string(ff.n_seg) + " planes=" + std::to_string(planes) + " dt=" + std::to_string(ff.dt)];
    { ProfScope ps_o(this, PC_OTHER, 0, bytes); ps_o.set_tag("freeu_filter"); SDMI_LAUNCH_IN(ps_o, 0, launch_freeu_filter(ff, stream_)); }
}

void Engine::freeu_backbone(const Act& cat, int cx, float b, int version) {
    if (b == 1.0f) return;
    const Act h = slice(cat, 0, cx / 2);
    if (!h.p || h.dt != edt() || cx % 2 || h.c % freeu_granule()) throw Error(SDMI_ERR_STATE, "freeu: a backbone tensor does not have the form the kernel takes");
    FreeuBackbone a{};
    a.y = h.p; a.y3 = h.p3; a.n = h.n; a.hw = h.h * h.w; a.c = h.c; a.ld = h.stride(); a.ld3 = h.ld3; a.dt = edt(); a.version = version; a.b = b;
    if (record_shapes_)
        ++choice_counts_["freeu_backbone v" + std::to_string(version) + " rows=" + std::to_string(h.rows()) + " c=" + std::to_string(h.c) + " cx=" + std::to_string(cx) +
                         " planes=" + std::to_string(a.y3 ? 1 : 0) + " dt=" + std::to_string(a.dt)];
    const double es = edt() ? 2.0 : 4.0;
    std::unique_ptr<Buf> mean;
    if (version == 2) {
        mean.reset(new Buf(this, (size_t)h.rows() * sizeof(float)));
        { ProfScope ps_o(this, PC_OTHER, 0, (double)h.rows() * (cx * es + 4.0)); ps_o.set_tag("freeu_mean");
          SDMI_LAUNCH_IN(ps_o, 0, launch_freeu_mean(cat.p, mean->f(), h.rows(), cx, cat.stride(), edt(), stream_)); }
        a.mean = mean->f();
    }
    { ProfScope ps_o(this, PC_OTHER, 0, (double)h.rows() * h.c * (edt() ? 4.0 : (a.y3 ? 14.0 : 8.0))); ps_o.set_tag("freeu_backbone");
      SDMI_LAUNCH_IN(ps_o, 0, launch_freeu_backbone(a, stream_)); }
}

Act Engine::control_hint_embed(const uint8_t* hint_rgb_dev, int n, int hint_h, int hint_w) {
    Range rng(this, "ControlNet hint");
    // one picture at a time, like the VAE encoder (encode_image_dev): the launches of a picture -- tiles, split-K, summation order -- do not depend on how many hints the
    // call has, so n_hint = 1 and the same hint given n times are the same bits
    Act emb = new_act(n, hint_h / 8, hint_w / 8, ctl_hint_[7].cout, /*dt=*/0);
    const size_t per = (size_t)emb.h * emb.w * emb.c;
    for (int img = 0; img < n; ++img) {
        Act x = new_act(1, hint_h, hint_w, 4, /*dt=*/0);
        { ProfScope ps_o(this, PC_OTHER, 0, (double)x.rows() * 19.0); SDMI_LAUNCH_IN(ps_o, 0, launch_hint_u8_to_nhwc4(hint_rgb_dev + (size_t)img * hint_h * hint_w * 3, x.p, x.rows(), stream_)); }
        for (int i = 0; i < 8; ++i) {
            const ConvW& w = ctl_hint_[i];
            const int stride = (i == 2 || i == 4 || i == 6) ? 2 : 1;
            Act y;
            if (i == 7) { y = emb; y.n = 1; y.p = emb.p + (size_t)img * per; y.view = true; }
            else y = new_act(1, x.h / stride, x.w / stride, w.cout, /*dt=*/0);
            conv(w, x, y, stride, 0, nullptr, 0, nullptr);
            release(x);
            if (i != 7) {
                ProfScope ps_o(this, PC_OTHER, 0, (double)y.rows() * y.c * 8.0);
                SDMI_LAUNCH_IN(ps_o, 0, launch_silu(y.p, y.p, y.rows() * y.c, stream_));
            }
            x = y;
        }
    }
    return emb;
}

// The control encoder on the UNet's own assembled input: block 0's convolution takes the hint embedding as its GEMM residual, blocks 1 - 11 and the middle block
// follow, and behind block j zero_convs/j writes r[j] (middle_block_out: r[12]), dense, in the engine's activation type.  Both halves of a CFG batch are computed.
void Engine::control_run(const float* x_nhwc, int nb, int step, Act (&r)[13]) {
    Range rng(this, "ControlNet::forward step " + std::to_string(step));
    Act x; x.p = const_cast<float*>(x_nhwc); x.n = nb; x.h = lat_h_; x.w = lat_w_; x.c = ctl_blocks_[0].conv.cin; x.dt = 0;
    Act prev{};
    for (int j = 0; j < 12; ++j) {
        const UBlock& b = ctl_blocks_[j];
        Range rb(this, "control input_block " + std::to_string(j));
        const int ho = b.kind == BK_DOWN ? x.h / 2 : x.h, wo = b.kind == BK_DOWN ? x.w / 2 : x.w;
        Act y = new_act(nb, ho, wo, b.cout);
        if (j == 0) {
            Act hint; hint.p = us_.hint_rows; hint.n = nb; hint.h = ho; hint.w = wo; hint.c = b.cout; hint.dt = 0; hint.view = true;
            conv(b.conv, x, y, 1, 0, nullptr, 0, &hint);   // (precision >= 1: an fp32 -> bf16 layer, the fp32 embedding is added in front of the rounding)
        } else {
            run_block(b, x, y, step);
        }
        if (prev.p) release(prev);
        r[j] = new_act(nb, ho, wo, b.cout);
        conv(ctl_zero_[j], y, r[j], 1, 0, nullptr, 0, nullptr);
        prev = y;
        x = y;
    }
    Act a = new_act(x.n, x.h, x.w, ctl_mid_res1_.cout); res_block(ctl_mid_res1_, x, a, step);
    release(prev);
    Act b = new_act(a.n, a.h, a.w, ctl_mid_st_.c); spatial_transformer(ctl_mid_st_, a, b); release(a);
    Act c = new_act(b.n, b.h, b.w, ctl_mid_res2_.cout); res_block(ctl_mid_res2_, b, c, step); release(b);
    r[12] = new_act(c.n, c.h, c.w, ctl_mid_out_.cout);
    conv(ctl_mid_out_, c, r[12], 1, 0, nullptr, 0, nullptr);
    release(c);
}

void Engine::control_hint_embed_dev(const uint8_t* hint_rgb, int n, int hint_h, int hint_w, float* out_nchw) {
    if (!has_control()) throw Error(SDMI_ERR_STATE, "control_hint_embed: this context has no ControlNet (sdmi_config.control_hint_ch = 0)");
    if (!control_ready()) throw Error(SDMI_ERR_STATE, "control_hint_embed: the ControlNet weights (controlnet/...) are not loaded");
    if (n < 1 || hint_h < 64 || hint_w < 64 || hint_h % 64 || hint_w % 64) throw Error(SDMI_ERR_INVALID, "control_hint_embed: n >= 1, hint_h / hint_w positive multiples of 64");
    check_batch(n);
    Act emb = control_hint_embed(hint_rgb, n, hint_h, hint_w);
    SDMI_LAUNCH(launch_nhwc_to_nchw(emb.p, out_nchw, n, emb.c, emb.h, emb.w, stream_));
    release(emb);
}

size_t Engine::control_residual_elems(int n) const {
    size_t total = 0;
    int h = lat_h_, w = lat_w_;
    for (const UBlock& b : ctl_blocks_) {
        if (b.kind == BK_DOWN) { h /= 2; w /= 2; }
        total += (size_t)n * b.cout * h * w;
    }
    return total + (size_t)n * ctl_mid_out_.cout * h * w;
}

void Engine::control_residuals_dev(const float* x_nchw, int t, const float* context, int n, int T, float* out) {
    if (!finalized_) throw Error(SDMI_ERR_STATE, "weights not finalized");
    if (!has_control()) throw Error(SDMI_ERR_STATE, "control_residuals: this context has no ControlNet (sdmi_config.control_hint_ch = 0)");
    if (!ctrl_.set) throw Error(SDMI_ERR_STATE, "control_residuals: no control is set (sdmi_set_control)");
    if (n <= 0 || T <= 0) throw Error(SDMI_ERR_INVALID, "control_residuals: n and T must be positive");
    check_batch(n);
    const int H = lat_h_, W = lat_w_;
    std::vector<int> kv(n, T), ts(1, t);
    unet_prepare(context, n, T, kv.data(), ts, n, /*window=*/false, /*force_control=*/true);
    Buf xin(this, (size_t)n * H * W * 4 * 4);
    SDMI_LAUNCH(launch_nchw_to_nhwc(x_nchw, xin.f(), n, 4, H, W, 1.0f, stream_));
    Act r[13];
    control_run(xin.f(), n, 0, r);
    size_t off = 0;
    for (auto& a : r) {
        if (a.dt) { SDMI_HIP(launch_nhwc_bf16_to_nchw_f32(a.p, out + off, a.n, a.c, a.h, a.w, stream_)); count_kernel(); }   // (outside the profile, counted)
        else SDMI_LAUNCH(launch_nhwc_to_nchw(a.p, out + off, a.n, a.c, a.h, a.w, stream_));
        off += (size_t)a.rows() * a.c;
        release(a);
    }
    unet_release();
}

void Engine::run_block(const UBlock& b, const Act& in, Act& y, int step) {
    switch (b.kind) {
        case BK_CONV: conv(b.conv, in, y, 1, 0, nullptr, 0, nullptr); return;
        case BK_DOWN: conv_raw(b.conv, in, y, 2, 0); return;
        case BK_RES: res_block(b.res, in, y, step); return;
        case BK_RES_ST: {
            Act r = new_act(in.n, in.h, in.w, b.cout); res_block(b.res, in, r, step);
            spatial_transformer(b.st, r, y); release(r); return;
        }
        case BK_RES_UP: {   // (fp32 engine: the tensor between the block and its up-convolution exists only as planes)
            Act r = plane_gemm(b.cout, b.cout) ? new_act3(in.n, in.h, in.w, b.cout, 2) : new_act(in.n, in.h, in.w, b.cout);
            res_block(b.res, in, r, step);
            conv_raw(b.up, r, y, 1, 1); release(r); return;
        }
        case BK_RES_ST_UP: {
            Act r = new_act(in.n, in.h, in.w, b.cout); res_block(b.res, in, r, step);
            Act s = plane_gemm(b.cout, b.cout) ? new_act3(in.n, in.h, in.w, b.cout, 2) : new_act(in.n, in.h, in.w, b.cout);
            spatial_transformer(b.st, r, s); release(r);
            conv_raw(b.up, s, y, 1, 1); release(s); return;
        }
    }
    throw Error(SDMI_ERR_STATE, "bad block kind");
}

// UNet::forward (unet/mod.rs:109-143) on NHWC activations.
// Tensor::cat(vec![x, saved_inputs.pop()], 1) (unet/mod.rs:134) is not a copy here: the input buffer `cats[i]` of
// output block i ([x channels | skip channels]) is allocated when its skip is produced on the way down; input block
// 11 - i writes its result straight into the skip slice (the GEMM epilogue's row stride), output block i - 1 (or
// the middle block) writes the x slice, and output block i reads the whole buffer.
void Engine::unet_run(const float* x_nhwc, int nb, int step, float* out_nhwc, bool cfg_pair) {
    Range rng(this, "UNet::forward step " + std::to_string(step));
    const int H = lat_h_, W = lat_w_;
    // latents stay fp32; a conditioned model (unet_in_ch > 4) reads the assembled [latent | cond | pad] rows of launch_assemble_unet_in
    Act x; x.p = const_cast<float*>(x_nhwc); x.n = nb; x.h = H; x.w = W; x.c = in_blocks_[0].conv.cin; x.dt = 0;

    // a controlled step: the control encoder runs first, on the same input; its residuals wait in r[] until the skips exist
    const bool controlled = control_on(step);
    Act ctl_r[13];
    if (controlled) control_run(x_nhwc, nb, step, ctl_r);
    // an adapted step (IP-Adapter): the UNet's own cross attentions add the image term (spatial_transformer); the control encoder above does not
    struct IpLive { bool& f; ~IpLive() { f = false; } } ip_guard{ip_live_};
    ip_live_ = ip_on(step);
    if (ip_live_ && us_.kip.empty()) {
        if (nb != us_.nb) throw Error(SDMI_ERR_STATE, "ip_adapter: batch mismatch");
        ip_prepare(nb, us_.n_images, [&](size_t bytes) { void* p = pool_.alloc(bytes); us_.owned.push_back(p); return p; });
    }

    const int nblk = (int)in_blocks_.size();
    // a FreeU step: which output blocks take which pair of parameters is freeu_plan's to say; nothing below runs when none is left
    const bool freeu = freeu_on(step);
    int fplan[60];
    if (freeu) {
        if (nblk != 12) throw Error(SDMI_ERR_STATE, "freeu: the block rule is stated for 12 output blocks");
        if (!freeu_filter_size_ok(H, W)) throw Error(SDMI_ERR_UNSUPPORTED, "freeu: the latent size in force is beyond what the filter kernel's tables hold");
        freeu_plan(cfg_.model_channels, H, W, fplan);
    }
    std::vector<Act> cats(nblk);
    for (int j = 0; j < nblk; ++j) {
        const UBlock& b = in_blocks_[j];
        Range rb(this, "input_block " + std::to_string(j));
        const int i = nblk - 1 - j;   // the output block that pops this skip (saved_inputs is a stack, unet/mod.rs:126,134)
        const int ctot = out_blocks_[i].cin, cskip = b.cout, cx = ctot - cskip;
        if (cx <= 0) throw Error(SDMI_ERR_STATE, "unet: block table inconsistent");
        const int ho = b.kind == BK_DOWN ? x.h / 2 : x.h, wo = b.kind == BK_DOWN ? x.w / 2 : x.w;
        // fp32 engine: the buffer also exists as planes -- the skip convolution of output block i (cin != cout) and the down-convolutions read those,
        // written by the epilogues (or split-K reduce kernels) of the GEMMs that produce the two halves
        const bool catp = plane_gemm(ctot, out_blocks_[i].cout) && cx % 32 == 0 && cskip % 32 == 0;
        cats[i] = catp ? new_act3(nb, ho, wo, ctot, 3) : new_act(nb, ho, wo, ctot);
        Act y = slice(cats[i], cx, cskip);
        if (cfg_pair && j == 1 && b.kind == BK_RES_ST && nb % 2 == 0) {
            // The two halves of a CFG step's batch -- uncond rows, then cond rows (stablediffusion/mod.rs:173-179: two forwards of the SAME x and t) -- are identical
            // until the text context first enters: conv_in, this block's ResBlock and its transformer up to the cross attention.  That prefix is computed ONCE on
            // the first half and duplicated in front of the cross attention (spatial_transformer): the same values the two forwards would produce, per sample
            // (GroupNorm and attention are per sample), for half the 64x64-level ResBlock convolutions and one of its five self-attentions less.  Option cfg_share=0
            // computes both halves.
            Act xh = x; xh.n = nb / 2;
            Act r = new_act(nb / 2, x.h, x.w, b.cout);
            res_block(b.res, xh, r, step);
            spatial_transformer(b.st, r, y);
            release(r);
        } else {
            run_block(b, x, y, step);
        }
        x = y;
    }
    {   // middle block: reads the last skip, writes the x slice of output block 0's input
        Act a = new_act(x.n, x.h, x.w, mid_res1_.cout); res_block(mid_res1_, x, a, step);
        Act b = new_act(x.n, x.h, x.w, mid_st_.c); spatial_transformer(mid_st_, a, b); release(a);
        Act c = slice(cats[0], 0, cats[0].c - x.c);
        if (c.c != mid_res2_.cout) throw Error(SDMI_ERR_STATE, "unet: middle block width mismatch");
        res_block(mid_res2_, b, c, step); release(b);
    }
    if (controlled) {
        // ControlNet adds to the SAVED copies only: the encoder above ran on the unmodified activations, the output blocks below read the sums.  One launch for
        // the 12 skip slices (input block j's skip lives in cats[11 - j]) and the middle block's output (the x slice of cats[0]), in every form they exist in.
        ControlAdd ca{};
        ca.n_seg = 13; ca.dt = edt(); ca.strength = (float)ctrl_.strength;
        double bytes = 0;
        for (int j = 0; j < 13; ++j) {
            const Act& cat = cats[j < 12 ? nblk - 1 - j : 0];
            const Act dst = j < 12 ? slice(cat, cat.c - ctl_r[j].c, ctl_r[j].c) : slice(cat, 0, ctl_r[j].c);
            if (!dst.p || dst.dt != ctl_r[j].dt || dst.rows() != ctl_r[j].rows()) throw Error(SDMI_ERR_STATE, "control: a residual does not match its skip");
            ControlSeg& g = ca.seg[j];
            g.y = dst.p; g.r = ctl_r[j].p; g.y3 = dst.p3; g.rows = dst.rows(); g.c = dst.c; g.ld = dst.stride(); g.ld3 = dst.ld3;
            bytes += (double)g.rows * g.c * (edt() ? 6.0 : (g.y3 ? 18.0 : 12.0));
        }
        if (record_shapes_) {   // option dump_choices: how many of the segments also carry planes
            int planes = 0;
            for (int j = 0; j < ca.n_seg; ++j) planes += ca.seg[j].y3 ? 1 : 0;
            ++choice_counts_["control_add segs=" + std::to_string(ca.n_seg) + " planes=" + std::to_string(planes) + " dt=" + std::to_string(ca.dt)];
        }
        { ProfScope ps_o(this, PC_OTHER, 0, bytes); ps_o.set_tag("control_add"); SDMI_LAUNCH_IN(ps_o, 0, launch_control_add(ca, stream_)); }
        for (auto& a : ctl_r) release(a);
    }
    if (freeu) {
        // every affected skip exists now (with the control's residuals in it): ONE launch filters them all.  The backbone halves follow block by block below.
        const Act* fc[12]; int fcx[12]; float fs[12];
        for (int i = 0; i < nblk; ++i) {
            const int* pl = fplan + 5 * i;
            if (pl[0] && (cats[i].c != pl[1] + pl[2] || cats[i].h != pl[3] || cats[i].w != pl[4])) throw Error(SDMI_ERR_STATE, "freeu: the block plan does not match the model");
            fc[i] = &cats[i]; fcx[i] = pl[1]; fs[i] = pl[0] == 1 ? freeu_.s1 : pl[0] == 2 ? freeu_.s2 : 1.0f;
        }
        freeu_filter(fc, fcx, fs, nblk);
    }
    Act last{};
    for (int i = 0; i < nblk; ++i) {
        const UBlock& b = out_blocks_[i];
        Range rb(this, "output_block " + std::to_string(i));
        if (freeu && fplan[5 * i]) freeu_backbone(cats[i], fplan[5 * i + 1], fplan[5 * i] == 1 ? freeu_.b1 : freeu_.b2, freeu_.version);
        const bool up = b.kind == BK_RES_UP || b.kind == BK_RES_ST_UP;
        Act y;
        if (i + 1 < nblk) {
            y = slice(cats[i + 1], 0, cats[i + 1].c - in_blocks_[nblk - 2 - i].cout);
            if (y.c != b.cout || y.h != (cats[i].h << (up ? 1 : 0))) throw Error(SDMI_ERR_STATE, "unet: output block shape mismatch");
        } else {
            y = new_act(nb, cats[i].h << (up ? 1 : 0), cats[i].w << (up ? 1 : 0), b.cout);
            last = y;
        }
        run_block(b, cats[i], y, step);
        release(cats[i]);
    }
    Act gn = new_act(last.n, last.h, last.w, last.c);
    group_norm(unet_norm_out_, last, gn, true);
    release(last);
    Act out; out.p = out_nhwc; out.n = nb; out.h = H; out.w = W; out.c = 4; out.dt = 0;  // eps stays fp32
    conv(unet_conv_out_, gn, out, 1, 0, nullptr, 0, nullptr);
    release(gn);
}

// CLIP::forward (clip/mod.rs:56-75) with ResidualDecoderAttentionBlock (:110-114), MultiHeadSelfAttention
// (:158-180), MLP + QuickGELU (:207-226) and attn_decoder_mask (backend.rs:130-139).  fp32 in both precisions.
void Engine::clip_forward_dev(const int32_t* tokens, int n, int T, float* out) { clip_forward_dev(tokens, nullptr, nullptr, n, T, 1, out); }

void Engine::clip_forward_dev(const int32_t* tokens, const int32_t* emb_row, const float* weights, int n, int T, int clip_skip, float* out) {
    if (!finalized_) throw Error(SDMI_ERR_STATE, "weights not finalized");
    if (!clip_ready_) throw Error(SDMI_ERR_STATE, "CLIP weights are not loaded (clip/... tensors; clip_layers > 0 in the config)");
    if (n <= 0 || T <= 0) throw Error(SDMI_ERR_INVALID, "clip_forward: n and seq_len must be positive");
    if (T > cfg_.clip_ctx) throw Error(SDMI_ERR_INVALID, "clip_forward: sequence longer than n_ctx");  // reference: slice panics
    if (clip_skip < 1 || clip_skip > cfg_.clip_layers)
        throw Error(SDMI_ERR_INVALID, "clip_forward: clip_skip must be 1 .. clip_layers = " + std::to_string(cfg_.clip_layers) + ", got " + std::to_string(clip_skip));
    if (emb_row && !emb_bank_) throw Error(SDMI_ERR_INVALID, "clip_forward: embedding rows given, but the context has no embeddings");
    const int C = cfg_.ctx_dim, H = cfg_.clip_heads;
    const long long M = (long long)n * T;
    Act x = new_rows(M, C, 1, 0), h = new_rows(M, C, 1, 0), qkv = new_rows(M, 3 * C, 1, 0), a = new_rows(M, C, 1, 0), f = new_rows(M, 4 * C, 1, 0);
    Act mask = new_rows(T, T, 1, 0);
    if (emb_row) SDMI_LAUNCH(launch_clip_embed_bank(tokens, emb_row, clip_tok_, emb_bank_, clip_pos_, x.p, n, T, C, stream_));
    else SDMI_LAUNCH(launch_clip_embed(tokens, clip_tok_, clip_pos_, x.p, n, T, C, stream_));
    SDMI_LAUNCH(launch_causal_mask(mask.p, T, stream_));
    Attn at;
    attn_packed_qkv(qkv, T, at); at.o = attn_rows(a, T);
    at.n = n; at.nq = T; at.nk = T; at.n_head = H; at.d_head = C / H;
    at.mask = mask.p; at.mask_ld = T; at.dt = 0;
    const int n_blocks = cfg_.clip_layers - clip_skip + 1;   // the web UI's "CLIP skip s": hidden_states[-s] through the final LayerNorm
    for (int bi = 0; bi < n_blocks; ++bi) {
        const ClipBlockW& b = clip_blocks_[bi];
        layer_norm(b.attn_ln, x, h);
        linear(b.q, h, qkv);         // query | key | value, one GEMM
        attention(at);
        linear(b.out, a, x, &x);     // x += out(attn)
        layer_norm(b.mlp_ln, x, h);
        linear(b.fc1, h, f);
        SDMI_LAUNCH(cfg_.variant == 1 ? launch_gelu_erf(f.p, M * 4 * C, stream_) : launch_quick_gelu(f.p, M * 4 * C, stream_));
        linear(b.fc2, f, x, &x);     // x += fc2(gelu(fc1))
    }
    layer_norm(clip_ln_, x, rows_view(out, M, C, 0));
    if (weights) {
        ProfScope ps(this, PC_OTHER, 0, (double)M * C * 12.0);
        ps.set_tag("clip_reweight");
        SDMI_LAUNCH_IN(ps, 0, launch_clip_reweight(out, weights, n, T, C, stream_));
    }
    release(mask); release(f); release(a); release(qkv); release(h); release(x);
}

// ---- textual-inversion embeddings (include/sdmi.h "web-UI prompt encoding") ------------------------------------------------
// The bank is one allocation of exactly the rows in use: adding or removing an embedding builds the new bank beside the old one and swaps.  These are
// rare, blocking calls; no forward is in flight when they return.
void Engine::embedding_add(const std::string& name, const std::vector<int32_t>& ids, const float* vectors, int n_vectors, bool on_device) {
    if (cfg_.clip_layers <= 0) throw Error(SDMI_ERR_STATE, "embedding_add: this context has no text encoder (clip_layers = 0)");
    if (name.empty() || name.find_first_of("\t\n") != std::string::npos) throw Error(SDMI_ERR_INVALID, "embedding_add: the name must not be empty or hold a tab or a newline");
    if (ids.empty()) throw Error(SDMI_ERR_INVALID, "embedding_add: the tokenizer gives the name '" + name + "' no tokens");
    if (!vectors) throw Error(SDMI_ERR_INVALID, "embedding_add: null vectors");
    const int L = cfg_.clip_ctx - 2;
    if (n_vectors < 1 || n_vectors > L)
        throw Error(SDMI_ERR_INVALID, "embedding_add: '" + name + "' has " + std::to_string(n_vectors) + " vectors; 1 .. clip_ctx - 2 = " + std::to_string(L) + " fit a chunk");
    for (const Embedding& e : embeddings_)
        if (e.name == name) throw Error(SDMI_ERR_INVALID, "embedding_add: the context already has an embedding named '" + name + "'");
    SDMI_HIP(hipSetDevice(cfg_.device));
    const size_t row = (size_t)cfg_.ctx_dim * sizeof(float);
    float* bank = nullptr;
    SDMI_HIP(hipMalloc(reinterpret_cast<void**>(&bank), (size_t)(emb_rows_ + n_vectors) * row));
    hipError_t st = hipSuccess;
    if (emb_rows_) st = hipMemcpyAsync(bank, emb_bank_, (size_t)emb_rows_ * row, hipMemcpyDeviceToDevice, stream_);
    if (st == hipSuccess)
        st = hipMemcpyAsync(bank + (size_t)emb_rows_ * cfg_.ctx_dim, vectors, (size_t)n_vectors * row, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream_);
    if (st == hipSuccess) st = hipStreamSynchronize(stream_);
    if (st != hipSuccess) { (void)hipFree(bank); SDMI_HIP(st); }
    if (emb_bank_) (void)hipFree(emb_bank_);
    emb_bank_ = bank;
    emb_rows_ += n_vectors;
    embeddings_.push_back(Embedding{name, ids, n_vectors});
}

void Engine::embedding_remove(const std::string& name) {
    size_t at = 0;
    int first = 0;
    while (at < embeddings_.size() && embeddings_[at].name != name) first += embeddings_[at++].n_vectors;
    if (at == embeddings_.size()) throw Error(SDMI_ERR_INVALID, "embedding_remove: the context has no embedding named '" + name + "'");
    SDMI_HIP(hipSetDevice(cfg_.device));
    SDMI_HIP(hipStreamSynchronize(stream_));
    const int v = embeddings_[at].n_vectors, after = emb_rows_ - first - v;
    const size_t row = (size_t)cfg_.ctx_dim * sizeof(float);
    float* bank = nullptr;
    if (emb_rows_ - v > 0) {
        SDMI_HIP(hipMalloc(reinterpret_cast<void**>(&bank), (size_t)(emb_rows_ - v) * row));
        hipError_t st = hipSuccess;
        if (first) st = hipMemcpy(bank, emb_bank_, (size_t)first * row, hipMemcpyDeviceToDevice);
        if (st == hipSuccess && after)
            st = hipMemcpy(bank + (size_t)first * cfg_.ctx_dim, emb_bank_ + (size_t)(first + v) * cfg_.ctx_dim, (size_t)after * row, hipMemcpyDeviceToDevice);
        if (st != hipSuccess) { (void)hipFree(bank); SDMI_HIP(st); }
    }
    (void)hipFree(emb_bank_);
    emb_bank_ = bank;
    emb_rows_ -= v;
    embeddings_.erase(embeddings_.begin() + (long)at);
}

// A textual-inversion file: the tensor "emb_params" or else the file's only tensor, [C] or [v, C] in F32 / F16 / BF16, through the mapped reader and
// k_unpack.hip's widening (the route checkpoints take).  Runs inside the caller's Call.
void Engine::embedding_load_safetensors(const std::string& name, const std::vector<int32_t>& ids, const char* path) {
    if (!path) throw Error(SDMI_ERR_INVALID, "embedding_load_safetensors: null path");
    if (cfg_.clip_layers <= 0) throw Error(SDMI_ERR_STATE, "embedding_load_safetensors: this context has no text encoder (clip_layers = 0)");
    SafetensorsFile f(path);
    const StTensor* t = f.find("emb_params");
    if (!t && f.tensors().size() == 1) t = &f.tensors()[0];
    if (!t) throw Error(SDMI_ERR_WEIGHTS, std::string("embedding_load_safetensors: ") + path + " has no tensor 'emb_params' and " + std::to_string(f.tensors().size()) + " tensors to choose from");
    const int dt = unpack_dtype(t->dtype);
    if (dt < 0) throw Error(SDMI_ERR_UNSUPPORTED, "embedding_load_safetensors: '" + t->key + "' has dtype " + t->dtype + "; F32, F16 and BF16 are supported");
    const size_t nd = t->shape.size();
    if (nd < 1 || nd > 2 || t->shape[nd - 1] != cfg_.ctx_dim || t->count == 0)
        throw Error(SDMI_ERR_INVALID, "embedding_load_safetensors: '" + t->key + "' has shape " + shape_str(t->shape.data(), nd) + ", expected [" +
                                          std::to_string(cfg_.ctx_dim) + "] or [v, " + std::to_string(cfg_.ctx_dim) + "]");
    const int64_t v = nd == 2 ? t->shape[0] : 1;
    if (v > cfg_.clip_ctx - 2) throw Error(SDMI_ERR_INVALID, "embedding_load_safetensors: '" + t->key + "' has " + std::to_string(v) + " vectors; at most clip_ctx - 2 fit a chunk");
    Buf raw(this, t->nbytes), wide(this, t->count * sizeof(float));
    SDMI_HIP(hipMemcpyAsync(raw.p, t->data, t->nbytes, hipMemcpyHostToDevice, stream_));
    SDMI_LAUNCH(launch_unpack_tensor(raw.p, dt, 0, (long long)t->count, 1, wide.f(), stream_));
    embedding_add(name, ids, wide.f(), (int)v, true);   // synchronises: the mapping and the two buffers outlive the copies
}

// ---- conditioned UNet input (unet_in_ch > 4; include/sdmi.h "conditioned UNet") ---------------------------------------
// An entry point that takes no conditioning cannot serve a model that needs it, and the other way round: both are SDMI_ERR_STATE.
void Engine::check_cond(const char* entry, bool given) const {
    if (cond_ch() > 0 && !given)
        throw Error(SDMI_ERR_STATE, std::string(entry) + ": this context's UNet takes " + std::to_string(cond_ch()) + " conditioning channels (unet_in_ch = " +
                                        std::to_string(cfg_.unet_in_ch) + "): use the _cond entry (sdmi_unet_forward_cond, sdmi_img2img_latent_cond, sdmi_inpaint_image)");
    if (cond_ch() == 0 && given) throw Error(SDMI_ERR_STATE, std::string(entry) + ": this context's UNet takes no conditioning channels (unet_in_ch = 4)");
}

// the caller's cond [n, cond_ch, h, w] (device, NCHW) -> a pool buffer [n][hw][padded_in_ch - 4] (the caller frees it)
float* Engine::cond_to_nhwc(const float* cond_nchw, int n) {
    const long long hw = (long long)lat_h_ * lat_w_;
    const int pcc = unet_in_padded() - 4;
    float* c = reinterpret_cast<float*>(pool_.alloc((size_t)n * hw * pcc * sizeof(float)));
    SDMI_LAUNCH(launch_cond_nchw_to_nhwc(cond_nchw, c, n, cond_ch(), hw, pcc, stream_));
    return c;
}

// unet_in [rows][hw][4] + cond [n][hw][pc - 4] -> dst [rows][hw][pc], in front of a unet_run
void Engine::assemble_unet_in(const float* unet_in, const float* cond_nhwc, int rows, int n, float* dst) {
    const long long hw = (long long)lat_h_ * lat_w_;
    const int pc = unet_in_padded();
    ProfScope ps_o(this, PC_OTHER, 0, (double)rows * hw * (4 + (pc - 4) + pc) * 4.0);
    SDMI_LAUNCH_IN(ps_o, 0, launch_assemble_unet_in(unet_in, cond_nhwc, dst, (long long)rows * hw, (long long)n * hw, pc, cond_ch(), stream_));
}

void Engine::unet_forward_dev(const float* x_nchw, int t, const float* context, int n, int T, float* out_nchw, const float* cond_nchw) {
    if (!finalized_) throw Error(SDMI_ERR_STATE, "weights not finalized");
    check_cond("unet_forward", cond_nchw != nullptr);
    if (n <= 0 || T <= 0) throw Error(SDMI_ERR_INVALID, "unet_forward: n and T must be positive");
    check_batch(n);
    const int H = lat_h_, W = lat_w_;
    std::vector<int> kv(n, T), ts(1, t);
    unet_prepare(context, n, T, kv.data(), ts, n, /*window=*/false);
    Buf xin(this, (size_t)n * H * W * 4 * 4), xout(this, (size_t)n * H * W * 4 * 4);
    SDMI_LAUNCH(launch_nchw_to_nhwc(x_nchw, xin.f(), n, 4, H, W, 1.0f, stream_));
    if (cond_nchw) {
        Buf xc(this, (size_t)n * H * W * unet_in_padded() * 4);
        float* c = cond_to_nhwc(cond_nchw, n);
        assemble_unet_in(xin.f(), c, n, n, xc.f());
        pool_.free(c);
        unet_run(xc.f(), n, 0, xout.f());
    } else
    unet_run(xin.f(), n, 0, xout.f());
    SDMI_LAUNCH(launch_nhwc_to_nchw(xout.f(), out_nchw, n, 4, H, W, stream_));
    unet_release();
}

// StableDiffusion::sample_latent + forward_diffuser (stablediffusion/mod.rs:102-192)
void Engine::sample_latent_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale,
                               size_t n_steps, const float* init_latent, float* latent_out, bool out_nhwc) {
    if (!finalized_) throw Error(SDMI_ERR_STATE, "weights not finalized");
    check_cond("sample_latent", false);
    if (n <= 0 || T <= 0 || Tu <= 0) throw Error(SDMI_ERR_INVALID, "sample_latent: n, T, Tu must be positive");
    check_batch(n);
    check_schedule("sample_latent");
    const size_t total = alphas_.size();
    if (n_steps == 0 || n_steps > total) throw Error(SDMI_ERR_INVALID, "sample_latent: n_steps out of range");
    const int H = lat_h_, W = lat_w_;
    const size_t step_size = total / n_steps;                       // :111
    std::vector<int> ts;
    for (long long t = (long long)total - 1; t >= 0; t -= (long long)step_size) ts.push_back((int)t);  // :123
    std::vector<double> kplan;   // a k-sampler plans its own schedule; init_latent is the VP latent at its first sigma
    if (kset_) kplan = kplan_for(n_steps, 1.0, nullptr);
    sample_loop(context, n, T, uncond, Tu, scale, ts, step_size, [&](float* latent, float* unet_in, long long per_half) {
        SDMI_HIP(launch_nchw_to_nhwc(init_latent, latent, n, 4, H, W, 1.0f, stream_));   // (outside the profile, counted)
        count_kernel();
        SDMI_LAUNCH(launch_dup_latent(latent, unet_in, per_half, stream_));
    }, nullptr, latent_out, out_nhwc, nullptr, kset_ ? &kplan : nullptr);
}

void Engine::check_sampler(const sdmi_sampler& s) {
    if (s.kind < 0 || s.kind > 2) throw Error(SDMI_ERR_INVALID, "sampler: kind must be 0 (DDIM), 1 (DPM-Solver++ 2M) or 2 (PLMS)");
    if (!(s.eta >= 0.0 && s.eta <= 1.0)) throw Error(SDMI_ERR_INVALID, "sampler: eta must satisfy 0 <= eta <= 1");
    if (s.kind != 0 && s.eta != 0.0) throw Error(SDMI_ERR_INVALID, "sampler: eta belongs to kind 0 (DDIM) only");
}

void Engine::set_sampler(const sdmi_sampler* s) {
    if (s) check_sampler(*s);
    sampler_ = s ? *s : sdmi_sampler{};
    ksampler_ = sdmi_ksampler{};   // the two sticky states exclude each other
    kset_ = false;
}

void Engine::set_prediction(int kind) {
    if (kind != 0 && kind != 1) throw Error(SDMI_ERR_INVALID, "set_prediction: kind must be 0 (eps) or 1 (v)");
    prediction_ = kind;
}

void Engine::set_guidance_rescale(double phi) {
    if (!(phi >= 0.0 && phi <= 1.0)) throw Error(SDMI_ERR_INVALID, "set_guidance_rescale: phi must satisfy 0 <= phi <= 1");
    rescale_ = phi;
}

void Engine::rescale_zero_snr(const float* in, float* out, int n) {
    if (!in || !out) throw Error(SDMI_ERR_INVALID, "rescale_zero_snr: null pointer");
    if (n < 2) throw Error(SDMI_ERR_INVALID, "rescale_zero_snr: the table needs at least two entries");
    for (int j = 0; j < n; ++j)
        if (!(in[j] >= 0.0f && in[j] <= 1.0f)) throw Error(SDMI_ERR_INVALID, "rescale_zero_snr: alphas_cumprod must lie inside [0, 1]");
    const double s0 = std::sqrt((double)in[0]), sT = std::sqrt((double)in[n - 1]);
    if (!(s0 > sT)) throw Error(SDMI_ERR_INVALID, "rescale_zero_snr: the first entry must be larger than the last");
    const double k = s0 / (s0 - sT);
    for (int j = 1; j < n - 1; ++j) {
        const double s = (std::sqrt((double)in[j]) - sT) * k;
        out[j] = (float)(s * s);
    }
    out[0] = in[0];     // (s_0 - s_T) s_0 / (s_0 - s_T) = s_0: the bits it had
    out[n - 1] = 0.0f;
}

void Engine::refresh_schedule() {
    alphas_ = alphas_loaded_;
    if (zero_snr_ && alphas_loaded_.size() >= 2) rescale_zero_snr(alphas_loaded_.data(), alphas_.data(), (int)alphas_.size());
}

void Engine::set_zero_snr(bool on) {
    if (on && alphas_loaded_.size() >= 2) {   // refused before the state moves
        std::vector<float> probe(alphas_loaded_.size());
        rescale_zero_snr(alphas_loaded_.data(), probe.data(), (int)probe.size());
    }
    zero_snr_ = on;
    refresh_schedule();
}

void Engine::check_schedule(const char* entry) const {
    bool zero = false;
    for (float a : alphas_) zero = zero || a == 0.0f;
    if (!zero) return;
    if (kset_)
        throw Error(SDMI_ERR_UNSUPPORTED, std::string(entry) + ": a sigma-schedule sampler cannot run on a schedule that holds alphas_cumprod = 0 (zero terminal SNR): sigma_max is infinite");
    if (prediction_ == 0)
        throw Error(SDMI_ERR_INVALID, std::string(entry) + ": eps-prediction on a schedule that holds alphas_cumprod = 0 (zero terminal SNR): eps does not determine x0 there; set v-prediction");
}

void Engine::set_ksampler(const sdmi_ksampler* k) {
    if (!k) { ksampler_ = sdmi_ksampler{}; kset_ = false; return; }
    check_ksampler(*k, alphas_.empty() ? nullptr : alphas_.data(), (int)alphas_.size());
    ksampler_ = *k;
    kset_ = true;
    sampler_ = sdmi_sampler{};
}

std::vector<double> Engine::kplan_for(size_t n_steps, double strength, double* a0) const {
    std::vector<double> rows = ksampler_plan(ksampler_, alphas_.data(), (int)alphas_.size(), n_steps, strength, nullptr, prediction_);
    const double s0 = rows[KP_SIGMA];
    if (a0) *a0 = 1.0 / (1.0 + s0 * s0);
    return rows;
}

void Engine::sample_loop(const float* context, int n, int T, const float* uncond, int Tu, double scale, const std::vector<int>& ts,
                         size_t step_size, const std::function<void(float* latent, float* unet_in, long long per_half)>& start,
                         const Blend* blend, float* latent_out, bool out_nhwc, const float* cond_nhwc, const std::vector<double>* kplan) {
    const int H = lat_h_, W = lat_w_, cd = cfg_.ctx_dim;
    const int nb = 2 * n, t_max = std::max(T, Tu);
    check_schedule("sample_loop");

    // packed context [2n][t_max][cd]: rows 0..n-1 = uncond (broadcast, :173-177), n..2n-1 = cond
    Buf ctx(this, (size_t)nb * t_max * cd * 4);
    SDMI_HIP(hipMemsetAsync(ctx.p, 0, (size_t)nb * t_max * cd * 4, stream_));
    for (int b = 0; b < n; ++b)
        SDMI_HIP(hipMemcpyAsync(ctx.f() + (size_t)b * t_max * cd, uncond, (size_t)Tu * cd * 4, hipMemcpyDeviceToDevice, stream_));
    for (int b = 0; b < n; ++b)
        SDMI_HIP(hipMemcpyAsync(ctx.f() + (size_t)(n + b) * t_max * cd, context + (size_t)b * T * cd, (size_t)T * cd * 4,
                                hipMemcpyDeviceToDevice, stream_));
    std::vector<int> kv(nb);
    for (int b = 0; b < n; ++b) { kv[b] = Tu; kv[n + b] = T; }
    const size_t n_eval = kplan ? kplan->size() / KPLAN_COLS : 0;
    if (kplan) {   // a k-sampler: one row of the time tables per UNet evaluation, at the plan's fractional times
        std::vector<double> tf(n_eval);
        std::vector<int> eval_step(n_eval);
        const int first_step = (int)(*kplan)[KP_STEP];
        for (size_t i = 0; i < n_eval; ++i) {
            tf[i] = (*kplan)[i * KPLAN_COLS + KP_T];
            eval_step[i] = (int)(*kplan)[i * KPLAN_COLS + KP_STEP] - first_step;
        }
        unet_prepare(ctx.f(), nb, t_max, kv.data(), tf, eval_step, eval_step.back() + 1, n);
    } else
    unet_prepare(ctx.f(), nb, t_max, kv.data(), ts, n);

    const long long per_half = (long long)n * H * W * 4;
    Buf latent(this, per_half * 4), unet_in(this, 2 * per_half * 4), eps(this, 2 * per_half * 4);
    // a conditioned model: the update kernels keep writing unet_in [2n][hw][4]; one launch per step assembles [latent | cond | pad] from it (k_inpaint.hip)
    std::unique_ptr<Buf> unet_in_c;
    if (cond_nhwc) unet_in_c.reset(new Buf(this, (size_t)(2 * per_half / 4) * unet_in_padded() * 4));
    // sampler choice: the coefficient table of the call and its history slots (x0 for DPM-Solver++(2M), three e for PLMS)
    // (v-prediction: the default path too runs on the table -- DDIM(eta = 0), depth 0 -- because cfg_ddim_update divides by sqrt(a_t) and is kept as it is)
    // (CFG rescale, section 9k: the same -- the statistics need launch_sampler_step's one-workgroup-per-image kernel; with rescale_ = 0 nothing here changes)
    const float rescale = (float)rescale_;
    const bool custom = !kplan && (sampler_.kind != 0 || sampler_.eta != 0.0 || prediction_ != 0 || rescale_ != 0.0);
    const int depth = !custom ? 0 : sampler_.kind == 1 ? 1 : sampler_.kind == 2 ? 3 : 0;
    std::vector<double> coefs;
    std::unique_ptr<Buf> hist[3];
    if (custom) {
        coefs.resize(ts.size() * 8);
        const int st = sdmi_sampler_coefs_ex(&sampler_, alphas_.data(), (int32_t)alphas_.size(), ts.data(), (int32_t)ts.size(), (int64_t)step_size, prediction_, coefs.data());
        if (st != SDMI_OK) throw Error(st, "sample_loop: sdmi_sampler_coefs refused the schedule");
        for (int k = 0; k < depth; ++k) hist[k].reset(new Buf(this, per_half * 4));
    }
    if (kplan && ksampler_.kind != 0) hist[0].reset(new Buf(this, per_half * 4));   // depth 1 everywhere; euler keeps nothing
    start(latent.f(), unet_in.f(), per_half);
    for (size_t i = 0; i < n_eval; ++i) {   // the k-sampler's loop: one UNet run and ONE update launch per evaluation
        const double* k = &(*kplan)[i * KPLAN_COLS];
        if (cond_nhwc) assemble_unet_in(unet_in.f(), cond_nhwc, nb, n, unet_in_c->f());
        unet_run(cond_nhwc ? unet_in_c->f() : unet_in.f(), nb, (int)i, eps.f(), opt_cfg_share_ != 0);
        const int depth = hist[0] ? 1 : 0;
        SamplerStep p{};
        p.scale = (float)scale;
        p.cx = (float)k[KP_CX]; p.ce = (float)k[KP_CE]; p.h[0] = (float)k[KP_H1]; p.cz = (float)k[KP_CZ]; p.cz2 = (float)k[KP_CZ2];
        p.qx = (float)k[KP_QX]; p.qe = (float)k[KP_QE];
        p.n_hist = (depth && i > 0) ? 1 : 0;   // (history starts empty; where the row's h1 is 0 the slot is read and weighs nothing)
        const bool last = k[KP_AEND] >= 0.0;   // the mask blend follows a step's last evaluation only
        if (last) { p.blend_prev = (float)std::sqrt(k[KP_AEND]); p.blend_dir = (float)std::sqrt(1.0 - k[KP_AEND]); }
        const float* q_prev[3] = {p.n_hist ? hist[0]->f() : nullptr, nullptr, nullptr};
        const uint64_t key = ksampler_.noise_seed + (uint64_t)ksampler_.image_base + (((uint64_t)k[KP_STEP] + 1) << 32);
        const bool bl = blend && last;
        SDMI_LAUNCH(launch_sampler_step(eps.f(), latent.f(), unet_in.f(), per_half, (long long)H * W, p, rescale, depth, q_prev, depth ? hist[0]->f() : nullptr, key,
                                        key + (1ull << 62), bl ? blend->mask : nullptr, bl ? blend->z0 : nullptr, bl ? blend->eps : nullptr, stream_));
    }
    for (size_t s = 0; s < (kplan ? 0 : ts.size()); ++s) {
        const size_t t = (size_t)ts[s];
        const double cur = (double)alphas_[t];                                           // :124-129
        const double prev = t >= step_size ? (double)alphas_[t - step_size] : 1.0;       // :131-140
        DdimCoef c{};
        c.scale = (float)scale;
        c.sqrt_noise = (float)std::sqrt(1.0 - cur);                                      // :142
        c.sqrt_cur = (float)std::sqrt(cur);
        c.sqrt_prev = (float)std::sqrt(prev);
        c.dir_coef = (float)std::sqrt(1.0 - prev - 0.0);                                 // :153 (sigma = 0)
        if (cond_nhwc) assemble_unet_in(unet_in.f(), cond_nhwc, nb, n, unet_in_c->f());
        unet_run(cond_nhwc ? unet_in_c->f() : unet_in.f(), nb, (int)s, eps.f(), opt_cfg_share_ != 0);   // unet_in = [latent | latent]: a CFG pair (with the same cond rows)
        if (custom) {
            const double* k = &coefs[s * 8];
            SamplerStep p{};
            p.scale = (float)scale;
            p.cx = (float)k[0]; p.ce = (float)k[1]; p.h[0] = (float)k[2]; p.h[1] = (float)k[3]; p.h[2] = (float)k[4]; p.cz = (float)k[5];
            p.qx = (float)k[6]; p.qe = (float)k[7];
            p.blend_prev = c.sqrt_prev; p.blend_dir = c.dir_coef;
            p.n_hist = (int)std::min<size_t>(s, (size_t)depth);
            // slot (s mod depth) receives this step's q: the slot of the oldest one.  q of k + 1 steps ago sits in slot (s - 1 - k) mod depth.
            const float* q_prev[3] = {nullptr, nullptr, nullptr};
            for (int j = 0; j < p.n_hist; ++j) q_prev[j] = hist[(s - 1 - (size_t)j) % (size_t)depth]->f();
            float* q_out = depth ? hist[s % (size_t)depth]->f() : nullptr;
            // index of this step in the FULL schedule (ts may be its img2img tail): the noise key does not depend on strength
            const uint64_t s_full = (uint64_t)((alphas_.size() - 1 - t) / step_size);
            const uint64_t key = sampler_.noise_seed + (uint64_t)sampler_.image_base + ((s_full + 1) << 32);
            SDMI_LAUNCH(launch_sampler_step(eps.f(), latent.f(), unet_in.f(), per_half, (long long)H * W, p, rescale, depth, q_prev, q_out, key, 0,
                                            blend ? blend->mask : nullptr, blend ? blend->z0 : nullptr, blend ? blend->eps : nullptr, stream_));
        } else
        if (blend) SDMI_LAUNCH(launch_cfg_ddim_masked(eps.f(), latent.f(), unet_in.f(), per_half, c, blend->mask, blend->z0, blend->eps, stream_));
        else SDMI_LAUNCH(launch_cfg_ddim(eps.f(), latent.f(), unet_in.f(), per_half, c, stream_));
    }
    if (out_nhwc) {
        SDMI_HIP(hipMemcpyAsync(latent_out, latent.p, (size_t)per_half * 4, hipMemcpyDeviceToDevice, stream_));
    } else {
        SDMI_LAUNCH(launch_nhwc_to_nchw(latent.f(), latent_out, n, 4, H, W, stream_));
    }
    unet_release();
}

// img2img rule 1 (sdmi_img2img_timesteps, DESIGN.md "img2img") plus the checks of sample_latent
std::vector<int> Engine::img2img_schedule(int n, int T, int Tu, size_t n_steps, double strength, size_t* step_size) {
    if (!finalized_) throw Error(SDMI_ERR_STATE, "weights not finalized");
    if (n <= 0 || T <= 0 || Tu <= 0) throw Error(SDMI_ERR_INVALID, "img2img: n, T, Tu must be positive");
    check_batch(n);
    check_schedule("img2img");
    const size_t total = alphas_.size();
    if (n_steps == 0 || n_steps > total) throw Error(SDMI_ERR_INVALID, "img2img: n_steps out of range");
    *step_size = total / n_steps;
    if (kset_) {   // a k-sampler applies the strength rule to its own steps: kplan_for refuses what leaves none; ts is unused then
        (void)kplan_for(n_steps, strength, nullptr);
        return std::vector<int>(1, 0);
    }
    std::vector<int> ts(total);
    int32_t count = 0;
    const int st = sdmi_img2img_timesteps((int32_t)total, n_steps, strength, ts.data(), (int32_t)total, &count);
    if (st != SDMI_OK) throw Error(st, "img2img: strength must satisfy 0 < strength <= 1 and leave at least one step");
    ts.resize(count);
    *step_size = total / n_steps;
    return ts;
}

void Engine::img2img_latent_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale, size_t n_steps,
                                double strength, const float* z0, const float* mask, const float* noise, uint64_t seed, float* latent_out, const float* cond_nchw) {
    if (finalized_) check_cond("img2img_latent", cond_nchw != nullptr);
    size_t step_size = 0;
    const std::vector<int> ts = img2img_schedule(n, T, Tu, n_steps, strength, &step_size);
    struct PoolPtr { DevPool& pool; float* p; ~PoolPtr() { if (p) pool.free(p); } } cond{pool_, nullptr};
    if (cond_nchw) cond.p = cond_to_nhwc(cond_nchw, n);
    const long long hw = (long long)lat_h_ * lat_w_, elems = (long long)n * hw * 4;
    double a0 = (double)alphas_[ts[0]];
    std::vector<double> kplan;
    if (kset_) kplan = kplan_for(n_steps, strength, &a0);
    const float sqrt_a = (float)std::sqrt(a0), sqrt_1ma = (float)std::sqrt(1.0 - a0);
    Buf z0k(this, mask ? elems * 4 : 256), e0k(this, mask ? elems * 4 : 256);   // z0 and eps for the blend (NHWC)
    const Blend blend{mask, z0k.f(), e0k.f()};
    sample_loop(context, n, T, uncond, Tu, scale, ts, step_size, [&](float* latent, float* unet_in, long long per_half) {
        SDMI_LAUNCH(launch_img2img_start(z0, false, noise, seed, sqrt_a, sqrt_1ma, latent, unet_in, per_half, mask ? z0k.f() : nullptr, mask ? e0k.f() : nullptr, n, hw,
                                         stream_));
    }, mask ? &blend : nullptr, latent_out, false, cond.p, kset_ ? &kplan : nullptr);
}

void Engine::img2img_image_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale, size_t n_steps,
                               double strength, const uint8_t* init_rgb, const float* mask, const float* noise, uint64_t seed, float* latent_out, const float* cond_nhwc) {
    if (finalized_) check_cond("img2img_image", cond_nhwc != nullptr);
    if (finalized_ && !enc_ready_) throw Error(SDMI_ERR_STATE, "VAE encoder weights are not loaded (autoencoder/encoder/..., autoencoder/quant_conv)");
    size_t step_size = 0;
    const std::vector<int> ts = img2img_schedule(n, T, Tu, n_steps, strength, &step_size);
    const int H = lat_h_, W = lat_w_;
    const long long hw = (long long)H * W, elems = (long long)n * hw * 4;
    double a0 = (double)alphas_[ts[0]];
    std::vector<double> kplan;
    if (kset_) kplan = kplan_for(n_steps, strength, &a0);
    const float sqrt_a = (float)std::sqrt(a0), sqrt_1ma = (float)std::sqrt(1.0 - a0);
    Buf z0k(this, mask ? elems * 4 : 256), e0k(this, mask ? elems * 4 : 256);
    const Blend blend{mask, z0k.f(), e0k.f()};
    sample_loop(context, n, T, uncond, Tu, scale, ts, step_size, [&](float* latent, float* unet_in, long long per_half) {
        for (int i = 0; i < n; ++i) {   // one image at a time through the encoder, as encode_image_dev; its start latent right behind its quant_conv
            Act rgb = new_act(1, 8 * H, 8 * W, 4, /*dt=*/0);
            SDMI_LAUNCH(launch_rgb_u8_to_nhwc4(init_rgb + (size_t)i * 3 * 64 * hw, rgb.p, 64 * hw, stream_));
            Act q8 = encode_one(rgb);
            const long long off = (long long)i * hw * 4;
            SDMI_LAUNCH(launch_img2img_start(q8.p, true, noise ? noise + off : nullptr, seed + (uint64_t)i, sqrt_a, sqrt_1ma, latent + off, unet_in + off, per_half,
                                             mask ? z0k.f() + off : nullptr, mask ? e0k.f() + off : nullptr, 1, hw, stream_));
            release(q8);
        }
    }, mask ? &blend : nullptr, latent_out, false, cond_nhwc, kset_ ? &kplan : nullptr);
}

// ---- inpainting (unet_in_ch = 9; include/sdmi.h "inpainting") ---------------------------------------------------------
void Engine::check_inpaint(const char* entry) const {
    if (!finalized_) throw Error(SDMI_ERR_STATE, "weights not finalized");
    if (cfg_.unet_in_ch != 9)
        throw Error(SDMI_ERR_STATE, std::string(entry) + ": needs an inpainting UNet (unet_in_ch = 9: latent, mask, masked-picture latent); this context has unet_in_ch = " +
                                        std::to_string(cfg_.unet_in_ch));
    if (!enc_ready_) throw Error(SDMI_ERR_STATE, "VAE encoder weights are not loaded (autoencoder/encoder/..., autoencoder/quant_conv)");
}

// cond rows [n][hw][8] = latent mask | 0.18215 * posterior mean of the masked picture | 0 0 0; lat_mask (may be null) [n][hw].  One image at a time through
// encode_one, as img2img_image_dev.
void Engine::inpaint_cond_nhwc(const uint8_t* init_rgb, const uint8_t* mask_u8, int n, float* cond_nhwc, float* lat_mask) {
    const int H = lat_h_, W = lat_w_;
    const long long hw = (long long)H * W;
    for (int i = 0; i < n; ++i) {
        Act rgb = new_act(1, 8 * H, 8 * W, 4, /*dt=*/0);
        SDMI_LAUNCH(launch_rgb_u8_masked_to_nhwc4(init_rgb + (size_t)i * 3 * 64 * hw, mask_u8 + (size_t)i * 64 * hw, rgb.p, 64 * hw, stream_));
        Act q8 = encode_one(rgb);
        SDMI_LAUNCH(launch_inpaint_cond_pack(q8.p, mask_u8 + (size_t)i * 64 * hw, cond_nhwc + (size_t)i * hw * 8, lat_mask ? lat_mask + (size_t)i * hw : nullptr, H, W, stream_));
        release(q8);
    }
}

void Engine::inpaint_cond_dev(const uint8_t* init_rgb, const uint8_t* mask_u8, int n, float* cond_nchw) {
    check_inpaint("inpaint_cond");
    if (n <= 0) throw Error(SDMI_ERR_INVALID, "inpaint_cond: n must be positive");
    check_batch(n);
    const int H = lat_h_, W = lat_w_;
    Buf cond(this, (size_t)n * H * W * 8 * sizeof(float));
    inpaint_cond_nhwc(init_rgb, mask_u8, n, cond.f(), nullptr);
    SDMI_LAUNCH(launch_nhwc_to_nchw_slice(cond.f(), cond_nchw, n, 8, 5, H, W, stream_));
}

void Engine::inpaint_image_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale, size_t n_steps, double strength,
                               const uint8_t* init_rgb, const uint8_t* mask_u8, const sdmi_inpaint* opt, const float* noise, uint64_t seed, uint8_t* rgb_out) {
    check_inpaint("inpaint_image");
    if (n <= 0) throw Error(SDMI_ERR_INVALID, "inpaint_image: n must be positive");
    check_batch(n);
    const bool latent_blend = opt && opt->latent_blend != 0, paste_back = opt && opt->paste_back != 0;
    const int H = lat_h_, W = lat_w_;
    const size_t hw = (size_t)H * W;
    Buf cond(this, (size_t)n * hw * 8 * sizeof(float)), lmask(this, latent_blend ? (size_t)n * hw * sizeof(float) : 256), lat(this, (size_t)n * hw * 4 * sizeof(float));
    inpaint_cond_nhwc(init_rgb, mask_u8, n, cond.f(), latent_blend ? lmask.f() : nullptr);
    img2img_image_dev(context, n, T, uncond, Tu, scale, n_steps, strength, init_rgb, latent_blend ? lmask.f() : nullptr, noise, seed, lat.f(), cond.f());
    decode_latent_dev(lat.f(), n, (float)(1.0 / 0.18215), nullptr, rgb_out);
    if (paste_back) {
        SDMI_LAUNCH(launch_inpaint_paste(rgb_out, init_rgb, mask_u8, rgb_out, (long long)n * 64 * hw, stream_));
    }
}

// ---- latent resampler + hires fix (include/sdmi.h "hires fix") ----------------------------------------------------
namespace {
// the table of one axis on the device: [first: out ints][count: out ints][taps: out * max_taps floats] in one pool buffer
struct AxisTable {
    std::unique_ptr<Engine::Buf> buf;
    int max_taps = 0, out = 0;
    const int* first() const { return reinterpret_cast<const int*>(buf->p); }
    const int* count() const { return first() + out; }
    const float* taps() const { return reinterpret_cast<const float*>(count() + out); }
};
AxisTable upload_axis(Engine& e, int in_size, int out_size, int mode, int antialias) {
    const std::vector<ResizeRow> rows = resize_rows(in_size, out_size, mode, antialias != 0);
    size_t T = 0;
    for (const ResizeRow& r : rows) {   // the kernel reads x[first .. first + count) unchecked
        if (r.first < 0 || r.w.empty() || r.first + (long long)r.w.size() > in_size) throw Error(SDMI_ERR_STATE, "resize: tap table out of range");
        T = std::max(T, r.w.size());
    }
    std::vector<int32_t> img(2 * (size_t)out_size + (size_t)out_size * T, 0);
    float* tf = reinterpret_cast<float*>(img.data() + 2 * (size_t)out_size);
    for (int o = 0; o < out_size; ++o) {
        const ResizeRow& r = rows[(size_t)o];
        img[(size_t)o] = r.first;
        img[(size_t)out_size + o] = (int32_t)r.w.size();
        for (size_t j = 0; j < r.w.size(); ++j) tf[(size_t)o * T + j] = (float)r.w[j];
    }
    AxisTable t;
    t.max_taps = (int)T; t.out = out_size;
    t.buf.reset(new Engine::Buf(&e, img.size() * 4));
    // `img` is pageable and dies with this frame: HIP stages a pageable host-to-device copy before hipMemcpyAsync returns (the operator entries' epilogue staging and unet_prepare rely on the same)
    SDMI_HIP(hipMemcpyAsync(t.buf->p, img.data(), img.size() * 4, hipMemcpyHostToDevice, e.stream()));
    return t;
}
}  // namespace

void Engine::resize_nhwc4(const float* x, int n, int h, int w, int oh, int ow, int mode, int antialias, float* y) {
    if (n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) throw Error(SDMI_ERR_INVALID, "resize: sizes must be positive");
    if (mode < 0 || mode > 2) throw Error(SDMI_ERR_INVALID, "resize: mode must be 0 (nearest-exact), 1 (bilinear) or 2 (bicubic)");
    if (mode == 0 && antialias) throw Error(SDMI_ERR_INVALID, "resize: antialias belongs to modes 1 and 2");
    if (h == oh && w == ow) {   // both axes are the identity
        SDMI_HIP(hipMemcpyAsync(y, x, (size_t)n * h * w * 16, hipMemcpyDeviceToDevice, stream_));
        return;
    }
    const float* src = x;
    std::unique_ptr<Buf> mid;
    if (w != ow) {   // horizontal: [n * h][w] -> [n * h][ow]
        float* dst = y;
        if (h != oh) { mid.reset(new Buf(this, (size_t)n * h * ow * 16)); dst = mid->f(); }
        AxisTable t = upload_axis(*this, w, ow, mode, antialias);
        SDMI_LAUNCH(launch_resize_axis(src, dst, t.first(), t.count(), t.taps(), t.max_taps, (long long)n * h, w, ow, 1, mode == 0, stream_));
        src = dst;
    }
    if (h != oh) {   // vertical: [n][h][ow] -> [n][oh][ow]
        AxisTable t = upload_axis(*this, h, oh, mode, antialias);
        SDMI_LAUNCH(launch_resize_axis(src, y, t.first(), t.count(), t.taps(), t.max_taps, n, h, oh, ow, mode == 0, stream_));
    }
}

void Engine::check_hires(const sdmi_hires* hr) {
    if (!hr) throw Error(SDMI_ERR_INVALID, "hires: null sdmi_hires");
    check_latent_size(hr->base_h, hr->base_w);
    if (hr->mode < 0 || hr->mode > 2) throw Error(SDMI_ERR_INVALID, "hires: mode must be 0 (nearest-exact), 1 (bilinear) or 2 (bicubic)");
    if (hr->mode == 0 && hr->antialias) throw Error(SDMI_ERR_INVALID, "hires: antialias belongs to modes 1 and 2");
    if (!(hr->strength > 0.0 && hr->strength <= 1.0)) throw Error(SDMI_ERR_INVALID, "hires: strength must satisfy 0 < strength <= 1");
    if (hr->hires_steps < 0) throw Error(SDMI_ERR_INVALID, "hires: hires_steps must not be negative");
}

void Engine::hires_latent_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale, size_t n_steps, const float* init_latent,
                              const sdmi_hires& hr, const float* hires_noise, float* latent_out) {
    check_hires(&hr);
    if (ctrl_.set) throw Error(SDMI_ERR_UNSUPPORTED, "hires: a control is set (sdmi_set_control) and the first pass runs at another size than its hint: clear it first");
    if (finalized_) check_cond("hires", false);
    const size_t steps2 = hr.hires_steps ? (size_t)hr.hires_steps : n_steps;
    {   // the second pass's argument errors before the first pass runs
        size_t step_size = 0;
        (void)img2img_schedule(n, T, Tu, steps2, hr.strength, &step_size);
    }
    const int H = lat_h_, W = lat_w_;
    Buf zb(this, (size_t)n * hr.base_h * hr.base_w * 16), zr(this, (size_t)n * H * W * 16), z0(this, (size_t)n * H * W * 16);
    {
        struct Restore { Engine* e; int h, w; ~Restore() { e->lat_h_ = h; e->lat_w_ = w; } } restore{this, H, W};
        lat_h_ = hr.base_h; lat_w_ = hr.base_w;
        sample_latent_dev(context, n, T, uncond, Tu, scale, n_steps, init_latent, zb.f(), /*out_nhwc=*/true);
    }
    resize_nhwc4(zb.f(), n, hr.base_h, hr.base_w, H, W, hr.mode, hr.antialias, zr.f());
    // launch_img2img_start reads its caller's z0 as NCHW: one transposing launch in front of it, and the second pass is img2img_latent_dev itself
    SDMI_LAUNCH(launch_nhwc_to_nchw(zr.f(), z0.f(), n, 4, H, W, stream_));
    img2img_latent_dev(context, n, T, uncond, Tu, scale, steps2, hr.strength, z0.f(), nullptr, hires_noise, hr.hires_seed, latent_out);
}

// Autoencoder::decode_latent (autoencoder/mod.rs:68-71) -> Decoder::forward (:205-217)
void Engine::decode_one(const float* z_nhwc, int n, Act& img) {
    Range rng(this, "Decoder::forward");
    const int H = lat_h_, W = lat_w_, vc = cfg_.vae_ch;
    Act z; z.p = const_cast<float*>(z_nhwc); z.n = n; z.h = H; z.w = W; z.c = 4; z.dt = 0;
    Act pq = new_act(n, H, W, 4, /*dt=*/0);  // the two Cin = 4 layers run on the fp32 kernel in both precisions
    conv(post_quant_, z, pq, 1, 0, nullptr, 0, nullptr);
    Act x = new_act(n, H, W, 4 * vc);
    conv(dec_conv_in_, pq, x, 1, 0, nullptr, 0, nullptr);
    release(pq);
    {   // Mid (:457-462)
        Act a = new_act(n, H, W, 4 * vc); res_block(dec_mid1_, x, a, 0); release(x);
        Act b = new_act(n, H, W, 4 * vc); vae_attn(dec_attn_, a, b); release(a);
        Act c = new_act(n, H, W, 4 * vc); res_block(dec_mid2_, b, c, 0); release(b);
        x = c;
    }
    for (int i = 0; i < 4; ++i) {  // DecoderBlock::forward (:308-323)
        const DecBlockW& b = dec_blocks_[i];
        for (int r = 0; r < 3; ++r) {
            // fp32 engine: the block's last tensor is read by the up-convolution only -> planes only
            Act y = (r == 2 && b.has_up && plane_gemm(b.cout, b.cout)) ? new_act3(x.n, x.h, x.w, b.cout, 2) : new_act(x.n, x.h, x.w, b.cout);
            res_block(b.res[r], x, y, 0);
            release(x);
            x = y;
        }
        if (b.has_up) {
            // the next block's first ResnetBlock has a 1x1 shortcut (cin != cout): it reads the up-convolution's output as planes too
            const bool both = i + 1 < 4 && dec_blocks_[i + 1].res[0].has_skip && plane_gemm(b.cout, dec_blocks_[i + 1].cout);
            Act y = both ? new_act3(x.n, x.h * 2, x.w * 2, b.cout, 3) : new_act(x.n, x.h * 2, x.w * 2, b.cout);
            conv_raw(b.upsampler, x, y, 1, 1);
            release(x);
            x = y;
        }
    }
    Act gn = new_act(x.n, x.h, x.w, x.c);
    group_norm(dec_norm_out_, x, gn, true);
    release(x);
    conv(dec_conv_out_, gn, img, 1, 0, nullptr, 0, nullptr);
    release(gn);
}

// Autoencoder::encode_image (autoencoder/mod.rs:60-66): Encoder::forward (:133-144) -> quant_conv -> channels 0..3
// (the posterior mean; the reference does not sample).  One image at a time, like the decoder.
void Engine::encode_image_dev(const float* img_nchw, int n, float* latent_nchw) {
    if (!finalized_) throw Error(SDMI_ERR_STATE, "weights not finalized");
    if (!enc_ready_) throw Error(SDMI_ERR_STATE, "VAE encoder weights are not loaded (autoencoder/encoder/..., autoencoder/quant_conv)");
    if (n <= 0) throw Error(SDMI_ERR_INVALID, "encode_image: n must be positive");
    check_batch(n);
    const int H = 8 * lat_h_, W = 8 * lat_w_;
    const size_t img_elems = (size_t)3 * H * W, lat_elems = (size_t)4 * lat_h_ * lat_w_;
    for (int i = 0; i < n; ++i) {
        Act rgb = new_act(1, H, W, 4, /*dt=*/0);
        SDMI_LAUNCH(launch_nchw3_to_nhwc4(img_nchw + i * img_elems, rgb.p, 1, H, W, stream_));
        Act q8 = encode_one(rgb);
        // latent.slice([0..n, 0..4]): the first 4 of the 8 channels, NHWC8 -> NCHW4
        SDMI_LAUNCH(launch_nhwc_to_nchw_slice(q8.p, latent_nchw + i * lat_elems, 1, 8, 4, q8.h, q8.w, stream_));
        release(q8);
    }
}

Act Engine::encode_one(Act& rgb) {
    Act x = new_act(1, rgb.h, rgb.w, enc_conv_in_.cout);
    conv(enc_conv_in_, rgb, x, 1, 0, nullptr, 0, nullptr);
    release(rgb);
    for (int bi = 0; bi < 4; ++bi) {  // EncoderBlock::forward (:257-265)
        const EncBlockW& b = enc_blocks_[bi];
        for (int r = 0; r < 2; ++r) {
            Act y = new_act(x.n, x.h, x.w, b.cout);
            res_block(b.res[r], x, y, 0);
            release(x);
            x = y;
        }
        if (b.has_down) {
            Act y = new_act(x.n, x.h / 2, x.w / 2, b.cout);
            conv(b.down, x, y, 2, 0, nullptr, 0, nullptr, /*pad_br=*/true);
            release(x);
            x = y;
        }
    }
    {   // Mid (:457-462)
        Act a = new_act(x.n, x.h, x.w, x.c); res_block(enc_mid1_, x, a, 0); release(x);
        Act b = new_act(a.n, a.h, a.w, a.c); vae_attn(enc_attn_, a, b); release(a);
        Act c = new_act(b.n, b.h, b.w, b.c); res_block(enc_mid2_, b, c, 0); release(b);
        x = c;
    }
    Act gn = new_act(x.n, x.h, x.w, x.c);
    group_norm(enc_norm_out_, x, gn, true);
    release(x);
    Act m8 = new_act(gn.n, gn.h, gn.w, 8, /*dt=*/0);   // moments stay fp32 in both precisions
    conv(enc_conv_out_, gn, m8, 1, 0, nullptr, 0, nullptr);
    release(gn);
    Act q8 = new_act(m8.n, m8.h, m8.w, 8, /*dt=*/0);
    conv(quant_conv_, m8, q8, 1, 0, nullptr, 0, nullptr);
    release(m8);
    return q8;
}

// in_scale = 1/0.18215 for latent_to_image (stablediffusion/mod.rs:71), 1 for decode_latent.
// Exactly one of img_nchw / rgb_u8 is written.
void Engine::decode_latent_dev(const float* latent_nchw, int n, float in_scale, float* img_nchw, uint8_t* rgb_u8) {
    if (!finalized_) throw Error(SDMI_ERR_STATE, "weights not finalized");
    if (n <= 0) throw Error(SDMI_ERR_INVALID, "decode: n must be positive");
    check_batch(n);
    const int H = lat_h_, W = lat_w_;
    const size_t lat_elems = (size_t)4 * H * W, img_elems = (size_t)3 * 64 * H * W;
    for (int i = 0; i < n; ++i) {  // one image at a time: peak activations are ~1 GB per image at 512x512
        Buf z(this, lat_elems * 4);
        SDMI_LAUNCH(launch_nchw_to_nhwc(latent_nchw + i * lat_elems, z.f(), 1, 4, H, W, in_scale, stream_));
        Act img = new_act(1, 8 * H, 8 * W, 3, /*dt=*/0);  // RGB stays fp32 (conv_out writes fp32 in both precisions)
        decode_one(z.f(), 1, img);
        if (rgb_u8) SDMI_LAUNCH(launch_image_to_u8(img.p, rgb_u8 + i * img_elems, (long long)img_elems, stream_));
        else SDMI_LAUNCH(launch_nhwc_to_nchw(img.p, img_nchw + i * img_elems, 1, 3, 8 * H, 8 * W, stream_));
        release(img);
    }
}

// ---- IP-Adapter (include/sdmi.h "IP-Adapter") ------------------------------------------------------------------------
void Engine::ip_adapter_layer(int model_channels, int ctx_index, int* j, int* c) {
    if (ctx_index < 0 || ctx_index >= kIpLayers) throw Error(SDMI_ERR_INVALID, "ip_adapter: ctx_index must be 0 .. 15");
    // st_list_ order (build_model): input blocks 1, 2, 4, 5, 7, 8 -- the middle block -- output blocks 3 .. 11; the file counts down, up, mid
    static const int kMul[kIpLayers] = {1, 1, 2, 2, 4, 4, 4, 4, 4, 4, 2, 2, 2, 1, 1, 1};
    const int rank = ctx_index < 6 ? ctx_index : (ctx_index == 6 ? 15 : ctx_index - 1);
    if (j) *j = 2 * rank + 1;
    if (c) *c = kMul[ctx_index] * model_channels;
}

std::string Engine::ip_adapter_key(int model_channels, int ctx_index, int which) {
    if (which != 0 && which != 1) throw Error(SDMI_ERR_INVALID, "ip_adapter_key: which must be 0 (to_k_ip) or 1 (to_v_ip)");
    int j = 0;
    ip_adapter_layer(model_channels, ctx_index, &j, nullptr);
    return "ip_adapter." + std::to_string(j) + (which ? ".to_v_ip.weight" : ".to_k_ip.weight");
}

void Engine::ip_set_weights(const IpTensor& proj_w, const IpTensor& proj_b, const IpTensor& norm_g, const IpTensor& norm_b, int D, int T, const IpTensor* wk,
                            const IpTensor* wv) {
    SDMI_HIP(hipSetDevice(cfg_.device));
    const int cd = cfg_.ctx_dim, mc = cfg_.model_channels;
    if (!proj_w.p || !proj_b.p || !norm_g.p || !norm_b.p || !wk || !wv) throw Error(SDMI_ERR_INVALID, "ip_adapter: null pointer");
    if (T < 1 || T > kIpMaxTokens) throw Error(SDMI_ERR_INVALID, "ip_adapter: T (tokens per image) must be 1 .. 64");
    if (D < 32 || D % 32) throw Error(SDMI_ERR_INVALID, "ip_adapter: D (the image embedding's width) must be a positive multiple of 32");
    if ((int)n_st_unet_ != kIpLayers || st_list_[6] != &mid_st_) throw Error(SDMI_ERR_STATE, "ip_adapter: the layer rule is stated for 16 cross attentions");
    for (int i = 0; i < kIpLayers; ++i) {
        if (!wk[i].p || !wv[i].p) throw Error(SDMI_ERR_INVALID, "ip_adapter: null layer weight");
        int c = 0;
        ip_adapter_layer(mc, i, nullptr, &c);
        const SpatialW& st = *st_list_[(size_t)i];
        if (st.c != c) throw Error(SDMI_ERR_STATE, "ip_adapter: the layer rule does not match this model's cross attention " + std::to_string(i));
        if (!ip_attention_head_dim(c / unet_heads(c)))
            throw Error(SDMI_ERR_UNSUPPORTED, "ip_adapter: head width " + std::to_string(c / unet_heads(c)) + " of cross attention " + std::to_string(i) + " (40, 64, 80, 160 are served)");
    }
    IpWeights nw;
    nw.D = D; nw.T = T;
    auto dalloc = [&](size_t bytes) { void* p = nullptr; SDMI_HIP(hipMalloc(&p, bytes)); nw.allocs.push_back(p); return static_cast<float*>(p); };
    // raw bytes -> device -> fp32 by k_unpack.hip (a Linear weight: torch [out, in] -> [in, out]) -> the loader's Linear packing
    auto widen = [&](const IpTensor& t, long long d0, long long d1, int transform, float* out) {
        if (t.dtype < 0 || t.dtype > 2) throw Error(SDMI_ERR_INVALID, "ip_adapter: element type must be F32, F16 or BF16");
        const size_t bytes = (size_t)d0 * d1 * (t.dtype ? 2 : 4);
        Buf raw(this, bytes);
        SDMI_HIP(hipMemcpyAsync(raw.p, t.p, bytes, hipMemcpyHostToDevice, stream_));
        SDMI_HIP(launch_unpack_tensor(raw.p, t.dtype, transform, d0, d1, out, stream_));
        SDMI_HIP(hipStreamSynchronize(stream_));   // the host bytes (a mapped file) and the staging block are free again
    };
    auto linear = [&](const IpTensor& t, int cin, int cout) {
        float* bt = dalloc((size_t)cin * cout * 4);
        Buf stage(this, (size_t)cin * cout * 4);
        widen(t, cout, cin, 1, stage.f());
        SDMI_HIP(launch_pack_linear_weight(stage.f(), bt, cin, cout, stream_));
        SDMI_HIP(hipStreamSynchronize(stream_));
        return bt;
    };
    try {
        nw.proj_bt = linear(proj_w, D, T * cd);
        nw.proj_b = dalloc((size_t)T * cd * 4);
        widen(proj_b, (long long)T * cd, 1, 0, nw.proj_b);
        nw.norm.c = cd; nw.norm.eps = 1e-5f;
        nw.norm.gamma = dalloc((size_t)cd * 4);
        nw.norm.beta = dalloc((size_t)cd * 4);
        widen(norm_g, cd, 1, 0, nw.norm.gamma);
        widen(norm_b, cd, 1, 0, nw.norm.beta);
        for (int i = 0; i < kIpLayers; ++i) {
            const int c = st_list_[(size_t)i]->c;
            nw.kbt.push_back(linear(wk[i], cd, c));
            nw.vbt.push_back(linear(wv[i], cd, c));
        }
        ip_clear();   // the old adapter and a setting made for it; in here, so that its refusal frees the new blocks
    } catch (...) {
        (void)hipStreamSynchronize(stream_);
        for (void* p : nw.allocs) (void)hipFree(p);
        throw;
    }
    nw.ready = true;
    ipw_ = std::move(nw);
}

void Engine::ip_clear() {
    SDMI_HIP(hipSetDevice(cfg_.device));
    SDMI_HIP(hipStreamSynchronize(stream_));
    set_ip_adapter(nullptr);
    for (void* p : ipw_.allocs) (void)hipFree(p);
    ipw_ = IpWeights{};
}

// every refusal of sdmi_ip_adapter_load_safetensors, host only: the file against a model with mc model channels and a cd-wide context
void Engine::ip_check_safetensors(const char* path, int mc, int cd, int* D_out, int* T_out) {
    if (!path) throw Error(SDMI_ERR_INVALID, "ip_adapter: null path");
    const std::string ps(path);
    auto ends_with = [&](const char* suf) { const size_t n = std::strlen(suf); return ps.size() >= n && ps.compare(ps.size() - n, n, suf) == 0; };
    if (ends_with(".bin") || ends_with(".pt") || ends_with(".pth") || ends_with(".ckpt"))
        throw Error(SDMI_ERR_UNSUPPORTED, "ip_adapter: '" + ps + "' is a pickle file; convert it to .safetensors");
    {   // a pickle under another name.  A .safetensors file opens with its header's length as a little-endian u64, and any byte can stand there: so only a file
        // that cannot be one (the header would pass the file's end, or does not open with '{') is looked at for a zip archive's or a pickle stream's signature
        unsigned char m[9] = {0};
        if (FILE* f = std::fopen(path, "rb")) {
            const size_t got = std::fread(m, 1, 9, f);
            long long size = -1;
            if (std::fseek(f, 0, SEEK_END) == 0) size = (long long)std::ftell(f);
            std::fclose(f);
            uint64_t hlen = 0;
            for (int i = 7; i >= 0; --i) hlen = (hlen << 8) | m[i];
            const bool plausible = got == 9 && size >= 9 && hlen >= 2 && hlen <= (uint64_t)size - 8 && m[8] == '{';
            const bool zip = got >= 4 && m[0] == 'P' && m[1] == 'K' && m[2] == 3 && m[3] == 4;
            const bool pickle = got >= 2 && m[0] == 0x80 && m[1] >= 2 && m[1] <= 5;
            if (!plausible && (zip || pickle)) throw Error(SDMI_ERR_UNSUPPORTED, "ip_adapter: '" + ps + "' is a pickle file; convert it to .safetensors");
        }
    }
    SafetensorsFile file(ps);
    auto dtype_of = [&](const StTensor& t) {
        if (t.dtype == "F32") return 0;
        if (t.dtype == "F16") return 1;
        if (t.dtype == "BF16") return 2;
        throw Error(SDMI_ERR_WEIGHTS, "ip_adapter: '" + t.key + "' has dtype " + t.dtype + " (F32, F16, BF16 are read)");
    };
    auto shape_str = [](const std::vector<int64_t>& sh) { std::string o = "["; for (size_t i = 0; i < sh.size(); ++i) o += (i ? ", " : "") + std::to_string(sh[i]); return o + "]"; };
    std::map<std::string, std::vector<int64_t>> want;   // every key the adapter has, with the shape this model needs (the projection's: checked below)
    for (int i = 0; i < kIpLayers; ++i) {
        int c = 0;
        ip_adapter_layer(mc, i, nullptr, &c);
        want[ip_adapter_key(mc, i, 0)] = {c, cd};
        want[ip_adapter_key(mc, i, 1)] = {c, cd};
    }
    for (const StTensor& t : file.tensors()) {
        if (t.key.rfind("image_proj.latents", 0) == 0 || t.key.rfind("image_proj.layers.", 0) == 0 || t.key.rfind("image_proj.proj_in", 0) == 0 || t.key.rfind("image_proj.proj_out", 0) == 0)
            throw Error(SDMI_ERR_UNSUPPORTED, "ip_adapter: '" + t.key + "' belongs to the \"plus\" Resampler; project outside and pass tokens");
        if (t.key.rfind("ip_adapter.", 0) == 0 && !want.count(t.key)) throw Error(SDMI_ERR_WEIGHTS, "ip_adapter: '" + t.key + "' is not a layer of this model");
    }
    auto need = [&](const std::string& key) -> const StTensor& {
        const StTensor* t = file.find(key);
        if (!t) throw Error(SDMI_ERR_WEIGHTS, "ip_adapter: '" + key + "' is missing");
        (void)dtype_of(*t);
        return *t;
    };
    const StTensor& pw = need("image_proj.proj.weight");
    if (pw.shape.size() != 2 || pw.shape[0] < cd || pw.shape[0] % cd || pw.shape[0] / cd > kIpMaxTokens || pw.shape[1] < 32 || pw.shape[1] % 32)
        throw Error(SDMI_ERR_WEIGHTS, "ip_adapter: 'image_proj.proj.weight' is " + shape_str(pw.shape) + ", need [T x " + std::to_string(cd) + ", D] with T <= 64 and D a multiple of 32");
    const int T = (int)(pw.shape[0] / cd), D = (int)pw.shape[1];
    want["image_proj.proj.bias"] = {(int64_t)T * cd};
    want["image_proj.norm.weight"] = {cd};
    want["image_proj.norm.bias"] = {cd};
    for (auto& kv : want) {
        const StTensor& t = need(kv.first);
        if (t.shape != kv.second) throw Error(SDMI_ERR_WEIGHTS, "ip_adapter: '" + kv.first + "' is " + shape_str(t.shape) + ", this model needs " + shape_str(kv.second));
    }
    if (D_out) *D_out = D;
    if (T_out) *T_out = T;
}

void Engine::ip_load_safetensors(const char* path) {
    const int cd = cfg_.ctx_dim, mc = cfg_.model_channels;
    int D = 0, T = 0;
    ip_check_safetensors(path, mc, cd, &D, &T);   // the whole file, before anything is uploaded
    SafetensorsFile file(path);
    auto src = [&](const std::string& key) {
        const StTensor* t = file.find(key);
        if (!t) throw Error(SDMI_ERR_WEIGHTS, "ip_adapter: '" + key + "' is missing");
        return IpTensor{t->data, t->dtype == "F32" ? 0 : t->dtype == "F16" ? 1 : 2};
    };
    IpTensor wk[kIpLayers], wv[kIpLayers];
    for (int i = 0; i < kIpLayers; ++i) { wk[i] = src(ip_adapter_key(mc, i, 0)); wv[i] = src(ip_adapter_key(mc, i, 1)); }
    ip_set_weights(src("image_proj.proj.weight"), src("image_proj.proj.bias"), src("image_proj.norm.weight"), src("image_proj.norm.bias"), D, T, wk, wv);
}

void Engine::ip_image_tokens_dev(const float* embeds, int n, float* out) {
    if (!ipw_.ready) throw Error(SDMI_ERR_STATE, "ip_image_tokens: no adapter is loaded");
    if (n < 1) throw Error(SDMI_ERR_INVALID, "ip_image_tokens: n must be at least 1");
    const int cd = cfg_.ctx_dim, T = ipw_.T;
    Act lin = new_rows(n, T * cd, 1, 0);   // fp32 at every precision, like the adapter's weights
    linear(LinW{ipw_.proj_bt, ipw_.proj_b, ipw_.D, T * cd}, rows_view(embeds, n, ipw_.D, 0), lin);
    layer_norm(ipw_.norm, rows_view(lin.p, (long long)n * T, cd, 0), rows_view(out, (long long)n * T, cd, 0));
    release(lin);
}

void Engine::check_ip_adapter(const sdmi_ip_adapter& a) {
    if ((a.tokens != nullptr) == (a.embeds != nullptr)) throw Error(SDMI_ERR_INVALID, "ip_adapter: give exactly one of tokens and embeds");
    if (a.n_sets < 1) throw Error(SDMI_ERR_INVALID, "ip_adapter: n_sets must be at least 1");
    if (a.T_ip < 1) throw Error(SDMI_ERR_INVALID, "ip_adapter: T_ip must be at least 1");
    if (a.T_ip > kIpMaxTokens) throw Error(SDMI_ERR_UNSUPPORTED, "ip_adapter: more than 64 image tokens");
    if (!std::isfinite(a.scale)) throw Error(SDMI_ERR_INVALID, "ip_adapter: scale must be finite");
    if (!(a.start >= 0.0 && a.start <= a.end && a.end <= 1.0)) throw Error(SDMI_ERR_INVALID, "ip_adapter: the step window must satisfy 0 <= start <= end <= 1");
}

// every refusal of set_ip_adapter: the arguments, then against this context's adapter.  Host only, changes nothing.
void Engine::check_ip_setting(const sdmi_ip_adapter& a) const {
    check_ip_adapter(a);
    if (!ipw_.ready) throw Error(SDMI_ERR_STATE, "set_ip_adapter: no adapter is loaded (sdmi_ip_adapter_load_safetensors / sdmi_ip_adapter_set_weights)");
    const int cd = cfg_.ctx_dim, T = ipw_.T;
    if ((a.tokens || a.neg_tokens) && a.token_dim != cd)
        throw Error(SDMI_ERR_INVALID, "ip_adapter: tokens are " + std::to_string(a.token_dim) + " wide, ctx_dim is " + std::to_string(cd));
    if (a.embeds && a.embed_dim != ipw_.D) throw Error(SDMI_ERR_INVALID, "ip_adapter: embeds are " + std::to_string(a.embed_dim) + " wide, the adapter's D is " + std::to_string(ipw_.D));
    if (a.embeds && a.T_ip % T) throw Error(SDMI_ERR_INVALID, "ip_adapter: with embeds T_ip must be a multiple of the adapter's T = " + std::to_string(T));
}

void Engine::set_ip_adapter(const sdmi_ip_adapter* a) {
    SDMI_HIP(hipSetDevice(cfg_.device));
    if (!a) {
        SDMI_HIP(hipStreamSynchronize(stream_));
        if (ip_.tokens) (void)hipFree(ip_.tokens);
        if (ip_.neg) (void)hipFree(ip_.neg);
        ip_ = IpState{};
        return;
    }
    check_ip_setting(*a);
    const int cd = cfg_.ctx_dim, T = ipw_.T, Tip = a->T_ip;
    const size_t set_elems = (size_t)Tip * cd;
    IpState ns;
    ns.set = true; ns.n_sets = a->n_sets; ns.T_ip = Tip; ns.scale = a->scale; ns.start = a->start; ns.end = a->end; ns.neg_given = a->neg_tokens != nullptr;
    ns.neg_sets = a->neg_tokens ? a->n_sets : 1;
    try {
        SDMI_HIP(hipMalloc((void**)&ns.tokens, (size_t)ns.n_sets * set_elems * 4));
        SDMI_HIP(hipMalloc((void**)&ns.neg, (size_t)ns.neg_sets * set_elems * 4));
        if (a->tokens) SDMI_HIP(hipMemcpyAsync(ns.tokens, a->tokens, (size_t)ns.n_sets * set_elems * 4, hipMemcpyHostToDevice, stream_));
        else {
            const int rows = ns.n_sets * (Tip / T);
            Buf e(this, (size_t)rows * ipw_.D * 4);
            SDMI_HIP(hipMemcpyAsync(e.p, a->embeds, (size_t)rows * ipw_.D * 4, hipMemcpyHostToDevice, stream_));
            ip_image_tokens_dev(e.f(), rows, ns.tokens);
        }
        if (a->neg_tokens) SDMI_HIP(hipMemcpyAsync(ns.neg, a->neg_tokens, (size_t)ns.neg_sets * set_elems * 4, hipMemcpyHostToDevice, stream_));
        else {   // image_proj(0), its T tokens repeated along the token axis
            Buf z(this, (size_t)ipw_.D * 4), t0(this, (size_t)T * cd * 4);
            SDMI_HIP(hipMemsetAsync(z.p, 0, (size_t)ipw_.D * 4, stream_));
            ip_image_tokens_dev(z.f(), 1, t0.f());
            for (int t = 0; t < Tip; t += T)
                SDMI_HIP(hipMemcpyAsync(ns.neg + (size_t)t * cd, t0.f(), (size_t)std::min(T, Tip - t) * cd * 4, hipMemcpyDeviceToDevice, stream_));
        }
        SDMI_HIP(hipStreamSynchronize(stream_));
    } catch (...) {
        (void)hipStreamSynchronize(stream_);
        if (ns.tokens) (void)hipFree(ns.tokens);
        if (ns.neg) (void)hipFree(ns.neg);
        throw;
    }
    if (ip_.tokens) (void)hipFree(ip_.tokens);
    if (ip_.neg) (void)hipFree(ip_.neg);
    ip_ = ns;
}

// sdmi_set_ip_adapter_file: the tensor "image_embeds" [n, D] (F32 / F16 / BF16) of a .safetensors file, widened on the host, as ONE set of n pictures
void Engine::set_ip_adapter_file(const char* path, float scale, double start, double end) {
    if (!path) throw Error(SDMI_ERR_INVALID, "ip_adapter: null path");
    if (!ipw_.ready) throw Error(SDMI_ERR_STATE, "set_ip_adapter: no adapter is loaded (sdmi_ip_adapter_load_safetensors / sdmi_ip_adapter_set_weights)");
    SafetensorsFile file(path);
    const StTensor* t = file.find("image_embeds");
    if (!t) throw Error(SDMI_ERR_WEIGHTS, std::string("ip_adapter: '") + path + "' holds no tensor 'image_embeds'");
    if (t->shape.size() != 2 || t->shape[0] < 1 || t->shape[1] != ipw_.D)
        throw Error(SDMI_ERR_INVALID, "ip_adapter: 'image_embeds' must be [n, " + std::to_string(ipw_.D) + "]");
    if (t->shape[0] * ipw_.T > kIpMaxTokens) throw Error(SDMI_ERR_UNSUPPORTED, "ip_adapter: more than 64 image tokens");
    std::vector<float> e(t->count);
    if (t->dtype == "F32") std::memcpy(e.data(), t->data, t->count * 4);
    else if (t->dtype == "BF16" || t->dtype == "F16") {
        const bool bf = t->dtype == "BF16";
        for (size_t i = 0; i < t->count; ++i) {
            uint16_t h;
            std::memcpy(&h, t->data + 2 * i, 2);
            uint32_t u;
            if (bf) u = (uint32_t)h << 16;
            else {   // IEEE half -> float, exact
                const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 1023u;
                if (ex == 31) u = sign | 0x7f800000u | (man << 13);
                else if (ex) u = sign | ((ex + 112u) << 23) | (man << 13);
                else if (!man) u = sign;
                else { int sh = 0; uint32_t m = man; while (!(m & 1024u)) { m <<= 1; ++sh; } u = sign | ((113u - sh) << 23) | ((m & 1023u) << 13); }
            }
            std::memcpy(&e[i], &u, 4);
        }
    } else throw Error(SDMI_ERR_WEIGHTS, "ip_adapter: 'image_embeds' has dtype " + t->dtype + " (F32, F16, BF16 are read)");
    sdmi_ip_adapter a{};
    a.embeds = e.data(); a.n_sets = 1; a.T_ip = (int32_t)t->shape[0] * ipw_.T; a.embed_dim = ipw_.D; a.scale = scale; a.start = start; a.end = end;
    check_ip_adapter(a);
    set_ip_adapter(&a);
}

bool Engine::get_ip_adapter(sdmi_ip_adapter* out) const {
    if (!ip_.set) return false;
    if (out) {
        *out = sdmi_ip_adapter{};
        out->n_sets = ip_.n_sets; out->T_ip = ip_.T_ip; out->token_dim = cfg_.ctx_dim; out->embed_dim = ipw_.D;
        out->scale = ip_.scale; out->start = ip_.start; out->end = ip_.end;
    }
    return true;
}

// K_ip / V_ip of the nb batch rows of the call, once per call: image i of either half reads token set i mod n_sets, the unconditional half (the first n_images rows of
// a 2 n_images batch) the negative tokens.  fp32 at every precision: the adapter's matrices are packed for the fp32 GEMM.
void Engine::ip_prepare(int nb, int n_images, const std::function<void*(size_t)>& own) {
    if (!ipw_.ready) throw Error(SDMI_ERR_STATE, "ip_adapter: the adapter's weights are gone");
    const int cd = cfg_.ctx_dim, Tip = ip_.T_ip;
    const size_t set_elems = (size_t)Tip * cd;
    Buf rows(this, (size_t)nb * set_elems * 4);
    for (int b = 0; b < nb; ++b) {
        const bool uncond = nb == 2 * n_images && b < n_images;
        const int img = b % n_images;
        const float* src = uncond ? ip_.neg + (size_t)(img % ip_.neg_sets) * set_elems : ip_.tokens + (size_t)(img % ip_.n_sets) * set_elems;
        SDMI_HIP(hipMemcpyAsync(rows.f() + (size_t)b * set_elems, src, set_elems * 4, hipMemcpyDeviceToDevice, stream_));
    }
    us_.kip.resize(kIpLayers);
    us_.vip.resize(kIpLayers);
    const Act tokens = rows_view(rows.p, nb * Tip, cd, 0);
    for (int i = 0; i < kIpLayers; ++i) {
        const int c = st_list_[(size_t)i]->c;
        us_.kip[i] = (float*)own((size_t)nb * Tip * c * 4);
        us_.vip[i] = (float*)own((size_t)nb * Tip * c * 4);
        linear(LinW{ipw_.kbt[(size_t)i], nullptr, cd, c}, tokens, rows_view(us_.kip[i], nb * Tip, c, 0));
        linear(LinW{ipw_.vbt[(size_t)i], nullptr, cd, c}, tokens, rows_view(us_.vip[i], nb * Tip, c, 0));
    }
    us_.ip_s_host.assign((size_t)nb, ip_.scale);
    us_.ip_s = (float*)own((size_t)nb * 4);
    SDMI_HIP(hipMemcpyAsync(us_.ip_s, us_.ip_s_host.data(), (size_t)nb * 4, hipMemcpyHostToDevice, stream_));
}

void Engine::ip_attention(const SpatialW& w, const Act& qa, const Act& oa, int nb, int hw, int heads, int d) {
    const float* q = qa.p; float* o = oa.p; void* o3 = oa.p3;
    if (!ip_live_ || w.ctx_index < 0 || w.ctx_index >= (int)us_.kip.size()) return;
    if (nb != us_.nb) throw Error(SDMI_ERR_STATE, "ip_attention: batch mismatch");
    IpAttnParams p{};
    p.q = q; p.k = us_.kip[(size_t)w.ctx_index]; p.v = us_.vip[(size_t)w.ctx_index]; p.s = us_.ip_s;
    p.o_text = o3 ? o3 : (void*)o; p.o = o3 ? o3 : (void*)o;
    p.n = nb; p.nq = hw; p.T = ip_.T_ip; p.n_head = heads; p.d_head = d;
    p.ldq = heads * d; p.q_bs = (long long)hw * heads * d;
    p.ldo3 = (heads * d / 32) * 192;
    p.bf16 = edt(); p.form = o3 ? 2 : (edt() ? 1 : 0);
    p.q_log2 = q_prescaled(edt(), d) ? 1 : 0;
    p.scale = (float)std::pow((double)d, -0.25);
    const double fl = 4.0 * nb * heads * (double)hw * p.T * d;
    ProfScope ps(this, PC_ATTENTION, fl, 0);
    ps.set_tag("ip_attention n%d nq%d T%d h%d d%d", nb, hw, p.T, heads, d);
    SDMI_LAUNCH_IN(ps, fl, launch_ip_attention(p, stream_));
}

size_t Engine::ip_kv_elems(int nb) const {
    size_t e = 0;
    for (int i = 0; i < kIpLayers && i < (int)n_st_unet_; ++i) e += 2 * (size_t)nb * ip_.T_ip * st_list_[(size_t)i]->c;
    return e;
}

void Engine::ip_kv_dev(int n_images, bool cfg_pair, float* out) {
    if (!ip_.set) throw Error(SDMI_ERR_STATE, "ip_kv: no adapter is set");
    if (n_images < 1) throw Error(SDMI_ERR_INVALID, "ip_kv: n must be at least 1");
    const int nb = cfg_pair ? 2 * n_images : n_images;
    unet_release();
    us_.nb = nb;
    ip_prepare(nb, n_images, [&](size_t bytes) { void* p = pool_.alloc(bytes); us_.owned.push_back(p); return p; });
    size_t off = 0;
    for (int i = 0; i < kIpLayers; ++i) {
        const size_t e = (size_t)nb * ip_.T_ip * st_list_[(size_t)i]->c;
        SDMI_HIP(hipMemcpyAsync(out + off, us_.kip[(size_t)i], e * 4, hipMemcpyDeviceToDevice, stream_));
        SDMI_HIP(hipMemcpyAsync(out + off + e, us_.vip[(size_t)i], e * 4, hipMemcpyDeviceToDevice, stream_));
        off += 2 * e;
    }
    SDMI_HIP(hipStreamSynchronize(stream_));
    unet_release();
}

}  // namespace sdmi
