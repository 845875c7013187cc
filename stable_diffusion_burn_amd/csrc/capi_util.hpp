// capi_util.hpp -- what the translation units of the C ABI (sdmi_capi.cpp, sdmi_capi_ops.cpp) share: exceptions -> status codes, the context's engine, host <->
// device staging.  Internal; no kernel unit includes it.
#pragma once
#include <memory>
#include <string>

#include "engine.hpp"

using sdmi::Engine;
using sdmi::Error;

template <class F>
static int guarded(F&& f) {
    try {
        f();
        return SDMI_OK;
    } catch (const Error& e) {
        sdmi::set_last_error(e.what());
        return e.status;
    } catch (const std::exception& e) {
        sdmi::set_last_error(std::string("internal error: ") + e.what());
        return SDMI_ERR_INVALID;
    } catch (...) {
        sdmi::set_last_error("unknown internal error");
        return SDMI_ERR_INVALID;
    }
}

static Engine& eng(sdmi_ctx* c) {
    if (!c || !c->engine) throw Error(SDMI_ERR_INVALID, "null sdmi_ctx");
    return *c->engine;
}

namespace {
// host <-> device staging on the context stream
struct DevIn {
    Engine::Buf buf;
    DevIn(Engine& e, const void* host, size_t bytes) : buf(&e, bytes) {
        if (!host) throw Error(SDMI_ERR_INVALID, "null input pointer");
        SDMI_HIP(hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, e.stream()));
    }
    const float* f() const { return buf.f(); }
};
struct DevOut {
    Engine& e; Engine::Buf buf; void* host; size_t bytes;
    DevOut(Engine& e_, void* host_, size_t bytes_) : e(e_), buf(&e_, bytes_), host(host_), bytes(bytes_) {
        if (!host) throw Error(SDMI_ERR_INVALID, "null output pointer");
    }
    void fetch() {
        SDMI_HIP(hipMemcpyAsync(host, buf.p, bytes, hipMemcpyDeviceToHost, e.stream()));
        SDMI_HIP(hipStreamSynchronize(e.stream()));
    }
    float* f() const { return buf.f(); }
};
}  // namespace

// optional host input (mask, noise): staged when given
static std::unique_ptr<DevIn> dev_in_opt(Engine& e, const void* host, size_t bytes) {
    return host ? std::unique_ptr<DevIn>(new DevIn(e, host, bytes)) : nullptr;
}
