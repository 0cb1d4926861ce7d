// mem.hip -- the one owner of device and pinned-host memory (Mem) and the grow-on-demand buffer built on it (Scratch): internal.h
#include "internal.h"
#include <algorithm>

namespace trexhip {

int Mem::alloc(void** p, size_t bytes, bool pinned, const char* who) {
    *p = nullptr;
    if (bytes == 0) bytes = 1;
    const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    if (e != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();   // clear the sticky error: the caller may free something and try again
        const char* what = pinned ? "pinned host" : "device";
        if (e == hipErrorOutOfMemory) { set_error(std::string(who) + ": out of " + what + " memory"); return TREXHIP_E_NOMEM; }
        set_error(std::string(who) + ": allocating " + what + " memory: " + hipGetErrorString(e));
        return TREXHIP_E_DEVICE;
    }
    (pinned ? host : dev).push_back(*p);
    return TREXHIP_OK;
}

void Mem::release(void* d) {
    const auto it = std::find(dev.begin(), dev.end(), d);
    if (it == dev.end()) return;
    (void)hipFree(d);
    dev.erase(it);
}

void Mem::free_all() {
    for (void* d : dev) (void)hipFree(d);
    for (void* h : host) (void)hipHostFree(h);
    dev.clear();
    host.clear();
}

int Scratch::reserve(trexhip_ctx* ctx, size_t need, const char* who) {
    if (p && need <= bytes) return TREXHIP_OK;
    if (p) {
        TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        ctx->mem.release(p);
        p = nullptr; bytes = 0;
    }
    const int rc = ctx->mem.device_bytes(&p, need, who);
    if (rc == TREXHIP_OK) bytes = need;
    return rc;
}

int ensure_staging(trexhip_ctx* ctx, const char* who) {
    if (ctx->d_staging) return TREXHIP_OK;
    return ctx->mem.device(&ctx->d_staging, (size_t)ctx->p.max_batch * ctx->p.width * ctx->p.height + 16, who);
}

}  // namespace trexhip
