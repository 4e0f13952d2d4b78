// Test-only stage access to a live decode engine (wmar_{gpt,rar,cham}_probe_*): what the three engines' entries share.  An engine
// states its own buffer table, stage switch and plan text; the argument checks, the copy and the waiting are here, once.  `who` is
// the entry's name as the error texts print it ("gpt_probe_copy").
#pragma once
#include "common.h"

namespace wmar {

struct ProbeBuf { const char* name; void* ptr; size_t bytes; };

// The contract of *_probe_copy (include/wmar_hip.h) behind an engine's table of `n` buffers.
inline int64_t probe_copy(const char* who, const ProbeBuf* bufs, size_t n, const char* name, void* ptr_dev, int64_t bytes,
                          int32_t to_engine, hipStream_t st) {
    const ProbeBuf* b = nullptr;
    for (size_t i = 0; i < n && !b; ++i)
        if (!strcmp(bufs[i].name, name)) b = &bufs[i];
    if (!b) { set_error("%s: unknown buffer '%s'", who, name); return WMAR_EINVAL; }
    if (!b->ptr) { set_error("%s: this engine has no buffer '%s' (its shape is not eligible for the kernel that uses it)", who, name); return WMAR_EINVAL; }
    const size_t sz = b->bytes;
    if (!ptr_dev) return (int64_t)sz;
    if (bytes != (int64_t)sz) { set_error("%s: '%s' holds %zu bytes, caller passed %lld", who, name, sz, (long long)bytes); return WMAR_EINVAL; }
    hipError_t e = to_engine ? hipMemcpyAsync(b->ptr, ptr_dev, sz, hipMemcpyDeviceToDevice, st)
                             : hipMemcpyAsync(ptr_dev, b->ptr, sz, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(e)); return WMAR_EHIP; }
    return (int64_t)sz;
}

// 0 <= first <= last <= head_stage, and the HEAD stage writes logits_dev
inline int probe_stage_range(const char* who, int first, int last, int head_stage, const void* logits_dev) {
    WMAR_REQUIRE(first >= 0 && last <= head_stage && first <= last, "%s: stages %d..%d", who, first, last);
    WMAR_REQUIRE(last < head_stage || logits_dev, "%s: the HEAD stage needs logits_dev", who);
    return WMAR_OK;
}

// The tail of *_probe_run: waits for the stream whatever `rc` says; an earlier error wins over the one of the wait.
inline int probe_wait(const char* who, int rc, hipStream_t st) {
    const hipError_t e = hipStreamSynchronize(st);
    if (rc == WMAR_OK && e != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(e)); rc = WMAR_EHIP; }
    return rc;
}

// "EMBED,QKV,...": the names of the stages 0..n-1 for which has(stage) holds
template <typename Pred>
std::string probe_stage_list(const char* const* names, int n, Pred has) {
    std::string s;
    for (int i = 0; i < n; ++i)
        if (has(i)) s += std::string(s.empty() ? "" : ",") + names[i];
    return s;
}

}  // namespace wmar
