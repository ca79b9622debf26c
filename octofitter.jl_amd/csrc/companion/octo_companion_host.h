// octo_companion_host.h — the host-side scaffold every companion library (csrc/draws, predict, pointwise, psis) is built on: the part of a
// handle they all carry, the error path, the HIP check macro, device opening, buffer growth, the pinned staging buffer, sync.
// It depends on <hip/hip_runtime.h> and include/octofitter_hip.h alone — nothing of the main library's csrc/*.h — so the PSIS library,
// which links nothing of the main library, can use it. Everything lives in an unnamed namespace: the companions are separate shared
// objects loaded RTLD_GLOBAL, and each keeps a copy of its own (its own create-error string above all).
// It lives under csrc/companion/, not directly under csrc/: kernel_source_hash() covers exactly the files directly under csrc/, and the
// main library's counter evidence (profiles/pmc_traffic.json) is keyed to that hash.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <new>
#include <string>

#include "octofitter_hip.h"

namespace {

// What every handle starts with: struct octo_<name> derives from it.
struct CompanionBase {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
};

// … and the pinned staging buffer of the host-buffer calls (grown on demand), for the libraries that have them
struct CompanionStaged : CompanionBase {
    double* h_stage = nullptr; int64_t cap_stage = 0;
    int64_t stage_bytes = (int64_t)16 << 20;
};

thread_local std::string g_create_error;      // what octo_<name>_last_error(NULL) answers: one per library and thread

inline int fail(CompanionBase* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

#define OCHK(h, expr)                                                                                                   \
    do {                                                                                                                \
        const hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) return fail(h, e_ == hipErrorOutOfMemory ? OCTO_ENOMEM : OCTO_EHIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

inline const char* last_error(const CompanionBase* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

inline hipStream_t stream_of(const CompanionBase* h, void* hip_stream) { return hip_stream == OCTO_STREAM_CTX ? h->stream : (hipStream_t)hip_stream; }

inline int sync_handle(CompanionBase* h) {
    if (!h) return OCTO_EINVAL;
    OCHK(h, hipSetDevice(h->device));
    OCHK(h, hipStreamSynchronize(h->stream));
    return OCTO_OK;
}

// The device part of octo_<name>_create: a device exists, device_id names one, a value-initialised handle on it with a non-blocking stream
// of its own. fn is the message prefix ("octo_<name>_create: "). On failure h is null and nothing is left allocated.
template <class H>
int open_device(int device_id, const std::string& fn, H*& h) {
    h = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return fail(nullptr, OCTO_ENODEV, fn + "no HIP device"); }
    if (device_id < 0 || device_id >= n_dev) return fail(nullptr, OCTO_EINVAL, fn + "device_id out of range");
    H* n = new (std::nothrow) H();
    if (!n) return fail(nullptr, OCTO_ENOMEM, fn + "host allocation failed");
    n->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess) { delete n; return fail(nullptr, OCTO_EHIP, fn + "hipSetDevice failed"); }
    if (hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking) != hipSuccess) { delete n; return fail(nullptr, OCTO_EHIP, fn + "stream creation failed"); }
    h = n;
    return OCTO_OK;
}

// a device array of `need` doubles: kept while it is large enough, otherwise freed (behind the stream's work) and allocated anew
inline int grow(CompanionBase* h, double*& p, int64_t& cap, int64_t need) {
    if (need <= cap) return OCTO_OK;
    OCHK(h, hipStreamSynchronize(h->stream));
    if (p) { OCHK(h, hipFree(p)); p = nullptr; cap = 0; }
    OCHK(h, hipMalloc((void**)&p, sizeof(double) * (size_t)need));
    cap = need;
    return OCTO_OK;
}

// a byte count from the environment (the OCTO_*_BYTES knobs); unset, empty or not positive: the default
inline int64_t env_bytes(const char* name, int64_t dflt) {
    const char* s = std::getenv(name);
    if (!s || !*s) return dflt;
    const long long v = std::atoll(s);
    return v > 0 ? (int64_t)v : dflt;
}

// the pinned staging buffer holds at least want_stage doubles
inline int ensure_stage(CompanionStaged* h, int64_t want_stage) {
    if (h->cap_stage >= want_stage) return OCTO_OK;
    if (h->h_stage) { OCHK(h, hipHostFree(h->h_stage)); h->h_stage = nullptr; h->cap_stage = 0; }
    OCHK(h, hipHostMalloc((void**)&h->h_stage, sizeof(double) * (size_t)want_stage, hipHostMallocDefault));
    h->cap_stage = want_stage;
    return OCTO_OK;
}

}  // namespace
