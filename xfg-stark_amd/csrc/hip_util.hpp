// HIP error handling and the one kernel launcher (every .hip file), the XFG_TRACE switch and the owning
// device / pinned-host buffer types of the prover's host code (tables.hip, lane_unit.hip, prover.hip,
// debug_abi.hip, verify_batch_gpu.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace xfg {

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess)                                                                      \
            throw HipError(std::string("HIP error ") + hipGetErrorString(e_) + " at " #x);        \
    } while (0)

// Every kernel launch of the library: XFG_LAUNCH(kernel, grid, block, dynamic LDS bytes, stream, args...).
// The parameter types come from the kernel's own signature and each argument is converted to its parameter
// as a direct call would convert it, so a wrong pointer type or argument count does not compile. A launch the
// runtime refuses (a grid row past 65535, a block or an LDS request over the limit, no device) throws
// HipError naming the kernel: it would otherwise leave no trace, not even at the next synchronisation.
template <class T>
struct SameType {
    using type = T;
};
inline void launch_checked(const char* name, const void* fn, dim3 grid, dim3 block, void** args, size_t lds,
                           hipStream_t s) {
    const hipError_t e = hipLaunchKernel(fn, grid, block, args, lds, s);
    if (e != hipSuccess) throw HipError(std::string("launch of ") + name + ": " + hipGetErrorString(e));
}
template <class... P>
void launch_kernel(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                   typename SameType<P>::type... p) {  // P is deduced from the kernel alone
    void* args[sizeof...(P) + 1] = {(void*)&p..., nullptr};
    launch_checked(name, (const void*)kernel, grid, block, args, lds, s);
}
#define XFG_LAUNCH(kernel, ...) ::xfg::launch_kernel(#kernel, kernel, __VA_ARGS__)

// XFG_TRACE=1: host-side phase timestamps of every prove call (and any workspace reallocation,
// which synchronises the device), printed to stderr
static inline bool trace_on() {
    static const bool on = getenv("XFG_TRACE") && *getenv("XFG_TRACE") == '1';
    return on;
}
static inline void trace_realloc(const char* kind, size_t old_n, size_t new_n, size_t elem) {
    if (trace_on()) fprintf(stderr, "[xfg] realloc %s %zu -> %zu bytes\n", kind, old_n * elem, new_n * elem);
}

// ------------------------------------------------------------------ device buffers
// Both buffer types own their allocation (freed by the destructor) and are move-only, so a buffer
// added to a lane or a table map is released with it.
template <class T>
struct DBuf {
    T* p = nullptr;
    size_t n = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    DBuf(DBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    DBuf& operator=(DBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, n = o.n;
            o.p = nullptr, o.n = 0;
        }
        return *this;
    }
    ~DBuf() { release(); }
    void ensure(size_t cnt) {
        if (cnt <= n) return;
        trace_realloc("device", n, std::max<size_t>(cnt + cnt / 8, 1), sizeof(T));
        release();
        size_t want = std::max<size_t>(cnt + cnt / 8, 1);
        HIPCHK(hipMalloc((void**)&p, want * sizeof(T)));
        n = want;
    }
    void release() noexcept {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// pinned host staging (hipHostMalloc) so D2H/H2D copies are true async DMA, grown with headroom.
// Flags: hipHostMallocDefault for DMA staging; MappedHBuf for the blocks kernels read and write in
// place through hipHostGetDevicePointer (the per-unit AIR constants, coins, replay block, opening
// indices / values / digests): fine-grained (coherent) memory, so a kernel never reads a line the GPU
// cached for an earlier unit and its stores reach the host without relying on the dispatch packets'
// system-scope release (coarse-grained host memory is coherent only at those fences).
template <class T, unsigned Flags = hipHostMallocDefault>
struct HBuf {
    T* p = nullptr;
    size_t n = 0;
    HBuf() = default;
    HBuf(const HBuf&) = delete;
    HBuf& operator=(const HBuf&) = delete;
    HBuf(HBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    HBuf& operator=(HBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, n = o.n;
            o.p = nullptr, o.n = 0;
        }
        return *this;
    }
    ~HBuf() { release(); }
    T* ensure(size_t cnt) {
        if (cnt <= n) return p;
        trace_realloc("pinned", n, cnt + cnt / 4 + 16, sizeof(T));
        release();
        size_t want = cnt + cnt / 4 + 16;
        HIPCHK(hipHostMalloc((void**)&p, want * sizeof(T), Flags));
        n = want;
        return p;
    }
    void release() noexcept {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    T& operator[](size_t i) { return p[i]; }
    T* data() { return p; }
};

template <class T>
using MappedHBuf = HBuf<T, hipHostMallocMapped | hipHostMallocCoherent>;

}  // namespace xfg
