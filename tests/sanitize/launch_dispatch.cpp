// Stand-alone driver of the instantiation dispatchers (csrc/dispatch.hpp) and of the one kernel launcher
// (csrc/hip_util.hpp launch_kernel / XFG_LAUNCH), host code under ASan + UBSan, built by
// `make -C xfg-stark_amd sanitize` (tests/test_launch_dispatch.py runs it). It fails unless
//   (a) every dispatcher hands its callee the right integral constants for every value that has a kernel --
//       ext 1, 2; folding factor 2, 4, 8, 16 (and fold_log2 says the same); both bools; the 21 pairs of
//       {7, 2, 1} columns x blowup 2^1..2^7, and the seven of the fixed-width with_logbeta<7> -- and throws
//       std::invalid_argument, with the value in its text and the callee never called, for ext 0 and 3, fold
//       0, 1, 3, 32, the column counts 0, 3, 8 and log2 blowup 0 and 8; the same for the (ext, fold)
//       composition that picks the FRI kernels;
//   (b) where the process can reach no GPU: a launch of an empty kernel, and of a templated one that takes
//       a struct by value and converted arguments, throws HipError with the kernel's name and the runtime's
//       reason in its text. With a GPU in reach (the kernel driver's device node can be opened) no launch
//       is sent -- a launch meant to fail is not for a device -- and the HIP runtime is left alone.
// Prints two lines to stdout: "dispatch ok: <checks>" and "launcher: ...".
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../xfg-stark_amd/csrc/dispatch.hpp"
#include "../../xfg-stark_amd/csrc/hip_util.hpp"

using namespace xfg;

static int failures = 0, checks = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        checks++;                                      \
        if (!(c)) {                                    \
            if (failures++ < 20) {                     \
                std::fprintf(stderr, "FAIL %s: ", #c); \
                std::fprintf(stderr, __VA_ARGS__);     \
                std::fprintf(stderr, "\n");            \
            }                                          \
        }                                              \
    } while (0)

// f() must throw std::invalid_argument whose text holds `value`; `called` counts the callee's runs
template <class F>
static void refused(const char* what, long long value, int& called, F f) {
    called = 0;
    bool threw = false;
    try {
        f();
    } catch (const std::invalid_argument& e) {
        threw = true;
        CHECK(std::strstr(e.what(), std::to_string(value).c_str()) != nullptr, "%s %lld: the text is \"%s\"", what,
              value, e.what());
    }
    CHECK(threw, "%s %lld: nothing thrown", what, value);
    CHECK(called == 0, "%s %lld: the callee ran", what, value);
}

static void dispatchers() {
    int called = 0;
    for (int ext : {1, 2}) {
        int got = 0;
        with_ext(ext, [&](auto D) {
            static_assert(D == 1 || D == 2, "a constant expression");
            got = D;
        });
        CHECK(got == ext, "ext %d -> %d", ext, got);
    }
    for (int ext : {0, 3}) refused("ext", ext, called, [&] { with_ext(ext, [&](auto) { called++; }); });

    for (int logf = 1; logf <= 4; logf++) {
        int got = 0;
        with_fold(1 << logf, [&](auto LF) { got = LF; });
        CHECK(got == logf && fold_log2(1 << logf) == logf, "fold %d -> %d, fold_log2 %d", 1 << logf, got,
              fold_log2(1 << logf));
    }
    for (int fold : {0, 1, 3, 32}) {
        CHECK(fold_log2(fold) == 0, "fold_log2(%d) = %d", fold, fold_log2(fold));
        refused("fold", fold, called, [&] { with_fold(fold, [&](auto) { called++; }); });
    }

    for (bool v : {false, true}) {
        int got = -1;
        with_bool(v, [&](auto B) { got = B ? 1 : 0; });
        CHECK(got == (int)v, "bool %d -> %d", (int)v, got);
    }

    for (int nc : {7, 2, 1})
        for (int lb = 1; lb <= 7; lb++) {
            int gn = 0, gl = 0;
            with_nc_logbeta(nc, lb, [&](auto NC, auto LB) { gn = NC, gl = LB; });
            CHECK(gn == nc && gl == lb, "(%d, %d) -> (%d, %d)", nc, lb, gn, gl);
        }
    for (int lb = 1; lb <= 7; lb++) {
        int gn = 0, gl = 0;
        with_logbeta<7>(lb, [&](auto NC, auto LB) { gn = NC, gl = LB; });
        CHECK(gn == 7 && gl == lb, "<7>(%d) -> (%d, %d)", lb, gn, gl);
    }
    for (int nc : {0, 3, 8})
        refused("columns", nc, called, [&] { with_nc_logbeta(nc, 3, [&](auto, auto) { called++; }); });
    for (int lb : {0, 8}) {
        for (int nc : {7, 2, 1})
            refused("log2 blowup", lb, called, [&] { with_nc_logbeta(nc, lb, [&](auto, auto) { called++; }); });
        refused("log2 blowup", lb, called, [&] { with_logbeta<7>(lb, [&](auto, auto) { called++; }); });
    }

    // the FRI kernels' (D, LOGF): one dispatcher inside the other
    auto ext_fold = [&](int ext, int fold, int& d, int& lf) {
        with_ext(ext, [&](auto D) { with_fold(fold, [&](auto LF) { called++, d = D, lf = LF; }); });
    };
    for (int ext : {1, 2})
        for (int logf = 1; logf <= 4; logf++) {
            int d = 0, lf = 0;
            ext_fold(ext, 1 << logf, d, lf);
            CHECK(d == ext && lf == logf, "(ext %d, fold %d) -> (%d, %d)", ext, 1 << logf, d, lf);
        }
    int d, lf;
    for (int ext : {0, 3}) refused("ext", ext, called, [&] { ext_fold(ext, 8, d, lf); });
    for (int fold : {1, 3, 32}) refused("fold", fold, called, [&] { ext_fold(2, fold, d, lf); });
}

__global__ void empty_kernel() {}
struct ProbeArgs {
    const uint64_t* in;
    uint64_t* out;
    int logn;
};
template <int D, bool CC>
__global__ void probe_kernel(ProbeArgs a, const uint64_t* more, uint64_t n, const int k) {
    if (threadIdx.x == 0 && n && a.out) a.out[0] = a.in[0] + more[0] + D + CC + k;
}

template <class F>
static void launch_refused(const char* name, F f) {
    bool threw = false;
    try {
        f();
    } catch (const HipError& e) {
        threw = true;
        CHECK(std::strstr(e.what(), name) != nullptr, "the text \"%s\" does not name %s", e.what(), name);
        std::printf("launcher: %s\n", e.what());
    }
    CHECK(threw, "launch of %s: nothing thrown", name);
}

int main() {
    dispatchers();
    std::printf("dispatch ok: %d\n", checks);
    if (access("/dev/kfd", R_OK | W_OK) == 0) {
        std::printf("launcher: a GPU is in reach, no launch sent\n");
    } else {
        launch_refused("empty_kernel", [] { XFG_LAUNCH(empty_kernel, dim3(1), dim3(64), 0, nullptr); });
        uint64_t* none = nullptr;  // converted as a call would: u64* -> const u64*, int -> u64, short -> int
        launch_refused("probe_kernel<2, true>", [&] {
            XFG_LAUNCH((probe_kernel<2, true>), dim3(1), dim3(64), 0, nullptr, ProbeArgs{none, none, 3}, none, 1 << 3,
                       (short)5);
        });
    }
    if (failures) {
        std::fprintf(stderr, "%d of %d checks failed\n", failures, checks);
        return 1;
    }
    return 0;
}
