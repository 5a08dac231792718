// The one choice of a template instantiation from run-time values, for every launch wrapper: each with_*
// hands its callee the value as an integral constant, f(std::integral_constant<...>{}), and throws
// std::invalid_argument naming a value that has no kernel -- refused, never skipped and never replaced by
// another instantiation (the ABI entries validate the same values before anything is launched). No HIP here.
#pragma once
#include <stdexcept>
#include <string>
#include <type_traits>

namespace xfg {

template <int V>
using IntC = std::integral_constant<int, V>;

// D: the extension degree of the challenges, 1 (FieldExtension::None) or 2 (Quadratic)
template <class F>
void with_ext(int ext, F f) {
    switch (ext) {
        case 1: return f(IntC<1>{});
        case 2: return f(IntC<2>{});
        default: throw std::invalid_argument("no kernel for extension degree " + std::to_string(ext));
    }
}

// log2 of a folding factor the kernels have (2, 4, 8, 16), else 0: the only such map
constexpr int fold_log2(long long fold) { return fold == 2 ? 1 : fold == 4 ? 2 : fold == 8 ? 3 : fold == 16 ? 4 : 0; }
// LOGF = fold_log2(fold)
template <class F>
void with_fold(int fold, F f) {
    switch (fold_log2(fold)) {
        case 1: return f(IntC<1>{});
        case 2: return f(IntC<2>{});
        case 3: return f(IntC<3>{});
        case 4: return f(IntC<4>{});
        default: throw std::invalid_argument("no kernel for folding factor " + std::to_string(fold));
    }
}

// a kernel's bool parameter (CC: constant columns; AIR: the constraints besides the canonicity test)
template <class F>
void with_bool(bool v, F f) {
    v ? f(std::true_type{}) : f(std::false_type{});
}

// (NC, LOGB): the column count of an LDE, {7, 2, 1}, and log2 of its blowup, 1..7. with_logbeta fixes the
// column count at compile time (the constant-column kernels exist for the seven trace columns alone)
template <int NC, class F>
void with_logbeta(int logbeta, F f) {
    switch (logbeta) {
        case 1: return f(IntC<NC>{}, IntC<1>{});
        case 2: return f(IntC<NC>{}, IntC<2>{});
        case 3: return f(IntC<NC>{}, IntC<3>{});
        case 4: return f(IntC<NC>{}, IntC<4>{});
        case 5: return f(IntC<NC>{}, IntC<5>{});
        case 6: return f(IntC<NC>{}, IntC<6>{});
        case 7: return f(IntC<NC>{}, IntC<7>{});
        default: throw std::invalid_argument("no kernel for blowup 2^" + std::to_string(logbeta));
    }
}
template <class F>
void with_nc_logbeta(int nc, int logbeta, F f) {
    switch (nc) {
        case 7: return with_logbeta<7>(logbeta, f);
        case 2: return with_logbeta<2>(logbeta, f);
        case 1: return with_logbeta<1>(logbeta, f);
        default: throw std::invalid_argument("no kernel for an LDE of " + std::to_string(nc) + " columns");
    }
}

}  // namespace xfg
