// Stand-alone driver of the composed-LDE plan (lde_plan / lde_coset, xfg-stark_amd/csrc/ntt_plan.hpp), built
// host-only with ASan + UBSan by `make -C xfg-stark_amd sanitize`. It walks log2 n = 3..20 x blowup 32, 64, 128
// x launch-set sizes and fails unless
//   * a shape of at most 2^24 points whose blowup-16 transform has kernels is planned, any other refused,
//   * the planes the g sub-transforms write (plane u + g t' of a polynomial, words u n + t' out_plane from its
//     start) are a permutation of 0..beta - 1, each inside the polynomial's beta n words, and hold what the
//     coset-major layout wants there: row m of the plane, worked out from the sub-transform's evaluation point
//     7 w_(16n)^(t' + 16m) w_N^u = 7 w_N^K, sits at word (K mod beta) n + K / beta,
//   * the scratch regions -- one sub-transform's pass intermediate, then g - 1 twisted coefficient sets -- are
//     disjoint, in order, and end inside the npoly beta n words every caller allocates,
//   * the sub-transforms are planned by ntt_plan onto listed kernels with the tables the prover builds,
//   * blowup <= 16 stays the direct transform: one group, plane stride n.
#include <cstdio>
#include <vector>

#include "../../xfg-stark_amd/csrc/ntt_plan.hpp"

using namespace xfg;

static int failures = 0;
#define CHECK(c, ...)                             \
    do {                                          \
        if (!(c)) {                               \
            failures++;                           \
            std::fprintf(stderr, "FAIL %s: ", #c); \
            std::fprintf(stderr, __VA_ARGS__);    \
            std::fprintf(stderr, "\n");           \
        }                                         \
    } while (0)

int main() {
    const int npolys[] = {1, 2, 3, 7, 14, 56, 224};
    int planned = 0;
    for (int logn = 3; logn <= 20; logn++)
        for (int logbeta = 5; logbeta <= 7; logbeta++)
            for (int npoly : npolys) {
                const LdePlan p = lde_plan(logn, logbeta, npoly);
                const bool want = logn + logbeta <= 24 && ntt_supported(logn, 4, false);
                CHECK(p.ok == want && lde_supported(logn, logbeta) == want, "logn %d logbeta %d: ok = %d", logn, logbeta, (int)p.ok);
                if (!p.ok) continue;
                planned++;
                const unsigned long long n = 1ull << logn, beta = 1ull << logbeta, np = (unsigned long long)npoly;
                const int g = 1 << (logbeta - 4);
                CHECK(p.groups == g && p.sub_logbeta == 4 && p.out_plane == g * n, "groups %d stride %llu", p.groups,
                      (unsigned long long)p.out_plane);
                // every plane of a polynomial is written once, inside the polynomial
                std::vector<int> seen(beta, 0);
                for (int u = 0; u < p.groups; u++)
                    for (int ts = 0; ts < 16; ts++) {
                        const unsigned long long word = (unsigned long long)u * n + (unsigned long long)ts * p.out_plane;
                        const int t = lde_coset(p, u, ts);
                        CHECK(t >= 0 && (unsigned long long)t < beta, "coset %d of (%d, %d)", t, u, ts);
                        if (t < 0 || (unsigned long long)t >= beta) continue;
                        CHECK(word + n <= beta * n, "plane (%d, %d) at word %llu", u, ts, word);
                        // from the evaluation points, not from the plan: row m of that plane is the twisted polynomial
                        // at 7 w_(16n)^(ts + 16 m), i.e. P at 7 w_N^K with K = u + (N / 16n) (ts + 16 m); natural index
                        // K lies at word (K mod beta) n + K / beta of the coset-major polynomial
                        const unsigned long long rows[] = {0, 1, n / 2, n - 1};
                        for (unsigned long long m : rows) {
                            const unsigned long long K = (unsigned long long)u + (beta * n / (16 * n)) * ((unsigned long long)ts + 16 * m);
                            CHECK(K < beta * n && word + m == (K % beta) * n + K / beta, "row %llu of plane (%d, %d): K = %llu", m, u, ts, K);
                        }
                        CHECK(t == (int)((u + (beta / 16) * ts) % beta), "lde_coset(%d, %d) = %d", u, ts, t);
                        seen[(size_t)t]++;
                    }
                for (unsigned long long t = 0; t < beta; t++) CHECK(seen[t] == 1, "coset %llu written %d times", t, seen[t]);
                // scratch: [npoly][16][n] then [g - 1][npoly][n], inside npoly * beta * n
                CHECK(p.twist_off == np * 16 * n, "twisted coefficients at %llu", (unsigned long long)p.twist_off);
                CHECK(p.scratch_words == p.twist_off + (unsigned long long)(g - 1) * np * n, "scratch %llu",
                      (unsigned long long)p.scratch_words);
                CHECK(p.scratch_words <= np * beta * n, "scratch %llu past the caller's %llu", (unsigned long long)p.scratch_words,
                      np * beta * n);
                // the sub-transform itself
                const TableKind k = table_kind(logn, p.sub_logbeta);
                const NttPlan q = ntt_plan(logn, p.sub_logbeta, false, npoly, k == TableKind::fourstep, k != TableKind::none, 256);
                CHECK(q.ok, "sub-transform of logn %d has no kernel", logn);
            }
    CHECK(planned > 0, "nothing planned");
    for (int logn = 21; logn <= 26; logn++)
        for (int logbeta = 5; logbeta <= 7; logbeta++) CHECK(!lde_plan(logn, logbeta, 1).ok, "logn %d planned", logn);
    for (int logn = 3; logn <= 16; logn++) CHECK(!lde_plan(logn, 8, 1).ok && !lde_supported(logn, 8), "blowup 256 planned");
    for (int logn = 3; logn <= 22; logn++)
        for (int logbeta = 1; logbeta <= 4; logbeta++) {
            const LdePlan p = lde_plan(logn, logbeta, 7);
            CHECK(p.ok && p.groups == 1 && p.sub_logbeta == logbeta && p.out_plane == 1ull << logn, "direct plan of logn %d", logn);
            CHECK(lde_supported(logn, logbeta) == ntt_supported(logn, logbeta, false), "lde_supported(%d, %d)", logn, logbeta);
        }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::fprintf(stderr, "lde_plan: %d shapes planned, all checks passed\n", planned);
    return 0;
}
