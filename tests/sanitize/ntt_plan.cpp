// Stand-alone driver of the NTT launch planner (xfg-stark_amd/csrc/ntt_plan.hpp), built host-only with
// ASan + UBSan by `make -C xfg-stark_amd sanitize`. It walks log2 n = 1..24 x log2 blowup = 1..4 x both
// directions x launch-set sizes on either side of every threshold x the table states, and fails unless
//   * every shape is planned onto a listed kernel (XFG_NTT_KERNELS) or reported unsupported,
//   * the unsupported shapes are exactly sizes 2 and 4 and sizes >= 2^23 (and forward without pass tables),
//   * no launch asks for more than 160 KiB of LDS, and grid x tile covers the problem exactly,
//   * the LDS and pass-table regions are contiguous, disjoint and sum to the total,
//   * pass_tables_size / fourstep_size equal the entry counts written out by hand below,
//   * every listed kernel is planned by some shape.
// One line per shape goes to stdout (tests/test_ntt_plan.py compares them with launches recorded on the GPU).
#include <cstdio>
#include <cstdlib>
#include <string>
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

struct Listed {
    NttKey key;
    const char* name;
    int reached;
};
#define XFG_LISTED(K, SYM, S, INV, T, E) {{NttKernel::K, S, T, E, INV}, #SYM, 0},
static std::vector<Listed> listed = {XFG_NTT_KERNELS(XFG_LISTED)};

// "(ntt_pass_a<1, false, 8, 4>)" -> "ntt_pass_a<1, false, 8, 4>"
static std::string kernel_name(const Listed& l) {
    std::string s = l.name;
    return s.substr(1, s.size() - 2);
}
static Listed* find(const NttKey& k) {
    for (auto& l : listed)
        if (l.key == k) return &l;
    return nullptr;
}

static void check_pass(const NttPass& p, bool pass_a, const NttPlan& pl, int logn, int logbeta, bool inv, int npoly) {
    const int logS = pass_a ? pl.logR : pl.logC, logO = pass_a ? pl.logC : pl.logR;  // DFT size, lines per plane
    CHECK(p.key.logS == logS && p.key.inv == inv, "key of logn %d", logn);
    CHECK(p.block == 1u << p.key.logT, "block of logn %d", logn);
    CHECK(p.lds <= 160 * 1024, "%zu bytes of LDS at logn %d", p.lds, logn);
    const int full = p.key.logT + p.key.logE - logS, logtile = logO < full ? logO : full;
    CHECK(full >= 0, "tile holds no line at logn %d", logn);
    const unsigned long long planes = (unsigned long long)npoly << (inv ? 0 : logbeta);
    const bool all_cosets = p.key.kernel == NttKernel::pass_a_cos || p.key.kernel == NttKernel::pass_a_cos2;
    if (p.key.kernel == NttKernel::pass_b_pers) {
        CHECK(((unsigned long long)pl.ntx << logtile) == 1ull << logO && (unsigned long long)pl.ntiles == pl.ntx * planes,
              "persistent tiles at logn %d", logn);
        CHECK(p.gy == 1 && p.gx >= 8 && p.gx % 8 == 0 && (p.gx <= (unsigned)pl.ntiles || p.gx == 8), "persistent grid %u", p.gx);
    } else {
        // blocks x lines per tile x line length = planes x n
        const unsigned long long per_block = (1ull << (logtile + logS)) << (all_cosets ? logbeta : 0);
        CHECK((unsigned long long)p.gx * p.gy * per_block == planes << logn, "grid %u x %u at logn %d, %d polys", p.gx, p.gy,
              logn, npoly);
        CHECK(((unsigned long long)p.gx << logtile) == 1ull << logO, "grid.x %u at logn %d", p.gx, logn);
    }
}

// tile, twiddle table and pre-factors follow each other and end at `bytes`; sizes in words of `unit` bytes
static void check_lds(const LdsLayout& l, int unit, int tile, int tw, int pre) {
    CHECK(l.tw == tile && l.pre == l.tw + tw && l.bytes == (l.pre + pre) * unit, "LDS regions %d %d %d", l.tw, l.pre, l.bytes);
}

int main() {
    const int npolys[] = {1, 2, 3, 7, 8, 15, 16, 28, 31, 32, 33, 64, 224};
    for (int inv = 0; inv < 2; inv++)
        for (int logn = 1; logn <= 24; logn++)
            for (int logbeta = 1; logbeta <= (inv ? 1 : 4); logbeta++)
                for (int tables = 0; tables < 3; tables++) {  // 0: those the prover builds, 1: pass tables only, 2: none
                    const TableKind k = table_kind(logn, logbeta);
                    bool t4 = inv ? (logn >= 3 && logn <= FOURSTEP_MAX_LOG) : k == TableKind::fourstep;
                    bool pt = inv ? t4 : k != TableKind::none;
                    if (tables == 1 && (inv || !t4)) continue;
                    if (tables == 2 && !pt) continue;
                    if (tables >= 1) t4 = false;
                    if (tables == 2) pt = false;
                    for (int npoly : npolys) {
                        const NttPlan p = ntt_plan(logn, inv ? 0 : logbeta, inv, npoly, t4, pt, 256);
                        const bool want = logn >= 3 && logn <= 22 && (inv || pt);
                        CHECK(p.ok == want, "%s logn %d logbeta %d tables %d: ok = %d", inv ? "inv" : "fwd", logn, logbeta,
                              tables, (int)p.ok);
                        if (tables == 0) CHECK(ntt_supported(logn, inv ? 0 : logbeta, inv) == want, "ntt_supported(%d)", logn);
                        if (tables == 0 && !p.ok && npoly == 1)
                            std::printf("%s logn=%d logbeta=%d npoly=%d : unsupported\n", inv ? "inv" : "fwd", logn,
                                        inv ? 0 : logbeta, npoly);
                        if (!p.ok) continue;
                        Listed *a = find(p.a.key), *b = find(p.b.key);
                        CHECK(a && b, "logn %d plans a kernel that is not listed", logn);
                        if (!a || !b) continue;
                        a->reached++;
                        b->reached++;
                        check_pass(p.a, true, p, logn, logbeta, inv, npoly);
                        check_pass(p.b, false, p, logn, logbeta, inv, npoly);
                        if (tables == 0)
                            std::printf("%s logn=%d logbeta=%d npoly=%d : %s grid=%ux%u block=%u lds=%zu ; %s grid=%ux%u block=%u lds=%zu\n",
                                        inv ? "inv" : "fwd", logn, inv ? 0 : logbeta, npoly, kernel_name(*a).c_str(), p.a.gx,
                                        p.a.gy, p.a.block, p.a.lds, kernel_name(*b).c_str(), p.b.gx, p.b.gy, p.b.block,
                                        p.b.lds);
                    }
                }
    for (const auto& l : listed) CHECK(l.reached > 0, "%s is listed but no shape plans it", l.name);

    // LDS layouts of every listed kernel, at every size of the other pass
    for (const auto& l : listed) {
        const NttKey& k = l.key;
        const int S = 1 << k.logS, full = k.logT + k.logE - k.logS;
        for (int logO = 1; logO <= 13; logO++) {
            const int lines = 1 << (logO < full ? logO : full);
            switch (k.kernel) {
                case NttKernel::pass_a:
                case NttKernel::pass_a_cos:
                case NttKernel::pass_a_cos2:
                    check_lds(lds_pass_a(k.logS, k.logT, k.logE, logO, false), 8, lines * row_pitch(S, k.logE, full), S, S);
                    check_lds(lds_pass_a(k.logS, k.logT, k.logE, logO, true), 8, lines * row_pitch(S, k.logE, full), S, 0);
                    break;
                case NttKernel::pass_b:
                case NttKernel::pass_b_pers:
                    check_lds(lds_pass_b(k.logS, k.logT, k.logE, logO), 8, lines * row_pitch(S, k.logE, full), S, 0);
                    break;
                case NttKernel::pass_b_tq:
                    check_lds(lds_pass_b_tq(k.logS, k.logT, k.logE, logO), 4, lines * row_pitch(S, k.logE, full), 2 * S, 0);
                    break;
                case NttKernel::pass_a_r1024:
                    check_lds(lds_r1024(false), 8, (8 * split_pitch(1024, 5, 3) + 1) / 2, 1024, 32 * 8);
                    break;
                case NttKernel::pass_b_r1024:
                    check_lds(lds_r1024(true), 8, (8 * split_pitch(1024, 5, 3) + 1) / 2, 1024, 0);
                    break;
            }
        }
    }

    // pass tables: regions in order, each starting where the last one ended
    for (int logn = 1; logn <= 24; logn++)
        for (int logbeta = -1; logbeta <= 4; logbeta++) {
            const PassTableLayout L = pass_table_layout(logn, logbeta);
            const unsigned long long R = 1ull << L.logR, C = 1ull << L.logC, beta = logbeta >= 0 ? 1ull << logbeta : 0;
            CHECK(L.logR + L.logC == logn && L.logC >= L.logR && L.logC <= L.logR + 2, "split of %d", logn);
            unsigned long long at = 0;
            CHECK(L.wR() == at, "wR");
            at += R;
            CHECK(L.wC() == at, "wC");
            at += C;
            unsigned long long extra = 0;  // the parent's cos2_extra, written out
            if (logbeta >= 0) {
                for (unsigned long long t = 0; t < beta; t++) CHECK(L.pre(t) == at + t * R, "pre(%llu) at logn %d", t, logn);
                at += beta * R;
                if (L.logR == 10 && L.logC == 10) {
                    CHECK(L.has_r1024(), "r1024 tables at logn %d", logn);
                    for (unsigned long long t = 0; t < beta; t++) CHECK(L.comb(t) == at + t * 1024, "comb(%llu)", t);
                    at += beta * R;
                    for (unsigned long long t = 0; t < beta; t++) CHECK(L.r1024_seed(t) == at + t * C, "seed(%llu)", t);
                    at += beta * C;
                    CHECK(L.r1024_t4() == at, "t4 table");
                    at += R * C;
                    extra = beta * R + beta * C + R * C;
                } else if (L.logR == 8 && logbeta >= 2) {
                    CHECK(L.has_cos2() && !L.has_r1024(), "cos2 tables at logn %d", logn);
                    for (unsigned long long t = 0; t < beta; t++) CHECK(L.comb(t) == at + t * 256, "comb(%llu)", t);
                    at += beta * R;
                    CHECK(L.cos2_scal() == at, "class scalars");
                    at += 16 * (beta / 4);
                    extra = beta * R + 16 * (beta / 4);
                } else {
                    CHECK(!L.has_r1024() && !(L.has_cos2() && logbeta >= 2), "no extra tables at logn %d", logn);
                }
            }
            CHECK(L.total() == at, "total %llu, regions end at %llu (logn %d, logbeta %d)", (unsigned long long)L.total(), at,
                  logn, logbeta);
            CHECK(pass_tables_size(logn, logbeta) == R + C + beta * R + extra, "pass_tables_size(%d, %d)", logn, logbeta);
            CHECK(fourstep_size(logn, logbeta) == (1ull << (logn + (logbeta > 0 ? logbeta : 0))) + R + C + beta * R + extra,
                  "fourstep_size(%d, %d)", logn, logbeta);
        }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::fprintf(stderr, "ntt_plan: %zu kernels, all checks passed\n", listed.size());
    return 0;
}
