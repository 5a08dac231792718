// Host driver for xfg-stark_amd/csrc/acceptable.hpp (no HIP): the conjectured security level over the whole
// option domain check_options admits (against a restatement with signed arithmetic and loop logarithms) and on
// every header a parsed proof can state, the policy check for sets of 1 and 32 members and for a minimum, the
// refusals of make_acceptable, and bucket_queries over every split of up to four items across the four folding
// factors. Built with ASan + UBSan (make build/asan/acceptable) and run directly; the arrays handed to
// bucket_queries end exactly at `count` entries, so a write past them is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../xfg-stark_amd/csrc/acceptable.hpp"

using namespace xfg;
typedef uint64_t u64;

static int failures = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                            \
        }                                                          \
    } while (0)

// the formula of the header's comment, restated: signed, logarithms by counting
static long restated_level(u64 n, const Opts& o) {
    long lde = 0;
    for (u64 d = n * o.beta; d > 1; d >>= 1) lde++;
    long lb = 0;
    for (u64 b = o.beta; b > 1; b >>= 1) lb++;
    const long field = 64 * (long)o.ext - lde;
    long query = lb * (long)o.q;
    if (query >= 80) query += (long)o.grind;
    const long m = (field < query ? field : query) - 1;
    return m < 128 ? m : 128;
}

static void test_levels() {
    // the pinned values of the issue that introduced the policy: hand-derived
    CHECK(conjectured_security(64, Opts{42, 8, 4, 1, 8, 31}) == 54);
    CHECK(conjectured_security(1ULL << 16, Opts{42, 8, 4, 1, 8, 31}) == 44);
    CHECK(conjectured_security(1ULL << 20, Opts{24, 16, 4, 2, 8, 31}) == 99);
    CHECK(conjectured_security(8, Opts{7, 8, 4, 1, 8, 7}) == 20);  // 21 bits of queries: grinding not counted
    u64 admitted = 0;
    uint32_t top = 0;
    for (u64 n = 8; n <= (1ULL << 21); n <<= 1)
        for (u64 beta = 2; beta <= 128; beta <<= 1)
            for (u64 ext = 1; ext <= 2; ext++)
                for (u64 grind = 0; grind <= 32; grind++)
                    for (u64 q = 1; q <= 255; q++) {
                        const Opts o{q, beta, grind, ext, (u64)(2 << (q & 3)), (u64)((1 << (grind & 7)) - 1)};
                        if (check_options(n, o)) continue;
                        admitted++;
                        const uint32_t got = conjectured_security(n, o);
                        CHECK((long)got == restated_level(n, o));
                        top = got > top ? got : top;
                    }
    CHECK(admitted > 1000000);
    CHECK(top < HASH_COLLISION_RESISTANCE);  // the cap needs the cubic extension
    // what a parsed header can state before check_options sees it: one byte per option, logn 3..32, ext 1..3.
    // Defined for all of it (the sanitizer watches), at most 128, and the cap is reached with ext = 3
    uint32_t worst = 0;
    for (unsigned logn = 3; logn <= 32; logn++)
        for (u64 beta = 0; beta <= 255; beta++)
            for (u64 ext = 1; ext <= 3; ext++)
                for (u64 q : {0ULL, 1ULL, 42ULL, 255ULL})
                    for (u64 grind : {0ULL, 32ULL, 255ULL}) {
                        const uint32_t got = conjectured_security(1ULL << logn, Opts{q, beta, grind, ext, 8, 31});
                        CHECK(got <= HASH_COLLISION_RESISTANCE);
                        worst = got > worst ? got : worst;
                    }
    CHECK(worst == HASH_COLLISION_RESISTANCE);
    CHECK(conjectured_security(1ULL << 32, Opts{255, 0, 0, 1, 8, 31}) == 0);  // log2(0) counts as 0: no query security
}

static xfg_options c_opts(const Opts& o) {
    return xfg_options{(uint32_t)o.q, (uint32_t)o.beta, (uint32_t)o.grind, (uint32_t)o.ext, (uint32_t)o.fold, (uint32_t)o.remdeg};
}

static void test_policy() {
    const Opts A{42, 8, 4, 1, 8, 31};
    char buf[POLICY_ERROR_LEN];
    const std::string refused = "UnacceptableProofOptions";
    // one member
    {
        const Acceptable one = acceptable_one(A);
        CHECK(one.kind == XFG_ACCEPT_OPTION_SET && one.count == 1);
        CHECK(std::string(policy_error(one, 64, A, buf)).empty());
        u64 Opts::*const fields[6] = {&Opts::q, &Opts::beta, &Opts::grind, &Opts::ext, &Opts::fold, &Opts::remdeg};
        for (auto f : fields) {  // a member that differs in one field, any field, does not match
            Opts b = A;
            b.*f += 1;
            CHECK(policy_error(one, 64, b, buf) == refused);
            CHECK(policy_error(acceptable_one(b), 64, A, buf) == refused);
        }
    }
    // 32 members, the array exactly that long: the match is the last one, the first one, none
    for (uint32_t count : {1u, 2u, 31u, 32u}) {
        std::vector<xfg_options> set(count);
        for (uint32_t i = 0; i < count; i++) set[i] = c_opts(Opts{(u64)(i + 1), 8, 4, 1, 8, 31});
        xfg_acceptable p{XFG_ACCEPT_OPTION_SET, 77, set.data(), count};
        Acceptable a;
        CHECK(make_acceptable(&p, a) && a.count == count && a.min_security == 0);
        CHECK(std::string(policy_error(a, 64, Opts{(u64)count, 8, 4, 1, 8, 31}, buf)).empty());
        CHECK(std::string(policy_error(a, 64, Opts{1, 8, 4, 1, 8, 31}, buf)).empty());
        CHECK(policy_error(a, 64, Opts{(u64)count + 1, 8, 4, 1, 8, 31}, buf) == refused);
        CHECK(policy_error(a, 64, Opts{0, 8, 4, 1, 8, 31}, buf) == refused);
    }
    // a minimum: at the level, one above it, and the largest threshold (the longest text)
    {
        xfg_acceptable p{XFG_ACCEPT_MIN_CONJECTURED_SECURITY, 54, nullptr, 0};
        Acceptable a;
        CHECK(make_acceptable(&p, a) && a.kind == XFG_ACCEPT_MIN_CONJECTURED_SECURITY && a.min_security == 54);
        CHECK(std::string(policy_error(a, 64, A, buf)).empty());
        CHECK(std::string(policy_error(a, 1ULL << 16, A, buf)) == "InsufficientConjecturedSecurity(54, 44)");
        p.min_security = 55;
        CHECK(make_acceptable(&p, a));
        CHECK(std::string(policy_error(a, 64, A, buf)) == "InsufficientConjecturedSecurity(55, 54)");
        p.min_security = 0xFFFFFFFFu;
        CHECK(make_acceptable(&p, a));
        CHECK(std::string(policy_error(a, 64, A, buf)) == "InsufficientConjecturedSecurity(4294967295, 54)");
        CHECK(strlen(buf) < POLICY_ERROR_LEN);
        p.min_security = 0;  // everything passes a minimum of 0, a header check_options refuses included
        CHECK(make_acceptable(&p, a));
        CHECK(std::string(policy_error(a, 1ULL << 32, Opts{0, 0, 255, 3, 0, 0}, buf)).empty());
    }
    // refusals
    {
        Acceptable a;
        xfg_options o = c_opts(A);
        CHECK(!make_acceptable(nullptr, a));
        for (uint32_t kind : {2u, 3u, 0xFFFFFFFFu}) {
            xfg_acceptable p{kind, 0, &o, 1};
            CHECK(!make_acceptable(&p, a));
        }
        xfg_acceptable p{XFG_ACCEPT_OPTION_SET, 0, nullptr, 1};
        CHECK(!make_acceptable(&p, a));
        p.options = &o;
        p.num_options = 0;
        CHECK(!make_acceptable(&p, a));
        p.num_options = 33;  // refused before the 33rd entry (which does not exist) is read
        CHECK(!make_acceptable(&p, a));
        p.num_options = 1;
        CHECK(make_acceptable(&p, a) && same_opts(a.set[0], A));
    }
}

// every batch of `count` items, each with a folding factor 2^logf (0: not planned) and 0..2 queries
static void test_buckets() {
    u64 batches = 0;
    for (uint32_t count = 0; count <= 4; count++) {
        u64 combos = 1;
        for (uint32_t i = 0; i < count; i++) combos *= 15;
        for (u64 code = 0; code < combos; code++) {
            std::vector<uint32_t> nq(count);
            std::vector<uint8_t> logf(count);
            std::vector<u64> first(count, ~0ULL);
            u64 c = code;
            for (uint32_t i = 0; i < count; i++, c /= 15) {
                logf[i] = (uint8_t)(c % 5);
                nq[i] = (uint32_t)(c % 15 / 5);
            }
            FoldRanges R;
            CHECK(bucket_queries(count, nq.data(), logf.data(), first.data(), R));
            batches++;
            u64 size[5] = {0, 0, 0, 0, 0};
            for (uint32_t i = 0; i < count; i++)
                if (logf[i]) size[logf[i]] += nq[i];
            CHECK(R.begin[0] == 0);
            for (int r = 0; r < 4; r++) CHECK(R.begin[r + 1] - R.begin[r] == size[r + 1]);
            // the records of a range, in input order, tile it exactly
            u64 next[5] = {0, R.begin[0], R.begin[1], R.begin[2], R.begin[3]};
            for (uint32_t i = 0; i < count; i++) {
                if (!logf[i] || !nq[i]) continue;
                CHECK(first[i] == next[logf[i]]);
                next[logf[i]] += nq[i];
            }
            for (int r = 0; r < 4; r++) CHECK(next[r + 1] == R.begin[r + 1]);
        }
    }
    CHECK(batches == 1 + 15 + 225 + 3375 + 50625);
    // a factor without a kernel is refused, nothing written
    {
        std::vector<uint32_t> nq{3, 3};
        std::vector<uint8_t> logf{1, 5};
        std::vector<u64> first(2, 7);
        FoldRanges R{{9, 9, 9, 9, 9}};
        CHECK(!bucket_queries(2, nq.data(), logf.data(), first.data(), R));
        CHECK(first[0] == 7 && first[1] == 7 && R.begin[0] == 9 && R.begin[4] == 9);
    }
    // the sizes of a real batch: 64 proofs of 42 queries, 16 per factor, interleaved
    {
        std::vector<uint32_t> nq(64, 42);
        std::vector<uint8_t> logf(64);
        std::vector<u64> first(64);
        for (int i = 0; i < 64; i++) logf[i] = (uint8_t)(1 + i % 4);
        FoldRanges R;
        CHECK(bucket_queries(64, nq.data(), logf.data(), first.data(), R));
        for (int r = 0; r <= 4; r++) CHECK(R.begin[r] == (u64)r * 16 * 42);
        for (int i = 0; i < 64; i++) CHECK(first[i] == R.begin[i % 4] + (u64)(i / 4) * 42);
    }
}

int main() {
    test_levels();
    test_policy();
    test_buckets();
    if (failures) {
        fprintf(stderr, "acceptable: %d failures\n", failures);
        return 1;
    }
    printf("acceptable ok\n");
    return 0;
}
