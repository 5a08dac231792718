// Stand-alone driver of the two per-proof hoists that a trace's constant columns allow, built host-only with
// ASan + UBSan by `make -C xfg-stark_amd sanitize` (tests/test_leaf_prefix_cpu.py runs it). For each of the
// 128 constant-column masks it fails unless
//   (a) the leaf hash resumed from the round-1 prefix (blake3.hpp b3_row7_prefix, b3_hash_row7) equals
//       b3_hash_elems<7> on random canonical rows that share the constant columns -- the prefix is given
//       wrong values for the columns that are not constant, which it must not read;
//   (b) the planner's set of uniform round-1 G functions (b3_row7_uniform_gs) is the set found by brute force:
//       two rows that differ in every column that is not constant give the same four output words for a G
//       exactly when the planner marks it (round 1 is recomputed here, G by G, with this file's own G), and
//       the prefix holds those words. The same for the AIR's table of the columns a constraint reads
//       (air.hpp air_uniform_constraints) against the constraints evaluated on two such rows;
//   (c) the per-proof uniform part of the constraint sums plus the per-point rest (air.hpp ce_uniform_of,
//       ce_live_sums) equals the three full sums in host field arithmetic, in both fields, for random canonical
//       constants, AIR constants and coefficients. The constants do not satisfy the AIR: on a valid trace
//       every hoisted term is zero and a wrong split would pass (the driver checks the hoisted sums are not zero).
// Prints one summary line to stdout.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../xfg-stark_amd/csrc/air.hpp"
#include "../../xfg-stark_amd/csrc/blake3.hpp"

using namespace xfg;

static int failures = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (failures++ < 20) {                     \
                std::fprintf(stderr, "FAIL %s: ", #c); \
                std::fprintf(stderr, __VA_ARGS__);     \
                std::fprintf(stderr, "\n");            \
            }                                          \
        }                                              \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static uint64_t rnd_fe() {  // canonical, with the edges now and then
    const uint64_t r = rnd();
    switch (r & 31) {
        case 0: return 0;
        case 1: return P - 1;
        case 2: return 0xFFFFFFFFULL;
        default: return rnd() % P;
    }
}

// ---- round 1 of the seven-element hash, G by G: out[g] = the four state words G number g writes
static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static void ref_g(uint32_t* s, int a, int b, int c, int d, uint32_t x, uint32_t y, uint32_t out[4]) {
    s[a] = s[a] + s[b] + x; s[d] = rotr(s[d] ^ s[a], 16); s[c] = s[c] + s[d]; s[b] = rotr(s[b] ^ s[c], 12);
    s[a] = s[a] + s[b] + y; s[d] = rotr(s[d] ^ s[a], 8);  s[c] = s[c] + s[d]; s[b] = rotr(s[b] ^ s[c], 7);
    out[0] = s[a]; out[1] = s[b]; out[2] = s[c]; out[3] = s[d];
}
static const int G_WORDS[8][4] = {{0, 4, 8, 12}, {1, 5, 9, 13}, {2, 6, 10, 14}, {3, 7, 11, 15},
                                  {0, 5, 10, 15}, {1, 6, 11, 12}, {2, 7, 8, 13}, {3, 4, 9, 14}};
static void ref_round1(const uint64_t row[7], uint32_t out[8][4]) {
    uint32_t s[16] = {XFG_B3_IV, XFG_B3_IV0, XFG_B3_IV1, XFG_B3_IV2, XFG_B3_IV3, 0, 0, 56,
                      B3_CHUNK_START | B3_CHUNK_END | B3_ROOT};
    uint32_t m[16] = {0};
    for (int c = 0; c < 7; c++) {
        m[2 * c] = (uint32_t)row[c];
        m[2 * c + 1] = (uint32_t)(row[c] >> 32);
    }
    for (int g = 0; g < 8; g++)
        ref_g(s, G_WORDS[g][0], G_WORDS[g][1], G_WORDS[g][2], G_WORDS[g][3], m[2 * g], m[2 * g + 1], out[g]);
}

// two rows that agree on the constant columns and differ in every other one
static void row_pair(unsigned mask, uint64_t a[7], uint64_t b[7]) {
    for (int c = 0; c < 7; c++) {
        a[c] = rnd_fe();
        if ((mask >> c) & 1) {
            b[c] = a[c];
        } else {
            do b[c] = rnd_fe();
            while (b[c] == a[c]);
        }
    }
}
// what the descriptor holds: the value where the column is constant, a wrong word elsewhere
static void const_values(unsigned mask, const uint64_t row[7], uint64_t v[7]) {
    for (int c = 0; c < 7; c++) v[c] = (mask >> c) & 1 ? row[c] : ~row[c];
}

static void part_a(unsigned mask) {
    uint64_t a[7], b[7], v[7];
    row_pair(mask, a, b);
    const_values(mask, a, v);
    const B3RowPrefix p = b3_row7_prefix(v, mask);
    for (int k = 0; k < 6; k++) {
        const Digest want = b3_hash_elems<7>(a), got = b3_hash_row7(p, a);
        CHECK(std::memcmp(want.w, got.w, 32) == 0, "(a) mask %#x row %d", mask, k);
        for (int c = 0; c < 7; c++)  // the next row of the same proof
            if (!((mask >> c) & 1)) a[c] = k == 0 ? b[c] : rnd_fe();
    }
}

static void part_b(unsigned mask) {
    const unsigned ugs = b3_row7_uniform_gs(mask);
    CHECK(ugs < 256, "(b) mask %#x", mask);
    unsigned same_always = 0xFF, cons_same = 0x7F;
    uint64_t a[7], b[7], v[7];
    for (int k = 0; k < 4; k++) {
        row_pair(mask, a, b);
        uint32_t oa[8][4], ob[8][4];
        ref_round1(a, oa);
        ref_round1(b, ob);
        for (int g = 0; g < 8; g++)
            if (std::memcmp(oa[g], ob[g], 16) != 0) same_always &= ~(1u << g);
        const_values(mask, a, v);
        const B3RowPrefix p = b3_row7_prefix(v, mask);
        CHECK(p.ugs == ugs, "(b) prefix of mask %#x carries %#x", mask, p.ugs);
        // a word's latest uniform G: the diagonal one that writes it, else the column one
        for (int g = 7; g >= 0; g--)
            for (int w = 0; w < 4; w++) {
                const int word = G_WORDS[g][w];
                bool later = false;
                for (int h = g + 1; h < 8; h++)
                    for (int x = 0; x < 4; x++) later = later || (((ugs >> h) & 1) && G_WORDS[h][x] == word);
                if (((ugs >> g) & 1) && !later)
                    CHECK(p.s[word] == oa[g][w], "(b) mask %#x prefix word %d after G %d", mask, word, g);
            }
        // the AIR's read table: constraint k on the two rows (the next row's column 4 differs too unless constant)
        AirConst A = {};
        for (int i = 0; i < 12; i++) A.pub[i] = rnd_fe();
        A.nullifier = rnd_fe();
        A.commitment = rnd_fe();
        const uint64_t na = rnd_fe();
        uint64_t nb = na;
        if ((mask >> 4) & 1) {
            nb = b[4];  // a constant column: the next row's cell is the value
        } else {
            do nb = rnd_fe();
            while (nb == na);
        }
        uint64_t ra[7], rb[7];
        air_transition(A, a, (mask >> 4) & 1 ? a[4] : na, ra);
        air_transition(A, b, nb, rb);
        for (int c = 0; c < 7; c++)
            if (ra[c] != rb[c]) cons_same &= ~(1u << c);
    }
    CHECK(same_always == ugs, "(b) mask %#x: planner %#x, brute force %#x", mask, ugs, same_always);
    const unsigned ut = air_uniform_constraints(mask);
    // every marked constraint was the same on the pairs; an unmarked one reads a cell that differed (it may
    // still agree by chance on a product's zero, so only this direction is required of random data)
    CHECK((ut & ~cons_same) == 0, "(b) mask %#x: constraints marked %#x, the same on the pairs %#x", mask, ut, cons_same);
    for (int k = 0; k < 7; k++) {  // and the table itself against the constraints as written in air.hpp
        const unsigned reads = air_constraint_reads(k), cols = (reads | (reads >> 8)) & 0x7F;
        CHECK(((ut >> k) & 1) == ((cols & ~mask) == 0), "(b) mask %#x constraint %d", mask, k);
    }
}

template <int D>
static int part_c(unsigned mask) {
    using F = FE<D>;
    AirConst A = {};
    for (int i = 0; i < 12; i++) A.pub[i] = rnd_fe();
    A.nullifier = rnd_fe();
    A.commitment = rnd_fe();
    uint64_t co[15 * D], row[7], v[7];
    for (int i = 0; i < 15 * D; i++) co[i] = 1 + rnd() % (P - 1);  // no zero coefficient: a hoisted term shows
    for (int c = 0; c < 7; c++) row[c] = rnd() % P;
    const_values(mask, row, v);
    const CeUniform U = ce_uniform_of<D>(A, co, mask, v);
    int nonzero = 0;
    for (int d = 0; d < D; d++) nonzero += (U.tr[d] != 0) + (U.b0[d] != 0) + (U.b1[d] != 0);
    for (int d = 0; d < 2; d++) CHECK(U.tr[d] < P && U.b0[d] < P && U.b1[d] < P, "(c) mask %#x: not canonical", mask);
    for (int k = 0; k < 5; k++) {
        uint64_t cur[7];
        for (int c = 0; c < 7; c++) cur[c] = (mask >> c) & 1 ? row[c] : rnd_fe();
        const uint64_t nxt4 = (mask >> 4) & 1 ? row[4] : rnd_fe();
        // the full sums, as the dense evaluation forms them
        uint64_t r[7], v0[7];
        air_transition(A, cur, nxt4, r);
        air_step0_values(A, v0);
        F tr = F::zero(), b0 = F::zero();
        for (int c = 0; c < 7; c++) tr = fe_add(tr, fe_mulb(F::load(co + c * D), r[c]));
        for (int c = 0; c < 7; c++) b0 = fe_add(b0, fe_mulb(F::load(co + (7 + c) * D), gl_sub(cur[c], v0[c])));
        const F b1 = fe_mulb(F::load(co + 14 * D), gl_sub(cur[4], AIR_LAST_STATE));
        F gtr, gb0, gb1;
        ce_live_sums<D>(U, U.tr_live, U.as_live, co, A, cur, nxt4, gtr, gb0, gb1);
        for (int d = 0; d < D; d++)
            CHECK(gtr.c(d) == tr.c(d) && gb0.c(d) == b0.c(d) && gb1.c(d) == b1.c(d), "(c) D = %d mask %#x point %d", D, mask, k);
    }
    return nonzero;
}

int main() {
    long hoisted = 0;
    for (int rep = 0; rep < 4; rep++)
        for (unsigned mask = 0; mask < 128; mask++) {
            part_a(mask);
            part_b(mask);
            const int n1 = part_c<1>(mask), n2 = part_c<2>(mask);
            // every mask but the empty one hoists an assertion term at least: random constants make it non-zero
            if (mask) CHECK(n1 > 0 && n2 > 0, "(c) mask %#x hoists nothing but zeros", mask);
            else CHECK(n1 == 0 && n2 == 0, "(c) the empty mask hoists something");
            hoisted += n1 + n2;
        }
    // the burn proof's own pattern, by hand: all of round 1 but the diagonal G of column 4; six of seven constraints
    CHECK(b3_row7_uniform_gs(0x6F) == 0xEF, "planner on 0x6f: %#x", b3_row7_uniform_gs(0x6F));
    CHECK(b3_row7_uniform_gs(0x7F) == 0xFF && b3_row7_uniform_gs(0) == 0 && b3_row7_uniform_gs(0x77) == 0x07,
          "planner on the full, empty and column-3 masks");
    CHECK(air_uniform_constraints(0x6F) == 0x6F && air_uniform_constraints(0x02) == 0 && air_uniform_constraints(0x03) == 0x03,
          "constraint planner");
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("leaf_prefix ok: masks=128 reps=4 hoisted_nonzero=%ld\n", hoisted);
    return 0;
}
