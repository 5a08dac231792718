// Host driver for xfg-stark_amd/csrc/burn_record.hpp and the one host marshaller behind it (marshal.hpp): the
// record's size and offsets against the table of include/xfg_stark.h, record_to_inputs, the validation order (a
// statement wrong in two ways reports the earlier status, inputs and records with the same text), the length rules
// of xfg_burn_inputs on buffers of their exact lengths, the four Keccak message layouts against messages assembled
// by hand, the marshalled constants against this file's own hand-written marshalling (expected_air: it shares no
// code with the headers under test) on random and edge records, and the padding words. Built with ASan + UBSan
// (make build/asan/burn_statement; host code of the shared headers) and run directly.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../xfg-stark_amd/csrc/marshal.hpp"

using namespace xfg;

static int failures = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                            \
        }                                                          \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static xfg_burn_record random_record() {
    xfg_burn_record r;
    uint8_t* b = (uint8_t*)&r;
    for (size_t i = 0; i < sizeof r; i++) b[i] = (uint8_t)rnd();
    r.burn_amount = r.mint_amount = (rnd() & 1) ? REC_STANDARD_BURN : REC_LARGE_BURN;
    r.tx_prefix_hash[0] |= 1;
    memset(r.reserved, 0, sizeof r.reserved);
    return r;
}

// ---- the independent expectation: a statement's constants marshalled by hand, the messages assembled with memcpy
// (compute_nullifier / compute_recipient_hash / compute_commitment, src/burn_mint_air.rs:124-202; prove_burn_mint,
// src/burn_mint_prover.rs:62-118). Nothing below uses burn_record.hpp's helpers
static uint64_t le_u32(const uint8_t* b) {
    return (uint64_t)b[0] | ((uint64_t)b[1] << 8) | ((uint64_t)b[2] << 16) | ((uint64_t)b[3] << 24);
}
static uint64_t le_u64(const uint8_t* b) { return le_u32(b) | (le_u32(b + 4) << 32); }
static void put_le64(uint8_t* d, uint64_t v) {
    for (int i = 0; i < 8; i++) d[i] = (uint8_t)(v >> (8 * i));
}
static void air_constants(const uint64_t pub[12], uint64_t secret, uint64_t& nullifier, uint64_t& commitment) {
    uint8_t buf[160], h[32], rf[32];
    size_t k = 0;
    put_le64(buf, secret);
    k = 8;
    memcpy(buf + k, "nullifier", 9);
    k += 9;
    put_le64(buf + k, pub[0]);
    k += 8;
    keccak256(buf, k, h);
    nullifier = le_u32(h);
    k = 0;
    put_le64(buf, pub[3]);
    k = 8;
    memcpy(buf + k, "ethereum-recipient", 18);
    k += 18;
    memcpy(buf + k, "fuego-to-heat-bridge", 20);
    k += 20;
    keccak256(buf, k, rf);
    k = 0;
    const uint64_t fields[3] = {secret, pub[0], pub[1]};
    for (uint64_t f : fields) { put_le64(buf + k, f); k += 8; }
    for (int i = 0; i < 4; i++) { put_le64(buf + k, pub[5 + i]); k += 8; }
    memcpy(buf + k, rf, 32);
    k += 32;
    for (int i = 0; i < 3; i++) { put_le64(buf + k, pub[9 + i]); k += 8; }
    memcpy(buf + k, "heat-commitment-v1", 18);
    k += 18;
    keccak256(buf, k, h);
    commitment = le_u32(h);
}
// the constants of a record's statement, whether or not it is valid (20-byte recipient, at least 4 secret bytes)
static AirConst expected_air(const xfg_burn_record& r) {
    uint8_t buf[29], h[32];
    memcpy(buf, r.recipient, 20);
    memcpy(buf + 20, "recipient", 9);
    keccak256(buf, 29, h);
    AirConst a;
    memset(&a, 0, sizeof a);
    a.pub[0] = (uint32_t)r.burn_amount;
    a.pub[1] = (uint32_t)r.mint_amount;
    a.pub[2] = (uint32_t)le_u64(r.tx_prefix_hash);
    a.pub[3] = le_u32(h);
    a.pub[4] = 0;
    for (int i = 0; i < 4; i++) a.pub[5 + i] = le_u32(r.tx_prefix_hash + 4 * i);
    a.pub[9] = r.network_id;
    a.pub[10] = r.target_chain_id;
    a.pub[11] = r.commitment_version;
    air_constants(a.pub, le_u32(r.secret), a.nullifier, a.commitment);
    return a;
}

static void check_layout() {
    CHECK(sizeof(xfg_burn_record) == 128);
    CHECK(offsetof(xfg_burn_record, burn_amount) == 0);
    CHECK(offsetof(xfg_burn_record, mint_amount) == 8);
    CHECK(offsetof(xfg_burn_record, tx_prefix_hash) == 16);
    CHECK(offsetof(xfg_burn_record, recipient) == 48);
    CHECK(offsetof(xfg_burn_record, secret) == 68);
    CHECK(offsetof(xfg_burn_record, network_id) == 100);
    CHECK(offsetof(xfg_burn_record, target_chain_id) == 104);
    CHECK(offsetof(xfg_burn_record, commitment_version) == 108);
    CHECK(offsetof(xfg_burn_record, reserved) == 112);
    // little-endian fields, as the packed bytes of a scattered record state them
    uint8_t raw[128];
    for (int i = 0; i < 128; i++) raw[i] = (uint8_t)(i + 1);
    xfg_burn_record r;
    memcpy(&r, raw, 128);
    CHECK(r.burn_amount == 0x0807060504030201ULL && r.mint_amount == 0x100F0E0D0C0B0A09ULL);
    CHECK(r.tx_prefix_hash[0] == 17 && r.recipient[0] == 49 && r.recipient[19] == 68 && r.secret[0] == 69);
    CHECK(r.network_id == 0x68676665u && r.target_chain_id == 0x6C6B6A69u && r.commitment_version == 0x706F6E6Du);
    CHECK(r.reserved[0] == 113 && r.reserved[15] == 128);
}

static void check_view() {
    const xfg_burn_record r = random_record();
    const xfg_burn_inputs in = record_to_inputs(r);
    CHECK(in.burn_amount == r.burn_amount && in.mint_amount == r.mint_amount);
    CHECK(!memcmp(in.tx_prefix_hash, r.tx_prefix_hash, 32));
    CHECK(in.recipient_address == r.recipient && in.recipient_len == 20);
    CHECK(in.secret == r.secret && in.secret_len == 32);
    CHECK(in.network_id == r.network_id && in.target_chain_id == r.target_chain_id &&
          in.commitment_version == r.commitment_version);
}

// what marshal() must leave alone for an invalid statement
static AirConst untouched() {
    AirConst a;
    memset(&a, 0xA5, sizeof a);
    return a;
}
// the reference's texts (src/burn_mint_prover.rs:132-221), spelt out here and nowhere else in this file
static std::string expected_text(int status, uint64_t burn, uint64_t mint) {
    switch (status) {
        case XFG_INVALID_BURN_AMOUNT:
            return "Burn amount must be exactly 0.8 XFG (8,000,000 atomic units) or 800 XFG (8,000,000,000 atomic units)";
        case XFG_MINT_MISMATCH:
            return "Mint amount " + std::to_string(mint) + " does not match burn amount " + std::to_string(burn) +
                   " for 1:1 atomic unit conversion";
        case XFG_ZERO_TX_HASH: return "Transaction hash must be greater than 0";
        case XFG_BAD_RECIPIENT_LEN: return "Recipient address must be exactly 20 bytes";
        default: return "";
    }
}

// status and text of a record against marshal() on its view; the reserved bytes are the record's own rule. The
// constants of both forms against the hand-written ones
static void check_status(const xfg_burn_record& r, int want) {
    CHECK(record_status(r) == want);
    AirConst a = untouched(), b;
    std::string ea, eb;
    const xfg_burn_inputs in = record_to_inputs(r);
    const int host = marshal(&in, a, ea);
    const int rec = marshal_record(r, b, eb);
    const AirConst expect = expected_air(r), none = untouched();
    CHECK(rec == want);
    CHECK(!memcmp(&b, &expect, sizeof b));  // filled in for an invalid record too
    if (want != XFG_INVALID_ARGUMENT) {
        CHECK(host == want);
        CHECK(ea == eb);
        CHECK(ea == expected_text(want, r.burn_amount, r.mint_amount));
    } else {
        CHECK(host == XFG_OK);
        CHECK(eb == "record: the reserved bytes must be zero");
    }
    CHECK(!memcmp(&a, host == XFG_OK ? &expect : &none, sizeof a));
}
static void check_validation() {
    xfg_burn_record ok = random_record();
    check_status(ok, XFG_OK);
    xfg_burn_record r = ok;
    r.burn_amount = r.mint_amount = REC_LARGE_BURN;
    check_status(r, XFG_OK);
    r = ok;
    r.burn_amount = 0;
    check_status(r, XFG_INVALID_BURN_AMOUNT);  // and a mint mismatch behind it
    r.mint_amount = 0;
    check_status(r, XFG_INVALID_BURN_AMOUNT);
    memset(r.tx_prefix_hash, 0, 8);
    r.reserved[3] = 1;
    check_status(r, XFG_INVALID_BURN_AMOUNT);  // wrong in every way: the first check
    r = ok;
    r.mint_amount = r.burn_amount + 1;
    check_status(r, XFG_MINT_MISMATCH);
    memset(r.tx_prefix_hash, 0, 8);
    r.reserved[0] = 0xFF;
    check_status(r, XFG_MINT_MISMATCH);  // before the tx hash and the reserved bytes
    r = ok;
    memset(r.tx_prefix_hash, 0, 8);
    check_status(r, XFG_ZERO_TX_HASH);
    r.reserved[15] = 1;
    check_status(r, XFG_ZERO_TX_HASH);  // before the reserved bytes
    r = ok;
    memset(r.tx_prefix_hash, 0, 4);
    r.tx_prefix_hash[4] = 1;
    check_status(r, XFG_OK);  // the u64 is non-zero although pub[2], its low word, is 0
    uint64_t pub[12];
    record_public_inputs(r, pub);
    CHECK(pub[2] == 0 && pub[5] == 0 && pub[6] != 0);
    for (int i = 0; i < 16; i++) {
        r = ok;
        r.reserved[i] = 0x80;
        check_status(r, XFG_INVALID_ARGUMENT);
    }
    CHECK(record_status_text(XFG_MINT_MISMATCH, 8000000, 7) ==
          "Mint amount 7 does not match burn amount 8000000 for 1:1 atomic unit conversion");
}

// ---- the rules only xfg_burn_inputs can break: the lengths of the recipient and the secret. Both buffers are heap
// allocations of exactly the stated length (none for a null pointer), so ASan sees any read past them
struct SizedInputs {
    std::unique_ptr<uint8_t[]> recipient, secret;
    xfg_burn_inputs in;
};
static const size_t NO_BUFFER = (size_t)-1;  // a null pointer, its length stated as the valid 20 or 32
static void inputs_of(SizedInputs& s, const xfg_burn_record& r, size_t rlen, size_t slen) {
    s.in = record_to_inputs(r);
    s.in.recipient_address = nullptr;
    s.in.secret = nullptr;
    if (rlen != NO_BUFFER) {
        s.recipient.reset(new uint8_t[rlen]);
        for (size_t i = 0; i < rlen; i++) s.recipient[i] = i < 20 ? r.recipient[i] : (uint8_t)rnd();
        s.in.recipient_address = s.recipient.get();
        s.in.recipient_len = rlen;
    }
    if (slen != NO_BUFFER) {
        s.secret.reset(new uint8_t[slen]);
        for (size_t i = 0; i < slen; i++) s.secret[i] = i < 32 ? r.secret[i] : (uint8_t)rnd();
        s.in.secret = s.secret.get();
        s.in.secret_len = slen;
    }
}
// marshal() on r's statement with buffers of these lengths gives `want` with `text`; on top of each of the three
// earlier failures it gives that failure, text included, and an invalid statement leaves the constants alone.
// A valid one gives the constants of the record whose secret is the first min(slen, 32) bytes, zero-filled
static void check_lengths(const xfg_burn_record& ok, size_t rlen, size_t slen, int want, const char* text) {
    xfg_burn_record early[4] = {ok, ok, ok, ok};
    early[1].burn_amount = 7;  // and a mint mismatch behind it
    early[2].mint_amount = ok.burn_amount - 1;
    memset(early[3].tx_prefix_hash, 0, 8);
    const int early_status[4] = {XFG_OK, XFG_INVALID_BURN_AMOUNT, XFG_MINT_MISMATCH, XFG_ZERO_TX_HASH};
    for (int e = 0; e < 4; e++) {
        const xfg_burn_record& r = early[e];
        SizedInputs s;
        inputs_of(s, r, rlen, slen);
        AirConst a = untouched();
        std::string err;
        const int st = marshal(&s.in, a, err);
        const AirConst none = untouched();
        if (e) {
            CHECK(st == early_status[e]);
            CHECK(err == expected_text(st, r.burn_amount, r.mint_amount));
            AirConst b;
            std::string eb;
            CHECK(marshal_record(r, b, eb) == st && eb == err);  // the record form words it the same
        } else {
            CHECK(st == want);
            CHECK(err == text);
        }
        if (st) {
            CHECK(!memcmp(&a, &none, sizeof a));
            continue;
        }
        xfg_burn_record cut = r;
        memset(cut.secret, 0, sizeof cut.secret);
        memcpy(cut.secret, r.secret, std::min<size_t>(slen, 32));
        const AirConst expect = expected_air(cut);
        AirConst b;
        CHECK(marshal_record(cut, b, err) == XFG_OK);
        CHECK(!memcmp(&a, &expect, sizeof a) && !memcmp(&a, &b, sizeof a));
    }
}
static void check_input_lengths() {
    const xfg_burn_record ok = random_record();
    const char* const recipient = "Recipient address must be exactly 20 bytes";
    const char* const secret4 = "Secret must be at least 4 bytes";
    const char* const secret8 = "Secret must be at least 8 bytes (secret[..8] slice in secret_to_field_element)";
    check_lengths(ok, NO_BUFFER, 32, XFG_BAD_RECIPIENT_LEN, recipient);
    check_lengths(ok, 19, 32, XFG_BAD_RECIPIENT_LEN, recipient);
    check_lengths(ok, 21, 32, XFG_BAD_RECIPIENT_LEN, recipient);
    check_lengths(ok, 19, 3, XFG_BAD_RECIPIENT_LEN, recipient);  // the recipient before the secret
    check_lengths(ok, NO_BUFFER, NO_BUFFER, XFG_BAD_RECIPIENT_LEN, recipient);
    check_lengths(ok, 20, NO_BUFFER, XFG_SHORT_SECRET, secret4);
    check_lengths(ok, 20, 0, XFG_SHORT_SECRET, secret4);
    check_lengths(ok, 20, 3, XFG_SHORT_SECRET, secret4);
    check_lengths(ok, 20, 4, XFG_SHORT_SECRET, secret8);
    check_lengths(ok, 20, 7, XFG_SHORT_SECRET, secret8);
    check_lengths(ok, 20, 8, XFG_OK, "");
    check_lengths(ok, 20, 32, XFG_OK, "");
    check_lengths(ok, 20, 40, XFG_OK, "");
}

// the messages assembled by hand from the record, independently of burn_msg_byte
static void append(std::vector<uint8_t>& m, uint64_t v) {
    for (int i = 0; i < 8; i++) m.push_back((uint8_t)(v >> (8 * i)));
}
static void append(std::vector<uint8_t>& m, const char* s) {
    while (*s) m.push_back((uint8_t)*s++);
}
static void check_messages(const xfg_burn_record& r) {
    const AirConst want = expected_air(r);  // of an invalid record too
    std::string err;

    BurnMsgSrc s;
    memset(&s, 0, sizeof s);
    s.recipient = r.recipient;
    s.secret = record_secret(r);
    record_public_inputs(r, s.pub);
    CHECK(s.secret == le_u32(r.secret));
    uint8_t msg[KECCAK_RATE], h[32];
    std::vector<uint8_t> m;

    m.assign(r.recipient, r.recipient + 20);
    append(m, "recipient");
    CHECK(burn_msg_bytes(MSG_RECIPIENT, s, msg) == 29 && m.size() == 29 && !memcmp(msg, m.data(), 29));
    keccak256(msg, 29, h);
    s.pub[3] = le_u32(h);
    CHECK(s.pub[3] == want.pub[3]);  // the recipient does not depend on what makes a record invalid

    m.clear();
    append(m, s.secret), append(m, "nullifier"), append(m, s.pub[0]);
    CHECK(burn_msg_bytes(MSG_NULLIFIER, s, msg) == 25 && m.size() == 25 && !memcmp(msg, m.data(), 25));
    keccak256(msg, 25, h);
    const uint64_t nullifier = le_u32(h);

    m.clear();
    append(m, s.pub[3]), append(m, "ethereum-recipient"), append(m, "fuego-to-heat-bridge");
    CHECK(burn_msg_bytes(MSG_RECIPIENT_FULL, s, msg) == 46 && m.size() == 46 && !memcmp(msg, m.data(), 46));
    keccak256(msg, 46, h);
    for (int i = 0; i < 4; i++) s.rf[i] = le_u64(h + 8 * i);

    m.clear();
    append(m, s.secret), append(m, s.pub[0]), append(m, s.pub[1]);
    for (int i = 5; i < 9; i++) append(m, s.pub[i]);
    m.insert(m.end(), h, h + 32);
    for (int i = 9; i < 12; i++) append(m, s.pub[i]);
    append(m, "heat-commitment-v1");
    CHECK(burn_msg_bytes(MSG_COMMITMENT, s, msg) == 130 && m.size() == 130 && !memcmp(msg, m.data(), 130));
    for (unsigned k = 130; k < KECCAK_RATE; k++) CHECK(msg[k] == 0);
    keccak256(msg, 130, h);
    const uint64_t commitment = le_u32(h);

    // against this file's memcpy assembly of the same hashes, and the marshaller against both
    uint64_t nf = 0, cm = 0;
    air_constants(s.pub, s.secret, nf, cm);
    CHECK(nf == nullifier && cm == commitment);
    AirConst got;
    marshal_record(r, got, err);
    CHECK(got.nullifier == nullifier && got.commitment == commitment && !memcmp(got.pub, s.pub, sizeof got.pub));
    CHECK(!memcmp(&got, &want, sizeof got));
    // the words of a block are its bytes
    for (int which = 0; which < 4; which++) {
        burn_msg_bytes(which, s, msg);
        for (unsigned i = 0; i < KECCAK_RATE / 8; i++) CHECK(burn_msg_word(which, i, s) == le_u64(msg + 8 * i));
    }
}

// keccak_pad_word against the padding keccak256 applies: a block built from the words hashes like the message
static void check_padding() {
    for (unsigned len = 0; len < KECCAK_RATE; len++) {
        uint8_t block[KECCAK_RATE] = {0}, want[KECCAK_RATE] = {0};
        want[len] ^= 0x01;
        want[KECCAK_RATE - 1] ^= 0x80;
        for (unsigned i = 0; i < KECCAK_RATE / 8; i++) put_le64(block + 8 * i, keccak_pad_word(i, len));
        CHECK(!memcmp(block, want, KECCAK_RATE));
    }
    uint8_t last[8];
    put_le64(last, keccak_pad_word(16, 135));
    CHECK(last[7] == 0x81);
    put_le64(last, keccak_pad_word(16, 134));
    CHECK(last[6] == 0x01 && last[7] == 0x80);
}

int main() {
    check_layout();
    check_view();
    check_validation();
    check_input_lengths();
    check_padding();
    for (int i = 0; i < 200; i++) {
        const xfg_burn_record r = random_record();
        check_messages(r);
        check_status(r, XFG_OK);  // both forms of a valid statement against the hand-written constants
    }
    // edge records: all ones, all zeros (invalid: the constants are marshalled all the same), extreme ids
    xfg_burn_record r;
    memset(&r, 0xFF, sizeof r);
    check_messages(r);
    r.burn_amount = r.mint_amount = REC_LARGE_BURN;
    memset(r.reserved, 0, sizeof r.reserved);
    check_messages(r);
    check_status(r, XFG_OK);
    memset(&r, 0, sizeof r);
    check_messages(r);
    r = random_record();
    r.network_id = 0, r.target_chain_id = 0xFFFFFFFFu, r.commitment_version = 0;
    check_messages(r);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("burn_statement ok\n");
    return 0;
}
