// Host driver for xfg-stark_amd/csrc/burn_record.hpp: the record's size and offsets against the table of
// include/xfg_stark.h, record_to_inputs, the validation order (a record wrong in two ways reports the earlier
// status, with marshal()'s text), the four Keccak message layouts against messages assembled by hand and against
// marshal.hpp's air_constants / marshal() on random and edge records, and the padding words. Built with ASan +
// UBSan (make build/asan/burn_record; host code of the shared headers) and run directly.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// status and text of a record against marshal() on its view; the reserved bytes are the record's own rule
static void check_status(const xfg_burn_record& r, int want) {
    CHECK(record_status(r) == want);
    AirConst a, b;
    std::string ea, eb;
    const xfg_burn_inputs in = record_to_inputs(r);
    const int host = marshal(&in, a, ea);
    const int rec = marshal_record(r, b, eb);
    CHECK(rec == want);
    if (want != XFG_INVALID_ARGUMENT) {
        CHECK(host == want);
        CHECK(ea == eb);
    } else {
        CHECK(host == XFG_OK);
        CHECK(eb == "record: the reserved bytes must be zero");
    }
    if (host == XFG_OK) CHECK(!memcmp(&a, &b, sizeof a));
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

// the messages assembled by hand from the record, independently of burn_msg_byte
static void append(std::vector<uint8_t>& m, uint64_t v) {
    for (int i = 0; i < 8; i++) m.push_back((uint8_t)(v >> (8 * i)));
}
static void append(std::vector<uint8_t>& m, const char* s) {
    while (*s) m.push_back((uint8_t)*s++);
}
static void check_messages(const xfg_burn_record& r) {
    AirConst want;
    std::string err;
    const xfg_burn_inputs in = record_to_inputs(r);
    xfg_burn_inputs valid = in;  // the constants of an invalid record: marshal() on a statement made valid
    valid.burn_amount = valid.mint_amount = REC_STANDARD_BURN;
    if (le_u64(valid.tx_prefix_hash) == 0) valid.tx_prefix_hash[7] = 1;
    const bool as_is = marshal(&in, want, err) == XFG_OK;
    if (!as_is) CHECK(marshal(&valid, want, err) == XFG_OK);

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

    // against marshal.hpp's own assembly of the same hashes
    uint64_t nf = 0, cm = 0;
    air_constants(s.pub, s.secret, nf, cm);
    CHECK(nf == nullifier && cm == commitment);
    AirConst got;
    marshal_record(r, got, err);
    CHECK(got.nullifier == nullifier && got.commitment == commitment && !memcmp(got.pub, s.pub, sizeof got.pub));
    if (as_is) CHECK(!memcmp(&got, &want, sizeof got));
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
    check_padding();
    for (int i = 0; i < 200; i++) check_messages(random_record());
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
    printf("burn_record ok\n");
    return 0;
}
