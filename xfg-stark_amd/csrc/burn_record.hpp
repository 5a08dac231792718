// A burn statement as a packed record (xfg_burn_record, 128 bytes): its view as xfg_burn_inputs, its validation,
// the marshalling of its public inputs and the byte layouts of the four Keccak-256 messages of a statement. This
// header is the one statement of the validation order, the error texts and the message layouts: the host
// marshaller (marshal.hpp marshal_record, which xfg_burn_inputs go through as a record too) and the record kernel
// (burn_record.hip) both read them here, and tests/sanitize/burn_statement.cpp checks them against a hand-written
// copy of its own. Which function adds which rule: statement_status the three checks every statement has,
// record_status the record's reserved bytes behind them, marshal() (marshal.hpp) the lengths of an input's
// recipient and secret. Pure functions, no HIP: the header compiles with a plain host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "../../include/xfg_stark.h"

#if defined(__HIPCC__)
#define XFG_HD __host__ __device__
#else
#define XFG_HD
#endif

namespace xfg {

static_assert(sizeof(xfg_burn_record) == 128 && alignof(xfg_burn_record) == 8, "a record is 128 bytes");
static_assert(offsetof(xfg_burn_record, burn_amount) == 0 && offsetof(xfg_burn_record, mint_amount) == 8 &&
                  offsetof(xfg_burn_record, tx_prefix_hash) == 16 && offsetof(xfg_burn_record, recipient) == 48 &&
                  offsetof(xfg_burn_record, secret) == 68 && offsetof(xfg_burn_record, network_id) == 100 &&
                  offsetof(xfg_burn_record, target_chain_id) == 104 &&
                  offsetof(xfg_burn_record, commitment_version) == 108 && offsetof(xfg_burn_record, reserved) == 112,
              "the layout of the packed records a sharded run scatters");

constexpr uint64_t REC_STANDARD_BURN = 8000000ULL, REC_LARGE_BURN = 8000000000ULL;  // 0.8 XFG and 800 XFG

XFG_HD inline uint64_t rec_le32(const uint8_t* b) {
    return (uint64_t)b[0] | ((uint64_t)b[1] << 8) | ((uint64_t)b[2] << 16) | ((uint64_t)b[3] << 24);
}
XFG_HD inline uint64_t rec_le64(const uint8_t* b) { return rec_le32(b) | (rec_le32(b + 4) << 32); }

// the record as the arguments of prove_burn_mint: the pointers go into r, which must outlive the view
inline xfg_burn_inputs record_to_inputs(const xfg_burn_record& r) {
    xfg_burn_inputs in;
    memset(&in, 0, sizeof in);
    in.burn_amount = r.burn_amount;
    in.mint_amount = r.mint_amount;
    memcpy(in.tx_prefix_hash, r.tx_prefix_hash, 32);
    in.recipient_address = r.recipient;
    in.recipient_len = 20;
    in.secret = r.secret;
    in.secret_len = 32;
    in.network_id = r.network_id;
    in.target_chain_id = r.target_chain_id;
    in.commitment_version = r.commitment_version;
    return in;
}

// validate_inputs (src/burn_mint_prover.rs:132-221) on what every statement has, inputs and records alike: the
// first check that fails is the status. tx_legacy: the first 8 bytes of the tx hash as a LE u64
XFG_HD inline int statement_status(uint64_t burn_amount, uint64_t mint_amount, uint64_t tx_legacy) {
    if (burn_amount != REC_STANDARD_BURN && burn_amount != REC_LARGE_BURN) return XFG_INVALID_BURN_AMOUNT;
    if (mint_amount != burn_amount) return XFG_MINT_MISMATCH;
    return tx_legacy == 0 ? XFG_ZERO_TX_HASH : XFG_OK;
}
// a record: the recipient and the secret have their lengths by construction; the record's own rule, a non-zero
// reserved byte, comes last
XFG_HD inline int record_status(const xfg_burn_record& r) {
    if (const int st = statement_status(r.burn_amount, r.mint_amount, rec_le64(r.tx_prefix_hash))) return st;
    uint8_t any = 0;
    for (int i = 0; i < 16; i++) any |= r.reserved[i];
    return any ? XFG_INVALID_ARGUMENT : XFG_OK;
}
// the text of such a status, the reference's (the mint mismatch names the statement's two amounts)
inline std::string record_status_text(int status, uint64_t burn_amount, uint64_t mint_amount) {
    switch (status) {
        case XFG_INVALID_BURN_AMOUNT:
            return "Burn amount must be exactly 0.8 XFG (8,000,000 atomic units) or 800 XFG (8,000,000,000 atomic units)";
        case XFG_MINT_MISMATCH:
            return "Mint amount " + std::to_string(mint_amount) + " does not match burn amount " +
                   std::to_string(burn_amount) + " for 1:1 atomic unit conversion";
        case XFG_ZERO_TX_HASH: return "Transaction hash must be greater than 0";
        case XFG_INVALID_ARGUMENT: return "record: the reserved bytes must be zero";
        default: return "";
    }
}

// the 12 public inputs as prove_burn_mint forms them, every one a 32-bit value (hence a canonical field element), for
// an invalid record too; pub[3], the recipient hash, is left 0 for the caller to fill in. The secret's field
// element is the first four bytes of the secret
XFG_HD inline void record_public_inputs(const xfg_burn_record& r, uint64_t pub[12]) {
    pub[0] = (uint32_t)r.burn_amount;
    pub[1] = (uint32_t)r.mint_amount;
    pub[2] = rec_le32(r.tx_prefix_hash);
    pub[3] = 0;
    pub[4] = 0;
    for (int i = 0; i < 4; i++) pub[5 + i] = rec_le32(r.tx_prefix_hash + 4 * i);
    pub[9] = r.network_id;
    pub[10] = r.target_chain_id;
    pub[11] = r.commitment_version;
}
XFG_HD inline uint64_t record_secret(const xfg_burn_record& r) { return rec_le32(r.secret); }

// ---- the four Keccak-256 messages of a statement (compute_recipient_hash, compute_nullifier, the 32-byte
// recipient hash inside compute_commitment, compute_commitment: src/burn_mint_air.rs:124-202,
// src/burn_mint_prover.rs:211-221). u64 fields are little-endian:
//   RECIPIENT       recipient[20] "recipient"                                                   -> pub[3] = LE32 of the hash
//   NULLIFIER       secret "nullifier" pub[0]                                                   -> nullifier = LE32
//   RECIPIENT_FULL  pub[3] "ethereum-recipient" "fuego-to-heat-bridge"                          -> rf, all 32 bytes
//   COMMITMENT      secret pub[0] pub[1] pub[5..8] rf[32] pub[9..11] "heat-commitment-v1"       -> commitment = LE32
enum BurnMsg : int { MSG_RECIPIENT = 0, MSG_NULLIFIER = 1, MSG_RECIPIENT_FULL = 2, MSG_COMMITMENT = 3 };
constexpr unsigned KECCAK_RATE = 136;  // bytes of a Keccak-256 block
XFG_HD constexpr unsigned burn_msg_len(int which) {
    return which == MSG_RECIPIENT ? 20 + 9 : which == MSG_NULLIFIER ? 8 + 9 + 8 : which == MSG_RECIPIENT_FULL ? 8 + 18 + 20 : 8 * 7 + 32 + 8 * 3 + 18;
}
static_assert(burn_msg_len(MSG_RECIPIENT) == 29 && burn_msg_len(MSG_NULLIFIER) == 25 &&
                  burn_msg_len(MSG_RECIPIENT_FULL) == 46 && burn_msg_len(MSG_COMMITMENT) == 130,
              "the four message lengths");
static_assert(burn_msg_len(MSG_COMMITMENT) < KECCAK_RATE, "every message is one Keccak block with its padding");

// what the messages are made of. rf: the recipient-full hash as four LE words (COMMITMENT only); pub[3] is read
// by RECIPIENT_FULL
struct BurnMsgSrc {
    const uint8_t* recipient;  // 20 bytes
    uint64_t secret;
    uint64_t pub[12];
    uint64_t rf[4];
};
XFG_HD inline uint8_t msg_text(const char* text, unsigned k) { return (uint8_t)text[k]; }
XFG_HD inline uint8_t msg_u64(uint64_t v, unsigned k) { return (uint8_t)(v >> (8 * k)); }
// byte k of message `which`, 0 from its length on. Every field is picked by comparisons, never by a computed
// index into the struct (the kernel keeps it in registers)
XFG_HD inline uint8_t burn_msg_byte(int which, unsigned k, const BurnMsgSrc& s) {
    if (k >= burn_msg_len(which)) return 0;
    if (which == MSG_RECIPIENT) return k < 20 ? s.recipient[k] : msg_text("recipient", k - 20);
    if (which == MSG_NULLIFIER)
        return k < 8 ? msg_u64(s.secret, k) : k < 17 ? msg_text("nullifier", k - 8) : msg_u64(s.pub[0], k - 17);
    if (which == MSG_RECIPIENT_FULL)
        return k < 8 ? msg_u64(s.pub[3], k) : k < 26 ? msg_text("ethereum-recipient", k - 8) : msg_text("fuego-to-heat-bridge", k - 26);
    if (k >= 112) return msg_text("heat-commitment-v1", k - 112);
    const unsigned w = k >> 3;  // whole words up to byte 112
    const uint64_t v = w == 0 ? s.secret : w == 1 ? s.pub[0] : w == 2 ? s.pub[1] : w == 3 ? s.pub[5] : w == 4 ? s.pub[6]
                     : w == 5 ? s.pub[7] : w == 6 ? s.pub[8] : w == 7 ? s.rf[0] : w == 8 ? s.rf[1] : w == 9 ? s.rf[2]
                     : w == 10 ? s.rf[3] : w == 11 ? s.pub[9] : w == 12 ? s.pub[10] : s.pub[11];
    return msg_u64(v, k & 7);
}
// LE word i (0..16) of the message's block, before the padding
XFG_HD inline uint64_t burn_msg_word(int which, unsigned i, const BurnMsgSrc& s) {
    uint64_t w = 0;
    for (unsigned j = 0; j < 8; j++) w |= (uint64_t)burn_msg_byte(which, 8 * i + j, s) << (8 * j);
    return w;
}
// what Keccak's padding of a message of len <= 135 bytes adds to LE word i (0..16) of its block: 0x01 at byte len,
// 0x80 at byte 135; at len 135 the two meet in one byte, 0x81 (SHA-3 would start with 0x06)
XFG_HD inline uint64_t keccak_pad_word(unsigned i, unsigned len) {
    uint64_t w = 0;
    if ((len >> 3) == i) w ^= 1ULL << (8 * (len & 7));
    if (i == KECCAK_RATE / 8 - 1) w ^= 0x80ULL << 56;
    return w;
}
// the message as bytes (host): out[136] zero-filled past the length, which is returned. Unrolled in full: with
// `which` a constant at the call, every byte's comparisons fold away and the stores merge into whole fields, which
// puts the host marshaller on the submitting thread level with one that copies the fields in by hand
inline unsigned burn_msg_bytes(int which, const BurnMsgSrc& s, uint8_t out[KECCAK_RATE]) {
#pragma GCC unroll 136
    for (unsigned k = 0; k < KECCAK_RATE; k++) out[k] = burn_msg_byte(which, k, s);
    return burn_msg_len(which);
}

}  // namespace xfg
