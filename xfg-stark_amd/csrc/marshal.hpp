// Input validation and marshalling of a burn statement into the AIR constants (host only):
// validate_inputs + prove_burn_mint marshalling of the reference, same checks, error text and
// status codes.
#pragma once
#include <string>

#include "burn_record.hpp"
#include "host_common.hpp"
#include "kernels.hpp"

namespace xfg {

static const u64 STANDARD_BURN = 8000000ULL, LARGE_BURN = 8000000000ULL;
static inline u64 le_u32(const uint8_t* b) {
    return (u64)b[0] | ((u64)b[1] << 8) | ((u64)b[2] << 16) | ((u64)b[3] << 24);
}
static inline u64 le_u64(const uint8_t* b) { return le_u32(b) | (le_u32(b + 4) << 32); }
static inline void put_le64(uint8_t* d, u64 v) {
    for (int i = 0; i < 8; i++) d[i] = (uint8_t)(v >> (8 * i));
}

// compute_nullifier / compute_recipient_hash / compute_commitment (src/burn_mint_air.rs:124-202)
static inline void air_constants(const u64 pub[12], u64 secret, u64& nullifier, u64& commitment) {
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
    const u64 fields[3] = {secret, pub[0], pub[1]};
    for (u64 f : fields) { put_le64(buf + k, f); k += 8; }
    for (int i = 0; i < 4; i++) { put_le64(buf + k, pub[5 + i]); k += 8; }
    memcpy(buf + k, rf, 32);
    k += 32;
    for (int i = 0; i < 3; i++) { put_le64(buf + k, pub[9 + i]); k += 8; }
    memcpy(buf + k, "heat-commitment-v1", 18);
    k += 18;
    keccak256(buf, k, h);
    commitment = le_u32(h);
}

// validate_inputs + prove_burn_mint marshalling (src/burn_mint_prover.rs:62-118, 132-221)
static inline int marshal(const xfg_burn_inputs* in, AirConst& a, std::string& err) {
    u64 legacy = le_u64(in->tx_prefix_hash);
    if (in->burn_amount != STANDARD_BURN && in->burn_amount != LARGE_BURN) {
        err = "Burn amount must be exactly 0.8 XFG (8,000,000 atomic units) or 800 XFG (8,000,000,000 atomic units)";
        return XFG_INVALID_BURN_AMOUNT;
    }
    if (in->mint_amount != in->burn_amount) {
        err = "Mint amount " + std::to_string(in->mint_amount) + " does not match burn amount " +
              std::to_string(in->burn_amount) + " for 1:1 atomic unit conversion";
        return XFG_MINT_MISMATCH;
    }
    if (legacy == 0) {
        err = "Transaction hash must be greater than 0";
        return XFG_ZERO_TX_HASH;
    }
    if (!in->recipient_address || in->recipient_len != 20) {
        err = "Recipient address must be exactly 20 bytes";
        return XFG_BAD_RECIPIENT_LEN;
    }
    if (!in->secret || in->secret_len < 4) {
        err = "Secret must be at least 4 bytes";
        return XFG_SHORT_SECRET;
    }
    if (in->secret_len < 8) {  // the reference slices secret[..8] and panics (:203-204)
        err = "Secret must be at least 8 bytes (secret[..8] slice in secret_to_field_element)";
        return XFG_SHORT_SECRET;
    }
    u64 secret = le_u32(in->secret);
    uint8_t buf[29], h[32];
    memcpy(buf, in->recipient_address, 20);
    memcpy(buf + 20, "recipient", 9);
    keccak256(buf, 29, h);
    memset(&a, 0, sizeof a);
    a.pub[0] = (uint32_t)in->burn_amount;
    a.pub[1] = (uint32_t)in->mint_amount;
    a.pub[2] = (uint32_t)legacy;
    a.pub[3] = le_u32(h);
    a.pub[4] = 0;
    for (int i = 0; i < 4; i++) a.pub[5 + i] = le_u32(in->tx_prefix_hash + 4 * i);
    a.pub[9] = in->network_id;
    a.pub[10] = in->target_chain_id;
    a.pub[11] = in->commitment_version;
    air_constants(a.pub, secret, a.nullifier, a.commitment);
    return XFG_OK;
}

// marshal() for a packed record, through the helpers the record kernel shares (burn_record.hpp): the status and
// the text are marshal()'s for record_to_inputs(r); the constants are filled in for an invalid record too
static inline int marshal_record(const xfg_burn_record& r, AirConst& a, std::string& err) {
    const int st = record_status(r);
    if (st) err = record_status_text(st, r.burn_amount, r.mint_amount);
    BurnMsgSrc s;
    memset(&s, 0, sizeof s);
    s.recipient = r.recipient;
    s.secret = record_secret(r);
    record_public_inputs(r, s.pub);
    uint8_t msg[KECCAK_RATE], h[32];
    keccak256(msg, burn_msg_bytes(MSG_RECIPIENT, s, msg), h);
    s.pub[3] = le_u32(h);
    keccak256(msg, burn_msg_bytes(MSG_NULLIFIER, s, msg), h);
    const u64 nullifier = le_u32(h);
    keccak256(msg, burn_msg_bytes(MSG_RECIPIENT_FULL, s, msg), h);
    for (int i = 0; i < 4; i++) s.rf[i] = le_u64(h + 8 * i);
    keccak256(msg, burn_msg_bytes(MSG_COMMITMENT, s, msg), h);
    memset(&a, 0, sizeof a);
    memcpy(a.pub, s.pub, sizeof a.pub);
    a.nullifier = nullifier;
    a.commitment = le_u32(h);
    return st;
}

}  // namespace xfg
