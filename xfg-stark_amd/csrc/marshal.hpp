// Input validation and marshalling of a burn statement into the AIR constants (host only): validate_inputs +
// prove_burn_mint marshalling of the reference (src/burn_mint_prover.rs:62-118, 132-221), same checks, error text
// and status codes. There is one marshaller, marshal_record: the validation order, the texts and the message
// layouts are burn_record.hpp's, shared with the record kernel. marshal() adds what only xfg_burn_inputs can get
// wrong, the lengths of the recipient and the secret, and hands the statement on as a record.
#pragma once
#include <algorithm>
#include <string>

#include "burn_record.hpp"
#include "host_common.hpp"
#include "kernels.hpp"

namespace xfg {

// a packed record: status and text from record_status (the reserved bytes are the record's own rule, behind the
// three shared checks); the constants are filled in for an invalid record too
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
    s.pub[3] = rec_le32(h);
    keccak256(msg, burn_msg_bytes(MSG_NULLIFIER, s, msg), h);
    const u64 nullifier = rec_le32(h);
    keccak256(msg, burn_msg_bytes(MSG_RECIPIENT_FULL, s, msg), h);
    for (int i = 0; i < 4; i++) s.rf[i] = rec_le64(h + 8 * i);
    keccak256(msg, burn_msg_bytes(MSG_COMMITMENT, s, msg), h);
    memset(&a, 0, sizeof a);
    memcpy(a.pub, s.pub, sizeof a.pub);
    a.nullifier = nullifier;
    a.commitment = rec_le32(h);
    return st;
}

// xfg_burn_inputs: the three shared checks first, then the two length rules (neither pointer is read before its
// rule has passed), then the statement as a record through marshal_record. a is left untouched for an invalid one
static inline int marshal(const xfg_burn_inputs* in, AirConst& a, std::string& err) {
    if (const int st = statement_status(in->burn_amount, in->mint_amount, rec_le64(in->tx_prefix_hash))) {
        err = record_status_text(st, in->burn_amount, in->mint_amount);
        return st;
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
    xfg_burn_record r;
    memset(&r, 0, sizeof r);
    r.burn_amount = in->burn_amount;
    r.mint_amount = in->mint_amount;
    memcpy(r.tx_prefix_hash, in->tx_prefix_hash, 32);
    memcpy(r.recipient, in->recipient_address, 20);
    // only the first four bytes of the secret enter the statement (record_secret), so a secret cut at the
    // record's 32 bytes, or zero-filled up to them, gives the same constants
    memcpy(r.secret, in->secret, std::min<size_t>(in->secret_len, sizeof r.secret));
    r.network_id = in->network_id;
    r.target_chain_id = in->target_chain_id;
    r.commitment_version = in->commitment_version;
    return marshal_record(r, a, err);
}

}  // namespace xfg
