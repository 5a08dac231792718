// The record kernel: a unit's packed burn records (burn_record.hpp) -> its AIR constants, transcript seeds and
// validation statuses, at the head of the unit's chain in place of the two uploads of host-marshalled inputs. Per
// record: validation, the 12 public inputs, the four Keccak-256 hashes of the statement, BLAKE3 of Context ||
// public inputs. And the Keccak-256 alone on caller-supplied messages (xfg_debug_keccak256).
//
// Keccak-f[1600] with the state spread over lanes. One wave per record; each half of the wave (32 lanes) holds one
// state: lane x + 5 y of the half holds A[x][y] as two 32-bit halves (lanes 25..31 idle; they shadow lane 0 and are
// never read). Every step of a round that mixes lanes is a ds_bpermute_b32 (no LDS is allocated: the instruction
// only uses the crossbar): theta's column parity (4 pulls per half-word, all from the same register, so their
// latencies overlap), D[x] from the parities of columns x - 1 and x + 1, rho and pi as one pull from the source
// lane followed by the source's rotation (a per-lane rotate right by (64 - r) mod 64: a conditional swap of the
// halves and two v_alignbit_b32), chi from the two row neighbours. 18 pulls in 4 dependent stages per round. DPP
// does not fit: its row operations act on rows of 16 lanes and a state row is 5. One lane per record would put 4 x
// 24 rounds of ~300 VALU instructions on one lane at the head of every unit's chain.
// The nullifier's hash is independent of the others and runs in the wave's second half beside the recipient hash;
// the recipient-full hash and the commitment follow in the first half: three permutations deep.
#include "dev_coin.hpp"
#include "hip_util.hpp"

namespace xfg {

static __constant__ const uint32_t KECCAK_RC[24][2] = {  // round constants, (low, high)
    {0x00000001u, 0x00000000u}, {0x00008082u, 0x00000000u}, {0x0000808au, 0x80000000u}, {0x80008000u, 0x80000000u},
    {0x0000808bu, 0x00000000u}, {0x80000001u, 0x00000000u}, {0x80008081u, 0x80000000u}, {0x00008009u, 0x80000000u},
    {0x0000008au, 0x00000000u}, {0x00000088u, 0x00000000u}, {0x80008009u, 0x00000000u}, {0x8000000au, 0x00000000u},
    {0x8000808bu, 0x00000000u}, {0x0000008bu, 0x80000000u}, {0x00008089u, 0x80000000u}, {0x00008003u, 0x80000000u},
    {0x00008002u, 0x80000000u}, {0x00000080u, 0x80000000u}, {0x0000800au, 0x00000000u}, {0x8000000au, 0x80000000u},
    {0x80008081u, 0x80000000u}, {0x00008080u, 0x80000000u}, {0x80000001u, 0x00000000u}, {0x80008008u, 0x80000000u}};
// rho's rotation of lane x + 5 y
static __constant__ const unsigned char KECCAK_RHO[25] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43,
                                                          25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};

// where a lane pulls from in each step (byte addresses of ds_bpermute: lane * 4), and its rotation
struct KeccakLane {
    int par[4];    // the other four lanes of its column
    int cm1, cp1;  // a lane of column x - 1, of column x + 1 (its own row's)
    int rp;        // the lane whose rotated value pi moves here: A[(x + 3y) % 5][x]
    int x2;        // its row's lane of column x + 2 (cp1 is the one of column x + 1)
    unsigned t;    // that source's rotation as a rotate right by 32 swap + t, t < 32
    bool swap, first;
};
__device__ __forceinline__ KeccakLane keccak_lane() {
    const int lane = threadIdx.x & 63, base = lane & 32, i = lane & 31, ii = i < 25 ? i : 0;
    const int x = ii % 5, y = ii / 5, row = base + 5 * y;
    KeccakLane L;
#pragma unroll
    for (int k = 0; k < 4; k++) L.par[k] = (base + (ii + 5 * (k + 1)) % 25) << 2;
    L.cm1 = (row + (x + 4) % 5) << 2;
    L.cp1 = (row + (x + 1) % 5) << 2;
    L.x2 = (row + (x + 2) % 5) << 2;
    const int src = (x + 3 * y) % 5 + 5 * x;
    L.rp = (base + src) << 2;
    const unsigned t = (64u - KECCAK_RHO[src]) & 63u;
    L.swap = t >= 32;
    L.t = t & 31;
    L.first = ii == 0;
    return L;
}
__device__ __forceinline__ uint32_t pull(int addr, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v);
}
// ((a : b) >> s) & 0xFFFFFFFF, s < 32: v_alignbit_b32
__device__ __forceinline__ uint32_t alignbit(uint32_t a, uint32_t b, unsigned s) {
    return __builtin_amdgcn_alignbit(a, b, s);
}
// the permutation on both halves of the wave at once; every lane of the wave must be active
__device__ void keccak_f_lanes(const KeccakLane& L, uint32_t& lo, uint32_t& hi) {
#pragma unroll 1
    for (int r = 0; r < 24; r++) {
        // theta: the parity of the lane's column, then D[x] = C[x - 1] ^ rol(C[x + 1], 1)
        uint32_t cl = lo, ch = hi;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cl ^= pull(L.par[k], lo);
            ch ^= pull(L.par[k], hi);
        }
        const uint32_t ml = pull(L.cm1, cl), mh = pull(L.cm1, ch), pl = pull(L.cp1, cl), ph = pull(L.cp1, ch);
        lo ^= ml ^ alignbit(pl, ph, 31);
        hi ^= mh ^ alignbit(ph, pl, 31);
        // rho and pi: the source lane's value, rotated left by the source's offset
        const uint32_t sl = pull(L.rp, lo), sh = pull(L.rp, hi);
        const uint32_t a = L.swap ? sh : sl, b = L.swap ? sl : sh;
        const uint32_t bl = alignbit(b, a, L.t), bh = alignbit(a, b, L.t);
        // chi along the row, iota on lane 0
        const uint32_t n1l = pull(L.cp1, bl), n1h = pull(L.cp1, bh), n2l = pull(L.x2, bl), n2h = pull(L.x2, bh);
        lo = bl ^ (~n1l & n2l);
        hi = bh ^ (~n1h & n2h);
        if (L.first) {
            lo ^= KECCAK_RC[r][0];
            hi ^= KECCAK_RC[r][1];
        }
    }
}
// one single-block Keccak-256 per half of the wave: w = the lane's LE word of the padded block (lanes 0..16 of the
// half; anything elsewhere, the capacity is zero). Afterwards lanes 0..3 of the half hold the digest's four words
__device__ __forceinline__ void keccak256_lanes(const KeccakLane& L, u64 w, uint32_t& lo, uint32_t& hi) {
    const bool rate = (threadIdx.x & 31) < KECCAK_RATE / 8;
    lo = rate ? (uint32_t)w : 0u;
    hi = rate ? (uint32_t)(w >> 32) : 0u;
    keccak_f_lanes(L, lo, hi);
}
template <int WHICH>
__device__ __forceinline__ u64 padded_msg_word(unsigned i, const BurnMsgSrc& s) {
    return burn_msg_word(WHICH, i, s) ^ keccak_pad_word(i, burn_msg_len(WHICH));
}

// one wave per record
__global__ __launch_bounds__(64) void burn_marshal_kernel(const xfg_burn_record* records, CoinContext ctx,
                                                          AirConst* air_out, DevCoin* coin_out, int* status_out) {
    const xfg_burn_record& rec = records[blockIdx.x];
    const unsigned lane = threadIdx.x, i = lane & 31;
    const bool second = lane >= 32, rate = i < KECCAK_RATE / 8;
    const KeccakLane L = keccak_lane();
    const int status = record_status(rec);
    BurnMsgSrc s;
    s.recipient = rec.recipient;
    s.secret = record_secret(rec);
    record_public_inputs(rec, s.pub);
#pragma unroll
    for (int k = 0; k < 4; k++) s.rf[k] = 0;
    uint32_t lo, hi;
    // the recipient hash in the first half of the wave, the nullifier in the second
    u64 w = 0;
    if (rate) w = second ? padded_msg_word<MSG_NULLIFIER>(i, s) : padded_msg_word<MSG_RECIPIENT>(i, s);
    keccak256_lanes(L, w, lo, hi);
    s.pub[3] = (uint32_t)__shfl((int)lo, 0, 64);
    const u64 nullifier = (uint32_t)__shfl((int)lo, 32, 64);
    // the 32-byte recipient hash (the second half runs an empty block from here on; its result is not read)
    w = rate && !second ? padded_msg_word<MSG_RECIPIENT_FULL>(i, s) : 0;
    keccak256_lanes(L, w, lo, hi);
#pragma unroll
    for (int k = 0; k < 4; k++) s.rf[k] = (u64)(uint32_t)__shfl((int)lo, k, 64) | ((u64)(uint32_t)__shfl((int)hi, k, 64) << 32);
    // the commitment
    w = rate && !second ? padded_msg_word<MSG_COMMITMENT>(i, s) : 0;
    keccak256_lanes(L, w, lo, hi);
    const u64 commitment = (uint32_t)__shfl((int)lo, 0, 64);
    // the transcript seed: Context::to_elements || public inputs (ProverChannel::new), the whole wave on it
    u64 e[20];
#pragma unroll
    for (int k = 0; k < 8; k++) e[k] = ctx.e[k];
#pragma unroll
    for (int k = 0; k < 12; k++) e[8 + k] = s.pub[k];
    DevCoin coin;
    coin.seed = dev_hash_elems(e, 20);
    coin.counter = 0;  // as Coin::init leaves it
    coin.pad = 0;
    if (lane == 0) {
        AirConst a;
#pragma unroll
        for (int k = 0; k < 12; k++) a.pub[k] = s.pub[k];
        a.nullifier = nullifier;
        a.commitment = commitment;
        a.pad[0] = a.pad[1] = 0;
        air_out[blockIdx.x] = a;
        coin_out[blockIdx.x] = coin;
        status_out[blockIdx.x] = status;
    }
}
void launch_burn_marshal(const xfg_burn_record* records, int B, const CoinContext& ctx, AirConst* air_out,
                         DevCoin* coin_out, int* status_out, hipStream_t s) {
    if (B <= 0) return;
    XFG_LAUNCH(burn_marshal_kernel, dim3((unsigned)B), dim3(64), 0, s, records, ctx, air_out, coin_out, status_out);
}

// two messages per wave, one in each half
__global__ __launch_bounds__(64) void keccak256_kernel(const uint8_t* msgs, const u32* lens, int count, uint8_t* out) {
    const unsigned lane = threadIdx.x, i = lane & 31;
    const int m = 2 * (int)blockIdx.x + (int)(lane >> 5);
    const bool live = m < count;
    const KeccakLane L = keccak_lane();
    u64 w = 0;
    if (live && i < KECCAK_RATE / 8) {
        const unsigned len = lens[m];
        const uint8_t* p = msgs + (size_t)m * KECCAK_RATE + 8 * i;
#pragma unroll
        for (unsigned j = 0; j < 8; j++)
            if (8 * i + j < len) w |= (u64)p[j] << (8 * j);
        w ^= keccak_pad_word(i, len);
    }
    uint32_t lo, hi;
    keccak256_lanes(L, w, lo, hi);
    if (live && i < 4) ((u64*)(out + (size_t)m * 32))[i] = (u64)lo | ((u64)hi << 32);
}
void launch_keccak256(const uint8_t* msgs, const u32* lens, int count, uint8_t* out, hipStream_t s) {
    if (count <= 0) return;
    XFG_LAUNCH(keccak256_kernel, dim3((unsigned)(count + 1) / 2), dim3(64), 0, s, msgs, lens, count, out);
}

}  // namespace xfg
