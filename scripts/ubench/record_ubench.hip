// Microbenchmark: what stands at the head of a unit's chain for 32 statements.
//
// (1) the record kernel (xfg-stark_amd/csrc/burn_record.hip, compiled into this program as it is) on 32 packed
//     records resident in device memory: HIP events around `reps` back-to-back launches on an otherwise idle stream
//     after 20 warm ones, best and median of 5 windows, microseconds per launch. Its outputs are compared with the
//     host marshalling first.
// (2) marshal() (xfg-stark_amd/csrc/marshal.hpp: validation, the statement as a record, four Keccak-256) of the same 32 statements
//     on the host pool, as xfg_prove_batch_submit runs it on the submitting thread: a host clock around each of 200
//     parallel_for calls after 20 warm ones, best and median, microseconds per call.
//
// build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -pthread -o record_ubench record_ubench.hip
// usage: record_ubench [records per launch, default 32] [launches per window, default 200]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xfg-stark_amd/csrc/burn_record.hip"
#include "../../xfg-stark_amd/csrc/host_pool.hpp"
#include "../../xfg-stark_amd/csrc/marshal.hpp"

using namespace xfg;

int main(int argc, char** argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 32, reps = argc > 2 ? atoi(argv[2]) : 200;
    if (B < 1 || B > 65535 || reps < 1) return 2;
    std::vector<xfg_burn_record> recs(B);
    uint64_t x = 88172645463325252ULL;
    for (auto& r : recs) {
        uint8_t* b = (uint8_t*)&r;
        for (size_t i = 0; i < sizeof r; i++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            b[i] = (uint8_t)x;
        }
        r.burn_amount = r.mint_amount = REC_STANDARD_BURN;
        r.tx_prefix_hash[0] |= 1;
        memset(r.reserved, 0, sizeof r.reserved);
    }
    xfg_burn_record* d_rec = nullptr;
    AirConst* d_air = nullptr;
    DevCoin* d_coin = nullptr;
    int* d_st = nullptr;
    HIPCHK(hipMalloc((void**)&d_rec, B * sizeof(xfg_burn_record)));
    HIPCHK(hipMalloc((void**)&d_air, B * sizeof(AirConst)));
    HIPCHK(hipMalloc((void**)&d_coin, B * sizeof(DevCoin)));
    HIPCHK(hipMalloc((void**)&d_st, B * sizeof(int)));
    HIPCHK(hipMemcpy(d_rec, recs.data(), B * sizeof(xfg_burn_record), hipMemcpyHostToDevice));
    hipStream_t s;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    CoinContext cx;
    const Opts o{42, 8, 4, 1, 8, 31};
    context_elements(1 << 16, o, cx.e);

    // the kernel's outputs against the host's
    launch_burn_marshal(d_rec, B, cx, d_air, d_coin, d_st, s);
    HIPCHK(hipStreamSynchronize(s));
    std::vector<AirConst> airs(B);
    std::vector<DevCoin> coins(B);
    std::vector<int> sts(B);
    HIPCHK(hipMemcpy(airs.data(), d_air, B * sizeof(AirConst), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(coins.data(), d_coin, B * sizeof(DevCoin), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sts.data(), d_st, B * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; b++) {
        AirConst want;
        std::string err;
        const xfg_burn_inputs in = record_to_inputs(recs[b]);
        u64 e[20];
        Coin c;
        if (marshal(&in, want, err) != XFG_OK || sts[b] != XFG_OK || memcmp(&want, &airs[b], sizeof want)) {
            fprintf(stderr, "record %d: the kernel's constants differ from marshal()'s\n", b);
            return 1;
        }
        memcpy(e, cx.e, sizeof cx.e);
        memcpy(e + 8, want.pub, 12 * 8);
        c.init(e, 20);
        if (memcmp(&c.seed, &coins[b].seed, sizeof c.seed) || coins[b].counter != 0) {
            fprintf(stderr, "record %d: the kernel's transcript seed differs from Coin::init's\n", b);
            return 1;
        }
    }

    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int i = 0; i < 20; i++) launch_burn_marshal(d_rec, B, cx, d_air, d_coin, d_st, s);
    HIPCHK(hipStreamSynchronize(s));
    std::vector<double> win;
    for (int w = 0; w < 5; w++) {
        HIPCHK(hipEventRecord(e0, s));
        for (int i = 0; i < reps; i++) launch_burn_marshal(d_rec, B, cx, d_air, d_coin, d_st, s);
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        win.push_back(1e3 * ms / reps);
    }
    std::sort(win.begin(), win.end());
    printf("record kernel, %d records, %d back-to-back launches per window: best %.2f us, median %.2f us per launch\n", B,
           reps, win[0], win[2]);
    // one launch alone (launch latency included): events around a single launch, the stream idle before it
    std::vector<double> one;
    for (int i = 0; i < 50; i++) {
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipEventRecord(e0, s));
        launch_burn_marshal(d_rec, B, cx, d_air, d_coin, d_st, s);
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        one.push_back(1e3 * ms);
    }
    std::sort(one.begin(), one.end());
    printf("record kernel, %d records, one launch between two events on an idle stream: best %.2f us, median %.2f us\n", B,
           one[0], one[25]);

    // marshal() on the host pool
    std::vector<xfg_burn_inputs> ins;
    for (auto& r : recs) ins.push_back(record_to_inputs(r));
    std::vector<AirConst> out(B);
    std::vector<std::string> errs(B);
    std::vector<double> host;
    for (int i = 0; i < 220; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        host_pool().parallel_for(B, [&](int k) { marshal(&ins[k], out[k], errs[k]); });
        const auto t1 = std::chrono::steady_clock::now();
        if (i >= 20) host.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    std::sort(host.begin(), host.end());
    printf("marshal() of %d inputs on the host pool: best %.2f us, median %.2f us per call\n", B, host[0],
           host[host.size() / 2]);
    return 0;
}
