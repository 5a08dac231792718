// Stand-alone driver of the project's two hand-written concurrency primitives, the lane scheduler
// (xfg-stark_amd/csrc/unit_queue.hpp) and the host thread pool (xfg-stark_amd/csrc/host_pool.hpp): plain C++,
// no HIP. Built twice by xfg-stark_amd/Makefile, build/asan/unit_queue (ASan + UBSan) and build/tsan/unit_queue
// (TSan), and run by tests/test_unit_queue.py. A dummy batch and a work function that records
// (batch, lane, b0, b1), blocks on a gate or throws where a scenario says so, check
//   1. exactly-once coverage: the pieces of every batch partition [0, B), wait() returns it with units_left 0;
//   2. one worker never splits: its pieces are the submitted units in FIFO order;
//   3. held workers do not split what is submitted meanwhile;
//   4. idle workers halve a unit within bounds (sizes 32 / 2^k, none below split_min; one piece with
//      split_min 0 or the whole-units switch);
//   5. pinned units run on their lane only, unsplit, and do not block an unpinned unit behind them;
//   6. a throwing work function: the batch's later units are dropped, wait() carries the first exception,
//      the batches around it complete;
//   7. tickets (0, unknown, waited twice), busy(), drain(), stop() and waits in reverse order;
//   8. HostPool::parallel_for from 7 threads at once: every index once per call, an exception rethrown to its
//      caller only after that call's other indices ran, the pool usable afterwards.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <thread>

#include "../../xfg-stark_amd/csrc/host_pool.hpp"
#include "../../xfg-stark_amd/csrc/unit_queue.hpp"

using namespace xfg;

static std::atomic<int> failures{0};
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

// polls a condition another thread makes true; a scenario that never gets there fails instead of hanging
template <class F>
static bool eventually(F f) {
    const auto end = std::chrono::steady_clock::now() + std::chrono::seconds(30);
    while (!f()) {
        if (std::chrono::steady_clock::now() > end) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    return true;
}

struct DummyBatch {
    int B = 0;
    bool gated = false;  // every unit waits for a token of the rig's gate
    int throw_from = -1;  // units with b0 >= throw_from throw (-1: none)
    std::atomic<int> done{0};  // jobs whose unit has finished
    int units_left = 0;
    std::exception_ptr err;
};
struct Piece {
    DummyBatch* b;
    int lane, b0, b1;
    bool whole;
};
struct Gate {
    std::mutex m;
    std::condition_variable cv;
    int tokens = 0, held = 0;
    void pass() {
        std::unique_lock<std::mutex> g(m);
        held++;
        cv.wait(g, [&] { return tokens > 0; });
        tokens--;
        held--;
    }
    void release(int k) {
        {
            std::lock_guard<std::mutex> g(m);
            tokens += k;
        }
        cv.notify_all();
    }
    int waiting() {
        std::lock_guard<std::mutex> g(m);
        return held;
    }
};

// a queue with its workers, as xfg_ctx holds them
struct Rig {
    UnitQueue<DummyBatch> q;
    std::vector<std::thread> th;
    std::mutex rm;
    std::vector<Piece> rec;
    std::atomic<int> finished{0};
    Gate gate;

    Rig(int workers, int split_min) {
        for (int l = 0; l < workers; l++)
            th.emplace_back([this, l, split_min] {
                q.run(l, split_min, [this, l](DummyBatch* b, int b0, int b1, bool whole) {
                    {
                        std::lock_guard<std::mutex> g(rm);
                        rec.push_back(Piece{b, l, b0, b1, whole});
                    }
                    if (b->gated) gate.pass();
                    b->done += b1 - b0;
                    finished++;
                    if (b->throw_from >= 0 && b0 >= b->throw_from) throw std::runtime_error("unit " + std::to_string(b0));
                });
            });
    }
    void join() {
        q.drain();
        q.stop();
        for (auto& t : th) t.join();
        th.clear();
    }
    ~Rig() { join(); }
    std::vector<Piece> pieces_of(const DummyBatch* b) {
        std::lock_guard<std::mutex> g(rm);
        std::vector<Piece> out;
        for (auto& p : rec)
            if (p.b == b) out.push_back(p);
        return out;  // in the order they were started
    }
};

static std::unique_ptr<DummyBatch> batch(int B) {
    std::unique_ptr<DummyBatch> b(new DummyBatch());
    b->B = B;
    return b;
}
static std::vector<Unit> units_of(int B, int U, int lane = -1) {
    std::vector<Unit> u;
    for (int b0 = 0; b0 < B; b0 += U) u.push_back(Unit{b0, std::min(B, b0 + U), lane});
    return u;
}
// the pieces tile [0, B) with no gap or overlap
static void check_partition(std::vector<Piece> p, int B, const char* what) {
    std::sort(p.begin(), p.end(), [](const Piece& a, const Piece& b) { return a.b0 < b.b0; });
    int at = 0;
    for (auto& x : p) {
        CHECK(x.b0 == at && x.b1 > x.b0, "%s: piece [%d, %d) at %d of %d", what, x.b0, x.b1, at, B);
        at = x.b1;
    }
    CHECK(at == B, "%s: covered %d of %d", what, at, B);
}

// 1 and 2
static void coverage(int workers, int split_min) {
    static const int Bs[] = {1, 2, 31, 32, 33, 64, 100}, Us[] = {32, 5, 1};
    Rig r(workers, split_min);
    std::vector<uint64_t> tickets;
    std::vector<std::pair<DummyBatch*, std::vector<Unit>>> sub;
    for (int B : Bs)
        for (int U : Us) {
            auto b = batch(B);
            sub.push_back({b.get(), units_of(B, U)});
            tickets.push_back(r.q.submit(std::move(b), sub.back().second));
        }
    std::vector<std::unique_ptr<DummyBatch>> got;
    for (uint64_t t : tickets) got.push_back(r.q.wait(t));
    char what[64];
    std::snprintf(what, sizeof what, "coverage workers=%d split_min=%d", workers, split_min);
    for (size_t k = 0; k < got.size(); k++) {
        CHECK(got[k] && got[k].get() == sub[k].first, "%s: wait returned another batch", what);
        if (!got[k]) continue;
        CHECK(got[k]->units_left == 0 && !got[k]->err && got[k]->done == got[k]->B, "%s: units_left %d", what, got[k]->units_left);
        const std::vector<Piece> p = r.pieces_of(got[k].get());
        check_partition(p, got[k]->B, what);
        for (auto& x : p) CHECK(!x.whole, "%s: whole-units flag set", what);
        if (split_min == 0) CHECK(p.size() == sub[k].second.size(), "%s: split with split_min 0", what);
        for (auto& x : p) {  // a piece is a submitted unit, or a part of one that is no smaller than split_min
            bool whole_unit = false, inside = false;
            for (auto& u : sub[k].second) {
                whole_unit |= x.b0 == u.b0 && x.b1 == u.b1;
                inside |= x.b0 >= u.b0 && x.b1 <= u.b1;
            }
            CHECK(whole_unit || (inside && split_min > 0 && x.b1 - x.b0 >= split_min), "%s: piece [%d, %d)", what, x.b0, x.b1);
        }
    }
    CHECK(r.finished == (int)r.rec.size(), "%s: %d of %zu pieces finished", what, (int)r.finished, r.rec.size());
    if (workers == 1) {  // idle is 0 whenever the only worker picks: the units as submitted, in FIFO order
        size_t at = 0;
        for (auto& s : sub)
            for (auto& u : s.second) {
                CHECK(at < r.rec.size() && r.rec[at].b == s.first && r.rec[at].b0 == u.b0 && r.rec[at].b1 == u.b1 &&
                          r.rec[at].lane == 0,
                      "%s: piece %zu is not the unit submitted", what, at);
                at++;
            }
        CHECK(at == r.rec.size(), "%s: %zu pieces for %zu units", what, r.rec.size(), at);
    }
}

// 3
static void held_workers_do_not_split() {
    Rig r(3, 1);
    auto h = batch(3);
    h->gated = true;
    const uint64_t th = r.q.submit(std::move(h), units_of(3, 1));
    CHECK(eventually([&] { return r.gate.waiting() == 3; }), "held: the workers did not reach the gate");
    auto x = batch(64);
    DummyBatch* xp = x.get();
    const uint64_t tx = r.q.submit(std::move(x), units_of(64, 32));
    r.gate.release(1);  // one worker comes back and finds two units and nobody idle
    auto got = r.q.wait(tx);
    CHECK(r.gate.waiting() == 2, "held: %d workers at the gate", r.gate.waiting());
    const std::vector<Piece> p = r.pieces_of(xp);
    CHECK(p.size() == 2 && p[0].b0 == 0 && p[0].b1 == 32 && p[1].b0 == 32 && p[1].b1 == 64 && p[0].lane == p[1].lane,
          "held: %zu pieces", p.size());
    r.gate.release(2);
    CHECK(r.q.wait(th) != nullptr, "held: gated batch lost");
}

// 4
static void idle_workers_split(int split_min, bool whole, bool expect_split) {
    Rig r(4, split_min);
    r.q.set_whole_units(whole);
    CHECK(r.q.whole_units() == whole, "split: switch not stored");
    CHECK(eventually([&] { return r.q.idle() == 4; }), "split: the workers did not go idle");
    auto b = batch(32);
    DummyBatch* bp = b.get();
    auto got = r.q.wait(r.q.submit(std::move(b), units_of(32, 32)));
    const std::vector<Piece> p = r.pieces_of(bp);
    check_partition(p, 32, "split");
    CHECK(got && got->units_left == 0, "split: units_left");
    if (!expect_split) CHECK(p.size() == 1, "split: %zu pieces with split_min %d whole %d", p.size(), split_min, (int)whole);
    else CHECK(p.size() > 1, "split: one piece with three workers idle");
    for (auto& x : p) {
        const int s = x.b1 - x.b0;
        CHECK(32 % s == 0 && (s & (s - 1)) == 0 && (!expect_split || s >= split_min), "split: piece of %d", s);
        CHECK(x.whole == whole, "split: work saw whole = %d", (int)x.whole);
    }
}

// 5
static void pinned_units() {
    Rig r(3, 1);
    CHECK(eventually([&] { return r.q.idle() == 3; }), "pinned: the workers did not go idle");
    {  // on their lane only, never split (every other worker is idle when the first is picked)
        auto b = batch(32);
        DummyBatch* bp = b.get();
        const std::vector<Unit> u = {{0, 8, 0}, {8, 16, 1}, {16, 24, 2}, {24, 32, 1}};
        r.q.wait(r.q.submit(std::move(b), u));
        const std::vector<Piece> p = r.pieces_of(bp);
        check_partition(p, 32, "pinned");
        CHECK(p.size() == 4, "pinned: %zu pieces", p.size());
        for (auto& x : p) {
            const Unit& w = u[x.b0 / 8];
            CHECK(x.b0 == w.b0 && x.b1 == w.b1 && x.lane == w.lane, "pinned: [%d, %d) on lane %d", x.b0, x.b1, x.lane);
        }
    }
    // lane 0 held busy: the unit pinned to it waits, the unpinned one behind it is taken meanwhile
    auto g = batch(1);
    g->gated = true;
    const uint64_t tg = r.q.submit(std::move(g), {Unit{0, 1, 0}});
    CHECK(eventually([&] { return r.gate.waiting() == 1; }), "pinned: lane 0 did not reach the gate");
    auto b = batch(8);
    DummyBatch* bp = b.get();
    const uint64_t tb = r.q.submit(std::move(b), {Unit{0, 4, 0}, Unit{4, 8, -1}});
    CHECK(eventually([&] { return bp->done == 4; }), "pinned: the unpinned unit was not taken");
    for (auto& x : r.pieces_of(bp)) CHECK(x.lane != 0 && x.b0 >= 4, "pinned: [%d, %d) on lane %d", x.b0, x.b1, x.lane);
    r.gate.release(1);
    CHECK(r.q.wait(tg) != nullptr, "pinned: gated batch lost");
    r.q.wait(tb);
    const std::vector<Piece> p = r.pieces_of(bp);
    check_partition(p, 8, "pinned, behind a busy lane");
    for (auto& x : p)
        if (x.b0 < 4) CHECK(x.b0 == 0 && x.b1 == 4 && x.lane == 0, "pinned: [%d, %d) on lane %d", x.b0, x.b1, x.lane);
}

static std::string message_of(const std::exception_ptr& e) {
    try {
        if (e) std::rethrow_exception(e);
    } catch (const std::exception& x) {
        return x.what();
    }
    return "";
}

// 6
static void throwing_work(int workers) {
    Rig r(workers, 0);
    auto a = batch(10), t = batch(12), c = batch(10);
    DummyBatch *ap = a.get(), *tp = t.get(), *cp = c.get();
    t->throw_from = workers == 1 ? 4 : 0;
    const uint64_t ta = r.q.submit(std::move(a), units_of(10, 5));
    const uint64_t tt = r.q.submit(std::move(t), units_of(12, 2));
    const uint64_t tc = r.q.submit(std::move(c), units_of(10, 5));
    auto gt = r.q.wait(tt);
    CHECK(gt && gt->err && gt->units_left == 0, "throw: no exception carried");
    const std::vector<Piece> p = r.pieces_of(tp);
    if (workers == 1) {  // units 0 and 2 ran, 4 threw, 6 .. 10 were never handed over
        CHECK(p.size() == 3 && p[2].b0 == 4, "throw: %zu units of the failed batch started", p.size());
        CHECK(message_of(gt->err) == "unit 4", "throw: carried '%s'", message_of(gt->err).c_str());
    } else {  // the first unit threw while at most workers - 1 others had started: the rest were dropped
        CHECK(p.size() <= (size_t)workers && message_of(gt->err).rfind("unit ", 0) == 0, "throw: %zu units started", p.size());
    }
    auto ga = r.q.wait(ta), gc = r.q.wait(tc);
    CHECK(ga && !ga->err && ga->done == 10 && gc && !gc->err && gc->done == 10, "throw: a neighbouring batch suffered");
    check_partition(r.pieces_of(ap), 10, "throw, batch before");
    check_partition(r.pieces_of(cp), 10, "throw, batch after");
    // and one more after the failed batch has been collected
    auto d = batch(7);
    DummyBatch* dp = d.get();
    auto gd = r.q.wait(r.q.submit(std::move(d), units_of(7, 3)));
    CHECK(gd && !gd->err, "throw: the queue did not recover");
    check_partition(r.pieces_of(dp), 7, "throw, later batch");
}

// 7
static void tickets_and_shutdown() {
    Rig r(3, 2);
    CHECK(!r.q.busy() && !r.q.wait(0) && !r.q.wait(12345), "tickets: empty queue");
    r.q.drain();  // nothing pending: returns at once
    std::vector<uint64_t> t;
    for (int k = 0; k < 5; k++) {
        t.push_back(r.q.submit(batch(20 + k), units_of(20 + k, 6)));
        CHECK(t.back() != 0 && (k == 0 || t[k] != t[k - 1]), "tickets: %llu", (unsigned long long)t.back());
        CHECK(r.q.busy(), "tickets: not busy after submit");
    }
    r.q.drain();
    {
        std::lock_guard<std::mutex> g(r.rm);
        CHECK(r.finished == (int)r.rec.size() && !r.rec.empty(), "drain returned with %d of %zu pieces finished",
              (int)r.finished, r.rec.size());
    }
    CHECK(r.q.busy(), "tickets: drained batches are still to be waited for");
    const int last = r.q.last_lane();
    CHECK(last >= 0 && last < 3, "tickets: last lane %d", last);
    for (int k = 4; k >= 0; k--) {  // in reverse order of submission
        CHECK(r.q.busy(), "tickets: not busy before the last wait");
        auto b = r.q.wait(t[k]);
        CHECK(b && b->B == 20 + k && b->units_left == 0, "tickets: batch %d", k);
        CHECK(!r.q.wait(t[k]), "tickets: waited twice");
    }
    CHECK(!r.q.busy() && !r.q.wait(t[4] + 1), "tickets: busy after the last wait");
    CHECK(eventually([&] { return r.q.idle() == 3; }), "tickets: the workers did not go idle");
    r.join();  // stop() with every worker idle: all threads end
}

// 8
static void pool_from_seven_threads(int threads) {
    static const int counts[] = {0, 1, 2, 33, 64};
    HostPool pool(threads);
    std::vector<std::thread> callers;
    for (int k = 0; k < 7; k++)
        callers.emplace_back([&pool, k, threads] {
            for (int round = 0; round < 20; round++)
                for (int count : counts) {
                    std::vector<std::atomic<int>> seen(count);
                    const bool thrower = k == 3 && count == 33;
                    std::string caught;
                    try {
                        pool.parallel_for(count, [&](int i) {
                            seen[i]++;
                            if (thrower && i == 7) throw std::runtime_error("index 7");
                        });
                    } catch (const std::exception& e) {
                        caught = e.what();
                    }
                    CHECK(caught == (thrower ? "index 7" : ""), "pool of %d: caller %d caught '%s'", threads, k, caught.c_str());
                    for (int i = 0; i < count; i++)
                        CHECK(seen[i] == 1, "pool of %d: caller %d index %d of %d seen %d times", threads, k, i, count,
                              (int)seen[i]);
                }
        });
    for (auto& t : callers) t.join();
    std::atomic<int> sum{0};
    pool.parallel_for(64, [&](int i) { sum += i; });
    CHECK(sum == 64 * 63 / 2, "pool of %d: unusable afterwards", threads);
}

int main() {
    for (int workers : {1, 2, 7})
        for (int split_min : {0, 1, 2, 16}) coverage(workers, split_min);
    held_workers_do_not_split();
    idle_workers_split(4, false, true);
    idle_workers_split(0, false, false);
    idle_workers_split(4, true, false);
    pinned_units();
    throwing_work(1);
    throwing_work(3);
    tickets_and_shutdown();
    for (int threads : {0, 1, 8}) pool_from_seven_threads(threads);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", (int)failures);
        return 1;
    }
    std::printf("unit_queue ok\n");
    return 0;
}
