// The lane scheduler, free of HIP and of the prover context: a FIFO of work units [b0, b1) of
// submitted batches, pulled by one worker thread per lane (prover.hip runs prove_lane as the work
// function; tests/sanitize/unit_queue.cpp drives it with a dummy batch under ASan and TSan).
// The batch type needs an `int units_left` and a `std::exception_ptr err`; both belong to the queue
// from submit to wait and are touched under its lock only.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace xfg {

struct Unit {
    int b0, b1;
    int lane;  // -1: any worker
};

template <class Batch>
class UnitQueue {
    struct Item {
        Batch* b;
        int b0, b1, lane;
    };
    mutable std::mutex m_;
    std::condition_variable qcv_, dcv_;  // a unit was queued (or stop); a batch's last unit finished
    std::deque<Item> q_;
    std::map<uint64_t, std::unique_ptr<Batch>> pending_;
    uint64_t next_ticket_ = 1;
    bool stop_ = false;
    bool whole_units_ = false;
    int last_lane_ = 0;
    int idle_ = 0;  // workers waiting for a unit

   public:
    // the batch's units go to the back of the queue; the ticket (never 0) is what wait() takes
    uint64_t submit(std::unique_ptr<Batch> bp, const std::vector<Unit>& units) {
        Batch* b = bp.get();
        std::lock_guard<std::mutex> g(m_);
        const uint64_t t = next_ticket_++;
        b->units_left = (int)units.size();
        pending_[t] = std::move(bp);
        for (const Unit& u : units) q_.push_back(Item{b, u.b0, u.b1, u.lane});
        qcv_.notify_all();
        return t;
    }
    // blocks until every unit of the batch has finished, then hands the batch back; null for an
    // unknown ticket or one already waited for
    std::unique_ptr<Batch> wait(uint64_t t) {
        std::unique_lock<std::mutex> g(m_);
        auto it = pending_.find(t);
        if (it == pending_.end()) return nullptr;
        Batch* b = it->second.get();
        dcv_.wait(g, [&] { return b->units_left == 0; });
        std::unique_ptr<Batch> bp = std::move(it->second);
        pending_.erase(it);
        return bp;
    }
    // blocks until no submitted unit is queued or running
    void drain() {
        std::unique_lock<std::mutex> g(m_);
        dcv_.wait(g, [&] {
            for (auto& kv : pending_)
                if (kv.second->units_left) return false;
            return true;
        });
    }
    // true while a submitted batch has not been waited for
    bool busy() const {
        std::lock_guard<std::mutex> g(m_);
        return !pending_.empty();
    }
    // wakes every worker and ends its loop (queued units are dropped: drain first)
    void stop() {
        std::lock_guard<std::mutex> g(m_);
        stop_ = true;
        qcv_.notify_all();
    }
    // the lane that finished a unit last
    int last_lane() const {
        std::lock_guard<std::mutex> g(m_);
        return last_lane_;
    }
    int idle() const {
        std::lock_guard<std::mutex> g(m_);
        return idle_;
    }
    // whole units: no unit is halved (timing mode, where the stage times describe one launch set)
    void set_whole_units(bool on) {
        std::lock_guard<std::mutex> g(m_);
        whole_units_ = on;
    }
    bool whole_units() const {
        std::lock_guard<std::mutex> g(m_);
        return whole_units_;
    }

    // the loop of lane l's worker, until stop(): takes the first queued unit that is unpinned or pinned
    // to l and calls work(batch, b0, b1, whole) outside the lock, whole being the whole-units switch as
    // it stood at the pick. A batch keeps the first exception its work threw; its units not yet started
    // are then dropped without a call. split_min: smallest piece a unit is halved into (0: never)
    template <class Work>
    void run(int l, int split_min, Work work) {
        for (;;) {
            Item u;
            bool skip, whole;
            {
                std::unique_lock<std::mutex> g(m_);
                typename std::deque<Item>::iterator it;
                auto pick = [&] {
                    for (it = q_.begin(); it != q_.end(); ++it)
                        if (it->lane < 0 || it->lane == l) return true;
                    return false;
                };
                idle_++;
                qcv_.wait(g, [&] { return stop_ || pick(); });
                idle_--;
                if (stop_) return;
                u = *it;
                q_.erase(it);
                skip = (bool)u.b->err;  // a failed batch drops its remaining units
                whole = whole_units_;
                // fewer queued units than idle lanes (the end of a run of batches, or a lone batch):
                // halve this unit until every idle lane has a share, the halves at the queue's front
                if (u.lane < 0 && !whole && !skip && split_min > 0) {
                    int avail = 0;
                    for (auto& x : q_) avail += x.lane < 0;
                    bool pushed = false;
                    while (u.b1 - u.b0 >= 2 * split_min && avail < idle_) {
                        const int mid = u.b0 + (u.b1 - u.b0) / 2;
                        q_.push_front(Item{u.b, mid, u.b1, -1});
                        u.b->units_left++;
                        u.b1 = mid;
                        avail++;
                        pushed = true;
                    }
                    if (pushed) qcv_.notify_all();
                }
            }
            std::exception_ptr e;
            if (!skip) {
                try {
                    work(u.b, u.b0, u.b1, whole);
                } catch (...) {
                    e = std::current_exception();
                }
            }
            std::lock_guard<std::mutex> g(m_);
            if (e && !u.b->err) u.b->err = e;
            last_lane_ = l;
            if (--u.b->units_left == 0) dcv_.notify_all();
        }
    }
};

}  // namespace xfg
