// Host worker pool of the drop-in's host side: the CRC of a large payload (bu_container.hpp), the slices of an ETC1S file
// (bu_basis.hpp: decode_slices) and the streamed front door (bu_etc1s_stream.hpp) spread their serial items over it.
#pragma once
#include <unistd.h>

#include <condition_variable>
#include <functional>
#if defined(__linux__)
#include <sched.h>
#endif
#include <mutex>
#include <thread>
#include <vector>

namespace bu_host {

// ---- host worker pool --------------------------------------------------------------------------------------------
// The reference is single-threaded; the host work that stays serial per item here (one slice's symbol stream, one piece
// of a CRC) is spread over items.  Threads are created once (thread start costs ~50 us, as much as half a small slice)
// and parked on a condition variable.  A forked child finds no threads and runs inline.
class Pool {
    std::mutex run_m, m;
    std::condition_variable cv, cv_done;
    std::vector<std::thread> th;
    const std::function<void()>* job = nullptr;
    unsigned epoch = 0, want = 0, started = 0, running = 0, active_helpers = 0;
    bool stop = false;
    int owner_pid = 0;

    void worker()
    {
        unsigned seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv.wait(lk, [&] { return stop || (epoch != seen && started < want); });
            if (stop) return;
            seen = epoch;
            started++;
            running++;
            const std::function<void()>* f = job;
            lk.unlock();
            (*f)();
            lk.lock();
            if (--running == 0) cv_done.notify_all();
        }
    }

public:
    // helper threads worth starting: the CPUs this process may actually run on (its affinity mask -- a container pinned to a few
    // cores reports the machine's count through hardware_concurrency(), and helpers that only spin on each other's progress then compete
    // with the one thread that makes it), at most 32
    static unsigned capacity()
    {
        unsigned hw = std::thread::hardware_concurrency();
#if defined(__linux__)
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) {
            const int n = CPU_COUNT(&set);
            if (n > 0 && (hw == 0 || (unsigned)n < hw)) hw = (unsigned)n;
        }
#endif
        if (hw == 0) hw = 1;
        return hw < 32u ? hw : 32u;
    }
    // runs f on the calling thread and on up to `helpers` pool threads at once; returns when every copy has returned
    void run(unsigned helpers, const std::function<void()>& f)
    {
        begin(helpers, f);
        try {
            f();
        } catch (...) {
            end();
            throw;
        }
        end();
    }
    // the two halves of run() for a caller that has something else to do meanwhile (bu_read_to feeds the GPU while pool threads
    // decode): begin() starts up to `helpers` copies of f on pool threads and returns how many it started (0: no thread could
    // be had -- the caller must run f itself); end() waits for them.  The pool is reserved from begin() to end() -- ONE job at a time
    // per process: a begin() on another thread WAITS here until the current job's end() (concurrent whole-file calls on different
    // contexts therefore take turns on the host side of their work).  f must stay alive until end() returns.
    unsigned begin(unsigned helpers, const std::function<void()>& f)
    {
        run_m.lock();
        const int pid = (int)getpid();
        if (owner_pid != pid) {  // first use, or a forked child (threads do not survive fork: forget them)
            for (std::thread& t : th) t.detach();
            th.clear();
            owner_pid = pid;
        }
        if (helpers > capacity()) helpers = capacity();
        try {
            while (th.size() < helpers) th.emplace_back([this] { worker(); });
        } catch (...) {  // no more threads to be had (std::system_error): run with the helpers that exist -- every job
            helpers = (unsigned)th.size();  // pulls its items from a shared counter, so fewer copies only means less overlap
        }
        active_helpers = helpers;
        if (helpers) {
            std::lock_guard<std::mutex> lk(m);
            job = &f;
            want = helpers;
            started = 0;
            running = 0;  // counts copies that have actually started (worker()): end() waits for those, not for wake-ups that never came
            epoch++;
            // One wake-up per helper wanted (a pool that once ran 32 copies has 32 parked threads: waking them all for a 3-thread job
            // queues 29 of them on the mutex in front of the three that have work) -- issued UNDER the mutex: a woken thread cannot
            // run, finish and park again while the loop is still notifying, so every notification reaches a different parked thread.
            // (Notified outside the lock, a copy that finished at once re-entered the wait queue and swallowed the next
            // notification: the job then waited for a copy that was never going to start.)
            for (unsigned i = 0; i < helpers; i++) cv.notify_one();
        }
        return helpers;
    }
    void end()
    {
        if (active_helpers) {
            std::unique_lock<std::mutex> lk(m);
            want = 0;  // admissions are closed: a helper that has not started by now sits this job out (the items come from a shared counter)
            cv_done.wait(lk, [&] { return running == 0; });
            job = nullptr;
        }
        active_helpers = 0;
        run_m.unlock();
    }
    ~Pool()
    {
        if (owner_pid != (int)getpid()) {
            for (std::thread& t : th) t.detach();
            return;
        }
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        for (std::thread& t : th) t.join();
    }
};
inline Pool& pool()
{
    static Pool p;
    return p;
}

}  // namespace bu_host
