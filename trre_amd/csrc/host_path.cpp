// host_path.cpp — scans of host buffers: chunks staged through pinned memory with several in flight on one device, the input
// line-sharded over several devices, and their entry points of the C ABI (include/trre_mi355x.h).  They reach the scan core
// (runtime.cpp) through the names that runtime_state.hpp declares.
#include <cstdio>
#include <chrono>
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <thread>

#include "runtime_state.hpp"
#include "switches.hpp"

using namespace trre_host;

// grow one direction of a host slot (pinned staging + device buffer); need_pin false: the caller's own buffer is pinned, no staging on this side
int trre_host::slot_reserve(DeviceState::HostSlot& hs, bool input, size_t bytes, bool need_pin) {
    uint8_t*& pin = input ? hs.pin_in : hs.pin_out;
    uint8_t*& dev = input ? hs.d_in : hs.d_out;
    size_t& have = input ? hs.in_cap : hs.out_cap;
    if (have >= bytes && (pin || !need_pin)) return TRRE_OK;
    const bool grow = have < bytes;
    const size_t want = grow ? bytes + bytes / 8 : have;  // (head room: the next chunk is rarely the same size)
    if (grow) {
        if (dev) (void)hipFree(dev);
        pinned_put(pin);
        pin = nullptr; dev = nullptr; have = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dev), want + 64));
    }
    if (need_pin && !pin) HIP_TRY(pinned_get(&pin, want + 64));
    have = want;
    return TRRE_OK;
}

namespace {
constexpr size_t kHostChunk = (size_t)32 << 20;

// Staging copies between the caller's pageable buffers and pinned memory are spread over a few threads:
// one thread moves ~10 GB/s, a PCIe 5 x16 link ~55 GB/s each way.
class CopyPool {
public:
    static CopyPool& get() { static CopyPool pool; return pool; }
    struct Job { int left = 0; };
    // copies n bytes with up to `ways` workers; returns when done
    void copy(void* dst, const void* src, size_t n, int ways) {
        if (n < ((size_t)4 << 20) || ways <= 1) { std::memcpy(dst, src, n); return; }
        Job job;
        start(job, dst, src, n, ways);
        wait(job);
    }
    // the same in two halves: queue the pieces, collect later (the job must stay alive until wait() returns)
    void start(Job& job, void* dst, const void* src, size_t n, int ways) {
        if (n == 0) return;
        const size_t piece = std::max<size_t>((n / (size_t)(ways > 0 ? ways : 1) + 4095) & ~(size_t)4095, (size_t)1 << 20);
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t off = 0; off < n; off += piece) {
            queue_.push_back(Piece{&job, static_cast<uint8_t*>(dst) + off, static_cast<const uint8_t*>(src) + off, std::min(piece, n - off)});
            ++job.left;
        }
        cv_.notify_all();
    }
    void wait(Job& job) {
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return job.left == 0; });
    }

private:
    struct Piece { Job* job; uint8_t* dst; const uint8_t* src; size_t n; };
    CopyPool() {
        // (a copy asks for kCopyWays = 8 workers; trre_scan_host_multi runs one staging copy in and one out per device at a time: on a host with
        // the cores for it the pool holds 8 x 8 workers, so that eight devices do not queue behind two devices' worth of them)
        unsigned hw = std::thread::hardware_concurrency();
        const unsigned n = hw >= 256 ? 64 : (hw >= 128 ? 32 : (hw >= 32 ? 16 : (hw >= 8 ? hw / 2 : 2)));
        for (unsigned i = 0; i < n; ++i) workers_.emplace_back([this] { run(); });
    }
    ~CopyPool() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto& w : workers_) w.join();
    }
    void run() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || !queue_.empty(); });
            if (stop_) return;
            Piece pc = queue_.back();
            queue_.pop_back();
            lk.unlock();
            std::memcpy(pc.dst, pc.src, pc.n);
            lk.lock();
            if (--pc.job->left == 0) done_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::vector<Piece> queue_;
    std::vector<std::thread> workers_;
    bool stop_ = false;
};
constexpr int kCopyWays = 8;         // (4 and 16 measured the same through the command line, round 5)

// Host buffers on one device.  The input goes through in chunks cut at line ends (lines are independent, so
// the chunks' outputs simply concatenate), kHostSlots chunks in flight, each on its slot's stream: while one
// chunk is scanned the next is staged into pinned memory and copied up, and the previous one's output comes
// down and is copied out.  `out` may be null when cap == 0 (size query).
int scan_host_on(trre_prog* p, DeviceState* st, const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len) {
    for (auto& hs : st->slot) {
        if (!hs.stream) HIP_TRY(hipStreamCreateWithFlags(&hs.stream, hipStreamNonBlocking));
        int rc = ctx_init(hs.ctx);
        if (rc) return rc;
    }
    const int fam = scan_family(*p);
    const bool fixed_len = !is_gen(fam);              // output size == input size (unless a NUL forces a general family)
    // A caller's buffer that is pinned already (hipHostMalloc / hipHostRegister) goes over the link as it
    // is: no staging copy on that side (round 5; the copies run at 116 GB/s on 8 threads of one pool, which eight devices share).
    auto is_pinned = [](const void* ptr, size_t len) -> bool {
        if (!ptr || !len) return false;
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (at.type != hipMemoryTypeHost) return false;
        if (hipPointerGetAttributes(&at, static_cast<const uint8_t*>(ptr) + len - 1) != hipSuccess) { (void)hipGetLastError(); return false; }
        return at.type == hipMemoryTypeHost;
    };
    const bool no_direct = trre::switches().no_pinned_direct;
    const bool in_direct = !no_direct && is_pinned(in, n), out_direct = !no_direct && cap && is_pinned(out, cap);

    struct Chunk { size_t off = 0, len = 0, out_at = 0, m = 0, early_at = 0; bool submitted = false, copying = false, leaving = false, early = false; CopyPool::Job job; };
    Chunk ch[kHostSlots];
    size_t off = 0, total = 0;                        // input consumed, output produced (or needed)
    size_t total_bound = 0;                           // length-preserving: output of everything submitted so far
    bool overflow = false;                            // the caller's buffer is too small: keep counting only
    bool diverged = false;                            // a chunk reported TRRE_E_DIVERGES: its partial output is the last thing that counts
    std::string diverge_msg;
    int rc = TRRE_OK;
    auto abandon = [&](int code) -> int {             // leave nothing queued behind an error
        for (auto& hs : st->slot) { (void)hipStreamSynchronize(hs.stream); hs.ctx.pend = Pending(); }
        for (Chunk& c : ch)
            if (c.leaving) { CopyPool::get().wait(c.job); c.leaving = false; }
        return code;
    };
    // stage chunk k in and queue its upload + scan (and, when the output size is known beforehand, its download)
    const bool trace_on = trre::switches().trace;
    double t_reserve = 0, t_first = 0;
    bool first_done = false;
    auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    auto submit = [&](int b, size_t at, size_t len) -> int {
        DeviceState::HostSlot& hs = st->slot[b];
        const auto tr = std::chrono::steady_clock::now();
        int r = slot_reserve(hs, true, len, !in_direct);
        if (r) return r;
        r = slot_reserve(hs, false, fixed_len ? len : len + len / 2 + 4096, !out_direct);
        if (r) return r;
        t_reserve += ms_since(tr);
        if (in_direct) {
            HIP_TRY(hipMemcpyAsync(hs.d_in, in + at, len, hipMemcpyHostToDevice, hs.stream));
        } else {
            CopyPool::get().copy(hs.pin_in, in + at, len, kCopyWays);
            HIP_TRY(hipMemcpyAsync(hs.d_in, hs.pin_in, len, hipMemcpyHostToDevice, hs.stream));
        }
        ch[b].off = at; ch[b].len = len; ch[b].out_at = 0; ch[b].m = 0; ch[b].submitted = true; ch[b].early = false;
        hs.ctx.relaunches = 0;
        const auto te = std::chrono::steady_clock::now();
        r = enqueue(p, st, &hs.ctx, fam, hs.d_in, len, hs.d_out, hs.out_cap, hs.stream);
        if (r) return r;
        if (!first_done) { t_first = ms_since(te); first_done = true; }
        if (fixed_len && !overflow && total_bound + len <= cap) {
            // length-preserving: the output is `len` bytes unless a NUL turns up (then complete() downloads again).  (Straight to its
            // place when the caller's buffer is pinned — if the chunks before it come out shorter after all, complete() downloads again.)
            HIP_TRY(hipMemcpyAsync(out_direct ? out + total_bound : hs.pin_out, hs.d_out, len, hipMemcpyDeviceToHost, hs.stream));
            ch[b].early = true;
            ch[b].early_at = total_bound;
        }
        total_bound += len;
        return TRRE_OK;
    };
    // wait for chunk b's scan, learn its output size, queue the download (unless it is already there)
    auto complete = [&](int b) -> int {
        DeviceState::HostSlot& hs = st->slot[b];
        size_t m = 0;
        int r = finish(p, st, &hs.ctx, &m);
        bool again = false;
        while (r == TRRE_E_CAPACITY) {                // the general families report the size they need
            r = slot_reserve(hs, false, m + 4096, !out_direct);
            if (r) return r;
            r = enqueue(p, st, &hs.ctx, fam, hs.d_in, ch[b].len, hs.d_out, hs.out_cap, hs.stream);
            if (!r) r = finish(p, st, &hs.ctx, &m);
            again = true;
        }
        if (r == TRRE_E_DIVERGES) {                   // the reference stops inside this chunk: what it had printed (m bytes) still counts
            diverged = true;
            diverge_msg = g_error;
            again = true;
        } else if (r) {
            return r;
        }
        ch[b].m = m;
        ch[b].out_at = total;
        if (!overflow && total + m > cap) overflow = true;
        if (!overflow && m) {
            // (the early download holds the FIRST launch's bytes: a relaunch inside finish() — mask scratch for a long
            // line, a NUL, a bounded fold that overflowed — rewrote d_out afterwards)
            if (!(ch[b].early && m == ch[b].len && !again && hs.ctx.relaunches == 0 && (!out_direct || ch[b].early_at == total)))
                HIP_TRY(hipMemcpyAsync(out_direct ? out + total : hs.pin_out, hs.d_out, m, hipMemcpyDeviceToHost, hs.stream));
            ch[b].copying = true;
        }
        total += m;
        ch[b].submitted = false;
        return TRRE_OK;
    };
    // chunk output: pinned -> caller, once its download has finished.  The copy is only started here (it runs on the
    // pool's threads while this thread stages the next chunk in); settle() waits for it before the slot is used again.
    auto drain = [&](int b) -> int {
        if (!ch[b].copying) return TRRE_OK;
        HIP_TRY(hipStreamSynchronize(st->slot[b].stream));
        ch[b].copying = false;
        if (out_direct) return TRRE_OK;            // (the download went to its place)
        CopyPool::get().start(ch[b].job, out + ch[b].out_at, st->slot[b].pin_out, ch[b].m, kCopyWays);
        ch[b].leaving = true;
        return TRRE_OK;
    };
    auto settle = [&](int b) {
        if (ch[b].leaving) { CopyPool::get().wait(ch[b].job); ch[b].leaving = false; }
    };
    // software pipeline, per iteration: chunk k is staged in by this thread (while chunk k-1 is on the device and chunk
    // k-2 is copied out by the pool), uploaded and scanned; then chunk k-1 is collected and its copy-out started
    for (int64_t k = 0;; ++k) {
        const bool more = off < n;
        if (more) {
            const int b = (int)(k % kHostSlots);
            rc = drain(b);                            // the slot's previous output must have left its staging buffer
            if (rc) return abandon(rc);
            settle(b);
            size_t len = n - off;                     // this chunk: up to kHostChunk bytes, extended to the end of its last line
            if (len > kHostChunk) {
                const void* nl = std::memchr(in + off + kHostChunk - 1, '\n', n - off - (kHostChunk - 1));
                len = nl ? (size_t)(static_cast<const uint8_t*>(nl) - (in + off)) + 1 : n - off;
            }
            rc = submit(b, off, len);
            if (rc) return abandon(rc);
            off += len;
        }
        if (k >= 1) {
            const int b1 = (int)((k - 1) % kHostSlots);
            if (ch[b1].submitted) { rc = complete(b1); if (rc) return abandon(rc); }
            rc = drain(b1);
            if (rc) return abandon(rc);
            if (diverged) {
                // nothing after the diverging chunk counts: the chunk submitted in this iteration is dropped
                off = n;
                for (int b = 0; b < kHostSlots; ++b)
                    if (ch[b].submitted) {
                        (void)hipStreamSynchronize(st->slot[b].stream);
                        st->slot[b].ctx.pend = Pending();
                        ch[b].submitted = false;
                    }
            }
        }
        if (!more) {
            bool busy = false;
            for (const Chunk& c : ch) busy = busy || c.submitted || c.copying;
            if (!busy) break;
        }
    }
    for (int b = 0; b < kHostSlots; ++b) settle(b);
    if (trace_on && t_reserve + t_first > 1.0)
        fprintf(stderr, "trre: host call of %zu bytes: %.1f ms getting staging and device buffers, %.1f ms in the first chunk's launch calls\n", n, t_reserve, t_first);
    if (out_len) *out_len = total;
    if (overflow) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    if (diverged) return fail(TRRE_E_DIVERGES, diverge_msg);
    return TRRE_OK;
}

// RAII: make `device` current for the calling thread, restore the previous one on return
struct DeviceScope {
    int prev = -1;
    hipError_t err;
    explicit DeviceScope(int device) {
        const bool trace_on = trre::switches().trace;
        static std::atomic<bool> first{true};
        const auto t0 = std::chrono::steady_clock::now();
        err = hipGetDevice(&prev);
        if (err == hipSuccess) err = hipSetDevice(device);
        if (trace_on && first.exchange(false))
            fprintf(stderr, "trre: first HIP calls of the process (runtime start-up): %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// the host paths stage their chunks anyway: a scan in place saves nothing there, and any overlap (out == in too) is refused
int host_overlap(const uint8_t* in, size_t n, const uint8_t* out, size_t cap) {
    if (n && out && (out == in || ranges_overlap(in, n, out, cap)))
        return fail(TRRE_E_ARG, "error: input and output overlap (the host paths take separate buffers)");
    return TRRE_OK;
}

// The shards of one call: cut at line ends, every shard scanned by `scan_shard` on a host thread of its own, the outputs put together in
// shard order.  (A function of its own so that the CPU test tier can drive the reassembly — eight shards, one of them ending the output —
// with a stand-in for the device call: trre_debug_scan_host_multi.)
using ShardFn = std::function<int(int shard, const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len)>;
int scan_shards(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len, int G, bool fixed_len, const ShardFn& scan_shard) {
    std::vector<size_t> bounds((size_t)G + 1);
    int rc = trre_shard_bounds(in, n, G, bounds.data());
    if (rc) return rc;
    // A length-preserving program writes every shard straight to its place (output offset == input offset);
    // otherwise a shard's offset is known only when the shards before it are done: each goes to a buffer of its
    // own and is moved into place afterwards.
    struct Shard { int rc = TRRE_OK; size_t m = 0; std::string err; std::vector<uint8_t> buf; bool own = false; uint32_t flags = 0; };
    std::vector<Shard> sh((size_t)G);
    std::vector<std::thread> th;
    for (int g = 0; g < G; ++g) {
        th.emplace_back([&, g] {
            Shard& s = sh[(size_t)g];
            try {
                const size_t lo = bounds[(size_t)g], len = bounds[(size_t)g + 1] - lo;
                if (len == 0) return;
                const bool direct = fixed_len && lo + len <= cap;
                uint8_t* dst = nullptr;
                size_t room = 0;
                // cap == 0 is a size query; otherwise a shard that cannot go straight to its place gets a buffer of its
                // own — also for a length-preserving program whose place lies beyond `cap`: NUL bytes may shorten the
                // shards before it, and the call must succeed whenever the TOTAL fits
                if (direct) { dst = out + lo; room = len; }
                else if (cap > 0) { s.buf.resize(fixed_len ? len + 64 : len + len / 2 + 4096); s.own = true; dst = s.buf.data(); room = s.buf.size(); }
                g_scan_flags = 0;
                s.rc = scan_shard(g, in + lo, len, dst, room, &s.m);
                if (s.rc == TRRE_E_CAPACITY && s.own) {          // the shard needs s.m bytes
                    s.buf.resize(s.m + 64);
                    s.rc = scan_shard(g, in + lo, len, s.buf.data(), s.buf.size(), &s.m);
                }
                if (s.rc && s.rc != TRRE_E_CAPACITY) s.err = trre_last_error();
                s.flags = g_scan_flags;                          // (this thread's: handed to the caller's below)
            } catch (const std::bad_alloc&) {                    // a multi-GB shard buffer: an error code, not std::terminate
                s.rc = TRRE_E_TOO_BIG;
                s.err = "error: out of host memory for a shard's output buffer";
            } catch (const std::exception& e) {
                s.rc = TRRE_E_DEVICE;
                s.err = std::string("error: ") + e.what();
            }
        });
    }
    for (auto& t : th) t.join();
    for (int g = 0; g < G; ++g) g_scan_flags |= sh[(size_t)g].flags;
    size_t total = 0;
    bool short_cap = false;
    int last = G, diverged_at = -1;                   // shards [0, last) count; a shard on which the reference stops is the last one
    for (int g = 0; g < G; ++g) {
        const Shard& s = sh[(size_t)g];
        if (s.rc == TRRE_E_DIVERGES) { diverged_at = g; last = g + 1; total += s.m; break; }
        if (s.rc && s.rc != TRRE_E_CAPACITY) return fail(s.rc, s.err);
        if (s.rc == TRRE_E_CAPACITY) short_cap = true;
        total += s.m;
    }
    if (out_len) *out_len = total;
    if (short_cap || total > cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");   // (short_cap: a size query, cap == 0)
    // move the shards into place, in order (a direct shard that came out shorter — NUL bytes — moves down)
    size_t at = 0;
    for (int g = 0; g < last; ++g) {
        const Shard& s = sh[(size_t)g];
        const uint8_t* src = s.own ? s.buf.data() : out + bounds[(size_t)g];
        if (s.m && src != out + at) std::memmove(out + at, src, s.m);
        at += s.m;
    }
    if (diverged_at >= 0) return fail(TRRE_E_DIVERGES, sh[(size_t)diverged_at].err);
    return TRRE_OK;
}
}  // namespace

extern "C" {

int trre_scan_host(trre_prog* p, const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len, int device) {
    g_scan_flags = 0;
    if (!p || (n && !in) || (cap && !out)) return fail(TRRE_E_ARG, "error: null argument");
    if (own_call_only(*p)) return fail_empty(out_len, TRRE_E_ARG, own_call_only(*p));
    if (out_len) *out_len = 0;
    if (host_overlap(in, n, out, cap)) return TRRE_E_ARG;
    if (n == 0) return TRRE_OK;
    DeviceScope scope(device);
    HIP_TRY(scope.err);
    DeviceState* st;
    int rc = device_state(p, device, &st);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(st->mu);
    if (is_generate(p->mode)) {
        std::vector<uint8_t> result;
        bool diverged = false;
        rc = generate_on(p, st, in, n, result, diverged);
        if (rc) return rc;
        if (out_len) *out_len = result.size();
        if (result.size() > cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
        if (!result.empty()) std::memcpy(out, result.data(), result.size());
        return diverged ? fail(TRRE_E_DIVERGES, kDivergeMsg) : TRRE_OK;
    }
    return scan_host_on(p, st, in, n, out, cap, out_len);
}

// Host buffers, line-sharded over several GPUs of this node: the reference's scan has no exchange step
// (a line's output depends on that line and the read-only program, trre_nft.c:776-790), so the input is
// cut at line ends into one contiguous shard per device (trre_shard_bounds), every device scans its shard on
// its own host thread and streams, and the outputs are concatenated in shard order — an exclusive sum of G
// sizes on the host, no collective.
int trre_scan_host_multi(trre_prog* p, const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len, uint32_t device_mask) {
    g_scan_flags = 0;
    if (!p || (n && !in) || (cap && !out)) return fail(TRRE_E_ARG, "error: null argument");
    if (own_call_only(*p)) return fail_empty(out_len, TRRE_E_ARG, own_call_only(*p));
    if (out_len) *out_len = 0;
    if (host_overlap(in, n, out, cap)) return TRRE_E_ARG;
    int n_dev = 0;
    {
        const bool trace_on = trre::switches().trace;
        static std::atomic<bool> first{true};
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipGetDeviceCount(&n_dev));
        if (trace_on && first.exchange(false))
            fprintf(stderr, "trre: hipGetDeviceCount, the first HIP call of the process (runtime start-up): %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::vector<int> devs;
    for (int d = 0; d < n_dev && d < 32; ++d)
        if (device_mask == 0 || (device_mask >> d & 1u)) devs.push_back(d);
    if (devs.empty()) return fail(TRRE_E_ARG, "error: device_mask selects no visible device");
    if (n == 0) return TRRE_OK;
    // TRRE_SHARDS_PER_DEVICE=k (tests): k shards per selected device, so that the sharding, the per-shard threads and
    // the reassembly run on a box with a single GPU (shards on one device take turns: calls are serialised per device)
    const int per_dev = trre::switches().shards_per_device;
    if (per_dev > 1) {
        std::vector<int> rep;
        for (int d : devs) rep.insert(rep.end(), (size_t)per_dev, d);
        devs.swap(rep);
    }
    const int G = (int)devs.size();
    if (G == 1) return trre_scan_host(p, in, n, out, cap, out_len, devs[0]);
    const int fam = scan_family(*p);
    const bool fixed_len = !is_gen(fam) && !is_generate(p->mode);
    const uint32_t flags0 = g_scan_flags;
    const int rc = scan_shards(in, n, out, cap, out_len, G, fixed_len,
                               [&](int g, const uint8_t* sin, size_t sn, uint8_t* sout, size_t scap, size_t* sm) { return trre_scan_host(p, sin, sn, sout, scap, sm, devs[(size_t)g]); });
    g_scan_flags |= flags0;
    return rc;
}

// CPU test tier: the sharding and the reassembly of trre_scan_host_multi with the caller's stand-in for the per-shard device call.
int trre_debug_scan_host_multi(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len, int n_shards, int fixed_len, trre_debug_shard_fn fn, void* user) {
    g_scan_flags = 0;
    if ((n && !in) || (cap && !out) || n_shards < 1 || !fn) return fail(TRRE_E_ARG, "error: null argument");
    if (out_len) *out_len = 0;
    if (n == 0) return TRRE_OK;
    return scan_shards(in, n, out, cap, out_len, n_shards, fixed_len != 0,
                       [&](int g, const uint8_t* sin, size_t sn, uint8_t* sout, size_t scap, size_t* sm) { return fn(user, g, sin, sn, sout, scap, sm); });
}

int trre_shard_bounds(const uint8_t* in, size_t n, int nshards, size_t* bounds) {
    if (nshards < 1 || !bounds || (n && !in)) return fail(TRRE_E_ARG, "error: bad shard request");
    bounds[0] = 0;
    for (int s = 1; s < nshards; ++s) {
        size_t cut = n / (size_t)nshards * (size_t)s;
        if (cut < bounds[s - 1]) cut = bounds[s - 1];
        const void* nl = cut < n ? std::memchr(in + cut, '\n', n - cut) : nullptr;
        bounds[s] = nl ? (size_t)(static_cast<const uint8_t*>(nl) - in) + 1 : n;
    }
    bounds[nshards] = n;
    return TRRE_OK;
}

}  // extern "C"
