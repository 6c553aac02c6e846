// runtime.cpp — the scan core of the host runtime: table upload, kernel-family selection, launches, status collection and repairs;
// generator modes; the plain device entry points of the C ABI (include/trre_mi355x.h).  The scan always runs on the GPU; nothing here
// computes output bytes on the host.  (The pattern compiler is compile.cpp, the column calls column_calls.cpp, the host path host_path.cpp.)
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <algorithm>
#include <thread>

#include <sys/mman.h>

#include "runtime_state.hpp"
#include "launch.hpp"
#include "switches.hpp"
#include "splice_block.hpp"
#include "gen_block.hpp"
#include "lazy_block.hpp"
#include "one_block.hpp"
#include "map_block.hpp"
#include "guard_block.hpp"

namespace trre_host {

thread_local std::string g_error;
thread_local uint32_t g_scan_flags = 0;       // TRRE_SCAN_*: what the last scan call on this thread has to add to its return code

constexpr int kNotThisRoute = 1;              // a launch route declines (positive: no TRRE_E_* code): the caller takes the next one

int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}
int fail_empty(size_t* out_len, int code, const std::string& msg) { if (out_len) *out_len = 0; return fail(code, msg); }     // ... and no output stands

// Pinned staging memory: anonymous pages (huge ones where the kernel gives them), touched by a few threads, then registered with the
// runtime.  hipHostMalloc of the host path's six 36 MiB buffers took 56 ms of a process's first scan call (the runtime allocates, clears
// and pins 4 KiB pages on one thread); this takes 3 ms and copies at the same 57 GB/s (tools/probes/pin_cost.hip, round 5).
static std::mutex g_pin_mu;
static std::map<void*, size_t> g_pin_len;
hipError_t pinned_get(uint8_t** out, size_t bytes) {
    const size_t len = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    void* m = ::mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) return hipErrorOutOfMemory;
#ifdef MADV_HUGEPAGE
    (void)::madvise(m, len, MADV_HUGEPAGE);
#endif
    {
        const int ways = len >= ((size_t)8 << 20) ? 4 : 1;
        const size_t piece = (len / (size_t)ways + 4095) & ~(size_t)4095;
        auto touch = [m, len, piece](int w) {
            volatile uint8_t* q = static_cast<volatile uint8_t*>(m);
            for (size_t k = (size_t)w * piece; k < std::min(len, (size_t)(w + 1) * piece); k += 4096) q[k] = 0;
        };
        std::vector<std::thread> th;
        for (int w = 1; w < ways; ++w) th.emplace_back(touch, w);
        touch(0);
        for (auto& t : th) t.join();
    }
    const hipError_t e = hipHostRegister(m, len, hipHostRegisterDefault);
    if (e != hipSuccess) { ::munmap(m, len); return e; }
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pin_len[m] = len;
    *out = static_cast<uint8_t*>(m);
    return hipSuccess;
}
void pinned_put(uint8_t* p) {
    if (!p) return;
    size_t len = 0;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pin_len.find(p);
        if (it == g_pin_len.end()) return;
        len = it->second;
        g_pin_len.erase(it);
    }
    (void)hipHostUnregister(p);
    ::munmap(p, len);
}

bool is_generate(int mode) { return mode == TRRE_MODE_SCAN_ALL || mode == TRRE_MODE_MATCH_ALL; }
static bool is_stream(int fam) { return fam == TRRE_KERNEL_STREAM_LP || fam == TRRE_KERNEL_STREAM_GEN; }
static bool is_guided(int fam) { return fam == TRRE_KERNEL_GUIDED_LP || fam == TRRE_KERNEL_GUIDED_GEN; }
bool is_gen(int fam) {
    return fam == TRRE_KERNEL_TILE_GEN || fam == TRRE_KERNEL_STREAM_GEN || fam == TRRE_KERNEL_GUIDED_GEN || fam == TRRE_KERNEL_BACKTRACK || fam == TRRE_KERNEL_DFT_LAZY;
}
static bool is_guided_wide(const trre_prog& p, int fam) { return (fam == TRRE_KERNEL_GUIDED_LP || fam == TRRE_KERNEL_GUIDED_GEN) && p.gt.wide; }
// how the guided families' backward pass stores its symbols: 4 two per byte, 8 one per byte, 16 two bytes each (wide tables)
int guided_sym_bits(const trre_prog& p) { return p.gt.wide ? 16 : (p.gt.sym_bits == 4 && !trre::switches().no_g16 ? 4 : 8); }
static bool lp_inplace(uint32_t flags) { return (flags & trre::kFlagLengthPreserving) && (flags & trre::kFlagNoOverrun); }
// the family that takes over when a length-preserving launch met a NUL, or a bounded stream table a long run
static int general_family(const trre_prog& p, bool stream_ok) {
    if (p.lazy_only) return TRRE_KERNEL_DFT_LAZY;
    if (stream_ok && p.stt.ok) return TRRE_KERNEL_STREAM_GEN;
    if (p.gt.ok) return TRRE_KERNEL_GUIDED_GEN;
    if (p.engine == TRRE_ENGINE_DFT && p.mode == TRRE_MODE_SCAN) return TRRE_KERNEL_DFT_LAZY;      // (round 6: 100 GB/s against the tile kernels' 48)
    return p.has_engine_tables ? TRRE_KERNEL_TILE_GEN : TRRE_KERNEL_BACKTRACK;
}

static int auto_family(const trre_prog& p) {
    using namespace trre;
    if (p.mode == TRRE_MODE_FIND) return TRRE_KERNEL_GUIDED_GEN;      // (both scans of trre_find_device_strings: their outputs are no one's input length)
    if (p.mode == TRRE_MODE_SPANS) return TRRE_KERNEL_GUIDED_GEN;     // (the scan of trre_span_device_strings: the table is never length-preserving)
    if (p.mode == TRRE_MODE_SUB) return TRRE_KERNEL_GUIDED_GEN;       // (the spans scan of trre_sub_device_strings; its texts scan runs an inner find program)
    if (p.lazy_only) return TRRE_KERNEL_DFT_LAZY;      // beyond the eager construction's caps: the tables grow with the input (lazy_block.hpp)
    if (p.engine == TRRE_ENGINE_DFT && (p.dt.flags & kFlagMemoryless)) return TRRE_KERNEL_BYTEMAP;
    // a stream table too large for LDS is walked through L1/L2 (<= 0.35 TB/s); guided tables with a small forward table
    // run at 0.6-0.8 TB/s: prefer them then (patterns with `.` or wide ranges before a literal fold into hundreds of
    // states x 256 classes)
    const bool stream_small = p.stt.ok && (p.stt.g16_ok || p.stt.lpw_ok);
    const bool guided_small = p.gt.ok && p.gt.fwd.g16_ok && !p.gt.wide;
    // (a bounded fold whose flushes do not fit the 16-byte entries — 'a*b:x': up to 64 pending bytes go out raw when the b does not
    // come — walks them on its slow path: 0.30 TB/s against 0.60 for the guided tables of the same pattern; ' +: ' has none: 0.72 / 0.59)
    const bool bounded_slow = p.stt.ok && p.stt.bounded && (p.stt.flags & kFlagG16Slow) && guided_small;
    if (p.stt.ok && !bounded_slow && (stream_small || !guided_small)) return lp_inplace(p.stt.flags) ? TRRE_KERNEL_STREAM_LP : TRRE_KERNEL_STREAM_GEN;
    // (wide guided tables — 16-bit symbols, both tables through L1 / L2 — still beat the bitmask tile kernels: 37 against 17 GB/s
    // on 'a(a|b|c){9}c:x', 256 MiB of printable lines)
    if (p.gt.ok) return lp_inplace(p.gt.fwd.flags) && !p.gt.wide ? TRRE_KERNEL_GUIDED_LP : TRRE_KERNEL_GUIDED_GEN;
    if (p.mode == TRRE_MODE_MATCH) return TRRE_KERNEL_BACKTRACK;
    if (p.engine == TRRE_ENGINE_DFT) {
        // A DFT pattern without a fold and beyond the guided tables (a reduced backward automaton of more than 16 384 states, or one that its
        // construction's budget does not reach).  Rounds 1-5: the tile kernels, 48 GB/s; round 6: the lazily determinised family, which runs any
        // DFT scan at twice that once its tables have grown — a first scan that needs more than kLazyAutoRounds rounds of
        // growing hands the buffer to the tile kernels (finish_inner) and the tables keep what they learnt.
        if (p.mode == TRRE_MODE_SCAN) return TRRE_KERNEL_DFT_LAZY;
        if ((p.dt.flags & kFlagLengthPreserving) && (p.dt.flags & kFlagNoOverrun)) return TRRE_KERNEL_TILE_LP;
        return TRRE_KERNEL_TILE_GEN;
    }
    // beyond every table form (more than 64 nodes, a backward automaton beyond the guided limits, no fold): the search itself
    if (!p.has_engine_tables) return TRRE_KERNEL_BACKTRACK;
    return (p.nt.flags & kFlagLengthPreserving) ? TRRE_KERNEL_TILE_LP : TRRE_KERNEL_TILE_GEN;
}

// the family a scan call launches: the forced one, else the automatic choice — which leaves a bounded stream table alone once
// a launch on it has overflowed
int scan_family(const trre_prog& p) {
    if (p.forced_family) return p.forced_family;
    const int fam = auto_family(p);
    if (is_stream(fam) && p.stt.bounded && p.bounded_off.load()) return general_family(p, false);
    return fam;
}

static bool family_allowed(const trre_prog& p, int fam) {
    using namespace trre;
    if (fam == TRRE_KERNEL_DFT_LAZY) return p.engine == TRRE_ENGINE_DFT && p.mode == TRRE_MODE_SCAN;
    if (p.lazy_only) return false;
    if (fam == TRRE_KERNEL_STREAM_GEN) return p.stt.ok;
    if (fam == TRRE_KERNEL_STREAM_LP) return p.stt.ok && lp_inplace(p.stt.flags);
    if (fam == TRRE_KERNEL_GUIDED_GEN) return p.gt.ok;
    if (fam == TRRE_KERNEL_GUIDED_LP) return p.gt.ok && lp_inplace(p.gt.fwd.flags) && !p.gt.wide;
    if (fam == TRRE_KERNEL_BACKTRACK) return p.bt_ok;
    if (!p.has_engine_tables) return false;
    if (fam == TRRE_KERNEL_TILE_GEN) return true;
    if (p.engine == TRRE_ENGINE_DFT) {
        if (fam == TRRE_KERNEL_BYTEMAP) return (p.dt.flags & kFlagMemoryless) != 0;
        return (p.dt.flags & kFlagLengthPreserving) && (p.dt.flags & kFlagNoOverrun);
    }
    if (fam == TRRE_KERNEL_BYTEMAP) return false;
    return (p.nt.flags & kFlagLengthPreserving) != 0;
}

int ctx_init(ScanCtx& c) {
    if (c.d_status) return TRRE_OK;
    // status words [4], then the byte map's NUL list: a count, kNulCap offsets, kNulCap line ends (repair_bytemap_nuls)
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c.d_status), 24 + (size_t)trre::kNulCap * 16));
    HIP_TRY(hipMemset(c.d_status, 0, 24));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c.h_status), 16, hipHostMallocDefault));
    HIP_TRY(hipEventCreate(&c.ev0));
    HIP_TRY(hipEventCreate(&c.ev1));
    return TRRE_OK;
}
static void ctx_free(ScanCtx& c) {
    (void)hipFree(c.d_status);
    if (c.h_status) (void)hipHostFree(c.h_status);
    if (c.ev0) (void)hipEventDestroy(c.ev0);
    if (c.ev1) (void)hipEventDestroy(c.ev1);
    c = ScanCtx();               // (every DevBuf lets go of its memory here)
}

// the prog's state on device `dev` (tables uploaded on first use); the calling thread's current device must be `dev`
int device_state(trre_prog* p, int dev, DeviceState** out) {
    std::lock_guard<std::mutex> lock(p->dev_mu);
    auto it = p->dev.find(dev);
    if (it == p->dev.end()) {
        const bool trace_on = trre::switches().trace;
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_ptr<DeviceState> st(new DeviceState);
        st->device = dev;
        auto upload = [&](const std::vector<uint8_t>& b, uint8_t** d) -> int {
            if (b.empty()) return TRRE_OK;
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(d), b.size()));
            HIP_TRY(hipMemcpy(*d, b.data(), b.size(), hipMemcpyHostToDevice));
            return TRRE_OK;
        };
        int rc = upload(p->blob, &st->d_blob);
        if (!rc) rc = upload(p->sblob, &st->d_sblob);
        if (!rc) rc = upload(p->gblob, &st->d_gblob);
        if (!rc) rc = upload(p->rblob, &st->d_rblob);
        if (!rc) rc = upload(p->nblob, &st->d_nblob);
        if (!rc) rc = upload(p->kblob, &st->d_kblob);
        if (!rc) rc = upload(p->ablob, &st->d_ablob);
        if (!rc) rc = ctx_init(st->ctx);
        if (rc) return rc;
        if (trace_on) fprintf(stderr, "trre: device %d: tables up in %.1f ms\n", dev, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        it = p->dev.emplace(dev, std::move(st)).first;
    }
    *out = it->second.get();
    return TRRE_OK;
}

// the arguments every kernel starts from: the input as 16-byte vectors — its pointer split at the alignment — and the output at the same offset
static trre::ScanArgs base_args(const uint8_t* d_in, size_t n, uint8_t* d_out = nullptr) {
    const int64_t a = (int64_t)(reinterpret_cast<uintptr_t>(d_in) & 15u);
    trre::ScanArgs args{};
    args.in_v0 = d_in - a;
    if (d_out) { args.out_v0 = d_out - a; args.out = d_out; }
    args.vbeg = a;
    args.vend = a + (int64_t)n;
    return args;
}

static int ensure_workspace(ScanCtx* c, int64_t n_chunks, int threads) {
    n_chunks = n_chunks * ((threads + 255) / 256);      // sized in units of 256-lane chunks
    HIP_TRY(c->d_lane_counts.reserve((size_t)n_chunks, (size_t)n_chunks * 256 * 4));
    HIP_TRY(c->d_chunk_total.reserve((size_t)n_chunks, (size_t)n_chunks * 8));
    HIP_TRY(c->d_chunk_base.reserve((size_t)n_chunks, (size_t)(n_chunks + 1) * 8));
    return TRRE_OK;
}

constexpr uint32_t kCopyEvCap = 256;       // events per lane of the copy form (a 2 KiB sub-range of the dictionary corpus holds ~120)

// ---- the stack guard (guard_block.hpp) --------------------------------------------------------------------------------
constexpr int64_t kGuardSlots = 256;                       // lines searched at a time (a stack of 65 536 items each: 192 MiB in all)
constexpr size_t kGuardMaxRuns = 1024;                     // suspects per batch (the call's budget is looked at between batches)
constexpr uint64_t kGuardBudget = 1ull << 23;              // search steps per line; beyond: not decided (the scan's output stands)
// ... and per scan call, summed over its suspect lines in input order, batch by batch (TRRE_GUARD_CALL_BUDGET).  Steps, not seconds:
// the same input gives the same answer on a loaded host and on an idle one (round 4 stopped after 20 s of wall clock).  What the budgets
// leave undecided is SAID: TRRE_SCAN_GUARD_UNDECIDED in trre_last_scan_flags().
constexpr uint64_t kGuardCallBudget = 1ull << 35;
static bool guard_applies(const trre_prog& p, const ScanCtx& cx, size_t n) {
    return !trre::switches().no_stack_guard && p.guard.on && !cx.guard_off &&
           (p.mode == TRRE_MODE_SCAN || p.mode == TRRE_MODE_MATCH || p.mode == TRRE_MODE_FIND || p.mode == TRRE_MODE_SPANS || p.mode == TRRE_MODE_SUB) && n + 1 >= p.guard.l_min;
}
struct GuardHit {
    bool hit = false;
    uint64_t line_start = 0;
    uint32_t part = 0;         // bytes of the line's output in cx->d_gout, or ~0u: they could not be produced
};
template <class T>
static int guard_room(DevBuf<T>& d, size_t want) {
    if (d.reserve(want, want * sizeof(T)) != hipSuccess) return fail(TRRE_E_TOO_BIG, "error: out of device memory (stack guard)");
    return TRRE_OK;
}
// Looks for lines long enough to exhaust the reference's stack and runs the reference's search on them.  Synchronous: it ends
// with the stream idle.  hit: the first line (in input order) on which the search overflows, and what the reference had printed of it.
static int guard_check(trre_prog* p, DeviceState* st, ScanCtx* cx, const uint8_t* d_in, size_t n, hipStream_t stream, GuardHit* hit) {
    using namespace trre;
    const GuardTables& g = p->guard;
    ScanArgs args = base_args(d_in, n);
    const int64_t n_win = ((int64_t)n + g.window - 1) / g.window;
    const size_t n_words = (size_t)(n_win + 255) / 256 * 4;
    int rc = guard_room(cx->d_gflags, n_words);
    if (rc) return rc;
    args.blob = st->d_kblob;
    launch_guard_probe(args, g.window, n_win, cx->d_gflags, stream);
    HIP_TRY(hipGetLastError());
    std::vector<uint64_t> flags(n_words);
    HIP_TRY(hipMemcpyAsync(flags.data(), cx->d_gflags, n_words * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    // the runs of flagged windows, a batch at a time (input order: the first line that overflows is the one that counts)
    std::vector<GuardRun> runs;
    std::vector<GuardResult> res;
    GuardArgs ga{};
    GuardResult* d_res = nullptr;
    GuardRun* d_runs = nullptr;
    size_t bad = 0;
    bool found = false;
    const uint64_t call_budget = (uint64_t)switches().guard_call_budget.or_else((long long)kGuardCallBudget);
    uint64_t steps_spent = 0;
    bool undecided = false;
    for (int64_t w = 0; w < n_win && !found;) {
        if (steps_spent > call_budget) {            // suspects are left and the call's budget is spent: they are not decided — and the caller is told
            for (int64_t x = w; x < n_win && !undecided; x = (x | 63) + 1)
                if (flags[(size_t)(x >> 6)] >> (x & 63)) undecided = true;
            break;
        }
        runs.clear();
        while (w < n_win && runs.size() < kGuardMaxRuns) {
            const uint64_t word = flags[(size_t)(w >> 6)] >> (w & 63);
            if (!word) { w = (w | 63) + 1; continue; }
            if (!(word & 1u)) { w += __builtin_ctzll(word); continue; }
            int64_t e = w;
            while (e + 1 < n_win && ((flags[(size_t)((e + 1) >> 6)] >> ((e + 1) & 63)) & 1u)) ++e;
            runs.push_back(GuardRun{(uint32_t)w, (uint32_t)e});
            w = e + 1;
        }
        if (runs.empty()) break;
        const size_t n_runs = runs.size();
        rc = guard_room(cx->d_gruns, n_runs * (sizeof(GuardRun) + sizeof(GuardResult)));      // (runs and results share one allocation)
        if (!rc) rc = guard_room(cx->d_gstack, (size_t)kGuardSlots * kGuardStackMax * 3);     // (allocated once)
        if (rc) return rc;
        d_res = reinterpret_cast<GuardResult*>(cx->d_gruns.p);
        d_runs = reinterpret_cast<GuardRun*>(cx->d_gruns.p + n_runs * sizeof(GuardResult));
        HIP_TRY(hipMemcpyAsync(d_runs, runs.data(), n_runs * sizeof(GuardRun), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_res, 0, n_runs * sizeof(GuardResult), stream));
        ga = GuardArgs{};
        ga.blob = st->d_kblob;
        ga.runs = d_runs;
        ga.results = d_res;
        ga.stack = cx->d_gstack;
        ga.budget = (uint64_t)switches().guard_budget.or_else((long long)kGuardBudget);
        ga.obuf = nullptr;                    // (the search alone: PROD writes nothing, FINAL prints nothing)
        ga.obuf_cap = 0xffffffffu;
        launch_guard(false, args, ga, (int64_t)n_runs, kGuardSlots, stream);
        HIP_TRY(hipGetLastError());
        res.resize(n_runs);
        HIP_TRY(hipMemcpyAsync(res.data(), d_res, n_runs * sizeof(GuardResult), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (size_t k = 0; k < n_runs && !found; ++k) {
            if (res[k].status == 1u) { bad = k; found = true; break; }
            if (res[k].status == 2u) undecided = true;          // this line's search outran its budget (or the line has more than 4 GiB)
            steps_spent += res[k].bad_at;                       // (a line that did not overflow leaves its step count there)
        }
    }
    // (lines BEFORE a line that overflows and not decided themselves: the answer given is the first overflow found — flagged too)
    if (undecided) g_scan_flags |= TRRE_SCAN_GUARD_UNDECIDED;
    if (!found) return TRRE_OK;
    hit->hit = true;
    hit->line_start = res[bad].line_start;
    hit->part = 0xffffffffu;
    // the same line again, printing: what the reference had printed of it when it gave up
    const uint64_t line_len = res[bad].out_len;             // (the search pass leaves the line's length here)
    const uint64_t obuf_want = 16 * (line_len + 1) + 65536, out_want = 16 * (res[bad].bad_at + 1) + 65536;
    if (obuf_want > (1ull << 30) || out_want > (1ull << 30)) return TRRE_OK;
    if (guard_room(cx->d_gobuf, (size_t)obuf_want) || guard_room(cx->d_gout, (size_t)out_want)) return TRRE_OK;
    ga.runs = d_runs + bad;
    ga.results = d_res + bad;
    ga.obuf = cx->d_gobuf;
    ga.obuf_cap = (uint32_t)std::min<uint64_t>(cx->d_gobuf.cap, 0xfffffff0u);
    ga.out = cx->d_gout;
    ga.out_cap = cx->d_gout.cap;
    launch_guard(true, args, ga, 1, 1, stream);
    HIP_TRY(hipGetLastError());
    GuardResult again{};
    HIP_TRY(hipMemcpyAsync(&again, d_res + bad, sizeof again, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (again.status == 1u) hit->part = again.out_len;
    return TRRE_OK;
}

// the backtracking fallback: sub-range per thread, frames (= bytes an attempt may consume) and path bytes per thread, workgroups in the pool, steps per sub-range
constexpr int64_t kBtLaneBytes = 1024;
constexpr uint32_t kBtBudget = 16u << 20;
// The pool of stacks and path buffers sizes the scratch, not the input: 3.4-4.6 GB in every tier.  A launch in which an attempt outgrew its
// stack or its path buffer runs again on the next tier (round 4 gave up at 4 096 bytes / 4 KiB of output).  The search waits on memory — a
// stack frame, list bounds, a follow entry, the byte, its set: dependent loads — so the first tier is sized for the MACHINE: 1 536 workgroups
// are six waves per SIMD (k_bt's registers allow six), and 512 frames are what such a pool can have; the second tier is round 4's
// (one wave per SIMD: a sixth of the rate).
struct BtTier { int64_t pool_blocks; uint32_t frames, path_cap; };
constexpr int kBtTierCount = 4;
constexpr BtTier kBtTiers[kBtTierCount] = {{1536, 512, 512}, {256, 4096, 4096}, {16, 65536, 65536}, {1, 1u << 20, 1u << 20}};
// ---- the deterministic engine on tables still being built (front.hpp: LazyDft, lazy_block.hpp) ----
constexpr int64_t kLazyLaneBytes = 1024;
constexpr uint32_t kLazyMissCap = 1u << 16;
static_assert(trre::kLazyMissWords == trre::kLazyRecWords, "miss record layout");
constexpr uint64_t kLazyBudget = 1ull << 32;             // table steps per sub-range (an attempt per byte of a long line is quadratic, as in the reference)

// brings the device's copy of the tables up to the host's: the pool's new bytes, then the new rows, then the old rows that changed (an entry
// must never name a row or a text the device does not hold yet — scans of other chunks may be reading the tables meanwhile)
static int lazy_sync(trre_prog* p, DeviceState* st) {
    std::lock_guard<std::mutex> lock(p->lazy_mu);
    const trre::LazyDft& z = *p->lazy;
    const uint32_t n_cls = z.n_cls(), rows = z.n_rows();
    const size_t pool = z.pool_bytes();
    if (!st->d_lcls) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&st->d_lcls), 256));
        HIP_TRY(hipMemcpy(st->d_lcls, z.cls(), 256, hipMemcpyHostToDevice));
    }
    if (pool > st->lpool_cap) {
        size_t cap = st->lpool_cap ? st->lpool_cap : (size_t)1 << 20;
        while (cap < pool) cap *= 2;
        uint8_t* fresh = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&fresh), cap));
        if (st->d_lpool) st->retired.push_back(st->d_lpool);
        st->d_lpool = fresh;
        st->lpool_cap = cap;
        st->lazy_pool_up = 0;
    }
    if (rows > st->lent_cap) {
        size_t cap = st->lent_cap ? st->lent_cap : 4096;
        while (cap < rows) cap *= 2;
        uint64_t* fresh = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&fresh), cap * n_cls * 8));
        if (st->d_lent) st->retired.push_back(st->d_lent);
        st->d_lent = fresh;
        st->lent_cap = cap;
        st->lazy_rows_up = 0;
    }
    if (pool > st->lazy_pool_up) {
        HIP_TRY(hipMemcpy(st->d_lpool + st->lazy_pool_up, z.pool() + st->lazy_pool_up, pool - st->lazy_pool_up, hipMemcpyHostToDevice));
        st->lazy_pool_up = pool;
    }
    if (rows > st->lazy_rows_up) {
        HIP_TRY(hipMemcpy(st->d_lent + (size_t)st->lazy_rows_up * n_cls, z.ent() + (size_t)st->lazy_rows_up * n_cls, (size_t)(rows - st->lazy_rows_up) * n_cls * 8,
                          hipMemcpyHostToDevice));
    }
    const uint32_t dirty = z.first_dirty_row(st->lazy_epoch_up);
    if (dirty < st->lazy_rows_up)
        HIP_TRY(hipMemcpy(st->d_lent + (size_t)dirty * n_cls, z.ent() + (size_t)dirty * n_cls, (size_t)(st->lazy_rows_up - dirty) * n_cls * 8, hipMemcpyHostToDevice));
    st->lazy_rows_up = rows;
    st->lazy_epoch_up = z.epoch();
    return TRRE_OK;
}

// one round: the count pass (fresh: every lane; else the lanes that are still void), the exclusive sum, the emit pass (which leaves at once
// when the count pass met a miss)
static int lazy_round(trre_prog* p, DeviceState* st, ScanCtx* cx, const trre::ScanArgs& args, int64_t n_chunks, bool fresh, hipStream_t stream) {
    using namespace trre;
    int rc = lazy_sync(p, st);
    if (rc) return rc;
    HIP_TRY(cx->d_miss.reserve(1, (size_t)(2 + trre::kLazyMissWords * kLazyMissCap) * 4));       // (allocated once)
    HIP_TRY(hipMemsetAsync(cx->d_miss, 0, 8, stream));
    if (fresh) HIP_TRY(hipMemsetAsync(cx->d_lane_counts, 0xff, (size_t)n_chunks * 256 * 4, stream));
    LazyArgs la{};
    la.cls = st->d_lcls;
    la.ent = st->d_lent;
    la.pool = st->d_lpool;
    la.n_cls = p->lazy->n_cls();
    la.n_rows = st->lazy_rows_up;
    la.miss = cx->d_miss;
    la.miss_cap = kLazyMissCap;
    static std::atomic<uint32_t> launch_id{0};
    la.gen = ++launch_id;                     // (lazy_block.hpp: marks of other launches — other chunks in flight on the same table — are listed again)
    la.budget = (uint64_t)switches().lazy_budget.or_else((long long)kLazyBudget);
    launch_lazy(1, args, la, kLazyLaneBytes, n_chunks, stream);
    launch_chunk_scan(cx->d_chunk_total, cx->d_chunk_base, n_chunks, stream);
    launch_lazy(2, args, la, kLazyLaneBytes, n_chunks, stream);
    HIP_TRY(hipGetLastError());
    return TRRE_OK;
}

// Launches of the memoryless kernel wait for one another, device by device: the kernel wants its whole grid resident (a tile's look-back waits for
// the tiles of the other workgroups), and two of them on two streams — the host path's chunks in flight — would each hold a part of the machine
// and wait for the rest until their spins ran out.  (Other kernels beside it only delay it: they end, its workgroups move in.)
struct MapGenChain { std::mutex mu; hipEvent_t ev = nullptr; bool any = false; };
static MapGenChain g_mapgen_chain[64];

// the memoryless kernel's workspace and launch (map_block.hpp); TRRE_OK: launched (pd.total_at set), else the caller takes another route
static int mapgen_launch(ScanCtx* cx, const trre::ScanArgs& args, const trre::StreamTables& stt, hipStream_t stream, Pending& pd) {
    using namespace trre;
    MapGenArgs oa{};
    oa.n_tiles = (args.vend + kMapGenTile - 1) / kMapGenTile;
    const size_t groups = (size_t)(oa.n_tiles / 64 + 1);
    const Switches& sw = switches();
    const char* dbg_env = sw.mapgen_dbg;
    const size_t words = (size_t)oa.n_tiles + 2 * groups + 1 + 8 + (dbg_env ? 16 * (size_t)oa.n_tiles : 0);   // descriptors, group sums, group totals, the total, phase clocks
    if (dbg_env) cx->d_mg.release();                 // (a fresh allocation for every launch)
    if (cx->d_mg.reserve((size_t)oa.n_tiles, words * 8) != hipSuccess) { (void)hipGetLastError(); return kNotThisRoute; }
    oa.desc = cx->d_mg;
    oa.gsum = cx->d_mg + oa.n_tiles;
    oa.ginc = oa.gsum + groups;
    oa.total = oa.ginc + groups;
    // the windows (two: a tile is stored a trip after it was expanded): the whole output of a tile as a rule — 16 KiB of input and an eighth: four
    // workgroups' pairs of windows share a CU's 160 KiB; a tile that prints more takes the clipped path, window by window
    uint32_t window = sw.mapgen_window > 0 ? (uint32_t)sw.mapgen_window : (uint32_t)(kMapGenTile + kMapGenTile / 8);
    oa.window = (window + 15u) & ~15u;
    oa.spin = 1u << 16;
    if (sw.mapgen_nolb) oa.spin = 7u;
    oa.prof = sw.mapgen_prof ? oa.total + 1 : nullptr;
    oa.dbg = dbg_env ? oa.total + 1 + 8 : nullptr;
    oa.longest = stt.mg_max;
    oa.first_lookup = 0;
    for (int c = 0; c < 256; ++c)
        if ((stt.mg[4 * c + 2] & (15u | kMgNul)) == 1u && (stt.mg[4 * c] & 0xffu) != (uint32_t)c) oa.first_lookup = 1;   // (a NUL voids the launch: whatever it prints)
    if (hipMemsetAsync(cx->d_mg, 0, words * 8, stream) != hipSuccess) { (void)hipGetLastError(); return kNotThisRoute; }
    {
        int dev = 0;
        (void)hipGetDevice(&dev);
        MapGenChain& ch = g_mapgen_chain[dev & 63];
        std::lock_guard<std::mutex> lk(ch.mu);
        if (!ch.ev && hipEventCreateWithFlags(&ch.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ch.ev = nullptr; return kNotThisRoute; }
        if (ch.any && hipStreamWaitEvent(stream, ch.ev, 0) != hipSuccess) { (void)hipGetLastError(); return kNotThisRoute; }
        if (launch_mapgen(args, oa, stream) != 0) return kNotThisRoute;
        if (hipEventRecord(ch.ev, stream) != hipSuccess) { (void)hipGetLastError(); return kNotThisRoute; }
        ch.any = true;
    }
    pd.total_at = oa.total;
    pd.mapgen = true;
    return TRRE_OK;
}

// Long lines (round 5): is there a sample point without a line end within 32 KiB?  Asked once per buffer (a tiny kernel and a wait), for the
// families that have the exact sub-ranges to answer with; a length-preserving family then runs as its general sibling (count, exclusive sum,
// emit: the exact sub-ranges live there).  *family: the family that runs.
static int long_line_switch(trre_prog* p, ScanCtx* cx, int* family, const uint8_t* d_in, size_t n, size_t cap, hipStream_t stream) {
    const int exact_env = trre::switches().exact;
    const bool small_tables = (*family == TRRE_KERNEL_STREAM_LP && p->stt.g16_ok) || (*family == TRRE_KERNEL_GUIDED_LP && p->gt.fwd.g16_ok && !p->gt.wide);
    if (!small_tables || cx->exact_off || exact_env == 0 || cap < n) return TRRE_OK;
    if (cx->probe_in != d_in || cx->probe_n != n) {
        HIP_TRY(cx->d_probe.reserve(1, 16));                // (allocated once)
        uint32_t misses = 0;
        HIP_TRY(hipMemsetAsync(cx->d_probe, 0, 4, stream));
        trre::launch_line_probe(base_args(d_in, n), 32768, cx->d_probe, stream);
        HIP_TRY(hipMemcpyAsync(&misses, cx->d_probe, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        cx->probe_in = d_in; cx->probe_n = n;
        cx->long_lines = misses != 0;
    }
    if (exact_env == 2 || cx->long_lines)       // (TRRE_EXACT=2: the switch whatever the lines, for A/B runs and tests)
        *family = *family == TRRE_KERNEL_STREAM_LP ? TRRE_KERNEL_STREAM_GEN : TRRE_KERNEL_GUIDED_GEN;
    return TRRE_OK;
}

// the stream-form tables a launch of `family` walks
static const trre::StreamTables& walked_tables(const trre_prog* p, int family) { return is_guided(family) ? p->gt.fwd : p->stt; }

// the launch of `family` over [d_in, d_in + n): arguments, lanes, chunks, table forms.  Touches nothing on the device.
static LaunchPlan make_plan(const trre_prog* p, const DeviceState* st, const ScanCtx* cx, int family, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap) {
    using namespace trre;
    const Switches& sw = switches();
    LaunchPlan pl;
    ScanArgs& args = pl.args;
    args = base_args(d_in, n, d_out);
    args.blob = is_stream(family) ? st->d_sblob : (is_guided(family) ? st->d_gblob : st->d_blob);
    const StreamTables& stt = walked_tables(p, family);
    args.status = cx->d_status;
    args.cap = cap;
    // a mask scratch left by an earlier, smaller scan must not be used: the kernel asks for one again
    args.gscratch = cx->d_scratch.cap >= (n + 32) * (size_t)p->mask_bytes ? cx->d_scratch.p : nullptr;
    const bool backtrack = family == TRRE_KERNEL_BACKTRACK;
    const bool lazy = family == TRRE_KERNEL_DFT_LAZY;
    // (the stream and guided families run the direct kernels — a lane walks a long sub-range straight from memory —: their chunks are
    // counted below, once the sub-range is known.  Rounds 1-5 also kept LDS-tile kernels for the stream tables, TRRE_STREAM_IMPL=0:
    // 10-100 GB/s, no job since round 2, removed in round 6)
    const int chunk = backtrack ? (int)kBtLaneBytes * 256 : lazy ? (int)kLazyLaneBytes * 256
                      : is_stream(family) ? 2048 * direct_block_threads() : chunk_bytes(p->engine, p->mask_bytes);
    pl.threads = backtrack || lazy ? 256 : is_stream(family) ? direct_block_threads() : block_threads(p->engine, p->mask_bytes);
    pl.n_chunks = (args.vend + chunk - 1) / chunk;
    // the positional-window kernel (wave-tiled I/O) for length-preserving tables that have the window form, the direct walkers otherwise
    pl.window = is_stream(family) && family == TRRE_KERNEL_STREAM_LP && p->stt.lpw_ok &&
                (reinterpret_cast<uintptr_t>(args.out_v0) & 15u) == 0;   // its 16-byte stores: in and out congruent mod 16 (unaligned they work, at the pace
                                                                         // of the emit pass alone: 0.94 against 0.98 ms per GiB, round 4)
    // sub-range per lane: 2 KiB, growing with the input so that about half a million lanes (8192 waves)
    // walk it — per-lane costs (the skipped head, the tail beyond the sub-range, the wave waiting for its
    // slowest lane) shrink with longer lanes: cfg 4 at 8 GiB 1.72 TB/s with 2 KiB lanes, 2.06 with 16 KiB
    int64_t lane_auto = 2048;
    if (pl.window)
        while (lane_auto < 16384 && (int64_t)n / (lane_auto * 2) >= 524288) lane_auto *= 2;
    // (the count / emit pair on the 16-byte entries gains too — 'a:xyz' at 8 GiB: 920 GB/s with 2 KiB lanes, 967 with 8 KiB, 946 with
    // 32 KiB; ' +: ' 896 / 947 / 805 — and so does the mark + splice pair of a large table, its event lists growing with the sub-range:
    // cfg 5 at 4 GiB 594 / 663 (4 KiB) / 675; the guided families do not: 647 / 641)
    // (the guided families' forward passes gain 2 % at 8 GiB, their backward pass loses 15 %: it keeps 2 KiB)
    if ((family == TRRE_KERNEL_STREAM_GEN && (p->stt.g16_ok || p->stt.fb_ok)) || (is_guided(family) && !p->gt.wide))
        while (lane_auto < 8192 && (int64_t)n / (lane_auto * 2) >= 262144) lane_auto *= 2;
    pl.lane_bytes = sw.lane_bytes > 0 ? (sw.lane_bytes + 127) / 128 * 128 : lane_auto;
    pl.direct = is_stream(family) || is_guided(family);
    pl.rev_lane_bytes = sw.lane_bytes > 0 ? pl.lane_bytes : 2048;
    pl.direct_ent_lds = stt.ok && stt.ent.size() * 8 <= (size_t)direct_ent_lds_bytes();
    pl.g16_slow = (stt.flags & kFlagG16Slow) != 0;
    pl.g16 = stt.g16_ok && !sw.no_g16 ? (int)(align_up(stt.g16.size() * 4, 16) + stt.p32.size() * 4) : 0;   // LDS room: 16-byte + pair forms
    // memoryless programs in ONE pass (map_block.hpp) — `[aie]:` in 6.2 ms per 8 GiB where the pair takes 7.6, HTML escapes 8.4 against 11.0.
    // A program whose longer texts turn out to be frequent (finish(): the output 4 % longer than the input; `a:xyz` on text: 8.6 ms against 8.0)
    // goes back to the pair for the context's later scans.  TRRE_MAPGEN=1: every memoryless program, always; TRRE_MAPGEN=0: none
    pl.mapgen_on = stt.mg_max != 0 && (sw.mapgen < 0 ? !(stt.mg_max > 1u && cx->mapgen_dense) : sw.mapgen != 0) && !cx->mapgen_off && cx->mapgen_voids < 2;
    pl.sym_mode = !is_guided(family) ? 0 : (guided_sym_bits(*p) == 4 ? 2 : 1);
    if (pl.direct) pl.n_chunks = (args.vend + pl.lane_bytes * direct_block_threads() - 1) / (pl.lane_bytes * direct_block_threads());
    // Exact sub-ranges (round 5): every lane walks the bytes of its sub-range and nothing else, from the state the transducer is in
    // there — what makes a line of 400 KB as parallel as 4 000 lines of 100 bytes (rounds 1-4: a lane owns the lines that START in its
    // sub-range and walks them to their end alone, and the backward pass of the guided families has ONE thread carry the state through
    // a long line: 5.8-9.0 GB/s on such lines; 1 GiB of 400 KB lines now: ' +: ' 6.2 -> 700 GB/s, '(a|b)*c:x' 4.9 -> 520).  On ordinary text the
    // form costs nothing measurable (1 GiB: 745 against 733 GB/s), so the general families always run it — also what keeps ONE giant line in
    // a file of short ones from serialising the scan; TRRE_EXACT=0: the old ownership, for A/B runs.
    pl.use_exact = pl.g16 > 0 && !cx->exact_off && sw.exact != 0 && pl.lane_bytes % 128 == 0 && pl.rev_lane_bytes % 128 == 0 && !is_guided_wide(*p, family);
    return pl;
}

// ---- the routes: each queues its kernels on the stream; kNotThisRoute where a route can decline.  enqueue() has set the arguments every
// family shares and launch_route() where the output size will be; the order of launches, memsets and copies is each route's own.

// tables still being built (lazy_block.hpp): the first round; finish() builds what it missed and runs the next ones
static int route_lazy(trre_prog* p, DeviceState* st, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    return lazy_round(p, st, cx, pl.args, pl.n_chunks, true, stream);
}
// the search itself (gen_block.hpp: bt_lane): a pool of workgroups takes the chunks of 256 sub-ranges in turn, each thread
// with a stack and a path buffer of its own for the whole launch
static int route_backtrack(DeviceState* st, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    const BtTier& tier = kBtTiers[cx->bt_tier];
    const int64_t pool_blocks = pl.n_chunks < tier.pool_blocks ? pl.n_chunks : tier.pool_blocks;
    const uint32_t kBtFrames = tier.frames, kBtPathCap = tier.path_cap;
    const size_t need = (size_t)pool_blocks * 256 * ((size_t)kBtFrames * 16 + kBtPathCap);
    HIP_TRY(cx->d_scratch.reserve(need, need));
    GenArgs ga{};
    ga.stack = reinterpret_cast<uint32_t*>(cx->d_scratch.p);
    ga.path = cx->d_scratch + (size_t)pool_blocks * 256 * kBtFrames * 16;
    ga.frames = kBtFrames;
    ga.path_cap = kBtPathCap;
    pl.args.blob = st->d_nblob;
    const uint32_t budget = (uint32_t)switches().bt_budget.or_else(kBtBudget);
    launch_bt(1, pl.args, ga, kBtLaneBytes, pl.n_chunks, pool_blocks, budget, stream);
    launch_chunk_scan(cx->d_chunk_total, cx->d_chunk_base, pl.n_chunks, stream);
    launch_bt(2, pl.args, ga, kBtLaneBytes, pl.n_chunks, pool_blocks, budget, stream);
    return TRRE_OK;
}
// the positional-window kernel and its redo list
static int route_window(trre_prog* p, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    const int64_t n_lanes = (pl.args.vend + pl.lane_bytes - 1) / pl.lane_bytes;
    HIP_TRY(cx->d_redo.reserve((size_t)n_lanes, (size_t)(n_lanes + 1) * 4));
    HIP_TRY(hipMemsetAsync(cx->d_redo, 0, 4, stream));
    pl.args.redo = cx->d_redo;
    // (TRRE_TRACE=1: the route and the form of the entries launch_lpw_kernel chooses — the pair form is only built for narrow entries and
    // never larger than the kernel's LDS room (stream_pack.cpp) —; finish_inner adds how many lanes the redo pass took)
    if (switches().trace)
        fprintf(stderr, "trre: window kernel: %lld lane(s) of %lld bytes, %s entries\n", (long long)n_lanes, (long long)pl.lane_bytes,
                p->stt.lpw2_ok && !switches().no_lpw_pair ? "pair" : (p->stt.lpw_delay > 3 ? "wide" : "narrow"));
    // (the pair form of the window entries where the tables have it: two input bytes per table read.  TRRE_NO_LPW_PAIR=1: A/B runs)
    launch_lpw_kernel((int)(p->stt.lpw.size() * 4), p->stt.lpw_delay > 3, pl.direct_ent_lds, pl.args, pl.lane_bytes, stream,
                      p->stt.lpw2_ok && !switches().no_lpw_pair ? (int)(p->stt.lpw2.size() * 4) : 0);
    return TRRE_OK;
}
// a backward DFA of more than 256 states: 16-bit symbols, both tables through L1 / L2 (scan_block.hpp: wide guided tables)
static int route_wide_guided(ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    launch_rev_wide(pl.args, pl.lane_bytes, stream);
    launch_wide_fwd(1, pl.args, pl.lane_bytes, pl.n_chunks, stream);
    launch_chunk_scan(cx->d_chunk_total, cx->d_chunk_base, pl.n_chunks, stream);
    launch_wide_fwd(2, pl.args, pl.lane_bytes, pl.n_chunks, stream);
    return TRRE_OK;
}
// length-preserving without a window form: the emit pass alone, every lane writing its lines where it read them
static int route_lp_direct(trre_prog* p, int family, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    if (is_guided(family)) launch_rev_sweep(pl.args, (int)p->gt.n_rev * 256, pl.rev_lane_bytes, stream, pl.sym_mode == 2);
    pl.args.lp_emit = 1;
    launch_direct_kernel(2, pl.direct_ent_lds, pl.args, pl.lane_bytes, pl.n_chunks, stream, pl.g16, pl.sym_mode, pl.g16_slow);
    return TRRE_OK;
}
// A large table (a dictionary) in its copy form (default where the tables have it): the comb walk also lists where the replacement texts
// go, the second pass copies the input around them without walking any table (scan_block.hpp).  TRRE_NO_FB_COPY=1: the count pass + the
// emit pass on the 8-byte rows (route_large_table_pair), for A/B runs and what finish() falls back to (a NUL in the input, more texts in
// a sub-range than its event list holds).
static int route_large_table_copy(trre_prog* p, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    const Switches& sw = switches();
    // (the second pass is the wave-cooperative splice of splice_block.hpp; a table with an escape text longer than its tiles take — more than
    // 255 bytes — or too large for its LDS has no copy form: the pair)
    uint32_t esc_max = 0;
    for (size_t k = 0; k + 3 < p->stt.fb_esc.size(); k += 4) esc_max = std::max(esc_max, p->stt.fb_esc[k + 1]);
    if (sw.no_fb_copy || sw.fb_emit || cx->patch_off || p->copy_form_off.load() || pl.lane_bytes % 64 != 0 || !fb_copy_fits(p->sblob.data()) ||
        esc_max > kSpMaxText || !fb_splice_fits(p->sblob.data()))
        return kNotThisRoute;
    const int64_t n_lanes = pl.n_chunks * direct_block_threads();
    const int64_t ev_rows = (pl.lane_bytes + 2047) / 2048;                  // (the event list grows with the sub-range)
    const size_t rows = (size_t)(n_lanes * ev_rows);                        // (of kCopyEvCap events, 4 bytes each: a lane of more than 2 KiB takes several)
    HIP_TRY(cx->d_cevents.reserve(rows, rows * kCopyEvCap * 4));
    HIP_TRY(cx->d_chdr.reserve(rows, rows * 16));
    FbCopyArgs ca{};
    ca.events = cx->d_cevents;
    ca.lane_hdr = cx->d_chdr;
    ca.ev_cap = kCopyEvCap * (uint32_t)ev_rows;
    launch_fb_mark(pl.args, ca, p->sblob.data(), pl.lane_bytes, pl.n_chunks, stream);
    launch_chunk_scan(cx->d_chunk_total, cx->d_chunk_base, pl.n_chunks, stream);
    launch_fb_splice(pl.args, ca, p->sblob.data(), pl.lane_bytes, pl.n_chunks, stream);
    cx->pend.patched = true;
    return TRRE_OK;
}
// A large table in its fallback form: the count pass with every per-byte lookup in LDS (0.86 ms per GiB against 1.62 on the 8-byte rows
// through L1/L2).  The emit pass over the same form (TRRE_FB_EMIT=1) is correct but slower than the one over the 8-byte rows (3.8 against
// 2.9 ms): its tables leave LDS for only 512 staging rings per CU.  (TRRE_NO_FB=1 — both passes on the 8-byte rows, for A/B runs — is
// route_small_pair.)
static int route_large_table_pair(trre_prog* p, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    const bool fb_emit = switches().fb_emit && fb_fits(p->sblob.data());         // (the form next to 512 staging rings)
    launch_fb_kernel(1, pl.args, p->sblob.data(), pl.lane_bytes, pl.n_chunks, stream);
    launch_chunk_scan(cx->d_chunk_total, cx->d_chunk_base, pl.n_chunks, stream);
    if (fb_emit) launch_fb_kernel(2, pl.args, p->sblob.data(), pl.lane_bytes, pl.n_chunks, stream);
    else launch_direct_kernel(2, pl.direct_ent_lds, pl.args, pl.lane_bytes, pl.n_chunks, stream, 0, pl.sym_mode, pl.g16_slow);
    return TRRE_OK;
}
// ONE walk (round 6; one_block.hpp — SURVEY.md row f2): lanes of 128 bytes from guessed-and-verified states, a workgroup's whole output
// staged in LDS, its place in the output by look-back over the workgroups' totals: the input is read once and walked once.  What the
// kernel cannot answer in place — a lane whose output outgrows its LDS region, a workgroup whose first lane guessed wrong, a replacement
// text of more than 8 bytes, a wrong guess of the backward pass — voids the launch (kStOneVoid) and finish() runs the pair;
// after two such launches the program stops trying.
// MEASURED (profiles/r06_expand_one_*): bit-identical output, 1.05 GiB fetched and 1.06 GiB written per GiB (the pair:
// 2.2 x that) — and HALF the pair's speed (8 GiB of 'a:xyz': 15.7 ms against 7.9): with a workgroup's output held in LDS only three
// waves per SIMD are resident, and the walk is a chain of dependent table reads that wants twice that to hide.  So the pair stays
// the default and this form is opt-in: TRRE_ONE=1.
static int route_one_walk(trre_prog* p, ScanCtx* cx, const trre::StreamTables& stt, const LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    const Switches& sw = switches();
    if (!pl.use_exact || sw.one != 1 || cx->one_off || p->one_fails.load() >= 2 || stt.max_out > 8u) return kNotThisRoute;
    OneArgs oa{};
    oa.lane_bytes = sw.one_lane > 0 ? (uint32_t)((sw.one_lane + 63) / 64 * 64) : 128u;
    oa.region = sw.one_region > 0 ? (uint32_t)(sw.one_region / 8 * 8 + 4) : 172u;          // (an odd number of dwords)
    oa.look = sw.one_look > 0 ? (uint32_t)((sw.one_look + 15) / 16 * 16) : 32u;
    oa.spin = 1u << 20;
    oa.n_tiles = (pl.args.vend + (int64_t)oa.lane_bytes * kOneThreads - 1) / ((int64_t)oa.lane_bytes * kOneThreads);
    const size_t words = (size_t)(oa.n_tiles + 2 + 8 + 2 * (oa.n_tiles / 32 + 1));
    HIP_TRY(cx->d_one.reserve((size_t)oa.n_tiles, words * 8));
    oa.desc = cx->d_one;
    oa.ticket = reinterpret_cast<uint32_t*>(cx->d_one + oa.n_tiles);
    oa.total = cx->d_one + oa.n_tiles + 1;
    oa.gsum = cx->d_one + oa.n_tiles + 2 + 8;
    oa.ginc = oa.gsum + (oa.n_tiles / 32 + 1);
    HIP_TRY(hipMemsetAsync(cx->d_one, 0, words * 8, stream));
    oa.prof = sw.one_prof ? cx->d_one + oa.n_tiles + 2 : nullptr;
    ScanArgs wa = pl.args;
    wa.spec_look = oa.look;                            // (the forward lanes' look-back; the backward pass kept kSpecLook)
    if (launch_one(wa, oa, stream, (int)align_up(stt.g16.size() * 4, 16), pl.sym_mode, pl.g16_slow) != 0) return kNotThisRoute;      // (the 16-byte form alone: no pair form in LDS)
    cx->pend.total_at = oa.total;
    cx->pend.one = true;
    return TRRE_OK;
}
// the count / emit pair of the direct walkers, on exact sub-ranges where the tables have the 16-byte form — or, before it, the one walk
static int route_small_pair(trre_prog* p, ScanCtx* cx, int family, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    ScanArgs& args = pl.args;
    const int64_t rev_lanes = ((((args.vend + 127) & ~(int64_t)127) + pl.rev_lane_bytes - 1) / pl.rev_lane_bytes + 255) / 256 * 256;
    if (pl.use_exact) {
        const int64_t n_lanes = pl.n_chunks * direct_block_threads();
        const int64_t want = 3 * n_lanes + (is_guided(family) ? 2 * rev_lanes : 0);
        HIP_TRY(cx->d_spec.reserve((size_t)want, (size_t)want * 4));
        args.entry_rows = cx->d_spec;
        args.exit_rows = cx->d_spec + n_lanes;
        args.spec_flags = cx->d_spec + 2 * n_lanes;
        args.rev_guess = cx->d_spec + 3 * n_lanes;
        args.rev_flags = cx->d_spec + 3 * n_lanes + rev_lanes;
        args.exact = 1;
        args.spec_look = (uint32_t)kSpecLook;
    }
    if (is_guided(family)) {
        launch_rev_sweep(args, (int)p->gt.n_rev * 256, pl.rev_lane_bytes, stream, pl.sym_mode == 2);
        if (pl.use_exact) launch_rev_verify(args, pl.rev_lane_bytes, stream, pl.sym_mode == 2);
    }
    const int rc = route_one_walk(p, cx, walked_tables(p, family), pl, stream);
    if (rc != kNotThisRoute) return rc;
    // (Rounds 3 and 4 had two one-walk forms here — record + patch, and mark + splice for small tables; both lost to this pair and were removed
    // in round 5: DESIGN.md §4.5.)
    launch_direct_kernel(1, pl.direct_ent_lds, args, pl.lane_bytes, pl.n_chunks, stream, pl.g16, pl.sym_mode, pl.g16_slow);
    if (pl.use_exact) launch_spec_verify(args, (args.vend + pl.lane_bytes - 1) / pl.lane_bytes, stream);
    launch_chunk_scan(cx->d_chunk_total, cx->d_chunk_base, pl.n_chunks, stream);
    if (pl.use_exact) args.exact = 2;
    launch_direct_kernel(2, pl.direct_ent_lds, args, pl.lane_bytes, pl.n_chunks, stream, pl.g16, pl.sym_mode, pl.g16_slow);
    cx->pend.exact = pl.use_exact;
    return TRRE_OK;
}
// the general stream and guided families: the first of their routes that takes the launch
static int route_direct_general(trre_prog* p, ScanCtx* cx, int family, LaunchPlan& pl, hipStream_t stream) {
    const trre::StreamTables& stt = walked_tables(p, family);
    // a MEMORYLESS program (map_block.hpp; round 6): no state, so no walk — lengths, a prefix sum with look-back, the bytes' texts
    // at their places: ONE pass, one read of the input.  A NUL voids it (finish()).
    if (family == TRRE_KERNEL_STREAM_GEN && pl.mapgen_on && mapgen_launch(cx, pl.args, stt, stream, cx->pend) == TRRE_OK) return TRRE_OK;
    if (!is_guided(family) && stt.fb_ok && !trre::switches().no_fb) {
        const int rc = route_large_table_copy(p, cx, pl, stream);
        return rc != kNotThisRoute ? rc : route_large_table_pair(p, cx, pl, stream);
    }
    return route_small_pair(p, cx, family, pl, stream);
}
// the bitmask tile kernels (fallback of last resort)
static int route_tile_pair(trre_prog* p, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    launch_tile_kernel(1, p->engine, p->mask_bytes, pl.args, pl.n_chunks, stream);
    launch_chunk_scan(cx->d_chunk_total, cx->d_chunk_base, pl.n_chunks, stream);
    launch_tile_kernel(2, p->engine, p->mask_bytes, pl.args, pl.n_chunks, stream);
    return TRRE_OK;
}

static int launch_route(trre_prog* p, DeviceState* st, ScanCtx* cx, int family, LaunchPlan& pl, hipStream_t stream) {
    if (is_gen(family)) cx->pend.total_at = cx->d_chunk_base + pl.n_chunks;      // (count, exclusive sum, emit: the sum's last word; the one-pass kernels have their own)
    if (family == TRRE_KERNEL_DFT_LAZY) return route_lazy(p, st, cx, pl, stream);
    if (family == TRRE_KERNEL_BACKTRACK) return route_backtrack(st, cx, pl, stream);
    if (family == TRRE_KERNEL_BYTEMAP) { pl.args.nul_list = cx->d_status + 4; trre::launch_bytemap(pl.args, stream); return TRRE_OK; }
    if (family == TRRE_KERNEL_TILE_LP) { trre::launch_tile_kernel(0, p->engine, p->mask_bytes, pl.args, pl.n_chunks, stream); return TRRE_OK; }
    if (pl.window) return route_window(p, cx, pl, stream);
    if (is_guided(family) && p->gt.wide) return route_wide_guided(cx, pl, stream);
    if (pl.direct && !is_gen(family)) return route_lp_direct(p, family, pl, stream);
    if (pl.direct) return route_direct_general(p, cx, family, pl, stream);
    return route_tile_pair(p, cx, pl, stream);
}

int enqueue(trre_prog* p, DeviceState* st, ScanCtx* cx, int family, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap,
            hipStream_t stream) {
    Pending& pd = cx->pend;
    // Back-to-back enqueues without a finish() in between form one batch: status bits accumulate, the
    // timing events bracket the whole batch and finish() speaks for the last launch — so every launch of
    // a batch must be the same scan (benchmark loops); anything else has to be finished first.
    const bool batch = pd.active && pd.launched;
    if (pd.active && (pd.asked != family || pd.user_in != d_in || pd.d_out != d_out || pd.n != n || pd.cap != cap || pd.stream != stream))
        return fail(TRRE_E_ARG, "error: a different scan is still in flight on this device: call trre_scan_finish first");
    const int batch_count = batch ? pd.count : 0;
    const uint8_t* const user_in = d_in;
    // In place (d_in == d_out): the kernels write where they read, and neither a family whose output moves (count / emit, the one-pass
    // kernels, the lazy and backtracking lanes) nor a relaunch in finish() (a NUL, an overflow, a mask scratch) could read the input
    // again.  So the scan reads a copy, at the same offset mod 16 (the window kernel's stores stay aligned); the launches of a batch
    // read the copy the first one made — the caller's buffer holds their output by then.
    const bool aliased = n && d_in == d_out;
    if (aliased) {
        const size_t a0 = reinterpret_cast<uintptr_t>(d_in) & 15u;
        if (!batch) {
            HIP_TRY(cx->d_snap.reserve(n + 16, n + 16));
            HIP_TRY(hipMemcpyAsync(cx->d_snap + a0, d_in, n, hipMemcpyDeviceToDevice, stream));
        }
        d_in = cx->d_snap + a0;
    }
    pd = Pending();
    pd.active = true;
    pd.count = batch_count;
    pd.family = family; pd.asked = family;
    pd.d_in = d_in; pd.d_out = d_out; pd.n = n; pd.cap = cap; pd.stream = stream;
    pd.user_in = user_in; pd.aliased = aliased;
    if (n == 0) return TRRE_OK;
    int rc = long_line_switch(p, cx, &family, d_in, n, cap, stream);
    if (rc) return rc;
    pd.family = family;
    if (family == TRRE_KERNEL_DFT_LAZY) { rc = lazy_ensure(p); if (rc) return rc; }
    LaunchPlan pl = make_plan(p, st, cx, family, d_in, n, d_out, cap);
    if (!is_gen(family) && cap < n) return TRRE_OK;   // finish() reports the capacity error
    if (is_gen(family)) {
        rc = ensure_workspace(cx, pl.n_chunks, pl.direct ? trre::direct_block_threads() : pl.threads);
        if (rc) return rc;
        pl.args.lane_counts = cx->d_lane_counts;
        pl.args.chunk_total = cx->d_chunk_total;
        pl.args.chunk_base = cx->d_chunk_base;
    }
    if (is_guided(family)) {
        // one symbol per input byte, written by the backward pass (whole 64-byte pieces) and read by the forward pass
        const size_t need = ((size_t)((pl.args.vend + 63) & ~(int64_t)63) + 256) * (p->gt.wide ? 2 : 1);
        HIP_TRY(cx->d_sym.reserve(need, need));
        pl.args.rblob = st->d_rblob;
        pl.args.sym_v0 = cx->d_sym;
    }
    if (!batch) {
        HIP_TRY(hipMemsetAsync(cx->d_status, 0, 24, stream));          // (status words and the NUL count)
        if (p->profiling) HIP_TRY(hipEventRecord(cx->ev0, stream));
    }
    pd.timed = p->profiling;
    rc = launch_route(p, st, cx, family, pl, stream);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    // (the status word, the output size and the closing timing event are fetched by finish(): nothing
    // sits between the kernels of back-to-back launches)
    pd.plan = pl;
    pd.launched = true;
    pd.count += 1;
    return TRRE_OK;
}

// A byte map's launch met NUL bytes: a NUL cuts its line short (Q2) — the bytes before it are mapped, a '\n' stands at its
// position, the rest of the record is gone — so everything behind it moves up.  The kernel listed the NULs; the lines'
// ends are looked up, and the stretches between the cuts are mapped again from the input to where they belong (the
// first one is in place already).  Returns TRRE_OK with *out_len, an error, or -1: not a case for this (more NULs than the
// list holds, more than 256 cut lines) — the caller runs the buffer through the general family.
static int repair_bytemap_nuls(DeviceState* st, ScanCtx* cx, const Pending& was, size_t* out_len) {
    using namespace trre;
    if (switches().no_nul_repair) return -1;
    uint32_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, cx->d_status + 4, 4, hipMemcpyDeviceToHost, was.stream));
    HIP_TRY(hipStreamSynchronize(was.stream));
    if (count == 0 || count > kNulCap) return -1;
    uint64_t* d_pos = reinterpret_cast<uint64_t*>(cx->d_status + 6);
    uint64_t* d_eol = d_pos + kNulCap;
    launch_nul_eol(was.d_in, (int64_t)was.n, d_pos, d_eol, count, was.stream);
    std::vector<uint64_t> pos(count), eol(count);
    HIP_TRY(hipMemcpyAsync(pos.data(), d_pos, (size_t)count * 8, hipMemcpyDeviceToHost, was.stream));
    HIP_TRY(hipMemcpyAsync(eol.data(), d_eol, (size_t)count * 8, hipMemcpyDeviceToHost, was.stream));
    HIP_TRY(hipStreamSynchronize(was.stream));
    std::vector<std::pair<uint64_t, uint64_t>> cuts;          // (the NUL, the end of its line): the first NUL of every line
    {
        std::vector<std::pair<uint64_t, uint64_t>> all(count);
        for (uint32_t i = 0; i < count; ++i) {
            if (eol[i] == ~0ull) return -1;                   // (a line of many megabytes behind a NUL)
            all[i] = {pos[i], eol[i]};
        }
        std::sort(all.begin(), all.end());
        bool any = false;
        uint64_t done_to = 0;
        for (const auto& c : all) {
            if (any && c.first <= done_to) continue;
            cuts.push_back(c);
            done_to = c.second;
            any = true;
        }
    }
    if (cuts.size() > 256) return -1;
    const uint8_t* blob = st->d_blob;
    // stretch by stretch: input [s, the next NUL) mapped to s - shift, then a '\n'; the last one ends at the last byte of
    // the input, which is a terminator whatever it holds (Q1)
    uint64_t s = 0, shift = 0;
    const uint64_t last_byte = (uint64_t)was.n - 1;
    for (size_t j = 0; j < cuts.size(); ++j) {
        const uint64_t nul = cuts[j].first;
        if (j == 0) launch_bytemap_shift(blob, was.d_in + nul, was.d_out + nul, 0, true, was.stream);       // (in place already: only its '\n')
        else launch_bytemap_shift(blob, was.d_in + s, was.d_out + (s - shift), (int64_t)(nul - s), true, was.stream);
        shift += cuts[j].second - nul;
        s = cuts[j].second + 1;
    }
    if (s <= last_byte) launch_bytemap_shift(blob, was.d_in + s, was.d_out + (s - shift), (int64_t)(last_byte - s), true, was.stream);
    HIP_TRY(hipStreamSynchronize(was.stream));
    cx->relaunches += 1;
    if (out_len) *out_len = (size_t)((uint64_t)was.n - shift);
    return TRRE_OK;
}

// ---- finish(): what a launch left behind, outcome by outcome.  The scan that is being finished, as the outcomes hand it round:
struct Finishing { trre_prog* p; DeviceState* st; ScanCtx* cx; const Pending& was; size_t* out_len; };
constexpr int kGoOn = 1;                      // an outcome has nothing to return yet (positive: no TRRE_E_* code): finish_inner goes on down its list
static int finish_inner(trre_prog* p, DeviceState* st, ScanCtx* cx, size_t* out_len);

// the status word and the output size come down; the stream is idle afterwards
static int fetch_status(ScanCtx* cx, const Pending& was, uint32_t* status) {
    HIP_TRY(hipMemcpyAsync(cx->h_status, cx->d_status, 8, hipMemcpyDeviceToHost, was.stream));
    if (was.total_at) HIP_TRY(hipMemcpyAsync(cx->h_status + 2, was.total_at, 8, hipMemcpyDeviceToHost, was.stream));
    HIP_TRY(hipStreamSynchronize(was.stream));
    *status = cx->h_status[0];
    return TRRE_OK;
}

// The same scan again — as `family`, over the first n bytes — with one route switched off (`off`, a flag of the context; null: none): counted
// as a relaunch, enqueued, finished, the flag restored on every path.  hold false: the flag covers the enqueue alone, and whatever the
// finish has to run again sees it cleared (the exact sub-ranges: a rerun of the rerun tries them afresh).
static int rerun(const Finishing& f, int family, bool ScanCtx::*off = nullptr, bool hold = true, size_t n = ~(size_t)0) {
    ScanCtx* cx = f.cx;
    if (off) cx->*off = true;
    cx->relaunches += 1;
    int rc = enqueue(f.p, f.st, cx, family, f.was.d_in, n == ~(size_t)0 ? f.was.n : n, f.was.d_out, f.was.cap, f.was.stream);
    if (off && !hold) cx->*off = false;
    if (!rc) rc = finish_inner(f.p, f.st, cx, f.out_len);
    if (off) cx->*off = false;
    return rc;
}

// Rounds of the lazy family (lazy_block.hpp): the edges the launch listed are built on the host (trre_dft.c:1135-1175: nft_step, truncate_lcp,
// the lookup, the finality probe), the new rows go up, the lanes that were void walk again.  Every round explores at least one edge
// of a finite table over a finite input, so this ends — with the answer, or with the memory limit of the tables.
static int lazy_rounds(const Finishing& f, uint32_t* status_io) {
    using namespace trre;
    trre_prog* p = f.p; ScanCtx* cx = f.cx; const Pending& was = f.was; size_t* out_len = f.out_len;
    uint32_t status = *status_io;
    ScanArgs args = base_args(was.d_in, was.n, was.d_out);
    args.status = cx->d_status;
    args.cap = was.cap;
    args.lane_counts = cx->d_lane_counts;
    args.chunk_total = cx->d_chunk_total;
    args.chunk_base = cx->d_chunk_base;
    std::vector<uint32_t> miss;
    size_t spec = 1024;
    int empty_rounds = 0;
    for (int round = 1; (status & kStMiss) && !(status & (kStEditOverflow | kStDiverge)); ++round) {
        uint32_t head[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(head, cx->d_miss, 8, hipMemcpyDeviceToHost, was.stream));
        HIP_TRY(hipStreamSynchronize(was.stream));
        const uint32_t n_miss = head[0] < kLazyMissCap ? head[0] : kLazyMissCap;
        // a void lane lists the edge it stopped at unless this very launch has listed it (or the list was full: then it holds other
        // edges), so a round with a miss and an empty list cannot be — if it is, the device's rows go up afresh, and the scan gives up
        // rather than spin
        if (!n_miss) {
            if (++empty_rounds > 3) return fail_empty(out_len, TRRE_E_DEVICE, "error: the lazy tables make no progress (a miss with nothing listed, four rounds running)");
            std::lock_guard<std::mutex> lock(p->lazy_mu);
            f.st->lazy_rows_up = 0;
        } else {
            empty_rounds = 0;
        }
        miss.resize((size_t)trre::kLazyMissWords * n_miss + 2);
        if (n_miss) HIP_TRY(hipMemcpyAsync(miss.data(), cx->d_miss + 2, (size_t)n_miss * trre::kLazyMissWords * 4, hipMemcpyDeviceToHost, was.stream));
        HIP_TRY(hipStreamSynchronize(was.stream));
        try {
            std::lock_guard<std::mutex> lock(p->lazy_mu);
            p->lazy->explore(miss.data(), n_miss, spec);
        } catch (const trre::Error& e) {
            return fail_empty(out_len, e.code, e.what());
        } catch (const std::bad_alloc&) {
            return fail_empty(out_len, TRRE_E_TOO_BIG, "error: out of memory while determinising");
        }
        if (switches().trace) fprintf(stderr, "trre: lazy round %d: %u misses, %u rows, %u states\n", round, n_miss, p->lazy->n_rows(), p->lazy->n_states());
        // the automatic choice for a pattern that also has its eager tables: a scan that is still growing the lazy ones after kLazyAutoRounds
        // goes to the tile kernels (the next scan finds the tables that much further)
        constexpr int kLazyAutoRounds = 64;
        if (round >= kLazyAutoRounds && !p->forced_family && !p->lazy_only && p->has_engine_tables) return rerun(f, TRRE_KERNEL_TILE_GEN);
        if (spec < (1u << 16)) spec *= 2;                      // (the deeper the input digs, the further ahead the host looks)
        HIP_TRY(hipMemsetAsync(cx->d_status, 0, 8, was.stream));
        cx->relaunches += 1;
        int rc = lazy_round(p, f.st, cx, args, was.plan.n_chunks, false, was.stream);
        if (!rc) rc = fetch_status(cx, was, &status);
        if (rc) return rc;
    }
    *status_io = status;
    // (an edge whose closure runs round an epsilon cycle: the reference dies there with its output unflushed)
    if (status & kStDiverge) return fail_empty(out_len, TRRE_E_DIVERGES, kDivergeMsg);
    if (status & kStEditOverflow)
        return fail_empty(out_len, TRRE_E_UNSUPPORTED, "error: a sub-range of 1 KiB takes more than 2^32 table steps (TRRE_LAZY_BUDGET): lines of megabytes with an attempt per byte");
    return kGoOn;
}

// exact sub-ranges, every entry state verified: the sizes are final — the exclusive sum and the emit pass again, counted as a relaunch
static int exact_emit_again(const Finishing& f, trre::ScanArgs& xa) {
    const LaunchPlan& pl = f.was.plan;
    trre::launch_chunk_scan(f.cx->d_chunk_total, f.cx->d_chunk_base, pl.n_chunks, f.was.stream);
    xa.exact = 2;
    trre::launch_direct_kernel(2, pl.direct_ent_lds, xa, pl.lane_bytes, pl.n_chunks, f.was.stream, pl.g16, pl.sym_mode, pl.g16_slow);
    HIP_TRY(hipGetLastError());
    f.cx->relaunches += 1;
    return TRRE_OK;
}

// exact sub-ranges, the backward pass guessed wrong somewhere: its flagged lanes sweep again (and on to the left while what they arrive with is
// not what was assumed there) until every guess is what the lane to the right found; then the forward passes run — they had left at once
static int exact_repair_backward(const Finishing& f, uint32_t rev_misses, uint32_t* misses, uint32_t* status) {
    using namespace trre;
    ScanCtx* cx = f.cx; const Pending& was = f.was; const LaunchPlan& pl = was.plan;
    ScanArgs xa = pl.args;
    for (int64_t round = 0; rev_misses; ++round) {
        if (switches().trace) fprintf(stderr, "trre: exact sub-ranges, backward pass: round %lld, %u lane(s) to repair\n", (long long)round, rev_misses);
        HIP_TRY(hipMemsetAsync(cx->d_status + 2, 0, 4, was.stream));
        launch_rev_repair(xa, pl.rev_lane_bytes, was.stream, pl.sym_mode == 2);
        launch_rev_verify(xa, pl.rev_lane_bytes, was.stream, pl.sym_mode == 2);
        HIP_TRY(hipMemcpyAsync(&rev_misses, cx->d_status + 2, 4, hipMemcpyDeviceToHost, was.stream));
        HIP_TRY(hipStreamSynchronize(was.stream));
    }
    HIP_TRY(hipMemsetAsync(cx->d_status, 0, 16, was.stream));
    xa.exact = 1;
    launch_direct_kernel(1, pl.direct_ent_lds, xa, pl.lane_bytes, pl.n_chunks, was.stream, pl.g16, pl.sym_mode, pl.g16_slow);
    launch_spec_verify(xa, (xa.vend + pl.lane_bytes - 1) / pl.lane_bytes, was.stream);
    const int rc = exact_emit_again(f, xa);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(misses, cx->d_status + 3, 4, hipMemcpyDeviceToHost, was.stream));
    return fetch_status(cx, was, status);
}

// exact sub-ranges: lanes whose guessed entry state was not the exit state of the lane before them walk again (and on, while
// their exit keeps differing from what the next lane assumed), until k_spec_verify finds none; then the sizes are final
static int exact_repair(const Finishing& f, uint32_t* status) {
    using namespace trre;
    ScanCtx* cx = f.cx; const Pending& was = f.was; const LaunchPlan& pl = was.plan;
    uint32_t both[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(both, cx->d_status + 2, 8, hipMemcpyDeviceToHost, was.stream));
    HIP_TRY(hipStreamSynchronize(was.stream));
    uint32_t misses = both[1];
    if (both[0] && is_guided(was.family)) {
        const int rc = exact_repair_backward(f, both[0], &misses, status);
        if (rc) return rc;
    }
    if (!misses || (*status & (kStOverflow | kStDiverge))) return kGoOn;
    ScanArgs xa = pl.args;
    const int64_t n_lanes = (xa.vend + pl.lane_bytes - 1) / pl.lane_bytes;
    for (int64_t round = 0; misses; ++round) {
        if (switches().trace) fprintf(stderr, "trre: exact sub-ranges: round %lld, %u lane(s) to repair\n", (long long)round, misses);
        // A round settles a workgroup where ONE lane of it is flagged (the parity of `aa:x` in a run of `a`: the lanes behind the flagged one agree
        // with each other and the walk passes through them).  Where flagged lanes are neighbours — `aaa:xy` in such a run: two lanes in three —
        // a flagged lane ends the walk of the one before it and starts from an exit that is being rewritten: a round settles ONE lane, and a run
        // over more than n_chunks + 64 lanes ends here, scanned again the old way (tests/test_gpu_exact_repair.py: long_run_aaa_dft).  To do:
        // let a flagged lane walk on through flagged lanes — it knows their true entry.
        if (round > pl.n_chunks + 64)
            return rerun(f, was.family, &ScanCtx::exact_off, false);
        HIP_TRY(hipMemsetAsync(cx->d_status + 3, 0, 4, was.stream));
        xa.exact = 3;
        launch_direct_kernel(1, pl.direct_ent_lds, xa, pl.lane_bytes, pl.n_chunks, was.stream, pl.g16, pl.sym_mode, pl.g16_slow);
        launch_spec_verify(xa, n_lanes, was.stream);
        HIP_TRY(hipMemcpyAsync(&misses, cx->d_status + 3, 4, hipMemcpyDeviceToHost, was.stream));
        HIP_TRY(hipStreamSynchronize(was.stream));
    }
    int rc = exact_emit_again(f, xa);
    if (!rc) rc = fetch_status(cx, was, status);
    return rc ? rc : kGoOn;
}

// the one-pass kernels' phase clocks (TRRE_ONE_PROF, TRRE_MAPGEN_PROF) on stderr, the memoryless kernel's tiles (TRRE_MAPGEN_DBG) to their file
static int profile_dumps(ScanCtx* cx, const Pending& was) {
    const trre::Switches& sw = trre::switches();
    uint64_t pr[8] = {};
    if ((was.one && sw.one_prof) || (was.mapgen && sw.mapgen_prof)) HIP_TRY(hipMemcpy(pr, was.total_at + 1, sizeof(pr), hipMemcpyDeviceToHost));
    const double t = pr[7] ? (double)pr[7] : 1.0;
    if (was.one && sw.one_prof)
        fprintf(stderr, "trre: one-pass phases, shader clocks per tile (%llu tiles): ticket %.0f  walk %.0f  verify %.0f  sizes %.0f  look-back %.0f  store %.0f\n",
                (unsigned long long)pr[7], pr[0] / t, pr[1] / t, pr[2] / t, pr[3] / t, pr[4] / t, pr[5] / t);
    if (was.mapgen && sw.mapgen_prof)
        fprintf(stderr, "trre: memoryless kernel, shader clocks per trip (%llu trips): look-back %.0f  expand %.0f  next tile counted %.0f  store %.0f  barrier %.0f\n",
                (unsigned long long)pr[7], pr[1] / t, pr[2] / t, pr[3] / t, pr[4] / t, pr[5] / t);
    if (was.mapgen && sw.mapgen_dbg) {
        std::vector<uint64_t> d(16 * cx->d_mg.cap);
        HIP_TRY(hipMemcpy(d.data(), was.total_at + 1 + 8, d.size() * 8, hipMemcpyDeviceToHost));
        if (FILE* f = fopen(sw.mapgen_dbg, "wb")) { fwrite(d.data(), 8, d.size(), f); fclose(f); }
    }
    return kGoOn;
}

// A scan that met an attempt which does not return.  The NFT binary exits with everything it had printed so far (exit() flushes stdout):
// the lines before the bad one and the bad line's output up to the attempt that does not return.  The guided tables stop a lane exactly
// there (guided_build.cpp), the count pass names the first such lane in stream order and knows every lane's size: the output up to that
// point is in the buffer and its length is reported with the error.  (The DFT binary dies of unbounded recursion, its buffered output is
// lost: nothing to reproduce, *out_len = 0.)
static int report_divergence(const Finishing& f) {
    trre_prog* p = f.p; ScanCtx* cx = f.cx; const Pending& was = f.was; size_t* out_len = f.out_len;
    if (out_len) *out_len = 0;
    const bool knows_lane = (was.family == TRRE_KERNEL_GUIDED_GEN && !was.patched) || was.family == TRRE_KERNEL_BACKTRACK;
    if (p->engine != TRRE_ENGINE_NFT || (!p->gt.ok && !p->bt_ok)) return fail(TRRE_E_DIVERGES, kDivergeMsg);
    if (!knows_lane) {
        // (the count / emit pair knows every lane's size; the rerun comes back here through the branch below)
        const int rc = rerun(f, p->gt.ok ? TRRE_KERNEL_GUIDED_GEN : TRRE_KERNEL_BACKTRACK, &ScanCtx::patch_off);
        return rc == TRRE_OK ? fail(TRRE_E_DEVICE, "error: a diverging scan did not diverge when it was run again") : rc;
    }
    const uint32_t lane = 0xffffffffu - cx->h_status[1];
    const int64_t chunk = (int64_t)lane / 256;             // (workspace chunks are 256 lanes: ensure_workspace)
    std::vector<uint32_t> counts(256);
    uint64_t base = 0, chunk_total = 0;
    HIP_TRY(hipMemcpyAsync(counts.data(), cx->d_lane_counts + chunk * 256, 256 * 4, hipMemcpyDeviceToHost, was.stream));
    HIP_TRY(hipMemcpyAsync(&base, cx->d_chunk_base + chunk, 8, hipMemcpyDeviceToHost, was.stream));
    HIP_TRY(hipMemcpyAsync(&chunk_total, cx->d_chunk_total + chunk, 8, hipMemcpyDeviceToHost, was.stream));
    HIP_TRY(hipStreamSynchronize(was.stream));
    uint64_t upto = base;
    for (uint32_t k = 0; k <= lane % 256; ++k) upto += counts[k];
    if (base + chunk_total > was.cap) {                    // the emit pass skipped this chunk: ask for room, the retry reports
        if (out_len) *out_len = (size_t)(base + chunk_total);
        return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    }
    if (out_len) *out_len = (size_t)upto;
    return fail(TRRE_E_DIVERGES, kDivergeMsg);
}

// The backtracking fallback ran into a limit.  Which one: an attempt deeper than a lane's stack or with more output than its path buffer
// runs again with fewer, larger ones; the step budget is final (the reference's search is exponential here too)
static int backtrack_retry(const Finishing& f) {
    ScanCtx* cx = f.cx;
    uint32_t why = 0;
    HIP_TRY(hipMemcpyAsync(&why, cx->d_status + 2, 4, hipMemcpyDeviceToHost, f.was.stream));
    HIP_TRY(hipStreamSynchronize(f.was.stream));
    if (!(why & trre::kBtWhyBudget) && cx->bt_tier < kBtTierCount - 1) {
        const int tier = cx->bt_tier;
        cx->bt_tier = tier + 1;
        const int rc = rerun(f, f.was.family);
        cx->bt_tier = tier;
        return rc;
    }
    return fail_empty(f.out_len, TRRE_E_UNSUPPORTED, (why & trre::kBtWhyBudget) ? "error: the search takes more than 16 M steps in 1 KiB of this input (TRRE_BT_BUDGET; the backtracking fallback)"
                                                                : "error: an attempt of the search consumes more than 1 M bytes or prints more than 1 MiB (the backtracking fallback)");
}

// One-pass launches that were void, and what a good one of the memoryless kernel says about the corpus.
static int one_pass_outcome(const Finishing& f, uint32_t status) {
    using namespace trre;
    ScanCtx* cx = f.cx; const Pending& was = f.was;
    if (was.mapgen && (status & (kStNul | kStOneVoid))) {
        // a NUL cuts its record short — the rest of the record is swallowed: state after all — (or a look-back that gave up: a workgroup of
        // the grid was not resident — another process on the device —, tests: TRRE_MAPGEN_OVERSUB): the general small-table family takes the buffer
        if (switches().trace) fprintf(stderr, "trre: a one-pass launch of the memoryless kernel was void: status 0x%x\n", status);
        cx->mapgen_voids += 1;
        return rerun(f, was.family, &ScanCtx::mapgen_off);
    }
    if (was.mapgen) {
        // (the longer texts are frequent in what this context scans: see make_plan())
        uint64_t m = 0;
        std::memcpy(&m, cx->h_status + 2, 8);
        if (m > (uint64_t)was.n + (uint64_t)was.n / 25) cx->mapgen_dense = true;
    }
    if (was.one && (status & kStOneVoid)) {
        // the one-pass kernel could not answer (one_block.hpp: what voids it): the count / emit pair takes the buffer — and, the corpus being
        // what it is, after two such launches the program's later scans too
        if (switches().trace) fprintf(stderr, "trre: a one-pass launch of family %d was void: status 0x%x\n", was.family, status);
        f.p->one_fails.fetch_add(1);
        return rerun(f, was.family, &ScanCtx::one_off);
    }
    return kGoOn;
}

// The outcomes of a launch in the order they are believed — the order matters: a length-preserving launch that met a NUL, say, is void
// before its divergence bit is looked at.
static int finish_inner(trre_prog* p, DeviceState* st, ScanCtx* cx, size_t* out_len) {
    using namespace trre;
    Pending& pd = cx->pend;
    if (!pd.active) return fail(TRRE_E_ARG, "error: no scan in flight");
    const Pending was = pd;
    pd = Pending();
    if (was.n == 0) { if (out_len) *out_len = 0; return TRRE_OK; }
    if (!was.launched) {                                 // length-preserving family, buffer too small
        if (out_len) *out_len = was.n;
        return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    }
    const Finishing f{p, st, cx, was, out_len};
    uint32_t status = 0;
    if (was.timed) HIP_TRY(hipEventRecord(cx->ev1, was.stream));
    int rc = fetch_status(cx, was, &status);
    if (rc) return rc;
    if (was.timed) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, cx->ev0, cx->ev1));
        p->last_ms = ms / (float)(was.count > 0 ? was.count : 1);   // average per launch of the batch
    }
    if (switches().trace && was.launched && was.plan.window) {
        // (the stream is idle: the redo list is the last launch's.  One 4-byte copy, only when tracing)
        uint32_t redone = 0;
        HIP_TRY(hipMemcpy(&redone, cx->d_redo, 4, hipMemcpyDeviceToHost));
        fprintf(stderr, "trre: window kernel: %u lane(s) redone, status 0x%x\n", redone, status);
    }
    rc = was.family == TRRE_KERNEL_DFT_LAZY ? lazy_rounds(f, &status) : kGoOn;
    if (rc == kGoOn && was.exact && !(status & (kStOverflow | kStDiverge))) rc = exact_repair(f, &status);
    if (rc == kGoOn) rc = profile_dumps(cx, was);
    if (rc == kGoOn) rc = one_pass_outcome(f, status);
    if (rc != kGoOn) return rc;
    // an attempt that does not return: the lane bookkeeping of the error path (the first such lane in stream order, the sizes of the lanes
    // before it) is that of lanes that own lines — the same scan again, the old way
    if ((was.exact || was.one) && (status & kStDiverge)) return rerun(f, was.family, &ScanCtx::exact_off, false);
    // (a length-preserving launch that met a NUL is void — it went on walking behind the NUL, where the reference never
    // looks — and so is whatever else it reports: the general family decides, below)
    const bool void_by_nul = !is_gen(was.family) && (status & kStNul);
    if ((status & kStDiverge) && !void_by_nul) return report_divergence(f);
    if (was.family == TRRE_KERNEL_BACKTRACK && (status & kStEditOverflow)) return backtrack_retry(f);
    if (status & kStNeedScratch) {
        // a line longer than the LDS tile met the non-deterministic engine: give it
        // a mask scratch (one mask per input byte) and run again
        const size_t need = (was.n + 32) * (size_t)p->mask_bytes;
        HIP_TRY(cx->d_scratch.reserve(need, need));
        return rerun(f, was.family);
    }
    // (why a launch was void, on stderr)
    if (switches().trace && was.patched && (status & (kStEditOverflow | kStNul | kStOverflow | kStDiverge)))
        fprintf(stderr, "trre: a mark + splice launch of family %d was void: status 0x%x\n", was.family, status);
    if (was.patched && (status & (kStEditOverflow | kStNul))) {
        // copy
        // form of a large table: more texts in a sub-range (or in 64 bytes of it) than its event list holds, or a NUL byte —
        // the count / emit pair
        if (status & kStEditOverflow) p->copy_form_off.store(true);      // (a property of the dictionary and its corpus: do not try again)
        return rerun(f, was.family, &ScanCtx::patch_off);
    }
    // an undecided attempt outgrew the stream table (bounded fold): the guided (or the tile) kernels take the buffer — this one
    // and, the corpus being what it is, the ones after it (the count pass found out; the emit pass saw the mark and left at once)
    if (is_stream(was.family) && (status & kStOverflow)) {
        p->bounded_off.store(true);
        return rerun(f, general_family(*p, false));
    }
    if (!is_gen(was.family)) {
        // a NUL cuts its line short, so output positions no longer equal input positions: redo with a general family
        if ((status & kStNul) && was.family == TRRE_KERNEL_BYTEMAP) {
            rc = repair_bytemap_nuls(st, cx, was, out_len);
            if (rc >= 0) return rc;
        }
        // (the same repair for the other length-preserving families — the NULs looked up by a pass over the input, the stretches
        // scanned again by the window kernel with unaligned stores — was built and measured in round 4: 13.5 ms for 8 GiB with a
        // NUL per GiB against 12.9 ms for the general family over the whole buffer; not kept.  DESIGN.md §5)
        if (status & kStNul) return rerun(f, general_family(*p, !is_guided(was.family)));
        if (out_len) *out_len = was.n;
        return TRRE_OK;
    }
    uint64_t total;
    std::memcpy(&total, cx->h_status + 2, 8);
    if (out_len) *out_len = (size_t)total;
    if ((status & kStCapacity) || total > was.cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    return TRRE_OK;
}

// finish_inner, then the stack guard: a scan that went through may have met a line on which the reference's search runs out of
// stack (guard_block.hpp) — then the answer is what the reference gives: an error, and the output up to the attempt that
// overflowed (the lines before that line from a scan of exactly those lines, the line's own part from the guard's search).
static int finish_guarded(trre_prog* p, DeviceState* st, ScanCtx* cx, size_t* out_len) {
    using namespace trre;
    const Pending was = cx->pend;
    // the long-line probe's verdict holds for the batch it was asked in (identical launches); the caller may put other bytes into the same
    // buffer afterwards — the host path's slots do for every chunk — so the next batch asks again
    cx->probe_in = nullptr; cx->probe_n = 0;
    GuardHit hit;
    const int rc = finish_inner(p, st, cx, out_len);
    if (rc != TRRE_OK || !was.active || was.n == 0 || !guard_applies(*p, *cx, was.n)) return rc;
    const int grc = guard_check(p, st, cx, was.d_in, was.n, was.stream, &hit);     // (in place: the snapshot, which still holds the input)
    if (grc) return grc;
    if (!hit.hit) return rc;
    size_t pre = 0;
    if (hit.line_start > 0) {                  // the lines before the line the guard stopped at: not to be guarded again
        const int prc = rerun(Finishing{p, st, cx, was, &pre}, was.family, &ScanCtx::guard_off, true, (size_t)hit.line_start);
        if (prc) { if (out_len) *out_len = pre; return prc; }
    }
    const size_t part = hit.part == 0xffffffffu ? 0 : hit.part;
    if (out_len) *out_len = pre + part;
    if (pre + part > was.cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    if (part) {
        HIP_TRY(hipMemcpyAsync(was.d_out + pre, cx->d_gout, part, hipMemcpyDeviceToDevice, was.stream));
        HIP_TRY(hipStreamSynchronize(was.stream));
    }
    cx->relaunches += 1;
    return fail(TRRE_E_DIVERGES, kStackMsg);
}

// finish_guarded, and the promise of an in-place scan that asks for room: the caller's buffer holds its input again (the emit pass
// may have written the chunks that fit), so the size query and the retry from the same buffer work as with separate buffers
int finish(trre_prog* p, DeviceState* st, ScanCtx* cx, size_t* out_len) {
    const Pending was = cx->pend;
    const int rc = finish_guarded(p, st, cx, out_len);
    if (rc == TRRE_E_CAPACITY && was.active && was.aliased) {
        HIP_TRY(hipMemcpyAsync(was.d_out, was.d_in, was.n, hipMemcpyDeviceToDevice, was.stream));
        HIP_TRY(hipStreamSynchronize(was.stream));
    }
    return rc;
}


// [a, a + n) and [b, b + m) share a byte (no pointer is dereferenced, no sum can wrap)
bool ranges_overlap(const void* a, size_t n, const void* b, size_t m) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return n && m && (x >= y ? x - y < m : y - x < n);
}

// the device path: d_in == d_out is a scan in place; any other overlap is refused before anything touches the device
int device_overlap(const uint8_t* d_in, size_t n, const uint8_t* d_out, size_t cap) {
    if (d_in != d_out && ranges_overlap(d_in, n, d_out, cap))
        return fail(TRRE_E_ARG, "error: input and output overlap (only d_in == d_out, a scan in place, is allowed)");
    return TRRE_OK;
}

// the prog's state on the calling thread's current device
int current_state(trre_prog* p, DeviceState** st) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    return device_state(p, dev, st);
}

constexpr size_t kGenChunk = (size_t)16 << 20;
constexpr int64_t kGenLaneBytes = 512;          // generator modes on the device: a lane per 512 bytes of input (the records that start there),
constexpr uint32_t kGenFrames = 512, kGenPathCap = 2048;   // a stack of 512 frames and 2 KiB of path output each (deeper / longer: the host enumeration)

// Generator modes on one device, host buffers: chunks cut at record ends go up, the backward kernel leaves one viability
// symbol per byte (k_rev_sweep, the guided families' backward pass with the tables of generate.cpp), the symbols come
// down and the accepting paths are enumerated on a few host threads.  `result` takes what the reference prints; false
// through `diverged`: a path ran into an epsilon cycle (what was printed before it stays).
int generate_on(trre_prog* p, DeviceState* st, const uint8_t* in, size_t n, std::vector<uint8_t>& result, bool& diverged) {
    using namespace trre;
    diverged = false;
    DeviceState::HostSlot& hs = st->slot[0];
    if (!hs.stream) HIP_TRY(hipStreamCreateWithFlags(&hs.stream, hipStreamNonBlocking));
    int rc = ctx_init(hs.ctx);
    if (rc) return rc;
    static const int threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency() / 2));
    size_t off = 0;
    while (off < n && !diverged) {
        size_t len = n - off;
        if (len > kGenChunk) {
            const void* nl = std::memchr(in + off + kGenChunk - 1, '\n', n - off - (kGenChunk - 1));
            len = nl ? (size_t)(static_cast<const uint8_t*>(nl) - (in + off)) + 1 : n - off;
        }
        rc = slot_reserve(hs, true, len);
        if (!rc) rc = slot_reserve(hs, false, len + 512);                  // (pin_out / d_out of the slot carry the symbols)
        if (rc) return rc;
        std::memcpy(hs.pin_in, in + off, len);
        HIP_TRY(hipMemcpyAsync(hs.d_in, hs.pin_in, len, hipMemcpyHostToDevice, hs.stream));
        ScanArgs args{};
        args.in_v0 = hs.d_in;                                              // (hipMalloc'ed: 16-byte aligned, v == g)
        args.vbeg = 0;
        args.vend = (int64_t)len;
        args.rblob = st->d_rblob;
        args.sym_v0 = hs.d_out;
        args.status = hs.ctx.d_status;
        launch_rev_sweep(args, (int)p->gen.n_rev * 256, 2048, hs.stream, false);
        HIP_TRY(hipGetLastError());
        // The enumeration on the device (gen_block.hpp; TRRE_GEN_HOST=1: on host threads, as in round 3): count, exclusive
        // sum, emit.  A chunk on which a path never returns, a search goes deeper than a lane's stack or the sizes leave 32 bits
        // goes to the host enumeration below, which also knows what the reference had printed when it gave up.
        bool done = false;
        uint32_t handed_over = 0;                                           // the status bits that sent the chunk to the host
        if (!switches().gen_host) {
            const int64_t n_lanes_raw = ((int64_t)len + kGenLaneBytes - 1) / kGenLaneBytes;
            const int64_t n_chunks = (n_lanes_raw + 255) / 256, n_lanes = n_chunks * 256;
            rc = ensure_workspace(&hs.ctx, n_chunks, 256);
            const size_t need = (size_t)n_lanes * (kGenFrames * 16 + kGenPathCap);
            if (!rc) HIP_TRY(hs.ctx.d_scratch.reserve(need, need));
            if (rc) return rc;
            GenArgs ga{};
            ga.stack = reinterpret_cast<uint32_t*>(hs.ctx.d_scratch.p);
            ga.path = hs.ctx.d_scratch + (size_t)n_lanes * kGenFrames * 16;
            ga.frames = kGenFrames;
            ga.path_cap = kGenPathCap;
            args.blob = st->d_nblob;
            args.lane_counts = hs.ctx.d_lane_counts;
            args.chunk_total = hs.ctx.d_chunk_total;
            args.chunk_base = hs.ctx.d_chunk_base;
            HIP_TRY(hipMemsetAsync(hs.ctx.d_status, 0, 24, hs.stream));
            launch_gen(1, args, ga, kGenLaneBytes, n_chunks, hs.stream);
            launch_chunk_scan(hs.ctx.d_chunk_total, hs.ctx.d_chunk_base, n_chunks, hs.stream);
            uint64_t total = 0;
            HIP_TRY(hipMemcpyAsync(hs.ctx.h_status, hs.ctx.d_status, 8, hipMemcpyDeviceToHost, hs.stream));
            HIP_TRY(hipMemcpyAsync(&total, hs.ctx.d_chunk_base + n_chunks, 8, hipMemcpyDeviceToHost, hs.stream));
            HIP_TRY(hipStreamSynchronize(hs.stream));
            handed_over = hs.ctx.h_status[0] & (kStDiverge | kStEditOverflow | kStCapacity);
            if (!handed_over) {
                // (the symbols sit in the slot's output buffer: the output gets a buffer of its own, kept by the context)
                const size_t want = (size_t)total + (size_t)total / 4 + 4096;          // (head room: grown only when total + 64 does not fit)
                if (hs.ctx.d_gen_out.cap < total + 64 && hs.ctx.d_gen_out.reserve(want, want) != hipSuccess)
                    return fail(TRRE_E_TOO_BIG, "error: out of device memory for the outputs of generator mode");
                args.out = hs.ctx.d_gen_out;
                args.cap = hs.ctx.d_gen_out.cap;
                launch_gen(2, args, ga, kGenLaneBytes, n_chunks, hs.stream);
                HIP_TRY(hipGetLastError());
                try {
                    const size_t at = result.size();
                    result.resize(at + (size_t)total);
                    if (total) HIP_TRY(hipMemcpyAsync(result.data() + at, hs.ctx.d_gen_out, (size_t)total, hipMemcpyDeviceToHost, hs.stream));
                } catch (const std::bad_alloc&) {
                    return fail(TRRE_E_TOO_BIG, "error: out of host memory for the outputs of generator mode");
                }
                HIP_TRY(hipStreamSynchronize(hs.stream));
                done = true;
            }
        }
        // (TRRE_TRACE: who enumerated this chunk — the tests read it: the host enumeration is the fallback AND the checker)
        if (switches().trace) {
            if (done) fprintf(stderr, "trre: generate: chunk at %zu, %zu bytes: device\n", off, len);
            else if (switches().gen_host) fprintf(stderr, "trre: generate: chunk at %zu, %zu bytes: host (TRRE_GEN_HOST)\n", off, len);
            else fprintf(stderr, "trre: generate: chunk at %zu, %zu bytes: host (status 0x%x)\n", off, len, handed_over);
        }
        if (!done) {
            HIP_TRY(hipMemcpyAsync(hs.pin_out, hs.d_out, len, hipMemcpyDeviceToHost, hs.stream));
            HIP_TRY(hipStreamSynchronize(hs.stream));
            try {
                if (!generate_buffer(p->gen, in + off, len, hs.pin_out, result, threads)) diverged = true;
            } catch (const std::bad_alloc&) {
                return fail(TRRE_E_TOO_BIG, "error: out of host memory for the outputs of generator mode");
            }
        }
        off += len;
    }
    return TRRE_OK;
}

}  // namespace trre_host

using namespace trre_host;

extern "C" {

void trre_free(trre_prog* p) {
    if (!p) return;
    trre_free(p->find_marks.release());
    trre_free(p->sub_texts.release());
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (auto& kv : p->dev) {
        DeviceState& st = *kv.second;
        (void)hipSetDevice(st.device);
        for (void* b : {(void*)st.d_blob, (void*)st.d_sblob, (void*)st.d_gblob, (void*)st.d_rblob, (void*)st.d_nblob, (void*)st.d_kblob, (void*)st.d_ablob}) (void)hipFree(b);
        (void)hipFree(st.d_lent); (void)hipFree(st.d_lpool); (void)hipFree(st.d_lcls);
        for (void* r : st.retired) (void)hipFree(r);
        ctx_free(st.ctx);
        for (auto& hs : st.slot) {
            pinned_put(hs.pin_in);
            pinned_put(hs.pin_out);
            (void)hipFree(hs.d_in);
            (void)hipFree(hs.d_out);
            if (hs.stream) (void)hipStreamDestroy(hs.stream);
            ctx_free(hs.ctx);
        }
    }
    if (have_cur) (void)hipSetDevice(cur);
    delete p;
}

const char* trre_last_error(void) { return g_error.c_str(); }

int trre_get_info(const trre_prog* p, trre_info* info) {
    if (!p || !info) return fail(TRRE_E_ARG, "error: null argument");
    std::memset(info, 0, sizeof *info);
    info->engine = p->engine;
    info->kernel = is_generate(p->mode) ? TRRE_KERNEL_GENERATE : scan_family(*p);
    info->nft_states = p->nft_states;
    info->nft_cons_states = p->nft_cons;
    if (p->engine == TRRE_ENGINE_DFT) {
        info->dft_states = p->dt.n_states;
        info->table_rows = p->dt.n_rows;
        info->table_classes = p->dt.n_cls;
        info->flags = p->dt.flags;
        if (p->lazy_only) {       // (the tables grow with the inputs: what exists now)
            info->dft_states = p->lazy->n_states();
            info->table_rows = p->lazy->n_rows();
            info->table_classes = p->lazy->n_cls();
        }
    } else {
        info->table_rows = p->nt.n_cons;
        info->flags = p->nt.flags;
    }
    info->table_bytes = (uint32_t)(p->blob.size() + p->sblob.size() + p->gblob.size() + p->rblob.size());
    info->chunk_bytes = (uint32_t)trre::chunk_bytes(p->engine, p->mask_bytes);
    if (p->stt.ok) { info->stream_states = p->stt.n_states; info->stream_classes = p->stt.n_cls; }
    info->nft_nodes = p->nft_nodes;
    if (p->gt.ok) { info->guided_rev_states = p->gt.n_rev; info->guided_fwd_states = p->gt.fwd.n_states; }
    if (p->gen.ok) info->guided_rev_states = p->gen.n_rev;
    return TRRE_OK;
}

int trre_set_kernel(trre_prog* p, int family) {
    if (!p) return fail(TRRE_E_ARG, "error: null argument");
    if (is_generate(p->mode)) return family == TRRE_KERNEL_AUTO ? TRRE_OK : fail(TRRE_E_UNSUPPORTED, "error: generator mode has one implementation");
    if (family != TRRE_KERNEL_AUTO && !family_allowed(*p, family))
        return fail(TRRE_E_UNSUPPORTED, "error: this kernel family cannot run these tables");
    p->forced_family = family;
    return TRRE_OK;
}

int trre_scan_enqueue(trre_prog* p, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, void* stream) {
    g_scan_flags = 0;
    if (!p || (n && (!d_in || !d_out))) return fail(TRRE_E_ARG, "error: null argument");
    if (own_call_only(*p)) return fail(TRRE_E_ARG, own_call_only(*p));
    if (device_overlap(d_in, n, d_out, cap)) return TRRE_E_ARG;
    DeviceState* st;
    int rc = current_state(p, &st);
    if (rc) return rc;
    if (is_generate(p->mode)) return fail(TRRE_E_ARG, "error: generator mode has no split form: use trre_scan_device / trre_scan_host");
    const int fam = scan_family(*p);
    return enqueue(p, st, &st->ctx, fam, d_in, n, d_out, cap, static_cast<hipStream_t>(stream));
}

int trre_scan_finish(trre_prog* p, size_t* out_len) {
    if (!p) return fail(TRRE_E_ARG, "error: null argument");
    DeviceState* st;
    int rc = current_state(p, &st);
    if (rc) return rc;
    return finish(p, st, &st->ctx, out_len);
}

// host-only entry for the CPU test tier: the enumeration of generator mode with symbols computed elsewhere (tests/cpu_shim.cpp
// runs the backward kernel's per-thread body on the host).  Not part of the drop-in boundary.
int trre_debug_generate(trre_prog* p, const uint8_t* in, size_t n, const uint8_t* sym, uint8_t* out, size_t cap, size_t* out_len) {
    if (!p || !is_generate(p->mode) || (n && (!in || !sym))) return fail(TRRE_E_ARG, "error: bad argument");
    std::vector<uint8_t> result;
    bool ok;
    try {
        ok = trre::generate_buffer(p->gen, in, n, sym, result, 2);
    } catch (const std::bad_alloc&) {
        return fail(TRRE_E_TOO_BIG, "error: out of host memory for the outputs of generator mode");
    }
    if (out_len) *out_len = result.size();
    if (result.size() > cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    if (!result.empty()) std::memcpy(out, result.data(), result.size());
    return ok ? TRRE_OK : fail(TRRE_E_DIVERGES, kDivergeMsg);
}

uint32_t trre_last_scan_flags(void) { return g_scan_flags; }

int trre_scan_device(trre_prog* p, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, size_t* out_len,
                     void* stream) {
    g_scan_flags = 0;
    if (!p || (n && (!d_in || !d_out))) return fail(TRRE_E_ARG, "error: null argument");
    if (own_call_only(*p)) return fail_empty(out_len, TRRE_E_ARG, own_call_only(*p));
    if (device_overlap(d_in, n, d_out, cap)) return TRRE_E_ARG;
    DeviceState* st;
    int rc = current_state(p, &st);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(st->mu);        // one scan call at a time per (prog, device); other devices run in parallel
    if (is_generate(p->mode)) {
        // the enumeration runs on the host (generate.cpp): input down, output up; the device computes the viability symbols
        if (out_len) *out_len = 0;
        if (n == 0) return TRRE_OK;
        std::vector<uint8_t> host, result;
        try {
            host.resize(n);
        } catch (const std::bad_alloc&) {
            return fail(TRRE_E_TOO_BIG, "error: out of host memory for generator mode");
        }
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIP_TRY(hipMemcpyAsync(host.data(), d_in, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        bool diverged = false;
        rc = generate_on(p, st, host.data(), n, result, diverged);
        if (rc) return rc;
        if (out_len) *out_len = result.size();
        if (result.size() > cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
        if (!result.empty()) HIP_TRY(hipMemcpyAsync(d_out, result.data(), result.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        return diverged ? fail(TRRE_E_DIVERGES, kDivergeMsg) : TRRE_OK;
    }
    const int fam = scan_family(*p);
    rc = enqueue(p, st, &st->ctx, fam, d_in, n, d_out, cap, static_cast<hipStream_t>(stream));
    if (rc) { st->ctx.pend = Pending(); return rc; }
    return finish(p, st, &st->ctx, out_len);
}

int trre_set_profiling(trre_prog* p, int on) {
    if (!p) return fail(TRRE_E_ARG, "error: null argument");
    p->profiling = on != 0;
    return TRRE_OK;
}

int trre_last_kernel_ms(trre_prog* p, float* ms) {
    if (!p || !ms) return fail(TRRE_E_ARG, "error: null argument");
    *ms = p->last_ms.load();
    return *ms < 0 ? TRRE_E_ARG : TRRE_OK;
}

}  // extern "C"
