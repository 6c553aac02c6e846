// runtime.cpp — C ABI (include/trre_mi355x.h) and host runtime: pattern
// compilation, table upload, kernel-family selection, launches, status
// collection.  The scan always runs on the GPU; nothing here computes output
// bytes on the host.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <sys/mman.h>

#include "../../include/trre_mi355x.h"
#include "device_blob.hpp"
#include "front.hpp"
#include "launch.hpp"
#include "switches.hpp"
#include "scan_block.hpp"
#include "splice_block.hpp"
#include "gen_block.hpp"
#include "lazy_block.hpp"
#include "one_block.hpp"
#include "map_block.hpp"
#include "guard_block.hpp"
#include "records_block.hpp"

namespace {

thread_local std::string g_error;
thread_local uint32_t g_scan_flags = 0;       // TRRE_SCAN_*: what the last scan call on this thread has to add to its return code

constexpr int kNotThisRoute = 1;              // a launch route declines (positive: no TRRE_E_* code): the caller takes the next one

int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}
int fail_empty(size_t* out_len, int code, const std::string& msg) { if (out_len) *out_len = 0; return fail(code, msg); }     // ... and no output stands

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(TRRE_E_DEVICE, std::string("hip: ") + hipGetErrorString(e_) + " at " #expr); \
    } while (0)

// Pinned staging memory: anonymous pages (huge ones where the kernel gives them), touched by a few threads, then registered with the
// runtime.  hipHostMalloc of the host path's six 36 MiB buffers took 56 ms of a process's first scan call (the runtime allocates, clears
// and pins 4 KiB pages on one thread); this takes 3 ms and copies at the same 57 GB/s (tools/probes/pin_cost.hip, round 5).
std::mutex g_pin_mu;
std::map<void*, size_t> g_pin_len;
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

// What one launch is made of, computed once per enqueue (make_plan): the kernel arguments, the geometry of lanes and chunks, the table forms.
// finish() keeps it for the rounds it runs on the same launch (the lazy rounds, the repair rounds of the exact sub-ranges).
struct LaunchPlan {
    trre::ScanArgs args{};
    int64_t lane_bytes = 0, rev_lane_bytes = 0, n_chunks = 0;
    int threads = 0, sym_mode = 0;    // threads: per workgroup of the workspace's owner (ensure_workspace)
    int g16 = 0;                      // LDS room of the 16-byte + pair forms, 0: the 8-byte entries
    bool g16_slow = false, direct_ent_lds = false;
    bool direct = false;              // the stream and guided families: a lane walks a long sub-range straight from memory
    bool window = false, mapgen_on = false, use_exact = false;    // the window kernel; the memoryless one-pass kernel is to be tried; exact sub-ranges (ScanArgs::exact)
};

struct Pending {
    bool active = false;
    int family = 0;         // what runs
    int asked = 0;          // ... and what the caller's family choice was (a length-preserving family on an input with long lines runs as its general sibling)
    const uint8_t* d_in = nullptr;  // what the kernels read: the caller's input, or its snapshot (ScanCtx::d_snap) when the scan is in place
    uint8_t* d_out = nullptr;
    const uint8_t* user_in = nullptr;  // the caller's input pointer (a batch is the same scan as the caller named it)
    bool aliased = false;           // d_out is the caller's input: the kernels read the snapshot
    size_t n = 0, cap = 0;
    hipStream_t stream = nullptr;
    bool launched = false;
    bool timed = false;
    int count = 0;          // launches in the current batch
    const uint64_t* total_at = nullptr;   // general families: where the launch leaves its output size
    bool patched = false;                 // the launch was the mark + splice pair of a large table's copy form, not a count / emit pair
    bool one = false;                     // the launch was the one-pass kernel (one_block.hpp), not a count / emit pair
    bool mapgen = false;                  // ... the memoryless one-pass kernel (map_block.hpp)
    bool exact = false;                   // the launch ran exact sub-ranges: finish() runs repair rounds and the emit pass again, from the plan
    LaunchPlan plan;
};

// A device buffer that only grows, with its capacity in the units of whoever sizes it.  reserve() leaves pointer = null, capacity = 0 when
// the allocation fails and hands the error back: the caller chooses what that means (an error, another route, a message of its own).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    // (moved only — which rules copies out: a ScanCtx is only ever assigned from a fresh one, in ctx_free)
    DevBuf& operator=(DevBuf&& o) noexcept { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; return *this; }
    ~DevBuf() { release(); }
    operator T*() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t reserve(size_t want, size_t bytes) {
        if (want <= cap) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes);
        if (e != hipSuccess) p = nullptr; else cap = want;
        return e;
    }
};

// Everything ONE in-flight scan needs on a device besides the tables: status words, the workspaces of the
// general families, scratch buffers, timing events.  trre_scan_device / enqueue+finish use the device's own
// context; trre_scan_host keeps several chunks in flight, each with the context of its slot.
struct ScanCtx {
    uint32_t* d_status = nullptr;     // [4]
    uint32_t* h_status = nullptr;     // pinned mirror: [0] status bits; [2..3] total (u64)
    DevBuf<uint32_t> d_lane_counts;   // general families' workspace, in chunks of 256 lanes (ensure_workspace) ...
    DevBuf<uint64_t> d_chunk_total, d_chunk_base;
    DevBuf<uint8_t> d_scratch;        // NFT tile kernels: mask scratch for lines longer than the LDS tile; the backtracking pool (bytes)
    DevBuf<uint32_t> d_redo;          // window kernel redo list (lanes)
    DevBuf<uint8_t> d_sym;            // guided families: one symbol per input byte (bytes)
    DevBuf<uint8_t> d_snap;           // an in-place scan (d_in == d_out): a copy of its input, which every launch and fallback reads;
                                      // trre_scan_device_records / _strings: the staged copy, which the scan reads (bytes)
    DevBuf<uint64_t> d_rec;           // the five column calls: status word, then what the pass that runs carves (rec_carve; spans: span_on) (tiles)
    DevBuf<uint8_t> d_gen_out;        // generator modes: the enumeration's output before it goes down (bytes)
    DevBuf<uint8_t> d_framed;         // trre_scan_device_strings: the scan's output with every record's closing '\n' still in it (bytes)
    DevBuf<uint64_t> d_match;         // trre_match_device_strings: accepted strings per group of 256, then their exclusive scan [groups + 1] (groups)
    DevBuf<int64_t> d_find_off;       // trre_find_device_strings: the list offsets while they are ranks and located positions [nrec + 1] (entries)
    DevBuf<uint8_t> d_find_marks;     // ... the marks scan unframed: a byte per match (bytes)
    DevBuf<int64_t> d_filter_lists;   // trre_filter_device_strings, trre_field_device_strings, trre_sub_device_strings: the span call's list offsets [nrec + 1] (entries)
    DevBuf<int64_t> d_field_bounds;   // trre_field_device_strings: where every string's field starts [nrec], then where it ends [nrec] (strings)
    DevBuf<int64_t> d_sub_idx;        // trre_sub_device_strings: S, E, XO, P, each [found + 2] with entry -1 in front (matches)
    DevBuf<uint8_t> d_sub_texts;      // ... the texts scan unframed (bytes)
    DevBuf<uint64_t> d_sub_cnt;       // ... the status word, cnt [3][chunks], base [3][chunks + 1] (chunks)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the copy form of a large table (scan_block.hpp fb_lane<3> / fb_copy_lane): events, lane headers (rows of kCopyEvCap events)
    DevBuf<uint32_t> d_cevents, d_chdr;
    // the stack guard (guard_block.hpp): window flags, runs of flagged windows, results, the pool of stacks, the one line's output
    DevBuf<uint64_t> d_gflags;
    DevBuf<uint8_t> d_gruns;          // GuardRun[cap], then GuardResult[cap]
    DevBuf<uint32_t> d_gstack;        // [kGuardSlots][65 536][3]
    DevBuf<uint8_t> d_gobuf, d_gout;
    // exact sub-ranges: entry / exit states and flags per lane; the long-line probe and what it said about which buffer
    DevBuf<uint32_t> d_spec, d_probe;
    const uint8_t* probe_in = nullptr;
    size_t probe_n = 0;
    bool long_lines = false;
    bool exact_off = false;           // finish() runs a scan again the old way (a diverging attempt: the first lane in stream order has to be named)
    // the one-pass kernel (one_block.hpp): look-back descriptors [tiles], then the ticket counter and the total
    DevBuf<uint64_t> d_one;
    bool one_off = false;             // finish() runs the scan again as a count / emit pair (a void one-pass launch)
    DevBuf<uint64_t> d_mg;            // the memoryless kernel (map_block.hpp): descriptors, group sums and totals, the total (tiles)
    bool mapgen_off = false;          // finish() runs the scan again on the general family (a NUL in the input)
    int mapgen_voids = 0;             // launches of the memoryless kernel that were void (a NUL; a grid that was not resident): after two, the pair from the start
    bool mapgen_dense = false;        // a program with longer texts printed 4 % more than it read: its texts are frequent ('a:xyz': the pair is 7 % faster there)
    DevBuf<uint32_t> d_miss;          // lazy tables (lazy_block.hpp): [0] misses listed, then {row, class} pairs
    int bt_tier = 0;                  // the backtracking fallback: which size of stacks and path buffers the next launch uses (kBtTiers)
    bool guard_off = false;           // finish() scans the lines before a line the guard stopped at: not to be guarded again
    bool patch_off = false;           // finish() runs the scan again as a count / emit pair (diverged, or out of overflow records)
    int relaunches = 0;               // finish() ran the scan again (scratch, NUL, overflow): whatever was downloaded early is stale
    Pending pend;
};

constexpr int kHostSlots = 3;         // chunks in flight in trre_scan_host: staging in, on the device, staging out

struct DeviceState {
    std::mutex mu;                    // one scan call at a time per (prog, device): trre_scan_device, trre_scan_host
    int device = 0;
    uint8_t* d_blob = nullptr;
    uint8_t* d_sblob = nullptr;       // stream tables
    uint8_t* d_gblob = nullptr;       // guided families: forward tables (stream form) ...
    uint8_t* d_rblob = nullptr;       // ... and the backward DFA
    uint8_t* d_nblob = nullptr;       // generator modes: the enumeration's tables
    uint8_t* d_kblob = nullptr;       // the stack guard's tables (the NFT itself)
    uint8_t* d_ablob = nullptr;       // match mode: a bit per backward state, set where a line that starts with that symbol is accepted
    // the deterministic engine's tables while they are being built (front.hpp: LazyDft): this device's copy and how much of the host's it holds.
    // A buffer that has to grow is replaced, not freed: scans of other chunks may still be reading it (freed with the state).
    uint64_t* d_lent = nullptr;
    uint8_t* d_lpool = nullptr;
    uint8_t* d_lcls = nullptr;
    size_t lent_cap = 0, lpool_cap = 0;        // rows / bytes
    uint32_t lazy_rows_up = 0, lazy_epoch_up = 0;
    size_t lazy_pool_up = 0;
    std::vector<void*> retired;
    ScanCtx ctx;
    struct HostSlot {
        uint8_t *pin_in = nullptr, *pin_out = nullptr, *d_in = nullptr, *d_out = nullptr;
        size_t in_cap = 0, out_cap = 0;
        hipStream_t stream = nullptr;
        ScanCtx ctx;
    } slot[kHostSlots];
};

template <class T>
void put(std::vector<uint8_t>& b, size_t off, const T* src, size_t count) {
    if (b.size() < off + count * sizeof(T)) b.resize(off + count * sizeof(T));
    if (count) std::memcpy(b.data() + off, src, count * sizeof(T));
}
size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace

struct trre_prog {
    int engine = 0;
    int forced_family = TRRE_KERNEL_AUTO;
    uint32_t nft_states = 0, nft_cons = 0;
    trre::DftTables dt;
    trre::NftTables nt;
    trre::StreamTables stt;
    trre::GuidedTables gt;
    trre::GenTables gen;              // generator modes (`-a`): viability DFA for the device, follow lists for the host enumeration
    int mode = TRRE_MODE_SCAN;
    bool prints_newline = false;      // a '\n' of the program's own can be printed (nft_prints_newline): no records path
    uint32_t nft_nodes = 0;
    bool has_engine_tables = false;   // tile kernels available (always for DFT; NFT: <= 64 nodes, no epsilon cycle)
    std::vector<uint8_t> blob;
    std::vector<uint8_t> sblob;
    std::vector<uint8_t> gblob, rblob;
    std::vector<uint8_t> nblob;       // generator modes: the enumeration's tables (gen_block.hpp); scan mode, NFT engine: the same lists for the backtracking fallback
    bool bt_ok = false;               // scan mode, NFT engine: nblob holds the backtracking fallback's tables
    trre::Nft dft_nft;                // DFT engine: the automaton the lazy tables are built from
    std::unique_ptr<trre::LazyDft> lazy;   // DFT engine: the tables one miss at a time (front.hpp) — a pattern beyond the eager caps, or on request
    bool lazy_only = false;           // ... the eager construction gave up: nothing else exists
    std::mutex lazy_mu;               // explore() and the uploads
    trre::GuardTables guard;          // scan mode, NFT engine: which lines can exhaust the reference's stack (stack_guard.cpp)
    std::vector<uint8_t> kblob;
    std::vector<uint8_t> ablob;       // match mode, guided tables: GuidedTables::accept as bits (32-bit words; trre_match_device_strings)
    std::unique_ptr<trre_prog> find_marks;    // find mode: this program holds the texts table (gt), the inner one the marks table over the same
                                              // backward DFA — a program of its own, with its own device state (trre_find_device_strings)
    std::unique_ptr<trre_prog> sub_texts;     // sub mode: this program holds the markers' table of spans mode (gt) and the stack guard, the inner one
                                              // the texts table of find mode over the same nodes (trre_sub_device_strings)
    int mask_bytes = 0;
    bool profiling = false;
    std::atomic<float> last_ms{-1.f};
    std::atomic<bool> bounded_off{false};     // a launch on a bounded stream table met a run it was not built for: the guided / tile kernels from now on
    std::atomic<int> one_fails{0};            // void launches of the one-pass kernel (a region outgrown, a first guess wrong): after two the pair from now on
    std::atomic<bool> copy_form_off{false};   // a launch of the copy form met more texts than its event lists hold: the count / emit pair from now on
    std::mutex dev_mu;                                  // guards the map (not the states)
    std::map<int, std::unique_ptr<DeviceState>> dev;
};

namespace {

void serialize_dft(trre_prog& p) {
    using namespace trre;
    const DftTables& t = p.dt;
    DftBlobHeader h{};
    h.magic = kMagicDft;
    h.n_rows = t.n_rows;
    h.n_cls = t.n_cls;
    h.flags = t.flags;
    h.max_edge_out = t.max_edge_out;
    h.n_states = t.n_states;
    size_t off = sizeof h;
    h.off_ent0 = (uint32_t)off; off += 256 * 8;
    h.off_cls = (uint32_t)off; off += 256;
    h.off_bytemap = (uint32_t)off; off += 256;
    h.off_ent = (uint32_t)off; off += t.ent.size() * 8;
    h.off_pool = (uint32_t)off; h.pool_bytes = (uint32_t)t.pool.size(); off += t.pool.size();
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    std::vector<uint8_t>& b = p.blob;
    b.assign(off, 0);
    std::vector<uint64_t> ent0(256);
    for (int c = 0; c < 256; ++c) ent0[c] = t.ent[t.cls[c]];      // row 0, expanded over raw bytes
    put(b, 0, &h, 1);
    put(b, h.off_ent0, ent0.data(), 256);
    put(b, h.off_cls, t.cls.data(), 256);
    put(b, h.off_bytemap, t.bytemap.data(), 256);
    put(b, h.off_ent, t.ent.data(), t.ent.size());
    put(b, h.off_pool, t.pool.data(), t.pool.size());
}

void serialize_nft(trre_prog& p) {
    using namespace trre;
    const NftTables& t = p.nt;
    NftBlobHeader h{};
    h.magic = kMagicNft;
    h.n_cons = t.n_cons;
    h.flags = t.flags;
    h.n_follow = (uint32_t)t.follow.size();
    h.n_states = t.n_states;
    size_t off = sizeof h;
    h.off_cons_mask = (uint32_t)off; off += 256 * 8;
    h.off_pred = (uint32_t)off; off += (t.n_cons + 1) * 8;
    h.off_follow_off = (uint32_t)off; off += align_up((t.n_cons + 2) * 4, 8);
    h.off_follow = (uint32_t)off; off += t.follow.size() * sizeof(NftFollow);
    h.off_pool = (uint32_t)off; h.pool_bytes = (uint32_t)t.pool.size(); off += t.pool.size();
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    std::vector<uint8_t>& b = p.blob;
    b.assign(off, 0);
    std::vector<uint64_t> pred(t.pred);
    pred.push_back(t.to_final);
    put(b, 0, &h, 1);
    put(b, h.off_cons_mask, t.cons_mask.data(), 256);
    put(b, h.off_pred, pred.data(), pred.size());
    put(b, h.off_follow_off, t.follow_off.data(), t.follow_off.size());
    put(b, h.off_follow, t.follow.data(), t.follow.size());
    put(b, h.off_pool, t.pool.data(), t.pool.size());
}

void serialize_stream(const trre::StreamTables& t, std::vector<uint8_t>& b) {
    using namespace trre;
    StreamBlobHeader h{};
    h.magic = kMagicStream;
    h.n_states = t.n_states;
    h.n_cls = t.n_cls;
    h.flags = t.flags;
    h.max_out = t.max_out;
    size_t off = sizeof h;
    h.off_cls = (uint32_t)off; off += 256;
    h.off_ent = (uint32_t)off; h.ent_bytes = (uint32_t)(t.ent.size() * 8); off += t.ent.size() * 8;
    h.off_pool = (uint32_t)off; h.pool_bytes = (uint32_t)t.pool.size(); off += t.pool.size();
    off = align_up(off, 16);
    h.off_lpw = (uint32_t)off; h.lpw_bytes = (uint32_t)(t.lpw.size() * 4); h.lpw_delay = t.lpw_delay; off += t.lpw.size() * 4;
    off = align_up(off, 16);
    h.off_g16 = (uint32_t)off; h.g16_bytes = (uint32_t)(t.g16.size() * 4); off += t.g16.size() * 4;
    off = align_up(off, 16);
    h.off_p32 = (uint32_t)off; h.p32_bytes = (uint32_t)(t.p32.size() * 4); h.p32_slow = t.p32_slow ? 1u : 0u; off += t.p32.size() * 4;
    off = align_up(off, 16);
    h.off_lpw2 = (uint32_t)off; h.lpw2_bytes = (uint32_t)(t.lpw2.size() * 4); off += t.lpw2.size() * 4;
    off = align_up(off, 16);
    if (t.fb_ok) {
        h.fb_slots = (uint32_t)t.fb_comb.size(); h.off_fb_comb = (uint32_t)off; off = align_up(off + t.fb_comb.size() * 8, 16);
        h.fb_lits = (uint32_t)t.fb_lit.size(); h.off_fb_lit = (uint32_t)off; off = align_up(off + t.fb_lit.size() * 8, 16);
        h.fb_escs = (uint32_t)t.fb_esc_slot.size(); h.off_fb_esc_slot = (uint32_t)off; off = align_up(off + t.fb_esc_slot.size() * 4, 16);
        h.off_fb_esc = (uint32_t)off; off = align_up(off + t.fb_esc.size() * 4, 16);
        h.off_fb_pool = (uint32_t)off; off = align_up(off + t.fb_pool.size(), 16);
        if (t.fb_copy_ok) { h.off_fb_lit_meta = (uint32_t)off; off = align_up(off + t.fb_lit_meta.size() * 2, 16); }
        if (t.fb_mark4_ok) {
            h.fb4_slots = (uint32_t)t.fb_comb4.size(); h.off_fb_comb4 = (uint32_t)off; off = align_up(off + t.fb_comb4.size() * 4, 16);
            h.fb4_dense = (uint32_t)t.fb_dense_base.size(); h.off_fb_dense4 = (uint32_t)off; off = align_up(off + t.fb_dense4.size() * 4, 16);
            h.off_fb_dense_base = (uint32_t)off; off = align_up(off + t.fb_dense_base.size() * 2, 16);
            h.fb_pad = t.fb_pad;
            std::memcpy(h.fb_start4, t.fb_start4, sizeof h.fb_start4);
        }
        std::memcpy(h.fb_start, t.fb_start, sizeof h.fb_start);
    }
    if (t.mg_max) { h.off_mg = (uint32_t)off; h.mg_max = t.mg_max; off = align_up(off + t.mg.size() * 4, 16); }
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    b.assign(off, 0);
    put(b, 0, &h, 1);
    if (t.mg_max) put(b, h.off_mg, t.mg.data(), t.mg.size());
    if (t.fb_ok) {
        put(b, h.off_fb_comb, t.fb_comb.data(), t.fb_comb.size());
        put(b, h.off_fb_lit, t.fb_lit.data(), t.fb_lit.size());
        put(b, h.off_fb_esc_slot, t.fb_esc_slot.data(), t.fb_esc_slot.size());
        put(b, h.off_fb_esc, t.fb_esc.data(), t.fb_esc.size());
        put(b, h.off_fb_pool, t.fb_pool.data(), t.fb_pool.size());
        if (t.fb_copy_ok) put(b, h.off_fb_lit_meta, t.fb_lit_meta.data(), t.fb_lit_meta.size());
        if (t.fb_mark4_ok) {
            put(b, h.off_fb_comb4, t.fb_comb4.data(), t.fb_comb4.size());
            put(b, h.off_fb_dense4, t.fb_dense4.data(), t.fb_dense4.size());
            put(b, h.off_fb_dense_base, t.fb_dense_base.data(), t.fb_dense_base.size());
        }
    }
    put(b, h.off_cls, t.cls.data(), 256);
    put(b, h.off_ent, t.ent.data(), t.ent.size());
    put(b, h.off_pool, t.pool.data(), t.pool.size());
    put(b, h.off_lpw, t.lpw.data(), t.lpw.size());
    put(b, h.off_g16, t.g16.data(), t.g16.size());
    put(b, h.off_p32, t.p32.data(), t.p32.size());
    put(b, h.off_lpw2, t.lpw2.data(), t.lpw2.size());
}

void serialize_rev_table(uint32_t n_rev, uint32_t n_cls, uint32_t sym_bits, const std::array<uint8_t, 256>& cls, const std::vector<uint8_t>& rev,
                         std::vector<uint8_t>& b) {
    using namespace trre;
    RevBlobHeader h{};
    h.magic = kMagicRev;
    h.n_rev = n_rev;
    h.n_cls = n_cls;
    h.sym_bits = sym_bits;
    size_t off = sizeof h;
    h.off_cls = (uint32_t)off; off += 256;
    h.off_tab = (uint32_t)off; off += align_up(rev.size(), 16);
    h.off_wide = (uint32_t)off; off += (size_t)n_rev * 256;
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    b.assign(off, 0);
    std::vector<uint8_t> wide((size_t)n_rev * 256);
    for (uint32_t r = 0; r < n_rev; ++r)
        for (int c = 0; c < 256; ++c) wide[(size_t)r * 256 + c] = rev[(size_t)r * n_cls + cls[c]];
    put(b, 0, &h, 1);
    put(b, h.off_cls, cls.data(), 256);
    put(b, h.off_tab, rev.data(), rev.size());
    put(b, h.off_wide, wide.data(), wide.size());
}
void serialize_rev(const trre::GuidedTables& g, std::vector<uint8_t>& b) {
    if (!g.wide) { serialize_rev_table(g.n_rev, g.n_cls, g.sym_bits, g.cls, g.rev, b); return; }
    // more than 256 states: 16-bit entries, [state][raw byte], read through L1 / L2 by k_rev_wide
    using namespace trre;
    RevBlobHeader h{};
    h.magic = kMagicRev;
    h.n_rev = g.n_rev;
    h.n_cls = g.n_cls;
    h.sym_bits = 16;
    size_t off = sizeof h;
    h.off_cls = (uint32_t)off; off += 256;
    h.off_tab = (uint32_t)off; off += align_up(g.rev16.size() * 2, 16);
    h.off_wide = (uint32_t)off; off += (size_t)g.n_rev * 256 * 2;
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    b.assign(off, 0);
    std::vector<uint16_t> wide((size_t)g.n_rev * 256);
    for (uint32_t r = 0; r < g.n_rev; ++r)
        for (int c = 0; c < 256; ++c) wide[(size_t)r * 256 + c] = g.rev16[(size_t)r * g.n_cls + g.cls[c]];
    put(b, 0, &h, 1);
    put(b, h.off_cls, g.cls.data(), 256);
    put(b, h.off_tab, g.rev16.data(), g.rev16.size());
    put(b, h.off_wide, wide.data(), wide.size());
}

// generator modes: follow lists (every epsilon path), the nodes' byte sets, the viability sets per symbol (gen_block.hpp)
void serialize_gen(const trre::GenTables& g, std::vector<uint8_t>& b) {
    using namespace trre;
    const NftNodes& nd = g.nodes;
    const uint32_t n_nodes = (uint32_t)nd.node.size();
    std::vector<uint32_t> bytes((size_t)n_nodes * 8, 0), foff, follow;
    std::vector<uint8_t> echo(n_nodes, 0), pool;
    for (uint32_t t = 0; t < n_nodes; ++t) {
        for (int c = 0; c < 256; ++c)
            if (nd.node[t].reads((uint8_t)c)) bytes[(size_t)t * 8 + (c >> 5)] |= 1u << (c & 31);
        echo[t] = nd.node[t].echo ? 1 : 0;
    }
    for (size_t l = 0; l < nd.follow.size(); ++l) {
        foff.push_back((uint32_t)(follow.size() / 3));
        for (const NodeFollow& e : nd.follow[l]) {
            if (e.out.size() > 0xffff) throw Error(kErrTooBig, "error: an output of more than 64 KiB on one epsilon path (generator mode)");
            follow.push_back(e.target);
            follow.push_back((uint32_t)pool.size());
            follow.push_back((uint32_t)e.out.size() | (e.mute ? 1u << 16 : 0u));
            pool.insert(pool.end(), e.out.begin(), e.out.end());
        }
    }
    foff.push_back((uint32_t)(follow.size() / 3));
    GenBlobHeader h{};
    h.magic = kMagicGen;
    h.n_nodes = n_nodes;
    h.n_rev = g.n_rev;
    h.words = g.viable_words;
    h.match_mode = g.match_mode ? 1u : 0u;
    h.n_follow = (uint32_t)(follow.size() / 3);
    size_t off = align_up(sizeof h, 16);
    h.off_bytes = (uint32_t)off; off = align_up(off + bytes.size() * 4, 16);
    h.off_echo = (uint32_t)off; off = align_up(off + echo.size(), 16);
    h.off_foff = (uint32_t)off; off = align_up(off + foff.size() * 4, 16);
    h.off_follow = (uint32_t)off; off = align_up(off + follow.size() * 4, 16);
    h.off_pool = (uint32_t)off; h.pool_bytes = (uint32_t)pool.size(); off = align_up(off + pool.size() + 8, 16);
    h.off_viable = (uint32_t)off; off = align_up(off + g.viable.size() * 8, 16);
    h.total_bytes = (uint32_t)off;
    b.assign(off, 0);
    put(b, 0, &h, 1);
    put(b, h.off_bytes, bytes.data(), bytes.size());
    put(b, h.off_echo, echo.data(), echo.size());
    put(b, h.off_foff, foff.data(), foff.size());
    put(b, h.off_follow, follow.data(), follow.size());
    put(b, h.off_pool, pool.data(), pool.size());
    put(b, h.off_viable, g.viable.data(), g.viable.size());
}

bool is_generate(int mode) { return mode == TRRE_MODE_SCAN_ALL || mode == TRRE_MODE_MATCH_ALL; }
bool is_stream(int fam) { return fam == TRRE_KERNEL_STREAM_LP || fam == TRRE_KERNEL_STREAM_GEN; }
bool is_guided(int fam) { return fam == TRRE_KERNEL_GUIDED_LP || fam == TRRE_KERNEL_GUIDED_GEN; }
bool is_gen(int fam) {
    return fam == TRRE_KERNEL_TILE_GEN || fam == TRRE_KERNEL_STREAM_GEN || fam == TRRE_KERNEL_GUIDED_GEN || fam == TRRE_KERNEL_BACKTRACK || fam == TRRE_KERNEL_DFT_LAZY;
}
bool is_guided_wide(const trre_prog& p, int fam) { return (fam == TRRE_KERNEL_GUIDED_LP || fam == TRRE_KERNEL_GUIDED_GEN) && p.gt.wide; }
// how the guided families' backward pass stores its symbols: 4 two per byte, 8 one per byte, 16 two bytes each (wide tables)
int guided_sym_bits(const trre_prog& p) { return p.gt.wide ? 16 : (p.gt.sym_bits == 4 && !trre::switches().no_g16 ? 4 : 8); }
bool lp_inplace(uint32_t flags) { return (flags & trre::kFlagLengthPreserving) && (flags & trre::kFlagNoOverrun); }
// the family that takes over when a length-preserving launch met a NUL, or a bounded stream table a long run
int general_family(const trre_prog& p, bool stream_ok) {
    if (p.lazy_only) return TRRE_KERNEL_DFT_LAZY;
    if (stream_ok && p.stt.ok) return TRRE_KERNEL_STREAM_GEN;
    if (p.gt.ok) return TRRE_KERNEL_GUIDED_GEN;
    if (p.engine == TRRE_ENGINE_DFT && p.mode == TRRE_MODE_SCAN) return TRRE_KERNEL_DFT_LAZY;      // (round 6: 100 GB/s against the tile kernels' 48)
    return p.has_engine_tables ? TRRE_KERNEL_TILE_GEN : TRRE_KERNEL_BACKTRACK;
}

int auto_family(const trre_prog& p) {
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

bool family_allowed(const trre_prog& p, int fam) {
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
void ctx_free(ScanCtx& c) {
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
trre::ScanArgs base_args(const uint8_t* d_in, size_t n, uint8_t* d_out = nullptr) {
    const int64_t a = (int64_t)(reinterpret_cast<uintptr_t>(d_in) & 15u);
    trre::ScanArgs args{};
    args.in_v0 = d_in - a;
    if (d_out) { args.out_v0 = d_out - a; args.out = d_out; }
    args.vbeg = a;
    args.vend = a + (int64_t)n;
    return args;
}

int ensure_workspace(ScanCtx* c, int64_t n_chunks, int threads) {
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
constexpr const char* kStackMsg = "error: stack max capacity reached";
constexpr const char* kFindOnlyMsg = "error: a program compiled with TRRE_MODE_FIND runs through trre_find_device_strings only";
constexpr const char* kSpansOnlyMsg = "error: a program compiled with TRRE_MODE_SPANS runs through trre_span_device_strings, trre_split_device_strings, trre_filter_device_strings and trre_field_device_strings only";
constexpr const char* kDivergeMsg = "error: stack max capacity reached (the reference's search does not terminate on this input)";
// a program that one call alone runs: that call's name for every other call's refusal (null: any scan call may run it)
constexpr const char* kSubOnlyMsg = "error: a program compiled with TRRE_MODE_SUB runs through trre_sub_device_strings only";
const char* own_call_only(const trre_prog& p) {
    return p.mode == TRRE_MODE_FIND ? kFindOnlyMsg : p.mode == TRRE_MODE_SPANS ? kSpansOnlyMsg : p.mode == TRRE_MODE_SUB ? kSubOnlyMsg : nullptr;
}
bool guard_applies(const trre_prog& p, const ScanCtx& cx, size_t n) {
    return !trre::switches().no_stack_guard && p.guard.on && !cx.guard_off &&
           (p.mode == TRRE_MODE_SCAN || p.mode == TRRE_MODE_MATCH || p.mode == TRRE_MODE_FIND || p.mode == TRRE_MODE_SPANS || p.mode == TRRE_MODE_SUB) && n + 1 >= p.guard.l_min;
}
struct GuardHit {
    bool hit = false;
    uint64_t line_start = 0;
    uint32_t part = 0;         // bytes of the line's output in cx->d_gout, or ~0u: they could not be produced
};
template <class T>
int guard_room(DevBuf<T>& d, size_t want) {
    if (d.reserve(want, want * sizeof(T)) != hipSuccess) return fail(TRRE_E_TOO_BIG, "error: out of device memory (stack guard)");
    return TRRE_OK;
}
// Looks for lines long enough to exhaust the reference's stack and runs the reference's search on them.  Synchronous: it ends
// with the stream idle.  hit: the first line (in input order) on which the search overflows, and what the reference had printed of it.
int guard_check(trre_prog* p, DeviceState* st, ScanCtx* cx, const uint8_t* d_in, size_t n, hipStream_t stream, GuardHit* hit) {
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

int lazy_ensure(trre_prog* p) {
    std::lock_guard<std::mutex> lock(p->lazy_mu);
    if (p->lazy) return TRRE_OK;
    try {
        trre::LazyLimits lim;
        if (const trre::SwitchNum mb = trre::lazy_max_bytes_now(); mb.set) lim.max_bytes = (size_t)mb.v;
        if (const trre::SwitchNum ss = trre::lazy_seed_states_now(); ss.set) lim.seed_states = (size_t)ss.v;
        p->lazy.reset(new trre::LazyDft(p->dft_nft, lim));
    } catch (const trre::Error& e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc&) {
        return fail(TRRE_E_TOO_BIG, "error: out of memory while determinising");
    }
    return TRRE_OK;
}

// brings the device's copy of the tables up to the host's: the pool's new bytes, then the new rows, then the old rows that changed (an entry
// must never name a row or a text the device does not hold yet — scans of other chunks may be reading the tables meanwhile)
int lazy_sync(trre_prog* p, DeviceState* st) {
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
int lazy_round(trre_prog* p, DeviceState* st, ScanCtx* cx, const trre::ScanArgs& args, int64_t n_chunks, bool fresh, hipStream_t stream) {
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
MapGenChain g_mapgen_chain[64];

// the memoryless kernel's workspace and launch (map_block.hpp); TRRE_OK: launched (pd.total_at set), else the caller takes another route
int mapgen_launch(ScanCtx* cx, const trre::ScanArgs& args, const trre::StreamTables& stt, hipStream_t stream, Pending& pd) {
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
int long_line_switch(trre_prog* p, ScanCtx* cx, int* family, const uint8_t* d_in, size_t n, size_t cap, hipStream_t stream) {
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
const trre::StreamTables& walked_tables(const trre_prog* p, int family) { return is_guided(family) ? p->gt.fwd : p->stt; }

// the launch of `family` over [d_in, d_in + n): arguments, lanes, chunks, table forms.  Touches nothing on the device.
LaunchPlan make_plan(const trre_prog* p, const DeviceState* st, const ScanCtx* cx, int family, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap) {
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
int route_lazy(trre_prog* p, DeviceState* st, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    return lazy_round(p, st, cx, pl.args, pl.n_chunks, true, stream);
}
// the search itself (gen_block.hpp: bt_lane): a pool of workgroups takes the chunks of 256 sub-ranges in turn, each thread
// with a stack and a path buffer of its own for the whole launch
int route_backtrack(DeviceState* st, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
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
int route_window(trre_prog* p, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
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
int route_wide_guided(ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    launch_rev_wide(pl.args, pl.lane_bytes, stream);
    launch_wide_fwd(1, pl.args, pl.lane_bytes, pl.n_chunks, stream);
    launch_chunk_scan(cx->d_chunk_total, cx->d_chunk_base, pl.n_chunks, stream);
    launch_wide_fwd(2, pl.args, pl.lane_bytes, pl.n_chunks, stream);
    return TRRE_OK;
}
// length-preserving without a window form: the emit pass alone, every lane writing its lines where it read them
int route_lp_direct(trre_prog* p, int family, LaunchPlan& pl, hipStream_t stream) {
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
int route_large_table_copy(trre_prog* p, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
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
int route_large_table_pair(trre_prog* p, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
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
int route_one_walk(trre_prog* p, ScanCtx* cx, const trre::StreamTables& stt, const LaunchPlan& pl, hipStream_t stream) {
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
int route_small_pair(trre_prog* p, ScanCtx* cx, int family, LaunchPlan& pl, hipStream_t stream) {
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
int route_direct_general(trre_prog* p, ScanCtx* cx, int family, LaunchPlan& pl, hipStream_t stream) {
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
int route_tile_pair(trre_prog* p, ScanCtx* cx, LaunchPlan& pl, hipStream_t stream) {
    using namespace trre;
    launch_tile_kernel(1, p->engine, p->mask_bytes, pl.args, pl.n_chunks, stream);
    launch_chunk_scan(cx->d_chunk_total, cx->d_chunk_base, pl.n_chunks, stream);
    launch_tile_kernel(2, p->engine, p->mask_bytes, pl.args, pl.n_chunks, stream);
    return TRRE_OK;
}

int launch_route(trre_prog* p, DeviceState* st, ScanCtx* cx, int family, LaunchPlan& pl, hipStream_t stream) {
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
int repair_bytemap_nuls(DeviceState* st, ScanCtx* cx, const Pending& was, size_t* out_len) {
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
int finish_inner(trre_prog* p, DeviceState* st, ScanCtx* cx, size_t* out_len);

// the status word and the output size come down; the stream is idle afterwards
int fetch_status(ScanCtx* cx, const Pending& was, uint32_t* status) {
    HIP_TRY(hipMemcpyAsync(cx->h_status, cx->d_status, 8, hipMemcpyDeviceToHost, was.stream));
    if (was.total_at) HIP_TRY(hipMemcpyAsync(cx->h_status + 2, was.total_at, 8, hipMemcpyDeviceToHost, was.stream));
    HIP_TRY(hipStreamSynchronize(was.stream));
    *status = cx->h_status[0];
    return TRRE_OK;
}

// The same scan again — as `family`, over the first n bytes — with one route switched off (`off`, a flag of the context; null: none): counted
// as a relaunch, enqueued, finished, the flag restored on every path.  hold false: the flag covers the enqueue alone, and whatever the
// finish has to run again sees it cleared (the exact sub-ranges: a rerun of the rerun tries them afresh).
int rerun(const Finishing& f, int family, bool ScanCtx::*off = nullptr, bool hold = true, size_t n = ~(size_t)0) {
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
int lazy_rounds(const Finishing& f, uint32_t* status_io) {
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
int exact_emit_again(const Finishing& f, trre::ScanArgs& xa) {
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
int exact_repair_backward(const Finishing& f, uint32_t rev_misses, uint32_t* misses, uint32_t* status) {
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
int exact_repair(const Finishing& f, uint32_t* status) {
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
int profile_dumps(ScanCtx* cx, const Pending& was) {
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
int report_divergence(const Finishing& f) {
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
int backtrack_retry(const Finishing& f) {
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
int one_pass_outcome(const Finishing& f, uint32_t status) {
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
int finish_inner(trre_prog* p, DeviceState* st, ScanCtx* cx, size_t* out_len) {
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
int finish_guarded(trre_prog* p, DeviceState* st, ScanCtx* cx, size_t* out_len) {
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


int compile_impl(const std::string& pattern, int engine, trre_prog** out, int mode = TRRE_MODE_SCAN) {
    using namespace trre;
    if (!out) return fail(TRRE_E_ARG, "error: null output handle");
    *out = nullptr;
    if (engine != TRRE_ENGINE_NFT && engine != TRRE_ENGINE_DFT) return fail(TRRE_E_ARG, "error: unknown engine");
    if (mode != TRRE_MODE_SCAN && mode != TRRE_MODE_MATCH && mode != TRRE_MODE_FIND && mode != TRRE_MODE_SPANS && mode != TRRE_MODE_SUB && !is_generate(mode))
        return fail(TRRE_E_ARG, "error: unknown mode");
    if (mode == TRRE_MODE_SUB && engine != TRRE_ENGINE_NFT)
        return fail(TRRE_E_UNSUPPORTED, "error: sub mode is offered for the non-deterministic engine only (the deterministic engine's matches cannot be told from its raw bytes by the reference)");
    if (mode == TRRE_MODE_SPANS && engine != TRRE_ENGINE_NFT)
        return fail(TRRE_E_UNSUPPORTED, "error: spans mode is offered for the non-deterministic engine only (the deterministic engine's matches cannot be told from its raw bytes by the reference)");
    if (mode == TRRE_MODE_FIND && engine != TRRE_ENGINE_NFT)
        return fail(TRRE_E_UNSUPPORTED, "error: find mode is offered for the non-deterministic engine only (the deterministic engine's matches cannot be told from its raw bytes by the reference)");
    if (mode == TRRE_MODE_MATCH && engine != TRRE_ENGINE_NFT)
        return fail(TRRE_E_UNSUPPORTED, "error: match mode is offered for the non-deterministic engine only (trre_dft -m prints empty lines)");
    if (is_generate(mode) && engine != TRRE_ENGINE_NFT) return fail(TRRE_E_UNSUPPORTED, "Not supported yet");   // trre_dft.c:1227-1229
    try {
        std::unique_ptr<trre_prog> p(new trre_prog);
        p->engine = engine;
        p->mode = mode;
        Ast ast = parse_pattern(pattern);
        Nft nft = build_nft(ast, engine == TRRE_ENGINE_DFT);
        p->nft_states = (uint32_t)nft.st.size();
        p->nft_cons = (uint32_t)nft.n_cons;
        p->prints_newline = nft_prints_newline(nft);
        // the stack guard (guard_block.hpp): the NFT itself, for the lines long enough to exhaust the reference's stack
        auto make_guard = [&](bool match) {
            p->guard = build_guard(nft);
            if (!p->guard.on) return;
            GuardBlobHeader gh{};
            gh.magic = kMagicGuard;
            gh.n_states = (uint32_t)nft.st.size();
            gh.start = p->guard.start;
            gh.d = p->guard.d;
            gh.l_min = p->guard.l_min;
            gh.window = p->guard.window;
            gh.off_states = (uint32_t)sizeof gh;
            gh.total_bytes = (uint32_t)(sizeof gh + p->guard.states.size() * 4);
            gh.match = match ? 1u : 0u;
            gh.n_once = p->guard.n_once;
            for (int k = 0; k < 8; ++k) gh.bset[k] = p->guard.bset[k];
            put(p->kblob, 0, &gh, 1);
            put(p->kblob, gh.off_states, p->guard.states.data(), p->guard.states.size());
        };
        if (engine == TRRE_ENGINE_DFT) {
            p->dft_nft = nft;
            std::unique_ptr<Dft> eager;
            try {
                eager.reset(new Dft(determinize(nft)));
            } catch (const Error& e) {
                if (e.code != kErrTooBig) throw;
                // The eager construction does not end within its caps — a state per run length ('((a:x)*b)|((a:y)*c)'), 2^19 states
                // ('(a|b)*a(a|b){18}:x').  The reference builds only the states its input visits (trre_dft.c:1135-1175) and so does
                // the lazy family (lazy_block.hpp; rounds 1-4: TRRE_E_TOO_BIG).
            }
            if (!eager) {
                p->lazy_only = true;
                const int lrc = lazy_ensure(p.get());
                if (lrc) return lrc;
                *out = p.release();
                return TRRE_OK;
            }
            Dft& dft = *eager;
            p->dt = flatten_dft(dft);
            serialize_dft(*p);
            p->has_engine_tables = true;
            p->stt = build_stream_dft(dft);
            // the guided route (guided_build.cpp: GuidedDftBuilder): what a pattern whose scan loop does not fold runs on ('[a-z]+ing:X':
            // a loop before the decision), and what takes over when a bounded fold overflows ('a*b:x' behind a run of 65 a's) — the
            // tile kernels remain for tables beyond its limits.  (A byte map needs neither.)
            if (!(p->dt.flags & kFlagMemoryless)) p->gt = build_guided_dft(dft);
        } else if (is_generate(mode)) {
            // trre -a / -ma: every accepting path prints (generate.cpp): a viability DFA for the device, the lists for the host
            p->gen = build_gen_tables(nft, mode == TRRE_MODE_MATCH_ALL);      // (always ok since round 5: beyond 256 viability states the filter lets everything through)
            p->nft_nodes = (uint32_t)p->gen.nodes.node.size();
            serialize_rev_table(p->gen.n_rev, p->gen.n_cls, 8, p->gen.cls, p->gen.rev, p->rblob);
            serialize_gen(p->gen, p->nblob);
        } else if (mode == TRRE_MODE_MATCH) {
            // trre -m: one attempt per line, accepted at its end only — the guided tables in match form
            const NftNodes nodes = build_nft_nodes(nft, true);
            p->nft_nodes = (uint32_t)nodes.node.size();
            p->gt = build_guided_nft(nodes);
            // beyond the guided tables' limits (a backward automaton of more than 16 384 states): the search itself in match form
            // (gen_block.hpp: bt_lane; round 4: TRRE_E_UNSUPPORTED) — and on request for any pattern (the parity tests)
            {
                GenTables lists;
                lists.nodes = nodes;
                lists.match_mode = true;
                lists.ok = true;
                serialize_gen(lists, p->nblob);
                p->bt_ok = true;
            }
            make_guard(true);
        } else if (mode == TRRE_MODE_FIND) {
            // trre_find_device_strings: the scan loop's nodes under two forward tables over one backward DFA (guided_build.cpp: find_cell).
            // This program keeps the texts table; the marks table lives in an inner program, which also carries the stack guard — its
            // scan runs first.  Nothing else can run a find program: no tables, no find (the backtracking lists are kept so that
            // trre_set_kernel can name that family and the find call can refuse it)
            const NftNodes nodes = build_nft_nodes(nft);
            p->nft_nodes = (uint32_t)nodes.node.size();
            std::unique_ptr<trre_prog> marks(new trre_prog);
            if (!build_guided_find(nodes, p->gt, marks->gt))
                return fail(TRRE_E_UNSUPPORTED, "error: find mode runs on the guided tables, and this pattern is beyond their limits (a backward automaton of more than 16 384 states)");
            marks->engine = engine; marks->mode = mode;
            marks->nft_states = p->nft_states; marks->nft_cons = p->nft_cons; marks->nft_nodes = p->nft_nodes;
            marks->prints_newline = p->prints_newline;
            serialize_stream(marks->gt.fwd, marks->gblob);
            serialize_rev(marks->gt, marks->rblob);
            {
                GenTables lists;
                lists.nodes = nodes;
                lists.ok = true;
                serialize_gen(lists, p->nblob);
                p->bt_ok = true;
            }
            make_guard(false);
            marks->guard = std::move(p->guard);
            marks->kblob = std::move(p->kblob);
            p->guard = GuardTables();
            p->kblob.clear();
            p->find_marks = std::move(marks);
        } else if (mode == TRRE_MODE_SPANS) {
            // trre_span_device_strings: the scan loop's nodes under ONE forward table that prints markers and position bytes
            // (guided_build.cpp: span_cell).  Nothing else can run a spans program: no other tables (the backtracking lists are
            // kept so that trre_set_kernel can name that family and the span call can refuse it); the stack guard as in scan mode
            const NftNodes nodes = build_nft_nodes(nft);
            p->nft_nodes = (uint32_t)nodes.node.size();
            p->gt = build_guided_spans(nodes);
            if (!p->gt.ok)
                return fail(TRRE_E_UNSUPPORTED, "error: spans mode runs on the guided tables, and this pattern is beyond their limits (a backward automaton of more than 16 384 states)");
            {
                GenTables lists;
                lists.nodes = nodes;
                lists.ok = true;
                serialize_gen(lists, p->nblob);
                p->bt_ok = true;
            }
            make_guard(false);
        } else if (mode == TRRE_MODE_SUB) {
            // trre_sub_device_strings: the scan loop's nodes, built once, under two tables: this program keeps the markers' table of spans
            // mode and carries the stack guard — its scan runs first —; an inner program, held as find mode holds its marks program, keeps
            // the texts table of find mode (the marks table built with it is dropped).  Nothing else can run a sub program
            const NftNodes nodes = build_nft_nodes(nft);
            p->nft_nodes = (uint32_t)nodes.node.size();
            p->gt = build_guided_spans(nodes);
            std::unique_ptr<trre_prog> texts(new trre_prog);
            GuidedTables marks_gt;
            if (!p->gt.ok || !build_guided_find(nodes, texts->gt, marks_gt))
                return fail(TRRE_E_UNSUPPORTED, "error: sub mode runs on the guided tables, and this pattern is beyond their limits (a backward automaton of more than 16 384 states)");
            texts->engine = engine; texts->mode = TRRE_MODE_FIND;
            texts->nft_states = p->nft_states; texts->nft_cons = p->nft_cons; texts->nft_nodes = p->nft_nodes;
            texts->prints_newline = p->prints_newline;
            serialize_stream(texts->gt.fwd, texts->gblob);
            serialize_rev(texts->gt, texts->rblob);
            {
                GenTables lists;
                lists.nodes = nodes;
                lists.ok = true;
                serialize_gen(lists, p->nblob);
                p->bt_ok = true;
            }
            make_guard(false);
            p->sub_texts = std::move(texts);
        } else {
            // TRRE_TRACE=1: the stages of the NFT compile on stderr as they start (to find the one a pattern is slow in)
            auto trace = [&](const char* what) { if (switches().trace) fprintf(stderr, "compile: %s\n", what); };
            trace("nodes");
            const NftNodes nodes = build_nft_nodes(nft);
            p->nft_nodes = (uint32_t)nodes.node.size();
            std::unique_ptr<Error> deferred;
            trace("bitmask tables");
            try {
                p->nt = build_nft_tables(nodes);
                p->mask_bytes = p->nt.n_cons <= 8 ? 1 : p->nt.n_cons <= 16 ? 2 : p->nt.n_cons <= 32 ? 4 : 8;
                serialize_nft(*p);
                p->has_engine_tables = true;
            } catch (const Error& e) {
                if (e.code != kErrUnsupported) throw;
                deferred.reset(new Error(e));            // too many nodes (or an epsilon cycle) for the bitmask kernels
            }
            // the fold walks the follow lists (TRRE_NFT_FOLD=states: the NFT's states as the reference does, =both: both, compared)
            const char* fold = nft_fold_now();
            trace("fold");
            if (fold && !strcmp(fold, "states")) {
                p->stt = build_stream_nft(nft);
            } else {
                p->stt = build_stream_nodes(nodes);
                if (fold && !strcmp(fold, "both")) {
                    const StreamTables ref = build_stream_nft(nft);
                    // (the walk over the states may run out of budget where this one does not: no table to compare then)
                    if (ref.ok && !p->stt.ok) throw Error(kErrArg, "error: the fold over the follow lists gave up where the one over the states did not (TRRE_NFT_FOLD=both)");
                    if (ref.ok)
                    if (ref.ent != p->stt.ent || ref.pool != p->stt.pool || ref.cls != p->stt.cls || ref.flags != p->stt.flags ||
                        ref.pending_len != p->stt.pending_len || ref.lpw != p->stt.lpw || ref.g16 != p->stt.g16 || ref.fb_comb != p->stt.fb_comb)
                        throw Error(kErrArg, "error: the two folds of the NFT scan loop disagree (TRRE_NFT_FOLD=both)");
                }
            }
            trace("guided tables");
            p->gt = build_guided_nft(nodes);
            trace("done");
            // The backtracking fallback (gen_block.hpp: bt_lane) runs what no table form holds — more than 64 nodes with a backward
            // automaton beyond the guided limits and no fold (round 3: TRRE_E_UNSUPPORTED) — and can be asked for on any pattern
            // (trre_set_kernel: the differential tests do).  Its tables are the follow lists themselves.
            {
                GenTables lists;
                lists.nodes = nodes;
                lists.ok = true;
                serialize_gen(lists, p->nblob);
                p->bt_ok = true;
            }
            make_guard(false);
        }
        if (p->stt.ok) serialize_stream(p->stt, p->sblob);
        if (p->gt.ok) { serialize_stream(p->gt.fwd, p->gblob); serialize_rev(p->gt, p->rblob); }
        if (p->gt.ok && !p->gt.accept.empty()) {
            std::vector<uint32_t> bits((p->gt.accept.size() + 31) / 32, 0u);
            for (size_t y = 0; y < p->gt.accept.size(); ++y)
                if (p->gt.accept[y]) bits[y >> 5] |= 1u << (y & 31);
            put(p->ablob, 0, bits.data(), bits.size());
        }
        *out = p.release();
        return TRRE_OK;
    } catch (const Error& e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc&) {
        return fail(TRRE_E_TOO_BIG, "error: out of memory while compiling the pattern");
    }
}

}  // namespace

extern "C" {

int trre_compile(const char* pattern, int engine, trre_prog** out) {
    if (!pattern) return fail(TRRE_E_ARG, "error: missing trre expression");
    return compile_impl(std::string(pattern), engine, out);
}

int trre_compile_bytes(const uint8_t* pattern, size_t len, int engine, trre_prog** out) {
    if (!pattern) return fail(TRRE_E_ARG, "error: missing trre expression");
    return compile_impl(std::string(reinterpret_cast<const char*>(pattern), len), engine, out);
}

int trre_compile_mode(const uint8_t* pattern, size_t len, int engine, int mode, trre_prog** out) {
    if (!pattern) return fail(TRRE_E_ARG, "error: missing trre expression");
    return compile_impl(std::string(reinterpret_cast<const char*>(pattern), len), engine, out, mode);
}

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

static size_t export_blob(const std::vector<uint8_t>& b, void* buf, size_t cap) {
    if (buf && cap) std::memcpy(buf, b.data(), cap < b.size() ? cap : b.size());
    return b.size();
}
size_t trre_export_tables(const trre_prog* p, void* buf, size_t cap) { return p ? export_blob(p->blob, buf, cap) : 0; }
size_t trre_export_stream_tables(const trre_prog* p, void* buf, size_t cap) { return p ? export_blob(p->sblob, buf, cap) : 0; }

size_t trre_export_guided_tables(const trre_prog* p, int which, void* buf, size_t cap) {
    if (!p) return 0;
    if (which == 5 && p->sub_texts) return export_blob(p->sub_texts->gblob, buf, cap);      // (sub mode: the inner program's texts table)
    if (which == 5 || which == 6)                                     // (find mode: the texts / the marks forward tables; the backward DFA, 0, is one)
        return p->find_marks ? export_blob(which == 5 ? p->gblob : p->find_marks->gblob, buf, cap) : 0;
    if (which == 7) return p->mode == TRRE_MODE_SPANS || p->mode == TRRE_MODE_SUB ? export_blob(p->gblob, buf, cap) : 0;     // (spans mode: the markers' forward table)
    if (which == 3 && p->find_marks) return export_blob(p->find_marks->kblob, buf, cap);     // (find mode: the guard goes with the scan that runs first)
    if (which == 4) return export_blob(p->gt.accept, buf, cap);       // (match mode: a byte per backward state, 1: a line that starts with the symbol is accepted)
    return export_blob(which == 0 ? p->rblob : (which == 2 ? p->nblob : (which == 3 ? p->kblob : p->gblob)), buf, cap);   // (2: the enumeration's / the backtracking fallback's tables, 3: the stack guard's)
}

// CPU test tier (tests/cpu_shim.cpp runs lazy_block.hpp's lane body on the host): the lazy tables as they stand — which 0: u32 n_cls, u32 rows,
// then cls[256]; 1: the entries; 2: the pool — and the exploration of a list of misses.  Host only.
size_t trre_debug_lazy_tables(trre_prog* p, int which, void* buf, size_t cap) {
    if (!p || p->engine != TRRE_ENGINE_DFT || p->mode != TRRE_MODE_SCAN || lazy_ensure(p)) return 0;
    std::lock_guard<std::mutex> lock(p->lazy_mu);
    const trre::LazyDft& z = *p->lazy;
    std::vector<uint8_t> head;
    const void* src;
    size_t n;
    if (which == 0) {
        const uint32_t w[2] = {z.n_cls(), z.n_rows()};
        put(head, 0, w, 2);
        put(head, 8, z.cls(), 256);
        src = head.data(); n = head.size();
    } else if (which == 1) {
        src = z.ent(); n = (size_t)z.n_rows() * z.n_cls() * 8;
    } else {
        src = z.pool(); n = z.pool_bytes();
    }
    if (buf && cap) std::memcpy(buf, src, cap < n ? cap : n);
    return n;
}
int trre_debug_lazy_explore(trre_prog* p, const uint32_t* misses, size_t n, size_t spec_states) {
    if (!p || p->engine != TRRE_ENGINE_DFT || p->mode != TRRE_MODE_SCAN) return fail(TRRE_E_ARG, "error: no lazy tables");
    const int rc = lazy_ensure(p);
    if (rc) return rc;
    try {
        std::lock_guard<std::mutex> lock(p->lazy_mu);
        p->lazy->explore(misses, n, spec_states);
    } catch (const trre::Error& e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc&) {
        return fail(TRRE_E_TOO_BIG, "error: out of memory while determinising");
    }
    return TRRE_OK;
}

// [a, a + n) and [b, b + m) share a byte (no pointer is dereferenced, no sum can wrap)
static bool ranges_overlap(const void* a, size_t n, const void* b, size_t m) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return n && m && (x >= y ? x - y < m : y - x < n);
}

// the device path: d_in == d_out is a scan in place; any other overlap is refused before anything touches the device
static int device_overlap(const uint8_t* d_in, size_t n, const uint8_t* d_out, size_t cap) {
    if (d_in != d_out && ranges_overlap(d_in, n, d_out, cap))
        return fail(TRRE_E_ARG, "error: input and output overlap (only d_in == d_out, a scan in place, is allowed)");
    return TRRE_OK;
}

// the prog's state on the calling thread's current device
static int current_state(trre_prog* p, DeviceState** st) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    return device_state(p, dev, st);
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

namespace {
int slot_reserve(DeviceState::HostSlot& hs, bool input, size_t bytes, bool need_pin = true);
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
}  // namespace

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

// ---- the host passes the column calls share (records_block.hpp) ----------------------------------------------
// ScanCtx::d_rec: the status word, then part [tiles + 1], cnt [tiles], base [tiles + 1] for the tiles of the pass that runs
struct RecCarve {
    int64_t* part;
    uint64_t* cnt;
    uint64_t* base;
};
static hipError_t rec_room(ScanCtx* cx, int64_t tiles) { return cx->d_rec.reserve((size_t)tiles, (size_t)(3 * tiles + 3) * 8); }
// room for `tiles`, then the three arrays: carved after growing, which moves them
static int rec_carve(ScanCtx* cx, int64_t tiles, RecCarve* c) {
    HIP_TRY(rec_room(cx, tiles));
    c->part = reinterpret_cast<int64_t*>(cx->d_rec + 1);
    c->cnt = cx->d_rec + 2 + tiles;
    c->base = cx->d_rec + 2 + 2 * tiles;
    return TRRE_OK;
}
static int rec_status(ScanCtx* cx, hipStream_t s, uint64_t* extra_dev, uint64_t* extra) {
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, cx->d_rec, 4, hipMemcpyDeviceToHost, s));
    if (extra_dev) HIP_TRY(hipMemcpyAsync(extra, extra_dev, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return bad ? 1 : 0;
}

// The caller's offsets, on the device, before anything of the caller's is written: k_rec_check and its status word.  d_rec
// first gets room for `tiles`, the tiles the caller stages next (the status word at the least).
static int rec_check_offsets(ScanCtx* cx, int64_t tiles, const int64_t* d_off, size_t nrec, size_t n, hipStream_t s) {
    HIP_TRY(rec_room(cx, std::max<int64_t>(tiles, 1)));
    HIP_TRY(hipMemsetAsync(cx->d_rec, 0, 8, s));
    trre::launch_rec_check(d_off, (int64_t)nrec, (int64_t)n, reinterpret_cast<uint32_t*>(cx->d_rec.p), s);
    const int bad = rec_status(cx, s, nullptr, nullptr);
    if (bad < 0) return TRRE_E_DEVICE;
    return bad ? fail(TRRE_E_ARG, "error: record offsets must start at 0, end at n and never decrease") : TRRE_OK;
}

// The staged text of a column of strings, n + nrec bytes in d_snap (16-byte aligned, whole vectors): k_str_part(0), k_str_stage,
// k_chunk_scan.  The stage pass leaves the strings' tile-local ranks in `ranks` [nrec + 1]; *sa is what the passes ran with, for
// k_str_rank where the caller wants the ranks whole.
static int str_stage_text(ScanCtx* cx, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t* ranks, hipStream_t s,
                          trre::StrArgs* sa) {
    using namespace trre;
    const int64_t T = str_tile_bytes();
    const int64_t total = (int64_t)(n + nrec), tiles = (total + T - 1) / T;
    HIP_TRY(cx->d_snap.reserve((size_t)total + 64, (size_t)total + 64));
    RecCarve c;
    const int rc = rec_carve(cx, tiles, &c);
    if (rc) return rc;
    const int64_t a0 = (int64_t)(reinterpret_cast<uintptr_t>(d_in) & 15u);
    *sa = StrArgs{};
    sa->src_v0 = d_in - a0; sa->vbeg = a0; sa->total = total; sa->dst = cx->d_snap;
    sa->off = d_off; sa->nrec = (int64_t)nrec; sa->out_off = ranks;
    sa->part = c.part; sa->cnt = c.cnt; sa->base = c.base;
    launch_str_part(0, *sa, c.part, tiles, s);
    launch_str_stage(*sa, tiles, s);
    launch_chunk_scan(c.cnt, c.base, tiles, s);
    return TRRE_OK;
}
// ... and its newline total, base[tiles] of those passes, read back: nrec exactly when no string holds a '\n'
static int str_staged_newlines(ScanCtx* cx, const trre::StrArgs& sa, hipStream_t s, uint64_t* total) {
    const int64_t T = trre::str_tile_bytes();
    return rec_status(cx, s, const_cast<uint64_t*>(sa.base) + (sa.total + T - 1) / T, total);
}

// Record i's output ends just past newline number R_i of the text [vbeg, vend) over in_v0, R_i parked in out_off[i + 1]:
// k_rec_count, k_chunk_scan, k_rec_part(1), k_rec_locate put the end in its place.  One read-back: 1 when a rank fell outside
// its tile, *last = out_off[nrec] and, where the caller asks for it, *newlines = the text's newline total.
static int rec_locate_ends(ScanCtx* cx, const uint8_t* in_v0, int64_t vbeg, int64_t vend, size_t nrec, int64_t* out_off, hipStream_t s,
                           uint64_t* last, uint64_t* newlines) {
    using namespace trre;
    const int64_t T = rec_tile_bytes(), tiles = (vend + T - 1) / T;
    RecCarve c;
    const int rc = rec_carve(cx, tiles, &c);
    if (rc) return rc;
    RecArgs a{};
    a.in_v0 = in_v0; a.vbeg = vbeg; a.vend = vend; a.nrec = (int64_t)nrec; a.out_off = out_off;
    a.part = c.part; a.cnt = c.cnt; a.base = c.base;
    HIP_TRY(hipMemsetAsync(cx->d_rec, 0, 8, s));
    launch_rec_count(a, tiles, s);
    launch_chunk_scan(c.cnt, c.base, tiles, s);
    launch_rec_part(1, a, tiles, s);
    launch_rec_locate(a, tiles, reinterpret_cast<uint32_t*>(cx->d_rec.p), s);
    if (newlines) HIP_TRY(hipMemcpyAsync(newlines, c.base + tiles, 8, hipMemcpyDeviceToHost, s));
    return rec_status(cx, s, reinterpret_cast<uint64_t*>(out_off + nrec), last);
}

// '\n' per string tile (16 KiB) of a framed text of m bytes and before every tile: k_match_count, k_chunk_scan into a fresh
// carve; *base [tiles + 1]
static int str_tile_newlines(ScanCtx* cx, const uint8_t* framed, int64_t m, hipStream_t s, const uint64_t** base) {
    using namespace trre;
    const int64_t T = str_tile_bytes(), tiles = (m + T - 1) / T;
    RecCarve c;
    const int rc = rec_carve(cx, tiles, &c);
    if (rc) return rc;
    RecArgs a{};
    a.in_v0 = framed; a.vbeg = 0; a.vend = m;
    a.part = c.part; a.cnt = c.cnt; a.base = c.base;
    launch_match_count(a, tiles, s);
    launch_chunk_scan(c.cnt, c.base, tiles, s);
    *base = c.base;
    return TRRE_OK;
}

// A framed text of m bytes without its nrec closing newlines into dst, by the located offsets in out_off, which become the
// final ones: k_str_part(1), k_str_unframe
static int str_unframe_located(ScanCtx* cx, const uint8_t* framed, int64_t m, uint8_t* dst, size_t nrec, int64_t* out_off, hipStream_t s) {
    using namespace trre;
    const int64_t T = str_tile_bytes(), tiles = (m + T - 1) / T;
    RecCarve c;
    const int rc = rec_carve(cx, tiles, &c);
    if (rc) return rc;
    StrArgs a{};
    a.src_v0 = framed; a.total = m; a.dst = dst; a.dst_len = m - (int64_t)nrec;
    a.nrec = (int64_t)nrec; a.out_off = out_off; a.part = c.part;
    launch_str_part(1, a, c.part, tiles, s);
    launch_str_unframe(a, tiles, s);
    HIP_TRY(hipGetLastError());
    return TRRE_OK;
}

// k_chunk_scan over each of `count` arrays, cnt [count][tiles] into base [count][tiles + 1], and the totals' read-backs queued
// into tot: the caller synchronises
static int scan_counts(const uint64_t* cnt, const uint64_t* base, int count, int64_t tiles, hipStream_t s, uint64_t* tot) {
    for (int k = 0; k < count; ++k) {
        uint64_t* b = const_cast<uint64_t*>(base) + k * (tiles + 1);
        trre::launch_chunk_scan(cnt + k * tiles, b, tiles, s);
        HIP_TRY(hipMemcpyAsync(&tot[k], b + tiles, 8, hipMemcpyDeviceToHost, s));
    }
    return TRRE_OK;
}

// ---- what the column calls' entry points share ----------------------------------------------------------------------------
struct Range { const void* p; size_t bytes; };
// a range of `more` overlaps one of `have` or another of `more` (the pairs within `have` are the caller's: d_in == d_out may be
// a scan in place)
static bool any_overlap(std::initializer_list<Range> have, std::initializer_list<Range> more) {
    for (const Range* a = more.begin(); a != more.end(); ++a) {
        for (const Range& h : have)
            if (ranges_overlap(a->p, a->bytes, h.p, h.bytes)) return true;
        for (const Range* b = a + 1; b != more.end(); ++b)
            if (ranges_overlap(a->p, a->bytes, b->p, b->bytes)) return true;
    }
    return false;
}

// the program of the span, split, filter and field calls; `noun`: what the refusing call makes
static int spans_program(const trre_prog* p, const char* noun) {
    if (p->mode == TRRE_MODE_SUB) return fail(TRRE_E_ARG, kSubOnlyMsg);
    if (p->mode != TRRE_MODE_SPANS || !p->gt.ok) return fail(TRRE_E_ARG, std::string("error: ") + noun + " take a program compiled with TRRE_MODE_SPANS");
    if (p->forced_family == TRRE_KERNEL_BACKTRACK)
        return fail(TRRE_E_UNSUPPORTED, "error: spans mode runs on the guided tables, which this program was told not to use (the backtracking family)");
    return TRRE_OK;
}

// The prog's state on the current device, locked until the call returns — one column call at a time per (prog, device) —, and
// no split-form scan in flight.  inner: the find call's inner program, reached through that call only: the outer lock covers it.
struct ColumnCall {
    DeviceState* st = nullptr;
    DeviceState* inner = nullptr;
    std::unique_lock<std::mutex> lock;
    int begin(trre_prog* p, trre_prog* inner_prog = nullptr) {
        int rc = current_state(p, &st);
        if (!rc && inner_prog) rc = current_state(inner_prog, &inner);
        if (rc) return rc;
        lock = std::unique_lock<std::mutex>(st->mu);
        if (st->ctx.pend.active) return fail(TRRE_E_ARG, "error: a split-form scan is still in flight on this device: call trre_scan_finish first");
        return TRRE_OK;
    }
};

// ---- ragged records (records_block.hpp) ----------------------------------------------------------------------------------
static int records_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out,
                      size_t cap, int64_t* d_out_off, size_t* out_len, hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    const int64_t T = rec_tile_bytes();
    const int64_t a0 = (int64_t)(reinterpret_cast<uintptr_t>(d_in) & 15u);
    const int64_t tiles = n ? (a0 + (int64_t)n + T - 1) / T : 0;
    // 1. the offsets, on the device: nothing is written before they pass
    int rc = rec_check_offsets(cx, tiles, d_off, nrec, n, s);
    if (rc) return rc;
    if (n == 0) {                                        // every record is empty
        HIP_TRY(hipMemsetAsync(d_out_off, 0, (nrec + 1) * 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 2. the staged copy (the snapshot buffer, at the input's offset mod 16, whole 16-byte vectors) and the ranks
    HIP_TRY(cx->d_snap.reserve(n + 32, n + 32));
    RecArgs ra{};
    ra.in_v0 = d_in - a0; ra.snap_v0 = cx->d_snap; ra.vbeg = a0; ra.vend = a0 + (int64_t)n;
    ra.off = d_off; ra.nrec = (int64_t)nrec; ra.out_off = d_out_off; ra.keep = d_in == d_out ? 1u : 0u;
    RecCarve c;
    rc = rec_carve(cx, tiles, &c);
    if (rc) return rc;
    ra.part = c.part; ra.cnt = c.cnt; ra.base = c.base;
    launch_rec_part(0, ra, tiles, s);
    launch_rec_stage(ra, tiles, s);
    launch_chunk_scan(ra.cnt, const_cast<uint64_t*>(ra.base), tiles, s);
    launch_rec_rank(ra, s);
    // 3. the plain scan of the staged copy, family as chosen for the program
    rc = enqueue(p, st, cx, scan_family(*p), cx->d_snap + a0, n, d_out, cap, s);
    if (rc) { cx->pend = Pending(); return rc; }
    size_t m = 0;
    rc = finish(p, st, cx, &m);
    if (out_len) *out_len = m;
    if (rc == TRRE_E_CAPACITY && ra.keep) {               // in place: the caller's buffer holds the input again for the retry
        HIP_TRY(hipMemcpyAsync(d_out, cx->d_snap + a0, n, hipMemcpyDeviceToDevice, s));
        launch_rec_restore(ra, d_out, s);
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (rc) return rc;
    if (m == 0) {
        HIP_TRY(hipMemsetAsync(d_out_off, 0, (nrec + 1) * 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 4. record i's output ends just past output newline number R_i
    const int64_t b0 = (int64_t)(reinterpret_cast<uintptr_t>(d_out) & 15u);
    uint64_t last = 0;
    const int lost = rec_locate_ends(cx, d_out - b0, b0, b0 + (int64_t)m, nrec, d_out_off, s, &last, nullptr);
    if (lost < 0) return TRRE_E_DEVICE;
    if (lost || last != m) return fail(TRRE_E_DEVICE, "error: the records' output offsets do not add up (internal)");
    return TRRE_OK;
}

int trre_scan_device_records(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out, size_t cap,
                             int64_t* d_out_off, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (!p || !d_off || !d_out_off || (n && (!d_in || !d_out))) return fail(TRRE_E_ARG, "error: null argument");
    if (own_call_only(*p)) return fail(TRRE_E_ARG, own_call_only(*p));
    if (p->mode != TRRE_MODE_SCAN)
        return fail(TRRE_E_UNSUPPORTED, "error: records are offered in scan mode only (a line of -m, -a, -ma prints zero or many newlines)");
    if (p->prints_newline)
        return fail(TRRE_E_UNSUPPORTED, "error: the pattern can print a newline of its own: record outputs could not be told apart");
    if (nrec >= ((size_t)1 << 58) || n >= ((size_t)1 << 56)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    if (device_overlap(d_in, n, d_out, cap)) return TRRE_E_ARG;
    const size_t ob = (nrec + 1) * 8;
    if (any_overlap({{d_in, n}, {d_out, cap}}, {{d_off, ob}, {d_out_off, ob}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or the other offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p)) return rc;
    return records_on(p, c.st, d_in, n, d_off, nrec, d_out, cap, d_out_off, out_len, static_cast<hipStream_t>(stream));
}

// ---- packed strings (records_block.hpp) ------------------------------------------------------------------------------------
// d_rec holds the passes' arrays over string tiles (16 KiB) while staging and unframing, over record tiles (64 KiB) in between
static int strings_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out,
                      size_t cap, int64_t* d_out_off, size_t* out_len, hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    const int64_t T = str_tile_bytes();
    const int64_t total = (int64_t)(n + nrec);                     // the staged text
    // 1. the offsets, on the device: nothing is written before they pass
    int rc = rec_check_offsets(cx, (total + T - 1) / T, d_off, nrec, n, s);
    if (rc) return rc;
    if (nrec == 0) {
        HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 2. the staged text (the snapshot buffer, 16-byte aligned, whole vectors) and the ranks
    StrArgs sa;
    rc = str_stage_text(cx, d_in, n, d_off, nrec, d_out_off, s, &sa);
    if (rc) return rc;
    launch_str_rank(sa, s);
    // 3. the plain scan of the staged text into the framed buffer, family as chosen for the program
    const size_t fcap = cap + nrec;
    HIP_TRY(cx->d_framed.reserve(fcap + 64, fcap + 64));
    rc = enqueue(p, st, cx, scan_family(*p), cx->d_snap, (size_t)total, cx->d_framed, fcap, s);
    if (rc) { cx->pend = Pending(); return rc; }
    size_t m = 0;
    rc = finish(p, st, cx, &m);
    if (rc == TRRE_E_CAPACITY && out_len) *out_len = m >= nrec ? m - nrec : 0;
    if (rc) return rc;                                     // (TRRE_E_DIVERGES: *out_len stays 0)
    if (m < nrec) return fail(TRRE_E_DEVICE, "error: the strings' output offsets do not add up (internal)");
    // 4. record i's framed output ends just past framed newline number R_i
    uint64_t last = 0;
    const int lost = rec_locate_ends(cx, cx->d_framed, 0, (int64_t)m, nrec, d_out_off, s, &last, nullptr);
    if (lost < 0) return TRRE_E_DEVICE;
    if (lost || last != m) return fail(TRRE_E_DEVICE, "error: the strings' output offsets do not add up (internal)");
    // 5. the framed output without the closing newlines into the caller's buffer, and the final offsets
    rc = str_unframe_located(cx, cx->d_framed, (int64_t)m, d_out, nrec, d_out_off, s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (out_len) *out_len = m - nrec;
    return TRRE_OK;
}

int trre_scan_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out, size_t cap,
                             int64_t* d_out_off, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (!p || !d_off || !d_out_off || (n && !d_in) || (cap && !d_out)) return fail(TRRE_E_ARG, "error: null argument");
    if (own_call_only(*p)) return fail(TRRE_E_ARG, own_call_only(*p));
    if (p->mode != TRRE_MODE_SCAN)
        return fail(TRRE_E_UNSUPPORTED, "error: strings are offered in scan mode only (a line of -m, -a, -ma prints zero or many newlines)");
    if (p->prints_newline)
        return fail(TRRE_E_UNSUPPORTED, "error: the pattern can print a newline of its own: record outputs could not be told apart");
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    if (device_overlap(d_in, n, d_out, cap)) return TRRE_E_ARG;
    const size_t ob = (nrec + 1) * 8;
    if (any_overlap({{d_in, n}, {d_out, cap}}, {{d_off, ob}, {d_out_off, ob}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or the other offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p)) return rc;
    return strings_on(p, c.st, d_in, n, d_off, nrec, d_out, cap, d_out_off, out_len, static_cast<hipStream_t>(stream));
}

// ---- matched strings (records_block.hpp) -----------------------------------------------------------------------------------
// d_rec as for the strings call; d_match: cnt [groups], base [groups + 1] of the verdicts, kept until the final offsets
static int match_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out,
                    size_t cap, int64_t* d_out_off, uint64_t* d_valid, size_t* n_matched, size_t* out_len, hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    const int64_t T = str_tile_bytes();
    const int64_t total = (int64_t)(n + nrec);                     // the staged text
    // 1. the offsets, on the device: nothing is written before they pass
    int rc = rec_check_offsets(cx, (total + T - 1) / T, d_off, nrec, n, s);
    if (rc) return rc;
    if (nrec == 0) {
        HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 2. the staged text, as for the strings call; its '\n' are the strings' closing ones and nothing else exactly when their number is nrec
    StrArgs sa;
    rc = str_stage_text(cx, d_in, n, d_off, nrec, d_out_off, s, &sa);
    if (rc) return rc;
    uint64_t staged_nl = 0;
    if (str_staged_newlines(cx, sa, s, &staged_nl) < 0) return TRRE_E_DEVICE;
    if (staged_nl != nrec) return fail(TRRE_E_ARG, "error: a string holds a newline: it would be several lines with several verdicts");
    // 3. the plain match scan of the staged text into the framed buffer, on the general guided family: its count pass always runs, and with
    // it the backward pass, whose symbols the verdicts are read from (the length-preserving family does not launch into too small a buffer)
    const size_t fcap = cap + nrec;
    HIP_TRY(cx->d_framed.reserve(fcap + 64, fcap + 64));
    rc = enqueue(p, st, cx, TRRE_KERNEL_GUIDED_GEN, cx->d_snap, (size_t)total, cx->d_framed, fcap, s);
    if (rc) { cx->pend = Pending(); return rc; }
    size_t m = 0;
    rc = finish(p, st, cx, &m);
    if (rc && rc != TRRE_E_CAPACITY) return rc;            // (TRRE_E_DIVERGES: *out_len stays 0)
    // 4. the verdicts: the bitmap, M_i in out_off[i + 1], n_matched
    const int64_t groups = ((int64_t)nrec + kMatchThreads - 1) / kMatchThreads;
    HIP_TRY(cx->d_match.reserve((size_t)groups, (size_t)(2 * groups + 1) * 8));
    MatchArgs ma{};
    ma.sym_v0 = cx->d_sym; ma.vbeg = (int64_t)(reinterpret_cast<uintptr_t>(cx->d_snap.p) & 15u);
    ma.off = d_off; ma.nrec = (int64_t)nrec;
    ma.accept = reinterpret_cast<const uint32_t*>(st->d_ablob); ma.accept_words = (uint32_t)(p->ablob.size() / 4);
    ma.valid = d_valid; ma.words = ((int64_t)nrec + 63) / 64;
    ma.out_off = d_out_off; ma.cnt = cx->d_match; ma.base = cx->d_match + groups;
    launch_match_verdict(guided_sym_bits(*p), ma, s);
    launch_chunk_scan(ma.cnt, const_cast<uint64_t*>(ma.base), groups, s);
    launch_match_rank(ma, s);
    HIP_TRY(hipGetLastError());
    uint64_t matched = 0;
    if (rec_status(cx, s, const_cast<uint64_t*>(ma.base) + groups, &matched) < 0) return TRRE_E_DEVICE;
    if (n_matched) *n_matched = (size_t)matched;
    const size_t need = m >= matched ? m - (size_t)matched : 0;
    if (rc == TRRE_E_CAPACITY || need > cap) {
        if (out_len) *out_len = need;
        return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    }
    if (m == 0) {                                           // nothing accepted (an accepted string prints at least its framing '\n')
        if (matched) return fail(TRRE_E_DEVICE, "error: the matched strings' output offsets do not add up (internal)");
        HIP_TRY(hipMemsetAsync(d_out_off, 0, (nrec + 1) * 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 5. string i's framed output ends just past framed newline number M_i
    const int64_t utiles = ((int64_t)m + T - 1) / T;
    HIP_TRY(rec_room(cx, utiles));                          // (the compaction's tiles are the smaller ones: room for both)
    uint64_t last = 0, framed_nl = 0;
    const int lost = rec_locate_ends(cx, cx->d_framed, 0, (int64_t)m, nrec, d_out_off, s, &last, &framed_nl);
    if (lost < 0) return TRRE_E_DEVICE;
    if (lost || last != m || framed_nl != matched) return fail(TRRE_E_DEVICE, "error: the matched strings' output offsets do not add up (internal)");
    // 6. the final offsets; the framed output without its newlines into the caller's buffer
    launch_match_final(ma, s);
    const uint64_t* before = nullptr;                       // '\n' before every tile of the compaction
    rc = str_tile_newlines(cx, cx->d_framed, (int64_t)m, s, &before);
    if (rc) return rc;
    StrArgs ua{};
    ua.src_v0 = cx->d_framed; ua.total = (int64_t)m; ua.dst = d_out; ua.dst_len = (int64_t)(m - matched);
    ua.nrec = (int64_t)nrec; ua.out_off = d_out_off;
    ua.part = reinterpret_cast<const int64_t*>(before);
    launch_match_unframe(ua, utiles, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (out_len) *out_len = m - (size_t)matched;
    return TRRE_OK;
}

int trre_match_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out, size_t cap,
                              int64_t* d_out_off, uint8_t* d_valid, size_t* n_matched, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (n_matched) *n_matched = 0;
    if (!p || !d_off || !d_out_off || (n && !d_in) || (cap && !d_out) || (nrec && !d_valid)) return fail(TRRE_E_ARG, "error: null argument");
    if (p->mode == TRRE_MODE_SUB) return fail(TRRE_E_ARG, kSubOnlyMsg);
    if (p->mode != TRRE_MODE_MATCH) return fail(TRRE_E_ARG, "error: matched strings take a program compiled with TRRE_MODE_MATCH");
    if (p->prints_newline)
        return fail(TRRE_E_UNSUPPORTED, "error: the pattern can print a newline of its own: record outputs could not be told apart");
    if (!p->gt.ok || p->ablob.empty() || p->forced_family == TRRE_KERNEL_BACKTRACK)
        return fail(TRRE_E_UNSUPPORTED, "error: the verdicts come from the guided tables, which this program does not have or was told not to use (the backtracking family)");
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    if (reinterpret_cast<uintptr_t>(d_valid) & 7u) return fail(TRRE_E_ARG, "error: the validity bitmap must be 8-byte aligned (it is written as 64-bit words)");
    if (device_overlap(d_in, n, d_out, cap)) return TRRE_E_ARG;
    const size_t ob = (nrec + 1) * 8, vb = (nrec + 63) / 64 * 8;
    if (any_overlap({{d_in, n}, {d_out, cap}}, {{d_off, ob}, {d_out_off, ob}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or the other offsets array");
    if (any_overlap({{d_in, n}, {d_out, cap}, {d_off, ob}, {d_out_off, ob}}, {{d_valid, vb}}))
        return fail(TRRE_E_ARG, "error: the validity bitmap overlaps the data or an offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p)) return rc;
    return match_on(p, c.st, d_in, n, d_off, nrec, d_out, cap, d_out_off, reinterpret_cast<uint64_t*>(d_valid), n_matched, out_len,
                    static_cast<hipStream_t>(stream));
}

// ---- found strings (records_block.hpp) -------------------------------------------------------------------------------------
// One scan of the staged text under a find program's table into a buffer of the library, which grows on the size a scan reports: a
// scan that does not fit says how much it needs and runs once more.  (The staged text is the outer context's; the scan's own
// workspace — symbols, lane counts, status — is that of the program that runs.)
static int find_scan(trre_prog* p, DeviceState* st, const uint8_t* d_text, size_t total, DevBuf<uint8_t>& framed, size_t* m, hipStream_t s) {
    ScanCtx* cx = &st->ctx;
    HIP_TRY(framed.reserve(total + 64, total + 64));
    for (int round = 0;; ++round) {
        int rc = enqueue(p, st, cx, TRRE_KERNEL_GUIDED_GEN, d_text, total, framed, framed.cap - 64, s);
        if (rc) { cx->pend = Pending(); return rc; }
        rc = finish(p, st, cx, m);
        if (rc != TRRE_E_CAPACITY || round) return rc == TRRE_E_CAPACITY ? fail(TRRE_E_DEVICE, "error: a scan outgrew the size it reported (internal)") : rc;
        HIP_TRY(framed.reserve(*m + 64, *m + 64));
    }
}

// d_rec as for the strings call, of the outer program's context, which also holds the staged text (d_snap), the list offsets while
// they are being made (d_find_off), the marks unframed (d_find_marks) and the framed texts (d_framed); the inner program's context
// holds the framed marks (its d_framed)
static int find_on(trre_prog* p, DeviceState* st, DeviceState* stm, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec,
                   uint8_t* d_out, size_t cap, int64_t* d_match_off, size_t match_cap, int64_t* d_list_off, size_t* n_matches,
                   size_t* out_len, hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    const int64_t T = str_tile_bytes();
    const int64_t total = (int64_t)(n + nrec);                     // the staged text
    // 1. the offsets, on the device: nothing is written before they pass
    int rc = rec_check_offsets(cx, (total + T - 1) / T, d_off, nrec, n, s);
    if (rc) return rc;
    if (nrec == 0) {
        HIP_TRY(hipMemsetAsync(d_list_off, 0, 8, s));
        if (d_match_off) HIP_TRY(hipMemsetAsync(d_match_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 2. the staged text and the strings' ranks, as for the strings call — the ranks into the library's own array: the caller's
    // are not written before the strings have passed (3)
    HIP_TRY(cx->d_find_off.reserve(nrec + 1, (nrec + 1) * 8));
    int64_t* loff = cx->d_find_off;
    StrArgs sa;
    rc = str_stage_text(cx, d_in, n, d_off, nrec, loff, s, &sa);
    if (rc) return rc;
    launch_str_rank(sa, s);
    // 3. a string that holds a '\n' would be several lines: the staged newlines are the strings' closing ones exactly when they are nrec
    uint64_t staged_nl = 0;
    if (str_staged_newlines(cx, sa, s, &staged_nl) < 0) return TRRE_E_DEVICE;
    if (staged_nl != nrec) return fail(TRRE_E_ARG, "error: a string holds a newline: it would be several lines, each with matches of its own");
    // 4. the marks scan, and its unframing by the strings call's passes: string i's marks end just past framed newline number i + 1,
    // and the unframed offsets are the list offsets
    size_t mm = 0;
    rc = find_scan(p->find_marks.get(), stm, cx->d_snap, (size_t)total, stm->ctx.d_framed, &mm, s);
    if (rc) return rc;                                      // (TRRE_E_DIVERGES: *out_len stays 0)
    if (mm < nrec) return fail(TRRE_E_DEVICE, "error: the list offsets do not add up (internal)");
    const uint8_t* marks = stm->ctx.d_framed;
    const size_t found = mm - nrec;
    HIP_TRY(rec_room(cx, ((int64_t)mm + T - 1) / T));       // (the unframing's tiles are the smaller ones: room for both)
    HIP_TRY(cx->d_find_marks.reserve(found + 64, found + 64));
    uint64_t last = 0, marks_nl = 0;
    const int lost = rec_locate_ends(cx, marks, 0, (int64_t)mm, nrec, loff, s, &last, &marks_nl);
    if (lost < 0) return TRRE_E_DEVICE;
    if (lost || last != mm || marks_nl != nrec) return fail(TRRE_E_DEVICE, "error: the list offsets do not add up (internal)");
    rc = str_unframe_located(cx, marks, (int64_t)mm, cx->d_find_marks, nrec, loff, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_list_off, loff, (nrec + 1) * 8, hipMemcpyDeviceToDevice, s));
    // 5. the texts scan: every match's output and a '\n' — as many as there are marks
    size_t m = 0;
    rc = find_scan(p, st, cx->d_snap, (size_t)total, cx->d_framed, &m, s);
    if (rc) return rc;
    const int64_t utiles = ((int64_t)m + T - 1) / T;
    uint64_t closed = 0;
    const uint64_t* before = nullptr;                       // '\n' before every tile of the texts
    if (m) {
        rc = str_tile_newlines(cx, cx->d_framed, (int64_t)m, s, &before);
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        if (rec_status(cx, s, const_cast<uint64_t*>(before) + utiles, &closed) < 0) return TRRE_E_DEVICE;
    } else {
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (closed != found || m < found) return fail(TRRE_E_DEVICE, "error: the two scans of the strings disagree on the number of matches (internal)");
    if (n_matches) *n_matches = found;
    if (out_len) *out_len = m - found;
    if (m - found > cap || found > match_cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    // 6. the framed texts without their newlines into the caller's buffer, and where each match starts
    if (found == 0) {
        if (d_match_off) HIP_TRY(hipMemsetAsync(d_match_off, 0, 8, s));
    } else {
        StrArgs ua{};
        ua.src_v0 = cx->d_framed; ua.total = (int64_t)m; ua.dst = d_out; ua.dst_len = (int64_t)(m - found);
        ua.nrec = (int64_t)found; ua.out_off = d_match_off;
        ua.part = reinterpret_cast<const int64_t*>(before);
        launch_find_unframe(ua, utiles, s);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s));
    return TRRE_OK;
}

int trre_find_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out, size_t cap,
                             int64_t* d_match_off, size_t match_cap, int64_t* d_list_off, size_t* n_matches, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (n_matches) *n_matches = 0;
    if (!p || !d_off || !d_list_off || (n && !d_in) || (cap && !d_out) || (match_cap && !d_match_off)) return fail(TRRE_E_ARG, "error: null argument");
    if (p->mode == TRRE_MODE_SUB) return fail(TRRE_E_ARG, kSubOnlyMsg);
    if (p->mode != TRRE_MODE_FIND || !p->find_marks) return fail(TRRE_E_ARG, "error: found strings take a program compiled with TRRE_MODE_FIND");
    if (p->prints_newline)
        return fail(TRRE_E_UNSUPPORTED, "error: the pattern can print a newline of its own: the matches' outputs could not be told apart");
    if (p->forced_family == TRRE_KERNEL_BACKTRACK)
        return fail(TRRE_E_UNSUPPORTED, "error: find mode runs on the guided tables, which this program was told not to use (the backtracking family)");
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55) || match_cap >= ((size_t)1 << 58)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    if (device_overlap(d_in, n, d_out, cap)) return TRRE_E_ARG;
    const size_t ob = (nrec + 1) * 8, mb = d_match_off ? (match_cap + 1) * 8 : 0;
    if (any_overlap({{d_in, n}, {d_out, cap}}, {{d_off, ob}, {d_list_off, ob}, {d_match_off, mb}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or another offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p, p->find_marks.get())) return rc;
    return find_on(p, c.st, c.inner, d_in, n, d_off, nrec, d_out, cap, d_match_off, match_cap, d_list_off, n_matches, out_len, static_cast<hipStream_t>(stream));
}

// ---- match spans and split strings (records_block.hpp) ---------------------------------------------------------------------
// The context holds the staged text (d_snap), the staging passes' ranks (d_find_off: nobody reads them here, k_str_stage writes
// them), the framed text (d_framed) and, in d_rec behind the status word, cnt [3][tiles] and base [3][tiles + 1] — for the split
// call kcnt [tiles] and kbase [tiles + 1] behind them
struct SpanMarks {
    bool empty;             // nrec == 0: the offsets passed and nothing else ran
    trre::SpanArgs pa;      // src, total, nrec, tiles, cnt, base
    size_t found;           // matches
    uint64_t* kcnt;         // (kept) the kept bytes per framed tile,
    uint64_t* kbase;        // their exclusive scan,
    uint64_t kept;          // and their total
};

// What the span call and the split call share, up to the one read-back before anything of the caller's is written: the offsets'
// check, the staged text, its newline check, the one scan into d_framed, k_span_count with its three scans and the totals'
// check.  kept (the split call): k_split_count and its scan go in front of that read-back, and their total comes with the others.
static int span_marks(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, bool kept, hipStream_t s,
                      SpanMarks* out) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    const int64_t T = str_tile_bytes();
    const int64_t total = (int64_t)(n + nrec);                     // the staged text
    *out = SpanMarks{};
    // 1. the offsets, on the device: nothing is written before they pass
    int rc = rec_check_offsets(cx, (total + T - 1) / T, d_off, nrec, n, s);
    if (rc) return rc;
    if (nrec == 0) {
        out->empty = true;
        return TRRE_OK;
    }
    // 2. the staged text, as for the strings call; the ranks its stage pass leaves go into the library's own array
    HIP_TRY(cx->d_find_off.reserve(nrec + 1, (nrec + 1) * 8));
    StrArgs sa;
    rc = str_stage_text(cx, d_in, n, d_off, nrec, cx->d_find_off, s, &sa);
    if (rc) return rc;
    // 3. a string that holds a '\n' would be several lines: the staged newlines are the strings' closing ones exactly when they are nrec
    uint64_t staged_nl = 0;
    if (str_staged_newlines(cx, sa, s, &staged_nl) < 0) return TRRE_E_DEVICE;
    if (staged_nl != nrec) return fail(TRRE_E_ARG, "error: a string holds a newline: it would be several lines, each with matches of its own");
    // 4. the one scan: markers and position bytes
    size_t m = 0;
    rc = find_scan(p, st, cx->d_snap, (size_t)total, cx->d_framed, &m, s);
    if (rc) return rc;                                      // (TRRE_E_DIVERGES: the caller's sizes stay 0)
    if ((int64_t)m < total) return fail(TRRE_E_DEVICE, "error: the framed text is shorter than the staged text (internal)");
    // 5. the markers per framed tile and before it; the table and the passes must agree before anything of the caller's is written
    const int64_t ftiles = ((int64_t)m + T - 1) / T;
    RecCarve c;                                             // (room as for 2 ftiles + 2 tiles, 3 ftiles + 2 with the kept bytes; behind its part[0] the layout is this call's)
    rc = rec_carve(cx, (kept ? 3 : 2) * ftiles + 2, &c);
    if (rc) return rc;
    SpanArgs& pa = out->pa;
    pa.src = cx->d_framed; pa.total = (int64_t)m; pa.nrec = (int64_t)nrec; pa.tiles = ftiles;
    pa.cnt = reinterpret_cast<uint64_t*>(c.part) + 1; pa.base = pa.cnt + 3 * ftiles;
    launch_span_count(pa, s);
    uint64_t tot[3] = {0, 0, 0};
    rc = scan_counts(pa.cnt, pa.base, 3, ftiles, s, tot);
    if (rc) return rc;
    if (kept) {
        out->kcnt = const_cast<uint64_t*>(pa.base) + 3 * (ftiles + 1); out->kbase = out->kcnt + ftiles;
        SplitArgs ka{};
        ka.src = pa.src; ka.total = pa.total; ka.tiles = ftiles; ka.base = pa.base; ka.kcnt = out->kcnt;
        launch_split_count(ka, s);
        launch_chunk_scan(out->kcnt, out->kbase, ftiles, s);
        HIP_TRY(hipMemcpyAsync(&out->kept, out->kbase + ftiles, 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (tot[0] != tot[1] || tot[2] != nrec || m != (size_t)total + 2 * tot[0] || out->kept > n)
        return fail(TRRE_E_DEVICE, "error: the markers of the framed text do not add up (internal)");
    out->found = (size_t)tot[0];
    return TRRE_OK;
}

static int span_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t* d_start,
                   int64_t* d_end, size_t span_cap, int64_t* d_list_off, size_t* n_matches, hipStream_t s) {
    SpanMarks mk;
    const int rc = span_marks(p, st, d_in, n, d_off, nrec, false, s, &mk);
    if (rc) return rc;
    if (mk.empty) {
        HIP_TRY(hipMemsetAsync(d_list_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    const size_t found = mk.found;
    if (n_matches) *n_matches = found;
    // 6. the spans and the list offsets — the list offsets alone when the spans do not fit
    const bool over = found > span_cap;
    trre::SpanArgs& pa = mk.pa;
    pa.start = d_start; pa.end = d_end; pa.list_off = d_list_off; pa.n_match = over ? 0 : (int64_t)found; pa.lists_only = over ? 1u : 0u;
    trre::launch_span_emit(pa, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return over ? fail(TRRE_E_CAPACITY, "error: output buffer too small") : TRRE_OK;
}

int trre_span_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t* d_start, int64_t* d_end,
                             size_t span_cap, int64_t* d_list_off, size_t* n_matches, void* stream) {
    g_scan_flags = 0;
    if (n_matches) *n_matches = 0;
    if (!p || !d_off || !d_list_off || (n && !d_in) || (span_cap && (!d_start || !d_end))) return fail(TRRE_E_ARG, "error: null argument");
    if (int rc = spans_program(p, "match spans")) return rc;
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55) || span_cap >= ((size_t)1 << 58)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    const size_t ob = (nrec + 1) * 8, sb = d_start ? span_cap * 8 : 0, eb = d_end ? span_cap * 8 : 0;
    if (any_overlap({{d_in, n}}, {{d_off, ob}, {d_list_off, ob}, {d_start, sb}, {d_end, eb}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or another offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p)) return rc;
    return span_on(p, c.st, d_in, n, d_off, nrec, d_start, d_end, span_cap, d_list_off, n_matches, static_cast<hipStream_t>(stream));
}

// the pieces between the matches: steps 1 - 5 are the span call's, with the kept bytes counted in front of the read-back
static int split_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out, size_t cap,
                    int64_t* d_piece_off, size_t piece_cap, int64_t* d_list_off, size_t* n_pieces, size_t* out_len, hipStream_t s) {
    SpanMarks mk;
    const int rc = span_marks(p, st, d_in, n, d_off, nrec, true, s, &mk);
    if (rc) return rc;
    if (mk.empty) {
        HIP_TRY(hipMemsetAsync(d_list_off, 0, 8, s));
        if (d_piece_off) HIP_TRY(hipMemsetAsync(d_piece_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    const size_t pieces = mk.found + nrec, kept = (size_t)mk.kept;
    if (n_pieces) *n_pieces = pieces;
    if (out_len) *out_len = kept;
    // 6. the pieces, where each starts and the list offsets — the list offsets alone when either does not fit
    const bool over = kept > cap || pieces > piece_cap;
    trre::SplitArgs a{};
    a.src = mk.pa.src; a.total = mk.pa.total; a.in = d_in; a.n = (int64_t)n; a.list_off = d_list_off; a.nrec = (int64_t)nrec;
    a.tiles = mk.pa.tiles; a.base = mk.pa.base; a.kcnt = mk.kcnt; a.kbase = mk.kbase; a.lists_only = over ? 1u : 0u;
    if (!over) { a.out = d_out; a.out_len = (int64_t)kept; a.piece_off = d_piece_off; a.n_piece = (int64_t)pieces; }
    trre::launch_split_emit(a, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return over ? fail(TRRE_E_CAPACITY, "error: output buffer too small") : TRRE_OK;
}

int trre_split_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out, size_t cap,
                              int64_t* d_piece_off, size_t piece_cap, int64_t* d_list_off, size_t* n_pieces, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (n_pieces) *n_pieces = 0;
    if (!p || !d_off || !d_list_off || (n && !d_in) || (cap && !d_out) || (piece_cap && !d_piece_off)) return fail(TRRE_E_ARG, "error: null argument");
    if (int rc = spans_program(p, "split strings")) return rc;
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55) || piece_cap >= ((size_t)1 << 58)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    const size_t ob = (nrec + 1) * 8, pb = d_piece_off ? (piece_cap + 1) * 8 : 0, cb = d_out ? cap : 0;
    if (ranges_overlap(d_in, n, d_out, cb)) return fail(TRRE_E_ARG, "error: the output overlaps the input (the pieces are not made in place)");
    if (any_overlap({{d_in, n}, {d_out, cb}}, {{d_off, ob}, {d_list_off, ob}, {d_piece_off, pb}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or another offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p)) return rc;
    return split_on(p, c.st, d_in, n, d_off, nrec, d_out, cap, d_piece_off, piece_cap, d_list_off, n_pieces, out_len, static_cast<hipStream_t>(stream));
}

// What the filter call and the field call do with the span call's marks: the list offsets, and nothing else of the span call
// (k_span_emit, lists only), into the library's own array; the geometry of the INPUT's tiles; the field call's bounds (field: its
// arguments, *a their .f), which read the span call's tiles; then d_rec carved for the input's tiles — behind the status word:
// part [tiles + 1], cnt [2][tiles], base [2][tiles + 1] — into *a
static int filter_tiles(ScanCtx* cx, trre::SpanArgs& pa, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, hipStream_t s,
                        trre::FilterArgs* a, const trre::FieldArgs* field) {
    HIP_TRY(cx->d_filter_lists.reserve(nrec + 1, (nrec + 1) * 8));
    pa.start = pa.end = nullptr; pa.list_off = cx->d_filter_lists; pa.n_match = 0; pa.lists_only = 1u;
    trre::launch_span_emit(pa, s);
    const int64_t T = trre::str_tile_bytes();
    const int64_t a0 = (int64_t)(reinterpret_cast<uintptr_t>(d_in) & 15u);
    const int64_t tiles = std::max<int64_t>((a0 + (int64_t)n + T - 1) / T, 1);
    a->in_v0 = d_in - a0; a->vbeg = a0; a->n = (int64_t)n; a->off = d_off; a->loff = cx->d_filter_lists; a->nrec = (int64_t)nrec;
    a->tiles = tiles;
    if (field) trre::launch_field_bounds(pa, *field, s);
    RecCarve c;                                             // (room as for 2 tiles + 1: 6 tiles + 6 words)
    const int rc = rec_carve(cx, 2 * tiles + 1, &c);
    if (rc) return rc;
    a->part = c.part; a->cnt = reinterpret_cast<uint64_t*>(c.part) + tiles + 1; a->base = a->cnt + 2 * tiles;
    return TRRE_OK;
}

// the strings with a match (without one: TRRE_FILTER_INVERT), whole, and their rows: steps 1 - 5 are the span call's
static int filter_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint32_t flags, uint8_t* d_out,
                     size_t cap, int64_t* d_out_off, int64_t* d_rows, size_t row_cap, size_t* n_kept, size_t* out_len, hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    SpanMarks mk;
    int rc = span_marks(p, st, d_in, n, d_off, nrec, false, s, &mk);
    if (rc) return rc;
    if (mk.empty) {
        if (d_out_off) HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 6. the verdicts: the span call's list offsets; 7. over tiles of the INPUT: the first string of every tile, the kept strings
    //    and bytes per tile and before it; the two totals in one read-back
    FilterArgs a{};
    a.invert = (flags & TRRE_FILTER_INVERT) ? 1u : 0u;
    rc = filter_tiles(cx, mk.pa, d_in, n, d_off, nrec, s, &a, nullptr);
    if (rc) return rc;
    launch_filter_count(a, s);
    uint64_t tot[2] = {0, 0};
    rc = scan_counts(a.cnt, a.base, 2, a.tiles, s, tot);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (tot[0] > nrec || tot[1] > n) return fail(TRRE_E_DEVICE, "error: the kept strings do not add up (internal)");
    const size_t kept = (size_t)tot[0], bytes = (size_t)tot[1];
    if (n_kept) *n_kept = kept;
    if (out_len) *out_len = bytes;
    if (bytes > cap || kept > row_cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    // 8. the kept strings' bytes, where each starts and which row it was
    if (kept == 0) {
        if (d_out_off) HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, s));
    } else {
        a.out = d_out; a.out_len = (int64_t)bytes; a.out_off = d_out_off; a.rows = d_rows; a.n_kept = (int64_t)kept;
        launch_filter_emit(a, s);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s));
    return TRRE_OK;
}

int trre_filter_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint32_t flags, uint8_t* d_out,
                               size_t cap, int64_t* d_out_off, int64_t* d_rows, size_t row_cap, size_t* n_kept, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (n_kept) *n_kept = 0;
    if (!p || !d_off || (n && !d_in) || (cap && !d_out) || (row_cap && (!d_out_off || !d_rows))) return fail(TRRE_E_ARG, "error: null argument");
    if (flags & ~TRRE_FILTER_INVERT) return fail(TRRE_E_ARG, "error: unknown flag (TRRE_FILTER_INVERT is the only one)");
    if (int rc = spans_program(p, "filtered strings")) return rc;
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55) || row_cap >= ((size_t)1 << 58)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    const size_t ob = (nrec + 1) * 8, pb = d_out_off ? (row_cap + 1) * 8 : 0, rb = d_rows ? row_cap * 8 : 0, cb = d_out ? cap : 0;
    if (ranges_overlap(d_in, n, d_out, cb)) return fail(TRRE_E_ARG, "error: the output overlaps the input (the kept strings are not made in place)");
    if (any_overlap({{d_in, n}, {d_out, cb}}, {{d_off, ob}, {d_out_off, pb}, {d_rows, rb}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or another offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p)) return rc;
    return filter_on(p, c.st, d_in, n, d_off, nrec, flags, d_out, cap, d_out_off, d_rows, row_cap, n_kept, out_len, static_cast<hipStream_t>(stream));
}

// field k of every string: steps 1 - 6 are the filter call's
static int field_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t k, uint8_t* d_out,
                    size_t cap, int64_t* d_out_off, uint64_t* d_valid, size_t* n_valid, size_t* out_len, hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    SpanMarks mk;
    int rc = span_marks(p, st, d_in, n, d_off, nrec, false, s, &mk);
    if (rc) return rc;
    if (mk.empty) {
        if (d_out_off) HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 6. the span call's list offsets; 7. the bitmap, and where every field starts and ends: from the offsets and the list offsets,
    //    and from the framed text's markers — before the carve: it reads the span call's tiles, which the carve reuses
    HIP_TRY(cx->d_field_bounds.reserve(nrec, 2 * nrec * 8));
    FieldArgs a{};
    a.k = k; a.lo = cx->d_field_bounds; a.hi = a.lo + nrec; a.valid = d_valid; a.words = (int64_t)((nrec + 63) / 64);
    rc = filter_tiles(cx, mk.pa, d_in, n, d_off, nrec, s, &a.f, &a);
    if (rc) return rc;
    // 8. over tiles of the INPUT: the first string of every tile, the strings with the field and the field bytes per tile and before
    //    it; the two totals in one read-back
    launch_field_count(a, s);
    uint64_t tot[2] = {0, 0};
    rc = scan_counts(a.f.cnt, a.f.base, 2, a.f.tiles, s, tot);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (tot[0] > nrec || tot[1] > n) return fail(TRRE_E_DEVICE, "error: the fields do not add up (internal)");
    const size_t bytes = (size_t)tot[1];
    if (n_valid) *n_valid = (size_t)tot[0];
    if (out_len) *out_len = bytes;
    if (bytes > cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    // 9. the fields' bytes and where each starts (no byte at all: the offsets alone, all zero; the size query may have no room for them)
    if (d_out_off) {
        a.f.out = d_out; a.f.out_len = (int64_t)bytes; a.f.out_off = d_out_off;
        launch_field_emit(a, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    return TRRE_OK;
}

int trre_field_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t k, uint8_t* d_out, size_t cap,
                              int64_t* d_out_off, uint8_t* d_valid, size_t* n_valid, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (n_valid) *n_valid = 0;
    if (!p || !d_off || (n && !d_in) || (cap && !d_out) || (!d_out_off && (d_out || cap)) || (nrec && !d_valid))
        return fail(TRRE_E_ARG, "error: null argument");
    if (int rc = spans_program(p, "field strings")) return rc;
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    if (reinterpret_cast<uintptr_t>(d_valid) & 7u) return fail(TRRE_E_ARG, "error: the validity bitmap must be 8-byte aligned (it is written as 64-bit words)");
    const size_t ob = (nrec + 1) * 8, pb = d_out_off ? ob : 0, vb = (nrec + 63) / 64 * 8, cb = d_out ? cap : 0;
    if (ranges_overlap(d_in, n, d_out, cb)) return fail(TRRE_E_ARG, "error: the output overlaps the input (the fields are not made in place)");
    if (any_overlap({{d_in, n}, {d_out, cb}}, {{d_off, ob}, {d_out_off, pb}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or another offsets array");
    if (any_overlap({{d_in, n}, {d_out, cb}, {d_off, ob}, {d_out_off, pb}}, {{d_valid, vb}}))
        return fail(TRRE_E_ARG, "error: the validity bitmap overlaps the data or an offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p)) return rc;
    return field_on(p, c.st, d_in, n, d_off, nrec, k, d_out, cap, d_out_off, reinterpret_cast<uint64_t*>(d_valid), n_valid, out_len,
                    static_cast<hipStream_t>(stream));
}

// ---- replaced strings (records_block.hpp) -----------------------------------------------------------------------------------
// Steps 1 - 5 are the span call's, 6 its emit pass into the library's own arrays, 7 the find call's texts scan of the same staged
// text under the inner program (stt: its state; its context holds the framed texts).  The outer context holds everything else.
static int sub_on(trre_prog* p, DeviceState* st, DeviceState* stt, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t first,
                  int64_t count, uint8_t* d_out, size_t cap, int64_t* d_out_off, size_t* n_replaced, size_t* out_len, hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    SpanMarks mk;
    int rc = span_marks(p, st, d_in, n, d_off, nrec, false, s, &mk);
    if (rc) return rc;
    if (mk.empty) {
        if (d_out_off) HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 6. where every match starts and ends, and the list offsets: each array with its entry -1 in front
    const size_t found = mk.found, slots = found + 2;
    HIP_TRY(cx->d_sub_idx.reserve(slots, 4 * slots * 8));
    HIP_TRY(cx->d_filter_lists.reserve(nrec + 1, (nrec + 1) * 8));
    SubArgs a{};
    a.in = d_in; a.n = (int64_t)n; a.off = d_off; a.nrec = (int64_t)nrec; a.L = cx->d_filter_lists;
    a.S = cx->d_sub_idx + 1; a.E = a.S + slots; a.P = a.E + 2 * slots; a.found = (int64_t)found; a.first = first; a.count = count;
    int64_t* xo = a.E + slots;
    a.XO = xo;
    SpanArgs& pa = mk.pa;
    pa.start = a.S; pa.end = a.E; pa.list_off = cx->d_filter_lists; pa.n_match = (int64_t)found; pa.lists_only = 0u;
    launch_span_emit(pa, s);
    HIP_TRY(hipGetLastError());
    // 7. the texts scan: every match's output and a '\n' — as many as there are matches; unframed into the library's own buffer
    size_t m = 0;
    const size_t total = n + nrec;
    rc = find_scan(p->sub_texts.get(), stt, cx->d_snap, total, stt->ctx.d_framed, &m, s);
    if (rc) return rc;                                      // (TRRE_E_DIVERGES: the caller's sizes stay 0)
    const int64_t T = str_tile_bytes(), utiles = ((int64_t)m + T - 1) / T;
    uint64_t closed = 0;
    const uint64_t* before = nullptr;
    if (m) {
        rc = str_tile_newlines(cx, stt->ctx.d_framed, (int64_t)m, s, &before);
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        if (rec_status(cx, s, const_cast<uint64_t*>(before) + utiles, &closed) < 0) return TRRE_E_DEVICE;
    } else {
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (closed != found || m < found) return fail(TRRE_E_DEVICE, "error: the two scans of the strings disagree on the number of matches (internal)");
    const size_t texts = m - found;
    HIP_TRY(cx->d_sub_texts.reserve(texts + 64, texts + 64));
    a.X = cx->d_sub_texts; a.x_len = (int64_t)texts;
    if (found == 0) {
        HIP_TRY(hipMemsetAsync(xo, 0, 8, s));
    } else {
        StrArgs ua{};
        ua.src_v0 = stt->ctx.d_framed; ua.total = (int64_t)m; ua.dst = cx->d_sub_texts; ua.dst_len = (int64_t)texts;
        ua.nrec = (int64_t)found; ua.out_off = xo;
        ua.part = reinterpret_cast<const int64_t*>(before);
        launch_find_unframe(ua, utiles, s);
        HIP_TRY(hipGetLastError());
    }
    // 8. over chunks of matches: which are selected, and the selected matches, their texts' bytes and their matched bytes per chunk
    //    and before it; the three totals and the status word in one read-back
    const int64_t per = sub_chunk_matches();
    a.chunks = std::max<int64_t>(((int64_t)found + per - 1) / per, 1);
    HIP_TRY(cx->d_sub_cnt.reserve((size_t)a.chunks, (size_t)(6 * a.chunks + 4) * 8));
    a.status = reinterpret_cast<uint32_t*>(cx->d_sub_cnt.p);
    a.cnt = cx->d_sub_cnt + 1; a.base = a.cnt + 3 * a.chunks;
    HIP_TRY(hipMemsetAsync(cx->d_sub_cnt, 0, 8, s));
    launch_sub_plan(a, s);
    uint64_t tot[3] = {0, 0, 0};
    rc = scan_counts(a.cnt, a.base, 3, a.chunks, s, tot);
    if (rc) return rc;
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.status, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (bad || tot[0] > found || tot[1] > texts || tot[2] > n) return fail(TRRE_E_DEVICE, "error: the replaced matches do not add up (internal)");
    const size_t bytes = n - (size_t)tot[2] + (size_t)tot[1];
    if (n_replaced) *n_replaced = (size_t)tot[0];
    if (out_len) *out_len = bytes;
    if (bytes > cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    // 9. where every segment starts; the output offsets; the splice (the size query may have no room for either)
    if (d_out_off) {
        a.out = d_out; a.out_len = (int64_t)bytes; a.out_off = d_out_off;
        launch_sub_place(a, s);
        launch_sub_offsets(a, s);
        launch_sub_emit(a, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    return TRRE_OK;
}

int trre_sub_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t first, int64_t count,
                            uint8_t* d_out, size_t cap, int64_t* d_out_off, size_t* n_replaced, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (n_replaced) *n_replaced = 0;
    if (!p || !d_off || (n && !d_in) || (cap && !d_out) || (!d_out_off && (d_out || cap))) return fail(TRRE_E_ARG, "error: null argument");
    if (p->mode != TRRE_MODE_SUB || !p->sub_texts) return fail(TRRE_E_ARG, "error: replaced strings take a program compiled with TRRE_MODE_SUB");
    if (p->prints_newline)
        return fail(TRRE_E_UNSUPPORTED, "error: the pattern can print a newline of its own: the matches' outputs could not be told apart");
    if (p->forced_family == TRRE_KERNEL_BACKTRACK)
        return fail(TRRE_E_UNSUPPORTED, "error: sub mode runs on the guided tables, which this program was told not to use (the backtracking family)");
    if (first < 0) return fail(TRRE_E_ARG, "error: first must not be negative (count < 0 selects every match from first on)");
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    const size_t ob = (nrec + 1) * 8, pb = d_out_off ? ob : 0, cb = d_out ? cap : 0;
    if (ranges_overlap(d_in, n, d_out, cb)) return fail(TRRE_E_ARG, "error: the output overlaps the input (the replaced strings are not made in place)");
    if (any_overlap({{d_in, n}, {d_out, cb}}, {{d_off, ob}, {d_out_off, pb}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or another offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p, p->sub_texts.get())) return rc;
    return sub_on(p, c.st, c.inner, d_in, n, d_off, nrec, first, count, d_out, cap, d_out_off, n_replaced, out_len, static_cast<hipStream_t>(stream));
}

namespace {
// grow one direction of a host slot (pinned staging + device buffer); need_pin false: the caller's own buffer is pinned, no staging on this side
int slot_reserve(DeviceState::HostSlot& hs, bool input, size_t bytes, bool need_pin) {
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
}  // namespace

// the host paths stage their chunks anyway: a scan in place saves nothing there, and any overlap (out == in too) is refused
static int host_overlap(const uint8_t* in, size_t n, const uint8_t* out, size_t cap) {
    if (n && out && (out == in || ranges_overlap(in, n, out, cap)))
        return fail(TRRE_E_ARG, "error: input and output overlap (the host paths take separate buffers)");
    return TRRE_OK;
}

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
namespace {
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
