// runtime_state.hpp — what the host files of the runtime share (compile.cpp, runtime.cpp, column_calls.cpp, host_path.cpp): the error
// helpers, a scan's state on a device, the compiled program, and the few functions that cross a file boundary.  Host only: no .hip file
// includes this.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/trre_mi355x.h"
#include "front.hpp"
#include "scan_block.hpp"

namespace trre_host {

int fail(int code, const std::string& msg);                                   // (runtime.cpp, with the thread's error string)
int fail_empty(size_t* out_len, int code, const std::string& msg);            // ... and no output stands
extern thread_local std::string g_error;     // what trre_last_error() returns on this thread (runtime.cpp)
extern thread_local uint32_t g_scan_flags;    // TRRE_SCAN_*: what the last scan call on this thread has to add to its return code (runtime.cpp)

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(TRRE_E_DEVICE, std::string("hip: ") + hipGetErrorString(e_) + " at " #expr); \
    } while (0)

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
    DevBuf<int64_t> d_trim_marks;     // trre_trim_device_strings: where every string's matches 0, c - 1 and c - 2 start and end [6][nrec] (strings)
    DevBuf<uint64_t> d_splitn_cnt;    // trre_splitn_device_strings: cnt [2][tiles], base [2][tiles + 1]: kept bytes, cutting matches per framed tile (tiles)
    DevBuf<int64_t> d_sub_idx;        // trre_sub_device_strings: S, E, XO, P, each [found + 2] with entry -1 in front (matches)
    DevBuf<uint8_t> d_sub_texts;      // ... the texts scan unframed (bytes)
    DevBuf<uint64_t> d_sub_cnt;       // ... the status word, cnt [3][chunks], base [3][chunks + 1] (chunks)
    DevBuf<int64_t> d_nth_xo;         // trre_nth_device_strings: the texts' offsets XO [found + 1] (matches)
    DevBuf<uint8_t> d_nth_texts;      // ... the texts scan unframed (bytes)
    DevBuf<int64_t> d_nth_src;        // ... where every entry starts in the texts [nrec] (strings)
    DevBuf<uint64_t> d_nth_cnt;       // ... the status word, cnt [2][chunks], base [2][chunks + 1] (chunks)
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
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace trre_host

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
    std::map<int, std::unique_ptr<trre_host::DeviceState>> dev;
};

namespace trre_host {

constexpr const char* kStackMsg = "error: stack max capacity reached";
constexpr const char* kFindOnlyMsg = "error: a program compiled with TRRE_MODE_FIND runs through trre_find_device_strings only";
constexpr const char* kSpansOnlyMsg = "error: a program compiled with TRRE_MODE_SPANS runs through trre_span_device_strings, trre_split_device_strings, trre_filter_device_strings and trre_field_device_strings only";
constexpr const char* kDivergeMsg = "error: stack max capacity reached (the reference's search does not terminate on this input)";
// a program that one call alone runs: that call's name for every other call's refusal (null: any scan call may run it)
constexpr const char* kSubOnlyMsg = "error: a program compiled with TRRE_MODE_SUB runs through trre_sub_device_strings only";
inline const char* own_call_only(const trre_prog& p) {
    return p.mode == TRRE_MODE_FIND ? kFindOnlyMsg : p.mode == TRRE_MODE_SPANS ? kSpansOnlyMsg : p.mode == TRRE_MODE_SUB ? kSubOnlyMsg : nullptr;
}

// ---- what crosses a file boundary ------------------------------------------------------------------------------------------
// compile.cpp (host only: nothing in it launches or allocates on a device)
int lazy_ensure(trre_prog* p);
// runtime.cpp: the scan core
bool is_generate(int mode);
bool is_gen(int fam);
int scan_family(const trre_prog& p);
int guided_sym_bits(const trre_prog& p);
hipError_t pinned_get(uint8_t** out, size_t bytes);
void pinned_put(uint8_t* p);
int ctx_init(ScanCtx& c);
int device_state(trre_prog* p, int dev, DeviceState** out);
int current_state(trre_prog* p, DeviceState** st);
bool ranges_overlap(const void* a, size_t n, const void* b, size_t m);
int device_overlap(const uint8_t* d_in, size_t n, const uint8_t* d_out, size_t cap);
int enqueue(trre_prog* p, DeviceState* st, ScanCtx* cx, int family, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, hipStream_t stream);
int finish(trre_prog* p, DeviceState* st, ScanCtx* cx, size_t* out_len);
int generate_on(trre_prog* p, DeviceState* st, const uint8_t* in, size_t n, std::vector<uint8_t>& result, bool& diverged);
// host_path.cpp
int slot_reserve(DeviceState::HostSlot& hs, bool input, size_t bytes, bool need_pin = true);

}  // namespace trre_host
