// column_calls.cpp — the calls on a column of records or strings (records_block.hpp): their shared host passes, one
// function per call that queues its passes around the scan, and their entry points of the C ABI (include/trre_mi355x.h).  They reach
// the scan core (runtime.cpp) through the names that runtime_state.hpp declares.
#include <functional>
#include <initializer_list>

#include "runtime_state.hpp"
#include "launch.hpp"
#include "records_block.hpp"

using namespace trre_host;

extern "C" {

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

// The texts scan of the staged text (cx->d_snap, `total` bytes) under the program `texts` (stt: its state) into `framed`: every match's
// output and a '\n' — as many as `found`, the matches the other scan counted.  *m: the framed texts' bytes; *before [tiles + 1]: the
// '\n' before every string tile (16 KiB) of them, in a fresh carve of cx; their total is read back and checked.  What the find and
// nth calls' step 5 and the sub call's step 7 share.
static int find_texts(trre_prog* texts, DeviceState* stt, ScanCtx* cx, size_t total, DevBuf<uint8_t>& framed, size_t found, hipStream_t s,
                      size_t* m, const uint64_t** before) {
    int rc = find_scan(texts, stt, cx->d_snap, total, framed, m, s);
    if (rc) return rc;                                      // (TRRE_E_DIVERGES: the caller's sizes stay 0)
    const int64_t T = trre::str_tile_bytes(), utiles = ((int64_t)*m + T - 1) / T;
    uint64_t closed = 0;
    *before = nullptr;
    if (*m) {
        rc = str_tile_newlines(cx, framed, (int64_t)*m, s, before);
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        if (rec_status(cx, s, const_cast<uint64_t*>(*before) + utiles, &closed) < 0) return TRRE_E_DEVICE;
    } else {
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (closed != found || *m < found) return fail(TRRE_E_DEVICE, "error: the two scans of the strings disagree on the number of matches (internal)");
    return TRRE_OK;
}

// d_rec as for the strings call, of the outer program's context, which also holds the staged text (d_snap), the list offsets while
// they are being made and after (d_find_off), the marks unframed (d_find_marks) and the framed texts (d_framed); the inner program's
// context holds the framed marks (its d_framed)
struct FoundTexts {
    bool empty;             // nrec == 0: the offsets passed and nothing else ran
    size_t found;           // matches
    size_t m;               // the framed texts' bytes: the texts' and a '\n' per match
    const uint64_t* before; // [tiles + 1] '\n' before every string tile of the framed texts (null: m == 0)
};

// What the find call and the nth call share, steps 1 - 5: the offsets' check, the staged text, its newline check, the marks scan
// with the list offsets L into cx->d_find_off, the texts scan into cx->d_framed with the closed-count check.  d_list_off (the find
// call; null: the nth call): L is copied there as soon as it is made, behind the strings' check and before the texts scan.
static int find_marks_texts(trre_prog* p, DeviceState* st, DeviceState* stm, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec,
                            int64_t* d_list_off, hipStream_t s, FoundTexts* out) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    const int64_t T = str_tile_bytes();
    const int64_t total = (int64_t)(n + nrec);                     // the staged text
    *out = FoundTexts{};
    // 1. the offsets, on the device: nothing is written before they pass
    int rc = rec_check_offsets(cx, (total + T - 1) / T, d_off, nrec, n, s);
    if (rc) return rc;
    if (nrec == 0) {
        out->empty = true;
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
    if (d_list_off) HIP_TRY(hipMemcpyAsync(d_list_off, loff, (nrec + 1) * 8, hipMemcpyDeviceToDevice, s));
    // 5. the texts scan: every match's output and a '\n' — as many as there are marks
    out->found = found;
    return find_texts(p, st, cx, (size_t)total, cx->d_framed, found, s, &out->m, &out->before);
}

static int find_on(trre_prog* p, DeviceState* st, DeviceState* stm, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec,
                   uint8_t* d_out, size_t cap, int64_t* d_match_off, size_t match_cap, int64_t* d_list_off, size_t* n_matches,
                   size_t* out_len, hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    FoundTexts ft;
    const int rc = find_marks_texts(p, st, stm, d_in, n, d_off, nrec, d_list_off, s, &ft);
    if (rc) return rc;
    if (ft.empty) {
        HIP_TRY(hipMemsetAsync(d_list_off, 0, 8, s));
        if (d_match_off) HIP_TRY(hipMemsetAsync(d_match_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    const size_t found = ft.found, m = ft.m;
    if (n_matches) *n_matches = found;
    if (out_len) *out_len = m - found;
    if (m - found > cap || found > match_cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    // 6. the framed texts without their newlines into the caller's buffer, and where each match starts
    if (found == 0) {
        if (d_match_off) HIP_TRY(hipMemsetAsync(d_match_off, 0, 8, s));
    } else {
        const int64_t T = str_tile_bytes();
        StrArgs ua{};
        ua.src_v0 = cx->d_framed; ua.total = (int64_t)m; ua.dst = d_out; ua.dst_len = (int64_t)(m - found);
        ua.nrec = (int64_t)found; ua.out_off = d_match_off;
        ua.part = reinterpret_cast<const int64_t*>(ft.before);
        launch_find_unframe(ua, ((int64_t)m + T - 1) / T, s);
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

// ---- match k of every string (records_block.hpp) ---------------------------------------------------------------------------
// Steps 1 - 5 are the find call's.  The outer context also holds the texts unframed (d_nth_texts) with their offsets (d_nth_xo), the
// entries' sources (d_nth_src) and the plan's status word, counts and bases (d_nth_cnt).
static int nth_on(trre_prog* p, DeviceState* st, DeviceState* stm, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t k,
                  uint8_t* d_out, size_t cap, int64_t* d_out_off, uint64_t* d_valid, size_t* n_valid, size_t* out_len, hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    FoundTexts ft;
    int rc = find_marks_texts(p, st, stm, d_in, n, d_off, nrec, nullptr, s, &ft);
    if (rc) return rc;
    if (ft.empty) {
        if (d_out_off) HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 6. the framed texts without their newlines into the library's own buffer, and where each match's text starts
    const size_t found = ft.found, texts = ft.m - found;
    HIP_TRY(cx->d_nth_xo.reserve(found + 1, (found + 1) * 8));
    HIP_TRY(cx->d_nth_texts.reserve(texts + 64, texts + 64));
    if (found == 0) {
        HIP_TRY(hipMemsetAsync(cx->d_nth_xo, 0, 8, s));
    } else {
        const int64_t T = str_tile_bytes();
        StrArgs ua{};
        ua.src_v0 = cx->d_framed; ua.total = (int64_t)ft.m; ua.dst = cx->d_nth_texts; ua.dst_len = (int64_t)texts;
        ua.nrec = (int64_t)found; ua.out_off = cx->d_nth_xo;
        ua.part = reinterpret_cast<const int64_t*>(ft.before);
        launch_find_unframe(ua, ((int64_t)ft.m + T - 1) / T, s);
        HIP_TRY(hipGetLastError());
    }
    // 7. over chunks of strings: the bitmap, where every entry starts in the texts, and the strings with the match and the entries'
    //    bytes per chunk and before it; the two totals and the status word in one read-back
    const int64_t per = nth_chunk_strings();
    NthArgs a{};
    a.L = cx->d_find_off; a.nrec = (int64_t)nrec; a.XO = cx->d_nth_xo; a.X = cx->d_nth_texts; a.x_len = (int64_t)texts; a.found = (int64_t)found;
    a.k = k; a.valid = d_valid; a.words = (int64_t)((nrec + 63) / 64);
    a.chunks = ((int64_t)nrec + per - 1) / per;
    HIP_TRY(cx->d_nth_src.reserve(nrec, nrec * 8));
    HIP_TRY(cx->d_nth_cnt.reserve((size_t)a.chunks, (size_t)(4 * a.chunks + 3) * 8));
    a.src = cx->d_nth_src;
    a.status = reinterpret_cast<uint32_t*>(cx->d_nth_cnt.p);
    a.cnt = cx->d_nth_cnt + 1; a.base = a.cnt + 2 * a.chunks;
    HIP_TRY(hipMemsetAsync(cx->d_nth_cnt, 0, 8, s));
    launch_nth_plan(a, s);
    uint64_t tot[2] = {0, 0};
    rc = scan_counts(a.cnt, a.base, 2, a.chunks, s, tot);
    if (rc) return rc;
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.status, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (bad || tot[0] > nrec || tot[1] > texts) return fail(TRRE_E_DEVICE, "error: the selected matches do not add up (internal)");
    const size_t bytes = (size_t)tot[1];
    if (n_valid) *n_valid = (size_t)tot[0];
    if (out_len) *out_len = bytes;
    if (bytes > cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    // 8. where every entry starts; the entries' bytes (the size query may have no room for either)
    if (d_out_off) {
        a.out = d_out; a.out_len = (int64_t)bytes; a.out_off = d_out_off;
        launch_nth_offsets(a, s);
        launch_nth_emit(a, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    return TRRE_OK;
}

int trre_nth_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t k, uint8_t* d_out, size_t cap,
                            int64_t* d_out_off, uint8_t* d_valid, size_t* n_valid, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (n_valid) *n_valid = 0;
    if (!p || !d_off || (n && !d_in) || (cap && !d_out) || (!d_out_off && (d_out || cap)) || (nrec && !d_valid))
        return fail(TRRE_E_ARG, "error: null argument");
    if (p->mode == TRRE_MODE_SUB) return fail(TRRE_E_ARG, kSubOnlyMsg);
    if (p->mode != TRRE_MODE_FIND || !p->find_marks) return fail(TRRE_E_ARG, "error: match k of every string takes a program compiled with TRRE_MODE_FIND");
    if (p->prints_newline)
        return fail(TRRE_E_UNSUPPORTED, "error: the pattern can print a newline of its own: the matches' outputs could not be told apart");
    if (p->forced_family == TRRE_KERNEL_BACKTRACK)
        return fail(TRRE_E_UNSUPPORTED, "error: find mode runs on the guided tables, which this program was told not to use (the backtracking family)");
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    if (reinterpret_cast<uintptr_t>(d_valid) & 7u) return fail(TRRE_E_ARG, "error: the validity bitmap must be 8-byte aligned (it is written as 64-bit words)");
    const size_t ob = (nrec + 1) * 8, pb = d_out_off ? ob : 0, vb = (nrec + 63) / 64 * 8, cb = d_out ? cap : 0;
    if (ranges_overlap(d_in, n, d_out, cb)) return fail(TRRE_E_ARG, "error: the output overlaps the input (the selected matches are not made in place)");
    if (any_overlap({{d_in, n}, {d_out, cb}}, {{d_off, ob}, {d_out_off, pb}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or another offsets array");
    if (any_overlap({{d_in, n}, {d_out, cb}, {d_off, ob}, {d_out_off, pb}}, {{d_valid, vb}}))
        return fail(TRRE_E_ARG, "error: the validity bitmap overlaps the data or an offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p, p->find_marks.get())) return rc;
    return nth_on(p, c.st, c.inner, d_in, n, d_off, nrec, k, d_out, cap, d_out_off, reinterpret_cast<uint64_t*>(d_valid), n_valid, out_len,
                  static_cast<hipStream_t>(stream));
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

// the pieces between the first or last `limit` matches: steps 1 - 5 are the span call's, 6 its list offsets into the library's own
// array; d_splitn_cnt holds cnt [2][tiles] and base [2][tiles + 1] of the kept bytes and the cutting matches per framed tile
static int splitn_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t limit, uint32_t flags,
                     uint8_t* d_out, size_t cap, int64_t* d_piece_off, size_t piece_cap, int64_t* d_list_off, size_t* n_pieces, size_t* out_len,
                     hipStream_t s) {
    using namespace trre;
    ScanCtx* cx = &st->ctx;
    SpanMarks mk;
    int rc = span_marks(p, st, d_in, n, d_off, nrec, false, s, &mk);
    if (rc) return rc;
    if (mk.empty) {
        HIP_TRY(hipMemsetAsync(d_list_off, 0, 8, s));
        if (d_piece_off) HIP_TRY(hipMemsetAsync(d_piece_off, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return TRRE_OK;
    }
    // 6. the span call's list offsets: which match of its string a marker belongs to, and of how many
    SpanArgs& pa = mk.pa;
    const int64_t ftiles = pa.tiles;
    HIP_TRY(cx->d_filter_lists.reserve(nrec + 1, (nrec + 1) * 8));
    HIP_TRY(cx->d_splitn_cnt.reserve((size_t)ftiles, (size_t)(4 * ftiles + 2) * 8));
    pa.start = pa.end = nullptr; pa.list_off = cx->d_filter_lists; pa.n_match = 0; pa.lists_only = 1u;
    launch_span_emit(pa, s);
    // 7. the kept bytes and the cutting matches per framed tile and before it; the two totals in one read-back
    SplitnArgs a{};
    a.L = cx->d_filter_lists; a.limit = limit; a.flags = flags;
    a.s.src = pa.src; a.s.total = pa.total; a.s.in = d_in; a.s.n = (int64_t)n; a.s.list_off = d_list_off; a.s.nrec = (int64_t)nrec;
    a.s.tiles = ftiles; a.s.base = pa.base; a.s.kcnt = cx->d_splitn_cnt; a.s.kbase = a.s.kcnt + 2 * ftiles;
    launch_splitn_count(a, s);
    uint64_t tot[2] = {0, 0};
    rc = scan_counts(a.s.kcnt, a.s.kbase, 2, ftiles, s, tot);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (tot[0] > n || tot[1] > mk.found) return fail(TRRE_E_DEVICE, "error: the cutting matches do not add up (internal)");
    const size_t pieces = (size_t)tot[1] + nrec, kept = (size_t)tot[0];
    if (n_pieces) *n_pieces = pieces;
    if (out_len) *out_len = kept;
    // 8. the pieces, where each starts and the list offsets — the list offsets alone when either does not fit
    const bool over = kept > cap || pieces > piece_cap;
    a.s.lists_only = over ? 1u : 0u;
    if (!over) { a.s.out = d_out; a.s.out_len = (int64_t)kept; a.s.piece_off = d_piece_off; a.s.n_piece = (int64_t)pieces; }
    launch_splitn_emit(a, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return over ? fail(TRRE_E_CAPACITY, "error: output buffer too small") : TRRE_OK;
}

int trre_splitn_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t limit, uint32_t flags,
                               uint8_t* d_out, size_t cap, int64_t* d_piece_off, size_t piece_cap, int64_t* d_list_off, size_t* n_pieces,
                               size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (n_pieces) *n_pieces = 0;
    if (!p || !d_off || !d_list_off || (n && !d_in) || (cap && !d_out) || (piece_cap && !d_piece_off)) return fail(TRRE_E_ARG, "error: null argument");
    if (flags & ~TRRE_SPLIT_FROM_END) return fail(TRRE_E_ARG, "error: unknown flag (TRRE_SPLIT_FROM_END is the only one)");
    if (int rc = spans_program(p, "split strings")) return rc;
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55) || piece_cap >= ((size_t)1 << 58)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    const size_t ob = (nrec + 1) * 8, pb = d_piece_off ? (piece_cap + 1) * 8 : 0, cb = d_out ? cap : 0;
    if (ranges_overlap(d_in, n, d_out, cb)) return fail(TRRE_E_ARG, "error: the output overlaps the input (the pieces are not made in place)");
    if (any_overlap({{d_in, n}, {d_out, cb}}, {{d_off, ob}, {d_list_off, ob}, {d_piece_off, pb}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or another offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p)) return rc;
    return splitn_on(p, c.st, d_in, n, d_off, nrec, limit, flags, d_out, cap, d_piece_off, piece_cap, d_list_off, n_pieces, out_len,
                     static_cast<hipStream_t>(stream));
}

// What the filter call and the field call do with the span call's marks: the list offsets, and nothing else of the span call
// (k_span_emit, lists only), into the library's own array; the geometry of the INPUT's tiles; bounds(pa): the field calls' launch of
// their bounds' kernels (*a is the .f of their arguments; the filter call: nothing), which read the span call's tiles; then d_rec
// carved for the input's tiles — behind the status word: part [tiles + 1], cnt [2][tiles], base [2][tiles + 1] — into *a
static int filter_tiles(ScanCtx* cx, trre::SpanArgs& pa, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, hipStream_t s,
                        trre::FilterArgs* a, const std::function<void(const trre::SpanArgs&)>& bounds) {
    HIP_TRY(cx->d_filter_lists.reserve(nrec + 1, (nrec + 1) * 8));
    pa.start = pa.end = nullptr; pa.list_off = cx->d_filter_lists; pa.n_match = 0; pa.lists_only = 1u;
    trre::launch_span_emit(pa, s);
    const int64_t T = trre::str_tile_bytes();
    const int64_t a0 = (int64_t)(reinterpret_cast<uintptr_t>(d_in) & 15u);
    const int64_t tiles = std::max<int64_t>((a0 + (int64_t)n + T - 1) / T, 1);
    a->in_v0 = d_in - a0; a->vbeg = a0; a->n = (int64_t)n; a->off = d_off; a->loff = cx->d_filter_lists; a->nrec = (int64_t)nrec;
    a->tiles = tiles;
    bounds(pa);
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
    rc = filter_tiles(cx, mk.pa, d_in, n, d_off, nrec, s, &a, [](const SpanArgs&) {});
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
    rc = filter_tiles(cx, mk.pa, d_in, n, d_off, nrec, s, &a.f, [&](const SpanArgs& pa) { launch_field_bounds(pa, a, s); });
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

// field k of the split at the first or last `limit` matches: the field call's steps, with the limited index arithmetic in the
// bounds (7) and the verdicts (8)
static int fieldn_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t k, int64_t limit,
                     uint32_t flags, uint8_t* d_out, size_t cap, int64_t* d_out_off, uint64_t* d_valid, size_t* n_valid, size_t* out_len, hipStream_t s) {
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
    HIP_TRY(cx->d_field_bounds.reserve(nrec, 2 * nrec * 8));
    FieldnArgs fn{};
    fn.limit = limit; fn.flags = flags;
    FieldArgs& a = fn.a;
    a.k = k; a.lo = cx->d_field_bounds; a.hi = a.lo + nrec; a.valid = d_valid; a.words = (int64_t)((nrec + 63) / 64);
    rc = filter_tiles(cx, mk.pa, d_in, n, d_off, nrec, s, &a.f, [&](const SpanArgs& pa) { launch_fieldn_bounds(pa, fn, s); });
    if (rc) return rc;
    launch_fieldn_count(fn, s);
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
    if (d_out_off) {
        a.f.out = d_out; a.f.out_len = (int64_t)bytes; a.f.out_off = d_out_off;
        launch_field_emit(a, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    return TRRE_OK;
}

int trre_fieldn_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t k, int64_t limit, uint32_t flags,
                               uint8_t* d_out, size_t cap, int64_t* d_out_off, uint8_t* d_valid, size_t* n_valid, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (n_valid) *n_valid = 0;
    if (!p || !d_off || (n && !d_in) || (cap && !d_out) || (!d_out_off && (d_out || cap)) || (nrec && !d_valid))
        return fail(TRRE_E_ARG, "error: null argument");
    if (flags & ~TRRE_SPLIT_FROM_END) return fail(TRRE_E_ARG, "error: unknown flag (TRRE_SPLIT_FROM_END is the only one)");
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
    return fieldn_on(p, c.st, d_in, n, d_off, nrec, k, limit, flags, d_out, cap, d_out_off, reinterpret_cast<uint64_t*>(d_valid), n_valid, out_len,
                     static_cast<hipStream_t>(stream));
}

// every string without the match at its start and the match at its end: steps 1 - 6 are the filter call's; 7 the words the
// markers of every string's first and last two matches park, and the bounds from them — the ranges, also into the caller's d_begin
// and d_end, before the capacity decision; 8 and 9 the field call's count and emit passes with k = 0: every string has its entry
static int trim_on(trre_prog* p, DeviceState* st, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint32_t flags, uint8_t* d_out,
                   size_t cap, int64_t* d_out_off, int64_t* d_begin, int64_t* d_end, size_t* out_len, hipStream_t s) {
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
    HIP_TRY(cx->d_field_bounds.reserve(nrec, 2 * nrec * 8));
    HIP_TRY(cx->d_trim_marks.reserve(nrec, 6 * nrec * 8));
    TrimArgs t{};
    t.flags = flags; t.marks = cx->d_trim_marks; t.begin = d_begin; t.end = d_end;
    FieldArgs& a = t.a;
    a.k = 0; a.lo = cx->d_field_bounds; a.hi = a.lo + nrec;
    rc = filter_tiles(cx, mk.pa, d_in, n, d_off, nrec, s, &a.f, [&](const SpanArgs& pa) { launch_trim_bounds(pa, t, s); });
    if (rc) return rc;
    launch_field_count(a, s);
    uint64_t tot[2] = {0, 0};
    rc = scan_counts(a.f.cnt, a.f.base, 2, a.f.tiles, s, tot);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (tot[0] != nrec || tot[1] > n) return fail(TRRE_E_DEVICE, "error: the trimmed strings do not add up (internal)");
    const size_t bytes = (size_t)tot[1];
    if (out_len) *out_len = bytes;
    if (bytes > cap) return fail(TRRE_E_CAPACITY, "error: output buffer too small");
    if (d_out_off) {
        a.f.out = d_out; a.f.out_len = (int64_t)bytes; a.f.out_off = d_out_off;
        launch_field_emit(a, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    return TRRE_OK;
}

int trre_trim_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint32_t flags, uint8_t* d_out, size_t cap,
                             int64_t* d_out_off, int64_t* d_begin, int64_t* d_end, size_t* out_len, void* stream) {
    g_scan_flags = 0;
    if (out_len) *out_len = 0;
    if (!p || !d_off || (n && !d_in) || (cap && !d_out) || (!d_out_off && (d_out || cap)) || (!d_begin != !d_end))
        return fail(TRRE_E_ARG, "error: null argument");
    if (!flags || (flags & ~(TRRE_TRIM_LEFT | TRRE_TRIM_RIGHT)))
        return fail(TRRE_E_ARG, "error: flags must be TRRE_TRIM_LEFT, TRRE_TRIM_RIGHT or both");
    if (int rc = spans_program(p, "trimmed strings")) return rc;
    if (nrec >= ((size_t)1 << 55) || n >= ((size_t)1 << 55)) return fail(TRRE_E_ARG, "error: too many records or bytes");
    const size_t ob = (nrec + 1) * 8, pb = d_out_off ? ob : 0, rb = d_begin ? nrec * 8 : 0, cb = d_out ? cap : 0;
    if (ranges_overlap(d_in, n, d_out, cb)) return fail(TRRE_E_ARG, "error: the output overlaps the input (the trimmed strings are not made in place)");
    if (any_overlap({{d_in, n}, {d_out, cb}}, {{d_off, ob}, {d_out_off, pb}, {d_begin, rb}, {d_end, rb}}))
        return fail(TRRE_E_ARG, "error: an offsets array overlaps the data or another offsets array");
    ColumnCall c;
    if (const int rc = c.begin(p)) return rc;
    return trim_on(p, c.st, d_in, n, d_off, nrec, flags, d_out, cap, d_out_off, d_begin, d_end, out_len, static_cast<hipStream_t>(stream));
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
    const uint64_t* before = nullptr;
    rc = find_texts(p->sub_texts.get(), stt, cx, total, stt->ctx.d_framed, found, s, &m, &before);
    if (rc) return rc;                                      // (TRRE_E_DIVERGES: the caller's sizes stay 0)
    const int64_t T = str_tile_bytes(), utiles = ((int64_t)m + T - 1) / T;
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

}  // extern "C"
