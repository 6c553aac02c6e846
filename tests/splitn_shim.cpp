// splitn_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of k_splitn_count and k_splitn_emit (trre_amd/csrc/
// records_block.hpp: splitn_cut_markers, splitn_tile_depth, splitn_seg_cut, splitn_seg_kept, splitn_fill_pv, splitn_emit_pieces,
// behind k_span_count's counts and with k_chunk_scan between them) and of k_fieldn_init, k_fieldn_pick and k_fieldn_count
// (fieldn_init, fieldn_pick_markers, fieldn_count_strings) on the host, thread by thread, a wave as 64 sequential lanes, barriers
// as loop boundaries, so that tests/test_splitn_shim.py can check them against numpy without a GPU.  Not a product path: nothing
// in trre_amd/ links this file.  With -DSPLITN_SHIM_MAIN the file is a program of its own that drives the same entry points over
// generated shapes, for a build with -fsanitize=address,undefined (a process of its own: a sanitized build is never loaded into
// an interpreter).
//
// pos0 (a multiple of the tile), ra0, rl0, rk0 and rc0 place the framed text as if pos0 framed bytes holding ra0 A, ra0 B, rl0
// newlines, rk0 kept bytes and rc0 cutting matches came before it, as split_shim.cpp does.  The framed text ends with a newline:
// every marker belongs to a string.  The list offsets L the kernels look the rule up in are made here, by a plain loop.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "column_shim.hpp"

using namespace trre;

namespace {

// L[i + 1] = ra0 + the A before newline i of the text
std::vector<int64_t> list_offsets(const uint8_t* framed, int64_t m, int64_t ra0) {
    std::vector<int64_t> L{ra0};
    int64_t na = ra0;
    for (int64_t x = 0; x < m; ++x) {
        if (framed[x] == 1) ++na;
        else if (framed[x] == '\n') L.push_back(na);
    }
    return L;
}

struct Shift { int64_t pos0, ra0, rl0, rk0, rc0; };

// k_span_count, k_chunk_scan (three times), k_splitn_count, k_chunk_scan (twice), k_splitn_emit
template <class G>
int run(const uint8_t* framed, int64_t m, const uint8_t* in, int64_t n, int64_t found, int64_t lines, int64_t limit, uint32_t flags, int64_t kept,
        int64_t cuts, int lists_only, const Shift& sh, uint8_t* out, int64_t* piece_off, int64_t* list_off, int64_t* totals, int64_t* stores) {
    const int64_t pos0 = sh.pos0, ra0 = sh.ra0, rl0 = sh.rl0, rk0 = sh.rk0, rc0 = sh.rc0;
    if (pos0 % G::TILE) return 6;
    if (m && framed[m - 1] != '\n') return 6;
    const int64_t in0 = pos0 - 2 * ra0 - rl0;      // source bytes before the text
    if (in0 < 0) return 6;
    std::vector<uint8_t> buf((size_t)m + 64 + 16, 0xEE);
    uint8_t* v0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 15) & ~(uintptr_t)15);
    if (m) std::memcpy(v0, framed, (size_t)m);
    const int64_t b0 = pos0 / G::TILE, tiles = (m + G::TILE - 1) / G::TILE, pieces = cuts + lines;
    std::vector<uint64_t> cnt((size_t)(3 * tiles) + 1, 0), base((size_t)(3 * (tiles + 1)), 0), kcnt((size_t)(2 * tiles) + 1, 0),
        kbase((size_t)(2 * (tiles + 1)), 0);
    const std::vector<int64_t> L = list_offsets(framed, m, ra0);
    if ((int64_t)L.size() != lines + 1) return 4;
    Padded<uint8_t> wo(kept, kUnstoredByte);
    Padded<int64_t> wp(pieces + 1, kUnstored), wl(lines + 1, kUnstored);
    SpanArgs sp{};
    sp.src = shifted(v0, pos0); sp.total = pos0 + m; sp.tiles = tiles;
    sp.cnt = shifted(cnt.data(), b0);
    SplitnArgs a{};
    a.L = shifted(L.data(), rl0); a.limit = limit; a.flags = flags;
    SplitArgs& s = a.s;
    s.src = sp.src; s.total = sp.total; s.tiles = tiles;
    s.in = shifted(in, in0); s.n = in0 + n;
    s.base = shifted(static_cast<const uint64_t*>(base.data()), b0);
    s.kcnt = shifted(kcnt.data(), b0); s.kbase = shifted(static_cast<const uint64_t*>(kbase.data()), b0);
    s.list_off = shifted(wl.data(), rl0); s.nrec = rl0 + lines; s.lists_only = (uint32_t)lists_only;
    if (!lists_only) {
        s.out = shifted(wo.data(), rk0); s.out_len = rk0 + kept;
        s.piece_off = shifted(wp.data(), rc0 + rl0); s.n_piece = rc0 + rl0 + pieces;
    }
    // k_span_count
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        uint64_t t[3] = {0, 0, 0};
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint32_t c[3] = {0, 0, 0};
            span_mark_vecs<G>(sp, b, tid, nullptr, c);
            for (int x = 0; x < 3; ++x) t[x] += c[x];
        }
        for (int x = 0; x < 3; ++x) sp.cnt[x * tiles + b] = t[x];
    }
    // k_chunk_scan
    const int64_t rank0[3] = {ra0, ra0, rl0};
    for (int x = 0; x < 3; ++x) {
        uint64_t sum = (uint64_t)rank0[x];
        for (int64_t k = 0; k < tiles; ++k) { base[(size_t)(x * (tiles + 1) + k)] = sum; sum += cnt[(size_t)(x * tiles + k)]; }
        base[(size_t)(x * (tiles + 1) + tiles)] = sum;
        totals[x] = (int64_t)sum - rank0[x];
    }
    if (totals[0] != found || totals[1] != found || totals[2] != lines) return 4;
    // what both kernels share up to the cut image and the scan of its bits (splitn_tile_cuts)
    std::vector<uint16_t> bits((size_t)3 * G::NVEC), kbits(G::NVEC);
    std::vector<uint32_t> cut32((size_t)G::NVEC / 2 + 1), pv_ab(G::NVEC), pv_nl(G::NVEC), pv_kc(G::NVEC), pre_ab(G::THREADS), pre_nl(G::THREADS),
        pre_c(G::THREADS), pre_k(G::THREADS);
    auto tile_cuts = [&](int64_t b) {
        std::fill(bits.begin(), bits.end(), (uint16_t)0xA5A5);                          // (what a tile before left there)
        std::fill(pv_ab.begin(), pv_ab.end(), 0xDEADBEEFu);
        std::fill(pv_nl.begin(), pv_nl.end(), 0xDEADBEEFu);
        for (int tid = 0; tid < G::THREADS; ++tid) split_mark_vecs<G>(s, b, tid, bits.data());
        std::fill(cut32.begin(), cut32.end(), 0u);
        uint32_t run_ab = 0, run_nl = 0, run_c = 0;                                     // (barrier; the workgroup's scans)
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint32_t ab, nl;
            span_seg_count<G>(bits.data(), tid, ab, nl);
            pre_ab[tid] = run_ab; pre_nl[tid] = run_nl;
            run_ab += ab; run_nl += nl;
        }
        for (int tid = 0; tid < G::THREADS; ++tid) span_fill_pv<G>(bits.data(), pre_ab[tid], pre_nl[tid], tid, pv_ab.data(), pv_nl.data());
        for (int tid = 0; tid < G::THREADS; ++tid) splitn_cut_markers<G>(a, b, tid, bits.data(), pv_ab.data(), pv_nl.data(), cut32.data());
        const uint16_t* cut = reinterpret_cast<const uint16_t*>(cut32.data());          // (barrier)
        for (int tid = 0; tid < G::THREADS; ++tid) { pre_c[tid] = run_c; run_c += splitn_seg_cut<G>(bits.data(), cut, tid); }
        return cut;
    };
    // k_splitn_count
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        const uint16_t* cut = tile_cuts(b);
        uint64_t t = 0, c = 0;
        for (int tid = 0; tid < G::THREADS; ++tid) {
            t += splitn_seg_kept<G>(a, b, tid, bits.data(), cut, splitn_tile_depth(a, b), pre_c[tid], nullptr);
            c += splitn_seg_cut<G>(bits.data(), cut, tid) >> 16;
        }
        s.kcnt[b] = t; s.kcnt[tiles + b] = c;
    }
    // k_chunk_scan, twice
    const int64_t krank0[2] = {rk0, rc0};
    for (int x = 0; x < 2; ++x) {
        uint64_t sum = (uint64_t)krank0[x];
        for (int64_t k = 0; k < tiles; ++k) { kbase[(size_t)(x * (tiles + 1) + k)] = sum; sum += kcnt[(size_t)(x * tiles + k)]; }
        kbase[(size_t)(x * (tiles + 1) + tiles)] = sum;
        totals[3 + x] = (int64_t)sum - krank0[x];
    }
    if (totals[3] != kept || totals[4] != cuts) return 4;
    // k_splitn_emit
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        const uint16_t* cut = tile_cuts(b);
        std::fill(kbits.begin(), kbits.end(), (uint16_t)0xA5A5);
        std::fill(pv_kc.begin(), pv_kc.end(), 0xDEADBEEFu);
        uint32_t run_k = 0;
        for (int tid = 0; tid < G::THREADS; ++tid) {
            pre_k[tid] = run_k;
            run_k += splitn_seg_kept<G>(a, b, tid, bits.data(), cut, splitn_tile_depth(a, b), pre_c[tid], kbits.data());
        }
        if (run_k != kcnt[(size_t)(b - b0)]) return 5;
        for (int tid = 0; tid < G::THREADS; ++tid) splitn_fill_pv<G>(bits.data(), cut, kbits.data(), pre_k[tid], pre_c[tid], tid, pv_kc.data());
        // (barrier) the bytes and words: wave by wave, the lanes of a wave in turn; each may be stored once
        const std::vector<uint8_t> bo(wo.w);
        const std::vector<int64_t> bp(wp.w), bl(wl.w);
        for (int tid = 0; tid < G::THREADS; ++tid)
            splitn_emit_pieces<G>(a, b, tid, bits.data(), cut, kbits.data(), pv_ab.data(), pv_nl.data(), pv_kc.data());
        bool twice = false;
        stores[0] += changed(wo.w, bo, kUnstoredByte, &twice);
        stores[1] += changed(wp.w, bp, kUnstored, &twice);
        stores[2] += changed(wl.w, bl, kUnstored, &twice);
        if (twice) return 7;                                                            // stored by two tiles
    }
    if (kept) std::memcpy(out, wo.data(), (size_t)kept);
    std::memcpy(piece_off, wp.data(), (size_t)(pieces + 1) * 8);
    std::memcpy(list_off, wl.data(), (size_t)(lines + 1) * 8);
    return wo.pads_intact() && wp.pads_intact() && wl.pads_intact() ? 0 : 8;
}

// k_fieldn_init, k_span_count with its scans, k_fieldn_pick, k_filter_part, k_fieldn_count: the bounds, the bitmap and the two totals
template <class G>
int run_bounds(const uint8_t* framed, int64_t m, const int64_t* off, int64_t nrec, int64_t k, int64_t limit, uint32_t flags, int64_t* lo, int64_t* hi,
               uint64_t* valid, int64_t* totals, int64_t* stores) {
    if (nrec < 1 || !m || framed[m - 1] != '\n') return 6;
    const int64_t words = (nrec + 63) / 64, n = off[nrec];
    std::vector<uint8_t> fbuf((size_t)m + 64 + 16, 0xEE);
    uint8_t* f0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(fbuf.data()) + 15) & ~(uintptr_t)15);
    std::memcpy(f0, framed, (size_t)m);
    const std::vector<int64_t> L = list_offsets(framed, m, 0);
    if ((int64_t)L.size() != nrec + 1) return 3;
    Padded<int64_t> wlo(nrec, kUnstored), whi(nrec, kUnstored), wv(words, kUnstored);
    const int64_t tiles = (n + G::TILE - 1) / G::TILE > 0 ? (n + G::TILE - 1) / G::TILE : 1;
    FieldnArgs fn{};
    fn.limit = limit; fn.flags = flags;
    FieldArgs& a = fn.a;
    a.f.vbeg = 0; a.f.n = n; a.f.off = off; a.f.loff = L.data(); a.f.nrec = nrec; a.f.tiles = tiles;
    a.k = k; a.lo = wlo.data(); a.hi = whi.data(); a.valid = reinterpret_cast<uint64_t*>(wv.data()); a.words = words;
    bool twice = false;
    {
        const std::vector<int64_t> bl(wlo.w), bh(whi.w);
        const int64_t groups = (nrec + kMatchThreads - 1) / kMatchThreads;
        for (int64_t at = 0; at < groups * (kMatchThreads / 64); ++at) {
            uint64_t word = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int64_t i = at * 64 + lane;
                if (i < nrec && fieldn_init(fn, i)) word |= 1ull << lane;
            }
            if (at < a.words) { a.valid[at] = word; stores[0] += 1; }
        }
        stores[1] += changed(wlo.w, bl, kUnstored, &twice);
        stores[2] += changed(whi.w, bh, kUnstored, &twice);
    }
    const int64_t ftiles = (m + G::TILE - 1) / G::TILE;
    std::vector<uint64_t> fcnt((size_t)(3 * ftiles) + 1, 0), fbase((size_t)(3 * (ftiles + 1)), 0);
    SpanArgs sp{};
    sp.src = f0; sp.total = m; sp.tiles = ftiles; sp.nrec = nrec; sp.lists_only = 1u;
    sp.cnt = fcnt.data(); sp.base = fbase.data();
    for (int64_t b = 0; b < ftiles; ++b) {
        uint64_t t[3] = {0, 0, 0};
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint32_t cc[3] = {0, 0, 0};
            span_mark_vecs<G>(sp, b, tid, nullptr, cc);
            for (int x = 0; x < 3; ++x) t[x] += cc[x];
        }
        for (int x = 0; x < 3; ++x) sp.cnt[x * ftiles + b] = t[x];
    }
    for (int x = 0; x < 3; ++x) {
        uint64_t sum = 0;
        for (int64_t q = 0; q < ftiles; ++q) { fbase[(size_t)(x * (ftiles + 1) + q)] = sum; sum += fcnt[(size_t)(x * ftiles + q)]; }
        fbase[(size_t)(x * (ftiles + 1) + ftiles)] = sum;
        if ((int64_t)sum != (x < 2 ? L[(size_t)nrec] : nrec)) return 3;
    }
    {
        std::vector<uint16_t> bits((size_t)3 * G::NVEC);
        std::vector<uint32_t> pv_ab(G::NVEC), pv_nl(G::NVEC), pre_ab(G::THREADS), pre_nl(G::THREADS);
        for (int64_t b = 0; b < ftiles; ++b) {
            std::fill(bits.begin(), bits.end(), (uint16_t)0xA5A5);
            for (int tid = 0; tid < G::THREADS; ++tid) {
                uint32_t cc[3] = {0, 0, 0};
                span_mark_vecs<G>(sp, b, tid, bits.data(), cc);
            }
            uint32_t run_ab = 0, run_nl = 0;
            for (int tid = 0; tid < G::THREADS; ++tid) {
                uint32_t ab, nl;
                span_seg_count<G>(bits.data(), tid, ab, nl);
                pre_ab[tid] = run_ab; pre_nl[tid] = run_nl;
                run_ab += ab; run_nl += nl;
            }
            for (int tid = 0; tid < G::THREADS; ++tid) span_fill_pv<G>(bits.data(), pre_ab[tid], pre_nl[tid], tid, pv_ab.data(), pv_nl.data());
            const std::vector<int64_t> bl(wlo.w), bh(whi.w);
            for (int tid = 0; tid < G::THREADS; ++tid) fieldn_pick_markers<G>(fn, sp, b, tid, bits.data(), pv_ab.data(), pv_nl.data());
            stores[1] += changed(wlo.w, bl, kUnstored, &twice);
            stores[2] += changed(whi.w, bh, kUnstored, &twice);
        }
    }
    if (twice) return 7;
    std::memcpy(lo, wlo.data(), (size_t)nrec * 8);
    std::memcpy(hi, whi.data(), (size_t)nrec * 8);
    std::memcpy(valid, wv.data(), (size_t)words * 8);
    if (stores[1] != nrec || stores[2] != nrec) return 9;
    std::vector<int64_t> part((size_t)tiles + 1, -1);
    a.f.part = part.data();
    for (int64_t b = 0; b <= tiles; ++b) filter_part(a.f, G::TILE, b);
    totals[0] = totals[1] = 0;
    for (int64_t b = 0; b < tiles; ++b) {
        const FilterTile<G> t(a.f, b);
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint64_t vv, kk;
            fieldn_count_strings<G>(fn, t, tid, vv, kk);
            totals[0] += (int64_t)vv; totals[1] += (int64_t)kk;
        }
    }
    return wv.pads_intact() && wlo.pads_intact() && whi.pads_intact() ? 0 : 8;
}

}  // namespace

extern "C" {

int64_t shim_splitn_tile(int geo) { return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE; }

// the rule itself, for the tests of the yardstick
int shim_splitn_cuts(int64_t r, int64_t c, int64_t limit, uint32_t flags) { return splitn_cuts(r, c, limit, flags) ? 1 : 0; }

// framed: m bytes holding `found` A (0x01), `found` B (0x02), `lines` newlines (the last byte is one) and n position bytes; in: the
// n source bytes, none of them 0xEE; kept, cuts: the bytes outside the cutting matches and the cutting matches under (limit,
// flags).  Out: out[0 .. kept), piece_off[0 .. cuts + lines], list_off[0 .. lines] as the kernels leave them (a byte or word nobody
// stored reads 0xEE); totals[5]: A, B, newlines, kept bytes, cutting matches as the count passes and the scans found them;
// stores[3]: bytes of out, words of piece_off, words of list_off stored.
// 4: framed does not hold those counts, 5: the two kernels disagree on a tile, 6: bad arguments, 7: a byte or word was stored
// twice, 8: one outside the arrays was written
int shim_splitn(int geo, const uint8_t* framed, int64_t m, const uint8_t* in, int64_t n, int64_t found, int64_t lines, int64_t limit, uint32_t flags,
                int64_t kept, int64_t cuts, int lists_only, int64_t pos0, int64_t ra0, int64_t rl0, int64_t rk0, int64_t rc0, uint8_t* out,
                int64_t* piece_off, int64_t* list_off, int64_t* totals, int64_t* stores) {
    stores[0] = stores[1] = stores[2] = 0;
    const Shift sh{pos0, ra0, rl0, rk0, rc0};
    switch (geo) {
    case 0: return run<Geo0>(framed, m, in, n, found, lines, limit, flags, kept, cuts, lists_only, sh, out, piece_off, list_off, totals, stores);
    case 1: return run<Geo1>(framed, m, in, n, found, lines, limit, flags, kept, cuts, lists_only, sh, out, piece_off, list_off, totals, stores);
    case 2: return run<Geo2>(framed, m, in, n, found, lines, limit, flags, kept, cuts, lists_only, sh, out, piece_off, list_off, totals, stores);
    default: return run<Geo3>(framed, m, in, n, found, lines, limit, flags, kept, cuts, lists_only, sh, out, piece_off, list_off, totals, stores);
    }
}

// framed as above, for nrec strings with the offsets off [nrec + 1] from 0.  Out: lo, hi [nrec] and valid [ceil(nrec / 64)] as
// k_fieldn_init and k_fieldn_pick leave them; totals[2]: the strings with the field and the field bytes k_fieldn_count finds;
// stores[3]: words of the bitmap, of lo, of hi stored.  3: framed does not go with nrec, 7: a bound was stored twice, 8: a word
// outside the arrays was written, 9: a bound was not stored
int shim_fieldn_bounds(int geo, const uint8_t* framed, int64_t m, const int64_t* off, int64_t nrec, int64_t k, int64_t limit, uint32_t flags,
                       int64_t* lo, int64_t* hi, uint64_t* valid, int64_t* totals, int64_t* stores) {
    stores[0] = stores[1] = stores[2] = 0;
    switch (geo) {
    case 0: return run_bounds<Geo0>(framed, m, off, nrec, k, limit, flags, lo, hi, valid, totals, stores);
    case 1: return run_bounds<Geo1>(framed, m, off, nrec, k, limit, flags, lo, hi, valid, totals, stores);
    case 2: return run_bounds<Geo2>(framed, m, off, nrec, k, limit, flags, lo, hi, valid, totals, stores);
    default: return run_bounds<Geo3>(framed, m, off, nrec, k, limit, flags, lo, hi, valid, totals, stores);
    }
}

}  // extern "C"

#ifdef SPLITN_SHIM_MAIN
// Both entry points over generated shapes, checked against a plain restatement of the rule: framed lengths around the tile edges;
// no marker, one match over whole tiles, every byte a marker, A on the last byte of a piece or tile with its B on the first of
// the next, random texts; limits 0, 1, 2, many, -1 and the two ends of int64, from either end; the lists-only flag; a shift
// beyond 2^32.
#include <climits>
namespace {

uint32_t rng_state = 13579;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

std::vector<uint8_t> text(int pattern, int64_t m, int64_t T) {
    std::vector<uint8_t> f((size_t)m, (uint8_t)'.');
    bool open = false;
    for (int64_t x = 0; x + 1 < m; ++x) {
        uint8_t c = '.';
        const bool room = x + 2 < m;               // an A needs its B in front of the closing newline
        switch (pattern) {
        case 0: break;
        case 1: c = (uint8_t)(x % 3 == 0 ? (room ? 1 : '.') : x % 3 == 1 ? (f[(size_t)x - 1] == 1 ? 2 : '.') : '\n'); break;
        case 2: c = (uint8_t)(x % 2 == 0 ? (room ? 1 : '.') : 2); break;
        case 3: c = (uint8_t)(x % 64 == 63 ? (room ? 1 : '.') : x % 64 == 0 && x ? 2 : '.'); break;
        case 4: c = (uint8_t)(x % T == T - 1 ? (room ? 1 : '.') : x % T == 0 && x ? 2 : '.'); break;
        case 5: c = (uint8_t)(x % T == 0 || x % T == T - 1 ? '\n' : '.'); break;
        case 6: c = (uint8_t)(m >= 8 && x == 2 ? 1 : m >= 8 && x == m - 3 ? 2 : '.'); break;     // one match over whole tiles
        default: {
            const uint32_t r = rnd() % 8;
            if (!open && r == 0 && room) { c = 1; open = true; }
            else if (open && (r < 3 || !room)) { c = 2; open = false; }
            else if (!open && r == 1) c = '\n';
        }
        }
        f[(size_t)x] = c;
    }
    if (m) f[(size_t)m - 1] = '\n';
    return f;
}

int check(int geo, int64_t m, int pattern, int64_t limit, uint32_t flags, int lists_only, const Shift& sh) {
    const int64_t T = shim_splitn_tile(geo);
    const std::vector<uint8_t> f = text(pattern, m, T);
    // the strings' matches, then the rule match by match
    std::vector<int64_t> per;                      // matches per string
    {
        int64_t c = 0;
        for (uint8_t b : f) { if (b == 1) ++c; else if (b == '\n') { per.push_back(c); c = 0; } }
    }
    std::vector<uint8_t> in, wo;
    std::vector<int64_t> wp{sh.rk0}, wl{0}, off{0}, lo, hi;
    int64_t found = 0, cuts = 0, line = 0, r = 0;
    bool inside = false, cutting = false;
    for (int64_t x = 0; x < m; ++x) {
        const uint8_t c = f[(size_t)x];
        if (c == 1) { inside = true; cutting = splitn_cuts(r, per[(size_t)line], limit, flags); ++found; }
        else if (c == 2) {
            if (!inside) return 20;
            inside = false; ++r;
            if (cutting) { ++cuts; wp.push_back(sh.rk0 + (int64_t)wo.size()); }
        } else if (c == '\n') {
            if (inside) return 20;
            ++line; r = 0;
            wp.push_back(sh.rk0 + (int64_t)wo.size()); wl.push_back(sh.rc0 + cuts + sh.rl0 + line);
            off.push_back((int64_t)in.size());
        } else {
            in.push_back((uint8_t)('a' + rnd() % 26));
            if (!(inside && cutting)) wo.push_back(in.back());
        }
    }
    const int64_t lines = line, kept = (int64_t)wo.size(), n = (int64_t)in.size();
    std::vector<uint8_t> go((size_t)kept + 1, 0x11);
    std::vector<int64_t> gp((size_t)(cuts + lines) + 2, -1), gl((size_t)lines + 2, -1);
    int64_t totals[5], stores[3];
    int rc = shim_splitn(geo, f.data(), m, in.data(), n, found, lines, limit, flags, kept, cuts, lists_only, sh.pos0, sh.ra0, sh.rl0, sh.rk0, sh.rc0,
                         go.data(), gp.data(), gl.data(), totals, stores);
    if (rc) return rc;
    const bool tile0 = m && !sh.pos0;
    for (int64_t k = 0; k < kept; ++k)
        if (go[(size_t)k] != (lists_only ? kUnstoredByte : wo[(size_t)k])) return 11;
    for (int64_t k = 1; k <= cuts + lines; ++k)
        if (gp[(size_t)k] != (lists_only ? kUnstored : wp[(size_t)k])) return 12;
    for (int64_t i = 1; i <= lines; ++i)
        if (gl[(size_t)i] != wl[(size_t)i]) return 13;
    if (gl[0] != (tile0 ? 0 : kUnstored) || gp[0] != (tile0 && !lists_only ? 0 : kUnstored)) return 14;
    if (go[(size_t)kept] != 0x11 || gp[(size_t)(cuts + lines) + 1] != -1 || gl[(size_t)lines + 1] != -1) return 16;
    if (stores[0] != (lists_only ? 0 : kept) || stores[1] != (lists_only ? 0 : cuts + lines + (tile0 ? 1 : 0)) || stores[2] != lines + (tile0 ? 1 : 0)) return 15;
    if (sh.pos0 || lists_only || !lines) return 0;
    // the field form's bounds, for a few k: every bound stored once, nothing outside
    for (int64_t k : {(int64_t)0, (int64_t)1, (int64_t)-1, (int64_t)-2, (int64_t)INT64_MIN, (int64_t)INT64_MAX}) {
        std::vector<int64_t> glo((size_t)lines), ghi((size_t)lines);
        std::vector<uint64_t> gv((size_t)(lines + 63) / 64);
        int64_t t2[2], s3[3];
        rc = shim_fieldn_bounds(geo, f.data(), m, off.data(), lines, k, limit, flags, glo.data(), ghi.data(), gv.data(), t2, s3);
        if (rc) return 30 + rc;
        int64_t valid = 0, bytes = 0;
        for (int64_t i = 0; i < lines; ++i) {
            if (glo[(size_t)i] < off[(size_t)i] || ghi[(size_t)i] > off[(size_t)i + 1] || glo[(size_t)i] > ghi[(size_t)i]) return 41;
            valid += (gv[(size_t)i / 64] >> (i % 64)) & 1u;
            bytes += ghi[(size_t)i] - glo[(size_t)i];
        }
        if (valid != t2[0] || bytes != t2[1]) return 42;
    }
    return 0;
}

}  // namespace

int main() {
    int runs = 0;
    const int64_t limits[] = {0, 1, 2, 1000000, -1, LLONG_MAX, LLONG_MIN};
    for (int geo = 0; geo < 4; ++geo) {
        const int64_t T = shim_splitn_tile(geo);
        const int64_t sizes[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T, 2 * T + 77};
        for (int64_t m : sizes)
            for (int pattern = 0; pattern < 8; ++pattern)
                for (int64_t limit : limits) {
                    if (geo == 3 && m > T + 1 && (runs % 2)) { ++runs; continue; }     // (the device's tiles: every other of the long ones)
                    const bool far = (runs % 3) == 2;
                    const Shift sh{far ? ((5ll << 32) / T + 3) * T : 0, far ? (1ll << 32) + 5 : 0, far ? (1ll << 33) + 7 : 0, far ? (1ll << 34) + 11 : 0,
                                   far ? (1ll << 31) + 3 : 0};
                    const uint32_t flags = (uint32_t)(runs & 1);
                    const int lists_only = (runs % 5) == 4;
                    const int rc = check(geo, m, pattern, limit, flags, lists_only, sh);
                    if (rc) {
                        std::printf("FAILED: geo %d m %lld pattern %d limit %lld flags %u lists_only %d far %d: %d\n", geo, (long long)m, pattern,
                                    (long long)limit, flags, lists_only, (int)far, rc);
                        return 1;
                    }
                    ++runs;
                }
    }
    std::printf("splitn_shim: %d shapes ok\n", runs);
    return 0;
}
#endif
