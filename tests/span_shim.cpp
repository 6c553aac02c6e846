// span_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of k_span_count and k_span_emit (trre_amd/csrc/records_block.hpp:
// span_mark_vecs, span_seg_count, span_fill_pv, span_emit_pieces, with k_chunk_scan between them) on the host, thread by thread, a
// wave as 64 sequential lanes, barriers as loop boundaries, so that tests/test_span_shim.py can check them against numpy without
// a GPU.  Not a product path: nothing in trre_amd/ links this file.  With -DSPAN_SHIM_MAIN the file is a program of its own that
// drives the same entry point over generated shapes: tests/test_span_shim.py builds that program with
// -fsanitize=address,undefined and runs it (a process of its own: a sanitized build is never loaded into an interpreter).
//
// pos0 (a multiple of the tile), ra0 and rl0 place the framed text as if pos0 framed bytes holding ra0 A, ra0 B and rl0 newlines
// came before it: the tiles that run are those from pos0 / TILE on, and every position and rank carries the shift — the
// arithmetic beyond 2^32.  Only the bytes and words of the text itself exist; the pointers are shifted to match.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "column_shim.hpp"

using namespace trre;

namespace {

// k_span_count, k_chunk_scan (three times), k_span_emit
template <class G>
int run(const uint8_t* framed, int64_t m, int64_t found, int64_t lines, int lists_only, int64_t pos0, int64_t ra0, int64_t rl0, int64_t* start,
        int64_t* end, int64_t* list_off, int64_t* totals, int64_t* stores) {
    if (pos0 % G::TILE) return 6;
    // the framed text at a 16-byte aligned address with whole vectors behind its end, as the library's buffer is
    std::vector<uint8_t> buf((size_t)m + 64 + 16, 0xEE);
    uint8_t* v0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 15) & ~(uintptr_t)15);
    if (m) std::memcpy(v0, framed, (size_t)m);
    const int64_t b0 = pos0 / G::TILE, tiles = (m + G::TILE - 1) / G::TILE;
    std::vector<uint64_t> cnt((size_t)(3 * tiles) + 1, 0), base((size_t)(3 * (tiles + 1)), 0);
    Padded<int64_t> ws(found, kUnstored), we(found, kUnstored), wl(lines + 1, kUnstored);
    SpanArgs a{};
    a.src = shifted(v0, pos0); a.total = pos0 + m; a.tiles = tiles;
    a.cnt = shifted(cnt.data(), b0); a.base = shifted(static_cast<const uint64_t*>(base.data()), b0);
    a.start = shifted(ws.data(), ra0); a.end = shifted(we.data(), ra0); a.list_off = shifted(wl.data(), rl0);
    a.n_match = lists_only ? 0 : ra0 + found; a.nrec = rl0 + lines; a.lists_only = (uint32_t)lists_only;
    // k_span_count: the threads' counts, summed per tile
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        uint64_t t[3] = {0, 0, 0};
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint32_t c[3] = {0, 0, 0};
            span_mark_vecs<G>(a, b, tid, nullptr, c);
            for (int x = 0; x < 3; ++x) t[x] += c[x];
        }
        for (int x = 0; x < 3; ++x) a.cnt[x * tiles + b] = t[x];
    }
    // k_chunk_scan
    const int64_t rank0[3] = {ra0, ra0, rl0};
    for (int x = 0; x < 3; ++x) {
        uint64_t run = (uint64_t)rank0[x];
        for (int64_t k = 0; k < tiles; ++k) { base[(size_t)(x * (tiles + 1) + k)] = run; run += cnt[(size_t)(x * tiles + k)]; }
        base[(size_t)(x * (tiles + 1) + tiles)] = run;
        totals[x] = (int64_t)run - rank0[x];
    }
    if (totals[0] != found || totals[1] != found || totals[2] != lines) return 4;
    // k_span_emit
    std::vector<uint16_t> bits((size_t)3 * G::NVEC);
    std::vector<uint32_t> pv_ab(G::NVEC), pv_nl(G::NVEC), pre_ab(G::THREADS), pre_nl(G::THREADS);
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        std::fill(bits.begin(), bits.end(), (uint16_t)0xA5A5);                          // (what a tile before left there)
        std::fill(pv_ab.begin(), pv_ab.end(), 0xDEADBEEFu);
        std::fill(pv_nl.begin(), pv_nl.end(), 0xDEADBEEFu);
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint32_t c[3] = {0, 0, 0};
            span_mark_vecs<G>(a, b, tid, bits.data(), c);
        }
        uint32_t run_ab = 0, run_nl = 0;                                                // (barrier; the workgroup's two scans)
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint32_t ab, nl;
            span_seg_count<G>(bits.data(), tid, ab, nl);
            pre_ab[tid] = run_ab; pre_nl[tid] = run_nl;
            run_ab += ab; run_nl += nl;
        }
        if ((run_ab & 0xffffu) != cnt[(size_t)(b - b0)] || (run_ab >> 16) != cnt[(size_t)(tiles + b - b0)] || run_nl != cnt[(size_t)(2 * tiles + b - b0)]) return 5;
        for (int tid = 0; tid < G::THREADS; ++tid) span_fill_pv<G>(bits.data(), pre_ab[tid], pre_nl[tid], tid, pv_ab.data(), pv_nl.data());
        // (barrier) the words: wave by wave, the lanes of a wave in turn; a word may be stored once
        const std::vector<int64_t> bs(ws.w), be(we.w), bl(wl.w);
        for (int tid = 0; tid < G::THREADS; ++tid) span_emit_pieces<G>(a, b, tid, bits.data(), pv_ab.data(), pv_nl.data());
        bool twice = false;
        *stores += changed(ws.w, bs, kUnstored, &twice) + changed(we.w, be, kUnstored, &twice) + changed(wl.w, bl, kUnstored, &twice);
        if (twice) return 7;                                                            // a word stored by two tiles
    }
    if (found) { std::memcpy(start, ws.data(), (size_t)found * 8); std::memcpy(end, we.data(), (size_t)found * 8); }
    std::memcpy(list_off, wl.data(), (size_t)(lines + 1) * 8);
    return ws.pads_intact() && we.pads_intact() && wl.pads_intact() ? 0 : 8;
}

}  // namespace

extern "C" {

int64_t shim_span_tile(int geo) { return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE; }

// framed: m bytes holding `found` A (0x01), `found` B (0x02) and `lines` newlines.  Out: start[0 .. found), end[0 .. found),
// list_off[0 .. lines] as the kernel leaves them (a word nobody stored reads 0xEE..EE: list_off[0] when pos0 is not 0; every
// start and end with lists_only); totals[3]: what the count pass and the scans found; *stores: words stored.
// 4: framed does not hold those counts, 5: the two kernels disagree on a tile, 7: a word was stored twice, 8: a word outside
// the arrays was written
int shim_span(int geo, const uint8_t* framed, int64_t m, int64_t found, int64_t lines, int lists_only, int64_t pos0, int64_t ra0, int64_t rl0,
              int64_t* start, int64_t* end, int64_t* list_off, int64_t* totals, int64_t* stores) {
    *stores = 0;
    switch (geo) {
    case 0: return run<Geo0>(framed, m, found, lines, lists_only, pos0, ra0, rl0, start, end, list_off, totals, stores);
    case 1: return run<Geo1>(framed, m, found, lines, lists_only, pos0, ra0, rl0, start, end, list_off, totals, stores);
    case 2: return run<Geo2>(framed, m, found, lines, lists_only, pos0, ra0, rl0, start, end, list_off, totals, stores);
    default: return run<Geo3>(framed, m, found, lines, lists_only, pos0, ra0, rl0, start, end, list_off, totals, stores);
    }
}

}  // extern "C"

#ifdef SPAN_SHIM_MAIN
// The entry point over generated shapes, checked against a plain restatement: framed lengths around the tile edges; no marker,
// every byte a marker ("AB\n" repeated, "ABAB.."), A on the last byte of a piece or tile with its B on the first of the next,
// newlines at the first and last byte of tiles, random texts; the list-offsets-only flag; a shift beyond 2^32.
namespace {

uint32_t rng_state = 9876;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

std::vector<uint8_t> text(int pattern, int64_t m, int64_t T) {
    std::vector<uint8_t> f((size_t)m, (uint8_t)'.');
    bool open = false;
    for (int64_t x = 0; x < m; ++x) {
        uint8_t c = '.';
        switch (pattern) {
        case 0: break;
        case 1: c = (uint8_t)(x % 3 == 0 ? 1 : x % 3 == 1 ? 2 : '\n'); if (x % 3 == 0 && x + 1 >= m) c = '.'; break;
        case 2: c = (uint8_t)(x % 2 == 0 ? 1 : 2); if (x % 2 == 0 && x + 1 >= m) c = '.'; break;
        case 3: c = (uint8_t)(x % 64 == 63 ? 1 : x % 64 == 0 && x ? 2 : '.'); if (c == 1 && x + 1 >= m) c = '.'; break;
        case 4: c = (uint8_t)(x % T == T - 1 ? 1 : x % T == 0 && x ? 2 : '.'); if (c == 1 && x + 1 >= m) c = '.'; break;
        case 5: c = (uint8_t)(x % T == 0 || x % T == T - 1 ? '\n' : '.'); break;
        default: {
            const uint32_t r = rnd() % 8;
            if (!open && r == 0 && x + 1 < m) { c = 1; open = true; }
            else if (open && (r < 3 || x + 1 == m)) { c = 2; open = false; }
            else if (!open && r == 1) c = '\n';
        }
        }
        f[(size_t)x] = c;
    }
    return f;
}

int check(int geo, int64_t m, int pattern, int lists_only, int64_t pos0, int64_t ra0, int64_t rl0) {
    const int64_t T = shim_span_tile(geo);
    const std::vector<uint8_t> f = text(pattern, m, T);
    std::vector<int64_t> ws, we, wl{0};
    int64_t na = ra0, nb = ra0, nl = rl0;
    for (int64_t x = 0; x < m; ++x) {
        const int64_t pos = pos0 + x - na - nb - nl;
        if (f[(size_t)x] == 1) { ws.push_back(pos); ++na; }
        else if (f[(size_t)x] == 2) { we.push_back(pos); ++nb; }
        else if (f[(size_t)x] == '\n') { wl.push_back(na); ++nl; }
    }
    if (ws.size() != we.size()) return 20;
    const int64_t found = (int64_t)ws.size(), lines = (int64_t)wl.size() - 1;
    std::vector<int64_t> gs((size_t)found + 1, -1), ge((size_t)found + 1, -1), gl((size_t)lines + 1, -1);
    int64_t totals[3], stores = 0;
    const int rc = shim_span(geo, f.data(), m, found, lines, lists_only, pos0, ra0, rl0, gs.data(), ge.data(), gl.data(), totals, &stores);
    if (rc) return rc;
    for (int64_t j = 0; j < found; ++j) {
        if (gs[(size_t)j] != (lists_only ? kUnstored : ws[(size_t)j])) return 11;
        if (ge[(size_t)j] != (lists_only ? kUnstored : we[(size_t)j])) return 12;
    }
    for (int64_t i = 1; i <= lines; ++i)
        if (gl[(size_t)i] != wl[(size_t)i]) return 13;
    if (gl[0] != (m && !pos0 ? 0 : kUnstored)) return 14;
    if (stores != (lists_only ? 0 : 2 * found) + lines + (m && !pos0 ? 1 : 0)) return 15;
    return 0;
}

}  // namespace

int main() {
    int runs = 0;
    for (int geo = 0; geo < 4; ++geo) {
        const int64_t T = shim_span_tile(geo);
        const int64_t sizes[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T, 2 * T + 77};
        for (int64_t m : sizes)
            for (int pattern = 0; pattern < 7; ++pattern)
                for (int lists_only = 0; lists_only < 2; ++lists_only) {
                    const bool far = (runs % 3) == 2;
                    const int rc = check(geo, m, pattern, lists_only, far ? ((5ll << 32) / T + 3) * T : 0, far ? (1ll << 32) + 5 : 0, far ? (1ll << 33) + 7 : 0);
                    if (rc) { std::printf("FAILED: geo %d m %lld pattern %d lists_only %d far %d: %d\n", geo, (long long)m, pattern, lists_only, (int)far, rc); return 1; }
                    ++runs;
                }
    }
    std::printf("span_shim: %d shapes ok\n", runs);
    return 0;
}
#endif
