// split_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of k_split_count and k_split_emit (trre_amd/csrc/records_block.hpp:
// split_mark_vecs, split_seg_kept, split_fill_pv, split_emit_pieces, behind k_span_count's counts and with k_chunk_scan between
// them) on the host, thread by thread, a wave as 64 sequential lanes, barriers as loop boundaries, so that
// tests/test_split_shim.py can check them against numpy without a GPU.  Not a product path: nothing in trre_amd/ links this file.
// With -DSPLIT_SHIM_MAIN the file is a program of its own that drives the same entry point over generated shapes, for a build
// with -fsanitize=address,undefined (a process of its own: a sanitized build is never loaded into an interpreter).
//
// pos0 (a multiple of the tile), ra0, rl0 and rk0 place the framed text as if pos0 framed bytes holding ra0 A, ra0 B, rl0 newlines
// and rk0 kept bytes came before it: the tiles that run are those from pos0 / TILE on, and every position and rank carries the
// shift — the arithmetic beyond 2^32.  Only the bytes and words of the text itself exist; the pointers are shifted to match.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "column_shim.hpp"

using namespace trre;

namespace {

// k_span_count, k_chunk_scan (three times), k_split_count, k_chunk_scan, k_split_emit
template <class G>
int run(const uint8_t* framed, int64_t m, const uint8_t* in, int64_t n, int64_t found, int64_t lines, int64_t kept, int lists_only, int64_t pos0,
        int64_t ra0, int64_t rl0, int64_t rk0, uint8_t* out, int64_t* piece_off, int64_t* list_off, int64_t* totals, int64_t* stores) {
    if (pos0 % G::TILE) return 6;
    const int64_t in0 = pos0 - 2 * ra0 - rl0;      // source bytes before the text
    if (in0 < 0) return 6;
    // the framed text at a 16-byte aligned address with whole vectors behind its end, as the library's buffer is
    std::vector<uint8_t> buf((size_t)m + 64 + 16, 0xEE);
    uint8_t* v0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 15) & ~(uintptr_t)15);
    if (m) std::memcpy(v0, framed, (size_t)m);
    const int64_t b0 = pos0 / G::TILE, tiles = (m + G::TILE - 1) / G::TILE, pieces = found + lines;
    std::vector<uint64_t> cnt((size_t)(3 * tiles) + 1, 0), base((size_t)(3 * (tiles + 1)), 0), kcnt((size_t)tiles + 1, 0), kbase((size_t)tiles + 1, 0);
    Padded<uint8_t> wo(kept, kUnstoredByte);
    Padded<int64_t> wp(pieces + 1, kUnstored), wl(lines + 1, kUnstored);
    SpanArgs sp{};
    sp.src = shifted(v0, pos0); sp.total = pos0 + m; sp.tiles = tiles;
    sp.cnt = shifted(cnt.data(), b0);
    SplitArgs a{};
    a.src = sp.src; a.total = sp.total; a.tiles = tiles;
    a.in = shifted(in, in0); a.n = in0 + n;
    a.base = shifted(static_cast<const uint64_t*>(base.data()), b0);
    a.kcnt = shifted(kcnt.data(), b0); a.kbase = shifted(static_cast<const uint64_t*>(kbase.data()), b0);
    a.list_off = shifted(wl.data(), rl0); a.nrec = rl0 + lines; a.lists_only = (uint32_t)lists_only;
    if (!lists_only) {
        a.out = shifted(wo.data(), rk0); a.out_len = rk0 + kept;
        a.piece_off = shifted(wp.data(), ra0 + rl0); a.n_piece = ra0 + rl0 + pieces;
    }
    // k_span_count: the threads' counts, summed per tile
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
        uint64_t run = (uint64_t)rank0[x];
        for (int64_t k = 0; k < tiles; ++k) { base[(size_t)(x * (tiles + 1) + k)] = run; run += cnt[(size_t)(x * tiles + k)]; }
        base[(size_t)(x * (tiles + 1) + tiles)] = run;
        totals[x] = (int64_t)run - rank0[x];
    }
    if (totals[0] != found || totals[1] != found || totals[2] != lines) return 4;
    // k_split_count
    std::vector<uint16_t> bits((size_t)3 * G::NVEC), kbits(G::NVEC);
    std::vector<uint32_t> pv_ab(G::NVEC), pv_nl(G::NVEC), pv_k(G::NVEC), pre_ab(G::THREADS), pre_nl(G::THREADS), pre_k(G::THREADS);
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        std::fill(bits.begin(), bits.end(), (uint16_t)0xA5A5);                          // (what a tile before left there)
        for (int tid = 0; tid < G::THREADS; ++tid) split_mark_vecs<G>(a, b, tid, bits.data());
        uint32_t run_ab = 0;                                                            // (barrier; the workgroup's scan)
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint32_t ab, nl;
            span_seg_count<G>(bits.data(), tid, ab, nl);
            pre_ab[tid] = run_ab; run_ab += ab;
        }
        uint64_t t = 0;
        for (int tid = 0; tid < G::THREADS; ++tid) t += split_seg_kept<G>(a, b, tid, bits.data(), pre_ab[tid], nullptr);
        a.kcnt[b] = t;
    }
    // k_chunk_scan
    {
        uint64_t run = (uint64_t)rk0;
        for (int64_t k = 0; k < tiles; ++k) { kbase[(size_t)k] = run; run += kcnt[(size_t)k]; }
        kbase[(size_t)tiles] = run;
        totals[3] = (int64_t)run - rk0;
    }
    if (totals[3] != kept) return 4;
    // k_split_emit
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        std::fill(bits.begin(), bits.end(), (uint16_t)0xA5A5);
        std::fill(kbits.begin(), kbits.end(), (uint16_t)0xA5A5);
        std::fill(pv_ab.begin(), pv_ab.end(), 0xDEADBEEFu);
        std::fill(pv_nl.begin(), pv_nl.end(), 0xDEADBEEFu);
        std::fill(pv_k.begin(), pv_k.end(), 0xDEADBEEFu);
        for (int tid = 0; tid < G::THREADS; ++tid) split_mark_vecs<G>(a, b, tid, bits.data());
        uint32_t run_ab = 0, run_nl = 0, run_k = 0;                                     // (barrier; the workgroup's scans)
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint32_t ab, nl;
            span_seg_count<G>(bits.data(), tid, ab, nl);
            pre_ab[tid] = run_ab; pre_nl[tid] = run_nl;
            run_ab += ab; run_nl += nl;
        }
        for (int tid = 0; tid < G::THREADS; ++tid) span_fill_pv<G>(bits.data(), pre_ab[tid], pre_nl[tid], tid, pv_ab.data(), pv_nl.data());
        for (int tid = 0; tid < G::THREADS; ++tid) {
            pre_k[tid] = run_k;
            run_k += split_seg_kept<G>(a, b, tid, bits.data(), pre_ab[tid], kbits.data());
        }
        if (run_k != kcnt[(size_t)(b - b0)]) return 5;
        for (int tid = 0; tid < G::THREADS; ++tid) split_fill_pv<G>(kbits.data(), pre_k[tid], tid, pv_k.data());
        // (barrier) the bytes and words: wave by wave, the lanes of a wave in turn; each may be stored once
        const std::vector<uint8_t> bo(wo.w);
        const std::vector<int64_t> bp(wp.w), bl(wl.w);
        for (int tid = 0; tid < G::THREADS; ++tid)
            split_emit_pieces<G>(a, b, tid, bits.data(), kbits.data(), pv_ab.data(), pv_nl.data(), pv_k.data());
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

}  // namespace

extern "C" {

int64_t shim_split_tile(int geo) { return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE; }

// framed: m bytes holding `found` A (0x01), `found` B (0x02), `lines` newlines and n position bytes, of which `kept` lie outside
// every A..B; in: the n source bytes, one per position byte, none of them 0xEE.  Out: out[0 .. kept), piece_off[0 .. found +
// lines], list_off[0 .. lines] as the kernel leaves them (a byte or word nobody stored reads 0xEE: entry 0 of both arrays when
// pos0 is not 0; all of out and piece_off with lists_only); totals[4]: what the count passes and the scans found; stores[3]:
// bytes of out, words of piece_off, words of list_off stored.
// 4: framed does not hold those counts, 5: the two kernels disagree on a tile, 7: a byte or word was stored twice, 8: one
// outside the arrays was written
int shim_split(int geo, const uint8_t* framed, int64_t m, const uint8_t* in, int64_t n, int64_t found, int64_t lines, int64_t kept, int lists_only,
               int64_t pos0, int64_t ra0, int64_t rl0, int64_t rk0, uint8_t* out, int64_t* piece_off, int64_t* list_off, int64_t* totals,
               int64_t* stores) {
    stores[0] = stores[1] = stores[2] = 0;
    switch (geo) {
    case 0: return run<Geo0>(framed, m, in, n, found, lines, kept, lists_only, pos0, ra0, rl0, rk0, out, piece_off, list_off, totals, stores);
    case 1: return run<Geo1>(framed, m, in, n, found, lines, kept, lists_only, pos0, ra0, rl0, rk0, out, piece_off, list_off, totals, stores);
    case 2: return run<Geo2>(framed, m, in, n, found, lines, kept, lists_only, pos0, ra0, rl0, rk0, out, piece_off, list_off, totals, stores);
    default: return run<Geo3>(framed, m, in, n, found, lines, kept, lists_only, pos0, ra0, rl0, rk0, out, piece_off, list_off, totals, stores);
    }
}

}  // extern "C"

#ifdef SPLIT_SHIM_MAIN
// The entry point over generated shapes, checked against a plain restatement: framed lengths around the tile edges; no marker
// (everything kept), one match over whole tiles (tiles and pieces with no marker, nothing kept), every byte a marker ("AB\n"
// repeated, "ABAB.."), A on the last byte of a piece or tile with its B on the first of the next, newlines at the first and last
// byte of tiles, random texts; the lists-only flag; a shift beyond 2^32.
namespace {

uint32_t rng_state = 24680;
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
        case 6: c = (uint8_t)(m >= 8 && x == 2 ? 1 : m >= 8 && x == m - 3 ? 2 : x == m - 1 ? '\n' : '.'); break;     // one match over whole tiles
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

int check(int geo, int64_t m, int pattern, int lists_only, int64_t pos0, int64_t ra0, int64_t rl0, int64_t rk0) {
    const int64_t T = shim_split_tile(geo);
    const std::vector<uint8_t> f = text(pattern, m, T);
    std::vector<uint8_t> in, wo;
    std::vector<int64_t> wp{rk0}, wl{0};
    int64_t na = ra0, nb = ra0, nl = rl0;
    for (int64_t x = 0; x < m; ++x) {
        const uint8_t c = f[(size_t)x];
        if (c == 1) ++na;
        else if (c == 2) { ++nb; wp.push_back(rk0 + (int64_t)wo.size()); }
        else if (c == '\n') { ++nl; wp.push_back(rk0 + (int64_t)wo.size()); wl.push_back(na + nl); }
        else {
            in.push_back((uint8_t)('a' + rnd() % 26));
            if (na == nb) wo.push_back(in.back());
        }
    }
    if (na != nb) return 20;
    const int64_t found = na - ra0, lines = nl - rl0, kept = (int64_t)wo.size(), n = (int64_t)in.size();
    std::vector<uint8_t> go((size_t)kept + 1, 0x11);
    std::vector<int64_t> gp((size_t)(found + lines) + 2, -1), gl((size_t)lines + 2, -1);
    int64_t totals[4], stores[3];
    const int rc = shim_split(geo, f.data(), m, in.data(), n, found, lines, kept, lists_only, pos0, ra0, rl0, rk0, go.data(), gp.data(), gl.data(), totals, stores);
    if (rc) return rc;
    const bool tile0 = m && !pos0;
    for (int64_t k = 0; k < kept; ++k)
        if (go[(size_t)k] != (lists_only ? kUnstoredByte : wo[(size_t)k])) return 11;
    for (int64_t k = 1; k <= found + lines; ++k)
        if (gp[(size_t)k] != (lists_only ? kUnstored : wp[(size_t)k])) return 12;
    for (int64_t i = 1; i <= lines; ++i)
        if (gl[(size_t)i] != wl[(size_t)i]) return 13;
    if (gl[0] != (tile0 ? 0 : kUnstored) || gp[0] != (tile0 && !lists_only ? 0 : kUnstored)) return 14;
    if (go[(size_t)kept] != 0x11 || gp[(size_t)(found + lines) + 1] != -1 || gl[(size_t)lines + 1] != -1) return 16;
    if (stores[0] != (lists_only ? 0 : kept) || stores[1] != (lists_only ? 0 : found + lines + (tile0 ? 1 : 0)) || stores[2] != lines + (tile0 ? 1 : 0)) return 15;
    return 0;
}

}  // namespace

int main() {
    int runs = 0;
    for (int geo = 0; geo < 4; ++geo) {
        const int64_t T = shim_split_tile(geo);
        const int64_t sizes[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T, 2 * T + 77};
        for (int64_t m : sizes)
            for (int pattern = 0; pattern < 8; ++pattern)
                for (int lists_only = 0; lists_only < 2; ++lists_only) {
                    const bool far = (runs % 3) == 2;
                    const int rc = check(geo, m, pattern, lists_only, far ? ((5ll << 32) / T + 3) * T : 0, far ? (1ll << 32) + 5 : 0, far ? (1ll << 33) + 7 : 0,
                                         far ? (1ll << 34) + 11 : 0);
                    if (rc) { std::printf("FAILED: geo %d m %lld pattern %d lists_only %d far %d: %d\n", geo, (long long)m, pattern, lists_only, (int)far, rc); return 1; }
                    ++runs;
                }
    }
    std::printf("split_shim: %d shapes ok\n", runs);
    return 0;
}
#endif
