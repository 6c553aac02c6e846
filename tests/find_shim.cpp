// find_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of k_find_unframe (trre_amd/csrc/records_block.hpp: the
// compaction of k_match_unframe and find_offset_vecs, behind k_match_count and k_chunk_scan) on the host, thread by thread, a
// wave as 64 sequential lanes, barriers as loop boundaries, so that tests/test_find_shim.py can check them against numpy without
// a GPU.  Not a product path: nothing in trre_amd/ links this file.  With -DFIND_SHIM_MAIN the file is a program of its own that
// drives the same entry point over generated shapes: tests/test_find_shim.py builds that program with
// -fsanitize=address,undefined and runs it (a process of its own: a sanitized build is never loaded into an interpreter).
//
// pos0 (a multiple of the tile) and rank0 place the framed text as if pos0 framed bytes holding rank0 newlines came before it:
// the tiles that run are those from pos0 / TILE on, and every position, rank and destination carries the shift — the
// arithmetic beyond 2^32.  Only the bytes and words of the text itself exist; the pointers are shifted to match.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "column_shim.hpp"

using namespace trre;

namespace {

constexpr uint8_t kFill = 0xEE;

// n bytes at offset mis of a 16-byte aligned address, 64 sentinel bytes on either side
struct Aligned {
    std::vector<uint8_t> buf;
    uint8_t* v0;
    Aligned(const uint8_t* src, int64_t n, int64_t mis) : buf((size_t)(mis + n + 160), kFill) {
        v0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 64 + 15) & ~(uintptr_t)15);
        if (n && src) std::memcpy(v0 + mis, src, (size_t)n);
    }
    bool untouched_outside(int64_t from, int64_t to) const {
        for (const uint8_t* p = buf.data(); p < buf.data() + buf.size(); ++p)
            if ((p < v0 + from || p >= v0 + to) && *p != kFill) return false;
        return true;
    }
};

template <class G>
struct Lds {
    std::vector<U128> bytes;
    std::vector<uint32_t> bits32, pv, pre;
    std::vector<uint16_t> inv;
    std::vector<U128> w;
    Lds() : bytes(G::NVEC + 2), bits32(G::NVEC / 2 + 1), pv(G::NVEC + 1), pre(G::THREADS), inv(G::NVEC + 2), w((size_t)G::THREADS * (G::VECS + 1)) {}
    uint16_t* bits16() { return reinterpret_cast<uint16_t*>(bits32.data()); }
    U128 (&regs(int t))[G::VECS + 1] { return *reinterpret_cast<U128(*)[G::VECS + 1]>(&w[(size_t)t * (G::VECS + 1)]); }
    uint32_t scan() {
        uint32_t run = 0;
        for (int t = 0; t < G::THREADS; ++t) { pre[t] = run; run += rec_seg_count<G>(bits16(), t); }
        return run;
    }
};

// k_match_count, k_chunk_scan, k_find_unframe
template <class G>
int unframe(const uint8_t* framed, int64_t m, int64_t found, int64_t dst_mis, int64_t pos0, int64_t rank0, uint8_t* out, int64_t* match_off,
            int64_t* stores) {
    if (pos0 % G::TILE) return 6;
    Aligned src(framed, m, 0), dst(nullptr, m - found, dst_mis);
    const int64_t b0 = pos0 / G::TILE, tiles = (m + G::TILE - 1) / G::TILE;
    std::vector<uint64_t> cnt((size_t)tiles + 1), base((size_t)tiles + 1);
    RecArgs ca{};
    ca.in_v0 = shifted(src.v0, pos0); ca.vbeg = 0; ca.vend = pos0 + m;
    for (int64_t b = 0; b < tiles; ++b) {
        uint64_t c = 0;
        for (int k = 0; k < G::THREADS; ++k) c += rec_count_vecs<G>(ca, b0 + b, k, nullptr);
        cnt[b] = c;
    }
    uint64_t run = (uint64_t)rank0;
    for (int64_t b = 0; b < tiles; ++b) { base[b] = run; run += cnt[b]; }
    base[tiles] = run;
    if ((int64_t)run != rank0 + found) return 4;                                       // the framed newlines are the matches
    // the offsets as words with sentinels around them, every store counted
    std::vector<int64_t> words((size_t)found + 1 + 16, (int64_t)0xEEEEEEEEEEEEEEEEull);
    StrArgs a{};
    a.src_v0 = shifted(src.v0, pos0); a.total = pos0 + m;
    a.dst = shifted(dst.v0 + dst_mis, pos0 - rank0); a.dst_len = pos0 - rank0 + m - found;
    a.part = shifted(reinterpret_cast<const int64_t*>(base.data()), b0);
    a.nrec = rank0 + found; a.out_off = shifted(words.data() + 8, rank0);
    Lds<G> l;
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        const StrTile<G> t(a, b, false);
        for (int k = 0; k < G::THREADS; ++k) str_load_vecs<G>(a, t, k, l.regs(k));
        std::fill(l.bits32.begin(), l.bits32.end(), 0xA5A5A5A5u);                     // (what a tile before left there)
        std::memset(l.bytes.data(), 0x5A, l.bytes.size() * sizeof(U128));
        for (int k = 0; k < G::THREADS; ++k) { match_mark_vecs<G>(t, k, l.regs(k), l.bits16()); str_keep_vecs<G>(t, k, l.regs(k), l.bytes.data()); }
        const uint32_t marks = l.scan();
        if (marks != cnt[b - b0]) return 5;
        for (int k = 0; k < G::THREADS; ++k) str_fill_pv<G>(l.bits16(), l.pre[k], k, l.pv.data());
        // the offsets: wave by wave, the lanes of a wave in turn; a word may be stored once
        const std::vector<int64_t> before(words);
        for (int k = 0; k < G::THREADS; ++k) find_offset_vecs<G>(a, t, k, l.bits16(), l.pv.data());
        for (size_t x = 0; x < words.size(); ++x)
            if (words[x] != before[x]) {
                if (before[x] != (int64_t)0xEEEEEEEEEEEEEEEEull) return 7;             // a word stored by two tiles
                *stores += 1;
            }
        const StrOut<G> o(a, t, marks);
        std::fill(l.inv.begin(), l.inv.end(), (uint16_t)0xFFFF);
        for (int k = 0; k < G::THREADS; ++k) str_fill_inv<G>(t, o, k, l.bits16(), l.pv.data(), l.inv.data());
        for (int g = 0; g < o.ng; ++g) if (l.inv[g] == 0xFFFF) return 3;               // a destination vector without a source
        for (int k = 0; k < G::THREADS; ++k) str_unframe_vecs<G>(a, t, o, k, l.bytes.data(), l.bits16(), l.pv.data(), l.inv.data());
    }
    if (m - found) std::memcpy(out, dst.v0 + dst_mis, (size_t)(m - found));
    std::memcpy(match_off, words.data() + 8, (size_t)(found + 1) * 8);
    for (int k = 0; k < 8; ++k)
        if (words[k] != (int64_t)0xEEEEEEEEEEEEEEEEull || words[(size_t)found + 9 + k] != (int64_t)0xEEEEEEEEEEEEEEEEull) return 8;
    return dst.untouched_outside(dst_mis, dst_mis + m - found) ? 0 : 2;
}

}  // namespace

extern "C" {

int64_t shim_find_tile(int geo) { return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE; }

// framed: m bytes holding `found` newlines.  Out: the m - found other bytes, written at misalignment dst_mis; match_off[0 ..
// found] as the kernel leaves it (an entry nobody stored reads 0xEE..EE: entry 0 when pos0 is not 0); *stores: words stored.
// 2: a byte outside the output was written, 4: framed does not hold `found` newlines, 7: a word was stored twice, 8: a word
// outside match_off[0 .. found] was written
int shim_find_unframe(int geo, const uint8_t* framed, int64_t m, int64_t found, int64_t dst_mis, int64_t pos0, int64_t rank0, uint8_t* out,
                      int64_t* match_off, int64_t* stores) {
    *stores = 0;
    switch (geo) {
    case 0: return unframe<Geo0>(framed, m, found, dst_mis, pos0, rank0, out, match_off, stores);
    case 1: return unframe<Geo1>(framed, m, found, dst_mis, pos0, rank0, out, match_off, stores);
    case 2: return unframe<Geo2>(framed, m, found, dst_mis, pos0, rank0, out, match_off, stores);
    default: return unframe<Geo3>(framed, m, found, dst_mis, pos0, rank0, out, match_off, stores);
    }
}

}  // extern "C"

#ifdef FIND_SHIM_MAIN
// The entry point over generated shapes, checked against a plain restatement: framed lengths around the tile edges, newline
// patterns (none, one, all, first and last byte of pieces and tiles, random), every destination misalignment, a shift beyond 2^32.
namespace {

uint32_t rng_state = 4321;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int check(int geo, int64_t m, int pattern, int64_t mis, int64_t pos0, int64_t rank0) {
    const int64_t T = shim_find_tile(geo);
    std::vector<uint8_t> framed((size_t)m);
    for (int64_t x = 0; x < m; ++x) {
        bool nl = pattern == 0 ? false : pattern == 1 ? x == m / 2 : pattern == 2 ? true : pattern == 3 ? (x % 64 == 0 || x % 64 == 63)
                  : pattern == 4 ? (x % T == 0 || x % T == T - 1) : pattern == 5 ? (x % 16 == 0 || x % 16 == 15) : rnd() % 3 == 0;
        framed[(size_t)x] = nl ? (uint8_t)'\n' : (uint8_t)('a' + rnd() % 26);
    }
    std::vector<int64_t> want{0};
    std::vector<uint8_t> kept;
    for (int64_t x = 0; x < m; ++x) {
        if (framed[(size_t)x] == '\n') want.push_back(pos0 + x - (rank0 + (int64_t)want.size() - 1));
        else kept.push_back(framed[(size_t)x]);
    }
    const int64_t found = (int64_t)want.size() - 1;
    std::vector<uint8_t> out(kept.size() + 1, 0);
    std::vector<int64_t> got((size_t)found + 1, -1);
    int64_t stores = 0;
    const int rc = shim_find_unframe(geo, framed.data(), m, found, mis, pos0, rank0, out.data(), got.data(), &stores);
    if (rc) return rc;
    if (!kept.empty() && std::memcmp(out.data(), kept.data(), kept.size())) return 10;
    for (int64_t j = 1; j <= found; ++j)
        if (got[(size_t)j] != want[(size_t)j]) return 11;
    if (m && got[0] != (pos0 ? (int64_t)0xEEEEEEEEEEEEEEEEull : 0)) return 12;
    if (stores != found + (m && !pos0 ? 1 : 0)) return 13;
    return 0;
}

}  // namespace

int main() {
    int runs = 0;
    for (int geo = 0; geo < 4; ++geo) {
        const int64_t T = shim_find_tile(geo);
        const int64_t sizes[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T, 2 * T + 77};
        for (int64_t m : sizes)
            for (int pattern = 0; pattern < 7; ++pattern)
                for (int64_t mis = 0; mis < 16; mis += (geo == 3 ? 5 : 3)) {
                    const bool far = (runs & 3) == 3;
                    const int rc = check(geo, m, pattern, mis, far ? ((5ll << 32) / T + 3) * T : 0, far ? (4ll << 32) + 7 : 0);
                    if (rc) { std::printf("FAILED: geo %d m %lld pattern %d mis %lld far %d: %d\n", geo, (long long)m, pattern, (long long)mis, (int)far, rc); return 1; }
                    ++runs;
                }
    }
    std::printf("find_shim: %d shapes ok\n", runs);
    return 0;
}
#endif
