// match_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of the matched-strings passes
// (trre_amd/csrc/records_block.hpp: k_match_verdict, k_match_rank, k_match_final, k_match_count, k_match_unframe) on the host,
// thread by thread, a wave as 64 sequential lanes and its ballot as a loop, barriers as loop boundaries, so that
// tests/test_match_shim.py can check them against numpy without a GPU.  Not a product path: nothing in trre_amd/ links this
// file.  With -DMATCH_SHIM_MAIN the file is a program of its own that drives the same entry points over generated shapes:
// tests/test_match_shim.py builds that program with -fsanitize=address,undefined and runs it (a process of its own: a
// sanitized build is never loaded into an interpreter).
//
// base0 is added to every group base, as if base0 accepted strings came before the column: the rank arithmetic beyond 2^32.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../trre_amd/csrc/records_block.hpp"

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

// the accept table as the runtime uploads it: a bit per backward state
std::vector<uint32_t> accept_bits(const uint8_t* accept, uint32_t n_rev) {
    std::vector<uint32_t> bits((n_rev + 31) / 32, 0u);
    for (uint32_t y = 0; y < n_rev; ++y)
        if (accept[y]) bits[y >> 5] |= 1u << (y & 31);
    return bits;
}

// k_match_verdict over every group, k_chunk_scan, k_match_rank
template <int kBits>
int verdict(const uint8_t* sym, int64_t vbeg, const int64_t* off, int64_t nrec, const uint8_t* accept, uint32_t n_rev, uint64_t base0,
            uint64_t* valid_out, int64_t* out_off, int64_t* local, uint64_t* cnt_out, uint64_t* base_out) {
    const std::vector<uint32_t> acc = accept_bits(accept, n_rev);
    const int64_t words = (nrec + 63) / 64, groups = (nrec + kMatchThreads - 1) / kMatchThreads;
    Aligned valid(nullptr, 8 * words, 0);
    std::vector<uint64_t> cnt((size_t)groups + 1), base((size_t)groups + 1);
    MatchArgs a{};
    a.sym_v0 = sym; a.vbeg = vbeg; a.off = off; a.nrec = nrec;
    a.accept = acc.data(); a.accept_words = (uint32_t)acc.size();
    a.valid = reinterpret_cast<uint64_t*>(valid.v0); a.words = words;
    a.out_off = out_off; a.cnt = cnt.data(); a.base = base.data();
    constexpr int kWaves = kMatchThreads / 64;
    for (int64_t g = 0; g < groups; ++g) {
        uint64_t word[kWaves];
        uint32_t wtot[kWaves];
        for (int w = 0; w < kWaves; ++w) {
            word[w] = 0;
            for (int lane = 0; lane < 64; ++lane) {                    // the ballot
                const int64_t i = g * kMatchThreads + w * 64 + lane;
                if (i < nrec && match_verdict<kBits>(a, acc.data(), i)) word[w] |= 1ull << lane;
            }
            const int64_t at = g * kWaves + w;
            if (at < a.words) a.valid[at] = word[w];
            wtot[w] = match_popc64(word[w]);
        }
        uint32_t total = 0;
        for (int w = 0; w < kWaves; ++w) {
            for (int lane = 0; lane < 64; ++lane) match_park(a, g * kMatchThreads + w * 64 + lane, total, word[w], lane);
            total += wtot[w];
        }
        cnt[g] = total;
    }
    for (int64_t i = 0; i < nrec; ++i) local[i] = out_off[i + 1];
    uint64_t run = base0;
    for (int64_t g = 0; g < groups; ++g) { base[g] = run; run += cnt[g]; }
    base[groups] = run;
    for (int64_t i = 0; i < nrec; ++i) match_add_base(a, i);
    if (words) std::memcpy(valid_out, valid.v0, (size_t)(8 * words));
    for (int64_t g = 0; g < groups; ++g) cnt_out[g] = cnt[g];
    for (int64_t g = 0; g <= groups; ++g) base_out[g] = base[g];
    return valid.untouched_outside(0, 8 * words) ? 0 : 2;
}

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

// k_match_count, k_chunk_scan, k_match_unframe: the framed output without its newlines at misalignment dst_mis
template <class G>
int unframe(const uint8_t* framed, int64_t m, int64_t matched, int64_t dst_mis, uint8_t* out) {
    Aligned src(framed, m, 0), dst(nullptr, m - matched, dst_mis);
    const int64_t tiles = (m + G::TILE - 1) / G::TILE;
    std::vector<uint64_t> cnt((size_t)tiles + 1), base((size_t)tiles + 1);
    RecArgs ca{};
    ca.in_v0 = src.v0; ca.vbeg = 0; ca.vend = m; ca.cnt = cnt.data(); ca.base = base.data();
    for (int64_t b = 0; b < tiles; ++b) {
        uint64_t c = 0;
        for (int k = 0; k < G::THREADS; ++k) c += rec_count_vecs<G>(ca, b, k, nullptr);
        cnt[b] = c;
    }
    uint64_t run = 0;
    for (int64_t b = 0; b < tiles; ++b) { base[b] = run; run += cnt[b]; }
    base[tiles] = run;
    if ((int64_t)run != matched) return 4;                                             // the framed newlines are the accepted strings
    StrArgs a{};
    a.src_v0 = src.v0; a.total = m; a.dst = dst.v0 + dst_mis; a.dst_len = m - matched;
    a.part = reinterpret_cast<const int64_t*>(base.data());
    Lds<G> l;
    for (int64_t b = 0; b < tiles; ++b) {
        const StrTile<G> t(a, b, false);
        for (int k = 0; k < G::THREADS; ++k) str_load_vecs<G>(a, t, k, l.regs(k));
        std::fill(l.bits32.begin(), l.bits32.end(), 0xA5A5A5A5u);                     // (what a tile before left there)
        std::memset(l.bytes.data(), 0x5A, l.bytes.size() * sizeof(U128));
        for (int k = 0; k < G::THREADS; ++k) { match_mark_vecs<G>(t, k, l.regs(k), l.bits16()); str_keep_vecs<G>(t, k, l.regs(k), l.bytes.data()); }
        const uint32_t marks = l.scan();
        if (marks != cnt[b]) return 5;
        for (int k = 0; k < G::THREADS; ++k) str_fill_pv<G>(l.bits16(), l.pre[k], k, l.pv.data());
        const StrOut<G> o(a, t, marks);
        std::fill(l.inv.begin(), l.inv.end(), (uint16_t)0xFFFF);
        for (int k = 0; k < G::THREADS; ++k) str_fill_inv<G>(t, o, k, l.bits16(), l.pv.data(), l.inv.data());
        for (int g = 0; g < o.ng; ++g) if (l.inv[g] == 0xFFFF) return 3;               // a destination vector without a source
        for (int k = 0; k < G::THREADS; ++k) str_unframe_vecs<G>(a, t, o, k, l.bytes.data(), l.bits16(), l.pv.data(), l.inv.data());
    }
    if (m - matched) std::memcpy(out, dst.v0 + dst_mis, (size_t)(m - matched));
    return dst.untouched_outside(dst_mis, dst_mis + m - matched) ? 0 : 2;
}

using Geo0 = RecGeo<4, 1>;     // 64-byte tiles
using Geo1 = RecGeo<4, 2>;     // 128
using Geo2 = RecGeo<64, 1>;    // 1 KiB
using Geo3 = StrGeoDev;        // the device's

}  // namespace

extern "C" {

int64_t shim_match_group() { return kMatchThreads; }
int64_t shim_match_tile(int geo) { return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE; }

// sym: the symbols of the staged text in the layout `bits` names (4: two per byte, low nibble first; 8; 16), indexed from vbeg;
// accept: a byte per backward state.  Out: the bitmap (ceil(nrec / 64) words), M_i + base0 in out_off[1 .. nrec], the ranks
// inside the groups, the groups' counts and bases (groups + 1); 2: a byte outside the bitmap's words was written
int shim_match_verdict(int bits, const uint8_t* sym, int64_t vbeg, const int64_t* off, int64_t nrec, const uint8_t* accept, uint32_t n_rev,
                       uint64_t base0, uint64_t* valid, int64_t* out_off, int64_t* local, uint64_t* cnt, uint64_t* base) {
    switch (bits) {
    case 4: return verdict<4>(sym, vbeg, off, nrec, accept, n_rev, base0, valid, out_off, local, cnt, base);
    case 16: return verdict<16>(sym, vbeg, off, nrec, accept, n_rev, base0, valid, out_off, local, cnt, base);
    default: return verdict<8>(sym, vbeg, off, nrec, accept, n_rev, base0, valid, out_off, local, cnt, base);
    }
}

// out_off[1 .. nrec]: located positions in, output offsets out (k_match_final)
int shim_match_final(const uint64_t* valid, const uint64_t* base, int64_t* out_off, int64_t nrec) {
    MatchArgs a{};
    a.valid = const_cast<uint64_t*>(valid); a.words = (nrec + 63) / 64; a.base = base; a.out_off = out_off; a.nrec = nrec;
    for (int64_t i = 0; i < nrec; ++i) match_final(a, i);
    return 0;
}

// out: the m - matched bytes of framed that are not '\n', written at misalignment dst_mis; 2: a byte outside them was written,
// 4: framed does not hold `matched` newlines
int shim_match_unframe(int geo, const uint8_t* framed, int64_t m, int64_t matched, int64_t dst_mis, uint8_t* out) {
    switch (geo) {
    case 0: return unframe<Geo0>(framed, m, matched, dst_mis, out);
    case 1: return unframe<Geo1>(framed, m, matched, dst_mis, out);
    case 2: return unframe<Geo2>(framed, m, matched, dst_mis, out);
    default: return unframe<Geo3>(framed, m, matched, dst_mis, out);
    }
}

}  // extern "C"

#ifdef MATCH_SHIM_MAIN
// The entry points over generated shapes, checked against a plain restatement: nrec around the word and group edges, verdict
// patterns (all, none, alternating, first, last, runs), the three symbol layouts, every destination misalignment.
namespace {

uint32_t rng_state = 12345;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int check_verdicts(int bits, int64_t nrec, int pattern, int64_t vbeg) {
    const uint32_t n_rev = bits == 4 ? 16 : bits == 8 ? 200 : 700;
    std::vector<uint8_t> accept(n_rev);
    for (uint32_t y = 0; y < n_rev; ++y) accept[y] = (y % 3) == 1;
    std::vector<int64_t> off((size_t)nrec + 1, 0);
    for (int64_t i = 0; i < nrec; ++i) off[i + 1] = off[i] + (int64_t)(rnd() % 4);
    const int64_t total = off[nrec] + nrec;
    std::vector<uint32_t> syms((size_t)(vbeg + total) + 2, 0);
    std::vector<uint8_t> want((size_t)nrec);
    for (int64_t i = 0; i < nrec; ++i) {
        bool ok = pattern == 0 ? true : pattern == 1 ? false : pattern == 2 ? (i & 1) != 0 : pattern == 3 ? i == 0 : pattern == 4 ? i == nrec - 1
                  : pattern == 5 ? (i / 65) % 2 == 0 : (rnd() & 1) != 0;
        want[i] = ok;
        uint32_t y;
        do y = rnd() % n_rev; while ((accept[y] != 0) != ok);
        syms[(size_t)(vbeg + off[i] + i)] = y;
    }
    std::vector<uint8_t> sym;
    if (bits == 4) { sym.assign(syms.size() / 2 + 1, 0); for (size_t v = 0; v < syms.size(); ++v) sym[v >> 1] |= (uint8_t)(syms[v] << (4 * (v & 1))); }
    else if (bits == 8) { sym.resize(syms.size()); for (size_t v = 0; v < syms.size(); ++v) sym[v] = (uint8_t)syms[v]; }
    else { sym.resize(2 * syms.size()); for (size_t v = 0; v < syms.size(); ++v) { sym[2 * v] = (uint8_t)syms[v]; sym[2 * v + 1] = (uint8_t)(syms[v] >> 8); } }
    const int64_t words = (nrec + 63) / 64, groups = (nrec + kMatchThreads - 1) / kMatchThreads;
    std::vector<uint64_t> valid((size_t)words + 1, 0), cnt((size_t)groups + 1), base((size_t)groups + 1);
    std::vector<int64_t> out_off((size_t)nrec + 1, -1), local((size_t)nrec + 1);
    const uint64_t base0 = (7ull << 32) + 5;
    if (shim_match_verdict(bits, sym.data(), vbeg, off.data(), nrec, accept.data(), n_rev, base0, valid.data(), out_off.data(), local.data(), cnt.data(),
                           base.data()))
        return 1;
    uint64_t run = base0;
    for (int64_t i = 0; i < nrec; ++i) {
        run += want[i];
        if (((valid[(size_t)(i >> 6)] >> (i & 63)) & 1) != want[i] || (uint64_t)out_off[(size_t)i + 1] != run) return 2;
    }
    if (words && nrec % 64 && (valid[(size_t)words - 1] >> (nrec % 64)) != 0) return 3;
    if (base[(size_t)groups] != run) return 4;
    // the final offsets from located positions of a made-up framed output: every accepted string prints i % 3 bytes and its '\n'
    std::vector<int64_t> located((size_t)nrec + 1, 0), final_want((size_t)nrec + 1, 0);
    int64_t pos = 0, kept = 0;
    std::vector<uint8_t> framed;
    for (int64_t i = 0; i < nrec; ++i) {
        if (want[i]) {
            for (int64_t k = 0; k < i % 3; ++k) framed.push_back((uint8_t)('a' + k));
            framed.push_back('\n');
            pos += i % 3 + 1; kept += i % 3;
        }
        located[(size_t)i + 1] = pos; final_want[(size_t)i + 1] = kept;
    }
    // (base0 shifts every rank: the located positions carry it too here, so that the subtraction is the runtime's)
    for (int64_t i = 0; i < nrec; ++i) located[(size_t)i + 1] += (int64_t)base0;
    shim_match_final(valid.data(), base.data(), located.data(), nrec);
    for (int64_t i = 0; i < nrec; ++i)
        if (located[(size_t)i + 1] != final_want[(size_t)i + 1]) return 5;
    const int64_t m = (int64_t)framed.size(), matched = m - kept;
    for (int geo = 0; geo < 4; ++geo) {
        if (geo == 3 && nrec > 600) continue;
        for (int64_t mis = 0; mis < 16; mis += (geo == 0 ? 1 : 5)) {
            std::vector<uint8_t> out((size_t)kept + 1, 0);
            if (shim_match_unframe(geo, framed.data(), m, matched, mis, out.data())) return 6;
            int64_t at = 0;
            for (int64_t x = 0; x < m; ++x)
                if (framed[(size_t)x] != '\n' && out[(size_t)at++] != framed[(size_t)x]) return 7;
        }
    }
    return 0;
}

}  // namespace

int main() {
    const int64_t T = kMatchThreads;
    const int64_t sizes[] = {0, 1, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 3 * T + 5};
    int runs = 0;
    for (int bits : {4, 8, 16})
        for (int64_t nrec : sizes)
            for (int pattern = 0; pattern < 7; ++pattern)
                for (int64_t vbeg : {(int64_t)0, (int64_t)3}) {
                    const int rc = check_verdicts(bits, nrec, pattern, vbeg);
                    if (rc) { std::printf("FAILED: bits %d nrec %lld pattern %d vbeg %lld: %d\n", bits, (long long)nrec, pattern, (long long)vbeg, rc); return 1; }
                    ++runs;
                }
    std::printf("match_shim: %d shapes ok\n", runs);
    return 0;
}
#endif
