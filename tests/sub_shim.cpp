// sub_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of k_sub_plan, k_sub_place, k_sub_offsets and k_sub_emit
// (trre_amd/csrc/records_block.hpp: sub_plan_thread, sub_place_sums, sub_place_thread, sub_offset, sub_emit_window,
// sub_keep_window, sub_emit_vecs, with k_chunk_scan between them) on the host, thread by thread, barriers as loop boundaries, so
// that tests/test_sub_shim.py can check them against numpy without a GPU.  Not a product path: nothing in trre_amd/ links this
// file.  With -DSUB_SHIM_MAIN the file is a program of its own that drives the same entry point over generated shapes, for a
// build with -fsanitize=address,undefined (a process of its own: a sanitized build is never loaded into an interpreter).
//
// src_mis, x_mis and dst_mis are the addresses of the input, of the texts and of the output mod 16.  The spans, the texts and the
// list offsets are the caller's: what k_span_emit and k_find_unframe leave in the library's arrays.  pos0, ra0 (a multiple of the
// chunk) and rk0 place the column as if pos0 input bytes, ra0 matches and rk0 output bytes came before it: the offsets and spans the
// caller passes start at pos0, the list offsets at ra0, the chunks that run are those from ra0 / chunk on, the tiles those from rk0
// on, and every position, rank and output offset carries the shift — the arithmetic beyond 2^32.  Only the bytes and words of the
// column itself exist; the pointers are shifted to match.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "column_shim.hpp"

using namespace trre;

namespace {

// a copy of n bytes at `mis` behind a 16-byte aligned address, whole vectors readable around it
struct Staged {
    std::vector<uint8_t> buf;
    uint8_t* p;
    Staged(const uint8_t* src, int64_t n, int mis) : buf((size_t)n + 64 + 16, 0xEE) {
        uint8_t* v0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 15) & ~(uintptr_t)15);
        p = v0 + 16 + mis;
        if (n) std::memcpy(p, src, (size_t)n);
    }
};

template <class G>
int run(const uint8_t* in, int64_t n, const int64_t* off, const int64_t* loff, int64_t nrec, const int64_t* start, const int64_t* end,
        const int64_t* xoff, const uint8_t* x, int64_t found, int64_t first, int64_t count, int src_mis, int x_mis, int dst_mis, int64_t pos0, int64_t ra0, int64_t rk0,
        int64_t n_sel, int64_t out_len, uint8_t* out, int64_t* out_off, int64_t* totals, int64_t* stores) {
    const int64_t per = (int64_t)G::THREADS * kSubPer, chunks = (found + per - 1) / per > 0 ? (found + per - 1) / per : 1, c0 = ra0 / per;
    if (ra0 % per || pos0 < 0 || rk0 < 0) return 6;
    if (src_mis < 0 || src_mis > 15 || dst_mis < 0 || dst_mis > 15 || x_mis < 0 || x_mis > 15 || nrec < 1 || found < 0) return 6;
    const Staged si(in, n, src_mis), sx(x, xoff[found], x_mis);
    const size_t slots = (size_t)found + 2;
    std::vector<int64_t> S(slots, kUnstored), E(slots, kUnstored), XO(slots, kUnstored), P(slots, kUnstored);
    for (int64_t j = 0; j < found; ++j) { S[(size_t)j + 1] = start[j]; E[(size_t)j + 1] = end[j]; }
    for (int64_t j = 0; j <= found; ++j) XO[(size_t)j + 1] = xoff[j];
    std::vector<uint64_t> cnt((size_t)(3 * chunks), 0), base((size_t)(3 * (chunks + 1)), 0);
    uint32_t status = 0;
    Padded<uint8_t> wo(out_len, kUnstoredByte, dst_mis);
    Padded<int64_t> wf(nrec + 1, kUnstored);
    SubArgs a{};
    a.in = shifted(static_cast<const uint8_t*>(si.p), pos0); a.n = pos0 + n; a.off = off; a.nrec = nrec; a.L = loff;
    a.S = shifted(S.data() + 1, ra0); a.E = shifted(E.data() + 1, ra0); a.XO = shifted(static_cast<const int64_t*>(XO.data() + 1), ra0);
    a.P = shifted(P.data() + 1, ra0); a.X = sx.p; a.x_len = xoff[found];
    a.found = ra0 + found; a.j0 = ra0; a.out0 = rk0; a.first = first; a.count = count; a.chunks = chunks; a.status = &status;
    // (the kernels index cnt[k * chunks + c] and base[k * (chunks + 1) + c] with the absolute c)
    a.cnt = shifted(cnt.data(), c0); a.base = shifted(static_cast<const uint64_t*>(base.data()), c0);
    // k_sub_plan
    for (int64_t c = c0; c < c0 + chunks; ++c) {
        uint64_t t[3] = {0, 0, 0};
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint64_t c3[3];
            status |= sub_plan_thread<G::THREADS>(a, c, tid, c3);
            for (int k = 0; k < 3; ++k) t[k] += c3[k];
        }
        for (int k = 0; k < 3; ++k) a.cnt[k * chunks + c] = t[k];
    }
    if (status) return 9;
    // k_chunk_scan, three times
    const int64_t seed[3] = {0, rk0, pos0};             // (growth = texts - matched: the places come out as S[j] - pos0 + rk0 + growth)
    for (int k = 0; k < 3; ++k) {
        uint64_t sum = (uint64_t)seed[k];
        for (int64_t c = 0; c < chunks; ++c) { base[(size_t)(k * (chunks + 1) + c)] = sum; sum += cnt[(size_t)(k * chunks + c)]; }
        base[(size_t)(k * (chunks + 1) + chunks)] = sum;
        totals[k] = (int64_t)sum - seed[k];
    }
    if (totals[0] != n_sel || n - totals[2] + totals[1] != out_len) return 4;
    a.out = shifted(wo.data(), rk0); a.out_len = rk0 + out_len; a.out_off = wf.data();
    // k_sub_place: the threads' sums, their exclusive scan over the workgroup (barrier), the places
    for (int64_t c = c0; c < c0 + chunks; ++c) {
        std::vector<uint64_t> pt(G::THREADS), pm(G::THREADS);
        uint64_t rt = 0, rm = 0, rs = 0;
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint64_t c3[3];
            sub_place_sums<G::THREADS>(a, c, tid, c3);
            pt[(size_t)tid] = rt; pm[(size_t)tid] = rm;
            rs += c3[0]; rt += c3[1]; rm += c3[2];
        }
        if (rs != a.cnt[c] || rt != a.cnt[chunks + c] || rm != a.cnt[2 * chunks + c]) return 5;
        for (int tid = 0; tid < G::THREADS; ++tid) sub_place_thread<G::THREADS>(a, c, tid, pt[(size_t)tid], pm[(size_t)tid]);
    }
    for (size_t k = 0; k < slots; ++k)
        if (P[k] == kUnstored || (k + 1 < slots && E[k] == kUnstored) || (k > 0 && S[k] == kUnstored)) return 10;
    // k_sub_offsets
    {
        const std::vector<int64_t> bf(wf.w);
        for (int64_t i = 0; i <= nrec; ++i) sub_offset(a, i);
        bool twice = false;
        stores[1] += changed(wf.w, bf, kUnstored, &twice);
    }
    // k_sub_emit
    const int64_t A = (int64_t)(reinterpret_cast<uintptr_t>(a.out) & 15u);
    const int64_t b0 = (rk0 + A) / G::TILE, b1 = out_len ? (rk0 + out_len + A + G::TILE - 1) / G::TILE : b0;
    std::vector<int64_t> image((size_t)kSubWindow);
    for (int64_t b = b0; b < b1; ++b) {
        const SubTile<G> t(a, b);
        int64_t win[2] = {-7, -7};
        std::fill(image.begin(), image.end(), (int64_t)0x5A5A5A5A5A5A5A5All);            // (what a tile before left there)
        sub_emit_window<G>(a, t, win);                                                   // (thread 0; barrier)
        for (int tid = 0; tid < G::THREADS; ++tid) sub_keep_window<G>(a, win, tid, image.data());
        const std::vector<uint8_t> bo(wo.w);                                             // (barrier)
        for (int tid = 0; tid < G::THREADS; ++tid) sub_emit_vecs<G>(a, t, b, tid, win, image.data());
        bool twice = false;
        stores[0] += changed(wo.w, bo, kUnstoredByte, &twice);
        if (twice) return 7;                                                             // stored by two tiles
    }
    if (out_len) std::memcpy(out, wo.data(), (size_t)out_len);
    std::memcpy(out_off, wf.data(), (size_t)(nrec + 1) * 8);
    return wo.pads_intact() && wf.pads_intact() ? 0 : 8;
}

}  // namespace

extern "C" {

int64_t shim_sub_tile(int geo) { return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE; }
int64_t shim_sub_window() { return kSubWindow; }

// in: n bytes, x: the texts, none of them 0xEE; off [nrec + 1] from pos0 to pos0 + n; loff [nrec + 1] from ra0 to ra0 + found; start,
// end [found], from pos0 on; xoff [found + 1]; n_sel, out_len: what (first, count) selects and makes.  Out: out[0 .. out_len), out_off[0 .. nrec] as the kernels
// leave them (a byte or word nobody stored reads 0xEE; the offsets start at rk0); totals[3]: what the plan pass and the scans found; stores[2]: bytes of out and
// words of out_off stored.  4: the totals differ from n_sel / out_len, 5: the plan and the place pass disagree on a chunk, 6: bad
// arguments, 7: a byte was stored twice, 8: one outside the arrays was written, 9: the plan pass found the arrays out of order, 10: a
// place was not stored
int shim_sub(int geo, const uint8_t* in, int64_t n, const int64_t* off, const int64_t* loff, int64_t nrec, const int64_t* start, const int64_t* end,
             const int64_t* xoff, const uint8_t* x, int64_t found, int64_t first, int64_t count, int src_mis, int x_mis, int dst_mis, int64_t pos0, int64_t ra0, int64_t rk0,
             int64_t n_sel, int64_t out_len, uint8_t* out, int64_t* out_off, int64_t* totals, int64_t* stores) {
    stores[0] = stores[1] = 0;
    switch (geo) {
    case 0: return run<Geo0>(in, n, off, loff, nrec, start, end, xoff, x, found, first, count, src_mis, x_mis, dst_mis, pos0, ra0, rk0, n_sel, out_len, out, out_off, totals, stores);
    case 1: return run<Geo1>(in, n, off, loff, nrec, start, end, xoff, x, found, first, count, src_mis, x_mis, dst_mis, pos0, ra0, rk0, n_sel, out_len, out, out_off, totals, stores);
    case 2: return run<Geo2>(in, n, off, loff, nrec, start, end, xoff, x, found, first, count, src_mis, x_mis, dst_mis, pos0, ra0, rk0, n_sel, out_len, out, out_off, totals, stores);
    default: return run<Geo3>(in, n, off, loff, nrec, start, end, xoff, x, found, first, count, src_mis, x_mis, dst_mis, pos0, ra0, rk0, n_sel, out_len, out, out_off, totals, stores);
    }
}

}  // extern "C"

#ifdef SUB_SHIM_MAIN
// The entry point over generated shapes, checked against a plain restatement: input lengths around the tile edges; matches of 0 to
// a few bytes with texts of 0 to a few bytes, dense and sparse; strings with and without matches, empty ones among them; every
// selection kind; every misalignment; a shift beyond 2^32.
namespace {

uint32_t rng_state = 24680;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int check(int geo, int64_t n, int density, int64_t first, int64_t count, int src_mis, int x_mis, int dst_mis, int64_t pos0, int64_t ra0, int64_t rk0) {
    std::vector<uint8_t> in((size_t)n), x, want;
    for (auto& c : in) c = (uint8_t)('a' + rnd() % 26);
    std::vector<int64_t> off{0}, loff{0}, S, E, XO{0}, woff{0};
    int64_t at = 0, n_sel = 0;
    while (true) {
        // a string: some bytes with matches among them
        int64_t len = density == 0 ? n - at : (int64_t)(rnd() % 4 == 0 ? 0 : rnd() % 60);
        if (len > n - at) len = n - at;
        const int64_t s0 = at, s1 = at + len;
        int64_t r = 0, p = s0;
        while (density && p <= s1) {
            const int64_t gap = (int64_t)(rnd() % (density == 1 ? 3 : 40));
            int64_t ms = p + gap, ml = (int64_t)(rnd() % 4);
            if (ms > s1) break;
            if (ms + ml > s1) ml = s1 - ms;
            const bool sel = first <= r && (count < 0 || r - first < count);
            const int64_t tl = (int64_t)(rnd() % 3 == 0 ? 0 : rnd() % 20);
            want.insert(want.end(), in.begin() + p, in.begin() + ms);
            for (int64_t k = 0; k < tl; ++k) x.push_back((uint8_t)('A' + rnd() % 26));
            if (sel) { want.insert(want.end(), x.end() - tl, x.end()); ++n_sel; }
            else want.insert(want.end(), in.begin() + ms, in.begin() + ms + ml);
            S.push_back(ms); E.push_back(ms + ml); XO.push_back((int64_t)x.size());
            p = ms + ml; ++r;
        }
        if (p < s1) want.insert(want.end(), in.begin() + p, in.begin() + s1);
        at = s1;
        off.push_back(at); loff.push_back((int64_t)S.size()); woff.push_back((int64_t)want.size());
        if (at >= n) break;
    }
    const int64_t nrec = (int64_t)off.size() - 1, found = (int64_t)S.size(), out_len = (int64_t)want.size();
    for (auto& v : off) v += pos0;
    for (auto& v : S) v += pos0;
    for (auto& v : E) v += pos0;
    for (auto& v : loff) v += ra0;
    for (auto& v : woff) v += rk0;
    if (x.empty()) x.push_back(0);
    std::vector<uint8_t> go((size_t)out_len + 1, 0x11);
    std::vector<int64_t> gf((size_t)nrec + 2, -1);
    int64_t totals[3], stores[2];
    const int rc = shim_sub(geo, in.data(), n, off.data(), loff.data(), nrec, S.data(), E.data(), XO.data(), x.data(), found, first, count, src_mis, x_mis,
                            dst_mis, pos0, ra0, rk0, n_sel, out_len, go.data(), gf.data(), totals, stores);
    if (rc) return rc;
    for (int64_t k = 0; k < out_len; ++k)
        if (go[(size_t)k] != want[(size_t)k]) return 11;
    for (int64_t i = 0; i <= nrec; ++i)
        if (gf[(size_t)i] != woff[(size_t)i]) return 12;
    if (go[(size_t)out_len] != 0x11 || gf[(size_t)nrec + 1] != -1) return 16;
    if (stores[0] != out_len || stores[1] != nrec + 1) return 15;
    return 0;
}

}  // namespace

int main() {
    int runs = 0;
    const int64_t sel[][2] = {{0, -1}, {0, 1}, {1, 1}, {2, -1}, {0, 0}, {3, 2}, {INT64_MAX, 1}, {0, INT64_MIN}};
    for (int geo = 0; geo < 4; ++geo) {
        const int64_t T = shim_sub_tile(geo);
        const int64_t sizes[] = {0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T, 2 * T + 77};
        for (int64_t n : sizes)
            for (int density = 0; density < 3; ++density)
                for (const auto& fc : sel) {
                    const bool far = (runs % 3) == 2;
                    const int rc = check(geo, n, density, fc[0], fc[1], runs % 16, (runs / 3 + 7) % 16, (runs / 2 + 5) % 16, far ? (5ll << 32) + 3 : 0,
                                         far ? 1024ll << 23 : 0, far ? (1ll << 34) + 11 : 0);
                    if (rc) {
                        std::printf("FAILED: geo %d n %lld density %d first %lld count %lld run %d: %d\n", geo, (long long)n, density, (long long)fc[0],
                                    (long long)fc[1], runs, rc);
                        return 1;
                    }
                    ++runs;
                }
    }
    std::printf("sub_shim: %d shapes ok\n", runs);
    return 0;
}
#endif
