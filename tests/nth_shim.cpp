// nth_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of k_nth_plan, k_nth_offsets and k_nth_emit
// (trre_amd/csrc/records_block.hpp: nth_plan_string, nth_plan, nth_offsets_sum, nth_offsets_thread, nth_emit_window,
// nth_keep_window, nth_emit_vecs, with k_chunk_scan between them) on the host, thread by thread, barriers as loop boundaries and a
// wave's ballot as a loop over its 64 lanes, so that tests/test_nth_shim.py can check them against tests/nth_lib.py without a GPU.
// Not a product path: nothing in trre_amd/ links this file.  With -DNTH_SHIM_MAIN the file is a program of its own that drives the
// same entry point over generated shapes, for a build with -fsanitize=address,undefined (a process of its own: a sanitized build is
// never loaded into an interpreter).
//
// x_mis and dst_mis are the addresses of the texts and of the output mod 16.  The list offsets, the texts and their offsets are the
// caller's: what the find call's two scans and k_find_unframe leave in the library's arrays.
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
int run(const int64_t* loff, int64_t nrec, const int64_t* xoff, const uint8_t* x, int64_t found, int64_t k, int x_mis, int dst_mis, int64_t n_valid,
        int64_t out_len, uint8_t* out, int64_t* out_off, uint64_t* valid, int64_t* totals, int64_t* stores) {
    if (x_mis < 0 || x_mis > 15 || dst_mis < 0 || dst_mis > 15 || nrec < 1 || found < 0) return 6;
    const int64_t per = (int64_t)G::THREADS * kNthPer, chunks = (nrec + per - 1) / per, nwords = (nrec + 63) / 64;
    const Staged sx(x, xoff[found], x_mis);
    std::vector<uint64_t> cnt((size_t)(2 * chunks), 0), base((size_t)(2 * (chunks + 1)), 0);
    uint32_t status = 0;
    Padded<uint8_t> wo(out_len, kUnstoredByte, dst_mis);
    Padded<int64_t> wf(nrec + 1, kUnstored), ws(nrec, kUnstored), wv(nwords, kUnstored);
    NthArgs a{};
    a.L = loff; a.nrec = nrec; a.XO = xoff; a.X = sx.p; a.x_len = xoff[found]; a.found = found; a.k = k;
    a.src = ws.data(); a.valid = reinterpret_cast<uint64_t*>(wv.data()); a.words = nwords;
    a.chunks = chunks; a.cnt = cnt.data(); a.base = base.data(); a.status = &status;
    // k_nth_plan: every round of every wave is one ballot; lane 0 stores the word
    {
        const std::vector<int64_t> bs(ws.w), bv(wv.w);
        for (int64_t c = 0; c < chunks; ++c) {
            uint64_t t[2] = {0, 0};
            for (int w = 0; w < G::THREADS / 64; ++w)
                for (int r = 0; r < kNthPer; ++r) {
                    uint64_t word = 0;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int64_t i = nth_plan_string<G::THREADS>(c, r, w * 64 + lane);
                        uint32_t bad = 0;
                        if (i < nrec && nth_plan(a, i, t, bad)) word |= 1ull << lane;
                        status |= bad;
                    }
                    const int64_t at = nth_plan_string<G::THREADS>(c, r, w * 64) / 64;
                    if (at < a.words) a.valid[at] = word;
                }
            a.cnt[c] = t[0]; a.cnt[chunks + c] = t[1];
        }
        bool twice = false;
        stores[2] += changed(ws.w, bs, kUnstored, &twice);
        // (a bitmap word may be the sentinel's own pattern only if 64 strings in a row had it: the tests' columns have none)
        stores[1] += changed(wv.w, bv, kUnstored, &twice);
    }
    if (status) return 9;
    // k_chunk_scan, twice
    for (int q = 0; q < 2; ++q) {
        uint64_t sum = 0;
        for (int64_t c = 0; c < chunks; ++c) { base[(size_t)(q * (chunks + 1) + c)] = sum; sum += cnt[(size_t)(q * chunks + c)]; }
        base[(size_t)(q * (chunks + 1) + chunks)] = sum;
        totals[q] = (int64_t)sum;
    }
    if (totals[0] != n_valid || totals[1] != out_len) return 4;
    a.out = wo.data(); a.out_len = out_len; a.out_off = wf.data();
    // k_nth_offsets: the threads' sums, their exclusive scan over the workgroup (barrier), the offsets
    {
        const std::vector<int64_t> bf(wf.w);
        for (int64_t c = 0; c < chunks; ++c) {
            std::vector<uint64_t> pre(G::THREADS);
            uint64_t sum = 0;
            for (int tid = 0; tid < G::THREADS; ++tid) { pre[(size_t)tid] = sum; sum += nth_offsets_sum<G::THREADS>(a, c, tid); }
            if (sum != a.cnt[chunks + c]) return 5;
            for (int tid = 0; tid < G::THREADS; ++tid) nth_offsets_thread<G::THREADS>(a, c, tid, pre[(size_t)tid]);
        }
        bool twice = false;
        stores[3] += changed(wf.w, bf, kUnstored, &twice);
    }
    // k_nth_emit
    const int64_t A = (int64_t)(reinterpret_cast<uintptr_t>(a.out) & 15u);
    const int64_t tiles = out_len ? (out_len + A + G::TILE - 1) / G::TILE : 0;
    std::vector<int64_t> image((size_t)kSubWindow);
    for (int64_t b = 0; b < tiles; ++b) {
        const NthTile<G> t(a, b);
        int64_t win[2] = {-7, -7};
        std::fill(image.begin(), image.end(), (int64_t)0x5A5A5A5A5A5A5A5All);            // (what a tile before left there)
        nth_emit_window<G>(a, t, win);                                                   // (thread 0; barrier)
        for (int tid = 0; tid < G::THREADS; ++tid) nth_keep_window<G>(a, win, tid, image.data());
        const std::vector<uint8_t> bo(wo.w);                                             // (barrier)
        for (int tid = 0; tid < G::THREADS; ++tid) nth_emit_vecs<G>(a, t, b, tid, win, image.data());
        bool twice = false;
        stores[0] += changed(wo.w, bo, kUnstoredByte, &twice);
        if (twice) return 7;                                                             // stored by two tiles
    }
    if (out_len) std::memcpy(out, wo.data(), (size_t)out_len);
    std::memcpy(out_off, wf.data(), (size_t)(nrec + 1) * 8);
    std::memcpy(valid, wv.data(), (size_t)nwords * 8);
    return wo.pads_intact() && wf.pads_intact() && ws.pads_intact() && wv.pads_intact() ? 0 : 8;
}

}  // namespace

extern "C" {

int64_t shim_nth_tile(int geo) { return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE; }
int64_t shim_nth_chunk(int geo) { return kNthPer * (geo == 0 ? Geo0::THREADS : geo == 1 ? Geo1::THREADS : geo == 2 ? Geo2::THREADS : Geo3::THREADS); }
int64_t shim_nth_window() { return kSubWindow; }

// loff [nrec + 1] from 0 to found; xoff [found + 1]; x: the texts, none of their bytes 0xEE; n_valid, out_len: what k selects.
// Out: out[0 .. out_len), out_off[0 .. nrec], valid[ceil(nrec / 64)] as the kernels leave them (a byte or word nobody stored reads
// 0xEE); totals[2]: what the plan pass and the scans found; stores[4]: bytes of out, words of the bitmap, words of src and words of
// out_off stored.  4: the totals differ from n_valid / out_len, 5: the plan and the offsets pass disagree on a chunk, 6: bad
// arguments, 7: a byte was stored twice, 8: one outside the arrays was written, 9: the plan pass found the arrays out of order
int shim_nth(int geo, const int64_t* loff, int64_t nrec, const int64_t* xoff, const uint8_t* x, int64_t found, int64_t k, int x_mis, int dst_mis,
             int64_t n_valid, int64_t out_len, uint8_t* out, int64_t* out_off, uint64_t* valid, int64_t* totals, int64_t* stores) {
    stores[0] = stores[1] = stores[2] = stores[3] = 0;
    switch (geo) {
    case 0: return run<Geo0>(loff, nrec, xoff, x, found, k, x_mis, dst_mis, n_valid, out_len, out, out_off, valid, totals, stores);
    case 1: return run<Geo1>(loff, nrec, xoff, x, found, k, x_mis, dst_mis, n_valid, out_len, out, out_off, valid, totals, stores);
    case 2: return run<Geo2>(loff, nrec, xoff, x, found, k, x_mis, dst_mis, n_valid, out_len, out, out_off, valid, totals, stores);
    default: return run<Geo3>(loff, nrec, xoff, x, found, k, x_mis, dst_mis, n_valid, out_len, out, out_off, valid, totals, stores);
    }
}

}  // extern "C"

#ifdef NTH_SHIM_MAIN
// The entry point over generated shapes, checked against a plain restatement: string counts around the waves and the chunks;
// lists of 0 to a few matches with texts of 0 to many bytes; every k kind; every misalignment.
namespace {

uint32_t rng_state = 13579;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int check(int geo, int64_t nrec, int density, int64_t longest, int64_t k, int x_mis, int dst_mis) {
    std::vector<int64_t> loff{0}, xoff{0};
    std::vector<uint8_t> x;
    for (int64_t i = 0; i < nrec; ++i) {
        const int64_t c = density == 0 ? (int64_t)(rnd() % 2) : (int64_t)(rnd() % 5);
        for (int64_t r = 0; r < c; ++r) {
            const int64_t tl = rnd() % 3 == 0 ? 0 : (int64_t)(rnd() % (uint32_t)longest);
            for (int64_t q = 0; q < tl; ++q) x.push_back((uint8_t)('A' + rnd() % 26));
            xoff.push_back((int64_t)x.size());
        }
        loff.push_back((int64_t)xoff.size() - 1);
    }
    const int64_t found = (int64_t)xoff.size() - 1;
    std::vector<uint8_t> want;
    std::vector<int64_t> woff{0};
    std::vector<uint64_t> wbits((size_t)((nrec + 63) / 64), 0);
    int64_t n_valid = 0;
    for (int64_t i = 0; i < nrec; ++i) {
        const int64_t c = loff[(size_t)i + 1] - loff[(size_t)i];
        int64_t kk = -1;
        if (k >= 0 && k < c) kk = k;
        if (k < 0 && k >= -c) kk = c + k;
        if (kk >= 0) {
            const int64_t j = loff[(size_t)i] + kk;
            want.insert(want.end(), x.begin() + xoff[(size_t)j], x.begin() + xoff[(size_t)j + 1]);
            wbits[(size_t)(i / 64)] |= 1ull << (i % 64);
            ++n_valid;
        }
        woff.push_back((int64_t)want.size());
    }
    const int64_t out_len = (int64_t)want.size();
    if (x.empty()) x.push_back(0);
    std::vector<uint8_t> go((size_t)out_len + 1, 0x11);
    std::vector<int64_t> gf((size_t)nrec + 2, -1);
    std::vector<uint64_t> gv(wbits.size() + 1, 0x33);
    int64_t totals[2], stores[4];
    const int rc = shim_nth(geo, loff.data(), nrec, xoff.data(), x.data(), found, k, x_mis, dst_mis, n_valid, out_len, go.data(), gf.data(), gv.data(),
                            totals, stores);
    if (rc) return rc;
    for (int64_t q = 0; q < out_len; ++q)
        if (go[(size_t)q] != want[(size_t)q]) return 11;
    for (int64_t i = 0; i <= nrec; ++i)
        if (gf[(size_t)i] != woff[(size_t)i]) return 12;
    for (size_t w = 0; w < wbits.size(); ++w)
        if (gv[w] != wbits[w]) return 13;
    if (go[(size_t)out_len] != 0x11 || gf[(size_t)nrec + 1] != -1 || gv[wbits.size()] != 0x33) return 16;
    if (stores[0] != out_len || stores[1] != (int64_t)wbits.size() || stores[2] != nrec || stores[3] != nrec + 1) return 15;
    return 0;
}

}  // namespace

int main() {
    int runs = 0;
    const int64_t ks[] = {0, 1, 2, -1, -2, 4, INT64_MAX, INT64_MIN};
    for (int geo = 0; geo < 4; ++geo) {
        const int64_t C = shim_nth_chunk(geo), T = shim_nth_tile(geo);
        const int64_t counts[] = {1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 77};
        for (int64_t nrec : counts)
            for (int density = 0; density < 2; ++density)
                for (int64_t k : ks) {
                    const int64_t longest = (runs % 5) == 4 ? 2 * T + 50 : (runs % 5) == 3 ? 300 : 20;
                    const int64_t few = longest > 300 && nrec > 70 ? 70 : nrec;      // (long texts on a few strings)
                    const int rc = check(geo, few, density, longest, k, runs % 16, (runs / 2 + 5) % 16);
                    if (rc) {
                        std::printf("FAILED: geo %d nrec %lld density %d k %lld run %d: %d\n", geo, (long long)few, density, (long long)k, runs, rc);
                        return 1;
                    }
                    ++runs;
                }
    }
    std::printf("nth_shim: %d shapes ok\n", runs);
    return 0;
}
#endif
