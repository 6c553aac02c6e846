// filter_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of k_filter_part, k_filter_count and k_filter_emit
// (trre_amd/csrc/records_block.hpp: filter_part, filter_count_strings, filter_mark, filter_seg_kept, filter_emit_rows,
// filter_emit_vecs, with k_chunk_scan between them) on the host, thread by thread, barriers as loop boundaries, so that
// tests/test_filter_shim.py can check them against numpy without a GPU.  Not a product path: nothing in trre_amd/ links this file.
// With -DFILTER_SHIM_MAIN the file is a program of its own that drives the same entry point over generated shapes, for a build
// with -fsanitize=address,undefined (a process of its own: a sanitized build is never loaded into an interpreter).
//
// src_mis and dst_mis are the addresses of the input and of the output mod 16.  pos0 (a multiple of the tile), rr0 and rk0 place
// the column as if pos0 input bytes, rr0 kept strings and rk0 kept bytes came before it: the offsets the caller passes start at
// pos0, the tiles that run are those from pos0 / TILE on, and every position and rank carries the shift — the arithmetic beyond
// 2^32.  Only the bytes and words of the column itself exist; the pointers are shifted to match.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "column_shim.hpp"

using namespace trre;

namespace {

// k_filter_part, k_filter_count, k_chunk_scan (twice), k_filter_emit
template <class G>
int run(const uint8_t* in, int64_t n, const int64_t* off, const int64_t* loff, int64_t nrec, int invert, int src_mis, int dst_mis, int64_t pos0,
        int64_t rr0, int64_t rk0, int64_t n_kept, int64_t out_len, uint8_t* out, int64_t* out_off, int64_t* rows, int64_t* totals, int64_t* stores) {
    if (pos0 % G::TILE || src_mis < 0 || src_mis > 15 || dst_mis < 0 || dst_mis > 15 || nrec < 1) return 6;
    // the input at src_mis behind a 16-byte aligned address, whole vectors readable around it
    std::vector<uint8_t> buf((size_t)n + 64 + 16, 0xEE);
    uint8_t* v0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 15) & ~(uintptr_t)15);
    if (n) std::memcpy(v0 + src_mis, in, (size_t)n);
    const int64_t b0 = pos0 / G::TILE;
    const int64_t tiles = (src_mis + n + G::TILE - 1) / G::TILE > 0 ? (src_mis + n + G::TILE - 1) / G::TILE : 1;
    std::vector<int64_t> part((size_t)tiles + 1, -1);
    std::vector<uint64_t> cnt((size_t)(2 * tiles), 0), base((size_t)(2 * (tiles + 1)), 0);
    Padded<uint8_t> wo(out_len, kUnstoredByte, dst_mis);
    Padded<int64_t> wf(n_kept + 1, kUnstored), wr(n_kept, kUnstored);
    FilterArgs a{};
    a.in_v0 = shifted(static_cast<const uint8_t*>(v0), pos0); a.vbeg = src_mis; a.n = pos0 + n;
    a.off = off; a.loff = loff; a.nrec = nrec; a.invert = (uint32_t)invert; a.tiles = tiles;
    a.part = shifted(part.data(), b0);
    a.out = shifted(wo.data(), rk0); a.out_len = rk0 + out_len;
    a.out_off = shifted(wf.data(), rr0); a.rows = shifted(wr.data(), rr0); a.n_kept = rr0 + n_kept;
    // k_filter_part
    for (int64_t b = b0; b <= b0 + tiles; ++b) filter_part(a, G::TILE, b);
    if (b0 == 0 && part[0] != 0) return 6;
    // k_filter_count (the kernels index cnt[x * tiles + b] and base[x * (tiles + 1) + b] with the absolute b)
    a.cnt = shifted(cnt.data(), b0);
    a.base = shifted(static_cast<const uint64_t*>(base.data()), b0);
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        const FilterTile<G> t(a, b);
        uint64_t r = 0, k = 0;
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint64_t rr, kk;
            filter_count_strings<G>(a, t, tid, rr, kk);
            r += rr; k += kk;
        }
        a.cnt[b] = r; a.cnt[a.tiles + b] = k;
    }
    // k_chunk_scan, twice
    const int64_t rank0[2] = {rr0, rk0};
    for (int x = 0; x < 2; ++x) {
        uint64_t sum = (uint64_t)rank0[x];
        for (int64_t k = 0; k < tiles; ++k) { base[(size_t)(x * (tiles + 1) + k)] = sum; sum += cnt[(size_t)(x * tiles + k)]; }
        base[(size_t)(x * (tiles + 1) + tiles)] = sum;
        totals[x] = (int64_t)sum - rank0[x];
    }
    if (totals[0] != n_kept || totals[1] != out_len) return 4;
    // k_filter_emit
    std::vector<U128> lds((size_t)G::NVEC + 2);
    std::vector<uint32_t> bits32((size_t)G::NVEC / 2 + 1), pv((size_t)G::NVEC + 1), pre(G::THREADS), pre_t(G::THREADS);
    std::vector<uint64_t> r0(G::THREADS);
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        const FilterTile<G> t(a, b);
        std::memset(lds.data(), 0xA5, lds.size() * sizeof(U128));                       // (what a tile before left there)
        std::fill(pv.begin(), pv.end(), 0xDEADBEEFu);
        std::fill(bits32.begin(), bits32.end(), 0u);
        uint64_t run_r = 0;                                                             // (barrier)
        for (int tid = 0; tid < G::THREADS; ++tid) {
            U128 w[G::VECS];
            filter_load_vecs<G>(a, t, tid, w);
            r0[tid] = run_r;
            run_r += filter_mark<G>(a, t, tid, bits32.data());
            filter_keep_vecs<G>(tid, w, lds.data());
        }
        if (run_r != a.cnt[b]) return 5;
        uint16_t* bits16 = reinterpret_cast<uint16_t*>(bits32.data());
        uint32_t run_t = 0, run_k = 0;                                                  // (barrier; the workgroup's scans)
        for (int tid = 0; tid < G::THREADS; ++tid) { pre_t[tid] = run_t; run_t += rec_seg_count<G>(bits16, tid); }
        for (int tid = 0; tid < G::THREADS; ++tid) { pre[tid] = run_k; run_k += filter_seg_kept<G>(a, t, tid, bits16, pre_t[tid]); }
        if (run_k != a.cnt[a.tiles + b]) return 5;
        for (int tid = 0; tid < G::THREADS; ++tid) str_fill_pv<G>(bits16, pre[tid], tid, pv.data());
        // (barrier) the bytes and words; each may be stored once
        const std::vector<uint8_t> bo(wo.w);
        const std::vector<int64_t> bf(wf.w), br(wr.w);
        for (int tid = 0; tid < G::THREADS; ++tid) {
            filter_emit_rows<G>(a, t, b, tid, r0[tid], bits16, pv.data());
            filter_emit_vecs<G>(a, b, tid, lds.data(), bits16, pre.data(), pv.data());
        }
        bool twice = false;
        stores[0] += changed(wo.w, bo, kUnstoredByte, &twice);
        stores[1] += changed(wf.w, bf, kUnstored, &twice);
        stores[2] += changed(wr.w, br, kUnstored, &twice);
        if (twice) return 7;                                                            // stored by two tiles
    }
    if (out_len) std::memcpy(out, wo.data(), (size_t)out_len);
    std::memcpy(out_off, wf.data(), (size_t)(n_kept + 1) * 8);
    if (n_kept) std::memcpy(rows, wr.data(), (size_t)n_kept * 8);
    return wo.pads_intact() && wf.pads_intact() && wr.pads_intact() ? 0 : 8;
}

}  // namespace

extern "C" {

int64_t shim_filter_tile(int geo) { return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE; }

// in: n bytes, none of them 0xEE; off [nrec + 1]: the strings' offsets, from pos0 to pos0 + n; loff [nrec + 1]: list offsets, a
// string being kept exactly when (loff[i + 1] > loff[i]) != invert; n_kept, out_len: what that keeps.  Out: out[0 .. out_len),
// out_off[0 .. n_kept], rows[0 .. n_kept) as the kernel leaves them (a byte or word nobody stored reads 0xEE: out_off[0] when pos0
// is not 0); totals[2]: what the count pass and the scans found; stores[3]: bytes of out, words of out_off, words of rows stored.
// 4: the counts differ from n_kept / out_len, 5: the two kernels disagree on a tile, 6: bad arguments, 7: a byte or word was
// stored twice, 8: one outside the arrays was written
int shim_filter(int geo, const uint8_t* in, int64_t n, const int64_t* off, const int64_t* loff, int64_t nrec, int invert, int src_mis, int dst_mis,
                int64_t pos0, int64_t rr0, int64_t rk0, int64_t n_kept, int64_t out_len, uint8_t* out, int64_t* out_off, int64_t* rows,
                int64_t* totals, int64_t* stores) {
    stores[0] = stores[1] = stores[2] = 0;
    switch (geo) {
    case 0: return run<Geo0>(in, n, off, loff, nrec, invert, src_mis, dst_mis, pos0, rr0, rk0, n_kept, out_len, out, out_off, rows, totals, stores);
    case 1: return run<Geo1>(in, n, off, loff, nrec, invert, src_mis, dst_mis, pos0, rr0, rk0, n_kept, out_len, out, out_off, rows, totals, stores);
    case 2: return run<Geo2>(in, n, off, loff, nrec, invert, src_mis, dst_mis, pos0, rr0, rk0, n_kept, out_len, out, out_off, rows, totals, stores);
    default: return run<Geo3>(in, n, off, loff, nrec, invert, src_mis, dst_mis, pos0, rr0, rk0, n_kept, out_len, out, out_off, rows, totals, stores);
    }
}

}  // extern "C"

#ifdef FILTER_SHIM_MAIN
// The entry point over generated shapes, checked against a plain restatement: input lengths around the tile edges; nothing and
// everything kept; 1-byte strings kept and dropped in turn; empty strings between non-empty ones; strings over whole tiles;
// random columns; every source and destination misalignment; both senses; a shift beyond 2^32.
namespace {

uint32_t rng_state = 13579;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// string lengths that add up to n, and the verdicts
void column(int pattern, int64_t n, int64_t T, std::vector<int64_t>& len, std::vector<int>& hit) {
    len.clear(); hit.clear();
    int64_t left = n;
    auto put = [&](int64_t l, int h) { l = l < left ? l : left; len.push_back(l); hit.push_back(h); left -= l; };
    switch (pattern) {
    case 0: put(n, 0); break;                                                // one string, dropped
    case 1: put(n, 1); break;                                                // one string, kept
    case 2: while (left) put(1, (int)(len.size() & 1)); break;               // 1-byte strings in turn
    case 3: while (left) { put(0, 1); put(3, 0); } put(0, 1); break;         // empty kept strings between dropped ones
    case 4: while (left) { put(0, 0); put(5, 1); } put(0, 0); break;         // ... and the reverse
    case 5: put(1, 1); put(n > 2 ? n - 2 : 0, 0); put(1, 1); break;          // a dropped string over the tiles between two kept bytes
    case 6: put(1, 0); put(n > 2 ? n - 2 : 0, 1); put(1, 0); break;          // a kept string over the tiles between dropped neighbours
    case 7: while (left) put(T - 1 + (int64_t)(len.size() % 3), (int)(rnd() & 1)); break;     // ends at T - 1, T, T + 1 and on
    default:
        while (left) put((int64_t)(rnd() % 5 == 0 ? 0 : rnd() % 40), (int)(rnd() % 3 != 0));
        if (len.empty()) put(0, 1);
    }
    if (len.empty()) put(0, (int)(pattern & 1));
}

int check(int geo, int64_t n, int pattern, int invert, int src_mis, int dst_mis, int64_t pos0, int64_t rr0, int64_t rk0) {
    const int64_t T = shim_filter_tile(geo);
    std::vector<int64_t> len;
    std::vector<int> hit;
    column(pattern, n, T, len, hit);
    if (pos0 && len[0] == 0) { len.erase(len.begin()); hit.erase(hit.begin()); }    // (far: the first string is not empty)
    if (len.empty()) return 0;
    const int64_t nrec = (int64_t)len.size();
    std::vector<uint8_t> in((size_t)n), wo;
    for (auto& c : in) c = (uint8_t)('a' + rnd() % 26);
    std::vector<int64_t> off{pos0}, loff{0}, wf{rk0}, wr;
    for (int64_t i = 0; i < nrec; ++i) {
        const int64_t s = off.back() - pos0;
        off.push_back(off.back() + len[(size_t)i]);
        loff.push_back(loff.back() + (hit[(size_t)i] ? 1 + (int64_t)(rnd() % 3) : 0));
        if ((hit[(size_t)i] != 0) != (invert != 0)) {
            wo.insert(wo.end(), in.begin() + s, in.begin() + s + len[(size_t)i]);
            wf.push_back(rk0 + (int64_t)wo.size());
            wr.push_back(i);
        }
    }
    const int64_t n_kept = (int64_t)wr.size(), out_len = (int64_t)wo.size();
    std::vector<uint8_t> go((size_t)out_len + 1, 0x11);
    std::vector<int64_t> gf((size_t)n_kept + 2, -1), gr((size_t)n_kept + 1, -1);
    int64_t totals[2], stores[3];
    const int rc = shim_filter(geo, in.data(), n, off.data(), loff.data(), nrec, invert, src_mis, dst_mis, pos0, rr0, rk0, n_kept, out_len, go.data(),
                               gf.data(), gr.data(), totals, stores);
    if (rc) return rc;
    for (int64_t k = 0; k < out_len; ++k)
        if (go[(size_t)k] != wo[(size_t)k]) return 11;
    for (int64_t r = 1; r <= n_kept; ++r)
        if (gf[(size_t)r] != wf[(size_t)r]) return 12;
    for (int64_t r = 0; r < n_kept; ++r)
        if (gr[(size_t)r] != wr[(size_t)r]) return 13;
    if (gf[0] != (pos0 ? kUnstored : 0)) return 14;
    if (go[(size_t)out_len] != 0x11 || gf[(size_t)n_kept + 1] != -1 || gr[(size_t)n_kept] != -1) return 16;
    if (stores[0] != out_len || stores[1] != n_kept + (pos0 ? 0 : 1) || stores[2] != n_kept) return 15;
    return 0;
}

}  // namespace

int main() {
    int runs = 0;
    for (int geo = 0; geo < 4; ++geo) {
        const int64_t T = shim_filter_tile(geo);
        const int64_t sizes[] = {0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T, 2 * T + 77};
        for (int64_t n : sizes)
            for (int pattern = 0; pattern < 9; ++pattern)
                for (int invert = 0; invert < 2; ++invert) {
                    const bool far = (runs % 3) == 2;
                    const int rc = check(geo, n, pattern, invert, runs % 16, (runs / 2 + 5) % 16, far ? ((5ll << 32) / T + 3) * T : 0,
                                         far ? (1ll << 33) + 7 : 0, far ? (1ll << 34) + 11 : 0);
                    if (rc) {
                        std::printf("FAILED: geo %d n %lld pattern %d invert %d far %d run %d: %d\n", geo, (long long)n, pattern, invert, (int)far, runs, rc);
                        return 1;
                    }
                    ++runs;
                }
    }
    std::printf("filter_shim: %d shapes ok\n", runs);
    return 0;
}
#endif
