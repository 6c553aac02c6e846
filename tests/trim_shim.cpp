// trim_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of k_trim_pick and k_trim_bounds (trre_amd/csrc/records_block.hpp:
// trim_pick_markers, trim_bounds, with the span call's bodies they reuse) and then those of k_filter_part, k_field_count,
// k_chunk_scan and k_field_emit, which the trim call runs unchanged with k = 0, on the host, thread by thread, a wave as 64
// sequential lanes, barriers as loop boundaries, so that tests/test_trim_shim.py can check them against tests/trim_lib.py without
// a GPU.  Not a product path: nothing in trre_amd/ links this file.  With -DTRIM_SHIM_MAIN the file is a program of its own that
// drives the same entry point over generated shapes, for a build with -fsanitize=address,undefined (a process of its own: a
// sanitized build is never loaded into an interpreter).
//
// src_mis and dst_mis are the addresses of the input and of the output mod 16.  pos0 (a multiple of the tile), ra0 (a multiple
// of half the tile) and rk0 place the column as if pos0 input bytes with ra0 matches in them and rk0 kept bytes came before it,
// exactly as tests/field_shim.cpp does: the arithmetic beyond 2^32.  The strings are numbered from 0 always.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "column_shim.hpp"

using namespace trre;

namespace {

struct Column {
    const uint8_t* in; int64_t n;            // the strings' bytes
    const int64_t* off; const int64_t* loff; // [nrec + 1] from pos0; from ra0
    int64_t nrec; uint32_t flags;
    const uint8_t* framed; int64_t m;        // the span call's framed text
    int src_mis, dst_mis;
    int64_t pos0, ra0, rk0;
    int64_t out_len;                         // what to expect of the count pass
    int views;                               // the caller gives begin and end
};
struct Result {
    uint8_t* out; int64_t* out_off; int64_t* lo; int64_t* hi; int64_t* begin; int64_t* end;
    int64_t* marks;                          // [6][nrec] the parked words
    int64_t* totals;                         // [2] entries, kept bytes
    int64_t* stores;                         // [12] bytes of out, words of out_off, of lo, hi, begin, end, of each of the six parked words
};

template <class G>
int run(const Column& c, const Result& r) {
    const int64_t nrec = c.nrec, fpos0 = c.pos0 + 2 * c.ra0;
    if (c.pos0 % G::TILE || fpos0 % G::TILE || c.src_mis < 0 || c.src_mis > 15 || c.dst_mis < 0 || c.dst_mis > 15 || nrec < 1) return 6;
    // the input at src_mis behind a 16-byte aligned address, the framed text at one, whole vectors readable around both
    std::vector<uint8_t> buf((size_t)c.n + 64 + 16, 0xEE), fbuf((size_t)c.m + 64 + 16, 0xEE);
    uint8_t* v0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 15) & ~(uintptr_t)15);
    uint8_t* f0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(fbuf.data()) + 15) & ~(uintptr_t)15);
    if (c.n) std::memcpy(v0 + c.src_mis, c.in, (size_t)c.n);
    if (c.m) std::memcpy(f0, c.framed, (size_t)c.m);
    Padded<int64_t> wlo(nrec, kUnstored), whi(nrec, kUnstored), wb(nrec, kUnstored), we(nrec, kUnstored), wm(6 * nrec, kUnstored),
        wf(nrec + 1, kUnstored);
    Padded<uint8_t> wo(c.out_len, kUnstoredByte, c.dst_mis);
    const int64_t b0 = c.pos0 / G::TILE;
    const int64_t tiles = (c.src_mis + c.n + G::TILE - 1) / G::TILE > 0 ? (c.src_mis + c.n + G::TILE - 1) / G::TILE : 1;
    TrimArgs t{};
    FieldArgs& a = t.a;
    a.f.in_v0 = shifted(static_cast<const uint8_t*>(v0), c.pos0); a.f.vbeg = c.src_mis; a.f.n = c.pos0 + c.n;
    a.f.off = c.off; a.f.loff = c.loff; a.f.nrec = nrec; a.f.tiles = tiles;
    a.k = 0; a.lo = wlo.data(); a.hi = whi.data();
    t.flags = c.flags; t.marks = wm.data();
    if (c.views) { t.begin = wb.data(); t.end = we.data(); }
    bool twice = false;
    // k_span_count and k_chunk_scan (three times) over the framed text, as the span call leaves them
    const int64_t fb0 = fpos0 / G::TILE, ftiles = (c.m + G::TILE - 1) / G::TILE;
    std::vector<uint64_t> fcnt((size_t)(3 * ftiles) + 1, 0), fbase((size_t)(3 * (ftiles + 1)), 0);
    SpanArgs sp{};
    sp.src = shifted(static_cast<const uint8_t*>(f0), fpos0); sp.total = fpos0 + c.m; sp.tiles = ftiles; sp.nrec = nrec; sp.lists_only = 1u;
    sp.cnt = shifted(fcnt.data(), fb0); sp.base = shifted(static_cast<const uint64_t*>(fbase.data()), fb0);
    for (int64_t b = fb0; b < fb0 + ftiles; ++b) {
        uint64_t tt[3] = {0, 0, 0};
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint32_t cc[3] = {0, 0, 0};
            span_mark_vecs<G>(sp, b, tid, nullptr, cc);
            for (int x = 0; x < 3; ++x) tt[x] += cc[x];
        }
        for (int x = 0; x < 3; ++x) sp.cnt[x * ftiles + b] = tt[x];
    }
    const int64_t frank0[3] = {c.ra0, c.ra0, 0};
    for (int x = 0; x < 3; ++x) {
        uint64_t sum = (uint64_t)frank0[x];
        for (int64_t k = 0; k < ftiles; ++k) { fbase[(size_t)(x * (ftiles + 1) + k)] = sum; sum += fcnt[(size_t)(x * ftiles + k)]; }
        fbase[(size_t)(x * (ftiles + 1) + ftiles)] = sum;
        if ((int64_t)sum - frank0[x] != (x < 2 ? c.loff[nrec] - c.loff[0] : nrec)) return 3;      // framed does not go with loff
    }
    // k_trim_pick
    {
        std::vector<uint16_t> bits((size_t)3 * G::NVEC);
        std::vector<uint32_t> pv_ab(G::NVEC), pv_nl(G::NVEC), pre_ab(G::THREADS), pre_nl(G::THREADS);
        for (int64_t b = fb0; b < fb0 + ftiles; ++b) {
            std::fill(bits.begin(), bits.end(), (uint16_t)0xA5A5);                      // (what a tile before left there)
            std::fill(pv_ab.begin(), pv_ab.end(), 0xDEADBEEFu);
            std::fill(pv_nl.begin(), pv_nl.end(), 0xDEADBEEFu);
            for (int tid = 0; tid < G::THREADS; ++tid) {
                uint32_t cc[3] = {0, 0, 0};
                span_mark_vecs<G>(sp, b, tid, bits.data(), cc);
            }
            uint32_t run_ab = 0, run_nl = 0;                                            // (barrier; the workgroup's two scans)
            for (int tid = 0; tid < G::THREADS; ++tid) {
                uint32_t ab, nl;
                span_seg_count<G>(bits.data(), tid, ab, nl);
                pre_ab[tid] = run_ab; pre_nl[tid] = run_nl;
                run_ab += ab; run_nl += nl;
            }
            for (int tid = 0; tid < G::THREADS; ++tid) span_fill_pv<G>(bits.data(), pre_ab[tid], pre_nl[tid], tid, pv_ab.data(), pv_nl.data());
            const std::vector<int64_t> bm(wm.w);                                        // (barrier) a word may be stored once
            for (int tid = 0; tid < G::THREADS; ++tid) trim_pick_markers<G>(t, sp, b, tid, bits.data(), pv_ab.data(), pv_nl.data());
            for (int x = 0; x < 6; ++x)
                for (int64_t i = 0; i < nrec; ++i) {
                    const size_t at = wm.at + (size_t)(x * nrec + i);
                    if (wm.w[at] == bm[at]) continue;
                    if (bm[at] != kUnstored) twice = true;
                    r.stores[6 + x] += 1;
                }
        }
    }
    std::memcpy(r.marks, wm.data(), (size_t)(6 * nrec) * 8);
    if (twice) return 7;                                                                // a parked word stored by two lanes
    // k_trim_bounds: a wave's 64 lanes in turn
    {
        const std::vector<int64_t> bl(wlo.w), bh(whi.w), bb(wb.w), be(we.w), bm(wm.w);
        const int64_t groups = (nrec + kMatchThreads - 1) / kMatchThreads;
        for (int64_t g = 0; g < groups; ++g)
            for (int tid = 0; tid < kMatchThreads; ++tid) {
                const int64_t i = g * kMatchThreads + tid;
                if (i < nrec) trim_bounds(t, i);
            }
        r.stores[2] += changed(wlo.w, bl, kUnstored, &twice);
        r.stores[3] += changed(whi.w, bh, kUnstored, &twice);
        r.stores[4] += changed(wb.w, bb, kUnstored, &twice);
        r.stores[5] += changed(we.w, be, kUnstored, &twice);
        if (wm.w != bm) return 7;                                                       // the bounds pass parks nothing
    }
    std::memcpy(r.lo, wlo.data(), (size_t)nrec * 8);
    std::memcpy(r.hi, whi.data(), (size_t)nrec * 8);
    std::memcpy(r.begin, wb.data(), (size_t)nrec * 8);
    std::memcpy(r.end, we.data(), (size_t)nrec * 8);
    if (twice) return 7;
    if (r.stores[2] != nrec || r.stores[3] != nrec) return 9;                           // a bound nobody stored
    // k_filter_part, k_field_count (the kernels index cnt[x * tiles + b] and base[x * (tiles + 1) + b] with the absolute b)
    std::vector<int64_t> part((size_t)tiles + 1, -1);
    std::vector<uint64_t> cnt((size_t)(2 * tiles), 0), base((size_t)(2 * (tiles + 1)), 0);
    a.f.part = shifted(part.data(), b0);
    a.f.cnt = shifted(cnt.data(), b0);
    a.f.base = shifted(static_cast<const uint64_t*>(base.data()), b0);
    a.f.out = shifted(wo.data(), c.rk0); a.f.out_len = c.rk0 + c.out_len; a.f.out_off = wf.data();
    for (int64_t b = b0; b <= b0 + tiles; ++b) filter_part(a.f, G::TILE, b);
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        const FilterTile<G> ft(a.f, b);
        uint64_t v = 0, k = 0;
        for (int tid = 0; tid < G::THREADS; ++tid) {
            uint64_t vv, kk;
            field_count_strings<G>(a, ft, tid, vv, kk);
            v += vv; k += kk;
        }
        a.f.cnt[b] = v; a.f.cnt[a.f.tiles + b] = k;
    }
    // k_chunk_scan, twice
    const int64_t rank0[2] = {0, c.rk0};
    for (int x = 0; x < 2; ++x) {
        uint64_t sum = (uint64_t)rank0[x];
        for (int64_t k = 0; k < tiles; ++k) { base[(size_t)(x * (tiles + 1) + k)] = sum; sum += cnt[(size_t)(x * tiles + k)]; }
        base[(size_t)(x * (tiles + 1) + tiles)] = sum;
        r.totals[x] = (int64_t)sum - rank0[x];
    }
    if (r.totals[0] != nrec || r.totals[1] != c.out_len) return 4;
    // k_field_emit
    std::vector<U128> lds((size_t)G::NVEC + 2);
    std::vector<uint32_t> bits32((size_t)G::NVEC / 2 + 1), pv((size_t)G::NVEC + 1), pre(G::THREADS), pre_t(G::THREADS);
    for (int64_t b = b0; b < b0 + tiles; ++b) {
        const FilterTile<G> ft(a.f, b);
        std::memset(lds.data(), 0xA5, lds.size() * sizeof(U128));                       // (what a tile before left there)
        std::fill(pv.begin(), pv.end(), 0xDEADBEEFu);
        std::fill(bits32.begin(), bits32.end(), 0u);
        for (int tid = 0; tid < G::THREADS; ++tid) {                                    // (barrier)
            U128 w[G::VECS];
            filter_load_vecs<G>(a.f, ft, tid, w);
            field_mark<G>(a, ft, tid, bits32.data());
            filter_keep_vecs<G>(tid, w, lds.data());
        }
        uint16_t* bits16 = reinterpret_cast<uint16_t*>(bits32.data());
        uint32_t run_t = 0, run_k = 0;                                                  // (barrier; the workgroup's scans)
        for (int tid = 0; tid < G::THREADS; ++tid) { pre_t[tid] = run_t; run_t += rec_seg_count<G>(bits16, tid); }
        for (int tid = 0; tid < G::THREADS; ++tid) { pre[tid] = run_k; run_k += filter_seg_kept<G>(a.f, ft, tid, bits16, pre_t[tid]); }
        if (run_k != a.f.cnt[a.f.tiles + b]) return 5;
        for (int tid = 0; tid < G::THREADS; ++tid) str_fill_pv<G>(bits16, pre[tid], tid, pv.data());
        // (barrier) the bytes and words; each may be stored once
        const std::vector<uint8_t> bo(wo.w);
        const std::vector<int64_t> bf(wf.w);
        for (int tid = 0; tid < G::THREADS; ++tid) {
            field_emit_offsets<G>(a, ft, b, tid, bits16, pv.data());
            filter_emit_vecs<G>(a.f, b, tid, lds.data(), bits16, pre.data(), pv.data());
        }
        r.stores[0] += changed(wo.w, bo, kUnstoredByte, &twice);
        r.stores[1] += changed(wf.w, bf, kUnstored, &twice);
        if (twice) return 7;                                                            // stored by two tiles
    }
    if (c.out_len) std::memcpy(r.out, wo.data(), (size_t)c.out_len);
    std::memcpy(r.out_off, wf.data(), (size_t)(nrec + 1) * 8);
    return wo.pads_intact() && wf.pads_intact() && wm.pads_intact() && wlo.pads_intact() && whi.pads_intact() && wb.pads_intact() &&
                   we.pads_intact()
               ? 0
               : 8;
}

}  // namespace

extern "C" {

int64_t shim_trim_tile(int geo) { return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE; }

// in: n bytes, none of them 0xEE; off [nrec + 1]: the strings' offsets, from pos0 to pos0 + n; loff [nrec + 1]: the span call's
// list offsets, from ra0; framed: the m bytes of its framed text — per string its position bytes with A (0x01) in front of every
// match and B (0x02) behind it, then '\n'; flags: TRRE_TRIM_LEFT | TRRE_TRIM_RIGHT; out_len: what the trim keeps; views: the caller
// gives begin and end.  Out: out[0 .. out_len), out_off[0 .. nrec], lo, hi, begin, end [0 .. nrec), marks [6][nrec] as the kernels
// leave them (a byte or word nobody stored reads 0xEE: out_off[0] when pos0 is not 0, begin and end without views, a parked word
// of a match that does not exist or of a side not asked for); totals[2]: what the count pass and the scans found; stores[12]:
// bytes of out, words of out_off, lo, hi, begin, end and of each of the six parked words stored.  marks, lo, hi, begin and end are
// filled in even when a later pass fails.
// 3: framed does not go with loff, 4: the counts differ from nrec / out_len, 5: the two kernels disagree on a tile, 6: bad
// arguments, 7: a byte or word was stored twice, 8: one outside the arrays was written, 9: a bound was not stored
int shim_trim(int geo, const uint8_t* in, int64_t n, const int64_t* off, const int64_t* loff, int64_t nrec, uint32_t flags, const uint8_t* framed,
              int64_t m, int src_mis, int dst_mis, int64_t pos0, int64_t ra0, int64_t rk0, int64_t out_len, int views, uint8_t* out,
              int64_t* out_off, int64_t* lo, int64_t* hi, int64_t* begin, int64_t* end, int64_t* marks, int64_t* totals, int64_t* stores) {
    for (int x = 0; x < 12; ++x) stores[x] = 0;
    totals[0] = totals[1] = -1;
    const Column c{in, n, off, loff, nrec, flags, framed, m, src_mis, dst_mis, pos0, ra0, rk0, out_len, views};
    const Result r{out, out_off, lo, hi, begin, end, marks, totals, stores};
    switch (geo) {
    case 0: return run<Geo0>(c, r);
    case 1: return run<Geo1>(c, r);
    case 2: return run<Geo2>(c, r);
    default: return run<Geo3>(c, r);
    }
}

}  // extern "C"

#ifdef TRIM_SHIM_MAIN
// The entry point over generated shapes, checked against a plain restatement of the rule: input lengths around the tile edges;
// one string and many; no match, a match on every byte, empty matches, one match over the whole string, matches at both ends of a
// string over the tiles, random ones; the three sides; with and without views; every source and destination misalignment; a
// shift beyond 2^32.
namespace {

uint32_t rng_state = 13579;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Span { int64_t s, e; };

// string lengths that add up to n, and every string's matches (positions inside the string)
void column(int pattern, int64_t n, int64_t T, std::vector<int64_t>& len, std::vector<std::vector<Span>>& sp) {
    len.clear(); sp.clear();
    int64_t left = n;
    auto put = [&](int64_t l) { l = l < left ? l : left; len.push_back(l); sp.emplace_back(); left -= l; return l; };
    switch (pattern) {
    case 0: put(n); break;                                                              // one string, no match
    case 1: { const int64_t l = put(n); for (int64_t x = 0; x < l; ++x) sp.back().push_back({x, x + 1}); break; }      // every byte a match
    case 2: { const int64_t l = put(n); for (int64_t x = 0; x <= l; ++x) sp.back().push_back({x, x}); break; }        // an empty match everywhere
    case 3: while (left) { const int64_t l = put(1); if (l && (len.size() & 1)) sp.back().push_back({0, 1}); } break;  // 1-byte strings, matched in turn
    case 4: { const int64_t l = put(n); if (l > 2) { sp.back().push_back({0, 1}); sp.back().push_back({l - 1, l}); sp.back().push_back({l, l}); } break; }
    case 5: { const int64_t l = put(n); sp.back().push_back({0, l}); break; }                                          // the string is one match
    case 6: while (left) { const int64_t l = put(T - 1 + (int64_t)(len.size() % 3)); if (l > 4) { sp.back().push_back({0, l / 2}); sp.back().push_back({l - 2, l}); } } break;
    default:
        while (left) {
            const int64_t l = put((int64_t)(rnd() % 5 == 0 ? 0 : rnd() % 40));
            for (int64_t x = 0; x <= l;) {
                if (rnd() % 3 == 0) {
                    const int64_t w = (int64_t)(rnd() % 4); const int64_t e = x + w < l ? x + w : l;
                    sp.back().push_back({x, e});
                    if (e > x && e == l && rnd() % 2) sp.back().push_back({l, l});      // the empty tail attempt
                    x = e + 1;
                } else ++x;
            }
        }
    }
    if (len.empty()) put(0);
}

int check(int geo, int64_t n, int pattern, uint32_t flags, int views, int src_mis, int dst_mis, int64_t pos0, int64_t ra0, int64_t rk0) {
    const int64_t T = shim_trim_tile(geo);
    std::vector<int64_t> len;
    std::vector<std::vector<Span>> sp;
    column(pattern, n, T, len, sp);
    if (pos0 && len[0] == 0) { len.erase(len.begin()); sp.erase(sp.begin()); }          // (far: the first string is not empty)
    if (len.empty()) return 0;
    const int64_t nrec = (int64_t)len.size();
    std::vector<uint8_t> in((size_t)n), wo, framed;
    for (auto& c : in) c = (uint8_t)('a' + rnd() % 26);
    std::vector<int64_t> off{pos0}, loff{ra0}, wf{rk0}, wlo, whi, wm((size_t)(6 * nrec), kUnstored);
    int64_t parked[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = 0; i < nrec; ++i) {
        const int64_t s = off.back() - pos0, l = len[(size_t)i], c = (int64_t)sp[(size_t)i].size();
        size_t j = 0;
        for (int64_t x = 0; x <= l; ++x) {
            while (j < (size_t)c && sp[(size_t)i][j].s == x) {
                framed.push_back(1);
                for (int64_t y = x; y < sp[(size_t)i][j].e; ++y) framed.push_back((uint8_t)'.');
                framed.push_back(2);
                x = sp[(size_t)i][j].e; ++j;
            }
            if (x < l) framed.push_back((uint8_t)'.');
        }
        framed.push_back((uint8_t)'\n');
        off.push_back(off.back() + l);
        loff.push_back(loff.back() + c);
        int64_t a = 0, b = l;
        for (const Span& q : sp[(size_t)i]) {
            if ((flags & 1u) && q.s == 0 && q.e > a) a = q.e;
            if ((flags & 2u) && q.e == l && q.s < b) b = q.s;
        }
        if (b < a) b = a;
        const int64_t roles[3] = {0, c - 1, c - 2};
        for (int x = 0; x < 3; ++x) {
            if (roles[x] < 0 || roles[x] >= c || !(flags & (x == 0 ? 1u : 2u))) continue;
            wm[(size_t)((2 * x) * nrec + i)] = pos0 + s + sp[(size_t)i][(size_t)roles[x]].s;
            wm[(size_t)((2 * x + 1) * nrec + i)] = pos0 + s + sp[(size_t)i][(size_t)roles[x]].e;
            parked[2 * x] += 1; parked[2 * x + 1] += 1;
        }
        wlo.push_back(pos0 + s + a); whi.push_back(pos0 + s + b);
        wo.insert(wo.end(), in.begin() + s + a, in.begin() + s + b);
        wf.push_back(rk0 + (int64_t)wo.size());
    }
    const int64_t out_len = (int64_t)wo.size(), m = (int64_t)framed.size();
    std::vector<uint8_t> go((size_t)out_len + 1, 0x11);
    std::vector<int64_t> gf((size_t)nrec + 2, -1), glo((size_t)nrec + 1, -1), ghi((size_t)nrec + 1, -1), gb((size_t)nrec + 1, -1), ge((size_t)nrec + 1, -1),
        gm((size_t)(6 * nrec) + 1, -1);
    int64_t totals[2], stores[12];
    const int rc = shim_trim(geo, in.data(), n, off.data(), loff.data(), nrec, flags, framed.data(), m, src_mis, dst_mis, pos0, ra0, rk0, out_len, views,
                             go.data(), gf.data(), glo.data(), ghi.data(), gb.data(), ge.data(), gm.data(), totals, stores);
    if (rc) return rc;
    for (int64_t i = 0; i < nrec; ++i) {
        if (glo[(size_t)i] != wlo[(size_t)i] || ghi[(size_t)i] != whi[(size_t)i]) return 10;
        if (gb[(size_t)i] != (views ? wlo[(size_t)i] : kUnstored) || ge[(size_t)i] != (views ? whi[(size_t)i] : kUnstored)) return 17;
    }
    for (int64_t x = 0; x < 6 * nrec; ++x)
        if (gm[(size_t)x] != wm[(size_t)x]) return 13;
    for (int64_t x = 0; x < out_len; ++x)
        if (go[(size_t)x] != wo[(size_t)x]) return 11;
    for (int64_t i = 1; i <= nrec; ++i)
        if (gf[(size_t)i] != wf[(size_t)i]) return 12;
    if (gf[0] != (pos0 ? kUnstored : 0)) return 14;
    if (go[(size_t)out_len] != 0x11 || gf[(size_t)nrec + 1] != -1 || glo[(size_t)nrec] != -1 || ghi[(size_t)nrec] != -1 || gb[(size_t)nrec] != -1 ||
        ge[(size_t)nrec] != -1 || gm[(size_t)(6 * nrec)] != -1)
        return 16;
    if (stores[0] != out_len || stores[1] != nrec + (pos0 ? 0 : 1) || stores[2] != nrec || stores[3] != nrec || stores[4] != (views ? nrec : 0) ||
        stores[5] != (views ? nrec : 0))
        return 15;
    for (int x = 0; x < 6; ++x)
        if (stores[6 + x] != parked[x]) return 18;
    return 0;
}

}  // namespace

int main() {
    int runs = 0;
    for (int geo = 0; geo < 4; ++geo) {
        const int64_t T = shim_trim_tile(geo);
        const int64_t sizes[] = {0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T, 2 * T + 77};
        for (int64_t n : sizes)
            for (int pattern = 0; pattern < 8; ++pattern)
                for (uint32_t flags = 1; flags <= 3; ++flags)
                    for (int views = 0; views < 2; ++views) {
                        const bool far = (runs % 3) == 2;
                        const int rc = check(geo, n, pattern, flags, views, runs % 16, (runs / 2 + 5) % 16, far ? ((5ll << 32) / T + 3) * T : 0,
                                             far ? T << 23 : 0, far ? (1ll << 34) + 11 : 0);
                        if (rc) {
                            std::printf("FAILED: geo %d n %lld pattern %d flags %u views %d far %d run %d: %d\n", geo, (long long)n, pattern, flags, views,
                                        (int)far, runs, rc);
                            return 1;
                        }
                        ++runs;
                    }
    }
    std::printf("trim_shim: %d shapes ok\n", runs);
    return 0;
}
#endif
