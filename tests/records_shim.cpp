// records_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of the ragged-records passes
// (trre_amd/csrc/records_block.hpp: k_rec_part, k_rec_stage, k_rec_rank, k_rec_count, k_rec_locate, k_rec_restore) on the
// host, thread by thread, with barriers replaced by loop boundaries, so that tests/test_records_shim.py can check them against
// numpy over random buffers, record sizes, alignments and tile geometries without a GPU.  Not a product path: nothing in
// trre_amd/ links this file.
//
// base0 is added to every tile base, as if base0 newlines came before the buffer: the rank arithmetic beyond 2^32.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../trre_amd/csrc/records_block.hpp"

using namespace trre;

namespace {

// a 16-byte aligned copy of n bytes at offset mis (whole vectors behind the end)
struct Aligned {
    std::vector<uint8_t> buf;
    uint8_t* v0;
    Aligned(const uint8_t* src, int64_t n, int64_t mis) : buf((size_t)(mis + n + 64), 0xEE) {
        v0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 15) & ~(uintptr_t)15);
        if (n && src) std::memcpy(v0 + mis, src, (size_t)n);
    }
};

template <class G>
uint32_t scan_segments(const uint16_t* bits16, std::vector<uint32_t>& pre) {
    uint32_t run = 0;
    for (int t = 0; t < G::THREADS; ++t) {
        pre[t] = run;
        run += rec_seg_count<G>(bits16, t);
    }
    return run;
}

template <class G>
int stage(const uint8_t* in, int64_t n, int64_t mis, const int64_t* off, int64_t nrec, int keep, uint64_t base0, uint8_t* staged,
          int64_t* out_off, int64_t* part_out, uint64_t* cnt_out) {
    Aligned src(in, n, mis), snap(nullptr, n, mis);
    const int64_t tiles = n ? (mis + n + G::TILE - 1) / G::TILE : 0;
    std::vector<int64_t> part((size_t)tiles + 1);
    std::vector<uint64_t> cnt((size_t)tiles + 1), base((size_t)tiles + 1);
    RecArgs a{};
    a.in_v0 = src.v0; a.snap_v0 = snap.v0; a.vbeg = mis; a.vend = mis + n;
    a.off = off; a.nrec = nrec; a.out_off = out_off; a.part = part.data(); a.cnt = cnt.data(); a.base = base.data(); a.keep = (uint32_t)keep;
    for (int64_t b = 0; b <= tiles; ++b) rec_part_in(a, G::TILE, b);
    std::vector<uint32_t> bits32(G::NVEC / 2), pre(G::THREADS);
    uint16_t* bits16 = reinterpret_cast<uint16_t*>(bits32.data());
    std::vector<U128> w((size_t)G::THREADS * G::VECS);
    for (int64_t b = 0; b < tiles; ++b) {
        for (int t = 0; t < G::THREADS; ++t) rec_load_vecs<G>(a, b, t, *reinterpret_cast<U128(*)[G::VECS]>(&w[(size_t)t * G::VECS]));
        std::fill(bits32.begin(), bits32.end(), 0u);
        for (int t = 0; t < G::THREADS; ++t) rec_mark<G>(a, b, t, bits32.data());
        for (int t = 0; t < G::THREADS; ++t) rec_stage_vecs<G>(a, b, t, *reinterpret_cast<U128(*)[G::VECS]>(&w[(size_t)t * G::VECS]), bits16);
        cnt[b] = scan_segments<G>(bits16, pre);
        for (int t = 0; t < G::THREADS; ++t) rec_rank_records<G>(a, b, t, bits16, pre.data());
    }
    uint64_t run = base0;
    for (int64_t b = 0; b < tiles; ++b) { base[b] = run; run += cnt[b]; }
    base[tiles] = run;
    if (tiles == 0) base[0] = base0;
    for (int64_t i = 0; i < nrec; ++i) {
        if (tiles == 0) out_off[i + 1] = 0;                 // (n == 0: the runtime writes zeros without a launch)
        rec_add_base(a, G::TILE, i);
    }
    if (n) std::memcpy(staged, snap.v0 + mis, (size_t)n);
    for (int64_t b = 0; b <= tiles; ++b) part_out[b] = part[b];
    for (int64_t b = 0; b < tiles; ++b) cnt_out[b] = cnt[b];
    return 0;
}

template <class G>
int locate(const uint8_t* out, int64_t m, int64_t mis, int64_t* out_off, int64_t nrec, uint64_t base0) {
    Aligned src(out, m, mis);
    const int64_t tiles = (mis + m + G::TILE - 1) / G::TILE;
    std::vector<int64_t> part((size_t)tiles + 1);
    std::vector<uint64_t> cnt((size_t)tiles + 1), base((size_t)tiles + 1);
    RecArgs a{};
    a.in_v0 = src.v0; a.vbeg = mis; a.vend = mis + m;
    a.nrec = nrec; a.out_off = out_off; a.part = part.data(); a.cnt = cnt.data(); a.base = base.data();
    for (int64_t b = 0; b < tiles; ++b) {
        uint64_t c = 0;
        for (int t = 0; t < G::THREADS; ++t) c += rec_count_vecs<G>(a, b, t, nullptr);
        cnt[b] = c;
    }
    uint64_t run = base0;
    for (int64_t b = 0; b < tiles; ++b) { base[b] = run; run += cnt[b]; }
    base[tiles] = run;
    for (int64_t b = 0; b <= tiles; ++b) rec_part_out(a, b);
    std::vector<uint16_t> bits16(G::NVEC);
    std::vector<uint32_t> pre(G::THREADS);
    uint32_t bad = 0;
    for (int64_t b = 0; b < tiles; ++b) {
        for (int t = 0; t < G::THREADS; ++t) rec_count_vecs<G>(a, b, t, bits16.data());
        const uint32_t total = scan_segments<G>(bits16.data(), pre);
        for (int t = 0; t < G::THREADS; ++t) bad |= rec_locate_records<G>(a, b, t, bits16.data(), pre.data(), total);
    }
    return bad ? 1 : 0;
}

using Geo0 = RecGeo<4, 1>;     // 64-byte tiles
using Geo1 = RecGeo<4, 2>;     // 128
using Geo2 = RecGeo<64, 1>;    // 1 KiB
using Geo3 = RecGeoDev;        // the device's

}  // namespace

extern "C" {

int64_t shim_rec_tile(int geo) {
    return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE;
}

// staged copy (n bytes), ranks in out_off[1 .. nrec] (+ base0; bits 56..63: the replaced byte when keep), the first record of
// every tile (tiles + 1) and '\n' per tile
int shim_rec_stage(int geo, const uint8_t* in, int64_t n, int64_t mis, const int64_t* off, int64_t nrec, int keep, uint64_t base0,
                   uint8_t* staged, int64_t* out_off, int64_t* part, uint64_t* cnt) {
    switch (geo) {
    case 0: return stage<Geo0>(in, n, mis, off, nrec, keep, base0, staged, out_off, part, cnt);
    case 1: return stage<Geo1>(in, n, mis, off, nrec, keep, base0, staged, out_off, part, cnt);
    case 2: return stage<Geo2>(in, n, mis, off, nrec, keep, base0, staged, out_off, part, cnt);
    default: return stage<Geo3>(in, n, mis, off, nrec, keep, base0, staged, out_off, part, cnt);
    }
}

// out_off[1 .. nrec]: ranks (+ base0) in, output offsets out; returns 1 when a rank fell outside its tile
int shim_rec_locate(int geo, const uint8_t* out, int64_t m, int64_t mis, int64_t* out_off, int64_t nrec, uint64_t base0) {
    switch (geo) {
    case 0: return locate<Geo0>(out, m, mis, out_off, nrec, base0);
    case 1: return locate<Geo1>(out, m, mis, out_off, nrec, base0);
    case 2: return locate<Geo2>(out, m, mis, out_off, nrec, base0);
    default: return locate<Geo3>(out, m, mis, out_off, nrec, base0);
    }
}

// the replaced bytes back into dst (what an in-place call does after TRRE_E_CAPACITY)
void shim_rec_restore(uint8_t* dst, const int64_t* off, int64_t nrec, const int64_t* out_off) {
    RecArgs a{};
    a.off = off; a.nrec = nrec; a.out_off = const_cast<int64_t*>(out_off);
    for (int64_t i = 0; i < nrec; ++i) rec_restore(a, dst, i);
}

}  // extern "C"
