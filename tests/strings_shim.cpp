// strings_shim.cpp — TEST INFRASTRUCTURE: runs the per-thread bodies of the packed-strings passes
// (trre_amd/csrc/records_block.hpp: k_str_part, k_str_stage, k_str_rank, k_str_unframe) on the host, thread by thread, with
// barriers replaced by loop boundaries, so that tests/test_strings_shim.py can check them against numpy over random buffers,
// string sizes, alignments and tile geometries without a GPU.  Not a product path: nothing in trre_amd/ links this file.
//
// base0 is added to every tile base, as if base0 newlines came before the buffer: the rank arithmetic beyond 2^32.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../trre_amd/csrc/records_block.hpp"

using namespace trre;

namespace {

constexpr uint8_t kFill = 0xEE;

// n bytes at offset mis of a 16-byte aligned address, 64 sentinel bytes on either side
struct Aligned {
    std::vector<uint8_t> buf;
    uint8_t* v0;     // 16-byte aligned, 64 bytes into the buffer
    Aligned(const uint8_t* src, int64_t n, int64_t mis) : buf((size_t)(mis + n + 160), kFill) {
        v0 = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 64 + 15) & ~(uintptr_t)15);
        if (n && src) std::memcpy(v0 + mis, src, (size_t)n);
    }
    // every byte outside [v0 + from, v0 + to) still the sentinel
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
    // the exclusive scan of the segments' counts; returns the total
    uint32_t scan() {
        uint32_t run = 0;
        for (int t = 0; t < G::THREADS; ++t) { pre[t] = run; run += rec_seg_count<G>(bits16(), t); }
        return run;
    }
    // loads, marks, the image in LDS, the marks before every vector; returns the tile's marks
    uint32_t front(const StrArgs& a, const StrTile<G>& t, bool stage) {
        for (int k = 0; k < G::THREADS; ++k) str_load_vecs<G>(a, t, k, regs(k));
        std::fill(bits32.begin(), bits32.end(), 0u);
        std::memset(bytes.data(), 0x5A, bytes.size() * sizeof(U128));     // (what a tile before left there)
        for (int k = 0; k < G::THREADS; ++k) { str_mark<G>(a, t, k, bits32.data(), stage); str_keep_vecs<G>(t, k, regs(k), bytes.data()); }
        const uint32_t marks = scan();
        for (int k = 0; k < G::THREADS; ++k) str_fill_pv<G>(bits16(), pre[k], k, pv.data());
        return marks;
    }
};

template <class G>
int stage(const uint8_t* in, int64_t n, int64_t mis, const int64_t* off, int64_t nrec, uint64_t base0, uint8_t* staged, int64_t* out_off,
          int64_t* part_out, uint64_t* cnt_out) {
    const int64_t total = n + nrec;
    Aligned src(in, n, mis), snap(nullptr, total, 0);
    const int64_t tiles = (total + G::TILE - 1) / G::TILE;
    std::vector<int64_t> part((size_t)tiles + 1);
    std::vector<uint64_t> cnt((size_t)tiles + 1), base((size_t)tiles + 1);
    StrArgs a{};
    a.src_v0 = src.v0; a.vbeg = mis; a.total = total; a.dst = snap.v0;
    a.off = off; a.nrec = nrec; a.out_off = out_off; a.part = part.data(); a.cnt = cnt.data(); a.base = base.data();
    for (int64_t b = 0; b <= tiles; ++b) str_part(a, part.data(), G::TILE, 0, b);
    Lds<G> l;
    for (int64_t b = 0; b < tiles; ++b) {
        const StrTile<G> t(a, b, true);
        l.front(a, t, true);
        for (int k = 0; k < G::THREADS; ++k) str_stage_vecs<G>(a, t, k, l.bytes.data(), l.bits16(), l.pv.data());
        cnt[b] = l.scan();
        for (int k = 0; k < G::THREADS; ++k) str_rank_records<G>(a, t, k, l.bits16(), l.pre.data());
    }
    uint64_t run = base0;
    for (int64_t b = 0; b < tiles; ++b) { base[b] = run; run += cnt[b]; }
    base[tiles] = run;
    for (int64_t i = 0; i < nrec; ++i) str_add_base(a, G::TILE, i);
    if (total) std::memcpy(staged, snap.v0, (size_t)total);
    for (int64_t b = 0; b <= tiles; ++b) part_out[b] = part[b];
    for (int64_t b = 0; b < tiles; ++b) cnt_out[b] = cnt[b];
    return snap.untouched_outside(0, (total + 15) & ~(int64_t)15) ? 0 : 2;       // whole vectors, nothing else
}

template <class G>
int unframe(const uint8_t* framed, int64_t m, int64_t* out_off, int64_t nrec, int64_t dst_mis, uint8_t* out) {
    Aligned src(framed, m, 0), dst(nullptr, m - nrec, dst_mis);
    const int64_t tiles = (m + G::TILE - 1) / G::TILE;
    std::vector<int64_t> part((size_t)tiles + 1);
    StrArgs a{};
    a.src_v0 = src.v0; a.total = m; a.dst = dst.v0 + dst_mis; a.dst_len = m - nrec;
    a.nrec = nrec; a.out_off = out_off; a.part = part.data();
    for (int64_t b = 0; b <= tiles; ++b) str_part(a, part.data(), G::TILE, 1, b);
    Lds<G> l;
    for (int64_t b = 0; b < tiles; ++b) {
        const StrTile<G> t(a, b, false);
        const uint32_t marks = l.front(a, t, false);
        const StrOut<G> o(a, t, marks);
        std::fill(l.inv.begin(), l.inv.end(), (uint16_t)0xFFFF);
        for (int k = 0; k < G::THREADS; ++k) str_fill_inv<G>(t, o, k, l.bits16(), l.pv.data(), l.inv.data());
        for (int g = 0; g < o.ng; ++g) if (l.inv[g] == 0xFFFF) return 3;             // a destination vector without a source
        for (int k = 0; k < G::THREADS; ++k) str_unframe_vecs<G>(a, t, o, k, l.bytes.data(), l.bits16(), l.pv.data(), l.inv.data());
    }
    if (m - nrec) std::memcpy(out, dst.v0 + dst_mis, (size_t)(m - nrec));
    return dst.untouched_outside(dst_mis, dst_mis + m - nrec) ? 0 : 2;
}

using Geo0 = RecGeo<4, 1>;     // 64-byte tiles
using Geo1 = RecGeo<4, 2>;     // 128
using Geo2 = RecGeo<64, 1>;    // 1 KiB
using Geo3 = StrGeoDev;        // the device's

}  // namespace

extern "C" {

int64_t shim_str_tile(int geo) {
    return geo == 0 ? Geo0::TILE : geo == 1 ? Geo1::TILE : geo == 2 ? Geo2::TILE : Geo3::TILE;
}

// the staged text (n + nrec bytes), ranks in out_off[1 .. nrec] (+ base0), the first record of every tile (tiles + 1) and
// '\n' per tile; 2: a byte outside the staged text's whole vectors was written
int shim_str_stage(int geo, const uint8_t* in, int64_t n, int64_t mis, const int64_t* off, int64_t nrec, uint64_t base0, uint8_t* staged,
                   int64_t* out_off, int64_t* part, uint64_t* cnt) {
    switch (geo) {
    case 0: return stage<Geo0>(in, n, mis, off, nrec, base0, staged, out_off, part, cnt);
    case 1: return stage<Geo1>(in, n, mis, off, nrec, base0, staged, out_off, part, cnt);
    case 2: return stage<Geo2>(in, n, mis, off, nrec, base0, staged, out_off, part, cnt);
    default: return stage<Geo3>(in, n, mis, off, nrec, base0, staged, out_off, part, cnt);
    }
}

// out_off[1 .. nrec]: located positions in (just past each record's closing '\n' in framed), output offsets out; out: the
// m - nrec unframed bytes, written at misalignment dst_mis; 2: a byte outside them was written
int shim_str_unframe(int geo, const uint8_t* framed, int64_t m, int64_t* out_off, int64_t nrec, int64_t dst_mis, uint8_t* out) {
    switch (geo) {
    case 0: return unframe<Geo0>(framed, m, out_off, nrec, dst_mis, out);
    case 1: return unframe<Geo1>(framed, m, out_off, nrec, dst_mis, out);
    case 2: return unframe<Geo2>(framed, m, out_off, nrec, dst_mis, out);
    default: return unframe<Geo3>(framed, m, out_off, nrec, dst_mis, out);
    }
}

}  // extern "C"
