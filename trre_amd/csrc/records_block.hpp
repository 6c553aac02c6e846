// records_block.hpp — per-thread bodies of the ragged-records passes (trre_scan_device_records).
//
// Records are in[off[i] .. off[i+1]).  Record i alone prints what the reference prints for it as a file: its lines, the last
// one cut one byte short (getline's record minus its last byte, trre_nft.c:775-790).  So a copy of the input in which the last
// byte of every non-empty record is '\n' (the STAGED copy) holds exactly the records' lines, and the plain scan of that copy is
// the concatenation of the records' outputs.  In scan mode every line prints exactly one framing '\n' and, for the programs this
// path takes (runtime.cpp: prints_newline), no other: record i's output ends just past output newline number R_i, where
//     R_i = number of '\n' in staged[0, off[i+1])
// (an empty record has the R of the record before it, and prints nothing).  The passes:
//   k_rec_check   the offsets: off[0] = 0, off[nrec] = n, no decrease (a status word)
//   k_rec_part    the first record of every tile (a binary search per tile: the merge-path partition of records against tiles)
//   k_rec_stage   input tile -> staged copy, '\n' per tile, the tile-local R of every record whose end lies in the tile
//   k_chunk_scan  the tiles' bases
//   k_rec_rank    R_i = tile base + local rank, parked in out_off[i + 1] (bits 0..55; bits 56..63: the replaced byte, in place)
//   (the plain scan of the staged copy)
//   k_rec_count   '\n' per output tile;  k_chunk_scan;  k_rec_part on the ranks
//   k_rec_locate  out_off[i + 1] = position of output newline R_i, + 1
//   k_rec_restore (in place, TRRE_E_CAPACITY) the replaced bytes back into the caller's buffer
// Tiles are TILE bytes of the 16-byte aligned v-space (v = position + vbeg, vbeg = the buffer's address mod 16).  A tile's
// bytes are held as one 16-bit '\n' mask per 16-byte vector in LDS; a thread owns VECS consecutive vectors for the ranks, and
// a workgroup-wide exclusive scan of the threads' counts gives every position its rank in the tile.
//
// Written once as TRRE_HD functions: scan_kernels.hip instantiates them for the device, tests/records_shim.cpp runs them on the
// host thread by thread (barriers are loop boundaries) against numpy.
#pragma once
#include <cstdint>

#include "scan_block.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define TRRE_REC_LDS_OR(p, v) atomicOr((p), (v))
#else
#define TRRE_REC_LDS_OR(p, v) (*(p) |= (v))
#endif

namespace trre {

constexpr int kRecThreads = 256;
constexpr int kRecVecs = 16;                          // 16-byte vectors per thread: 64 KiB tiles
constexpr uint64_t kRecRankMask = (1ull << 56) - 1;   // a rank; bits 56..63 hold the byte the staged copy replaced

template <int THREADS_, int VECS_>
struct RecGeo {
    static constexpr int THREADS = THREADS_;
    static constexpr int VECS = VECS_;
    static constexpr int64_t TILE = (int64_t)THREADS_ * VECS_ * 16;
    static constexpr int NVEC = THREADS_ * VECS_;     // 16-bit masks in LDS
};
using RecGeoDev = RecGeo<kRecThreads, kRecVecs>;

struct RecArgs {
    const uint8_t* in_v0;   // the buffer the tiles are over (input; output for k_rec_count / k_rec_locate) - vbeg, 16-byte aligned
    uint8_t* snap_v0;       // the staged copy, same geometry as the input
    int64_t vbeg, vend;     // valid bytes: v in [vbeg, vend)
    const int64_t* off;     // [nrec + 1] the caller's record offsets
    int64_t nrec;
    int64_t* out_off;       // [nrec + 1] ranks, then output offsets
    int64_t* part;          // [tiles + 1] first record of each tile
    uint64_t* cnt;          // [tiles] '\n' per tile
    const uint64_t* base;   // [tiles + 1] exclusive scan of cnt
    uint32_t keep;          // in place: park the replaced byte in bits 56..63 of the rank (k_rec_restore)
};

TRRE_HD uint32_t rec_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// bad offsets: off[0] != 0, off[nrec] != n, off[i] > off[i + 1]; k in [0, nrec]
TRRE_HD uint32_t rec_check(const int64_t* off, int64_t nrec, int64_t n, int64_t k) {
    uint32_t bad = 0;
    if (k == 0 && off[0] != 0) bad = 1;
    if (k == nrec && off[nrec] != n) bad = 1;
    if (k < nrec && off[k] > off[k + 1]) bad = 1;
    return bad;
}

// first k in [0, n) with key(k) >= x, n when there is none (keys do not decrease)
template <class Key>
TRRE_HD int64_t rec_lower_bound(const Key& key, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key(mid) < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
struct RecEndKey {   // record i's end offset
    const int64_t* off;
    TRRE_HD int64_t operator()(int64_t i) const { return off[i + 1]; }
};
struct RecRankKey {  // record i's rank
    const int64_t* out_off;
    TRRE_HD int64_t operator()(int64_t i) const { return (int64_t)((uint64_t)out_off[i + 1] & kRecRankMask); }
};

// the tile that holds the end of a record ending at offset p (its last byte; p == 0: tile 0)
TRRE_HD int64_t rec_end_tile(int64_t p, int64_t vbeg, int64_t tile) { return p == 0 ? 0 : (p - 1 + vbeg) / tile; }

// k_rec_part, input side: part[b] = the first record whose end lies in tile b or after it (b in [0, tiles])
TRRE_HD void rec_part_in(const RecArgs& a, int64_t tile, int64_t b) {
    a.part[b] = b == 0 ? 0 : rec_lower_bound(RecEndKey{a.off}, a.nrec, b * tile - a.vbeg + 1);
}
// ... output side: the first record whose newline lies in tile b or after it (rank > base[b])
TRRE_HD void rec_part_out(const RecArgs& a, int64_t b) {
    a.part[b] = b == 0 ? 0 : rec_lower_bound(RecRankKey{a.out_off}, a.nrec, (int64_t)a.base[b] + 1);
}

// 16 bytes from v-space position v (16-byte aligned): non-temporal on the device (each byte is read once)
TRRE_HD U128 rec_load16(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const U128* s = reinterpret_cast<const U128*>(p);
    U128 w;
    w.x = __builtin_nontemporal_load(&s->x); w.y = __builtin_nontemporal_load(&s->y);
    w.z = __builtin_nontemporal_load(&s->z); w.w = __builtin_nontemporal_load(&s->w);
    return w;
#else
    return *reinterpret_cast<const U128*>(p);
#endif
}

TRRE_HD void rec_store16(uint8_t* p, const U128& w) {
    U128* d = reinterpret_cast<U128*>(p);
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_nontemporal_store(w.x, &d->x); __builtin_nontemporal_store(w.y, &d->y);
    __builtin_nontemporal_store(w.z, &d->z); __builtin_nontemporal_store(w.w, &d->w);
#else
    *d = w;
#endif
}

// 4-bit mask of the bytes of w that are '\n' (SWAR zero-byte test of w ^ 0x0a0a0a0a, exact: no carry crosses a byte)
TRRE_HD uint32_t rec_nl4(uint32_t w) {
    const uint32_t x = w ^ 0x0a0a0a0au;
    const uint32_t z = ~((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x)) & 0x80808080u;
    return (((z >> 7) * 0x00204081u) >> 21) & 0xfu;
}
TRRE_HD uint32_t rec_nl16(const U128& w) { return rec_nl4(w.x) | rec_nl4(w.y) << 4 | rec_nl4(w.z) << 8 | rec_nl4(w.w) << 12; }
// the bytes of the vector at v that lie in [vbeg, vend), as a 16-bit mask
TRRE_HD uint32_t rec_valid16(int64_t v, int64_t vbeg, int64_t vend) {
    uint32_t m = 0xffffu;
    if (v < vbeg) m &= 0xffffu << (uint32_t)(vbeg - v);
    if (vend - v < 16) m &= (1u << (uint32_t)(vend - v)) - 1u;
    return m;
}
// the bytes of w named by the 4-bit mask m become '\n'
TRRE_HD uint32_t rec_put_nl4(uint32_t w, uint32_t m) {
    const uint32_t e = ((m * 0x00204081u) & 0x01010101u) * 0xffu;
    return (w & ~e) | (0x0a0a0a0au & e);
}

// k_rec_stage, before the marks: the thread's vectors of tile b (vector q = j * THREADS + tid: coalesced), asked for at once
template <class G>
TRRE_HD void rec_load_vecs(const RecArgs& a, int64_t b, int tid, U128 (&w)[G::VECS]) {
    for (int j = 0; j < G::VECS; ++j) {
        const int64_t v = b * G::TILE + 16 * ((int64_t)j * G::THREADS + tid);
        if (v < a.vend) w[j] = rec_load16(a.in_v0 + v);
    }
}
// ... the marks: a bit per record end in the tile (bits32: TILE / 32 words, zeroed before)
template <class G>
TRRE_HD void rec_mark(const RecArgs& a, int64_t b, int tid, uint32_t* bits32) {
    const int64_t i1 = a.part[b + 1];
    for (int64_t i = a.part[b] + tid; i < i1; i += G::THREADS) {
        const int64_t p = a.off[i + 1];
        if (p > a.off[i]) {
            const int64_t x = p - 1 + a.vbeg - b * G::TILE;
            TRRE_REC_LDS_OR(bits32 + (x >> 5), 1u << (uint32_t)(x & 31));
        }
    }
}
// ... the staged vectors out, and in place of each vector's marks its '\n' mask (valid bytes only); returns the thread's count
template <class G>
TRRE_HD uint32_t rec_stage_vecs(const RecArgs& a, int64_t b, int tid, U128 (&w)[G::VECS], uint16_t* bits16) {
    uint32_t c = 0;
    for (int j = 0; j < G::VECS; ++j) {
        const int q = j * G::THREADS + tid;
        const int64_t v = b * G::TILE + 16 * (int64_t)q;
        if (v >= a.vend) { bits16[q] = 0; continue; }
        const uint32_t mk = bits16[q];
        U128 r = w[j];
        if (mk) {
            r.x = rec_put_nl4(r.x, mk & 15u); r.y = rec_put_nl4(r.y, (mk >> 4) & 15u);
            r.z = rec_put_nl4(r.z, (mk >> 8) & 15u); r.w = rec_put_nl4(r.w, mk >> 12);
        }
        rec_store16(a.snap_v0 + v, r);
        const uint32_t nl = rec_nl16(r) & rec_valid16(v, a.vbeg, a.vend);
        bits16[q] = (uint16_t)nl;
        c += rec_popc(nl);
    }
    return c;
}
// k_rec_count / k_rec_locate: the '\n' masks of the thread's vectors of an output tile (bits16 may be null: count only)
template <class G>
TRRE_HD uint32_t rec_count_vecs(const RecArgs& a, int64_t b, int tid, uint16_t* bits16) {
    U128 w[G::VECS];
    for (int j = 0; j < G::VECS; ++j) {
        const int64_t v = b * G::TILE + 16 * ((int64_t)j * G::THREADS + tid);
        if (v < a.vend) w[j] = rec_load16(a.in_v0 + v);
    }
    uint32_t c = 0;
    for (int j = 0; j < G::VECS; ++j) {
        const int q = j * G::THREADS + tid;
        const int64_t v = b * G::TILE + 16 * (int64_t)q;
        const uint32_t nl = v < a.vend ? rec_nl16(w[j]) & rec_valid16(v, a.vbeg, a.vend) : 0u;
        if (bits16) bits16[q] = (uint16_t)nl;
        c += rec_popc(nl);
    }
    return c;
}
// '\n' in the thread's rank segment: vectors [tid * VECS, tid * VECS + VECS)
template <class G>
TRRE_HD uint32_t rec_seg_count(const uint16_t* bits16, int tid) {
    uint32_t c = 0;
    for (int k = 0; k < G::VECS; ++k) c += rec_popc(bits16[tid * G::VECS + k]);
    return c;
}
// '\n' of the tile at byte indices <= x (pre: the segments' exclusive prefix)
template <class G>
TRRE_HD uint32_t rec_rank_at(const uint16_t* bits16, const uint32_t* pre, int64_t x) {
    const int q = (int)(x >> 4), t = q / G::VECS;
    uint32_t r = pre[t];
    for (int k = t * G::VECS; k < q; ++k) r += rec_popc(bits16[k]);
    return r + rec_popc(bits16[q] & ((2u << (uint32_t)(x & 15)) - 1u));
}
// k_rec_stage, last: the tile-local rank of every record whose end lies in tile b, into out_off[i + 1]
template <class G>
TRRE_HD void rec_rank_records(const RecArgs& a, int64_t b, int tid, const uint16_t* bits16, const uint32_t* pre) {
    const int64_t i1 = a.part[b + 1];
    for (int64_t i = a.part[b] + tid; i < i1; i += G::THREADS) {
        const int64_t p = a.off[i + 1];
        uint64_t r = 0;
        if (p > 0) {
            const int64_t x = p - 1 + a.vbeg - b * G::TILE;
            r = rec_rank_at<G>(bits16, pre, x);
            if (a.keep && p > a.off[i]) r |= (uint64_t)a.in_v0[b * G::TILE + x] << 56;
        }
        a.out_off[i + 1] = (int64_t)r;
    }
}
// k_rec_rank: the tile's base onto record i's local rank
TRRE_HD void rec_add_base(const RecArgs& a, int64_t tile, int64_t i) {
    a.out_off[i + 1] = (int64_t)((uint64_t)a.out_off[i + 1] + a.base[rec_end_tile(a.off[i + 1], a.vbeg, tile)]);
}
// byte index in the tile of its r-th '\n' (1-based; r <= the tile's count)
template <class G>
TRRE_HD int64_t rec_select(const uint16_t* bits16, const uint32_t* pre, uint32_t r) {
    int lo = 0, hi = G::THREADS - 1;                     // the last segment whose prefix is below r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] < r) lo = mid;
        else hi = mid - 1;
    }
    r -= pre[lo];
    int q = lo * G::VECS;
    for (int k = 0; k < G::VECS; ++k, ++q) {
        const uint32_t c = rec_popc(bits16[q]);
        if (r <= c) break;
        r -= c;
    }
    uint32_t m = bits16[q];
    for (; r > 1; --r) m &= m - 1u;
    return 16 * (int64_t)q + __builtin_ctz(m);
}
// k_rec_locate: out_off[i + 1] for the records whose newline lies in output tile b (total: the tile's '\n'); returns 1 when a
// rank falls outside the tile (the staging identity broken: an internal error)
template <class G>
TRRE_HD uint32_t rec_locate_records(const RecArgs& a, int64_t b, int tid, const uint16_t* bits16, const uint32_t* pre, uint32_t total) {
    uint32_t bad = 0;
    if (b == 0 && tid == 0) a.out_off[0] = 0;
    const int64_t i1 = a.part[b + 1];
    for (int64_t i = a.part[b] + tid; i < i1; i += G::THREADS) {
        const uint64_t rk = (uint64_t)a.out_off[i + 1] & kRecRankMask;
        if (rk <= a.base[0]) { a.out_off[i + 1] = 0; continue; }       // no newline up to the record's end (base[0] is 0)
        const uint64_t r = rk - a.base[b];
        if (rk <= a.base[b] || r > total) { bad = 1; continue; }
        a.out_off[i + 1] = b * G::TILE + rec_select<G>(bits16, pre, (uint32_t)r) - a.vbeg + 1;
    }
    return bad;
}
// k_rec_restore: record i's replaced byte back (dst: the caller's buffer, which holds the staged copy again)
TRRE_HD void rec_restore(const RecArgs& a, uint8_t* dst, int64_t i) {
    const int64_t p = a.off[i + 1];
    if (p > a.off[i]) dst[p - 1] = (uint8_t)((uint64_t)a.out_off[i + 1] >> 56);
}

// ---- packed strings (trre_scan_device_strings) ----------------------------------------------------------------------------
// Record i is the content of ONE line with its line end left off: out_i = R(rec_i + '\n') minus the framing '\n' that closes
// it.  The STAGED text holds in[off[i] .. off[i+1]) at off[i] + i and a '\n' at key(i) = off[i+1] + i; it is n + nrec bytes,
// key is strictly increasing, and the plain scan of it is the concatenation of the records' framed outputs.  Record i's framed
// output ends just past output newline number
//     R_i = number of '\n' in staged[0, key(i)] = (number of '\n' in in[0, off[i+1])) + i + 1
// and the byte at framed position t of record i goes to t - i, its closing '\n' nowhere.  The passes:
//   k_rec_check     the offsets (as above)
//   k_str_part(0)   the first record of every staged tile: the first i with key(i) >= b * TILE
//   k_str_stage     an expansion: input range of the tile -> LDS -> whole staged vectors; the tile's '\n'; the tile-local R_i
//   k_chunk_scan, k_str_rank   R_i = tile base + local rank, in out_off[i + 1]
//   (the plain scan of the staged text into the context's framed buffer)
//   k_rec_count, k_chunk_scan, k_rec_part(1), k_rec_locate   out_off[i + 1] = position just past framed newline R_i (as above)
//   k_str_part(1)   the first record of every framed tile: the first i with out_off[i + 1] - 1 >= b * TILE
//   k_str_unframe   a compaction: framed tile -> LDS -> d_out (output-parallel); the tile that holds record i's closing '\n'
//                   is the only reader of out_off[i + 1] in this pass and writes its final value, out_off[i + 1] - (i + 1)
// Both buffers the tiles are over (staged, framed) are the context's, 16-byte aligned, with whole vectors behind the end.  A tile
// keeps its BYTES in LDS (TILE + 32), a bit per byte for the record ends in it, the ends before every vector (pv) and, for the
// compaction, the source vector each destination vector starts in (inv): about 25 KiB for the device's 16 KiB tiles.
constexpr int kStrVecs = 4;                           // 16-byte vectors per thread: 16 KiB tiles
using StrGeoDev = RecGeo<kRecThreads, kStrVecs>;

struct StrArgs {
    const uint8_t* src_v0;  // stage: the caller's input - vbeg (16-byte aligned); unframe: the framed output (aligned)
    int64_t vbeg;           // stage: the input's address mod 16
    int64_t total;          // bytes of the space the tiles are over: n + nrec (staged) / the framed length
    uint8_t* dst;           // stage: the staged text (aligned); unframe: the caller's d_out (any alignment)
    int64_t dst_len;        // unframe: framed length - nrec; nothing is stored at or behind it
    const int64_t* off;     // [nrec + 1] the caller's offsets (stage)
    int64_t nrec;
    int64_t* out_off;       // [nrec + 1] ranks, located positions, then the output offsets
    const int64_t* part;    // [tiles + 1] first record of each tile
    uint64_t* cnt;          // [tiles] '\n' per staged tile
    const uint64_t* base;   // [tiles + 1] exclusive scan of cnt
};

struct StrStageKey {   // staged position of record i's closing '\n'
    const int64_t* off;
    TRRE_HD int64_t operator()(int64_t i) const { return off[i + 1] + i; }
};
struct StrFramedKey {  // framed position of record i's closing '\n'
    const int64_t* out_off;
    TRRE_HD int64_t operator()(int64_t i) const { return out_off[i + 1] - 1; }
};
// k_str_part: part[b] = the first record whose closing '\n' lies in tile b or after it (b in [0, tiles])
TRRE_HD void str_part(const StrArgs& a, int64_t* part, int64_t tile, int side, int64_t b) {
    part[b] = side == 0 ? rec_lower_bound(StrStageKey{a.off}, a.nrec, b * tile) : rec_lower_bound(StrFramedKey{a.out_off}, a.nrec, b * tile);
}

// 16 bytes from byte index s of an LDS image of whole vectors: two aligned vectors, funnel-shifted (the vector behind is
// read even when s is aligned: the image has one to spare)
TRRE_HD U128 str_funnel16(const U128* lds, int64_t s) {
    const U128 lo = lds[s >> 4], hi = lds[(s >> 4) + 1];
    uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t sh = (uint32_t)s & 15u;
    if (sh & 8u) { w[0] = w[2]; w[1] = w[3]; w[2] = w[4]; w[3] = w[5]; w[4] = w[6]; w[5] = w[7]; }
    if (sh & 4u) { w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = w[4]; w[4] = w[5]; }
    const uint32_t bs = (sh & 3u) * 8u;
    U128 r;
    r.x = (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> bs); r.y = (uint32_t)((((uint64_t)w[2] << 32) | w[1]) >> bs);
    r.z = (uint32_t)((((uint64_t)w[3] << 32) | w[2]) >> bs); r.w = (uint32_t)((((uint64_t)w[4] << 32) | w[3]) >> bs);
    return r;
}
TRRE_HD void str_put_byte(U128& r, int k, uint32_t c) {
    uint32_t& w = k < 4 ? r.x : k < 8 ? r.y : k < 12 ? r.z : r.w;
    w |= c << (8u * (uint32_t)(k & 3));
}

// the tile's source: stage — the input range [s0 - i0, s1 - i1) as whole vectors of the input's v-space, `shift` bytes in
// front; unframe — the framed tile itself
template <class G>
struct StrTile {
    int64_t s0, s1;      // the tile in its space
    int64_t i0, i1;      // records whose closing '\n' lies in it
    int64_t v0, vend;    // source vectors from v0 (16-byte aligned), loaded while below vend
    int shift;           // LDS byte index of the tile's first source byte
    TRRE_HD StrTile(const StrArgs& a, int64_t b, bool stage) {
        s0 = b * G::TILE;
        s1 = s0 + G::TILE < a.total ? s0 + G::TILE : a.total;
        i0 = a.part[b]; i1 = a.part[b + 1];
        if (stage) {
            const int64_t p = s0 - i0 + a.vbeg;
            v0 = p & ~(int64_t)15; shift = (int)(p & 15); vend = s1 - i1 + a.vbeg;
        } else {
            v0 = s0; shift = 0; vend = s1;
        }
    }
};
// the thread's source vectors (vector k = j * THREADS + tid: coalesced; thread 0 takes the one more that a shift needs)
template <class G>
TRRE_HD void str_load_vecs(const StrArgs& a, const StrTile<G>& t, int tid, U128 (&w)[G::VECS + 1]) {
    for (int j = 0; j <= G::VECS; ++j) {
        const int k = j * G::THREADS + tid;
        if (j == G::VECS && tid != 0) break;
        const int64_t v = t.v0 + 16 * (int64_t)k;
        if (v < t.vend) w[j] = rec_load16(a.src_v0 + v);
    }
}
template <class G>
TRRE_HD void str_keep_vecs(const StrTile<G>& t, int tid, const U128 (&w)[G::VECS + 1], U128* lds) {
    for (int j = 0; j <= G::VECS; ++j) {
        const int k = j * G::THREADS + tid;
        if (j == G::VECS && tid != 0) break;
        if (t.v0 + 16 * (int64_t)k < t.vend) lds[k] = w[j];
    }
}
// a bit per closing '\n' of the tile (bits32: TILE / 32 words, zeroed before).  stage: from the offsets.  unframe: from the
// located positions, which the owning tile replaces by the final offsets here
template <class G>
TRRE_HD void str_mark(const StrArgs& a, const StrTile<G>& t, int tid, uint32_t* bits32, bool stage) {
    for (int64_t i = t.i0 + tid; i < t.i1; i += G::THREADS) {
        int64_t x;
        if (stage) {
            x = a.off[i + 1] + i - t.s0;
        } else {
            const int64_t e = a.out_off[i + 1];
            x = e - 1 - t.s0;
            a.out_off[i + 1] = e - (i + 1);
        }
        if (x >= 0 && x < t.s1 - t.s0) TRRE_REC_LDS_OR(bits32 + (x >> 5), 1u << (uint32_t)(x & 31));
    }
}
// marks before each of the thread's segment vectors (pre_t: before the segment); pv[NVEC] = the tile's marks
template <class G>
TRRE_HD void str_fill_pv(const uint16_t* bits16, uint32_t pre_t, int tid, uint32_t* pv) {
    uint32_t run = pre_t;
    for (int k = 0; k < G::VECS; ++k) {
        pv[tid * G::VECS + k] = run;
        run += rec_popc(bits16[tid * G::VECS + k]);
    }
    if (tid == G::THREADS - 1) pv[G::NVEC] = run;
}
// k_str_stage: the thread's staged vectors out (vector q = j * THREADS + tid), and in place of each vector's marks its '\n'
// mask (valid bytes only).  A vector without a mark is 16 consecutive source bytes.
template <class G>
TRRE_HD void str_stage_vecs(const StrArgs& a, const StrTile<G>& t, int tid, const U128* lds, uint16_t* bits16, const uint32_t* pv) {
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(lds);
    for (int j = 0; j < G::VECS; ++j) {
        const int q = j * G::THREADS + tid;
        const int64_t s = t.s0 + 16 * (int64_t)q;
        if (s >= t.s1) { bits16[q] = 0; continue; }
        const uint32_t mk = bits16[q];
        const int64_t sb = t.shift + 16 * (int64_t)q - pv[q];
        U128 r;
        if (mk == 0) {
            r = str_funnel16(lds, sb);
        } else {
            r.x = r.y = r.z = r.w = 0;
            int64_t at = sb;
            for (int k = 0; k < 16 && s + k < t.s1; ++k) str_put_byte(r, k, (mk >> k) & 1u ? (uint32_t)'\n' : bytes[at++]);
        }
        rec_store16(a.dst + s, r);
        bits16[q] = (uint16_t)(rec_nl16(r) & rec_valid16(s, 0, t.s1));
    }
}
// ... the tile-local rank of every record whose closing '\n' lies in the tile, into out_off[i + 1]
template <class G>
TRRE_HD void str_rank_records(const StrArgs& a, const StrTile<G>& t, int tid, const uint16_t* bits16, const uint32_t* pre) {
    for (int64_t i = t.i0 + tid; i < t.i1; i += G::THREADS)
        a.out_off[i + 1] = (int64_t)rec_rank_at<G>(bits16, pre, a.off[i + 1] + i - t.s0);
}
// k_str_rank: the tile's base onto record i's local rank
TRRE_HD void str_add_base(const StrArgs& a, int64_t tile, int64_t i) {
    a.out_off[i + 1] = (int64_t)((uint64_t)a.out_off[i + 1] + a.base[(a.off[i + 1] + i) / tile]);
}

// k_str_unframe.  The tile's E = (s1 - s0) - marks kept bytes go to dst + d0, d0 = s0 - i0.  Destination vectors are those of
// the ADDRESS: vector g holds kept bytes [e0(g), e1(g)), e0 = 16 g - A (0 for g = 0), A = (address of dst + d0) mod 16, so that
// every whole one is an aligned 16-byte store and the ragged first and last, which neighbours share, are byte stores.
template <class G>
struct StrOut {
    int64_t d0, E;
    int A, ng;
    TRRE_HD StrOut(const StrArgs& a, const StrTile<G>& t, uint32_t marks) {
        d0 = t.s0 - t.i0;
        E = t.s1 - t.s0 - (int64_t)marks;
        A = (int)((reinterpret_cast<uintptr_t>(a.dst) + (uintptr_t)d0) & 15u);
        ng = E ? (int)((E + A + 15) >> 4) : 0;
    }
    TRRE_HD int64_t e0(int g) const { return g ? 16 * (int64_t)g - A : 0; }
};
// inv[g] = the source vector that holds kept byte e0(g): source vector q holds kept bytes [lo, hi), at most one e0 of each kind
template <class G>
TRRE_HD void str_fill_inv(const StrTile<G>& t, const StrOut<G>& o, int tid, const uint16_t* bits16, const uint32_t* pv, uint16_t* inv) {
    for (int j = 0; j < G::VECS; ++j) {
        const int q = j * G::THREADS + tid;
        const int64_t left = t.s1 - t.s0 - 16 * (int64_t)q;
        if (left <= 0) continue;
        const int64_t lo = 16 * (int64_t)q - pv[q];
        const int64_t hi = lo + (left < 16 ? left : 16) - rec_popc(bits16[q]);
        if (hi <= lo) continue;
        if (lo == 0) inv[0] = (uint16_t)q;
        const int64_t g = (lo + o.A + 15) >> 4, e = 16 * g - o.A;
        if (g >= 1 && e < hi) inv[g] = (uint16_t)q;
    }
}
template <class G>
TRRE_HD void str_unframe_vecs(const StrArgs& a, const StrTile<G>& t, const StrOut<G>& o, int tid, const U128* lds, const uint16_t* bits16,
                              const uint32_t* pv, const uint16_t* inv) {
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(lds);
    for (int g = tid; g < o.ng; g += G::THREADS) {
        const int64_t e0 = o.e0(g);
        const int64_t e1 = 16 * (int64_t)g - o.A + 16 < o.E ? 16 * (int64_t)g - o.A + 16 : o.E;
        if (o.d0 + e1 > a.dst_len) continue;                               // (never: the offsets were checked end to end before)
        const int q = inv[g];
        uint32_t um = ~(uint32_t)bits16[q] & 0xffffu;                      // kept bytes of the source vector
        for (int64_t r = e0 - (16 * (int64_t)q - pv[q]); r > 0; --r) um &= um - 1u;
        const int px = __builtin_ctz(um | 0x10000u);
        int64_t x = 16 * (int64_t)q + px;
        uint8_t* d = a.dst + o.d0 + e0;
        const bool whole = e1 - e0 == 16;
        const uint32_t ahead = ((uint32_t)bits16[q] | (q + 1 < G::NVEC ? (uint32_t)bits16[q + 1] << 16 : 0u)) >> px;
        if (whole && (ahead & 0xffffu) == 0) {
            rec_store16(d, str_funnel16(lds, x));
        } else if (whole) {
            U128 r;
            r.x = r.y = r.z = r.w = 0;
            for (int k = 0; k < 16; ++k) {
                while ((bits16[x >> 4] >> (x & 15)) & 1u) ++x;
                str_put_byte(r, k, bytes[x++]);
            }
            rec_store16(d, r);
        } else {
            for (int64_t e = e0; e < e1; ++e) {
                while ((bits16[x >> 4] >> (x & 15)) & 1u) ++x;
                *d++ = bytes[x++];
            }
        }
    }
}

// ---- matched strings (trre_match_device_strings) ---------------------------------------------------------------------------
// A match-mode program accepts a string or rejects it: valid[i], and out_i = M(rec_i + '\n') minus the framing '\n' (empty when
// rejected).  The staged text is the strings call's; no string holds a '\n' (the staged newline total is nrec exactly then) and
// the program prints none of its own, so every '\n' of the framed output closes exactly one ACCEPTED string, in order.  With
//     M_i = number of accepted strings among 0 .. i
// string i's framed output ends just past framed newline number M_i (position 0 when M_i is 0), its final offset is that
// position minus M_i, and the output bytes are the framed output with every '\n' dropped.  Whether string i is accepted is what
// the forward root cell decides at the column of the backward pass's symbol at the string's first staged byte,
// s_i = off[i] + i (its '\n' when the string is empty): accept[symbol] (guided_build.cpp: fill_accept).  The passes:
//   k_rec_check, k_str_part(0), k_str_stage, k_chunk_scan   as for the strings call; the staged newline total
//   (the plain match scan of the staged text into the framed buffer; a guided family: the symbols are in the context)
//   k_match_verdict   64 strings per wave: the bitmap word (one ballot), the rank inside the group of THREADS strings in
//                     out_off[i + 1], the group's count
//   k_chunk_scan, k_match_rank   M_i = group base + local rank, in out_off[i + 1]; the grand total is n_matched
//   k_rec_count, k_chunk_scan, k_rec_part(1), k_rec_locate   out_off[i + 1] = position just past framed newline M_i (as above)
//   k_match_final     out_off[i + 1] -= M_i, M_i again from the group bases and the bitmap words
//   k_match_count, k_chunk_scan   '\n' per framed tile of the compaction and before it
//   k_match_unframe   k_str_unframe's compaction with the marks taken from the bytes: every '\n' goes
constexpr int kMatchThreads = 256;                    // strings per group: four bitmap words

struct MatchArgs {
    const uint8_t* sym_v0;    // the backward pass's symbols of the staged text, in the scan's v-space
    int64_t vbeg;             // the staged text's address mod 16
    const int64_t* off;       // [nrec + 1] the caller's offsets
    int64_t nrec;
    const uint32_t* accept;   // a bit per backward state
    uint32_t accept_words;
    uint64_t* valid;          // [words] the bitmap
    int64_t words;            // ceil(nrec / 64)
    int64_t* out_off;         // [nrec + 1] local ranks, M_i, located positions, then the output offsets
    uint64_t* cnt;            // [groups] accepted strings per group
    const uint64_t* base;     // [groups + 1] exclusive scan of cnt
};

// the symbol at v: kBits 4 two per byte, 8 one per byte (rev_symbol_at), 16 two bytes each
template <int kBits>
TRRE_HD uint32_t match_symbol_at(const uint8_t* sym_v0, int64_t v) {
    if (kBits == 16) return reinterpret_cast<const uint16_t*>(sym_v0)[v];
    ScanArgs s{};
    s.sym_v0 = const_cast<uint8_t*>(sym_v0);
    return rev_symbol_at<kBits == 4>(s, v);
}
// k_match_verdict, one lane: is string i accepted (acc: the accept bits, in LDS on the device)
template <int kBits>
TRRE_HD bool match_verdict(const MatchArgs& a, const uint32_t* acc, int64_t i) {
    const uint32_t y = match_symbol_at<kBits>(a.sym_v0, a.off[i] + i + a.vbeg);
    return y < 32u * a.accept_words && ((acc[y >> 5] >> (y & 31u)) & 1u) != 0;
}
TRRE_HD uint32_t match_popc64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
// ... the lane's inclusive rank inside its wave's word
TRRE_HD uint32_t match_lane_rank(uint64_t word, int lane) { return match_popc64(word & (~0ull >> (63 - lane))); }
// ... what the group's lane `tid` leaves: its rank in the group (below: the accepted strings of the waves before its own)
TRRE_HD void match_park(const MatchArgs& a, int64_t i, uint32_t below, uint64_t word, int lane) {
    if (i < a.nrec) a.out_off[i + 1] = (int64_t)(below + match_lane_rank(word, lane));
}
// k_match_rank: the group's base onto string i's local rank
TRRE_HD void match_add_base(const MatchArgs& a, int64_t i) {
    a.out_off[i + 1] = (int64_t)((uint64_t)a.out_off[i + 1] + a.base[i / kMatchThreads]);
}
// M_i from the group bases and the bitmap words
TRRE_HD uint64_t match_rank_of(const MatchArgs& a, int64_t i) {
    const int64_t w = i >> 6;
    uint64_t r = a.base[i / kMatchThreads];
    for (int64_t k = (i / kMatchThreads) * (kMatchThreads / 64); k < w; ++k) r += match_popc64(a.valid[k]);
    return r + match_lane_rank(a.valid[w], (int)(i & 63));
}
// k_match_final: the located position minus the framing newlines before it
TRRE_HD void match_final(const MatchArgs& a, int64_t i) {
    a.out_off[i + 1] = (int64_t)((uint64_t)a.out_off[i + 1] - match_rank_of(a, i));
}
// k_match_unframe: the marks of the thread's vectors from their bytes — every '\n' of the framed tile (vector k of the image is
// vector k of the tile: the compaction's source has no shift)
template <class G>
TRRE_HD void match_mark_vecs(const StrTile<G>& t, int tid, const U128 (&w)[G::VECS + 1], uint16_t* bits16) {
    for (int j = 0; j < G::VECS; ++j) {
        const int q = j * G::THREADS + tid;
        const int64_t v = t.v0 + 16 * (int64_t)q;
        bits16[q] = v < t.vend ? (uint16_t)(rec_nl16(w[j]) & rec_valid16(v, 0, t.vend)) : (uint16_t)0;
    }
}

// ---- found strings (trre_find_device_strings) ------------------------------------------------------------------------------
// A find-mode program pulls every match out of every string: find(s) is the list of the outputs of the scan loop's successful
// attempts on the line s (trre_nft.c:775-790), the raw bytes gone.  Two scans of the strings call's staged text, under the two
// forward tables of guided_build.cpp: find_cell, give everything:
//   marks   per line one byte per match and the line's '\n': the strings call's own unframing of it leaves, as ITS output
//           offsets, the list offsets — list_off[i] = matches in strings 0 .. i - 1, list_off[nrec] = n_matches
//   texts   every match's output closed by a '\n' (the program prints none of its own): framed newline number j (0-based), at
//           framed position q, closes match j, so match_off[j + 1] = q - j, match_off[0] = 0, and the output bytes are the
//           framed text with every '\n' dropped — k_match_unframe's compaction.
// The passes behind the two scans: k_match_count, k_chunk_scan ('\n' per framed tile and before it; the total is n_matches
// again) and k_find_unframe: k_match_unframe plus the offsets.  Who writes which word: match_off[0] one thread of tile 0; every
// other word the lane that owns its newline, once.  A wave takes 64 framed bytes at a time: their marks are one 64-bit word
// (what a ballot of "my byte is a '\n'" gives, read from the tile's mark image instead), the rank of a lane's newline is the
// marks before the piece (pv, from the workgroup's scan: wave_scan_incl) plus the set bits below the lane, so the lanes of a
// wave store adjacent words for adjacent ranks — when every framed byte is a '\n' (every match empty) a wave's 64 stores are
// 512 contiguous bytes, and a tile's 16 384 offsets take 64 such rounds of its four waves.
template <class G>
TRRE_HD void find_offset_vecs(const StrArgs& a, const StrTile<G>& t, int tid, const uint16_t* bits16, const uint32_t* pv) {
    constexpr int kPieces = G::NVEC / 4, kWaves = G::THREADS / 64;
    const int lane = tid & 63;
    if (t.s0 == 0 && tid == 0) a.out_off[0] = 0;
    for (int k = tid >> 6; k < kPieces; k += kWaves) {
        const uint64_t word = (uint64_t)bits16[4 * k] | (uint64_t)bits16[4 * k + 1] << 16 | (uint64_t)bits16[4 * k + 2] << 32 |
                              (uint64_t)bits16[4 * k + 3] << 48;
        if (!((word >> lane) & 1u)) continue;
        const int64_t j = t.i0 + (int64_t)pv[4 * k] + (int64_t)match_popc64(word & ((1ull << lane) - 1ull));
        if (j < a.nrec) a.out_off[j + 1] = t.s0 + 64 * (int64_t)k + lane - j;       // (never beyond: the newline total was checked before)
    }
}

// ---- match spans (trre_span_device_strings) --------------------------------------------------------------------------------
// A spans-mode program says WHERE the scan loop's successful attempts start and end.  ONE scan of the strings call's staged
// text under the forward table of guided_build.cpp: span_cell gives the framed text: per staged byte one position byte ('\n'
// for a '\n'), A = 0x01 in front of the first position byte of every match, B = 0x02 behind its last.  With A and B taken out
// the framed text is the staged text, byte for byte in length and newlines; string i's bytes sit at off[i] + i in the staged
// text.  So with a, b, l the A, B, '\n' before framed position q:
//     A number j at q      start[j] = q - a - b - l         (a = j)
//     B number j at q      end[j]   = q - a - b - l         (b = j, a = j + 1)
//     '\n' number i at q   list_off[i + 1] = a              (l = i)
// positions in the caller's d_in, absolute.  The passes:
//   k_span_count  A, B, '\n' per framed tile: cnt[3][tiles];  k_chunk_scan, three times: base[3][tiles + 1]; the totals are
//                 read back and checked (#A = #B, #'\n' = nrec, framed length = staged length + 2 #A) before anything is stored
//   k_span_emit   the tile's marks (a bit per byte and kind, from the thread's own vectors) into LDS; a workgroup scan of the
//                 marks per thread segment (A and B share a word: a tile holds fewer than 65 536 bytes); then a wave takes 64
//                 framed bytes at a time: the three 64-bit words of a piece are what three ballots would give, read from the
//                 mark images; a lane's ranks are tile base + marks before the piece + set bits below the lane
// Who writes which word: list_off[0] thread 0 of tile 0; every other word the lane that owns its marker byte, once; adjacent
// ranks are stored by adjacent marker lanes.  lists_only: start and end are not stored at all (TRRE_E_CAPACITY, the size query).
struct SpanArgs {
    const uint8_t* src;     // the framed text: 16-byte aligned, whole vectors readable behind its end
    int64_t total;          // framed length
    int64_t* start;         // [n_match]
    int64_t* end;           // [n_match]
    int64_t* list_off;      // [nrec + 1]
    int64_t n_match, nrec;
    int64_t tiles;
    uint64_t* cnt;          // [3][tiles] A, B, '\n' per tile
    const uint64_t* base;   // [3][tiles + 1] their exclusive scans
    uint32_t lists_only;
};
constexpr uint32_t kSpanA4 = 0x01010101u, kSpanB4 = 0x02020202u, kSpanNl4 = 0x0a0a0a0au;

// 4-bit mask of the bytes of w equal to the byte c4 repeats (rec_nl4's exact zero-byte test)
TRRE_HD uint32_t span_eq4(uint32_t w, uint32_t c4) {
    const uint32_t x = w ^ c4;
    const uint32_t z = ~((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x)) & 0x80808080u;
    return (((z >> 7) * 0x00204081u) >> 21) & 0xfu;
}
TRRE_HD uint32_t span_eq16(const U128& w, uint32_t c4) {
    return span_eq4(w.x, c4) | span_eq4(w.y, c4) << 4 | span_eq4(w.z, c4) << 8 | span_eq4(w.w, c4) << 12;
}
// the marks of the thread's vectors of tile b (vector q = j * THREADS + tid: coalesced), valid bytes only; c[0..2] += the
// thread's A, B, '\n'.  bits: [3][NVEC] 16-bit masks, or null (k_span_count)
template <class G>
TRRE_HD void span_mark_vecs(const SpanArgs& a, int64_t b, int tid, uint16_t* bits, uint32_t (&c)[3]) {
    U128 w[G::VECS];
    for (int j = 0; j < G::VECS; ++j) {
        const int64_t v = b * G::TILE + 16 * ((int64_t)j * G::THREADS + tid);
        if (v < a.total) w[j] = rec_load16(a.src + v);
    }
    for (int j = 0; j < G::VECS; ++j) {
        const int q = j * G::THREADS + tid;
        const int64_t v = b * G::TILE + 16 * (int64_t)q;
        uint32_t m[3] = {0u, 0u, 0u};
        if (v < a.total) {
            const uint32_t ok = rec_valid16(v, 0, a.total);
            m[0] = span_eq16(w[j], kSpanA4) & ok; m[1] = span_eq16(w[j], kSpanB4) & ok; m[2] = span_eq16(w[j], kSpanNl4) & ok;
        }
        for (int x = 0; x < 3; ++x) {
            if (bits) bits[x * G::NVEC + q] = (uint16_t)m[x];
            c[x] += rec_popc(m[x]);
        }
    }
}
// marks in the thread's rank segment, vectors [tid * VECS, tid * VECS + VECS): A | B << 16, and '\n'
template <class G>
TRRE_HD void span_seg_count(const uint16_t* bits, int tid, uint32_t& ab, uint32_t& nl) {
    static_assert(G::TILE < 65536, "A and B counts of a tile share a 32-bit word");
    ab = nl = 0;
    for (int k = 0; k < G::VECS; ++k) {
        const int q = tid * G::VECS + k;
        ab += rec_popc(bits[q]) | rec_popc(bits[G::NVEC + q]) << 16;
        nl += rec_popc(bits[2 * G::NVEC + q]);
    }
}
// marks before each of the thread's segment vectors (pre_ab, pre_nl: before the segment)
template <class G>
TRRE_HD void span_fill_pv(const uint16_t* bits, uint32_t pre_ab, uint32_t pre_nl, int tid, uint32_t* pv_ab, uint32_t* pv_nl) {
    for (int k = 0; k < G::VECS; ++k) {
        const int q = tid * G::VECS + k;
        pv_ab[q] = pre_ab; pv_nl[q] = pre_nl;
        pre_ab += rec_popc(bits[q]) | rec_popc(bits[G::NVEC + q]) << 16;
        pre_nl += rec_popc(bits[2 * G::NVEC + q]);
    }
}
TRRE_HD uint64_t span_word(const uint16_t* bits16, int k) {
    return (uint64_t)bits16[4 * k] | (uint64_t)bits16[4 * k + 1] << 16 | (uint64_t)bits16[4 * k + 2] << 32 | (uint64_t)bits16[4 * k + 3] << 48;
}
// behind the barrier that completes bits and pv: every marker lane of the tile gets f(kind, na, nb, nl, pos) — kind 0 an A, 1 a
// B, 2 a '\n'; na, nb, nl the A, B, '\n' of the whole framed text before the lane's byte; pos its position in the caller's d_in
template <class G, class F>
TRRE_HD void span_each_marker(const SpanArgs& a, int64_t b, int tid, const uint16_t* bits, const uint32_t* pv_ab, const uint32_t* pv_nl, F f) {
    static_assert(G::THREADS % 64 == 0 && G::NVEC % 4 == 0, "a wave takes 64-byte pieces of the tile");
    constexpr int kPieces = G::NVEC / 4, kWaves = G::THREADS / 64;
    const int lane = tid & 63;
    const int64_t s0 = b * G::TILE;
    const int64_t a0 = (int64_t)a.base[b], b0 = (int64_t)a.base[a.tiles + 1 + b], l0 = (int64_t)a.base[2 * (a.tiles + 1) + b];
    for (int k = tid >> 6; k < kPieces; k += kWaves) {
        const uint64_t wa = span_word(bits, k), wb = span_word(bits + G::NVEC, k), wl = span_word(bits + 2 * G::NVEC, k);
        if (!(((wa | wb | wl) >> lane) & 1u)) continue;
        const uint64_t below = (1ull << lane) - 1ull;
        const int64_t na = a0 + (int64_t)(pv_ab[4 * k] & 0xffffu) + (int64_t)match_popc64(wa & below);
        const int64_t nb = b0 + (int64_t)(pv_ab[4 * k] >> 16) + (int64_t)match_popc64(wb & below);
        const int64_t nl = l0 + (int64_t)pv_nl[4 * k] + (int64_t)match_popc64(wl & below);
        const int64_t pos = s0 + 64 * (int64_t)k + lane - na - nb - nl;
        f((wa >> lane) & 1u ? 0 : (wb >> lane) & 1u ? 1 : 2, na, nb, nl, pos);
    }
}
// k_span_emit: the words of the tile's markers
template <class G>
TRRE_HD void span_emit_pieces(const SpanArgs& a, int64_t b, int tid, const uint16_t* bits, const uint32_t* pv_ab, const uint32_t* pv_nl) {
    if (b == 0 && tid == 0) a.list_off[0] = 0;
    span_each_marker<G>(a, b, tid, bits, pv_ab, pv_nl, [&](int kind, int64_t na, int64_t nb, int64_t nl, int64_t pos) {
        // (never beyond: the three totals were checked against n_match and nrec before this pass)
        if (kind == 0) {
            if (!a.lists_only && na < a.n_match) a.start[na] = pos;
        } else if (kind == 1) {
            if (!a.lists_only && nb < a.n_match) a.end[nb] = pos;
        } else if (nl < a.nrec) {
            a.list_off[nl + 1] = na;
        }
    });
}

// ---- split strings (trre_split_device_strings) -----------------------------------------------------------------------------
// The pieces of a column split at every match are the bytes OUTSIDE every span, in order: a stream compaction over the framed
// text of the span call.  A and B alternate strictly, so with a, b, l the A, B, '\n' before framed position q, the DEPTH at q
// is a - b (0 or 1), the parity of a + b; a position byte is KEPT exactly when its depth is 0; a '\n' is always at depth 0 and
// is never kept; a tile, or a 64-byte piece of one, may lie wholly inside one match and hold no marker at all.  With kp the
// kept bytes before q:
//     kept byte at q       out[kp] = in[q - a - b - l]
//     B number j at q      piece_off[j + 1 + l] = kp           (the piece behind match j starts here)
//     '\n' number i at q   piece_off[a + i + 1] = kp,  list_off[i + 1] = a + i + 1     (i = nrec - 1: the terminator, out_len)
// piece_off[0] = list_off[0] = 0.  The passes, behind k_span_count and its three scans (base[3][tiles + 1]):
//   k_split_count  the kept bytes per framed tile: kcnt[tiles] — the tile's depth on entry is base[0][b] - base[1][b], a thread
//                  segment's that plus the markers before it in the tile (a workgroup scan);  k_chunk_scan: kbase[tiles + 1];
//                  the total is out_len, read back with the other totals
//   k_split_emit   k_span_emit's three mark images, a fourth for the kept bits and its workgroup scan; then a wave takes 64
//                  framed bytes at a time, four 64-bit words per piece
// Who writes which byte and word: entry 0 of both arrays thread 0 of tile 0; every output byte the lane that owns its kept
// position byte (adjacent kept lanes store adjacent bytes); every other word the lane that owns its B or '\n', once.  An A lane
// stores nothing.  lists_only: out and piece_off are not stored at all (TRRE_E_CAPACITY, the size query).
struct SplitArgs {
    const uint8_t* src;     // the framed text: 16-byte aligned, whole vectors readable behind its end
    int64_t total;          // framed length
    const uint8_t* in;      // the caller's d_in
    int64_t n;
    uint8_t* out;           // [out_len]
    int64_t out_len;
    int64_t* piece_off;     // [n_piece + 1]
    int64_t n_piece;
    int64_t* list_off;      // [nrec + 1]
    int64_t nrec;
    int64_t tiles;
    const uint64_t* base;   // [3][tiles + 1] A, B, '\n' before every tile (k_span_count, k_chunk_scan)
    uint64_t* kcnt;         // [tiles] kept bytes per tile
    const uint64_t* kbase;  // [tiles + 1] their exclusive scan
    uint32_t lists_only;
};

// bit k: an odd number of the 16 bits of m below bit k are set
TRRE_HD uint32_t split_odd_below16(uint32_t m) {
    m ^= m << 1; m ^= m << 2; m ^= m << 4; m ^= m << 8;
    return (m << 1) & 0xffffu;
}
// the tile's marks, as k_span_emit takes them
template <class G>
TRRE_HD void split_mark_vecs(const SplitArgs& a, int64_t b, int tid, uint16_t* bits) {
    SpanArgs sp{};
    sp.src = a.src; sp.total = a.total;
    uint32_t c[3] = {0u, 0u, 0u};
    span_mark_vecs<G>(sp, b, tid, bits, c);
}
// the kept bits of the thread's rank segment, vectors [tid * VECS, tid * VECS + VECS) (pre_ab: A | B << 16 before the segment in
// the tile); kept: [NVEC] 16-bit masks, or null (k_split_count).  Returns the segment's kept bytes
template <class G>
TRRE_HD uint32_t split_seg_kept(const SplitArgs& a, int64_t b, int tid, const uint16_t* bits, uint32_t pre_ab, uint16_t* kept) {
    uint32_t d = (uint32_t)(a.base[b] + a.base[a.tiles + 1 + b] + (pre_ab & 0xffffu) + (pre_ab >> 16)) & 1u;
    uint32_t c = 0;
    for (int k = 0; k < G::VECS; ++k) {
        const int q = tid * G::VECS + k;
        const int64_t v = b * G::TILE + 16 * (int64_t)q;
        const uint32_t mk = (uint32_t)bits[q] | bits[G::NVEC + q], nl = bits[2 * G::NVEC + q];
        const uint32_t ok = v < a.total ? rec_valid16(v, 0, a.total) : 0u;
        const uint32_t kp = ~(split_odd_below16(mk) ^ (0u - d)) & ~mk & ~nl & ok;
        if (kept) kept[q] = (uint16_t)kp;
        c += rec_popc(kp);
        d ^= rec_popc(mk) & 1u;
    }
    return c;
}
// kept bytes before each of the thread's segment vectors (pre_k: before the segment)
template <class G>
TRRE_HD void split_fill_pv(const uint16_t* kept, uint32_t pre_k, int tid, uint32_t* pv_k) {
    for (int k = 0; k < G::VECS; ++k) {
        const int q = tid * G::VECS + k;
        pv_k[q] = pre_k;
        pre_k += rec_popc(kept[q]);
    }
}
// k_split_emit, behind the barrier that completes the four images and the three pv: the tile's bytes and words
template <class G>
TRRE_HD void split_emit_pieces(const SplitArgs& a, int64_t b, int tid, const uint16_t* bits, const uint16_t* kept, const uint32_t* pv_ab,
                               const uint32_t* pv_nl, const uint32_t* pv_k) {
    static_assert(G::THREADS % 64 == 0 && G::NVEC % 4 == 0, "a wave takes 64-byte pieces of the tile");
    constexpr int kPieces = G::NVEC / 4, kWaves = G::THREADS / 64;
    const int lane = tid & 63;
    const int64_t s0 = b * G::TILE;
    const int64_t a0 = (int64_t)a.base[b], b0 = (int64_t)a.base[a.tiles + 1 + b], l0 = (int64_t)a.base[2 * (a.tiles + 1) + b];
    const int64_t k0 = (int64_t)a.kbase[b];
    if (b == 0 && tid == 0) {
        a.list_off[0] = 0;
        if (!a.lists_only) a.piece_off[0] = 0;
    }
    for (int k = tid >> 6; k < kPieces; k += kWaves) {
        const uint64_t wa = span_word(bits, k), wb = span_word(bits + G::NVEC, k), wl = span_word(bits + 2 * G::NVEC, k);
        const uint64_t wk = span_word(kept, k);
        if (!(((a.lists_only ? wl : wb | wl | wk) >> lane) & 1u)) continue;
        const uint64_t below = (1ull << lane) - 1ull;
        const int64_t na = a0 + (int64_t)(pv_ab[4 * k] & 0xffffu) + (int64_t)match_popc64(wa & below);
        const int64_t nb = b0 + (int64_t)(pv_ab[4 * k] >> 16) + (int64_t)match_popc64(wb & below);
        const int64_t nl = l0 + (int64_t)pv_nl[4 * k] + (int64_t)match_popc64(wl & below);
        const int64_t kp = k0 + (int64_t)pv_k[4 * k] + (int64_t)match_popc64(wk & below);
        // (never beyond: the four totals were checked against n, the pieces and nrec before this pass)
        if ((wk >> lane) & 1u) {
            const int64_t at = s0 + 64 * (int64_t)k + lane - na - nb - nl;
            if (kp < a.out_len && at >= 0 && at < a.n) a.out[kp] = a.in[at];
        } else if ((wb >> lane) & 1u) {
            if (nb + 1 + nl <= a.n_piece) a.piece_off[nb + 1 + nl] = kp;
        } else if (nl < a.nrec) {
            a.list_off[nl + 1] = na + nl + 1;
            if (!a.lists_only && na + nl + 1 <= a.n_piece) a.piece_off[na + nl + 1] = kp;
        }
    }
}

// ---- filtered strings (trre_filter_device_strings) -------------------------------------------------------------------------
// The strings with a match (without one: invert), whole, in order, and which rows they were: a stream compaction of whole
// strings.  The verdict is the span call's: kept(i) = (list_off[i + 1] > list_off[i]) != invert, from k_span_emit's list offsets
// in an array of the library's own.  The tiles are over the INPUT's v-space (v = position + vbeg, vbeg = d_in's address mod 16),
// so a tile's source vectors are aligned; with no byte at all (every string empty) there is still one tile.  The passes:
//   k_filter_part   part[b] = the first string whose end lies in tile b or after it (rec_part_in's partition: the empty string
//                   at position 0 belongs to tile 0)
//   k_filter_count  per tile the kept strings among those that END in it, and its kept bytes: the overlap with the tile of every
//                   kept string that ends in it, and of the one string that covers the tile's end (string part[b + 1]).  Offsets
//                   and list offsets only; the text is not read.  cnt[2][tiles];  k_chunk_scan twice: base[2][tiles + 1]; the
//                   totals are n_kept and out_len, read back and checked before anything of the caller's is stored
//   k_filter_emit   the tile's source vectors into LDS; a bit per byte that TOGGLES where a kept string starts and where it ends
//                   (XOR: the end of a kept string and the start of the next kept one fall on one position and cancel, as the
//                   two toggles of an empty kept string do); the prefix XOR of the toggles is the kept image; its workgroup scan
//                   gives every byte its rank.  The tile's kept bytes go to out[kbase[b] .. kbase[b + 1]), output-parallel: the
//                   whole 16-byte vectors of the destination ADDRESS (as k_str_unframe's StrOut) are aligned vector stores, the
//                   ragged first and last ones, which the neighbouring tiles share, byte stores.
// Strings to threads: the tile's strings [i0, i1) in THREADS consecutive runs of ceil((i1 - i0) / THREADS), so a thread's rank in
// the tile is one workgroup scan away however many strings end in the tile.  No thread loops over the bytes of a string.
// Who writes which byte and word: out_off[0] thread 0 of tile 0; rows[r] and out_off[r + 1] the thread that owns kept string r,
// in the tile the string ends in; every output byte the thread that owns its destination vector, once.
#if defined(__HIP_DEVICE_COMPILE__)
#define TRRE_REC_LDS_XOR(p, v) atomicXor((p), (v))
#else
#define TRRE_REC_LDS_XOR(p, v) (*(p) ^= (v))
#endif

struct FilterArgs {
    const uint8_t* in_v0;   // the caller's d_in - vbeg: 16-byte aligned
    int64_t vbeg, n;        // d_in's address mod 16; its bytes
    const int64_t* off;     // [nrec + 1] the caller's offsets
    const int64_t* loff;    // [nrec + 1] the span call's list offsets
    int64_t nrec;
    uint32_t invert;
    int64_t tiles;
    int64_t* part;          // [tiles + 1] first string of each tile
    uint64_t* cnt;          // [2][tiles] kept strings, kept bytes per tile
    const uint64_t* base;   // [2][tiles + 1] their exclusive scans
    uint8_t* out;           // [out_len]
    int64_t out_len;
    int64_t* out_off;       // [n_kept + 1]
    int64_t* rows;          // [n_kept]
    int64_t n_kept;
};

TRRE_HD void filter_part(const FilterArgs& a, int64_t tile, int64_t b) {
    a.part[b] = b == 0 ? 0 : rec_lower_bound(RecEndKey{a.off}, a.nrec, b * tile - a.vbeg + 1);
}
TRRE_HD bool filter_kept(const FilterArgs& a, int64_t i) { return (a.loff[i + 1] > a.loff[i]) != (a.invert != 0u); }

// tile b: the positions [t0, t1) of the input, the strings [i0, i1) that end in it, `per` of them to a thread
template <class G>
struct FilterTile {
    int64_t s0, t0, t1, i0, i1, per;
    TRRE_HD FilterTile(const FilterArgs& a, int64_t b) {
        s0 = b * G::TILE;
        t0 = s0 > a.vbeg ? s0 - a.vbeg : 0;
        t1 = s0 + G::TILE - a.vbeg < a.n ? s0 + G::TILE - a.vbeg : a.n;
        i0 = a.part[b]; i1 = a.part[b + 1];
        per = (i1 - i0 + G::THREADS - 1) / G::THREADS;
    }
    TRRE_HD int64_t lo(int tid) const { return i0 + tid * per < i1 ? i0 + tid * per : i1; }
    TRRE_HD int64_t hi(int tid) const { return lo(tid) + per < i1 ? lo(tid) + per : i1; }
};
// k_filter_count: the thread's kept strings and their bytes in the tile; thread 0 adds the string that covers the tile's end
template <class G>
TRRE_HD void filter_count_strings(const FilterArgs& a, const FilterTile<G>& t, int tid, uint64_t& rows, uint64_t& bytes) {
    rows = bytes = 0;
    const int64_t hi = t.hi(tid);
    for (int64_t i = t.lo(tid); i < hi; ++i) {
        if (!filter_kept(a, i)) continue;
        ++rows;
        const int64_t s = a.off[i] > t.t0 ? a.off[i] : t.t0, e = a.off[i + 1] < t.t1 ? a.off[i + 1] : t.t1;
        if (e > s) bytes += (uint64_t)(e - s);
    }
    if (tid == 0 && t.i1 < a.nrec && filter_kept(a, t.i1)) {
        const int64_t s = a.off[t.i1] > t.t0 ? a.off[t.i1] : t.t0;
        if (t.t1 > s) bytes += (uint64_t)(t.t1 - s);
    }
}
// k_filter_emit: the thread's source vectors of the tile (vector q = j * THREADS + tid: coalesced), asked for at once
template <class G>
TRRE_HD void filter_load_vecs(const FilterArgs& a, const FilterTile<G>& t, int tid, U128 (&w)[G::VECS]) {
    for (int j = 0; j < G::VECS; ++j) {
        const int64_t v = t.s0 + 16 * ((int64_t)j * G::THREADS + tid);
        w[j].x = w[j].y = w[j].z = w[j].w = 0;                        // (behind the input's end: zeros)
        if (v < a.vbeg + a.n) w[j] = rec_load16(a.in_v0 + v);
    }
}
// ... into the LDS image: a vector of zeros, the tile's NVEC vectors, a vector of zeros (str_funnel16 reads from up to 15 bytes in
// front of the tile and one vector behind)
template <class G>
TRRE_HD void filter_keep_vecs(int tid, const U128 (&w)[G::VECS], U128* lds) {
    for (int j = 0; j < G::VECS; ++j) lds[1 + j * G::THREADS + tid] = w[j];
    if (tid == 0) {
        U128 z;
        z.x = z.y = z.z = z.w = 0;
        lds[0] = lds[G::NVEC + 1] = z;
    }
}
TRRE_HD void filter_toggle(uint32_t* bits32, int64_t x, int64_t tile) {
    if (x >= 0 && x < tile) TRRE_REC_LDS_XOR(bits32 + (x >> 5), 1u << (uint32_t)(x & 31));
}
// ... the toggles of the thread's kept strings (bits32: TILE / 32 words, zeroed before); returns the thread's kept strings
template <class G>
TRRE_HD uint64_t filter_mark(const FilterArgs& a, const FilterTile<G>& t, int tid, uint32_t* bits32) {
    uint64_t rows = 0;
    const int64_t hi = t.hi(tid);
    for (int64_t i = t.lo(tid); i < hi; ++i) {
        if (!filter_kept(a, i)) continue;
        ++rows;
        const int64_t s = a.off[i] > t.t0 ? a.off[i] : t.t0, e = a.off[i + 1];
        if (e > s) {
            filter_toggle(bits32, s + a.vbeg - t.s0, G::TILE);
            filter_toggle(bits32, e + a.vbeg - t.s0, G::TILE);      // (an end on the tile's last byte toggles nothing: behind the image)
        }
    }
    if (tid == 0 && t.i1 < a.nrec && filter_kept(a, t.i1)) {
        const int64_t s = a.off[t.i1] > t.t0 ? a.off[t.i1] : t.t0;
        if (t.t1 > s) filter_toggle(bits32, s + a.vbeg - t.s0, G::TILE);
    }
    return rows;
}
// toggles in the thread's rank segment, vectors [tid * VECS, tid * VECS + VECS): rec_seg_count.  Then, in place of the segment's
// toggles, its kept bits (pre_t: toggles before the segment); returns the segment's kept bytes
template <class G>
TRRE_HD uint32_t filter_seg_kept(const FilterArgs& a, const FilterTile<G>& t, int tid, uint16_t* bits16, uint32_t pre_t) {
    uint32_t d = pre_t & 1u, c = 0;
    for (int k = 0; k < G::VECS; ++k) {
        const int q = tid * G::VECS + k;
        const int64_t v = t.s0 + 16 * (int64_t)q;
        const uint32_t mk = bits16[q];
        const uint32_t ok = v < a.vbeg + a.n ? rec_valid16(v, a.vbeg, a.vbeg + a.n) : 0u;
        const uint32_t kp = (split_odd_below16(mk) ^ mk ^ (0u - d)) & ok;      // an odd number of toggles at or below the byte
        bits16[q] = (uint16_t)kp;
        c += rec_popc(kp);
        d ^= rec_popc(mk) & 1u;
    }
    return c;
}
// kept bytes of the tile at byte indices < x (x in [0, TILE]; pv: str_fill_pv of the kept image)
template <class G>
TRRE_HD uint32_t filter_kept_below(const uint16_t* bits16, const uint32_t* pv, int64_t x) {
    if (x >= G::TILE) return pv[G::NVEC];
    if (x <= 0) return 0u;
    return pv[x >> 4] + rec_popc(bits16[x >> 4] & ((1u << (uint32_t)(x & 15)) - 1u));
}
// ... behind the barrier that completes the kept image and pv: rows and out_off of the thread's kept strings (r0: kept strings of
// the tile before the thread's)
template <class G>
TRRE_HD void filter_emit_rows(const FilterArgs& a, const FilterTile<G>& t, int64_t b, int tid, uint64_t r0, const uint16_t* bits16,
                              const uint32_t* pv) {
    if (b == 0 && tid == 0) a.out_off[0] = 0;
    int64_t r = (int64_t)(a.base[b] + r0);
    const int64_t k0 = (int64_t)a.base[a.tiles + 1 + b];
    const int64_t hi = t.hi(tid);
    for (int64_t i = t.lo(tid); i < hi; ++i) {
        if (!filter_kept(a, i)) continue;
        if (r < a.n_kept) {                                           // (never beyond: the totals were checked before this pass)
            a.rows[r] = i;
            a.out_off[r + 1] = k0 + (int64_t)filter_kept_below<G>(bits16, pv, a.off[i + 1] + a.vbeg - t.s0);
        }
        ++r;
    }
}
// the bytes of a 32-bit word named by the 4-bit mask m4, as 0xff each
TRRE_HD uint32_t filter_bytes4(uint32_t m4) { return ((m4 * 0x00204081u) & 0x01010101u) * 0xffu; }
TRRE_HD uint32_t filter_get_byte(const U128& r, int k) {
    const uint32_t w = k < 4 ? r.x : k < 8 ? r.y : k < 12 ? r.z : r.w;
    return (w >> (8u * (uint32_t)(k & 3))) & 0xffu;
}
// ... the tile's E kept bytes to out + kbase[b].  Destination vector g of the address holds kept bytes [e0, e1), which are one
// or more RUNS of consecutive source bytes.  The first byte of a run is found by its rank (rec_select), its length is the kept
// bits in a row from there, and the run's bytes are str_funnel16 of the image from k bytes in front of it, k the run's place in
// the vector — so 16 source bytes in one run are one funnel and one store, and a vector of r runs takes r of each, merged under
// byte masks.  (lds: filter_keep_vecs' image, the tile's byte x at 16 + x)
template <class G>
TRRE_HD void filter_emit_vecs(const FilterArgs& a, int64_t b, int tid, const U128* lds, const uint16_t* bits16, const uint32_t* pre,
                              const uint32_t* pv) {
    const int64_t d0 = (int64_t)a.base[a.tiles + 1 + b], E = pv[G::NVEC];
    const int A = (int)((reinterpret_cast<uintptr_t>(a.out) + (uintptr_t)d0) & 15u);
    const int ng = E ? (int)((E + A + 15) >> 4) : 0;
    for (int g = tid; g < ng; g += G::THREADS) {
        const int64_t e0 = g ? 16 * (int64_t)g - A : 0;
        const int64_t e1 = 16 * (int64_t)g - A + 16 < E ? 16 * (int64_t)g - A + 16 : E;
        if (d0 + e1 > a.out_len) continue;                            // (never: the totals were checked before this pass)
        const int cnt = (int)(e1 - e0);
        int64_t x = rec_select<G>(bits16, pre, (uint32_t)e0 + 1u);
        U128 r;
        r.x = r.y = r.z = r.w = 0;
        for (int k = 0;;) {
            const int q = (int)(x >> 4);
            const uint32_t ahead = ((uint32_t)bits16[q] | (q + 1 < G::NVEC ? (uint32_t)bits16[q + 1] << 16 : 0u)) >> (uint32_t)(x & 15);
            int L = __builtin_ctz(~ahead | 0x10000u);                 // kept bytes in a row from x: 1 .. 16
            if (L > cnt - k) L = cnt - k;
            const U128 f = str_funnel16(lds, x + 16 - k);
            const uint32_t m = ((1u << (uint32_t)L) - 1u) << (uint32_t)k;
            r.x |= f.x & filter_bytes4(m & 15u); r.y |= f.y & filter_bytes4((m >> 4) & 15u);
            r.z |= f.z & filter_bytes4((m >> 8) & 15u); r.w |= f.w & filter_bytes4((m >> 12) & 15u);
            k += L;
            if (k >= cnt) break;
            x = rec_select<G>(bits16, pre, (uint32_t)(e0 + k) + 1u);
        }
        uint8_t* d = a.out + d0 + e0;
        if (cnt == 16) {
            rec_store16(d, r);
        } else {
            for (int k = 0; k < cnt; ++k) d[k] = (uint8_t)filter_get_byte(r, k);
        }
    }
}

// ---- field k of every string (trre_field_device_strings) -------------------------------------------------------------------
// One piece per string of the split call's c_i + 1 pieces: piece kk_i = k (k >= 0) or c_i + 1 + k (k < 0), c_i the string's
// matches; the string HAS the field exactly when kk_i lies in [0, c_i].  The field is one contiguous range [lo_i, hi_i) of d_in
// inside string i; the ranges are ordered and disjoint, so the output is the filter call's compaction with [lo_i, hi_i) in place
// of the whole string and its verdict.  An absent field is the empty range at the string's end.  The passes, behind k_span_emit's
// list offsets L in an array of the library's own:
//   k_field_init    over the strings, 64 to a wave: the bitmap word (one ballot), and the bounds no marker owns:
//                   lo_i = off[i] when kk_i = 0, hi_i = off[i + 1] when kk_i = c_i, both off[i + 1] when the field is absent
//   k_field_pick    k_span_emit's mark images, scans and ranks over the framed tiles; the A of match kk_i of string i stores
//                   hi_i (the piece ends where that match starts), the B of match kk_i - 1 stores lo_i; a '\n' lane stores nothing
//   k_filter_part, k_field_count, k_chunk_scan twice   as for the filter call, over 16 KiB tiles of the INPUT: the strings with the
//                   field among those that END in the tile, and the tile's field bytes: [lo_i, hi_i) clipped to the tile, of those
//                   strings and of the one string that covers the tile's end.  (A string that ends in tile b with its field in an
//                   earlier tile clips to nothing in b; the earlier tile has it as its covering string.)  The totals are n_valid
//                   and out_len, read back and checked before d_out and d_out_off are written
//   k_field_emit    k_filter_emit with the toggles at lo_i and hi_i (an empty range toggles nothing); the thread that owns string
//                   i, in the tile the string ends in, stores out_off[i + 1] = tile base + field bytes of the tile before off[i + 1]
// Who writes which byte and word: every bitmap word lane 0 of its wave in k_field_init; lo_i and hi_i either k_field_init or the
// one marker lane named above, never both; out_off[0] thread 0 of tile 0; out_off[i + 1] the thread that owns string i; every
// output byte the thread that owns its destination vector, once (filter_emit_vecs).
struct FieldArgs {
    FilterArgs f;           // the tiles of the input, as the filter call has them: in_v0, vbeg, n, off, loff, nrec, tiles, part, cnt
                            // (strings with the field, field bytes per tile), base, out, out_len; out_off is [nrec + 1] here;
                            // invert, rows and n_kept are not used
    int64_t k;              // which field
    int64_t* lo;            // [nrec] where string i's field starts
    int64_t* hi;            // [nrec] ... and ends
    uint64_t* valid;        // [words] the bitmap
    int64_t words;          // ceil(nrec / 64)
};

// the piece k selects in string i; true when the string has it.  (c + 1 > 0 > k: the sum cannot overflow, and k is never negated)
TRRE_HD bool field_index(const FieldArgs& a, int64_t i, int64_t& kk) {
    const int64_t c = a.f.loff[i + 1] - a.f.loff[i];
    kk = a.k >= 0 ? a.k : c + 1 + a.k;
    return kk >= 0 && kk <= c;
}
// k_field_init, one lane: the verdict, and the bounds that no marker stores
TRRE_HD bool field_init(const FieldArgs& a, int64_t i) {
    int64_t kk;
    const bool has = field_index(a, i, kk);
    const int64_t s = a.f.off[i], e = a.f.off[i + 1];
    if (!has) {
        a.lo[i] = a.hi[i] = e;
    } else {
        if (kk == 0) a.lo[i] = s;
        if (kk == a.f.loff[i + 1] - a.f.loff[i]) a.hi[i] = e;
    }
    return has;
}
// k_field_pick, behind the barrier that completes bits and pv: the bounds the tile's markers own.  A number j of string nl ends
// its piece j; B number j starts its piece j + 1
template <class G>
TRRE_HD void field_pick_markers(const FieldArgs& a, const SpanArgs& sp, int64_t b, int tid, const uint16_t* bits, const uint32_t* pv_ab,
                                const uint32_t* pv_nl) {
    span_each_marker<G>(sp, b, tid, bits, pv_ab, pv_nl, [&](int kind, int64_t na, int64_t nb, int64_t nl, int64_t pos) {
        if (kind == 2 || nl >= a.f.nrec) return;          // (never beyond: the newline total was checked against nrec before)
        int64_t kk;
        if (!field_index(a, nl, kk)) return;
        if ((kind == 0 ? na : nb + 1) - a.f.loff[nl] != kk) return;
        (kind == 0 ? a.hi : a.lo)[nl] = pos;
    });
}
// string i's field bytes among the positions [t0, t1)
TRRE_HD uint64_t field_clip(const FieldArgs& a, int64_t i, int64_t t0, int64_t t1) {
    const int64_t s = a.lo[i] > t0 ? a.lo[i] : t0, e = a.hi[i] < t1 ? a.hi[i] : t1;
    return e > s ? (uint64_t)(e - s) : 0u;
}
// k_field_count: the thread's strings with the field and their field bytes in the tile; thread 0 adds the string that covers the
// tile's end
template <class G>
TRRE_HD void field_count_strings(const FieldArgs& a, const FilterTile<G>& t, int tid, uint64_t& valid, uint64_t& bytes) {
    valid = bytes = 0;
    const int64_t hi = t.hi(tid);
    for (int64_t i = t.lo(tid); i < hi; ++i) {
        int64_t kk;
        if (field_index(a, i, kk)) ++valid;
        bytes += field_clip(a, i, t.t0, t.t1);
    }
    if (tid == 0 && t.i1 < a.f.nrec) bytes += field_clip(a, t.i1, t.t0, t.t1);
}
// k_field_emit: the toggles of string i's field (bits32: TILE / 32 words, zeroed before); an end behind the tile toggles nothing
template <class G>
TRRE_HD void field_toggle(const FieldArgs& a, const FilterTile<G>& t, int64_t i, uint32_t* bits32) {
    const int64_t s = a.lo[i] > t.t0 ? a.lo[i] : t.t0, e = a.hi[i];
    if (e > s && s < t.t1) {
        filter_toggle(bits32, s + a.f.vbeg - t.s0, G::TILE);
        filter_toggle(bits32, e + a.f.vbeg - t.s0, G::TILE);
    }
}
template <class G>
TRRE_HD void field_mark(const FieldArgs& a, const FilterTile<G>& t, int tid, uint32_t* bits32) {
    const int64_t hi = t.hi(tid);
    for (int64_t i = t.lo(tid); i < hi; ++i) field_toggle<G>(a, t, i, bits32);
    if (tid == 0 && t.i1 < a.f.nrec) field_toggle<G>(a, t, t.i1, bits32);
}
// ... behind the barrier that completes the kept image and pv: out_off of the thread's strings
template <class G>
TRRE_HD void field_emit_offsets(const FieldArgs& a, const FilterTile<G>& t, int64_t b, int tid, const uint16_t* bits16, const uint32_t* pv) {
    if (b == 0 && tid == 0) a.f.out_off[0] = 0;
    const int64_t k0 = (int64_t)a.f.base[a.f.tiles + 1 + b];
    const int64_t hi = t.hi(tid);
    for (int64_t i = t.lo(tid); i < hi; ++i)
        if (i < a.f.nrec)                                            // (never beyond: part[] holds string numbers)
            a.f.out_off[i + 1] = k0 + (int64_t)filter_kept_below<G>(bits16, pv, a.f.off[i + 1] + a.f.vbeg - t.s0);
}

// ---- split at the first or last matches only (trre_splitn_device_strings, trre_fieldn_device_strings) ----------------------
// The split call with a RULE: match r of a string's c matches CUTS exactly when splitn_cuts says so; a match that does not cut
// stays in its piece as ordinary text.  So the depth of the split call counts the cutting matches alone, a position byte is kept
// exactly when it lies outside every CUTTING match, and the markers of a match that does not cut are dropped and store nothing.
// The rule needs the match's rank in its string and, from the end, the string's matches: A number j (B number j) with l '\n'
// before it is match r = j - L[l] of c = L[l + 1] - L[l], L the span call's list offsets in an array of the library's own
// (k_span_emit, lists only).  It is resolved once per marker — never per byte — and once per tile that starts inside a match
// (base[0][b] > base[1][b]: match base[0][b] - 1 of string base[2][b], a tile may lie wholly inside it and hold no marker).
// With kp the kept bytes and cb the cutting B before framed position q:
//     kept byte at q        out[kp] = in[q - a - b - l]
//     cutting B at q        piece_off[cb + 1 + l] = kp
//     '\n' number i at q    piece_off[cb + i + 1] = kp,  list_off[i + 1] = cb + i + 1      (depth 0: every cutting A before is closed)
// The passes, behind k_span_count and its three scans and k_span_emit's L:
//   k_splitn_count  k_span_emit's three mark images, scans and prefixes; every marker lane resolves the rule and sets its bit of the
//                   CUT image (LDS, zeroed before); a workgroup scan of the cut bits per thread segment gives every segment its
//                   depth on entry; kcnt[2][tiles]: the tile's kept bytes and cutting B;  k_chunk_scan twice: kbase[2][tiles + 1];
//                   the totals are out_len and n_pieces - nrec, read back and checked before anything of the caller's is stored
//   k_splitn_emit   the same images, the kept image and the scan of kept bytes and cutting B (one word: a tile holds fewer than
//                   65 536 bytes); then a wave takes 64 framed bytes at a time, as k_split_emit does
// Who writes which byte and word: entry 0 of both arrays thread 0 of tile 0; every output byte the lane that owns its kept position
// byte; every other word the lane that owns its cutting B or '\n', once.  An A lane and the B of a match that does not cut store
// nothing.  lists_only: out and piece_off are not stored at all.
constexpr uint32_t kSplitFromEnd = 1u;                // TRRE_SPLIT_FROM_END

// THE RULE: does match r of a string's c matches cut.  (limit is compared, never added or negated: any int64 is legal)
TRRE_HD bool splitn_cuts(int64_t r, int64_t c, int64_t limit, uint32_t flags) {
    if (limit < 0) return true;
    return (flags & kSplitFromEnd) ? c - r <= limit : r < limit;
}
// ... and how many of the c do: they are the first or the last so many
TRRE_HD int64_t splitn_cutting(int64_t c, int64_t limit) { return limit < 0 || limit > c ? c : limit; }

struct SplitnArgs {
    SplitArgs s;            // as the split call has them; kcnt: [2][tiles] kept bytes, cutting B per tile; kbase: [2][tiles + 1]
    const int64_t* L;       // [nrec + 1] the span call's list offsets
    int64_t limit;
    uint32_t flags;
};

// does match j of the column, which lies in string l, cut (from the front the string's matches are not looked up)
TRRE_HD bool splitn_match_cuts(const SplitnArgs& a, int64_t j, int64_t l) {
    if (a.limit < 0) return true;
    if (l < 0 || l >= a.s.nrec) return false;         // (never: the newline total was checked against nrec before)
    const int64_t l0 = a.L[l];
    const int64_t c = (a.flags & kSplitFromEnd) ? a.L[l + 1] - l0 : 0;
    return splitn_cuts(j - l0, c, a.limit, a.flags);
}
// 1 when tile b starts inside a cutting match (the same for every thread of the workgroup)
TRRE_HD uint32_t splitn_tile_depth(const SplitnArgs& a, int64_t b) {
    const int64_t na = (int64_t)a.s.base[b], nb = (int64_t)a.s.base[a.s.tiles + 1 + b];
    if (na <= nb) return 0u;
    return splitn_match_cuts(a, na - 1, (int64_t)a.s.base[2 * (a.s.tiles + 1) + b]) ? 1u : 0u;
}
// behind the barrier that completes bits and pv: the bits of the tile's cutting markers (cut32: TILE / 32 words, zeroed before)
template <class G>
TRRE_HD void splitn_cut_markers(const SplitnArgs& a, int64_t b, int tid, const uint16_t* bits, const uint32_t* pv_ab, const uint32_t* pv_nl,
                                uint32_t* cut32) {
    SpanArgs sp{};
    sp.base = a.s.base; sp.tiles = a.s.tiles;
    span_each_marker<G>(sp, b, tid, bits, pv_ab, pv_nl, [&](int kind, int64_t na, int64_t nb, int64_t nl, int64_t pos) {
        if (kind == 2 || !splitn_match_cuts(a, kind == 0 ? na : nb, nl)) return;
        const int64_t x = pos + na + nb + nl - b * G::TILE;           // the marker's byte in the tile
        TRRE_REC_LDS_OR(cut32 + (x >> 5), 1u << (uint32_t)(x & 31));
    });
}
// cutting markers | cutting B << 16 in the thread's rank segment, vectors [tid * VECS, tid * VECS + VECS)
template <class G>
TRRE_HD uint32_t splitn_seg_cut(const uint16_t* bits, const uint16_t* cut, int tid) {
    static_assert(G::TILE < 65536, "two counts of a tile share a 32-bit word");
    uint32_t c = 0;
    for (int k = 0; k < G::VECS; ++k) {
        const int q = tid * G::VECS + k;
        c += rec_popc(cut[q]) | rec_popc((uint32_t)cut[q] & bits[G::NVEC + q]) << 16;
    }
    return c;
}
// the kept bits of the thread's rank segment (d0: splitn_tile_depth; pre_c: splitn_seg_cut before the segment in the tile); kept:
// [NVEC] 16-bit masks, or null (k_splitn_count).  Returns the segment's kept bytes
template <class G>
TRRE_HD uint32_t splitn_seg_kept(const SplitnArgs& a, int64_t b, int tid, const uint16_t* bits, const uint16_t* cut, uint32_t d0, uint32_t pre_c,
                                 uint16_t* kept) {
    uint32_t d = (d0 + (pre_c & 0xffffu)) & 1u;
    uint32_t c = 0;
    for (int k = 0; k < G::VECS; ++k) {
        const int q = tid * G::VECS + k;
        const int64_t v = b * G::TILE + 16 * (int64_t)q;
        const uint32_t mk = (uint32_t)bits[q] | bits[G::NVEC + q], cm = cut[q], nl = bits[2 * G::NVEC + q];
        const uint32_t ok = v < a.s.total ? rec_valid16(v, 0, a.s.total) : 0u;
        const uint32_t kp = ~(split_odd_below16(cm) ^ (0u - d)) & ~mk & ~nl & ok;
        if (kept) kept[q] = (uint16_t)kp;
        c += rec_popc(kp);
        d ^= rec_popc(cm) & 1u;
    }
    return c;
}
// kept bytes | cutting B << 16 before each of the thread's segment vectors (pre_k, pre_c: before the segment)
template <class G>
TRRE_HD void splitn_fill_pv(const uint16_t* bits, const uint16_t* cut, const uint16_t* kept, uint32_t pre_k, uint32_t pre_c, int tid, uint32_t* pv_kc) {
    uint32_t run = pre_k | (pre_c >> 16) << 16;
    for (int k = 0; k < G::VECS; ++k) {
        const int q = tid * G::VECS + k;
        pv_kc[q] = run;
        run += rec_popc(kept[q]) | rec_popc((uint32_t)cut[q] & bits[G::NVEC + q]) << 16;
    }
}
// k_splitn_emit, behind the barrier that completes the five images and the three pv: the tile's bytes and words
template <class G>
TRRE_HD void splitn_emit_pieces(const SplitnArgs& a, int64_t b, int tid, const uint16_t* bits, const uint16_t* cut, const uint16_t* kept,
                                const uint32_t* pv_ab, const uint32_t* pv_nl, const uint32_t* pv_kc) {
    static_assert(G::THREADS % 64 == 0 && G::NVEC % 4 == 0, "a wave takes 64-byte pieces of the tile");
    constexpr int kPieces = G::NVEC / 4, kWaves = G::THREADS / 64;
    const SplitArgs& s = a.s;
    const int lane = tid & 63;
    const int64_t s0 = b * G::TILE;
    const int64_t a0 = (int64_t)s.base[b], b0 = (int64_t)s.base[s.tiles + 1 + b], l0 = (int64_t)s.base[2 * (s.tiles + 1) + b];
    const int64_t k0 = (int64_t)s.kbase[b], c0 = (int64_t)s.kbase[s.tiles + 1 + b];
    if (b == 0 && tid == 0) {
        s.list_off[0] = 0;
        if (!s.lists_only) s.piece_off[0] = 0;
    }
    for (int k = tid >> 6; k < kPieces; k += kWaves) {
        const uint64_t wa = span_word(bits, k), wb = span_word(bits + G::NVEC, k), wl = span_word(bits + 2 * G::NVEC, k);
        const uint64_t wk = span_word(kept, k), wc = span_word(cut, k) & wb;
        if (!(((s.lists_only ? wl : wc | wl | wk) >> lane) & 1u)) continue;
        const uint64_t below = (1ull << lane) - 1ull;
        const int64_t nl = l0 + (int64_t)pv_nl[4 * k] + (int64_t)match_popc64(wl & below);
        const int64_t kp = k0 + (int64_t)(pv_kc[4 * k] & 0xffffu) + (int64_t)match_popc64(wk & below);
        const int64_t cb = c0 + (int64_t)(pv_kc[4 * k] >> 16) + (int64_t)match_popc64(wc & below);
        // (never beyond: the totals were checked against n, the pieces and nrec before this pass)
        if ((wk >> lane) & 1u) {
            const int64_t na = a0 + (int64_t)(pv_ab[4 * k] & 0xffffu) + (int64_t)match_popc64(wa & below);
            const int64_t nb = b0 + (int64_t)(pv_ab[4 * k] >> 16) + (int64_t)match_popc64(wb & below);
            const int64_t at = s0 + 64 * (int64_t)k + lane - na - nb - nl;
            if (kp < s.out_len && at >= 0 && at < s.n) s.out[kp] = s.in[at];
        } else if ((wc >> lane) & 1u) {
            if (cb + 1 + nl <= s.n_piece) s.piece_off[cb + 1 + nl] = kp;
        } else if (nl < s.nrec) {
            s.list_off[nl + 1] = cb + nl + 1;
            if (!s.lists_only && cb + nl + 1 <= s.n_piece) s.piece_off[cb + nl + 1] = kp;
        }
    }
}

// Field k of that split: the field call with the string's cc = splitn_cutting(c) cutting matches in place of its c.  They are the
// matches m0 .. m0 + cc - 1 of the string, m0 = 0 from the front and c - cc from the end; piece kk = k (k >= 0) or cc + 1 + k
// (k < 0) is there exactly when kk lies in [0, cc]; it starts at the string's start when kk = 0, otherwise where match
// m0 + kk - 1 ends, and ends at the string's end when kk = cc, otherwise where match m0 + kk starts.  Only which marker stores a
// bound is new (k_fieldn_init, k_fieldn_pick, and the verdicts of k_fieldn_count); the emit pass is the field call's.
struct FieldnArgs {
    FieldArgs a;            // as the field call has them
    int64_t limit;
    uint32_t flags;
};

// the piece k selects in string i; true when the string has it.  (cc + 1 > 0 > k: the sum cannot overflow; 0 <= m0 <= c)
TRRE_HD bool fieldn_index(const FieldnArgs& a, int64_t i, int64_t& kk, int64_t& cc, int64_t& m0) {
    const int64_t c = a.a.f.loff[i + 1] - a.a.f.loff[i];
    cc = splitn_cutting(c, a.limit);
    m0 = (a.flags & kSplitFromEnd) ? c - cc : 0;
    kk = a.a.k >= 0 ? a.a.k : cc + 1 + a.a.k;
    return kk >= 0 && kk <= cc;
}
// k_fieldn_init, one lane: the verdict, and the bounds that no marker stores
TRRE_HD bool fieldn_init(const FieldnArgs& a, int64_t i) {
    int64_t kk, cc, m0;
    const bool has = fieldn_index(a, i, kk, cc, m0);
    const int64_t s = a.a.f.off[i], e = a.a.f.off[i + 1];
    if (!has) {
        a.a.lo[i] = a.a.hi[i] = e;
    } else {
        if (kk == 0) a.a.lo[i] = s;
        if (kk == cc) a.a.hi[i] = e;
    }
    return has;
}
// k_fieldn_pick: the bounds the tile's markers own.  The A of the string's match m0 + kk ends piece kk (kk < cc); the B of its
// match m0 + kk - 1 starts it (kk > 0)
template <class G>
TRRE_HD void fieldn_pick_markers(const FieldnArgs& a, const SpanArgs& sp, int64_t b, int tid, const uint16_t* bits, const uint32_t* pv_ab,
                                 const uint32_t* pv_nl) {
    span_each_marker<G>(sp, b, tid, bits, pv_ab, pv_nl, [&](int kind, int64_t na, int64_t nb, int64_t nl, int64_t pos) {
        if (kind == 2 || nl >= a.a.f.nrec) return;        // (never beyond: the newline total was checked against nrec before)
        int64_t kk, cc, m0;
        if (!fieldn_index(a, nl, kk, cc, m0)) return;
        const int64_t r = (kind == 0 ? na : nb) - a.a.f.loff[nl];
        if (kind == 0 ? (kk < cc && r == m0 + kk) : (kk > 0 && r == m0 + kk - 1)) (kind == 0 ? a.a.hi : a.a.lo)[nl] = pos;
    });
}
// k_fieldn_count: field_count_strings with the limited verdict
template <class G>
TRRE_HD void fieldn_count_strings(const FieldnArgs& a, const FilterTile<G>& t, int tid, uint64_t& valid, uint64_t& bytes) {
    valid = bytes = 0;
    const int64_t hi = t.hi(tid);
    for (int64_t i = t.lo(tid); i < hi; ++i) {
        int64_t kk, cc, m0;
        if (fieldn_index(a, i, kk, cc, m0)) ++valid;
        bytes += field_clip(a.a, i, t.t0, t.t1);
    }
    if (tid == 0 && t.i1 < a.a.f.nrec) bytes += field_clip(a.a, t.i1, t.t0, t.t1);
}

// ---- trimmed strings (trre_trim_device_strings) -----------------------------------------------------------------------------
// Every string without the match that touches its start and the match that touches its end: str.strip / lstrip / rstrip, SQL's
// TRIM, removeprefix / removesuffix.  String i = [off[i], off[i + 1]) of len bytes has the spans (s_0, e_0) .. (s_{c-1}, e_{c-1}):
//     lo = max{ e_j : s_j == 0 }    (the left side asked for; else, and with no such match, 0)
//     hi = min{ s_j : e_j == len }  (the right side asked for; else, and with no such match, len)
// and the entry is [lo, max(lo, hi)).  At most one match starts at 0 (an attempt at a position yields one match), and it is
// match 0; at most two end at len, a non-empty one and the empty tail attempt behind it ('x*' on "xxbxx": (3, 5) and (5, 5), the
// trim is "b"), and they are matches c - 1 and c - 2.  So six words per string decide both bounds: where matches 0, c - 1 and
// c - 2 start and end.  The entry is one contiguous range inside its string, so the output is the field call's compaction with
// k = 0 (every string has its entry).  The passes, behind k_span_emit's list offsets L in an array of the library's own:
//   k_trim_pick     k_span_emit's mark images, scans and ranks over the framed tiles; the A (the B) of match r of its string's c
//                   parks its position in the word of every role the match plays: match 0 (the left side), match c - 1 and
//                   match c - 2 (the right side).  The test is on ranks alone: L twice per marker; a '\n' lane stores nothing
//   k_trim_bounds   over the strings, 64 to a wave: the rule above from off, L and the parked words that exist (none for c = 0,
//                   the words of c - 2 for c >= 2 only); lo_i and hi_i = max(lo_i, hi_i) into the field call's bounds, and into
//                   the caller's begin and end where given
//   k_filter_part, k_field_count, k_chunk_scan twice, k_field_emit   the field call's, unchanged, with k = 0
// Who writes which word: every parked word the one marker lane whose match plays the word's role in its string (a match that
// plays two roles — the only match of its string is match 0 and match c - 1 — parks twice, into two words); lo_i, hi_i, begin[i]
// and end[i] the lane of k_trim_bounds that owns string i.  A side that is not asked for parks nothing and reads nothing.
constexpr uint32_t kTrimLeft = 1u, kTrimRight = 2u;   // TRRE_TRIM_LEFT, TRRE_TRIM_RIGHT

struct TrimArgs {
    FieldArgs a;            // as the field call has them, k = 0; valid and words are not used
    uint32_t flags;
    int64_t* marks;         // [6][nrec] where match 0 starts and ends, match c - 1, match c - 2: positions in d_in
    int64_t* begin;         // [nrec] the caller's, or null: lo_i
    int64_t* end;           // [nrec] ... hi_i
};

// k_trim_pick, behind the barrier that completes bits and pv: the words the tile's markers park
template <class G>
TRRE_HD void trim_pick_markers(const TrimArgs& a, const SpanArgs& sp, int64_t b, int tid, const uint16_t* bits, const uint32_t* pv_ab,
                               const uint32_t* pv_nl) {
    span_each_marker<G>(sp, b, tid, bits, pv_ab, pv_nl, [&](int kind, int64_t na, int64_t nb, int64_t nl, int64_t pos) {
        if (kind == 2 || nl >= a.a.f.nrec) return;        // (never beyond: the newline total was checked against nrec before)
        const int64_t l0 = a.a.f.loff[nl], c = a.a.f.loff[nl + 1] - l0, r = (kind == 0 ? na : nb) - l0;
        int64_t* w = a.marks + kind * a.a.f.nrec + nl;    // (the A's word; the B's is nrec behind it)
        if ((a.flags & kTrimLeft) && r == 0) w[0] = pos;
        if (a.flags & kTrimRight) {
            if (r == c - 1) w[2 * a.a.f.nrec] = pos;
            if (r == c - 2) w[4 * a.a.f.nrec] = pos;
        }
    });
}
// k_trim_bounds, one lane: string i's bounds by the rule, from the parked words that exist
TRRE_HD void trim_bounds(const TrimArgs& a, int64_t i) {
    const int64_t nrec = a.a.f.nrec, s = a.a.f.off[i], e = a.a.f.off[i + 1], c = a.a.f.loff[i + 1] - a.a.f.loff[i];
    const int64_t* w = a.marks + i;
    int64_t lo = s, hi = e;
    if (c >= 1) {
        if ((a.flags & kTrimLeft) && w[0] == s) lo = w[nrec];
        if ((a.flags & kTrimRight) && w[3 * nrec] == e) {
            hi = w[2 * nrec];
            if (c >= 2 && w[5 * nrec] == e && w[4 * nrec] < hi) hi = w[4 * nrec];
        }
    }
    if (hi < lo) hi = lo;
    a.a.lo[i] = lo; a.a.hi[i] = hi;
    if (a.begin) { a.begin[i] = lo; a.end[i] = hi; }
}

// ---- replaced strings (trre_sub_device_strings) ----------------------------------------------------------------------------
// Some of every string's matches replaced by what they print: a splice of two sources the library already has.  The span call's
// emit pass leaves, in arrays of the library's own, S[j], E[j] (where match j of the column starts and ends in d_in) and the list
// offsets L[nrec + 1]; the find call's texts scan of the same staged text, unframed, leaves the texts X and XO[found + 1].  Match
// j belongs to string i = the first i with L[i + 1] > j (strings without matches are skipped by the search itself), has rank
// r = j - L[i] there, and is SELECTED when first <= r and (count < 0 or r - first < count).  With t_j the bytes of its text and
// m_j = E[j] - S[j] when selected, both 0 when not, the output is
//     in[0, S[0])   text 0   in[Ee[0], S[1])   text 1   in[Ee[1], S[2])   ...   text found-1   in[Ee[found-1], n)
// Ee[j] = E[j] when selected and S[j] when not: an unselected match is an empty text in front of its own bytes.  SEGMENT j is
// text j with the input behind it; it starts at output position
//     P[j] = S[j] + sum over k < j of (t_k - m_k),       P[found] = out_len = n - sum m + sum t
// Every array has one more entry in FRONT, index -1, for the bytes before the first match: P[-1] = 0, Ee[-1] = 0 with an empty
// text; and S[found] = n closes the last segment.  So segment j, j in [-1, found), covers the output [P[j], P[j + 1]), its
// text has (P[j + 1] - P[j]) - (S[j + 1] - Ee[j]) bytes at X + XO[j], and its input bytes start at Ee[j]: the emit pass needs
// no selection bit.  The passes, over CHUNKS of THREADS * kSubPer consecutive matches (a thread has kSubPer in a row):
//   k_sub_plan     the selection bit of every match, parked in P[j]; cnt[3][chunks]: the selected matches, their texts' bytes,
//                  their matched bytes; and the check that the spans and the texts' offsets are ordered (a status word)
//   k_chunk_scan   three times: base[3][chunks + 1]; the totals are n_replaced and out_len: the capacity decision
//   k_sub_place    P[j] and Ee[j] (in place of E[j]) from the chunk's bases and a workgroup scan of the threads' sums; thread 0 of
//                  chunk 0 stores P[-1], Ee[-1] = off[0], P[found] and S[found]
//   k_sub_offsets  a thread per entry: out_off[i] = off[i] + (P[L[i]] - S[L[i]]), the growth before the string's first match
//   k_sub_emit     output-driven, over tiles of TILE bytes of the OUTPUT's v-space (v = position + the address of out mod 16):
//                  thread 0 finds the segments the tile touches by two binary searches in P; when that window of P fits, all
//                  threads copy it into LDS; then a thread owns destination vectors (vector j * THREADS + tid of the tile:
//                  coalesced), finds the segment of each one's first byte (an upper bound in P, minus one) and fills it.  A
//                  whole vector inside one text or one run of input is one unaligned 16-byte read (two aligned loads and a
//                  funnel shift) and one aligned 16-byte store; any other is put together piece by piece, and leaves a
//                  segment for the next one that has bytes — the one behind it, or, behind a run of empty segments, an
//                  upper bound in P again: 40 000 empty segments at one position cost one search, not 40 000 steps.
// Who writes which byte and word: every P[j], Ee[j] the thread that owns match j; out_off[i] thread i; every output byte the
// thread that owns its destination vector, once; the ragged first and last vectors of the buffer are byte stores, and nothing
// at or behind out_len is stored.
constexpr int kSubPer = 4;                            // matches per thread: chunks of 1 024
constexpr int kSubWindow = 2048;                      // entries of P a tile keeps in LDS: 16 KiB

struct SubArgs {
    const uint8_t* in;      // the caller's d_in
    int64_t n;
    const int64_t* off;     // [nrec + 1] the caller's offsets
    int64_t nrec;
    const int64_t* L;       // [nrec + 1] the span call's list offsets
    int64_t* S;             // [-1 .. found] where match j starts (k_span_emit); S[found] = n (k_sub_place)
    int64_t* E;             // [-1 .. found) where it ends (k_span_emit), then the effective end Ee[j] (k_sub_place)
    const int64_t* XO;      // [0 .. found] the texts' offsets (k_find_unframe)
    const uint8_t* X;       // the texts
    int64_t x_len;          // their bytes: XO[found]
    int64_t* P;             // [-1 .. found] the selection bit (k_sub_plan), then where segment j starts in the output
    int64_t found;
    int64_t j0, out0;       // the first match and the output position of the column's start: 0 (the host shim: a column as if one came before)
    int64_t first, count;
    int64_t chunks;
    uint64_t* cnt;          // [3][chunks] selected matches, their texts' bytes, their matched bytes
    const uint64_t* base;   // [3][chunks + 1] their exclusive scans
    uint32_t* status;       // |= 1: the spans or the texts' offsets are not ordered (internal)
    uint8_t* out;           // [out_len]
    int64_t out_len;
    int64_t* out_off;       // [nrec + 1]
};

struct SubListKey {   // the matches before the end of string i
    const int64_t* L;
    TRRE_HD int64_t operator()(int64_t i) const { return L[i + 1]; }
};
struct SubPlaceKey {  // where segment k - 1 starts, k counted from the first one
    const int64_t* Pz;
    TRRE_HD int64_t operator()(int64_t k) const { return Pz[k]; }
};
TRRE_HD bool sub_selected(const SubArgs& a, int64_t r) { return a.first <= r && (a.count < 0 || r - a.first < a.count); }

// k_sub_plan: the thread's kSubPer matches of chunk c: their selection bits into P, c3 = their three sums; returns 1 when an
// array is out of order
template <int THREADS>
TRRE_HD uint32_t sub_plan_thread(const SubArgs& a, int64_t c, int tid, uint64_t (&c3)[3]) {
    c3[0] = c3[1] = c3[2] = 0;
    uint32_t bad = 0;
    const int64_t j0 = (c * THREADS + tid) * kSubPer;
    int64_t i = -1, iend = -1;                        // the string of the match before, and L[i + 1]
    for (int64_t j = j0; j < j0 + kSubPer && j < a.found; ++j) {
        if (j >= iend) {                              // (the string behind, where it has the match: short strings, a match or two each)
            i = i >= 0 && i + 2 <= a.nrec && j < a.L[i + 2] ? i + 1 : rec_lower_bound(SubListKey{a.L}, a.nrec, j + 1);
            if (i >= a.nrec) { bad = 1; break; }      // (never: L[nrec] = found)
            iend = a.L[i + 1];
        }
        const int64_t s = a.S[j], e = a.E[j], next = j + 1 < a.found ? a.S[j + 1] : a.n;
        const int64_t x0 = a.XO[j], x1 = a.XO[j + 1];
        if (s < 0 || s > e || e > next || next > a.n || x0 < 0 || x0 > x1 || x1 > a.x_len || (j == a.j0 && x0 != 0)) bad = 1;
        const bool sel = sub_selected(a, j - a.L[i]);
        a.P[j] = sel ? 1 : 0;
        if (sel) { c3[0] += 1; c3[1] += (uint64_t)(x1 - x0); c3[2] += (uint64_t)(e - s); }
    }
    return bad;
}
// k_sub_place: the thread's sums again, from the parked bits
template <int THREADS>
TRRE_HD void sub_place_sums(const SubArgs& a, int64_t c, int tid, uint64_t (&c3)[3]) {
    c3[0] = c3[1] = c3[2] = 0;
    const int64_t j0 = (c * THREADS + tid) * kSubPer;
    for (int64_t j = j0; j < j0 + kSubPer && j < a.found; ++j)
        if (a.P[j]) { c3[0] += 1; c3[1] += (uint64_t)(a.XO[j + 1] - a.XO[j]); c3[2] += (uint64_t)(a.E[j] - a.S[j]); }
}
// ... the same matches; pt, pm: the texts' and the matched bytes of the selected matches of the chunk before the thread's
template <int THREADS>
TRRE_HD void sub_place_thread(const SubArgs& a, int64_t c, int tid, uint64_t pt, uint64_t pm) {
    int64_t grow = (int64_t)(a.base[a.chunks + 1 + c] + pt) - (int64_t)(a.base[2 * (a.chunks + 1) + c] + pm);
    const int64_t j0 = (c * THREADS + tid) * kSubPer;
    for (int64_t j = j0; j < j0 + kSubPer && j < a.found; ++j) {
        const bool sel = a.P[j] != 0;
        a.P[j] = a.S[j] + grow;
        if (sel) grow += (a.XO[j + 1] - a.XO[j]) - (a.E[j] - a.S[j]);
        else a.E[j] = a.S[j];
    }
    if (j0 == a.j0) {
        a.P[a.j0 - 1] = a.out0; a.E[a.j0 - 1] = a.off[0];
        a.P[a.found] = a.out_len; a.S[a.found] = a.n;
    }
}
// k_sub_offsets: entry i of the output offsets, i in [0, nrec]
TRRE_HD void sub_offset(const SubArgs& a, int64_t i) {
    const int64_t j = a.L[i];
    a.out_off[i] = a.off[i] + (a.P[j] - a.S[j]);
}

// k_sub_emit.  The segments are counted from 0 here: k = j + 1, over Pz = P - 1 [found + 2], Sz = S - 1, Ez = E - 1, XOz = XO - 1
template <class G>
struct SubTile {
    int A;                  // the address of out mod 16
    int64_t o0, o1;         // the tile's output positions
    TRRE_HD SubTile(const SubArgs& a, int64_t b) {
        A = (int)(reinterpret_cast<uintptr_t>(a.out) & 15u);
        o0 = b * G::TILE - A > a.out0 ? b * G::TILE - A : a.out0;
        o1 = (b + 1) * G::TILE - A < a.out_len ? (b + 1) * G::TILE - A : a.out_len;
    }
};
// the segment that holds output position o (o < out_len): the last k with Pz[k] <= o
TRRE_HD int64_t sub_segment_of(const SubArgs& a, int64_t o) {
    return a.j0 + rec_lower_bound(SubPlaceKey{a.P - 1 + a.j0}, a.found + 1 - a.j0, o + 1) - 1;
}
// thread 0: the segments [win[0], win[1]] the tile touches
template <class G>
TRRE_HD void sub_emit_window(const SubArgs& a, const SubTile<G>& t, int64_t* win) {
    win[0] = sub_segment_of(a, t.o0);
    win[1] = sub_segment_of(a, t.o1 - 1);
}
// all threads: Pz[win[0] .. win[1] + 1] into the image, when it fits
template <class G>
TRRE_HD void sub_keep_window(const SubArgs& a, const int64_t* win, int tid, int64_t* image) {
    const int64_t cnt = win[1] - win[0] + 2;
    if (cnt > kSubWindow) return;
    for (int64_t k = tid; k < cnt; k += G::THREADS) image[k] = a.P[win[0] + k - 1];
}
// Pz through the tile's image where it has the entry
struct SubPlaces {
    const int64_t* Pz;
    const int64_t* image;
    int64_t k0, cnt;        // the image holds Pz[k0 .. k0 + cnt); cnt 0: no image
    TRRE_HD int64_t operator()(int64_t k) const { return k >= k0 && k - k0 < cnt ? image[k - k0] : Pz[k]; }
};
template <class G>
TRRE_HD SubPlaces sub_places(const SubArgs& a, const int64_t* win, const int64_t* image) {
    const int64_t cnt = win[1] - win[0] + 2;
    return SubPlaces{a.P - 1, image, win[0], cnt > kSubWindow ? 0 : cnt};
}
// the last k in [lo, hi] with Pz[k] <= o (Pz[lo] <= o)
TRRE_HD int64_t sub_segment_in(const SubPlaces& pz, int64_t lo, int64_t hi, int64_t o) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (pz(mid) <= o) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// 16 bytes from any address whose 16 bytes are all readable: two aligned loads, funnel-shifted (str_funnel16's arithmetic)
TRRE_HD U128 sub_load16u(const uint8_t* p) {
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    const U128* q = reinterpret_cast<const U128*>(p - sh);
    const U128 lo = q[0];
    if (sh == 0) return lo;
    const U128 hi = q[1];
    uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    if (sh & 8u) { w[0] = w[2]; w[1] = w[3]; w[2] = w[4]; w[3] = w[5]; w[4] = w[6]; w[5] = w[7]; }
    if (sh & 4u) { w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = w[4]; w[4] = w[5]; }
    const uint32_t bs = (sh & 3u) * 8u;
    U128 r;
    r.x = (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> bs); r.y = (uint32_t)((((uint64_t)w[2] << 32) | w[1]) >> bs);
    r.z = (uint32_t)((((uint64_t)w[3] << 32) | w[2]) >> bs); r.w = (uint32_t)((((uint64_t)w[4] << 32) | w[3]) >> bs);
    return r;
}
// the thread's destination vectors of tile b
template <class G>
TRRE_HD void sub_emit_vecs(const SubArgs& a, const SubTile<G>& t, int64_t b, int tid, const int64_t* win, const int64_t* image) {
    const SubPlaces pz = sub_places<G>(a, win, image);
    const int64_t* Sz = a.S - 1;
    const int64_t* Ez = a.E - 1;
    const int64_t* XOz = a.XO - 1;
    for (int j = 0; j < G::VECS; ++j) {
        const int64_t v = b * G::TILE + 16 * ((int64_t)j * G::THREADS + tid);
        const int64_t p0 = v - t.A > a.out0 ? v - t.A : a.out0, p1 = v + 16 - t.A < a.out_len ? v + 16 - t.A : a.out_len;
        if (p1 <= p0) continue;
        const int cnt = (int)(p1 - p0);
        int64_t k = sub_segment_in(pz, win[0], win[1], p0);
        int64_t beg = pz(k), end = pz(k + 1);
        int64_t tl = (end - beg) - (Sz[k + 1] - Ez[k]);               // the segment's text bytes
        uint8_t* d = a.out + p0;
        if (cnt == 16 && p0 + 16 <= end && (p0 - beg >= tl || p0 - beg + 16 <= tl)) {
            const int64_t at = p0 - beg;
            rec_store16(d, sub_load16u(at >= tl ? a.in + Ez[k] + (at - tl) : a.X + XOz[k] + at));
            continue;
        }
        U128 r;
        r.x = r.y = r.z = r.w = 0;
        int64_t o = p0;
        for (int f = 0;;) {
            const int64_t at = o - beg;
            const int take = end - o < cnt - f ? (int)(end - o) : cnt - f;
            const int64_t text = tl > 0 ? XOz[k] : 0, raw = Ez[k] - tl;
            for (int x = 0; x < take; ++x) str_put_byte(r, f + x, at + x < tl ? a.X[text + at + x] : a.in[raw + at + x]);
            f += take; o += take;
            if (f >= cnt) break;
            k = pz(k + 2) > o ? k + 1 : sub_segment_in(pz, k + 1, win[1], o);      // (o < out_len: segment k + 1 exists)
            beg = pz(k); end = pz(k + 1);
            tl = (end - beg) - (Sz[k + 1] - Ez[k]);
        }
        if (cnt == 16) {
            rec_store16(d, r);
        } else {
            for (int x = 0; x < cnt; ++x) d[x] = (uint8_t)filter_get_byte(r, x);
        }
    }
}

// ---- match k of every string (trre_nth_device_strings) ---------------------------------------------------------------------
// One entry per string of the find call's lists: with c_i = L[i + 1] - L[i] the string's matches, entry i is match
// j_i = L[i] + kk_i of the column, kk_i = k (k >= 0) or c_i + k (k < 0); the string HAS the match exactly when kk_i lies in
// [0, c_i).  The find call's two scans leave the list offsets L[nrec + 1] and, unframed, the texts X with XO[found + 1], in
// arrays of the library's own.  Entry i is X[src_i, src_i + len_i), src_i = XO[j_i], len_i = XO[j_i + 1] - XO[j_i], both 0 when
// the match is absent: the sources are ordered but NOT adjacent, so the passes are string-driven up to the sizes and
// output-driven for the bytes — no compaction over all the texts.  Over CHUNKS of THREADS * kNthPer consecutive strings:
//   k_nth_plan     string (c * kNthPer + r) * THREADS + tid in round r: 64 consecutive strings to a wave, so the wave's verdicts
//                  are one ballot, the bitmap word; src_i parked; cnt[2][chunks]: the strings with the match and the entries'
//                  bytes; and the check that L and the texts' offsets are ordered and in range (a status word)
//   k_chunk_scan   twice: base[2][chunks + 1]; the totals are n_valid and out_len: the capacity decision
//   k_nth_offsets  a thread has kNthPer strings in a row: out_off[i + 1] from the chunk's base and a workgroup scan of the
//                  threads' sums of len_i
//   k_nth_emit     k_sub_emit with one source: output-driven over tiles of TILE bytes of the OUTPUT's v-space (v = position + the
//                  address of out mod 16).  Thread 0 finds the entries the tile touches by two binary searches in out_off (the
//                  LAST entry that starts at or before a position: behind a run of empty entries at one position that is the one
//                  with the bytes, found by one search); when that window of out_off fits, all threads copy it into LDS (kSubWindow
//                  entries, 16 KiB: k_sub_emit's budget, which leaves the CU's residency to the registers); then a thread
//                  owns destination vectors j * THREADS + tid.  A whole vector inside one entry is one unaligned 16-byte read (two
//                  aligned loads and a funnel shift) and one aligned 16-byte store; any other is put together piece by piece.
// Who writes which byte and word: every bitmap word lane 0 of its wave in k_nth_plan (lanes at or beyond nrec vote false: the
// tail is zero); src_i the thread that owns string i there; out_off[0] thread 0 of chunk 0 in k_nth_offsets, out_off[i + 1] the
// thread that owns string i; every output byte the thread that owns its destination vector, once; the ragged first and last
// vectors of the buffer are byte stores, and nothing at or behind out_len is stored.
constexpr int kNthPer = 4;                            // strings per thread: chunks of 1 024

struct NthArgs {
    const int64_t* L;       // [nrec + 1] the find call's list offsets
    int64_t nrec;
    const int64_t* XO;      // [found + 1] the texts' offsets (k_find_unframe)
    const uint8_t* X;       // the texts
    int64_t x_len;          // their bytes: XO[found]
    int64_t found;
    int64_t k;              // which match
    int64_t* src;           // [nrec] where entry i starts in X
    uint64_t* valid;        // [words] the bitmap
    int64_t words;          // ceil(nrec / 64)
    int64_t chunks;
    uint64_t* cnt;          // [2][chunks] strings with the match, the entries' bytes
    const uint64_t* base;   // [2][chunks + 1] their exclusive scans
    uint32_t* status;       // |= 1: the list offsets or the texts' offsets are not ordered (internal)
    uint8_t* out;           // [out_len]
    int64_t out_len;
    int64_t* out_off;       // [nrec + 1]
};

// the match k selects in string i, as its number j in the column; true when the string has it.  (c >= 0 > k: the sum cannot
// overflow, k is never negated, and L[i] + kk is formed only where kk < c)
TRRE_HD bool nth_index(const NthArgs& a, int64_t i, int64_t& j) {
    const int64_t l0 = a.L[i], c = a.L[i + 1] - l0;
    const int64_t kk = a.k >= 0 ? a.k : c + a.k;
    if (kk < 0 || kk >= c) return false;
    j = l0 + kk;
    return true;
}
// k_nth_plan: the string of thread tid in round r of chunk c
template <int THREADS>
TRRE_HD int64_t nth_plan_string(int64_t c, int r, int tid) { return (c * kNthPer + r) * THREADS + tid; }
// ... its verdict; src_i parked; c2 += (1, len_i) when it has the match; bad |= 1 when an array is out of order (the string
// then counts as without the match)
TRRE_HD bool nth_plan(const NthArgs& a, int64_t i, uint64_t (&c2)[2], uint32_t& bad) {
    const int64_t l0 = a.L[i], l1 = a.L[i + 1];
    int64_t j, x0 = 0, x1 = 0;
    bool has = false;
    if (l0 < 0 || l0 > l1 || l1 > a.found) {
        bad = 1;
    } else if (nth_index(a, i, j)) {
        x0 = a.XO[j]; x1 = a.XO[j + 1];
        has = x0 >= 0 && x0 <= x1 && x1 <= a.x_len;
        if (!has) bad = 1;
    }
    a.src[i] = has ? x0 : 0;
    if (has) { c2[0] += 1; c2[1] += (uint64_t)(x1 - x0); }
    return has;
}
TRRE_HD int64_t nth_len(const NthArgs& a, int64_t i) {
    int64_t j;
    return nth_index(a, i, j) ? a.XO[j + 1] - a.XO[j] : 0;
}
// k_nth_offsets: the bytes of the thread's kNthPer strings of chunk c
template <int THREADS>
TRRE_HD uint64_t nth_offsets_sum(const NthArgs& a, int64_t c, int tid) {
    uint64_t s = 0;
    const int64_t i0 = (c * THREADS + tid) * kNthPer;
    for (int64_t i = i0; i < i0 + kNthPer && i < a.nrec; ++i) s += (uint64_t)nth_len(a, i);
    return s;
}
// ... and their offsets; pre: the bytes of the chunk before the thread's strings
template <int THREADS>
TRRE_HD void nth_offsets_thread(const NthArgs& a, int64_t c, int tid, uint64_t pre) {
    int64_t o = (int64_t)(a.base[a.chunks + 1 + c] + pre);
    const int64_t i0 = (c * THREADS + tid) * kNthPer;
    if (i0 == 0) a.out_off[0] = 0;
    for (int64_t i = i0; i < i0 + kNthPer && i < a.nrec; ++i) {
        o += nth_len(a, i);
        a.out_off[i + 1] = o;
    }
}

// k_nth_emit
template <class G>
struct NthTile {
    int A;                  // the address of out mod 16
    int64_t o0, o1;         // the tile's output positions
    TRRE_HD NthTile(const NthArgs& a, int64_t b) {
        A = (int)(reinterpret_cast<uintptr_t>(a.out) & 15u);
        o0 = b * G::TILE - A > 0 ? b * G::TILE - A : 0;
        o1 = (b + 1) * G::TILE - A < a.out_len ? (b + 1) * G::TILE - A : a.out_len;
    }
};
// thread 0: the entries [win[0], win[1]] the tile touches — the entry that holds output position o (o < out_len) is the last i
// with out_off[i] <= o (out_off[0] = 0 <= o < out_len = out_off[nrec]: 0 <= i < nrec, and it has bytes)
template <class G>
TRRE_HD void nth_emit_window(const NthArgs& a, const NthTile<G>& t, int64_t* win) {
    win[0] = rec_lower_bound(SubPlaceKey{a.out_off}, a.nrec + 1, t.o0 + 1) - 1;
    win[1] = rec_lower_bound(SubPlaceKey{a.out_off}, a.nrec + 1, t.o1) - 1;
}
// all threads: out_off[win[0] .. win[1] + 1] into the image, when it fits
template <class G>
TRRE_HD void nth_keep_window(const NthArgs& a, const int64_t* win, int tid, int64_t* image) {
    const int64_t cnt = win[1] - win[0] + 2;
    if (cnt > kSubWindow) return;
    for (int64_t k = tid; k < cnt; k += G::THREADS) image[k] = a.out_off[win[0] + k];
}
// the thread's destination vectors of tile b
template <class G>
TRRE_HD void nth_emit_vecs(const NthArgs& a, const NthTile<G>& t, int64_t b, int tid, const int64_t* win, const int64_t* image) {
    const int64_t wcnt = win[1] - win[0] + 2;
    const SubPlaces pz{a.out_off, image, win[0], wcnt > kSubWindow ? 0 : wcnt};
    for (int j = 0; j < G::VECS; ++j) {
        const int64_t v = b * G::TILE + 16 * ((int64_t)j * G::THREADS + tid);
        const int64_t p0 = v - t.A > 0 ? v - t.A : 0, p1 = v + 16 - t.A < a.out_len ? v + 16 - t.A : a.out_len;
        if (p1 <= p0) continue;
        const int cnt = (int)(p1 - p0);
        int64_t i = sub_segment_in(pz, win[0], win[1], p0);
        int64_t beg = pz(i), end = pz(i + 1);
        uint8_t* d = a.out + p0;
        if (cnt == 16 && p0 + 16 <= end) {
            rec_store16(d, sub_load16u(a.X + a.src[i] + (p0 - beg)));
            continue;
        }
        U128 r;
        r.x = r.y = r.z = r.w = 0;
        int64_t o = p0;
        for (int f = 0;;) {
            const int take = end - o < cnt - f ? (int)(end - o) : cnt - f;
            const uint8_t* x = a.X + a.src[i] + (o - beg);
            for (int q = 0; q < take; ++q) str_put_byte(r, f + q, x[q]);
            f += take; o += take;
            if (f >= cnt) break;
            i = pz(i + 2) > o ? i + 1 : sub_segment_in(pz, i + 1, win[1], o);      // (o < out_len: entry i + 1 exists)
            beg = pz(i); end = pz(i + 1);
        }
        if (cnt == 16) {
            rec_store16(d, r);
        } else {
            for (int q = 0; q < cnt; ++q) d[q] = (uint8_t)filter_get_byte(r, q);
        }
    }
}

}  // namespace trre
