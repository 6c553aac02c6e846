// compile.cpp — the pattern compiler of the host runtime: a pattern becomes a trre_prog with its tables serialised for the device
// (device_blob.hpp), mode by mode; the compile and export entry points of the C ABI (include/trre_mi355x.h).  Host only: nothing
// here launches or allocates on a device.
#include <cstdio>
#include <cstring>

#include "runtime_state.hpp"
#include "device_blob.hpp"
#include "gen_block.hpp"
#include "guard_block.hpp"
#include "switches.hpp"

using namespace trre_host;

// the deterministic engine's tables one miss at a time (front.hpp: LazyDft): built on first need — a lazy-only program at compile time
int trre_host::lazy_ensure(trre_prog* p) {
    std::lock_guard<std::mutex> lock(p->lazy_mu);
    if (p->lazy) return TRRE_OK;
    try {
        trre::LazyLimits lim;
        if (const trre::SwitchNum mb = trre::lazy_max_bytes_now(); mb.set) lim.max_bytes = (size_t)mb.v;
        if (const trre::SwitchNum ss = trre::lazy_seed_states_now(); ss.set) lim.seed_states = (size_t)ss.v;
        p->lazy.reset(new trre::LazyDft(p->dft_nft, lim));
    } catch (const trre::Error& e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc&) {
        return fail(TRRE_E_TOO_BIG, "error: out of memory while determinising");
    }
    return TRRE_OK;
}

namespace {

void serialize_dft(trre_prog& p) {
    using namespace trre;
    const DftTables& t = p.dt;
    DftBlobHeader h{};
    h.magic = kMagicDft;
    h.n_rows = t.n_rows;
    h.n_cls = t.n_cls;
    h.flags = t.flags;
    h.max_edge_out = t.max_edge_out;
    h.n_states = t.n_states;
    size_t off = sizeof h;
    h.off_ent0 = (uint32_t)off; off += 256 * 8;
    h.off_cls = (uint32_t)off; off += 256;
    h.off_bytemap = (uint32_t)off; off += 256;
    h.off_ent = (uint32_t)off; off += t.ent.size() * 8;
    h.off_pool = (uint32_t)off; h.pool_bytes = (uint32_t)t.pool.size(); off += t.pool.size();
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    std::vector<uint8_t>& b = p.blob;
    b.assign(off, 0);
    std::vector<uint64_t> ent0(256);
    for (int c = 0; c < 256; ++c) ent0[c] = t.ent[t.cls[c]];      // row 0, expanded over raw bytes
    put(b, 0, &h, 1);
    put(b, h.off_ent0, ent0.data(), 256);
    put(b, h.off_cls, t.cls.data(), 256);
    put(b, h.off_bytemap, t.bytemap.data(), 256);
    put(b, h.off_ent, t.ent.data(), t.ent.size());
    put(b, h.off_pool, t.pool.data(), t.pool.size());
}

void serialize_nft(trre_prog& p) {
    using namespace trre;
    const NftTables& t = p.nt;
    NftBlobHeader h{};
    h.magic = kMagicNft;
    h.n_cons = t.n_cons;
    h.flags = t.flags;
    h.n_follow = (uint32_t)t.follow.size();
    h.n_states = t.n_states;
    size_t off = sizeof h;
    h.off_cons_mask = (uint32_t)off; off += 256 * 8;
    h.off_pred = (uint32_t)off; off += (t.n_cons + 1) * 8;
    h.off_follow_off = (uint32_t)off; off += align_up((t.n_cons + 2) * 4, 8);
    h.off_follow = (uint32_t)off; off += t.follow.size() * sizeof(NftFollow);
    h.off_pool = (uint32_t)off; h.pool_bytes = (uint32_t)t.pool.size(); off += t.pool.size();
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    std::vector<uint8_t>& b = p.blob;
    b.assign(off, 0);
    std::vector<uint64_t> pred(t.pred);
    pred.push_back(t.to_final);
    put(b, 0, &h, 1);
    put(b, h.off_cons_mask, t.cons_mask.data(), 256);
    put(b, h.off_pred, pred.data(), pred.size());
    put(b, h.off_follow_off, t.follow_off.data(), t.follow_off.size());
    put(b, h.off_follow, t.follow.data(), t.follow.size());
    put(b, h.off_pool, t.pool.data(), t.pool.size());
}

void serialize_stream(const trre::StreamTables& t, std::vector<uint8_t>& b) {
    using namespace trre;
    StreamBlobHeader h{};
    h.magic = kMagicStream;
    h.n_states = t.n_states;
    h.n_cls = t.n_cls;
    h.flags = t.flags;
    h.max_out = t.max_out;
    size_t off = sizeof h;
    h.off_cls = (uint32_t)off; off += 256;
    h.off_ent = (uint32_t)off; h.ent_bytes = (uint32_t)(t.ent.size() * 8); off += t.ent.size() * 8;
    h.off_pool = (uint32_t)off; h.pool_bytes = (uint32_t)t.pool.size(); off += t.pool.size();
    off = align_up(off, 16);
    h.off_lpw = (uint32_t)off; h.lpw_bytes = (uint32_t)(t.lpw.size() * 4); h.lpw_delay = t.lpw_delay; off += t.lpw.size() * 4;
    off = align_up(off, 16);
    h.off_g16 = (uint32_t)off; h.g16_bytes = (uint32_t)(t.g16.size() * 4); off += t.g16.size() * 4;
    off = align_up(off, 16);
    h.off_p32 = (uint32_t)off; h.p32_bytes = (uint32_t)(t.p32.size() * 4); h.p32_slow = t.p32_slow ? 1u : 0u; off += t.p32.size() * 4;
    off = align_up(off, 16);
    h.off_lpw2 = (uint32_t)off; h.lpw2_bytes = (uint32_t)(t.lpw2.size() * 4); off += t.lpw2.size() * 4;
    off = align_up(off, 16);
    if (t.fb_ok) {
        h.fb_slots = (uint32_t)t.fb_comb.size(); h.off_fb_comb = (uint32_t)off; off = align_up(off + t.fb_comb.size() * 8, 16);
        h.fb_lits = (uint32_t)t.fb_lit.size(); h.off_fb_lit = (uint32_t)off; off = align_up(off + t.fb_lit.size() * 8, 16);
        h.fb_escs = (uint32_t)t.fb_esc_slot.size(); h.off_fb_esc_slot = (uint32_t)off; off = align_up(off + t.fb_esc_slot.size() * 4, 16);
        h.off_fb_esc = (uint32_t)off; off = align_up(off + t.fb_esc.size() * 4, 16);
        h.off_fb_pool = (uint32_t)off; off = align_up(off + t.fb_pool.size(), 16);
        if (t.fb_copy_ok) { h.off_fb_lit_meta = (uint32_t)off; off = align_up(off + t.fb_lit_meta.size() * 2, 16); }
        if (t.fb_mark4_ok) {
            h.fb4_slots = (uint32_t)t.fb_comb4.size(); h.off_fb_comb4 = (uint32_t)off; off = align_up(off + t.fb_comb4.size() * 4, 16);
            h.fb4_dense = (uint32_t)t.fb_dense_base.size(); h.off_fb_dense4 = (uint32_t)off; off = align_up(off + t.fb_dense4.size() * 4, 16);
            h.off_fb_dense_base = (uint32_t)off; off = align_up(off + t.fb_dense_base.size() * 2, 16);
            h.fb_pad = t.fb_pad;
            std::memcpy(h.fb_start4, t.fb_start4, sizeof h.fb_start4);
        }
        std::memcpy(h.fb_start, t.fb_start, sizeof h.fb_start);
    }
    if (t.mg_max) { h.off_mg = (uint32_t)off; h.mg_max = t.mg_max; off = align_up(off + t.mg.size() * 4, 16); }
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    b.assign(off, 0);
    put(b, 0, &h, 1);
    if (t.mg_max) put(b, h.off_mg, t.mg.data(), t.mg.size());
    if (t.fb_ok) {
        put(b, h.off_fb_comb, t.fb_comb.data(), t.fb_comb.size());
        put(b, h.off_fb_lit, t.fb_lit.data(), t.fb_lit.size());
        put(b, h.off_fb_esc_slot, t.fb_esc_slot.data(), t.fb_esc_slot.size());
        put(b, h.off_fb_esc, t.fb_esc.data(), t.fb_esc.size());
        put(b, h.off_fb_pool, t.fb_pool.data(), t.fb_pool.size());
        if (t.fb_copy_ok) put(b, h.off_fb_lit_meta, t.fb_lit_meta.data(), t.fb_lit_meta.size());
        if (t.fb_mark4_ok) {
            put(b, h.off_fb_comb4, t.fb_comb4.data(), t.fb_comb4.size());
            put(b, h.off_fb_dense4, t.fb_dense4.data(), t.fb_dense4.size());
            put(b, h.off_fb_dense_base, t.fb_dense_base.data(), t.fb_dense_base.size());
        }
    }
    put(b, h.off_cls, t.cls.data(), 256);
    put(b, h.off_ent, t.ent.data(), t.ent.size());
    put(b, h.off_pool, t.pool.data(), t.pool.size());
    put(b, h.off_lpw, t.lpw.data(), t.lpw.size());
    put(b, h.off_g16, t.g16.data(), t.g16.size());
    put(b, h.off_p32, t.p32.data(), t.p32.size());
    put(b, h.off_lpw2, t.lpw2.data(), t.lpw2.size());
}

void serialize_rev_table(uint32_t n_rev, uint32_t n_cls, uint32_t sym_bits, const std::array<uint8_t, 256>& cls, const std::vector<uint8_t>& rev,
                         std::vector<uint8_t>& b) {
    using namespace trre;
    RevBlobHeader h{};
    h.magic = kMagicRev;
    h.n_rev = n_rev;
    h.n_cls = n_cls;
    h.sym_bits = sym_bits;
    size_t off = sizeof h;
    h.off_cls = (uint32_t)off; off += 256;
    h.off_tab = (uint32_t)off; off += align_up(rev.size(), 16);
    h.off_wide = (uint32_t)off; off += (size_t)n_rev * 256;
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    b.assign(off, 0);
    std::vector<uint8_t> wide((size_t)n_rev * 256);
    for (uint32_t r = 0; r < n_rev; ++r)
        for (int c = 0; c < 256; ++c) wide[(size_t)r * 256 + c] = rev[(size_t)r * n_cls + cls[c]];
    put(b, 0, &h, 1);
    put(b, h.off_cls, cls.data(), 256);
    put(b, h.off_tab, rev.data(), rev.size());
    put(b, h.off_wide, wide.data(), wide.size());
}
void serialize_rev(const trre::GuidedTables& g, std::vector<uint8_t>& b) {
    if (!g.wide) { serialize_rev_table(g.n_rev, g.n_cls, g.sym_bits, g.cls, g.rev, b); return; }
    // more than 256 states: 16-bit entries, [state][raw byte], read through L1 / L2 by k_rev_wide
    using namespace trre;
    RevBlobHeader h{};
    h.magic = kMagicRev;
    h.n_rev = g.n_rev;
    h.n_cls = g.n_cls;
    h.sym_bits = 16;
    size_t off = sizeof h;
    h.off_cls = (uint32_t)off; off += 256;
    h.off_tab = (uint32_t)off; off += align_up(g.rev16.size() * 2, 16);
    h.off_wide = (uint32_t)off; off += (size_t)g.n_rev * 256 * 2;
    off = align_up(off + 16, 16);
    h.total_bytes = (uint32_t)off;
    b.assign(off, 0);
    std::vector<uint16_t> wide((size_t)g.n_rev * 256);
    for (uint32_t r = 0; r < g.n_rev; ++r)
        for (int c = 0; c < 256; ++c) wide[(size_t)r * 256 + c] = g.rev16[(size_t)r * g.n_cls + g.cls[c]];
    put(b, 0, &h, 1);
    put(b, h.off_cls, g.cls.data(), 256);
    put(b, h.off_tab, g.rev16.data(), g.rev16.size());
    put(b, h.off_wide, wide.data(), wide.size());
}

// generator modes: follow lists (every epsilon path), the nodes' byte sets, the viability sets per symbol (gen_block.hpp)
void serialize_gen(const trre::GenTables& g, std::vector<uint8_t>& b) {
    using namespace trre;
    const NftNodes& nd = g.nodes;
    const uint32_t n_nodes = (uint32_t)nd.node.size();
    std::vector<uint32_t> bytes((size_t)n_nodes * 8, 0), foff, follow;
    std::vector<uint8_t> echo(n_nodes, 0), pool;
    for (uint32_t t = 0; t < n_nodes; ++t) {
        for (int c = 0; c < 256; ++c)
            if (nd.node[t].reads((uint8_t)c)) bytes[(size_t)t * 8 + (c >> 5)] |= 1u << (c & 31);
        echo[t] = nd.node[t].echo ? 1 : 0;
    }
    for (size_t l = 0; l < nd.follow.size(); ++l) {
        foff.push_back((uint32_t)(follow.size() / 3));
        for (const NodeFollow& e : nd.follow[l]) {
            if (e.out.size() > 0xffff) throw Error(kErrTooBig, "error: an output of more than 64 KiB on one epsilon path (generator mode)");
            follow.push_back(e.target);
            follow.push_back((uint32_t)pool.size());
            follow.push_back((uint32_t)e.out.size() | (e.mute ? 1u << 16 : 0u));
            pool.insert(pool.end(), e.out.begin(), e.out.end());
        }
    }
    foff.push_back((uint32_t)(follow.size() / 3));
    GenBlobHeader h{};
    h.magic = kMagicGen;
    h.n_nodes = n_nodes;
    h.n_rev = g.n_rev;
    h.words = g.viable_words;
    h.match_mode = g.match_mode ? 1u : 0u;
    h.n_follow = (uint32_t)(follow.size() / 3);
    size_t off = align_up(sizeof h, 16);
    h.off_bytes = (uint32_t)off; off = align_up(off + bytes.size() * 4, 16);
    h.off_echo = (uint32_t)off; off = align_up(off + echo.size(), 16);
    h.off_foff = (uint32_t)off; off = align_up(off + foff.size() * 4, 16);
    h.off_follow = (uint32_t)off; off = align_up(off + follow.size() * 4, 16);
    h.off_pool = (uint32_t)off; h.pool_bytes = (uint32_t)pool.size(); off = align_up(off + pool.size() + 8, 16);
    h.off_viable = (uint32_t)off; off = align_up(off + g.viable.size() * 8, 16);
    h.total_bytes = (uint32_t)off;
    b.assign(off, 0);
    put(b, 0, &h, 1);
    put(b, h.off_bytes, bytes.data(), bytes.size());
    put(b, h.off_echo, echo.data(), echo.size());
    put(b, h.off_foff, foff.data(), foff.size());
    put(b, h.off_follow, follow.data(), follow.size());
    put(b, h.off_pool, pool.data(), pool.size());
    put(b, h.off_viable, g.viable.data(), g.viable.size());
}

// the stack guard (guard_block.hpp): the NFT itself, for the lines long enough to exhaust the reference's stack — into the program whose
// scan runs first
void serialize_guard(trre_prog& into, const trre::Nft& nft, bool match) {
    using namespace trre;
    into.guard = build_guard(nft);
    if (!into.guard.on) return;
    GuardBlobHeader gh{};
    gh.magic = kMagicGuard;
    gh.n_states = (uint32_t)nft.st.size();
    gh.start = into.guard.start;
    gh.d = into.guard.d;
    gh.l_min = into.guard.l_min;
    gh.window = into.guard.window;
    gh.off_states = (uint32_t)sizeof gh;
    gh.total_bytes = (uint32_t)(sizeof gh + into.guard.states.size() * 4);
    gh.match = match ? 1u : 0u;
    gh.n_once = into.guard.n_once;
    for (int k = 0; k < 8; ++k) gh.bset[k] = into.guard.bset[k];
    put(into.kblob, 0, &gh, 1);
    put(into.kblob, gh.off_states, into.guard.states.data(), into.guard.states.size());
}

// The follow lists themselves as tables (gen_block.hpp: bt_lane).  Scan and match mode: the backtracking fallback runs what no table form
// holds — more than 64 nodes with a backward automaton beyond the guided limits and no fold (round 3: TRRE_E_UNSUPPORTED; match mode, round
// 4) — and can be asked for on any pattern (trre_set_kernel: the differential and parity tests do).  Find, spans and sub mode keep them so
// that trre_set_kernel can name that family and their calls can refuse it.
void serialize_bt_lists(trre_prog& p, const trre::NftNodes& nodes, bool match_mode = false) {
    trre::GenTables lists;
    lists.nodes = nodes;
    lists.match_mode = match_mode;
    lists.ok = true;
    serialize_gen(lists, p.nblob);
    p.bt_ok = true;
}

// A program inside another — find mode's marks, sub mode's texts: the outer one's engine and counts, a mode and guided tables of its own
// over the same nodes; a program of its own, with its own device state
std::unique_ptr<trre_prog> inner_program(const trre_prog& outer, int mode, trre::GuidedTables&& gt) {
    std::unique_ptr<trre_prog> in(new trre_prog);
    in->gt = std::move(gt);
    in->engine = outer.engine; in->mode = mode;
    in->nft_states = outer.nft_states; in->nft_cons = outer.nft_cons; in->nft_nodes = outer.nft_nodes;
    in->prints_newline = outer.prints_newline;
    serialize_stream(in->gt.fwd, in->gblob);
    serialize_rev(in->gt, in->rblob);
    return in;
}

// the modes that run on the guided tables alone
int beyond_guided(const char* mode) {
    return fail(TRRE_E_UNSUPPORTED, std::string("error: ") + mode + " mode runs on the guided tables, and this pattern is beyond their limits (a backward automaton of more than 16 384 states)");
}

// what the deterministic engine does not offer
int nft_only(int mode) {
    const char* spans_like = mode == TRRE_MODE_SUB ? "sub" : mode == TRRE_MODE_SPANS ? "spans" : mode == TRRE_MODE_FIND ? "find" : nullptr;
    if (spans_like)
        return fail(TRRE_E_UNSUPPORTED, std::string("error: ") + spans_like + " mode is offered for the non-deterministic engine only (the deterministic engine's matches cannot be told from its raw bytes by the reference)");
    if (mode == TRRE_MODE_MATCH)
        return fail(TRRE_E_UNSUPPORTED, "error: match mode is offered for the non-deterministic engine only (trre_dft -m prints empty lines)");
    if (is_generate(mode)) return fail(TRRE_E_UNSUPPORTED, "Not supported yet");   // trre_dft.c:1227-1229
    return TRRE_OK;
}

// ---- one function per mode: the tables of `p` from the pattern's NFT.  TRRE_OK, or what fail() gave; a trre::Error goes to compile_impl.

int compile_dft(trre_prog& p, const trre::Nft& nft) {
    using namespace trre;
    p.dft_nft = nft;
    std::unique_ptr<Dft> eager;
    try {
        eager.reset(new Dft(determinize(nft)));
    } catch (const Error& e) {
        if (e.code != kErrTooBig) throw;
        // The eager construction does not end within its caps — a state per run length ('((a:x)*b)|((a:y)*c)'), 2^19 states
        // ('(a|b)*a(a|b){18}:x').  The reference builds only the states its input visits (trre_dft.c:1135-1175) and so does
        // the lazy family (lazy_block.hpp; rounds 1-4: TRRE_E_TOO_BIG).
    }
    if (!eager) {
        p.lazy_only = true;
        return lazy_ensure(&p);       // (nothing else exists: no table for compile_impl to serialise)
    }
    Dft& dft = *eager;
    p.dt = flatten_dft(dft);
    serialize_dft(p);
    p.has_engine_tables = true;
    p.stt = build_stream_dft(dft);
    // the guided route (guided_build.cpp: GuidedDftBuilder): what a pattern whose scan loop does not fold runs on ('[a-z]+ing:X':
    // a loop before the decision), and what takes over when a bounded fold overflows ('a*b:x' behind a run of 65 a's) — the
    // tile kernels remain for tables beyond its limits.  (A byte map needs neither.)
    if (!(p.dt.flags & kFlagMemoryless)) p.gt = build_guided_dft(dft);
    return TRRE_OK;
}

// trre -a / -ma: every accepting path prints (generate.cpp): a viability DFA for the device, the lists for the host
int compile_generate(trre_prog& p, const trre::Nft& nft) {
    using namespace trre;
    p.gen = build_gen_tables(nft, p.mode == TRRE_MODE_MATCH_ALL);      // (always ok since round 5: beyond 256 viability states the filter lets everything through)
    p.nft_nodes = (uint32_t)p.gen.nodes.node.size();
    serialize_rev_table(p.gen.n_rev, p.gen.n_cls, 8, p.gen.cls, p.gen.rev, p.rblob);
    serialize_gen(p.gen, p.nblob);
    return TRRE_OK;
}

// trre -m: one attempt per line, accepted at its end only — the guided tables in match form; beyond their limits (a backward automaton
// of more than 16 384 states) the search itself in match form
int compile_match(trre_prog& p, const trre::Nft& nft) {
    using namespace trre;
    const NftNodes nodes = build_nft_nodes(nft, true);
    p.nft_nodes = (uint32_t)nodes.node.size();
    p.gt = build_guided_nft(nodes);
    serialize_bt_lists(p, nodes, true);
    serialize_guard(p, nft, true);
    return TRRE_OK;
}

// trre_find_device_strings: the scan loop's nodes under two forward tables over one backward DFA (guided_build.cpp: find_cell).
// This program keeps the texts table; the marks table lives in an inner program, which also carries the stack guard — its
// scan runs first.  Nothing else can run a find program: no tables, no find
int compile_find(trre_prog& p, const trre::Nft& nft) {
    using namespace trre;
    const NftNodes nodes = build_nft_nodes(nft);
    p.nft_nodes = (uint32_t)nodes.node.size();
    GuidedTables marks_gt;
    if (!build_guided_find(nodes, p.gt, marks_gt)) return beyond_guided("find");
    p.find_marks = inner_program(p, p.mode, std::move(marks_gt));
    serialize_bt_lists(p, nodes);
    serialize_guard(*p.find_marks, nft, false);
    return TRRE_OK;
}

// trre_span_device_strings: the scan loop's nodes under ONE forward table that prints markers and position bytes
// (guided_build.cpp: span_cell).  Nothing else can run a spans program: no other tables; the stack guard as in scan mode
int compile_spans(trre_prog& p, const trre::Nft& nft) {
    using namespace trre;
    const NftNodes nodes = build_nft_nodes(nft);
    p.nft_nodes = (uint32_t)nodes.node.size();
    p.gt = build_guided_spans(nodes);
    if (!p.gt.ok) return beyond_guided("spans");
    serialize_bt_lists(p, nodes);
    serialize_guard(p, nft, false);
    return TRRE_OK;
}

// trre_sub_device_strings: the scan loop's nodes, built once, under two tables: this program keeps the markers' table of spans
// mode and carries the stack guard — its scan runs first —; an inner program, held as find mode holds its marks program, keeps
// the texts table of find mode (the marks table built with it is dropped).  Nothing else can run a sub program
int compile_sub(trre_prog& p, const trre::Nft& nft) {
    using namespace trre;
    const NftNodes nodes = build_nft_nodes(nft);
    p.nft_nodes = (uint32_t)nodes.node.size();
    p.gt = build_guided_spans(nodes);
    GuidedTables texts_gt, marks_gt;
    if (!p.gt.ok || !build_guided_find(nodes, texts_gt, marks_gt)) return beyond_guided("sub");
    p.sub_texts = inner_program(p, TRRE_MODE_FIND, std::move(texts_gt));
    serialize_bt_lists(p, nodes);
    serialize_guard(p, nft, false);
    return TRRE_OK;
}

int compile_nft_scan(trre_prog& p, const trre::Nft& nft) {
    using namespace trre;
    // TRRE_TRACE=1: the stages of the NFT compile on stderr as they start (to find the one a pattern is slow in)
    auto trace = [&](const char* what) { if (switches().trace) fprintf(stderr, "compile: %s\n", what); };
    trace("nodes");
    const NftNodes nodes = build_nft_nodes(nft);
    p.nft_nodes = (uint32_t)nodes.node.size();
    trace("bitmask tables");
    try {
        p.nt = build_nft_tables(nodes);
        p.mask_bytes = p.nt.n_cons <= 8 ? 1 : p.nt.n_cons <= 16 ? 2 : p.nt.n_cons <= 32 ? 4 : 8;
        serialize_nft(p);
        p.has_engine_tables = true;
    } catch (const Error& e) {
        if (e.code != kErrUnsupported) throw;      // too many nodes (or an epsilon cycle) for the bitmask kernels: the other families run the pattern
    }
    // the fold walks the follow lists (TRRE_NFT_FOLD=states: the NFT's states as the reference does, =both: both, compared)
    const char* fold = nft_fold_now();
    trace("fold");
    if (fold && !strcmp(fold, "states")) {
        p.stt = build_stream_nft(nft);
    } else {
        p.stt = build_stream_nodes(nodes);
        if (fold && !strcmp(fold, "both")) {
            const StreamTables ref = build_stream_nft(nft);
            // (the walk over the states may run out of budget where this one does not: no table to compare then)
            if (ref.ok && !p.stt.ok) throw Error(kErrArg, "error: the fold over the follow lists gave up where the one over the states did not (TRRE_NFT_FOLD=both)");
            if (ref.ok)
            if (ref.ent != p.stt.ent || ref.pool != p.stt.pool || ref.cls != p.stt.cls || ref.flags != p.stt.flags ||
                ref.pending_len != p.stt.pending_len || ref.lpw != p.stt.lpw || ref.g16 != p.stt.g16 || ref.fb_comb != p.stt.fb_comb)
                throw Error(kErrArg, "error: the two folds of the NFT scan loop disagree (TRRE_NFT_FOLD=both)");
        }
    }
    trace("guided tables");
    p.gt = build_guided_nft(nodes);
    trace("done");
    serialize_bt_lists(p, nodes);
    serialize_guard(p, nft, false);
    return TRRE_OK;
}

int compile_impl(const std::string& pattern, int engine, trre_prog** out, int mode = TRRE_MODE_SCAN) {
    using namespace trre;
    if (!out) return fail(TRRE_E_ARG, "error: null output handle");
    *out = nullptr;
    if (engine != TRRE_ENGINE_NFT && engine != TRRE_ENGINE_DFT) return fail(TRRE_E_ARG, "error: unknown engine");
    if (mode != TRRE_MODE_SCAN && mode != TRRE_MODE_MATCH && mode != TRRE_MODE_FIND && mode != TRRE_MODE_SPANS && mode != TRRE_MODE_SUB && !is_generate(mode))
        return fail(TRRE_E_ARG, "error: unknown mode");
    if (engine != TRRE_ENGINE_NFT)
        if (const int rc = nft_only(mode)) return rc;
    try {
        std::unique_ptr<trre_prog> p(new trre_prog);
        p->engine = engine;
        p->mode = mode;
        Ast ast = parse_pattern(pattern);
        Nft nft = build_nft(ast, engine == TRRE_ENGINE_DFT);
        p->nft_states = (uint32_t)nft.st.size();
        p->nft_cons = (uint32_t)nft.n_cons;
        p->prints_newline = nft_prints_newline(nft);
        const int rc = engine == TRRE_ENGINE_DFT ? compile_dft(*p, nft)
                     : is_generate(mode)         ? compile_generate(*p, nft)
                     : mode == TRRE_MODE_MATCH   ? compile_match(*p, nft)
                     : mode == TRRE_MODE_FIND    ? compile_find(*p, nft)
                     : mode == TRRE_MODE_SPANS   ? compile_spans(*p, nft)
                     : mode == TRRE_MODE_SUB     ? compile_sub(*p, nft)
                                                 : compile_nft_scan(*p, nft);
        if (rc) return rc;
        if (p->stt.ok) serialize_stream(p->stt, p->sblob);
        if (p->gt.ok) { serialize_stream(p->gt.fwd, p->gblob); serialize_rev(p->gt, p->rblob); }
        if (p->gt.ok && !p->gt.accept.empty()) {
            std::vector<uint32_t> bits((p->gt.accept.size() + 31) / 32, 0u);
            for (size_t y = 0; y < p->gt.accept.size(); ++y)
                if (p->gt.accept[y]) bits[y >> 5] |= 1u << (y & 31);
            put(p->ablob, 0, bits.data(), bits.size());
        }
        *out = p.release();
        return TRRE_OK;
    } catch (const Error& e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc&) {
        return fail(TRRE_E_TOO_BIG, "error: out of memory while compiling the pattern");
    }
}

}  // namespace

extern "C" {

int trre_compile(const char* pattern, int engine, trre_prog** out) {
    if (!pattern) return fail(TRRE_E_ARG, "error: missing trre expression");
    return compile_impl(std::string(pattern), engine, out);
}

int trre_compile_bytes(const uint8_t* pattern, size_t len, int engine, trre_prog** out) {
    if (!pattern) return fail(TRRE_E_ARG, "error: missing trre expression");
    return compile_impl(std::string(reinterpret_cast<const char*>(pattern), len), engine, out);
}

int trre_compile_mode(const uint8_t* pattern, size_t len, int engine, int mode, trre_prog** out) {
    if (!pattern) return fail(TRRE_E_ARG, "error: missing trre expression");
    return compile_impl(std::string(reinterpret_cast<const char*>(pattern), len), engine, out, mode);
}

static size_t export_blob(const std::vector<uint8_t>& b, void* buf, size_t cap) {
    if (buf && cap && !b.empty()) std::memcpy(buf, b.data(), cap < b.size() ? cap : b.size());      // (an empty table has no data(): nothing to copy from)
    return b.size();
}
size_t trre_export_tables(const trre_prog* p, void* buf, size_t cap) { return p ? export_blob(p->blob, buf, cap) : 0; }
size_t trre_export_stream_tables(const trre_prog* p, void* buf, size_t cap) { return p ? export_blob(p->sblob, buf, cap) : 0; }

size_t trre_export_guided_tables(const trre_prog* p, int which, void* buf, size_t cap) {
    if (!p) return 0;
    if (which == 5 && p->sub_texts) return export_blob(p->sub_texts->gblob, buf, cap);      // (sub mode: the inner program's texts table)
    if (which == 5 || which == 6)                                     // (find mode: the texts / the marks forward tables; the backward DFA, 0, is one)
        return p->find_marks ? export_blob(which == 5 ? p->gblob : p->find_marks->gblob, buf, cap) : 0;
    if (which == 7) return p->mode == TRRE_MODE_SPANS || p->mode == TRRE_MODE_SUB ? export_blob(p->gblob, buf, cap) : 0;     // (spans mode: the markers' forward table)
    if (which == 3 && p->find_marks) return export_blob(p->find_marks->kblob, buf, cap);     // (find mode: the guard goes with the scan that runs first)
    if (which == 4) return export_blob(p->gt.accept, buf, cap);       // (match mode: a byte per backward state, 1: a line that starts with the symbol is accepted)
    return export_blob(which == 0 ? p->rblob : (which == 2 ? p->nblob : (which == 3 ? p->kblob : p->gblob)), buf, cap);   // (2: the enumeration's / the backtracking fallback's tables, 3: the stack guard's)
}

// CPU test tier (tests/cpu_shim.cpp runs lazy_block.hpp's lane body on the host): the lazy tables as they stand — which 0: u32 n_cls, u32 rows,
// then cls[256]; 1: the entries; 2: the pool — and the exploration of a list of misses.  Host only.
size_t trre_debug_lazy_tables(trre_prog* p, int which, void* buf, size_t cap) {
    if (!p || p->engine != TRRE_ENGINE_DFT || p->mode != TRRE_MODE_SCAN || lazy_ensure(p)) return 0;
    std::lock_guard<std::mutex> lock(p->lazy_mu);
    const trre::LazyDft& z = *p->lazy;
    std::vector<uint8_t> head;
    const void* src;
    size_t n;
    if (which == 0) {
        const uint32_t w[2] = {z.n_cls(), z.n_rows()};
        put(head, 0, w, 2);
        put(head, 8, z.cls(), 256);
        src = head.data(); n = head.size();
    } else if (which == 1) {
        src = z.ent(); n = (size_t)z.n_rows() * z.n_cls() * 8;
    } else {
        src = z.pool(); n = z.pool_bytes();
    }
    if (buf && cap) std::memcpy(buf, src, cap < n ? cap : n);
    return n;
}
int trre_debug_lazy_explore(trre_prog* p, const uint32_t* misses, size_t n, size_t spec_states) {
    if (!p || p->engine != TRRE_ENGINE_DFT || p->mode != TRRE_MODE_SCAN) return fail(TRRE_E_ARG, "error: no lazy tables");
    const int rc = lazy_ensure(p);
    if (rc) return rc;
    try {
        std::lock_guard<std::mutex> lock(p->lazy_mu);
        p->lazy->explore(misses, n, spec_states);
    } catch (const trre::Error& e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc&) {
        return fail(TRRE_E_TOO_BIG, "error: out of memory while determinising");
    }
    return TRRE_OK;
}

}  // extern "C"
