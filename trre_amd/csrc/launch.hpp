// launch.hpp — host-callable launchers implemented in scan_kernels.hip.
#pragma once
#include <cstdint>

namespace trre {

struct ScanArgs;
struct FbCopyArgs;
struct GenArgs;
struct GuardArgs;
struct LazyArgs;
struct OneArgs;
struct MapGenArgs;
struct RecArgs;
struct StrArgs;
struct MatchArgs;
struct SpanArgs;
struct SplitArgs;
struct FilterArgs;
struct FieldArgs;
struct SplitnArgs;
struct FieldnArgs;
struct TrimArgs;
struct SubArgs;
struct NthArgs;

constexpr int kEngineNft = 0, kEngineDft = 1;

// bytes of input owned by one workgroup / threads per workgroup for an engine
int chunk_bytes(int engine, int mask_bytes);
int block_threads(int engine, int mask_bytes);

// which: 0 length-preserving scan, 1 count pass, 2 emit pass
void launch_tile_kernel(int which, int engine, int mask_bytes, const ScanArgs& a, int64_t n_chunks, void* stream);
// stream families (tables from stream_build.cpp): the direct kernels — a lane walks a long sub-range straight from memory; which: 1 count, 2 emit
// (0: the in-place ring walker, kept for the window kernel's redo lanes only)
int direct_ent_lds_bytes();
int direct_block_threads();
// sym: guided families — columns are the symbols of the backward pass (a.sym_v0): 1 one per byte, 2 packed two per byte
// (16-byte entries only)
void launch_direct_kernel(int which, bool ent_in_lds, const ScanArgs& a, int64_t lane_bytes, int64_t n_blocks, void* stream, int g16_bytes = 0,
                          int sym = 0, bool g16_slow = true);
// the one-pass form of the general families on small tables (one_block.hpp: one walk, the workgroup's output in LDS, look-back for its place);
// oa.desc / oa.ticket zeroed by the caller; -1: the tables and regions do not fit the LDS
int launch_one(const ScanArgs& a, const OneArgs& oa, void* stream, int g16_bytes, int sym, bool g16_slow);
// memoryless programs of any output length in one pass (map_block.hpp); a.blob: the stream blob with its mg table; oa's arrays zeroed by the caller;
// -1: the window does not fit the LDS
int launch_mapgen(const ScanArgs& a, const MapGenArgs& oa, void* stream);
// backward pass of the guided families: fills a.sym_v0 for positions [0 .. round_up(a.vend, 64)) (packed: round_up(.., 128), two per byte)
void launch_rev_sweep(const ScanArgs& a, int tab_bytes, int64_t lane_bytes, void* stream, bool packed);
// wide guided tables (more than 256 backward states: 16-bit symbols at a.sym_v0, both tables through L1 / L2); which: 1 count, 2 emit
void launch_rev_wide(const ScanArgs& a, int64_t lane_bytes, void* stream);
void launch_wide_fwd(int which, const ScanArgs& a, int64_t lane_bytes, int64_t n_blocks, void* stream);
void launch_lpw_kernel(int ent_bytes, bool wide, bool direct_ent_in_lds, const ScanArgs& a, int64_t lane_bytes, void* stream, int pair_bytes = 0);
// count / emit passes over the fallback form of a large table (StreamTables::fb_*); hdr: the host's copy of the stream
// blob's header.  Chunks are those of the direct kernels (direct_block_threads() lanes each).
void launch_fb_kernel(int which, const ScanArgs& a, const void* hdr, int64_t lane_bytes, int64_t n_chunks, void* stream);
bool fb_fits(const void* hdr);
// the copy form of a large table (scan_block.hpp): mark pass (count + events); the second pass is the splice below
void launch_fb_mark(const ScanArgs& a, const FbCopyArgs& ca, const void* hdr, int64_t lane_bytes, int64_t n_chunks, void* stream);
bool fb_copy_fits(const void* hdr);
// ... its second pass as a wave-cooperative splice (splice_block.hpp); the workspace's chunks must be full (the mark pass fills every lane's header)
void launch_fb_splice(const ScanArgs& a, const FbCopyArgs& ca, const void* hdr, int64_t lane_bytes, int64_t n_chunks, void* stream);
bool fb_splice_fits(const void* hdr);
// generator modes (gen_block.hpp): which 1 count, 2 emit; a.blob = the tables of serialize_gen (runtime.cpp), chunks of 256 lanes
void launch_gen(int which, const ScanArgs& a, const GenArgs& ga, int64_t lane_bytes, int64_t n_chunks, void* stream);
// the stack guard (guard_block.hpp): flags = a bit per window of `window` bytes without a '\n' (u64 per 64 windows, room for a multiple
// of 256 windows); then the reference's search on the lines that cover the runs of such windows — `slots` stacks, a thread each
void launch_guard_probe(const ScanArgs& a, int64_t window, int64_t n_windows, uint64_t* flags, void* stream);
void launch_guard(bool out, const ScanArgs& a, const GuardArgs& ga, int64_t n_runs, int64_t slots, void* stream);
// the backtracking fallback (gen_block.hpp: bt_lane): which 1 count, 2 emit; pool_blocks workgroups of 256 threads take the chunks in turn (ga holds
// pool_blocks * 256 stacks and path buffers)
void launch_bt(int which, const ScanArgs& a, const GenArgs& ga, int64_t lane_bytes, int64_t n_chunks, int64_t pool_blocks, uint32_t budget, void* stream);
// the deterministic engine on tables still being built (lazy_block.hpp): which 1 count (lanes whose lane_counts entry is not kLazyVoid keep
// it), 2 emit (leaves at once when the count pass was not final); chunks of 256 lanes
void launch_lazy(int which, const ScanArgs& a, const LazyArgs& la, int64_t lane_bytes, int64_t n_chunks, void* stream);
// exact sub-ranges (scan_block.hpp: ScanArgs::exact): flags the lanes whose guessed entry state is not the exit state of the lane before
// them (a.spec_flags, a.status[3] counts them); the repair round is launch_direct_kernel(1, ...) with a.exact == 3
void launch_spec_verify(const ScanArgs& a, int64_t n_lanes, void* stream);
// ... and of the backward pass: a.rev_guess against the symbols the lanes to the right left (a.rev_flags, a.status[2] counts the wrong ones); the
// flagged lanes sweep again (and on to the left while their result is not what was assumed there)
void launch_rev_verify(const ScanArgs& a, int64_t lane_bytes, void* stream, bool packed);
void launch_rev_repair(const ScanArgs& a, int64_t lane_bytes, void* stream, bool packed);
// 4 096 samples: how many find no '\n' within `window` bytes (added to *out)
void launch_line_probe(const ScanArgs& a, int64_t window, uint32_t* out, void* stream);
void launch_chunk_scan(const uint64_t* total, uint64_t* base, int64_t n_chunks, void* stream);
void launch_bytemap(const ScanArgs& a, void* stream);
void launch_nul_eol(const uint8_t* in, int64_t n, const uint64_t* pos, uint64_t* eol, uint32_t count, void* stream);
// ragged records (records_block.hpp): bytes per tile; the offsets' check (status |= 1 when bad); the first record of every
// tile (side 0: by end offset over the input's tiles, 1: by rank over the output's); staging; ranks; the output's '\n' per
// tile; the output offsets (status |= 1 when a rank falls outside its tile); the replaced bytes back into dst
int64_t rec_tile_bytes();
void launch_rec_check(const int64_t* off, int64_t nrec, int64_t n, uint32_t* status, void* stream);
void launch_rec_part(int side, const RecArgs& a, int64_t tiles, void* stream);
void launch_rec_stage(const RecArgs& a, int64_t tiles, void* stream);
void launch_rec_rank(const RecArgs& a, void* stream);
void launch_rec_count(const RecArgs& a, int64_t tiles, void* stream);
void launch_rec_locate(const RecArgs& a, int64_t tiles, uint32_t* status, void* stream);
void launch_rec_restore(const RecArgs& a, uint8_t* dst, void* stream);
// packed strings (records_block.hpp): bytes per tile; the first record of every tile (side 0: by the staged position of its
// closing '\n', 1: by the framed position); the staged text, its '\n' per tile and the tile-local ranks; the ranks; the
// compaction of the framed output into the caller's buffer, with the final offsets
int64_t str_tile_bytes();
void launch_str_part(int side, const StrArgs& a, int64_t* part, int64_t tiles, void* stream);
void launch_str_stage(const StrArgs& a, int64_t tiles, void* stream);
void launch_str_rank(const StrArgs& a, void* stream);
void launch_str_unframe(const StrArgs& a, int64_t tiles, void* stream);
// matched strings (records_block.hpp): the verdicts (sym_bits: 4, 8 or 16, the layout of the symbols), their bitmap, the local ranks and the
// groups' counts; the ranks; the final offsets; '\n' per tile of the compaction (the strings' tiles); the compaction that drops every '\n'
// (a.part: the '\n' before every tile)
void launch_match_verdict(int sym_bits, const MatchArgs& a, void* stream);
void launch_match_rank(const MatchArgs& a, void* stream);
void launch_match_final(const MatchArgs& a, void* stream);
void launch_match_count(const RecArgs& a, int64_t tiles, void* stream);
void launch_match_unframe(const StrArgs& a, int64_t tiles, void* stream);
// found strings (records_block.hpp): launch_match_unframe's compaction and the matches' offsets (a.part: the '\n' before every tile,
// a.out_off: match_off, a.nrec: the number of matches)
void launch_find_unframe(const StrArgs& a, int64_t tiles, void* stream);
// match spans (records_block.hpp): the markers per framed tile (a.cnt), then — behind the three exclusive scans — the spans and
// the list offsets (a.tiles tiles each)
void launch_span_count(const SpanArgs& a, void* stream);
void launch_span_emit(const SpanArgs& a, void* stream);
// split strings (records_block.hpp), behind launch_span_count and its scans: the kept bytes per framed tile (a.kcnt), then — behind
// their exclusive scan — the pieces' bytes, the piece offsets and the list offsets
void launch_split_count(const SplitArgs& a, void* stream);
void launch_split_emit(const SplitArgs& a, void* stream);
// filtered strings (records_block.hpp), behind launch_span_emit's list offsets: the first string of every tile of the input
// (a.part) and the kept strings and bytes per tile (a.cnt), then — behind their two exclusive scans — the kept strings' bytes,
// their offsets and their rows (a.tiles tiles of str_tile_bytes() each)
void launch_filter_count(const FilterArgs& a, void* stream);
void launch_filter_emit(const FilterArgs& a, void* stream);
// field k of every string (records_block.hpp), behind launch_span_emit's list offsets: the bitmap and the fields' bounds (a.lo,
// a.hi; sp: the span call's tiles of the framed text); over the filter call's tiles of the input the first string of every tile
// and the strings with the field and the field bytes per tile; then — behind their two exclusive scans — the fields' bytes and
// their offsets
void launch_field_bounds(const SpanArgs& sp, const FieldArgs& a, void* stream);
void launch_field_count(const FieldArgs& a, void* stream);
void launch_field_emit(const FieldArgs& a, void* stream);
// split at the first or last matches only (records_block.hpp), behind launch_span_count with its scans and launch_span_emit's list
// offsets (a.L): the kept bytes and the cutting matches per framed tile (a.s.kcnt [2][tiles]), then — behind their two exclusive
// scans (a.s.kbase) — the pieces' bytes, the piece offsets and the list offsets
void launch_splitn_count(const SplitnArgs& a, void* stream);
void launch_splitn_emit(const SplitnArgs& a, void* stream);
// field k of that split: launch_field_bounds and launch_field_count with the limited index arithmetic; the emit pass is
// launch_field_emit(a.a)
void launch_fieldn_bounds(const SpanArgs& sp, const FieldnArgs& a, void* stream);
void launch_fieldn_count(const FieldnArgs& a, void* stream);
// trimmed strings (records_block.hpp), behind launch_span_emit's list offsets: the words the markers of every string's first and
// last two matches park (a.marks; sp: the span call's tiles of the framed text), then every string's bounds from them (a.a.lo,
// a.a.hi, a.begin, a.end); the count and emit passes are launch_field_count(a.a) and launch_field_emit(a.a)
void launch_trim_bounds(const SpanArgs& sp, const TrimArgs& a, void* stream);
// replaced strings (records_block.hpp), behind launch_span_emit's spans and list offsets and launch_find_unframe's texts: the
// selection bits and the selected matches, texts' bytes and matched bytes per chunk of sub_chunk_matches() matches (a.cnt; a.status
// |= 1 when the arrays are out of order); then — behind their three exclusive scans — where every segment starts; the output
// offsets; the outputs' bytes (nothing is launched for an empty output)
int64_t sub_chunk_matches();
void launch_sub_plan(const SubArgs& a, void* stream);
void launch_sub_place(const SubArgs& a, void* stream);
void launch_sub_offsets(const SubArgs& a, void* stream);
void launch_sub_emit(const SubArgs& a, void* stream);
// match k of every string (records_block.hpp), behind the find call's list offsets and launch_find_unframe's texts: the bitmap, the
// entries' sources and the strings with the match and the entries' bytes per chunk of nth_chunk_strings() strings (a.cnt; a.status
// |= 1 when the arrays are out of order); then — behind their two exclusive scans — the output offsets; the entries' bytes
// (nothing is launched for an empty output)
int64_t nth_chunk_strings();
void launch_nth_plan(const NthArgs& a, void* stream);
void launch_nth_offsets(const NthArgs& a, void* stream);
void launch_nth_emit(const NthArgs& a, void* stream);
void launch_bytemap_shift(const uint8_t* blob, const uint8_t* src, uint8_t* dst, int64_t len, bool nl, void* stream);

}  // namespace trre
