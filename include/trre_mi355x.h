/*
 * trre_mi355x.h — C ABI of the MI355X-native transducer scan engine.
 *
 * Drop-in boundary for the scan-mode hot path of c0stya/trre.  The reference
 * has no library interface: both engines are main() programs whose only seam
 * is the per-position call inside the scan line loop
 *
 *     ioffset = infer_backtrack(start, ch, stack, mode, all);   trre_nft.c:781
 *     ioffset = infer_dft(dstart, (unsigned char*)ch, dcache, mode);  trre_dft.c:1278
 *
 * (contract: NUL-terminated bytes in -> bytes appended to stdout, returns the
 * number of bytes consumed or <= 0).  One device call per input position is
 * far too fine a grain, so the boundary sits one level up: a whole
 * '\n'-delimited input buffer in, the whole output buffer out, same per-line
 * function, i.e. what main()'s scan branch computes for a FILE
 * (trre_nft.c:775-790, trre_dft.c:1272-1286).  INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Plain C types only.  The scan itself always runs on the GPU; there is no CPU
 * fallback in this library (a missing/failed device is an error).
 */
#ifndef TRRE_MI355X_H
#define TRRE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* engines: which reference binary's semantics to reproduce */
#define TRRE_ENGINE_NFT 0 /* ./trre      priority backtracking, trre_nft.c:593-657 */
#define TRRE_ENGINE_DFT 1 /* ./trre_dft  shortest-match determinised, trre_dft.c:1110-1196 */

/* modes: which branch of the reference's main() to reproduce */
#define TRRE_MODE_SCAN 0  /* default: every line is scanned for matches, the rest is copied (trre_nft.c:775-790) */
#define TRRE_MODE_MATCH 1 /* `trre -m`: the whole line must match; its output and '\n' are printed, a line that does not
                             match prints nothing (trre_nft.c:791-797, 635-642).  NFT engine only: the reference's
                             trre_dft -m prints an empty line per record (its emit is commented out, trre_dft.c:1185-1190) */
#define TRRE_MODE_SCAN_ALL 2  /* `trre -a` (generator mode, trre_nft.c:736-738 with 647-648): at every position of a line the
                                 outputs of ALL accepting paths that start there are printed, in the search's depth-first
                                 priority order, then that position's raw byte (no attempt returns a match: trre_nft.c:780-786) */
#define TRRE_MODE_MATCH_ALL 3 /* `trre -ma` (what the reference's own test.sh runs, test.sh:4): one output + '\n' per path
                                 that accepts at the end of the line (trre_nft.c:635-642).
                                 Both generator modes: NFT engine only (trre_dft -a prints "Not supported yet",
                                 trre_dft.c:1227-1229).  The amount of output is unbounded in the input; the device computes
                                 the viability filter (one symbol per input byte: which nodes have an accepting or a
                                 non-terminating continuation) and, since round 4, enumerates the accepting paths itself —
                                 count, exclusive sum, emit: trre_amd/csrc/gen_block.hpp —; the host enumeration of round 3
                                 (trre_amd/csrc/generate.cpp) takes a chunk on which a path never returns or a search
                                 outgrows a lane's stack. */
#define TRRE_MODE_FIND 4 /* every match of every string, the rest thrown away (findall, grep -o): the outputs of the scan loop's
                          * successful attempts (trre_nft.c:775-790) as a list per string.  NFT engine only; runs through
                          * trre_find_device_strings and nothing else */
#define TRRE_MODE_SPANS 8 /* where every match of every string starts and ends (finditer().span(), str.find, str.count): the positions
                           * of the same attempts, nothing of what they print.  NFT engine only; runs through
                           * trre_span_device_strings, trre_split_device_strings, trre_filter_device_strings,
                           * trre_field_device_strings, trre_splitn_device_strings, trre_fieldn_device_strings,
                           * trre_trim_device_strings and nothing else.  (8, not 5: 5, 6 and 7 read as sums of the modes above and
                           * stay TRRE_E_ARG, as they were) */
#define TRRE_MODE_SUB 16 /* the first n matches of every string replaced by what they print, the rest of the string kept
                          * (sed 's/x/y/', re.sub(p, r, s, count), str.replace(p, r, n)): the spans table and the texts table over the
                          * same attempts.  NFT engine only; runs through trre_sub_device_strings and nothing else */

/* return codes */
#define TRRE_OK 0
#define TRRE_E_SYNTAX (-1)      /* the reference prints "error: ..." and exits 1 (message kept) */
#define TRRE_E_UNDEFINED (-2)   /* the reference reads outside its buffers on this pattern */
#define TRRE_E_EPS_CYCLE (-3)   /* epsilon cycle: the reference recurses without bound (DFT) */
#define TRRE_E_TOO_BIG (-4)     /* DFT engine, at run time: the determinised states THIS INPUT visits do not fit the memory limit of the lazy
                                   tables (TRRE_LAZY_MAX_BYTES, 16 GiB; the reference keeps every state it meets, too).  Rounds 1-4 returned it
                                   at compile time for every pattern beyond the eager construction's caps. */
#define TRRE_E_UNSUPPORTED (-5) /* legal pattern, outside this engine's GPU limits (modes other than scan: a backward DFA beyond the guided
                                   families' limits; scan mode, NFT engine, at run time: an attempt beyond the backtracking fallback's limits) */
#define TRRE_E_DEVICE (-6)      /* HIP runtime failure / no GPU */
#define TRRE_E_ARG (-7)
#define TRRE_E_DIVERGES (-8)    /* the reference does not survive this input: an epsilon cycle is entered (NFT: "error: stack max
                                   capacity reached", exit 1; DFT: unbounded recursion, SIGSEGV).  NFT engine: the reference exits
                                   with everything it had printed so far — the lines before the bad one and the bad line's output up
                                   to the attempt that does not return (trre_nft.c:551-553, exit() flushes stdout) — and so does the
                                   scan: those bytes are in the output buffer and *out_len is their count.  DFT engine: the
                                   reference's buffered output dies with it; *out_len = 0.  The same error, with the same bytes, when
                                   an attempt of the NFT engine's search would hold more than 65 536 untried alternatives
                                   (trre_nft.c:35-36,548-556: a greedy loop over a run of 65 536 bytes): the stack guard (round 4;
                                   rounds 1-3 printed the match) finds the lines long enough for that and runs the reference's search
                                   on them, scan and match modes; TRRE_NO_STACK_GUARD=1 switches it off.  Not decided, and left as
                                   the table kernels print it: a line whose search takes more than 8 M steps (TRRE_GUARD_BUDGET), the
                                   suspect lines behind the first 2^35 steps of such searches in one call (TRRE_GUARD_CALL_BUDGET) —
                                   step counts, not a clock (round 4: 20 s): the same input gives the same answer whatever the host is
                                   busy with, and the call SAYS so: TRRE_SCAN_GUARD_UNDECIDED in trre_last_scan_flags() —, patterns
                                   whose loops nest more than 64 first-tried branches between two reads, generator modes */
#define TRRE_E_CAPACITY (-9)    /* output buffer too small; *out_len holds the size needed */

/* kernel families (trre_info.kernel, trre_set_kernel) */
#define TRRE_KERNEL_AUTO 0
#define TRRE_KERNEL_BYTEMAP 1   /* memoryless tables: streaming byte map */
#define TRRE_KERNEL_TILE_LP 2   /* length-preserving tables: one lane per line, single launch */
#define TRRE_KERNEL_TILE_GEN 3  /* any tables: count + scan + emit */
#define TRRE_KERNEL_STREAM_LP 4 /* scan loop folded into the tables, length-preserving: output at the input's positions, single launch */
#define TRRE_KERNEL_STREAM_GEN 5 /* scan loop folded into the tables, any output length: count + scan + emit */
#define TRRE_KERNEL_GUIDED_LP 6  /* NFT engine, any pattern (round 4: DFT engine too, any pattern that is not a byte map): backward DFA sweep (one symbol per byte) + guided forward transducer, output at the input's positions */
#define TRRE_KERNEL_GUIDED_GEN 7 /* the same, any output length: backward sweep, count + scan + emit */

#define TRRE_KERNEL_GENERATE 8    /* generator modes: backward viability sweep and enumeration (count, exclusive sum, emit) on the device;
                                     a chunk on which a path never returns or a search outgrows a lane's stack: the host enumeration */

#define TRRE_KERNEL_BACKTRACK 9   /* NFT engine, scan mode, any pattern: the reference's depth-first search itself, a lane per sub-range with an
                                     explicit stack (round 4).  What a pattern beyond the limits of every other family runs on (round 3:
                                     TRRE_E_UNSUPPORTED); exponential where the reference is.  A 1 KiB sub-range whose search takes more than 16 M steps, an
                                     attempt that consumes more than 4 096 bytes or builds more than 4 KiB of output: TRRE_E_UNSUPPORTED at run time */

#define TRRE_KERNEL_DFT_LAZY 10   /* DFT engine, scan mode, any pattern: determinisation on the fly as in the reference (trre_dft.c:1135-1175) — a lane per
                                     sub-range walks the rows that exist, an edge nobody has explored yet is listed and built on the host, the lanes that met
                                     it run again (round 5).  What a pattern beyond the eager construction's caps runs on ('((a:x)*b)|((a:y)*c)',
                                     '(a|b)*a(a|b){18}:x'; rounds 1-4: TRRE_E_TOO_BIG at compile time) */

typedef struct trre_prog trre_prog;

typedef struct trre_info {
    int32_t engine;
    int32_t kernel;            /* family AUTO resolves to */
    uint32_t nft_states;       /* states of the compiled NFT (trre_nft.c:334-340) */
    uint32_t nft_cons_states;
    uint32_t dft_states;       /* determinised states incl. final ones (DFT engine) */
    uint32_t table_rows;       /* rows kept on the device (non-final states) */
    uint32_t table_classes;    /* byte classes (columns) */
    uint32_t table_bytes;      /* size of the device blob */
    uint32_t flags;            /* bit0 length-preserving, bit1 memoryless, bit2 no-overrun */
    uint32_t chunk_bytes;      /* input bytes owned by one workgroup */
    uint32_t stream_states;    /* states of the folded scan transducer (0 = pattern does not fold) */
    uint32_t stream_classes;
    uint32_t nft_nodes;         /* consuming nodes of the NFT engine's tables (a byte range is one node) */
    uint32_t guided_rev_states; /* states of the backward DFA of the guided families (0 = not available) */
    uint32_t guided_fwd_states;
} trre_info;

/* Replaces parse() + create_nft() (trre_nft.c:752-754) and, for the DFT engine,
 * the lazy table construction of infer_dft (trre_dft.c:1135-1175) run to
 * completion.  Host-only; no GPU needed.  On failure returns a negative code
 * and *out = NULL; trre_last_error() then holds the reference's stderr text. */
int trre_compile(const char* pattern, int engine, trre_prog** out);
int trre_compile_bytes(const uint8_t* pattern, size_t len, int engine, trre_prog** out);
int trre_compile_mode(const uint8_t* pattern, size_t len, int engine, int mode, trre_prog** out);
void trre_free(trre_prog* p);
const char* trre_last_error(void); /* thread-local */
int trre_get_info(const trre_prog* p, trre_info* info);
int trre_set_kernel(trre_prog* p, int kernel_family); /* force a family (benchmarks/tests) */

/* Copy of the device table blob (for offline inspection and the host-side table
 * tests).  Returns the blob size; copies min(size, cap) bytes. */
size_t trre_export_tables(const trre_prog* p, void* buf, size_t cap);
size_t trre_export_stream_tables(const trre_prog* p, void* buf, size_t cap); /* 0 if the pattern does not fold */
size_t trre_export_guided_tables(const trre_prog* p, int which, void* buf, size_t cap); /* which: 0 backward DFA, 1 forward tables, 4 (match mode) a byte per backward state: 1 where a line that starts with that symbol is accepted, 5 / 6 (find mode) the texts / the marks forward tables, both over the backward DFA of 0, 7 (spans mode) the markers' forward table, over the backward DFA of 0; a sub program answers 0 and 7 as a spans program and 5 with its inner texts table; 0 if none */

/* Replaces the scan branch of main() (trre_nft.c:775-790 / trre_dft.c:1272-1286)
 * for a whole buffer that is already resident in HBM.
 *   d_in/d_out : device pointers (any alignment; 16-byte aligned is the fast path)
 *   n          : input bytes        cap : capacity of d_out in bytes
 *   out_len    : bytes produced (or needed, with TRRE_E_CAPACITY)
 *   stream     : hipStream_t (NULL = default stream)
 * Semantics, byte for byte: output = concat over getline() records of
 * scan_line(record minus its last byte, cut at the first NUL) + "\n".
 * Synchronous with respect to `stream` on return.
 * Aliasing: d_in == d_out (a scan in place) is valid for every family and mode, with any cap that holds the
 * output, and gives byte for byte what separate buffers give (the scan reads a device copy of the input:
 * n more bytes of device memory and one device-to-device copy per call).  Any other overlap of
 * [d_in, d_in + n) and [d_out, d_out + cap) returns TRRE_E_ARG before the device is touched: nothing is
 * launched or written.  In place, TRRE_E_CAPACITY leaves the first n bytes holding the input, so the size
 * query and a retry from the same buffer work; TRRE_E_DIVERGES leaves the reference's partial output and
 * *out_len its length, as with separate buffers. */
int trre_scan_device(trre_prog* p, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, size_t* out_len,
                     void* stream);

/* Ragged records: a batch of separate strings held as one packed byte buffer plus int64 offsets (Arrow string columns,
 * torch.nested, HF datasets).  Record i is d_in[d_off[i] .. d_off[i+1]) for i < nrec; d_off (nrec + 1 entries, device memory)
 * starts at 0, ends at n and never decreases.  Record i's output is exactly what trre_scan_device gives for that record alone,
 * i.e. what the reference prints for it as its input file (printf '%s' "$rec" | trre P); the outputs are concatenated into
 * d_out, and d_out_off[i] (nrec + 1 entries, device memory) is where record i's output starts, d_out_off[nrec] = *out_len.
 * The reference's framing holds per record: a record may hold several lines; a record whose last byte is not '\n' loses that
 * byte and still prints a '\n' (printf 'abc' | trre 'c:X' prints "ab\n", as for "ab\n"); an empty record prints nothing; a NUL
 * cuts its line.  nrec == 0 is valid with n == 0 (d_out_off[0] = 0); n == 0 makes every record empty.
 * How: a copy of the input whose records' last bytes are '\n' is scanned as it stands (same family, same kernels), and every
 * line prints exactly one framing '\n', so record i's output ends just past the output newline that ends its last line.
 * Refused with TRRE_E_UNSUPPORTED before the device is touched: match and generator modes (a line prints zero or many
 * newlines there) and a program that can print a '\n' of its own (a raw newline on the output side, an output range over
 * 0x0a; byte copies such as '.', '[a-z]', '[a:A-z:Z]' are taken).  Bad offsets (checked on the device, one status word
 * read back): TRRE_E_ARG, nothing written to d_out or d_out_off.  Any overlap of d_off or d_out_off with the data buffers or
 * with each other: TRRE_E_ARG; d_in / d_out as for trre_scan_device (d_in == d_out, in place, is valid).  TRRE_E_CAPACITY:
 * *out_len is the size needed, d_out_off is unspecified, in place the first n bytes hold the input again: a retry with the
 * same arguments works.  TRRE_E_DIVERGES: d_out and *out_len are what the scan of all records gives — the outputs of the
 * records before the failing one and the failing record's partial output; d_out_off is unspecified.  A split-form scan
 * still in flight on this (prog, device): TRRE_E_ARG.  Synchronous with respect to `stream`; trre_last_scan_flags as for
 * trre_scan_device.  Device memory: n + 32 bytes of staging and 24 bytes per 64 KiB of input and of output. */
int trre_scan_device_records(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out,
                             size_t cap, int64_t* d_out_off, size_t* out_len, void* stream);

/* Packed strings: the same packed buffer plus offsets, but record i is the CONTENT of one input line, its line end left off,
 * which is what a column of strings holds (Arrow large_string, torch.nested values + offsets, a HF dataset column):
 *     out_i = R(rec_i + "\n") without its last byte,
 * R being what the reference prints for that input file.  Whatever the program prints for the line ends in exactly one
 * framing '\n', and that byte is removed: "cat" under [a:A-z:Z] gives "CAT".  A record that itself holds '\n' bytes is several
 * lines; their inner framing newlines stay and only the last one goes.  A NUL cuts its line.  An empty record is an empty
 * line: its output is what the program prints for one, empty or not (':x' prints "x" under the non-deterministic engine; the
 * reference's deterministic engine prints nothing for an empty line, whatever the program).  nrec == 0 is valid with n == 0.  The
 * outputs are concatenated into d_out; d_out_off[i] is where record i's output starts, d_out_off[nrec] = *out_len.
 * Arguments, overlaps, the offsets' check (TRRE_E_ARG, nothing written), scan mode only, the refusal of a program that can
 * print a '\n' of its own (TRRE_E_UNSUPPORTED), d_in == d_out and a split-form scan in flight: as for
 * trre_scan_device_records; d_out may be null when cap is 0.  The differences:
 *   TRRE_E_CAPACITY  *out_len is the size of the unframed output (the framed size minus nrec).  d_out has not been written at
 *                    all — in place the input is intact, no restore pass runs — and d_out_off is unspecified.  A retry with
 *                    room works; cap == 0 is a size query.
 *   TRRE_E_DIVERGES  *out_len = 0; d_out and d_out_off are unspecified; trre_last_error() holds the reference's message.
 *                    There is no partial output here: a caller who wants the reference's takes the records call.
 * How: the strings are expanded into a staged text with a '\n' behind each, that text is scanned as it stands into a buffer
 * of the library's own, and the framed output is compacted into d_out without each record's closing '\n'.
 * Device memory, kept by the (prog, device) until trre_free: the staged text, n + nrec + 64 bytes; the framed output,
 * cap + nrec + 64 bytes; 24 bytes per 16 KiB of staged text and per 64 KiB of framed output.  Synchronous with respect to
 * `stream`. */
int trre_scan_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out,
                             size_t cap, int64_t* d_out_off, size_t* out_len, void* stream);

/* Matched strings: the same column of strings under a program compiled with TRRE_MODE_MATCH — which of the strings does the
 * pattern accept, and what do the accepted ones become.  With M what the reference prints under `trre -m`, for string i
 *     m_i = M(rec_i + "\n"),   valid[i] = (m_i is not empty),   out_i = m_i without its last byte (the framing '\n'),
 * and out_i is empty when the string is rejected.  The outputs are concatenated into d_out; d_out_off[i] is where out_i
 * starts, d_out_off[nrec] = *out_len; a rejected string has d_out_off[i + 1] == d_out_off[i].  A NUL cuts its line.  An empty
 * string is an empty line: '(a:x)*' accepts it with an empty output, 'a+:x' rejects it, ':x' accepts it with "x".
 * d_valid is an Arrow validity bitmap — bit i & 7 of byte i >> 3 — of 8 * ceil(nrec / 64) bytes, 8-byte aligned (anything else:
 * TRRE_E_ARG), written as whole 64-bit words; the bits at and beyond nrec are zero.  *n_matched (may be null) receives the
 * number of set bits.
 * Arguments, overlaps (d_valid is one more array that overlaps nothing), d_in == d_out, d_out null with cap == 0, the offsets'
 * check (TRRE_E_ARG, nothing written) and a split-form scan in flight: as for trre_scan_device_strings.
 * Refused before the device is touched: a program not compiled with TRRE_MODE_MATCH (TRRE_E_ARG); one that can print a '\n' of
 * its own (TRRE_E_UNSUPPORTED); one without guided tables — a backward automaton beyond 16 384 states, which runs on the
 * backtracking family — or with TRRE_KERNEL_BACKTRACK forced through trre_set_kernel (TRRE_E_UNSUPPORTED: the verdicts come
 * from the guided tables).  The scan itself always runs on the general guided family.
 * A string that holds a '\n' would be several lines with several verdicts: TRRE_E_ARG, found on the device from the staged
 * text's newline count before anything is written to d_out; d_out_off and d_valid are unspecified then.
 *   TRRE_E_CAPACITY  exactly when the framed length minus n_matched exceeds cap; *out_len is that size.  d_out has not been
 *                    written at all (in place the input is intact), d_out_off is unspecified, d_valid and *n_matched are
 *                    valid: cap == 0 with d_out == NULL answers "which strings match, and how much room do their outputs
 *                    need", and a retry with room works.
 *   TRRE_E_DIVERGES  *out_len = 0; d_out, d_out_off and d_valid are unspecified; trre_last_error() holds the reference's
 *                    message (a search that does not return, or one that exhausts the reference's stack).
 * How: the strings call's staged text is scanned in match mode into the library's framed buffer; a line's fate is what the
 * backward pass's symbol at its first byte says (one table lookup per string: the bitmap and the ranks M_i = accepted strings
 * among 0 .. i); string i's framed output ends just past framed newline number M_i, and the framed output goes into d_out with
 * every '\n' dropped.
 * Device memory, kept by the (prog, device) until trre_free: the strings call's buffers — the staged text, n + nrec + 64
 * bytes; the framed output, cap + nrec + 64 bytes; 24 bytes per 16 KiB of staged text and of framed output — plus the
 * symbols of the staged text (1 byte per staged byte; half a byte up to 16 backward states, 2 bytes beyond 256) and the verdict
 * workspace, 16 bytes per 256 strings.  Synchronous with respect to `stream`; trre_last_scan_flags as for the strings call. */
int trre_match_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out,
                              size_t cap, int64_t* d_out_off, uint8_t* d_valid, size_t* n_matched, size_t* out_len, void* stream);

/* Found strings: the same column of strings under a program compiled with TRRE_MODE_FIND — every match of every string, the
 * rest thrown away (re.findall, grep -o, str.extract_all).  For a string s that holds no '\n', let L be s cut at its first NUL.
 * The reference's scan loop (trre_nft.c:775-790) runs an attempt at position 0 of L; an attempt that reaches FINAL prints its
 * output o; if it consumed k > 0 bytes the next attempt starts k bytes on, otherwise one raw byte is copied and the next attempt
 * starts one byte on; one more attempt runs on the empty tail.  find(s) is the list of all those o, in order, the raw bytes
 * gone — attempts that consumed nothing included ('x*' on "bb": three empty matches, as Python's findall), an o being what
 * fputs prints (an output that holds a NUL ends before it).  A string without a successful attempt has an empty list.
 * With A = 0x01, B = 0x02 and W = (:A)(P)(:B), find(s) is the pieces between A and B of what the reference prints for W on s.
 *   d_list_off   nrec + 1 entries: d_list_off[i] is the number of matches in strings 0 .. i - 1, d_list_off[nrec] = *n_matches
 *   d_match_off  room for match_cap + 1 entries: entry j is where match j's output starts in d_out, entry *n_matches = *out_len
 *   d_out        cap bytes: the outputs, concatenated
 * *n_matches may be null.  nrec == 0 is valid with n == 0: d_list_off[0] = 0, and d_match_off[0] = 0 if d_match_off is not null.
 * Arguments, overlaps (the two offset arrays are two more arrays that overlap nothing), d_in == d_out, d_out null with cap == 0,
 * d_match_off null with match_cap == 0, the offsets' check (TRRE_E_ARG, nothing written) and a split-form scan in flight: as
 * for trre_match_device_strings.  A string that holds a '\n' would be several lines: TRRE_E_ARG, found on the device from the
 * staged text's newline count before anything of the caller's is written.
 * Refused before the device is touched: a program not compiled with TRRE_MODE_FIND (TRRE_E_ARG) — and a find program given to
 * any other scan call (TRRE_E_ARG) —; one that can print a '\n' of its own (TRRE_E_UNSUPPORTED); TRRE_KERNEL_BACKTRACK forced
 * through trre_set_kernel (TRRE_E_UNSUPPORTED).  Refused by trre_compile_mode (TRRE_E_UNSUPPORTED): TRRE_ENGINE_DFT (the
 * identity above does not hold for the deterministic engine: nothing to test it against) and a pattern without guided tables.
 * Both scans run on the general guided family (trre_info.kernel: TRRE_KERNEL_GUIDED_GEN); the stack guard applies as in scan mode.
 *   TRRE_E_CAPACITY  exactly when the outputs need more than cap bytes or there are more than match_cap matches; *out_len and
 *                    *n_matches hold what is needed and d_list_off is valid.  d_out and d_match_off have not been written at
 *                    all (in place the input is intact): cap == 0 and match_cap == 0 with both null is the size query, and
 *                    a retry with room works.
 *   TRRE_E_DIVERGES  *out_len = 0; the arrays are unspecified; trre_last_error() holds the reference's message.
 * How: the strings call's staged text is scanned twice on the general guided family, under two forward tables over one backward
 * automaton.  The marks table prints one byte per match and each line's '\n': unframed by the strings call's passes, its
 * offsets are d_list_off.  The texts table prints every match's output and a '\n' behind it: framed newline number j at framed
 * position q closes match j, d_match_off[j + 1] = q - j, and the framed text goes into d_out with every '\n' dropped.
 * Device memory, kept by the (prog, device) until trre_free: the staged text, n + nrec + 64 bytes; the framed marks and the
 * marks unframed, n_matches + nrec + 64 and n_matches + 64 bytes (at least n + nrec + 64); the framed texts, *out_len + n_matches
 * + 64 bytes (at least n + nrec + 64) — these two grow on the size a scan reports, which costs the first call on a larger
 * column one more scan —; 8 (nrec + 1) bytes of list offsets; 24 bytes per 16 KiB of the staged and the framed texts; and the
 * general guided family's workspace twice (each scan has its own: symbols, 1 byte per staged byte — half a byte up to 16
 * backward states, 2 bytes beyond 256 —, and lane counts).  Synchronous with respect to `stream`; trre_last_scan_flags as for
 * the strings call. */
int trre_find_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out, size_t cap,
                             int64_t* d_match_off, size_t match_cap, int64_t* d_list_off, size_t* n_matches, size_t* out_len, void* stream);

/* Match spans: the same column of strings under a program compiled with TRRE_MODE_SPANS — WHERE every match of every string
 * starts and ends (re.finditer().span(), str.find, str.count, str.contains, the boundaries for splitting a column).  The
 * attempts are those of trre_find_device_strings: for a string s that holds no '\n', L is s cut at its first NUL; the scan
 * loop (trre_nft.c:775-790) runs an attempt at position 0 of L; an attempt that reaches FINAL after consuming k bytes from
 * position p is the match (p, p + k); if k > 0 the next attempt starts at p + k, otherwise one raw byte is skipped; one more
 * attempt runs on the empty tail.  Empty matches count ('x*' on "bb": (0,0) (1,1) (2,2)); a NUL ends the search ('(cat|dog)'
 * on "a cat\0dog": (2,5) alone).  What the program prints plays no part: a program that prints a '\n' of its own is served.
 *   d_start, d_end  room for span_cap entries each: match j is d_in[d_start[j] .. d_end[j]) — byte positions in d_in, absolute,
 *                   d_off[i] <= d_start[j] <= d_end[j] <= d_off[i + 1] for the string i that holds match j.  Two arrays, so
 *                   that adjacent matches store adjacent words.  Both may be null with span_cap == 0
 *   d_list_off      nrec + 1 entries: d_list_off[i] is the number of matches in strings 0 .. i - 1, d_list_off[nrec] = *n_matches
 * *n_matches may be null.  d_in is only read; there is no output buffer.  nrec == 0 is valid with n == 0: d_list_off[0] = 0.
 * The offsets' check (TRRE_E_ARG, nothing written), a string that holds a '\n' (TRRE_E_ARG, found on the device from the staged
 * text's newline count before anything of the caller's is written) and a split-form scan in flight: as for
 * trre_find_device_strings.  Any overlap among d_off, d_start, d_end, d_list_off, or of one of them with d_in: TRRE_E_ARG.
 * Refused before the device is touched: a program not compiled with TRRE_MODE_SPANS (TRRE_E_ARG) — and a spans program given
 * to any other scan call (TRRE_E_ARG) —; TRRE_KERNEL_BACKTRACK forced through trre_set_kernel (TRRE_E_UNSUPPORTED).  Refused by
 * trre_compile_mode (TRRE_E_UNSUPPORTED): TRRE_ENGINE_DFT and a pattern without guided tables.  The scan runs on the general
 * guided family (trre_info.kernel: TRRE_KERNEL_GUIDED_GEN); the stack guard applies as in scan mode.
 *   TRRE_E_CAPACITY  exactly when there are more than span_cap matches: *n_matches holds the number needed and d_list_off is
 *                    valid; d_start and d_end have not been written at all.  span_cap == 0 is the size query — and all that
 *                    count and contains need.
 *   TRRE_E_DIVERGES  *n_matches = 0; the arrays are unspecified; trre_last_error() holds the reference's message.
 * How: ONE scan of the strings call's staged text under a forward table that prints none of the program's output: a position
 * byte per staged byte ('\n' for a '\n'), 0x01 in front of the first byte of every match, 0x02 behind its last.  With the
 * markers taken out the framed text is the staged text's length with its newlines in place, so for a marker at framed
 * position q, position = q - (0x01 before q) - (0x02 before q) - ('\n' before q): 0x01 number j gives d_start[j], 0x02 number j
 * d_end[j], and '\n' number i gives d_list_off[i + 1] = 0x01 before q.  A count pass (three counters per 16 KiB framed tile), their
 * exclusive sums and a rank pass do that arithmetic; every word is stored once, by the lane that owns its byte.
 * Device memory, kept by the (prog, device) until trre_free: the staged text, n + nrec + 64 bytes; the framed text, n + nrec +
 * 2 * n_matches + 64 bytes (it grows on the size the scan reports, which costs the first call on a column with more matches
 * one more scan); 8 (nrec + 1) bytes of the staging passes' ranks; 48 bytes per 16 KiB of the framed text; and the general
 * guided family's workspace once.  Synchronous with respect to `stream`; trre_last_scan_flags as for the strings call. */
int trre_span_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t* d_start,
                             int64_t* d_end, size_t span_cap, int64_t* d_list_off, size_t* n_matches, void* stream);

/* Split strings: the same column of strings under a program compiled with TRRE_MODE_SPANS, cut at every match — a list of
 * pieces per string (re.split, str.split, Arrow's split_pattern).  The definition rests on the spans of
 * trre_span_device_strings: string i has bytes s and spans (s_0,e_0) .. (s_{c-1},e_{c-1}) relative to the string, ordered and
 * disjoint (e_{k-1} <= s_k); its pieces are the c + 1 byte strings s[0:s_0], s[e_0:s_1], .., s[e_{c-1}:len(s)].  A string without
 * a match is one piece, itself; an empty string is one empty piece; empty matches split ('x*' on "bb": '', 'b', 'b', '', as
 * re.split); the search ends at a NUL, so the last piece keeps the NUL and everything behind it.  What the program prints plays
 * no part.
 *   d_out        cap bytes: the pieces, concatenated — the bytes of d_in outside every span, in order; *out_len = n minus the
 *                matched bytes
 *   d_piece_off  room for piece_cap + 1 entries: piece k is d_out[d_piece_off[k] .. d_piece_off[k + 1]), entry *n_pieces = *out_len
 *   d_list_off   nrec + 1 entries: string i owns pieces d_list_off[i] .. d_list_off[i + 1] - 1; d_list_off[i] is the number of
 *                matches in strings 0 .. i - 1, plus i; d_list_off[nrec] = *n_pieces = n_matches + nrec
 * *n_pieces and *out_len may be null.  nrec == 0 is valid with n == 0: d_list_off[0] = 0, and d_piece_off[0] = 0 if d_piece_off
 * is not null.  d_out may be null with cap == 0, d_piece_off with piece_cap == 0.  The offsets' check (TRRE_E_ARG, nothing
 * written), a string that holds a '\n' (TRRE_E_ARG, found on the device before anything of the caller's is written) and a
 * split-form scan in flight: as for trre_span_device_strings.  Any overlap among d_in, d_off, d_out, d_piece_off and
 * d_list_off: TRRE_E_ARG — there is no in-place form.  Refused before the device is touched: a program not compiled with
 * TRRE_MODE_SPANS (TRRE_E_ARG); TRRE_KERNEL_BACKTRACK forced through trre_set_kernel (TRRE_E_UNSUPPORTED); 2^55 strings or
 * bytes, a piece_cap of 2^58 (TRRE_E_ARG).
 *   TRRE_E_CAPACITY  exactly when *out_len > cap or *n_pieces > piece_cap: both sizes hold what is needed and d_list_off is
 *                    valid; d_out and d_piece_off have not been written at all.  cap == 0 and piece_cap == 0 with both null is
 *                    the size query, and a retry with room works.
 *   TRRE_E_DIVERGES  *out_len = *n_pieces = 0; the arrays are unspecified; trre_last_error() holds the reference's message.
 * How: the span call's passes up to its totals — the staged text, the one scan into the framed text (a position byte per
 * staged byte, 0x01 in front of a match, 0x02 behind it), the three counters per 16 KiB framed tile and their sums.  0x01 and
 * 0x02 alternate, so a position byte lies outside every match exactly when the number of markers before it is even: one more
 * count pass gives the kept bytes per tile, their sum *out_len, and one compaction pass copies every kept byte from d_in to its
 * place; the lane that owns 0x02 number j, behind l newlines, stores d_piece_off[j + 1 + l], the lane that owns newline number
 * i, behind a matches, d_piece_off[a + i + 1] and d_list_off[i + 1] = a + i + 1.  Every byte and word is stored once.
 * Device memory, kept by the (prog, device) until trre_free: the span call's — the staged text, n + nrec + 64 bytes; the framed
 * text, n + nrec + 2 * n_matches + 64 bytes; 8 (nrec + 1) bytes of ranks; the general guided family's workspace once — with 72
 * bytes per 16 KiB of the framed text in place of 48: the kept bytes per tile and before it.  Synchronous with respect to
 * `stream`; trre_last_scan_flags as for the strings call. */
int trre_split_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint8_t* d_out, size_t cap,
                              int64_t* d_piece_off, size_t piece_cap, int64_t* d_list_off, size_t* n_pieces, size_t* out_len, void* stream);

/* Filtered strings: the same column of strings under a program compiled with TRRE_MODE_SPANS, with the strings the pattern
 * matches somewhere kept and the rest dropped — s[s.str.contains(p)], grep / grep -v on a column, Arrow's filter over
 * match_substring_regex — and the rows that were kept, for the sibling columns.  The definition rests on the spans of
 * trre_span_device_strings: string i is kept exactly when it has at least one match there (d_list_off[i + 1] - d_list_off[i] > 0);
 * with TRRE_FILTER_INVERT in `flags`, exactly when it has none.  Empty matches count ('x*' keeps every string, the empty one
 * included); the search ends at a NUL ('(cat|dog)' drops "\0cat" and keeps "a cat\0dog"); what the program prints plays no
 * part.  A kept string is copied whole, a NUL and everything behind it included.
 *   d_out      cap bytes: the kept strings, concatenated in input order; *out_len is their total
 *   d_out_off  room for row_cap + 1 entries: kept string r is d_out[d_out_off[r] .. d_out_off[r + 1]); d_out_off[0] = 0,
 *              d_out_off[*n_kept] = *out_len
 *   d_rows     room for row_cap entries: d_rows[r] is the index in the input column of kept string r; strictly increasing
 * *n_kept and *out_len may be null.  d_out may be null only with cap == 0, d_out_off and d_rows only with row_cap == 0; all
 * three null with both capacities 0 is the size query.  nrec == 0 is valid with n == 0: TRRE_OK, and d_out_off[0] = 0 if
 * d_out_off is not null; the same when nrec > 0 and nothing is kept (*n_kept = *out_len = 0).  The offsets' check (TRRE_E_ARG,
 * nothing written), a string that holds a '\n' (TRRE_E_ARG, found on the device before anything of the caller's is written) and
 * a split-form scan in flight: as for trre_span_device_strings.  Any overlap among d_in, d_off, d_out, d_out_off and d_rows:
 * TRRE_E_ARG — there is no in-place form.  Refused before the device is touched: a null argument, a bit of `flags` other than
 * TRRE_FILTER_INVERT, a program not compiled with TRRE_MODE_SPANS (TRRE_E_ARG); TRRE_KERNEL_BACKTRACK forced through
 * trre_set_kernel (TRRE_E_UNSUPPORTED); 2^55 strings or bytes, a row_cap of 2^58 (TRRE_E_ARG).
 *   TRRE_E_CAPACITY  exactly when *out_len > cap or *n_kept > row_cap: both sizes hold what is needed; d_out, d_out_off and
 *                    d_rows have not been written at all, and a retry with that room succeeds.
 *   TRRE_E_DIVERGES  *n_kept = *out_len = 0; the arrays are unspecified; trre_last_error() holds the reference's message.
 * How: the span call's passes with its list offsets, and nothing else of it, stored into an array of the library's own.  Then,
 * over 16 KiB tiles of the INPUT (aligned to 16 bytes by address): the first string that ends in every tile (a binary search
 * per tile); per tile the kept strings that end in it and its kept bytes, from the offsets and the list offsets alone; their
 * two exclusive sums, whose totals are *n_kept and *out_len, read back in one synchronisation; and one compaction pass that
 * takes the tile into LDS as whole vectors, marks the kept bytes with a bit each (start and end toggles of the kept strings
 * and a prefix XOR) and writes the tile's contiguous part of d_out as whole aligned 16-byte vectors, bytes only at the two
 * ends it shares with its neighbours.  The thread that owns kept string r stores d_rows[r] and d_out_off[r + 1].  Every byte
 * and word is stored once.
 * Device memory, kept by the (prog, device) until trre_free: the span call's, and 8 (nrec + 1) bytes of list offsets and 48
 * bytes per 16 KiB of the input.  Synchronous with respect to `stream`; trre_last_scan_flags as for the strings call. */
#define TRRE_FILTER_INVERT 1u   /* keep the strings WITHOUT a match (grep -v) */
int trre_filter_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint32_t flags,
                               uint8_t* d_out, size_t cap, int64_t* d_out_off, int64_t* d_rows, size_t row_cap, size_t* n_kept,
                               size_t* out_len, void* stream);

/* Field k of every string: the same column of strings under a program compiled with TRRE_MODE_SPANS, split at every match, and
 * ONE piece of every string taken — SQL's split_part(s, delim, k), s.str.split(p).str.get(k), s.str.rsplit(p, n=1).str.get(-1),
 * cut -f — as a flat column with one entry per string and a validity bitmap.  The definition rests on the spans of
 * trre_span_device_strings, as trre_split_device_strings' does: string i with c matches has the c + 1 pieces of the split call;
 * k >= 0 selects piece k, k < 0 piece c + 1 + k (-1: the last).  The string HAS the field exactly when that index lies in [0, c]:
 * then the field's bytes are that piece and the validity bit is set; otherwise the field is empty and the bit is clear (pandas'
 * NaN; a caller who wants SQL's empty string ignores the bitmap).  Empty matches split ('x*' on "bb": fields 0 .. 3 are "", "b",
 * "b", "", field 4 is absent); the search ends at a NUL, so the last piece keeps the NUL and everything behind it (',' on
 * "a,b\0c,d": field 1 and field -1 are both "b\0c,d"); a string without a match is one piece, itself (k = 0 and k = -1 return it
 * whole); an empty string has one empty piece; what the program prints plays no part.  Any k is legal: INT64_MIN selects nothing.
 *   d_out      cap bytes: the fields, concatenated in input order; *out_len is their total
 *   d_out_off  nrec + 1 entries: field i is d_out[d_out_off[i] .. d_out_off[i + 1]); d_out_off[0] = 0, d_out_off[nrec] = *out_len;
 *              an absent field has d_out_off[i + 1] == d_out_off[i]
 *   d_valid    the Arrow validity bitmap, exactly as trre_match_device_strings defines it: 8 * ceil(nrec / 64) bytes, 8-byte
 *              aligned (else TRRE_E_ARG), written as whole 64-bit words, bits at and beyond nrec zero
 *   *n_valid   (may be null) the number of set bits;  *out_len may be null
 * d_out may be null only with cap == 0, and d_out_off only when d_out is: that is the size query.  When no field has bytes the
 * call returns TRRE_OK and writes the offsets (all zero; if d_out_off is not null) and the bitmap.  nrec == 0 is valid with
 * n == 0: TRRE_OK, and d_out_off[0] = 0 if d_out_off is not null.  The offsets' check (TRRE_E_ARG, nothing written), a string that
 * holds a '\n' (TRRE_E_ARG, found on the device before anything of the caller's is written) and a split-form scan in flight: as
 * for trre_span_device_strings.  Any overlap among d_in, d_off, d_out, d_out_off and d_valid: TRRE_E_ARG — there is no in-place
 * form.  Refused before the device is touched: a null argument, a program not compiled with TRRE_MODE_SPANS (TRRE_E_ARG);
 * TRRE_KERNEL_BACKTRACK forced through trre_set_kernel (TRRE_E_UNSUPPORTED); 2^55 strings or bytes (TRRE_E_ARG).
 *   TRRE_E_CAPACITY  exactly when *out_len > cap: *out_len, *n_valid and d_valid are valid; d_out and d_out_off have not been
 *                    written at all, and a retry with that room succeeds.
 *   TRRE_E_DIVERGES  *out_len = *n_valid = 0; the arrays are unspecified; trre_last_error() holds the reference's message.
 * How: the span call's passes with its list offsets, and nothing else of it, stored into an array of the library's own.  One
 * pass over the strings writes the bitmap and the bounds of the fields that start or end where their string does; one more pass
 * over the framed text, the span call's emit pass with other stores, lets the two markers that bound a field store where it
 * starts and ends.  Then the filter call's passes with those ranges in place of whole strings, over 16 KiB tiles of the INPUT:
 * the strings with the field and the field bytes per tile, their two exclusive sums, whose totals are *n_valid and *out_len, read
 * back in one synchronisation; and one compaction pass that writes the tile's contiguous part of d_out as whole aligned 16-byte
 * vectors.  The thread that owns string i stores d_out_off[i + 1].  Every byte and word is stored once.
 * Device memory, kept by the (prog, device) until trre_free: the filter call's, and 16 nrec bytes of bounds.  Synchronous with
 * respect to `stream`; trre_last_scan_flags as for the strings call. */
int trre_field_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t k,
                              uint8_t* d_out, size_t cap, int64_t* d_out_off, uint8_t* d_valid, size_t* n_valid,
                              size_t* out_len, void* stream);

/* Split strings at the first or last matches only: trre_split_device_strings with a LIMIT — line.split('=', 1),
 * re.split(p, s, maxsplit=n), s.str.split(p, n=1), s.rsplit('.', 1), s.str.rsplit(p, n=1), str.partition / rpartition, the first
 * three columns of a log line and "the rest".  String i has c matches (s_r, e_r), r = 0 .. c - 1, exactly those of
 * trre_span_device_strings (the string cut at its first NUL, empty matches counted, what the program prints playing no part).
 * Match r CUTS exactly when limit < 0, or TRRE_SPLIT_FROM_END is clear and r < limit, or it is set and c - r <= limit.  limit
 * is compared, never added or negated: any int64 is legal, INT64_MIN and INT64_MAX included; limit == 0 cuts nothing.  With cc
 * cutting matches (cc = c when limit < 0, otherwise min(c, limit)) the string has cc + 1 pieces: the bytes outside the CUTTING
 * matches, in order.  A match that does not cut stays in its piece as ordinary text ('=' with limit 1 on "a=b=c": "a", "b=c";
 * '\.' with limit 1 from the end on "x.tar.gz": "x.tar", "gz"); a NUL and everything behind it stays in the last piece; an empty
 * cutting match yields an empty piece where the split call would; an empty match that does not cut changes nothing.
 *   d_out        cap bytes: the bytes of d_in outside the cutting matches, in order; *out_len = n minus those matches' bytes
 *   d_piece_off  room for piece_cap + 1 entries, as the split call's; entry *n_pieces = *out_len
 *   d_list_off   nrec + 1 entries: d_list_off[i] is the number of cutting matches in strings 0 .. i - 1, plus i;
 *                d_list_off[nrec] = *n_pieces
 * Two identities: with limit < 0, or limit >= every string's c, the three arrays are byte for byte trre_split_device_strings',
 * with either flag value; with limit == 0, d_out is d_in, d_piece_off[i] = d_off[i] - d_off[0] and d_list_off[i] = i.
 * Null rules, the size query, nrec == 0, TRRE_E_CAPACITY (exactly when *out_len > cap or *n_pieces > piece_cap: both sizes and
 * d_list_off valid, d_out and d_piece_off not written at all), TRRE_E_DIVERGES, a string that holds a '\n', the offsets' check,
 * overlaps (no in-place form), the 2^55 / 2^58 limits and a split-form scan in flight: word for word the split call's.  Refused
 * before the device is touched, in this order: a null argument; a bit of `flags` other than TRRE_SPLIT_FROM_END; a program
 * compiled with TRRE_MODE_SUB; any other program not compiled with TRRE_MODE_SPANS (all TRRE_E_ARG); TRRE_KERNEL_BACKTRACK
 * forced (TRRE_E_UNSUPPORTED); the sizes; the overlaps.
 * How: the span call's passes up to its totals, and its list offsets L, and nothing else of it, into an array of the library's
 * own.  Match number j of the column, behind l newlines, is match r = j - L[l] of c = L[l + 1] - L[l]: the lane that owns a
 * marker resolves the rule once, and a tile that starts inside a match once for that match — never per byte.  One count pass
 * over the 16 KiB framed tiles gives the kept bytes and the cutting matches that close in every tile; their two exclusive sums'
 * totals are *out_len and *n_pieces - nrec, read back in one synchronisation and checked before anything of the caller's is
 * written.  One compaction pass copies every kept byte from d_in; the lane that owns the 0x02 of a cutting match, behind cb
 * others and l newlines, stores d_piece_off[cb + 1 + l]; the lane that owns newline i, behind ca cutting matches,
 * d_piece_off[ca + i + 1] and d_list_off[i + 1] = ca + i + 1; the markers of a match that does not cut store nothing.  Every
 * byte and word is stored once.
 * Device memory, kept by the (prog, device) until trre_free: the span call's, 8 (nrec + 1) bytes of list offsets, and two
 * counters and their sums per framed tile (32 bytes per 16 KiB of the framed text).  Synchronous with respect to `stream`;
 * trre_last_scan_flags as for the strings call. */
#define TRRE_SPLIT_FROM_END 1u   /* the LAST `limit` matches cut (rsplit), not the first */
int trre_splitn_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t limit,
                               uint32_t flags, uint8_t* d_out, size_t cap, int64_t* d_piece_off, size_t piece_cap,
                               int64_t* d_list_off, size_t* n_pieces, size_t* out_len, void* stream);

/* Field k of that limited split: trre_field_device_strings with `limit` and `flags` as trre_splitn_device_strings defines them —
 * key and value of "k=v=w" ('=', limit 1: fields 0 and 1 are "k" and "v=w"), stem and extension ('\.', limit 1 from the end, on
 * "x.tar.gz": field 0 is "x.tar", field -1 "gz"), str.partition / rpartition.  With cc the string's cutting matches: kk = k for
 * k >= 0 and cc + 1 + k for k < 0; the field is valid exactly when 0 <= kk <= cc.  With m0 the first cutting match (0 from the
 * front, c - cc from the end) the field starts at the string's start when kk = 0, otherwise at e_{m0 + kk - 1}, and ends at the
 * string's end when kk = cc, otherwise at s_{m0 + kk}.  With limit < 0 the call returns what trre_field_device_strings returns.
 * The outputs, the null rules, the size query, TRRE_E_CAPACITY, TRRE_E_DIVERGES and every refusal are the field call's; a bit of
 * `flags` other than TRRE_SPLIT_FROM_END is refused (TRRE_E_ARG) behind the null arguments and before the program's mode.
 * How: the field call's passes; only which marker stores a bound, and which strings have the field, follow the limited index
 * arithmetic.  Device memory: the field call's. */
int trre_fieldn_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t k,
                               int64_t limit, uint32_t flags, uint8_t* d_out, size_t cap, int64_t* d_out_off, uint8_t* d_valid,
                               size_t* n_valid, size_t* out_len, void* stream);

/* Trimmed strings: the same column of strings under a program compiled with TRRE_MODE_SPANS, every string without the match that
 * touches its start and the match that touches its end — s.str.strip() / lstrip / rstrip, SQL's TRIM(LEADING | TRAILING | BOTH ..
 * FROM s), removeprefix / removesuffix, regexp_replace(s, '^P|P$', '') — as a flat column with one entry per string.  trre's
 * grammar has no anchors; this call is the anchored form of the span call's matches.  The definition rests on the spans of
 * trre_span_device_strings: string i has bytes s of length len, the UNCUT length (a NUL and what follows are part of it), and the
 * spans (s_0, e_0) .. (s_{c-1}, e_{c-1}), relative to the string, from the attempts on s cut at its first NUL.  Then
 *     lo = max{ e_j : s_j == 0 }     with TRRE_TRIM_LEFT in `flags`; otherwise, and when no match starts at 0, lo = 0
 *     hi = min{ s_j : e_j == len }   with TRRE_TRIM_RIGHT in `flags`; otherwise, and when no match ends at len, hi = len
 * and the entry is s[lo : max(lo, hi)].  The min matters for a pattern that matches the empty string: 'x*' on "xxbxx" has the
 * spans (0,2) (2,2) (3,5) (5,5); (3,5) and (5,5) both end at 5, and the entry is "b", as re.sub('^x*|x*$', '', s) gives.  At most
 * one match starts at 0, and at most two end at len: a non-empty one and the empty tail attempt behind it; so the right side
 * depends on the string's last two matches only.  A string that holds a NUL is never trimmed on the right (every span ends at or
 * before the NUL); it is still trimmed on the left, and what is kept keeps the NUL and everything behind it (' +' on " a\0 ":
 * "a\0 ").  A string that is one match (' +' on three spaces, '(cat|dog)' on "dogcat") becomes empty: lo = len, hi = 0, the entry
 * s[len:len].  Only ONE match is removed from each side: a form that trims repeated matches is the caller's to write, as (P)+.
 * What the program prints plays no part.
 *   flags      TRRE_TRIM_LEFT, TRRE_TRIM_RIGHT or both; 0 and any other bit are refused (TRRE_E_ARG)
 *   d_out      cap bytes: the entries, concatenated in input order; *out_len (may be null) is their total
 *   d_out_off  nrec + 1 entries: entry i is d_out[d_out_off[i] .. d_out_off[i + 1]); d_out_off[0] = 0, d_out_off[nrec] = *out_len
 *   d_begin, d_end   both null or both given, nrec entries each: the VIEW form, absolute positions in d_in:
 *              d_off[i] <= d_begin[i] <= d_end[i] <= d_off[i + 1], and entry i is d_in[d_begin[i] .. d_end[i]).  They are written
 *              before the capacity decision and are valid under TRRE_E_CAPACITY: with d_out and d_out_off null and cap == 0 they
 *              are all that a caller of string views needs, and *out_len is still reported.
 * d_out may be null only with cap == 0, and d_out_off only when d_out is: that is the size query.  When no entry has bytes the
 * call returns TRRE_OK and writes the offsets (all zero; if d_out_off is not null) and the ranges.  nrec == 0 is valid with
 * n == 0: TRRE_OK, and d_out_off[0] = 0 if d_out_off is not null.  The offsets' check (TRRE_E_ARG, nothing written), a string that
 * holds a '\n' (TRRE_E_ARG, found on the device before anything of the caller's is written) and a split-form scan in flight: as
 * for trre_field_device_strings.  Refused before the device is touched, in this order: a null argument, only one of d_begin and
 * d_end among them; flags == 0 or a bit other than the two defined; a program compiled with TRRE_MODE_SUB; any other program not
 * compiled with TRRE_MODE_SPANS (all TRRE_E_ARG); TRRE_KERNEL_BACKTRACK forced through trre_set_kernel (TRRE_E_UNSUPPORTED);
 * 2^55 strings or bytes; d_out overlapping d_in — there is no in-place form; any other overlap among d_in, d_out, d_off,
 * d_out_off, d_begin and d_end (all TRRE_E_ARG).
 *   TRRE_E_CAPACITY  exactly when *out_len > cap: *out_len, d_begin and d_end are valid; d_out and d_out_off have not been
 *                    written at all, and a retry with that room succeeds.
 *   TRRE_E_DIVERGES  *out_len = 0; the arrays are unspecified; trre_last_error() holds the reference's message.
 * How: the span call's passes with its list offsets L, and nothing else of it, stored into an array of the library's own.  One
 * more pass over the framed text, the span call's emit pass with other stores: the markers of match r of a string's c matches
 * park their positions when r is 0 (the left side), c - 1 or c - 2 (the right side) — six words per string at the most, each
 * stored by one lane, the test on ranks alone.  One pass over the strings, 64 to a wave, applies the rule above to the parked
 * words that exist and stores every string's range, into d_begin and d_end too.  Then the field call's passes, unchanged, with
 * those ranges and k = 0 over 16 KiB tiles of the INPUT: the entries and their bytes per tile, their two exclusive sums, whose
 * totals are nrec and *out_len, read back in one synchronisation; and its compaction pass, which writes the tile's contiguous
 * part of d_out as whole aligned 16-byte vectors.  Every byte and word is stored once.
 * Device memory, kept by the (prog, device) until trre_free: the field call's, and 48 nrec bytes of parked words.  Synchronous
 * with respect to `stream`; trre_last_scan_flags as for the strings call. */
#define TRRE_TRIM_LEFT  1u   /* remove the match that starts at the string's start */
#define TRRE_TRIM_RIGHT 2u   /* remove the match that ends at the string's end */
int trre_trim_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, uint32_t flags,
                             uint8_t* d_out, size_t cap, int64_t* d_out_off, int64_t* d_begin, int64_t* d_end,
                             size_t* out_len, void* stream);

/* Replaced strings: the same column of strings under a program compiled with TRRE_MODE_SUB, with SOME of every string's matches
 * replaced by what they print — sed 's/x/y/' (the first match only), re.sub(p, r, s, count), s.str.replace(p, r, n=1), SQL's
 * regexp_replace(s, p, r, 1, k) (the k-th occurrence only), sed 's/x/y/2g' (from the second on).  String i has bytes s; L is s
 * cut at its first NUL; the scan loop's attempts on L are exactly those of trre_span_device_strings and
 * trre_find_device_strings: matches (s_r, e_r), r = 0 .. c - 1, ordered and disjoint, each with the output o_r that the find call
 * defines (what fputs prints: an output that holds a NUL ends before it).  Match r of its string is SELECTED exactly when
 * first <= r and (count < 0 or r - first < count) — compared, never added: any count is legal, count == 0 selects nothing, and
 * first < 0 is TRRE_E_ARG.  out_i is s with the bytes s[s_r .. e_r) of every selected match replaced by o_r; everything else
 * stays: the gaps, the unselected matches, and a NUL with everything behind it (as the split and field calls keep it).  An empty
 * selected match inserts o_r at its position ('x*:y' on "bb": (0, -1) gives "ybyby", (0, 1) "ybb", (2, 1) "bby", (3, 1) "bb").
 * Two identities: for a string without a NUL, (first, count) = (0, -1) is byte for byte what trre_scan_device_strings returns
 * for the same pattern compiled in scan mode on the NFT engine; with nothing selected d_out is d_in and
 * d_out_off[i] = d_off[i] - d_off[0].
 *   d_out        cap bytes: the outputs, concatenated in input order; *out_len is their total (longer or shorter than n)
 *   d_out_off    nrec + 1 entries: d_out_off[0] = 0, d_out_off[nrec] = *out_len
 *   *n_replaced  (may be null) the number of selected matches in the column;  *out_len may be null
 * d_out may be null only with cap == 0, and d_out_off only when d_out is: that is the size query.  nrec == 0 is valid with
 * n == 0: TRRE_OK, and d_out_off[0] = 0 if d_out_off is not null.  The offsets' check (TRRE_E_ARG, nothing written), a string that
 * holds a '\n' (TRRE_E_ARG, found on the device before anything of the caller's is written) and a split-form scan in flight: as
 * for trre_span_device_strings.  Any overlap among d_in, d_off, d_out and d_out_off: TRRE_E_ARG — there is no in-place form.
 * Refused before the device is touched: a null argument, a program not compiled with TRRE_MODE_SUB (TRRE_E_ARG) — and a sub
 * program given to any other scan or column call is TRRE_E_ARG there —; a program that can print a '\n' of its own
 * (TRRE_E_UNSUPPORTED: the framed texts could not be told apart); TRRE_KERNEL_BACKTRACK forced through trre_set_kernel
 * (TRRE_E_UNSUPPORTED); first < 0, 2^55 strings or bytes (TRRE_E_ARG).
 *   TRRE_E_CAPACITY  exactly when *out_len > cap: *out_len and *n_replaced are valid; d_out and d_out_off have not been written
 *                    at all, and a retry with that room succeeds.
 *   TRRE_E_DIVERGES  from either scan: *out_len = *n_replaced = 0; trre_last_error() holds the reference's message.
 *   TRRE_E_DEVICE    the two scans disagree on the number of matches (internal), before anything of the caller's is written.
 * How: the span call's passes and its emit pass into arrays of the library's own (where every match starts and ends, the list
 * offsets); the find call's texts scan of the SAME staged text under the inner program's table, unframed into the library's
 * own buffer with the texts' offsets.  One pass over the matches finds each match's string by a binary search in the list
 * offsets, its rank there and so whether it is selected, and leaves per chunk of 1 024 matches the selected matches, their
 * texts' bytes and their matched bytes; three exclusive sums, whose totals give *n_replaced and
 * *out_len = n - matched + texts, read back in one synchronisation: the capacity decision.  A second pass over the matches
 * stores the output position at which each match's place begins; a pass over the strings stores d_out_off; and one
 * output-driven splice writes d_out in 16 KiB tiles of its own address space as whole aligned 16-byte vectors, every vector
 * filled from the alternating sources — a text, then the input up to the next match — which it finds by a binary search among
 * the places (the tile's window of them in LDS when it fits).  Every byte and word is stored once.
 * Device memory, kept by the (prog, device) until trre_free: the span call's, the inner program's framed texts, the texts
 * unframed, and 32 bytes per match.  Synchronous with respect to `stream`; trre_last_scan_flags as for the strings call. */
int trre_sub_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t first,
                            int64_t count, uint8_t* d_out, size_t cap, int64_t* d_out_off, size_t* n_replaced, size_t* out_len,
                            void* stream);

/* Match k of every string: the same column of strings under a program compiled with TRRE_MODE_FIND, and ONE of every string's
 * matches taken — re.search(p, s).group(), s.str.extract(p), s.str.findall(p).str.get(k), SQL's regexp_extract(s, p) and
 * regexp_substr(s, p, 1, k + 1), grep -o | head -1 per row — as a flat column with one entry per string and a validity bitmap.  The
 * definition rests on trre_find_device_strings: string i has the list find(s_i) of c outputs o_0 .. o_{c-1} — the same attempts,
 * cut at the first NUL, empty matches counted, an output that holds a NUL ending before it.  k >= 0 selects match k, k < 0 match
 * c + k (-1: the last).  The string HAS the match exactly when that index lies in [0, c): then entry i is that output and the
 * validity bit is set; otherwise the entry is empty and the bit is clear.  An empty output with the bit set is not an absent
 * match ('x*' on "bb": k = 0, 1, 2 are valid and empty, k = 3 is absent; '[aie]:' on "kiwi": k = 0 is valid and empty).  Any k is
 * legal: INT64_MIN selects nothing (k is compared, never negated).
 *   d_out      cap bytes: the entries, concatenated in input order; *out_len is their total
 *   d_out_off  nrec + 1 entries: entry i is d_out[d_out_off[i] .. d_out_off[i + 1]); d_out_off[0] = 0, d_out_off[nrec] = *out_len;
 *              an absent entry has d_out_off[i + 1] == d_out_off[i]
 *   d_valid    the Arrow validity bitmap, exactly as trre_field_device_strings defines it: 8 * ceil(nrec / 64) bytes, 8-byte
 *              aligned (else TRRE_E_ARG), written as whole 64-bit words, bits at and beyond nrec zero
 *   *n_valid   (may be null) the number of set bits;  *out_len may be null
 * d_out may be null only with cap == 0, and d_out_off only when d_out is: that is the size query.  When no entry has bytes the
 * call returns TRRE_OK and writes the offsets (all zero; if d_out_off is not null) and the bitmap.  nrec == 0 is valid with
 * n == 0: TRRE_OK, and d_out_off[0] = 0 if d_out_off is not null.  The offsets' check (TRRE_E_ARG, nothing written), a string that
 * holds a '\n' (TRRE_E_ARG, found on the device before anything of the caller's is written) and a split-form scan in flight: as
 * for trre_find_device_strings.  Any overlap among d_in, d_off, d_out, d_out_off and d_valid: TRRE_E_ARG — there is no in-place
 * form.  Refused before the device is touched, in this order: a null argument; a program compiled with TRRE_MODE_SUB (TRRE_E_ARG,
 * with the message every call but trre_sub_device_strings gives it); any other program not compiled with TRRE_MODE_FIND
 * (TRRE_E_ARG); a program that can print a '\n' of its own, TRRE_KERNEL_BACKTRACK forced through trre_set_kernel
 * (TRRE_E_UNSUPPORTED); 2^55 strings or bytes, a misaligned bitmap, the overlaps (TRRE_E_ARG).
 *   TRRE_E_CAPACITY  exactly when *out_len > cap: *out_len, *n_valid and d_valid are valid; d_out and d_out_off have not been
 *                    written at all, and a retry with that room succeeds.
 *   TRRE_E_DIVERGES  from either scan: *out_len = *n_valid = 0; the arrays are unspecified; trre_last_error() holds the message.
 *   TRRE_E_DEVICE    the two scans disagree on the number of matches (internal), before anything of the caller's is written.
 * How: the find call's two scans of the staged text — the marks scan, whose unframed offsets are the list offsets, and the texts
 * scan — with everything they leave kept in arrays of the library's own: the list offsets, and the texts unframed with where each
 * starts.  One pass over the strings, 64 to a wave, finds each string's match, writes the bitmap word by one ballot, parks where
 * the entry starts in the texts, and leaves per chunk of 1 024 strings the strings with the match and the entries' bytes; two
 * exclusive sums, whose totals are *n_valid and *out_len, read back in one synchronisation: the capacity decision.  A second pass
 * over the strings stores d_out_off; and one output-driven pass writes d_out in 16 KiB tiles of its own address space as whole
 * aligned 16-byte vectors, every vector's entry found by a binary search among the output offsets (the tile's window of them in
 * LDS when it fits) — the unselected texts are never visited.  Every byte and word is stored once.
 * Device memory, kept by the (prog, device) until trre_free: the find call's, the texts unframed (their bytes + 64), 8 bytes per
 * match, 8 bytes per string and 32 bytes per 1 024 strings.  Synchronous with respect to `stream`; trre_last_scan_flags as for
 * the find call. */
int trre_nth_device_strings(trre_prog* p, const uint8_t* d_in, size_t n, const int64_t* d_off, size_t nrec, int64_t k,
                            uint8_t* d_out, size_t cap, int64_t* d_out_off, uint8_t* d_valid, size_t* n_valid, size_t* out_len,
                            void* stream);

/* What the last trre_scan_* call on the calling thread has to say beside its return code (thread-local, like trre_last_error;
 * trre_scan_finish adds to what its trre_scan_enqueue found). */
#define TRRE_SCAN_GUARD_UNDECIDED 1u /* NFT engine: the input holds a line long enough to exhaust the reference's 65 536-item stack
                                        (trre_nft.c:35-36,548-556) whose search the stack guard did not finish within its step budgets: the
                                        output is what the table kernels print — the match — where the reference MAY have exited 1 */
uint32_t trre_last_scan_flags(void);

/* Split form for back-to-back launches: enqueue only (no host sync), then collect status/size once.
 * One scan may be in flight per (prog, device); enqueues repeated before the finish must be the same
 * scan (same buffers, size and stream: a benchmark loop) — anything else returns TRRE_E_ARG.  The split
 * form uses the calling thread's current device and is not serialised against other threads.
 * Aliasing as for trre_scan_device.  Repeated enqueues of the same scan in place all read the input as
 * it was at the first enqueue of the batch (its copy), not what an earlier launch wrote over it. */
int trre_scan_enqueue(trre_prog* p, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, void* stream);
int trre_scan_finish(trre_prog* p, size_t* out_len);

/* Host buffers on `device` (in and out must not overlap at all, out == in included: TRRE_E_ARG): what the scan branch of the reference's main() does with a FILE* (the
 * getline loop of trre_nft.c:776-790 / trre_dft.c:1272-1286).  The input goes through in 64 MiB chunks
 * cut at line ends, three in flight on their own streams (staging copy, H2D, scan, D2H and the copy out
 * overlap); records are independent, so the chunks' outputs concatenate to exactly the output of one scan.
 * On TRRE_E_CAPACITY *out_len is the size the whole output needs (cap 0 / out NULL: a size query).  The
 * caller's current device is left as it was. */
int trre_scan_host(trre_prog* p, const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len, int device);

/* The same over several GPUs of this node, line-sharded: the input is cut at line ends into one contiguous
 * shard per selected device (trre_shard_bounds), each shard runs trre_scan_host on its device from a host
 * thread of its own, the outputs are concatenated in shard order (an exclusive sum of the shard sizes on
 * the host — the path has no exchange step, hence no collective).  device_mask: bit d selects visible
 * device d; 0 selects all of them.
 *
 * Threading: a compiled program may be used from several host threads at once; calls that target the same
 * device are serialised per (prog, device), calls on different devices run in parallel.  Compilation
 * (trre_compile) is single-threaded host work and trre_last_error() is per thread. */
/* (overlapping buffers: TRRE_E_ARG, as for trre_scan_host) */
int trre_scan_host_multi(trre_prog* p, const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len,
                         uint32_t device_mask);

/* Kernel timing for the last finished scan on this prog (HIP events recorded on
 * the launch stream around the scan kernels).  Enable first. */
int trre_set_profiling(trre_prog* p, int on);
int trre_last_kernel_ms(trre_prog* p, float* ms);

/* Diagnostics / CPU test tier: the enumeration of the generator modes with viability symbols computed elsewhere (sym[i] for
 * byte i; tests/cpu_shim.cpp runs the backward kernel's per-thread body on the host).  Host-only, no device involved; not a
 * replacement for trre_scan_host, which computes the symbols on the GPU. */
int trre_debug_generate(trre_prog* p, const uint8_t* in, size_t n, const uint8_t* sym, uint8_t* out, size_t cap, size_t* out_len);

/* Diagnostics / CPU test tier: the lazily determinised tables as they stand (which 0: u32 n_cls, u32 rows, u8 cls[256]; 1: the entries
 * [rows][n_cls] of 8 bytes; 2: the pool of texts) and the exploration of a list of n miss records (16 words: row, class, m, 0, the m <= 48 bytes behind the byte that missed) plus up to spec_states states
 * ahead — what trre_scan_* does between two rounds of a launch of TRRE_KERNEL_DFT_LAZY.  Host-only. */
size_t trre_debug_lazy_tables(trre_prog* p, int which, void* buf, size_t cap);
int trre_debug_lazy_explore(trre_prog* p, const uint32_t* misses, size_t n, size_t spec_states);

/* Diagnostics / CPU test tier: the sharding and reassembly of trre_scan_host_multi — n_shards shards cut at line ends, a host thread each, outputs
 * concatenated in shard order, a shard that returns TRRE_E_DIVERGES ends the output, TRRE_E_CAPACITY asks for room — with the caller's function in
 * place of the per-shard device call (fixed_len: the stand-in is length-preserving, shards go straight to their place).  Host-only. */
typedef int (*trre_debug_shard_fn)(void* user, int shard, const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len);
int trre_debug_scan_host_multi(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len, int n_shards, int fixed_len,
                               trre_debug_shard_fn fn, void* user);

/* Line sharding (multi-GPU, trre has no exchange step: lines are independent).
 * Fills bounds[0..nshards] with byte offsets such that every shard but the
 * last ends just past a '\n'.  `in` is a host pointer. */
int trre_shard_bounds(const uint8_t* in, size_t n, int nshards, size_t* bounds);

#ifdef __cplusplus
}
#endif
#endif /* TRRE_MI355X_H */
