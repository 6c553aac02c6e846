// switches.hpp — every TRRE_* environment switch the library reads, named in this one place ("The switches, one table";
// tests/test_switches.py compares the two).  The command line (cli.cpp, a binary of its own) reads its three itself.
#pragma once
#include <cstdlib>

namespace trre {

// a numeric switch whose default is the reader's business: set or not, and the value as the site parsed it
struct SwitchNum {
    bool set = false;
    long long v = 0;
    long long or_else(long long unset) const { return set ? v : unset; }
};

inline bool switch_on(const char* v) { return v != nullptr; }
inline int switch_int(const char* v, int unset) { return v ? atoi(v) : unset; }
inline SwitchNum switch_wide(const char* v) { return v ? SwitchNum{true, atoll(v)} : SwitchNum{}; }
inline SwitchNum switch_narrow(const char* v) { return v ? SwitchNum{true, atoi(v)} : SwitchNum{}; }

// read once per process
struct Switches {
    bool trace = switch_on(getenv("TRRE_TRACE"));                      // what the compile, the lazy rounds, the repair rounds, a void launch, the host path's stages and generator mode (who enumerated each chunk: the device or the host) did, on stderr
    bool no_stack_guard = switch_on(getenv("TRRE_NO_STACK_GUARD"));    // the stack guard (guard_block.hpp) off
    SwitchNum guard_budget = switch_wide(getenv("TRRE_GUARD_BUDGET")); // search steps per line of the stack guard; beyond: not decided
    SwitchNum guard_call_budget = switch_wide(getenv("TRRE_GUARD_CALL_BUDGET"));   // ... and per scan call, summed over its suspect lines
    SwitchNum lazy_budget = switch_wide(getenv("TRRE_LAZY_BUDGET"));   // table steps per sub-range of the lazy family (named in its error message)
    SwitchNum bt_budget = switch_wide(getenv("TRRE_BT_BUDGET"));       // steps per sub-range of the backtracking fallback
    int exact = switch_int(getenv("TRRE_EXACT"), -1);                  // 0: the old ownership of lines, for A/B runs; 2: the exact sub-ranges whatever the lines (A/B runs and tests)
    long long lane_bytes = switch_wide(getenv("TRRE_LANE_BYTES")).v;   // sub-range per lane (> 0: rounded up to 128), instead of the size-dependent choice
    bool no_g16 = switch_on(getenv("TRRE_NO_G16"));                    // A/B: the 8-byte entries
    bool no_fb = switch_on(getenv("TRRE_NO_FB"));                      // A/B: large tables walk their 8-byte rows in both passes
    bool fb_emit = switch_on(getenv("TRRE_FB_EMIT"));                  // the emit pass over the fallback form too (correct, slower)
    bool no_fb_copy = switch_on(getenv("TRRE_NO_FB_COPY"));            // A/B: the count pass + the emit pass on the 8-byte rows instead of the copy form
    bool no_fb_mark4 = switch_on(getenv("TRRE_NO_FB_MARK4"));          // A/B: the mark pass on the 8-byte comb, not the 4-byte one
    bool no_lpw_pair = switch_on(getenv("TRRE_NO_LPW_PAIR"));          // A/B: the window kernel without the pair form of its entries
    int mapgen = switch_int(getenv("TRRE_MAPGEN"), -1);                // 1: every memoryless program in one pass, always; 0: none
    const char* mapgen_dbg = getenv("TRRE_MAPGEN_DBG");                // a file: every tile's total and place, written by finish() (a fresh workspace per launch)
    int mapgen_window = switch_int(getenv("TRRE_MAPGEN_WINDOW"), 0);   // the memoryless kernel's LDS window in bytes (> 0), instead of a tile and an eighth
    bool mapgen_nolb = switch_on(getenv("TRRE_MAPGEN_NOLB"));          // an experiment: no look-back — the pace of the rest; the output is void
    bool mapgen_prof = switch_on(getenv("TRRE_MAPGEN_PROF"));          // phase clocks of the memoryless kernel, printed by finish()
    int mapgen_oversub = switch_int(getenv("TRRE_MAPGEN_OVERSUB"), 0); // tests: a grid that is NOT resident (> 1: so many times the resident one) — the launch must give up, not hang
    int one = switch_int(getenv("TRRE_ONE"), 0);                       // 1: the general families in ONE walk (one_block.hpp): opt-in
    int one_lane = switch_int(getenv("TRRE_ONE_LANE"), 0);             // ... its geometry: bytes per lane,
    int one_region = switch_int(getenv("TRRE_ONE_REGION"), 0);         // LDS region per lane,
    int one_look = switch_int(getenv("TRRE_ONE_LOOK"), 0);             // look-back of the forward lanes
    bool one_prof = switch_on(getenv("TRRE_ONE_PROF"));                // phase clocks of the one-pass kernel, printed by finish()
    bool no_nul_repair = switch_on(getenv("TRRE_NO_NUL_REPAIR"));      // a byte map that met a NUL goes to the general family, not to the repair
    bool gen_host = switch_on(getenv("TRRE_GEN_HOST"));                // generator modes: the enumeration on host threads, as in round 3
    bool no_pinned_direct = switch_on(getenv("TRRE_NO_PINNED_DIRECT"));    // A/B: a caller's pinned buffer is staged like a pageable one
    int shards_per_device = switch_int(getenv("TRRE_SHARDS_PER_DEVICE"), 1);   // tests: so many shards per selected device, so that the sharding runs on a box with a single GPU
};

// the environment as the process found it, read on first use
inline const Switches& switches() {
    static const Switches s;
    return s;
}

// read at their point of use on every call: the CPU tests change them inside a running process
inline SwitchNum lazy_max_bytes_now() { return switch_wide(getenv("TRRE_LAZY_MAX_BYTES")); }       // the lazy tables' memory limit
inline SwitchNum lazy_seed_states_now() { return switch_wide(getenv("TRRE_LAZY_SEED_STATES")); }   // states built before the first scan
inline const char* nft_fold_now() { return getenv("TRRE_NFT_FOLD"); }     // "states": the fold walks the NFT's states as the reference does; "both": both, compared
inline SwitchNum gen_max_rev_now() { return switch_narrow(getenv("TRRE_GEN_MAX_REV")); }             // generator modes: viability states before the filter lets everything through (>= 3)

}  // namespace trre
