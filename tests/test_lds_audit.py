"""CPU tier: the two listing audits (tools/barrier_audit.py, tools/lds_entry_audit.py) over the gfx950 listings of BOTH device translation
units, and over small listings written by hand.  A listing is built once per session (`hipcc -S --cuda-device-only` with the Makefile's
flags: map_kernels.hip seconds, scan_kernels.hip two minutes) and kept under the untracked build directory, keyed on the sources' contents."""
import hashlib
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trre_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lds_entry_audit  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]
MAPGEN_KERNELS = ["_ZN4trre8k_mapgenILb%dELb%dEEEvNS_8ScanArgsENS_10MapGenArgsE" % (f, m) for f in (1, 0) for m in (1, 0)]
_listings = {}


def _compile(src, dst):
    subprocess.run([HIPCC] + FLAGS + ["-I", CSRC, src, "-o", dst], check=True, stderr=subprocess.DEVNULL)


def listing(unit):
    """the path of `unit`.hip's device listing: built at most once per session, and once per state of the sources across sessions"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    if unit not in _listings:
        h = hashlib.sha256(" ".join(FLAGS).encode())
        for name in sorted(os.listdir(CSRC)) + [os.path.join("..", "..", "include", "trre_mi355x.h")]:
            if name.endswith((".hip", ".hpp", ".h")):
                with open(os.path.join(CSRC, name), "rb") as f:
                    h.update(name.encode() + b"\0" + f.read() + b"\0")
        d = os.path.join(ROOT, "trre_amd", "_build", "listings")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "%s-%s.s" % (unit, h.hexdigest()[:16]))
        if not os.path.exists(path):
            tmp = "%s.%d.tmp" % (path, os.getpid())
            _compile(os.path.join(CSRC, unit + ".hip"), tmp)
            os.replace(tmp, path)
        _listings[unit] = path
    return _listings[unit]


def barriers_flagged(path, depth=60):
    """tools/barrier_audit.py's last line and its output (depth 60: where the two entries that depth 12 leaves undecided in
    k_stream_g16<1,2,false> and <1,1,false> resolve)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), path, str(depth)], stdout=subprocess.PIPE, check=True)
    return r.stdout.decode().strip().splitlines()[-1], r.stdout.decode()[-3000:]


def findings(path):
    return {k: v for k, v in lds_entry_audit.audit(path).items() if v}


def test_the_memoryless_kernel_reads_no_lds_before_its_first_barrier():
    """k_mapgen stages its tables with all 256 threads and looks them up in the first count: a barrier lies between.  All four
    instantiations are in the listing by name and none has a finding."""
    got = lds_entry_audit.audit(listing("map_kernels"))
    for k in MAPGEN_KERNELS:
        assert k in got, (k, sorted(got))
    assert {k: v[:2] for k, v in got.items() if v} == {}


def test_without_the_staging_barrier_all_four_instantiations_are_flagged(tmp_path):
    """The audit sees the fault it was written for: map_kernels.hip as it was at commit 7e74f62 — here: today's source with the MG_SYNC() behind
    the staging block taken out again — has a ds_read_u8 of the length table on a path from the entry with the tables' ds_write behind it and
    no s_barrier, in every one of the four instantiations, and in nothing else."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with open(os.path.join(CSRC, "map_kernels.hip")) as f:
        src = f.read()
    old, n = re.subn(r"(if \(tid == 0\) misc\[12\] = misc\[14\] = 0;\n(?:\s*//[^\n]*\n)*)\s*MG_SYNC\(\);\n", r"\1", src)
    assert n == 1
    with open(str(tmp_path / "map_kernels_old.hip"), "w") as f:
        f.write(old)
    _compile(str(tmp_path / "map_kernels_old.hip"), str(tmp_path / "old.s"))
    got = findings(str(tmp_path / "old.s"))
    assert sorted(got) == sorted(MAPGEN_KERNELS), sorted(got)
    for k in MAPGEN_KERNELS:
        assert any(t.startswith("ds_read_u8") for _, t in got[k]), (k, got[k][:3])


def test_no_barrier_of_the_memoryless_kernel_is_left_with_lds_stores_in_flight():
    last, out = barriers_flagged(listing("map_kernels"))
    assert last == "barriers flagged: 0", out


def test_the_scan_kernels_read_no_lds_before_their_first_barrier():
    got = lds_entry_audit.audit(listing("scan_kernels"))
    assert len(got) >= 90, len(got)                         # (every kernel of the unit was looked at)
    assert {k: v[:2] for k, v in got.items() if v} == {}


def test_no_barrier_of_the_scan_kernels_is_left_with_lds_stores_in_flight():
    last, out = barriers_flagged(listing("scan_kernels"))
    assert last == "barriers flagged: 0", out


HEAD = "_Z1kv:\n\ts_load_dword s0, s[4:5], 0x0\n\tv_cmp_gt_u32_e32 vcc, 16, v0\n"
STAGE = "\ts_and_saveexec_b64 s[2:3], vcc\n\ts_cbranch_execz .LBB0_2\n\tds_write_b32 v0, v1\n.LBB0_2:\n\ts_or_b64 exec, exec, s[2:3]\n"
TAIL = "\tds_read_b32 v2, v3\n\ts_waitcnt lgkmcnt(0)\n\tv_add_u32_e32 v2, 1, v2\n\ts_endpgm\n.Lfunc_end0:\n"


def _audit_text(tmp_path, name, text):
    p = str(tmp_path / name)
    with open(p, "w") as f:
        f.write(text)
    return findings(p)


def test_the_entry_audit_on_listings_written_by_hand(tmp_path):
    """a ds_write under an s_cbranch_execz and then a ds_read with no barrier: flagged (on the path through the write; the lanes that skip it
    read what the others were asked to fill).  The same with s_waitcnt lgkmcnt(0) + s_barrier in between: clean.  A thread that reads LDS before
    anybody writes, then writes behind a barrier: clean.  A kernel's blocks end at its .Lfunc_end: the write of one kernel does not flag the
    read of the next."""
    assert _audit_text(tmp_path, "bad.s", HEAD + STAGE + TAIL) == {"_Z1kv": [(".LBB0_2", "ds_read_b32 v2, v3")]}
    assert _audit_text(tmp_path, "good.s", HEAD + STAGE + "\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n" + TAIL) == {}
    assert _audit_text(tmp_path, "read_first.s", HEAD + "\tds_read_b32 v2, v3\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n" + STAGE + "\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n" + TAIL) == {}
    # an LDS atomic and a load with the lds modifier are writes too
    assert list(_audit_text(tmp_path, "atomic.s", HEAD + "\tds_add_u32 v0, v1\n" + TAIL)) == ["_Z1kv"]
    assert list(_audit_text(tmp_path, "load_lds.s", HEAD + "\tglobal_load_dword v0, s[0:1] offset:16 lds\n" + TAIL)) == ["_Z1kv"]
    # the cross-lane operations of the DS unit touch no LDS
    assert _audit_text(tmp_path, "permute.s", HEAD + "\tds_bpermute_b32 v1, v0, v2\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n" + TAIL) == {}
    two = HEAD + "\tds_write_b32 v0, v1\n.Lfunc_end0:\n\t.size _Z1kv, .Lfunc_end0-_Z1kv\n_Z2k2v:\n" + TAIL.replace(".Lfunc_end0", ".Lfunc_end1")
    assert _audit_text(tmp_path, "two.s", two) == {}
    # a loop: the write at the loop's end reaches the read at its head over the back edge
    loop = HEAD + ".LBB0_1:\n\tds_read_b32 v2, v3\n\ts_waitcnt lgkmcnt(0)\n\tds_write_b32 v0, v2\n\ts_cbranch_scc1 .LBB0_1\n\ts_endpgm\n.Lfunc_end0:\n"
    assert list(_audit_text(tmp_path, "loop.s", loop)) == ["_Z1kv"]
