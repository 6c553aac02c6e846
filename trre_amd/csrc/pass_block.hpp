// pass_block.hpp — what the device translation units share (device code only; included by scan_kernels.hip and map_kernels.hip): the wave
// helpers, the LDS limit, and the handshake between the two passes of the variable-length families.
//
//   count pass   every lane leaves its output size in lane_counts[lane] (32 bits, saturated), every chunk of kChunk lanes its sum in chunk_total
//   k_chunk_scan chunk_base = exclusive scan of chunk_total
//   emit pass    a lane's place in the output: chunk_base[chunk] + the counts of the chunk's lanes before it; a chunk that ends behind the
//                caller's capacity makes the launch void (kStCapacity)
//   status       a lane's status bits reach status[0] by one atomic per wave
//
// The helpers take the kernel's arguments (ScanArgs) by reference and read lane_counts, chunk_total, chunk_base, cap where they use them; no
// kernel gained scratch memory or registers by it (DESIGN.md 4.11 has the table).  Should one ever: see OneTailArgs in scan_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "scan_core.hpp"

namespace trre {
namespace {

constexpr int kWave = 64;

// Kernels that take more than 64 KiB of dynamic LDS need the limit raised — once per kernel and device, not per launch
// (a launch is ~5 us of host time; the call is another 2-3): the limit is set to the CU's whole 160 KiB.
constexpr int kLdsLimit = 160 * 1024;
template <auto Kernel>
void allow_big_lds() {
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_relaxed) & bit) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
    done.fetch_or(bit, std::memory_order_relaxed);
}

__device__ __forceinline__ int wave_min(int v) {
    for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d, kWave));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d, kWave));
    return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    for (int d = 32; d; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d, kWave);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int d = 32; d; d >>= 1) {
        uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, kWave);
        uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, kWave);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}
// inclusive scan inside a wave
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
    const int lane = threadIdx.x & (kWave - 1);
    for (int d = 1; d < kWave; d <<= 1) {
        uint32_t u = (uint32_t)__shfl_up((int)v, d, kWave);
        if (lane >= d) v += u;
    }
    return v;
}

// ---- the handshake -----------------------------------------------------------------------------------------------------------
// A chunk is kChunk consecutive lanes: `chunk` its index, `gtid` the lane's index in it, `live` false for the chunks beyond the workspace
// in the last workgroup of a kernel that takes several chunks per workgroup (uniform per chunk).  A kernel with one chunk per workgroup
// passes blockIdx.x, threadIdx.x, true.  kReuse: the workgroup is persistent and comes by again — a barrier before the LDS words are rewritten.
// `a`: the kernel's ScanArgs.

// status publish
__device__ __forceinline__ void pass_publish(uint32_t* status, uint32_t st) {
    st = wave_or(st);
    if (st && (threadIdx.x & (kWave - 1)) == 0) atomicOr(status, st);
}

// count epilogue, the lane's part: a count that does not fit its 32-bit word (`limit`: the largest that does) is a capacity error
__device__ __forceinline__ void pass_saturate(uint64_t& n, uint32_t& st, uint64_t limit = 0xffffffffull) {
    if (n > limit) { st |= kStCapacity; n = limit; }
}
template <class Args>
__device__ __forceinline__ void pass_count_store(const Args& a, int64_t lane, uint64_t& n, uint32_t& st) {
    pass_saturate(n, st);
    a.lane_counts[lane] = (uint32_t)n;
}
// count epilogue, the chunk's part: part[kChunk / kWave]
template <int kChunk, bool kReuse = false, class Args>
__device__ __forceinline__ void pass_count_reduce(const Args& a, int64_t chunk, int gtid, bool live, uint64_t* part, uint64_t n) {
    const uint64_t wsum = wave_sum(live ? n : 0ull);
    if (kReuse) __syncthreads();
    if ((gtid & (kWave - 1)) == 0) part[gtid / kWave] = wsum;
    __syncthreads();
    if (gtid == 0 && live) {
        uint64_t t = 0;
        for (int w = 0; w < kChunk / kWave; ++w) t += part[w];
        a.chunk_total[chunk] = t;
    }
}
template <int kChunk, bool kReuse = false, class Args>
__device__ __forceinline__ void pass_count_epilogue(const Args& a, int64_t chunk, int gtid, bool live, uint64_t* part, uint64_t& n, uint32_t& st) {
    pass_saturate(n, st);
    if (live) a.lane_counts[chunk * kChunk + gtid] = (uint32_t)n;
    pass_count_reduce<kChunk, kReuse>(a, chunk, gtid, live, part, n);
}

// emit prologue: the lane's place in the output (0 for a lane that is not live); wpart[kChunk / kWave]
template <int kChunk, bool kReuse = false, class Args>
__device__ __forceinline__ uint64_t pass_emit_base(const Args& a, int64_t chunk, int gtid, bool live, uint32_t* wpart) {
    const uint32_t mine = live ? a.lane_counts[chunk * kChunk + gtid] : 0u;
    const uint32_t incl = wave_scan_incl(mine);
    if (kReuse) __syncthreads();
    if ((gtid & (kWave - 1)) == kWave - 1) wpart[gtid / kWave] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < gtid / kWave; ++w) wbase += wpart[w];
    return live ? a.chunk_base[chunk] + wbase + incl - mine : 0ull;
}
// ... and whether `chunk` ends behind the caller's capacity: uniform for whoever asks about the same chunk.  Bases grow with the chunk index, so
// a workgroup of several chunks asks about its last live one (pass_last_chunk): if that one does not fit, the output is void anyway.
template <class Args>
__device__ __forceinline__ bool pass_over_capacity(const Args& a, int64_t chunk) {
    return a.chunk_base[chunk] + a.chunk_total[chunk] > a.cap;
}
template <int kGroups>
__device__ __forceinline__ int64_t pass_last_chunk(int64_t n_chunks) {
    const int64_t last = ((int64_t)blockIdx.x + 1) * kGroups - 1;
    return last < n_chunks - 1 ? last : n_chunks - 1;
}

}  // namespace
}  // namespace trre
