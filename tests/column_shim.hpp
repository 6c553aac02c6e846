// column_shim.hpp — TEST INFRASTRUCTURE: what the host shims of the column calls (tests/{span,split,filter,field,find}_shim.cpp)
// share: the geometries they run, pointers shifted as if a longer column came before, and arrays with sentinels around them
// whose stores are counted.  Not a product path: nothing in trre_amd/ includes this file.
#pragma once
#include <cstdint>
#include <vector>

#include "../trre_amd/csrc/records_block.hpp"

namespace {

using Geo0 = trre::RecGeo<64, 1>;    // 1 KiB tiles, one wave
using Geo1 = trre::RecGeo<128, 1>;   // 2 KiB, two waves
using Geo2 = trre::RecGeo<64, 2>;    // 2 KiB, one wave, two vectors per thread
using Geo3 = trre::StrGeoDev;        // the device's

constexpr int64_t kUnstored = (int64_t)0xEEEEEEEEEEEEEEEEull;
constexpr uint8_t kUnstoredByte = 0xEE;      // (no source byte of a test is this one)
constexpr int kPad = 8;

template <class P>
P* shifted(P* p, int64_t elements) {
    return reinterpret_cast<P*>(reinterpret_cast<uintptr_t>(p) - (uintptr_t)elements * sizeof(P));
}

// an array of n elements with kPad sentinel elements on either side, element 0 at an address that is `mis` mod 16
template <class E>
struct Padded {
    std::vector<E> w;
    E fill;
    size_t at;
    Padded(int64_t n, E f, int mis = 0) : w((size_t)n + 2 * kPad + 32, f), fill(f), at(kPad) {
        if (sizeof(E) == 1)
            while ((reinterpret_cast<uintptr_t>(w.data() + at) & 15u) != (uintptr_t)mis) ++at;
        w.resize(at + (size_t)n + kPad);         // (shrinks: the storage stays where it is)
    }
    E* data() { return w.data() + at; }
    bool pads_intact() const {
        for (size_t k = 0; k < at; ++k)
            if (w[k] != fill) return false;
        for (int k = 0; k < kPad; ++k)
            if (w[w.size() - 1 - (size_t)k] != fill) return false;
        return true;
    }
};

// elements that changed; *twice when one that had been stored before changed again
template <class E>
int64_t changed(const std::vector<E>& now, const std::vector<E>& was, E fill, bool* twice) {
    int64_t c = 0;
    for (size_t k = 0; k < now.size(); ++k)
        if (now[k] != was[k]) {
            if (was[k] != fill) *twice = true;
            ++c;
        }
    return c;
}

}  // namespace
