// MT19937 (numpy's legacy RandomState) run by one 256-thread workgroup with the state in LDS: the
// stream both seeded generators consume (snpgen.hip, distgen.hip), pinned to numpy by
// snpmi_dev_mt19937_random_sample.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace snpmi {

constexpr uint32_t kMtN = 624;
constexpr uint32_t kGenBlock = 256;  // one workgroup per stream; one double per lane per tile

__device__ __forceinline__ uint32_t mt_twist(uint32_t hi, uint32_t lo, uint32_t far) {
    const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// init_genrand (numpy's legacy integer seeding); leaves the stream at the end of the state
__device__ __forceinline__ void mt_seed(uint32_t* key, uint32_t seed) {
    if (threadIdx.x == 0) {
        uint32_t s = seed;
        for (uint32_t i = 0; i < kMtN; i++) {
            key[i] = s;
            s = 1812433253u * (s ^ (s >> 30)) + i + 1;
        }
    }
    __syncthreads();
}

// The next 624 words.  The recurrence's three phases (words 0-226 from old words, 227-453 from the
// new 0-226, 454-623 from the new 227-396) are a dependent chain PER LANE: lane t makes words t,
// t+227 and t+454, and each needs only the lane's own previous result besides old words -- except
// word 623, whose low bits are the new word 0, which lane 169 recomputes for itself.  So all old
// words are read first, one barrier separates the reads from the writes, and one ends the writes.
__device__ __forceinline__ void mt_regen(uint32_t* key) {
    const uint32_t t = threadIdx.x;
    uint32_t a0 = 0, a1 = 0, af = 0, b0 = 0, b1 = 0, c0 = 0, c1 = 0, z0 = 0, z1 = 0, zf = 0;
    if (t < 227) {
        a0 = key[t];
        a1 = key[t + 1];
        af = key[t + 397];
        b0 = key[t + 227];
        b1 = key[t + 228];
        if (t < 170) {
            c0 = key[t + 454];
            c1 = key[t < 169 ? t + 455 : 0];
        }
        if (t == 169) {
            z0 = key[0];
            z1 = key[1];
            zf = key[397];
        }
    }
    __syncthreads();
    if (t < 227) {
        const uint32_t n0 = mt_twist(a0, a1, af);
        const uint32_t n1 = mt_twist(b0, b1, n0);
        key[t] = n0;
        key[t + 227] = n1;
        if (t < 170) {
            const uint32_t lo = t == 169 ? mt_twist(z0, z1, zf) : c1;
            key[t + 454] = mt_twist(c0, lo, n1);
        }
    }
    __syncthreads();
}

// Lane l < cnt gets the next cnt doubles' l-th as its 53-bit integer (the double is v / 2^53:
// numpy's random_sample); cnt <= 256 and pos (always even) are workgroup-uniform.  A tile takes at
// most one regeneration: lanes whose pair lies in the current state read it first.
__device__ __forceinline__ uint64_t mt_take(uint32_t* key, uint32_t& pos, uint32_t cnt) {
    const uint32_t l = threadIdx.x;
    const uint32_t w = pos + 2 * l;
    const bool mine = l < cnt;
    uint2 y = make_uint2(0, 0);
    if (mine && w < kMtN) y = *reinterpret_cast<const uint2*>(key + w);
    if (pos + 2 * cnt > kMtN) {
        mt_regen(key);
        if (mine && w >= kMtN) y = *reinterpret_cast<const uint2*>(key + (w - kMtN));
        pos = pos + 2 * cnt - kMtN;
    } else {
        pos += 2 * cnt;
    }
    return ((uint64_t)(mt_temper(y.x) >> 5) << 26) | (uint64_t)(mt_temper(y.y) >> 6);
}

}  // namespace snpmi
