// Device-side inflate of zlib streams (BGEN genotype blocks, compression 1), and the check of the
// inflated blocks' headers.  The decoder itself is inflate_core.hpp; this file is
// its wave form, the launchers and the C ABI.
//
//   k_inflate      one wave per stream, one wave per workgroup (64 threads), streams by grid stride.
//                  The wave's whole state besides registers -- the 32 KiB window, the 512-byte input
//                  chunk, both lookup tables and the build arrays: inflate_core::Scratch, 37,632 B --
//                  is the workgroup's static LDS, so four waves share a CU and no wave ever waits for
//                  another: there is no workgroup barrier, no flag, no spin.  Every lane runs the
//                  symbol walk in lockstep on wave-uniform values (what the lookups return goes
//                  through readfirstlane, so the walk runs on the scalar unit: the cost of one lane
//                  walking, with nothing to broadcast afterwards); the 64 lanes share the refill of
//                  the input chunk, the table fills, the match copies inside the window, the
//                  stores to dst (512 bytes at a time, 8 per lane, from the window) and the Adler-32
//                  partial sums, which are reduced across the wave.  dst is never read.
//                  Ordering between lanes: LDS instructions of one wave execute in issue order, so
//                  WaveLanes::sync() only has to keep the compiler from moving LDS accesses across it.
//   k_bgen_check   one workgroup per inflated block: the header fields and the range of the
//                  per-sample ploidy bytes, as a record of ten words per block.
#include <algorithm>
#include <memory>

#include "inflate_core.hpp"
#include "snpmi_internal.hpp"

namespace snpmi {
namespace {

namespace zc = inflate_core;

struct WaveLanes {
    static constexpr uint32_t LANES = 64;
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x; }  // 64-thread workgroups
    static __device__ __forceinline__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    static __device__ __forceinline__ uint32_t sum(uint32_t v) {
#pragma unroll
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    }
    static __device__ __forceinline__ uint32_t uni(uint32_t v) {
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    }
};

struct StreamRow {
    uint64_t src_off, stored, dst_off, D;
};

__global__ __launch_bounds__(64) void k_inflate(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                const StreamRow* __restrict__ tab, uint64_t streams,
                                                uint32_t* __restrict__ status) {
    __shared__ zc::Scratch scratch;
    for (uint64_t s = blockIdx.x; s < streams; s += gridDim.x) {
        const StreamRow r = tab[s];
        const uint32_t st = zc::inflate_zlib<WaveLanes>(src + r.src_off, r.stored, dst + r.dst_off, r.D, scratch);
        if (threadIdx.x == 0) status[s] = st;
    }
}

// rec[b][10]: 0 = ok / 1 = the block is shorter than 10 + n bytes (nothing else is read then, but
// the first eight bytes when it has them), bits, the block's N, K, the header's min and max ploidy,
// min and max of the samples' ploidy bits (255 and 0 when n = 0), the phased byte, the bytes n
// samples at that bit depth need
constexpr int kCheckBlock = 256;
struct BlockRow {
    uint64_t off, len;
};

__global__ __launch_bounds__(kCheckBlock) void k_bgen_check(const uint8_t* __restrict__ blocks,
                                                            const BlockRow* __restrict__ tab, uint64_t blocks_n,
                                                            uint64_t n, uint64_t* __restrict__ rec) {
    __shared__ uint32_t lo_s[kCheckBlock / 64], hi_s[kCheckBlock / 64];
    for (uint64_t b = blockIdx.x; b < blocks_n; b += gridDim.x) {
        const BlockRow r = tab[b];
        const uint8_t* p = blocks + r.off;  // 8-byte aligned
        const bool fits = r.len >= 10 + n;
        uint32_t lo = 255, hi = 0;
        if (fits) {
            const uint64_t* w = reinterpret_cast<const uint64_t*>(p + 8);
            for (uint64_t g = threadIdx.x; g < n / 8; g += kCheckBlock) {
                const uint64_t v = w[g] & 0x3f3f3f3f3f3f3f3full;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const uint32_t q = (uint32_t)(v >> (8 * k)) & 0xff;
                    lo = min(lo, q), hi = max(hi, q);
                }
            }
            for (uint64_t i = n / 8 * 8 + threadIdx.x; i < n; i += kCheckBlock) {
                const uint32_t q = p[8 + i] & 0x3f;
                lo = min(lo, q), hi = max(hi, q);
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor(lo, o, 64));
            hi = max(hi, (uint32_t)__shfl_xor(hi, o, 64));
        }
        if ((threadIdx.x & 63) == 0) lo_s[threadIdx.x >> 6] = lo, hi_s[threadIdx.x >> 6] = hi;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 0; q < kCheckBlock / 64; q++) lo = min(lo, lo_s[q]), hi = max(hi, hi_s[q]);
            uint64_t* o = rec + b * 10;
            uint64_t nf = 0, k = 0, pmin = 0, pmax = 0, phased = 0, bits = 0;
            if (r.len >= 8) {
                nf = (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16 | (uint64_t)p[3] << 24;
                k = (uint64_t)p[4] | (uint64_t)p[5] << 8;
                pmin = p[6], pmax = p[7];
            }
            if (fits) phased = p[8 + n], bits = p[9 + n];
            o[0] = fits ? 0 : 1, o[1] = bits, o[2] = nf, o[3] = k, o[4] = pmin, o[5] = pmax, o[6] = lo, o[7] = hi;
            o[8] = phased, o[9] = 10 + n + (2 * bits * n + 7) / 8;
        }
        __syncthreads();
    }
}

struct DevBuf {
    char* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

constexpr uint64_t kMaxWaves = 256 * 4 * 4;  // four resident waves per CU, the rest by grid stride

void dev_inflate(const uint8_t* src, uint64_t src_bytes, uint8_t* dst, uint64_t dst_bytes, const uint64_t* table,
                 uint64_t streams, uint32_t* status) {
    std::lock_guard<std::recursive_mutex> lk(call_mutex());
    if (streams == 0) return;
    SNPMI_REQUIRE(src != nullptr && dst != nullptr && table != nullptr && status != nullptr, SNPMI_E_ARG, "NULL argument");
    SNPMI_REQUIRE(streams < (1ull << 32), SNPMI_E_ARG, "too many streams");
    // every range inside its buffer, dst ranges 8-byte aligned and disjoint: before any device work
    std::vector<std::pair<uint64_t, uint64_t>> out(streams);
    for (uint64_t s = 0; s < streams; s++) {
        const uint64_t so = table[4 * s], sn = table[4 * s + 1], dof = table[4 * s + 2], dn = table[4 * s + 3];
        SNPMI_REQUIRE(sn < zc::kMaxStored && dn < zc::kMaxOut, SNPMI_E_ARG, "stream too long for device inflate");
        SNPMI_REQUIRE(so <= src_bytes && sn <= src_bytes - so, SNPMI_E_INDEX, "stored range outside the source buffer");
        SNPMI_REQUIRE(dof <= dst_bytes && dn <= dst_bytes - dof, SNPMI_E_INDEX,
                      "inflated range outside the destination buffer");
        SNPMI_REQUIRE(dof % 8 == 0, SNPMI_E_ARG, "inflated offsets must be multiples of 8");
        out[s] = {dof, dn};
    }
    std::sort(out.begin(), out.end());
    uint64_t end = 0;
    for (const auto& r : out) {
        if (r.second == 0) continue;
        SNPMI_REQUIRE(r.first >= end, SNPMI_E_ARG, "inflated ranges overlap");
        end = r.first + r.second;
    }
    Device& d = device();
    SNPMI_REQUIRE(is_device_ptr(d, src) && is_device_ptr(d, dst), SNPMI_E_ARG, "src and dst must be device memory");
    SNPMI_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 8 == 0, SNPMI_E_ARG, "dst must be 8-byte aligned");
    hipStream_t st = d.stream;
    DevBuf scratch;
    const uint64_t tab_bytes = round_up(streams * sizeof(StreamRow), 256);
    SNPMI_HIP(hipMalloc((void**)&scratch.p, tab_bytes + streams * sizeof(uint32_t)));
    SNPMI_HIP(hipMemcpy(scratch.p, table, streams * sizeof(StreamRow), hipMemcpyHostToDevice));
    uint32_t* status_dev = (uint32_t*)(scratch.p + tab_bytes);
    k_inflate<<<(unsigned)std::min(streams, kMaxWaves), 64, 0, st>>>(src, dst, (const StreamRow*)scratch.p, streams,
                                                                      status_dev);
    SNPMI_HIP(hipGetLastError());
    SNPMI_HIP(hipStreamSynchronize(st));
    SNPMI_HIP(hipMemcpy(status, status_dev, streams * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

void dev_bgen_check(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* table, uint64_t blocks_n,
                    uint64_t n_samples, uint64_t* rec) {
    std::lock_guard<std::recursive_mutex> lk(call_mutex());
    if (blocks_n == 0) return;
    SNPMI_REQUIRE(blocks != nullptr && table != nullptr && rec != nullptr, SNPMI_E_ARG, "NULL argument");
    SNPMI_REQUIRE(n_samples < (1ull << 32) && blocks_n < (1ull << 32), SNPMI_E_ARG, "BGEN block has too many samples");
    for (uint64_t b = 0; b < blocks_n; b++) {
        const uint64_t off = table[2 * b], len = table[2 * b + 1];
        SNPMI_REQUIRE(off % 8 == 0 && off <= blocks_bytes && len <= blocks_bytes - off, SNPMI_E_INDEX,
                      "BGEN block outside the inflated buffer");
    }
    Device& d = device();
    SNPMI_REQUIRE(is_device_ptr(d, blocks), SNPMI_E_ARG, "blocks must be device memory");
    SNPMI_REQUIRE(reinterpret_cast<uintptr_t>(blocks) % 8 == 0, SNPMI_E_ARG, "blocks must be 8-byte aligned");
    hipStream_t st = d.stream;
    DevBuf scratch;
    const uint64_t tab_bytes = round_up(blocks_n * sizeof(BlockRow), 256);
    SNPMI_HIP(hipMalloc((void**)&scratch.p, tab_bytes + blocks_n * 10 * sizeof(uint64_t)));
    SNPMI_HIP(hipMemcpy(scratch.p, table, blocks_n * sizeof(BlockRow), hipMemcpyHostToDevice));
    uint64_t* rec_dev = (uint64_t*)(scratch.p + tab_bytes);
    k_bgen_check<<<(unsigned)std::min<uint64_t>(blocks_n, 4096), kCheckBlock, 0, st>>>(
        blocks, (const BlockRow*)scratch.p, blocks_n, n_samples, rec_dev);
    SNPMI_HIP(hipGetLastError());
    SNPMI_HIP(hipStreamSynchronize(st));
    SNPMI_HIP(hipMemcpy(rec, rec_dev, blocks_n * 10 * sizeof(uint64_t), hipMemcpyDeviceToHost));
}

}  // namespace
}  // namespace snpmi

using namespace snpmi;

extern "C" {

int snpmi_dev_inflate(const uint8_t* src, uint64_t src_bytes, uint8_t* dst, uint64_t dst_bytes, const uint64_t* table,
                      uint64_t streams, uint32_t* status) {
    return guarded([&] { dev_inflate(src, src_bytes, dst, dst_bytes, table, streams, status); });
}

int snpmi_dev_bgen_check(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* table, uint64_t blocks_n,
                         uint64_t n_samples, uint64_t* rec) {
    return guarded([&] { dev_bgen_check(blocks, blocks_bytes, table, blocks_n, n_samples, rec); });
}

int snpmi_inflate_host(const uint8_t* src, uint64_t stored, uint8_t* dst, uint64_t D, uint32_t* status) {
    return guarded([&] {
        SNPMI_REQUIRE(status != nullptr && (src != nullptr || stored == 0) && (dst != nullptr || D == 0), SNPMI_E_ARG,
                      "NULL argument");
        SNPMI_REQUIRE(stored < zc::kMaxStored && D < zc::kMaxOut, SNPMI_E_ARG, "stream too long");
        std::unique_ptr<zc::Scratch> scratch(new zc::Scratch);
        *status = zc::inflate_zlib<zc::HostLanes>(src, stored, dst, D, *scratch);
    });
}

}  // extern "C"
