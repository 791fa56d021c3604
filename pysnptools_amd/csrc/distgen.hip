// DistGen on the GPU (reference distreader/distgen.py:110-165): the reference's seeded genotype
// distributions, bit for bit.  SNP s belongs to batch s / block_size, and a batch is one MT19937
// stream (numpy's legacy RandomState, init_genrand(seed + batch * block_size)) of ALWAYS B =
// block_size SNPs -- also the last, partial batch of a reader -- consumed in a fixed order, with
// n = iid_count:
//
//   doubles [0, 3nB)     random_sample((n, B, 3)), C order [iid][sid][3]: the raw triples
//   doubles [3nB, 4nB)   rand(n, B), [iid][sid]: the triple is missing where the double is < 0.218
//
// (a double is two words, so the mask starts at word 6nB).  As in snpgen.hip a batch is the unit of
// parallelism: ONE 256-thread workgroup per stream, the workgroups of a launch are dealt its batches
// round-robin, none waits on another, and the state lives in LDS (mt19937.hpp).  A workgroup makes
// two passes over its stream and needs no scratch:
//
//   value  tiles of 255 doubles = 85 whole triples (a triple never straddles two tiles) are staged
//          in LDS; lane l reads its triple's three values, forms (r0 + r1) + r2 as NumPy's sum over
//          the last axis does, divides ITS component by it in f64 (one IEEE division), casts once if
//          the output is f32, and stores it to every output column that asked for its SNP.
//   mask   continues the stream in tiles of 256 doubles; a lane whose double is below 0.218 stores
//          three quiet NaNs over its triple, in every output column of its SNP.
//
// The NaN stores overwrite values stored by other lanes of the same workgroup, so the passes are
// separated by a device-scope fence and a workgroup barrier: every value store of the batch is
// performed before any lane passes the barrier, and the NaN stores are issued after it.  Different
// batches hold different SNPs, so no two workgroups ever store to the same element.
//
// Stores: the stream's order is C ([iid][sid][3]), so in C order consecutive lanes store
// consecutive elements of a requested SNP run.  F order (strides 1, n, n * n_sel) is stored
// directly with those strides: with B = 1 the lanes of one component are consecutive iids, hence
// consecutive addresses; with larger B they are n apart.
#include <algorithm>
#include <cmath>

#include "mt19937.hpp"
#include "snpmi_internal.hpp"

namespace snpmi {
namespace {

constexpr uint32_t kTileTriples = 85;          // 255 doubles per value tile
constexpr uint64_t kGroupPairs = 1ull << 22;   // requested columns per launch (bounds outc)
constexpr uint64_t kGroupEntries = 1ull << 22; // column-table entries per launch (batches x (B + 1))

template <typename T>
__device__ __forceinline__ T quiet_nan();
template <>
__device__ __forceinline__ double quiet_nan<double>() {
    return __longlong_as_double(0x7ff8000000000000ll);
}
template <>
__device__ __forceinline__ float quiet_nan<float>() {
    return __uint_as_float(0x7fc00000u);
}

// One workgroup slot: takes batches until none are left.  colptr: per batch B + 1 offsets into
// outc, the output columns of each of the batch's SNPs (CSR: SNP j's are [colptr[j], colptr[j + 1]);
// repeats of a SNP are several entries).  out: element (i, c, k) at i * si + c * sc + k * sk.
// Every loop that holds a barrier has workgroup-uniform control.
template <typename T, bool ORDER_C>
__global__ __launch_bounds__(kGenBlock) void k_distgen(uint32_t n_batches, const uint32_t* seeds,
                                                       const uint32_t* colptr, const uint64_t* outc, uint64_t n,
                                                       uint32_t B, uint64_t n_sel, uint64_t thr_miss,
                                                       T* __restrict__ out) {
    __shared__ __attribute__((aligned(8))) uint32_t key[kMtN];
    __shared__ double stage[2][kGenBlock];
    const uint32_t l = threadIdx.x, tl = l / 3, k = l - 3 * tl;
    const uint64_t nB = n * B;
    const uint64_t si = ORDER_C ? 3 * n_sel : 1, sc = ORDER_C ? 3 : n, sk = ORDER_C ? 1 : n * n_sel;
    // a tile advances the (iid, SNP) position by q iids and r SNPs
    const uint32_t vq = kTileTriples / B, vr = kTileTriples % B, mq = kGenBlock / B, mr = kGenBlock % B;
    for (uint32_t b = blockIdx.x; b < n_batches; b += gridDim.x) {
        const uint32_t* cp = colptr + (uint64_t)b * ((uint64_t)B + 1);
        mt_seed(key, seeds[b]);
        uint32_t pos = kMtN;
        // ---- value: triples [g0, g0 + 85) of the batch, triple g = (iid g / B, SNP g % B)
        uint64_t i0 = 0;
        uint32_t j0 = 0, buf = 0;
        for (uint64_t g0 = 0; g0 < nB; g0 += kTileTriples) {
            const uint32_t cnt = 3 * (uint32_t)min((uint64_t)kTileTriples, nB - g0);
            const uint64_t v = mt_take(key, pos, cnt);
            stage[buf][l] = (double)v * 0x1p-53;
            __syncthreads();  // (the buffer written two tiles on was read before the next tile's barrier)
            if (l < cnt) {
                const double* s = stage[buf] + 3 * tl;
                const double sum = (s[0] + s[1]) + s[2];
                const T q = (T)(s[k] / sum);
                const uint32_t jj = j0 + tl, c = jj / B, j = jj - c * B;
                T* o = out + (i0 + c) * si + k * sk;
                for (uint32_t p = cp[j], p1 = cp[j + 1]; p < p1; p++) o[outc[p] * sc] = q;
            }
            buf ^= 1u;
            i0 += vq;
            j0 += vr;
            if (j0 >= B) {
                j0 -= B;
                i0++;
            }
        }
        // every value store of the batch is performed before any NaN store below is issued
        __threadfence();
        __syncthreads();
        // ---- mask: doubles [g0, g0 + 256) of the batch's n * B, one per (iid, SNP)
        i0 = 0;
        j0 = 0;
        for (uint64_t g0 = 0; g0 < nB; g0 += kGenBlock) {
            const uint32_t cnt = (uint32_t)min((uint64_t)kGenBlock, nB - g0);
            const uint64_t v = mt_take(key, pos, cnt);
            if (l < cnt && v < thr_miss) {
                const uint32_t jj = j0 + l, c = jj / B, j = jj - c * B;
                T* o = out + (i0 + c) * si;
                const T miss = quiet_nan<T>();
                for (uint32_t p = cp[j], p1 = cp[j + 1]; p < p1; p++) {
                    T* e = o + outc[p] * sc;
                    e[0] = miss;
                    e[sk] = miss;
                    e[2 * sk] = miss;
                }
            }
            i0 += mq;
            j0 += mr;
            if (j0 >= B) {
                j0 -= B;
                i0++;
            }
        }
        __syncthreads();  // the next batch's seeding overwrites the state read above
    }
}

struct DevBuf {
    char* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

struct Want {
    uint64_t batch;
    uint32_t loc;
    uint64_t outc;
};

template <typename T>
void distgen(T* out, uint64_t n, uint64_t seed, uint64_t B, const uint64_t* sid_idx, uint64_t n_sel, int out_c) {
    std::lock_guard<std::recursive_mutex> lk(call_mutex());
    SNPMI_REQUIRE(n < (1ull << 40), SNPMI_E_ARG, "DistGen needs iid_count < 2**40");
    SNPMI_REQUIRE(B >= 1 && B < (1ull << 31) - kGenBlock, SNPMI_E_ARG, "DistGen needs 1 <= block_size < 2**31 - 256");
    SNPMI_REQUIRE(n * B < (1ull << 58), SNPMI_E_ARG, "DistGen batch too large");
    SNPMI_REQUIRE(n_sel < (1ull << 40), SNPMI_E_ARG, "DistGen selection too large");
    if (n_sel == 0) return;
    SNPMI_REQUIRE(sid_idx != nullptr, SNPMI_E_ARG, "sid_idx is NULL");
    // every batch touched, once: the requested columns sorted by (batch, column of the batch)
    std::vector<Want> want(n_sel);
    for (uint64_t k = 0; k < n_sel; k++) want[k] = {sid_idx[k] / B, (uint32_t)(sid_idx[k] % B), k};
    std::sort(want.begin(), want.end(), [](const Want& a, const Want& b) {
        return a.batch != b.batch ? a.batch < b.batch : a.loc != b.loc ? a.loc < b.loc : a.outc < b.outc;
    });
    // all seeds are checked before any launch
    SNPMI_REQUIRE(seed <= 0xffffffffull && want.back().batch <= (0xffffffffull - seed) / B, SNPMI_E_ARG,
                  "Seed must be between 0 and 2**32 - 1");
    if (n == 0) return;
    Device& d = device();
    SNPMI_REQUIRE(out != nullptr && is_device_ptr(d, out), SNPMI_E_ARG, "out must be device memory");
    hipStream_t st = d.stream;

    // launches: whole batches while the column tables fit (at least one batch each)
    struct Launch {
        uint64_t i0, i1, nbat;
    };
    std::vector<Launch> launches;
    uint64_t max_bat = 0, max_pairs = 0;
    for (uint64_t i0 = 0; i0 < n_sel;) {
        uint64_t i = i0, nbat = 0;
        while (i < n_sel) {
            uint64_t j = i;
            while (j < n_sel && want[j].batch == want[i].batch) j++;
            if (nbat && ((nbat + 1) * (B + 1) > kGroupEntries || j - i0 > kGroupPairs)) break;
            nbat++;
            i = j;
        }
        SNPMI_REQUIRE(i - i0 <= 0xffffffffull, SNPMI_E_ARG, "DistGen: too many repeats of one batch's SNPs");
        launches.push_back({i0, i, nbat});
        max_bat = std::max(max_bat, nbat);
        max_pairs = std::max(max_pairs, i - i0);
        i0 = i;
    }
    auto al = [](uint64_t x) { return round_up(x, 256); };
    const uint64_t o_seeds = 0, o_ptr = o_seeds + al(max_bat * 4), o_outc = o_ptr + al(max_bat * (B + 1) * 4),
                   tab_bytes = o_outc + al(max_pairs * 8);
    DevBuf tables;
    SNPMI_HIP(hipMalloc((void**)&tables.p, tab_bytes));
    uint32_t* seeds_d = (uint32_t*)(tables.p + o_seeds);
    uint32_t* ptr_d = (uint32_t*)(tables.p + o_ptr);
    uint64_t* outc_d = (uint64_t*)(tables.p + o_outc);
    const uint64_t thr_miss = (uint64_t)std::ceil(std::ldexp(0.218, 53));
    // more workgroups than the device holds at once (8 per CU) buy nothing
    const uint64_t max_slots = 8 * (uint64_t)std::max(d.cu_count, 1);

    std::vector<uint32_t> h_seeds, h_ptr;
    std::vector<uint64_t> h_outc;
    for (const Launch& L : launches) {
        h_seeds.clear();
        h_ptr.assign(L.nbat * (B + 1), 0);
        h_outc.resize(L.i1 - L.i0);
        uint64_t bi = 0;
        for (uint64_t i = L.i0; i < L.i1; bi++) {
            uint64_t j = i;
            uint32_t* cp = h_ptr.data() + bi * (B + 1);
            h_seeds.push_back((uint32_t)(seed + want[i].batch * B));
            // CSR over the batch's B columns: counts, then their running sum from the launch's offset
            for (; j < L.i1 && want[j].batch == want[i].batch; j++) cp[want[j].loc + 1]++;
            cp[0] = (uint32_t)(i - L.i0);
            for (uint64_t c = 0; c < B; c++) cp[c + 1] += cp[c];
            for (uint64_t k = i; k < j; k++) h_outc[k - L.i0] = want[k].outc;
            i = j;
        }
        SNPMI_HIP(hipMemcpyAsync(seeds_d, h_seeds.data(), L.nbat * 4, hipMemcpyHostToDevice, st));
        SNPMI_HIP(hipMemcpyAsync(ptr_d, h_ptr.data(), h_ptr.size() * 4, hipMemcpyHostToDevice, st));
        SNPMI_HIP(hipMemcpyAsync(outc_d, h_outc.data(), h_outc.size() * 8, hipMemcpyHostToDevice, st));
        const uint32_t grid = (uint32_t)std::min<uint64_t>(L.nbat, max_slots);
        if (out_c)
            k_distgen<T, true><<<grid, kGenBlock, 0, st>>>((uint32_t)L.nbat, seeds_d, ptr_d, outc_d, n, (uint32_t)B,
                                                           n_sel, thr_miss, out);
        else
            k_distgen<T, false><<<grid, kGenBlock, 0, st>>>((uint32_t)L.nbat, seeds_d, ptr_d, outc_d, n, (uint32_t)B,
                                                            n_sel, thr_miss, out);
        SNPMI_HIP(hipGetLastError());
        SNPMI_HIP(hipStreamSynchronize(st));  // the host lists are refilled for the next launch
    }
}

}  // namespace
}  // namespace snpmi

using namespace snpmi;

extern "C" {

int snpmi_dev_distgen_f32(float* out, uint64_t n_iid, uint64_t seed, uint64_t block_size, const uint64_t* sid_idx,
                          uint64_t n_sel, int out_order_c) {
    return guarded([&] { distgen(out, n_iid, seed, block_size, sid_idx, n_sel, out_order_c); });
}
int snpmi_dev_distgen_f64(double* out, uint64_t n_iid, uint64_t seed, uint64_t block_size, const uint64_t* sid_idx,
                          uint64_t n_sel, int out_order_c) {
    return guarded([&] { distgen(out, n_iid, seed, block_size, sid_idx, n_sel, out_order_c); });
}

}  // extern "C"
