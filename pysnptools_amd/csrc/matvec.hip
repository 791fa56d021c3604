// Products of the standardized genotypes Z with tall matrices, straight from the 2-bit codes
// (gfx950): Z[i, s] = lut[4 s + code(i, s)] is never written anywhere.
//   k_packed_tdot    G = Z^T V   (n_sid x k): a reduction along the packed axis
//   k_tdot_reduce    folds the iid chunks' partials in chunk order
//   k_packed_dot     Y (+)= Z W  (n_iid x k): a reduction across packed rows
//   k_dot_reduce     folds the SNP segments' partials in global segment order
// Plain VALU code: per genotype three selects pick the LUT value (sel4 of kernels.hip) and feed one
// FMA per column.  No atomics; every sum has one fixed order, so results are the same bits on every
// run.  The reference has no counterpart: its callers use NumPy on SnpData.val.
// Built with -ffp-contract=off like the rest of the library: the FMAs below are spelled out.
#include "snpmi_internal.hpp"

namespace snpmi {
namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kLaneIids = 16;                      // one 32-bit code word per lane
constexpr uint64_t kSpan = kWave * kLaneIids;      // iids of one wave: 1024 (256 B of codes per SNP)
constexpr uint64_t kChunk = kWaves * kSpan;        // tdot: iids of one workgroup, one slab row: 4096
constexpr int kTdotSub = 64;                       // tdot: SNPs between two LDS folds of the four waves
constexpr uint64_t kTdotSnps = 256;                // tdot: SNPs per workgroup (V stays in registers across them)
constexpr uint64_t kSeg = 256;                     // dot: SNPs per segment (the unit of the global fold)
constexpr int kLoads = 8;                          // code words in flight per lane
constexpr uint64_t kSlabBytes = 128ull << 20;      // bound of the partials' scratch per launch
// widest column panel per dtype: 16 iids x panel values (tdot: V, dot: accumulators) in 128 VGPRs
template <typename T>
constexpr int kPanel = sizeof(T) == 4 ? 8 : 4;

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the 4-entry LUT select of kernels.hip: three v_cndmask, no divergent branch
template <typename T>
__device__ __forceinline__ T sel4(T l0, T l1, T l2, T l3, uint32_t c) {
    const bool b0 = (c & 1u) != 0, b1 = (c & 2u) != 0;
    const T lo = b0 ? l1 : l0;
    const T hi = b0 ? l3 : l2;
    return b1 ? hi : lo;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// ------------------------------------------------------------------ Z^T V
// Workgroup = (iid chunk of 4096, SNP tile of kTdotSnps); wave w owns iids [chunk + 1024 w, + 1024),
// lane l the 16 of them in code word l.  The lane's 16 x KP values of V are loaded once and stay in
// registers; per SNP the lane sums its 16 products per column, the wave sums its 64 lanes, and
// every kTdotSub SNPs the waves' sums are folded in wave order through LDS into the slab
// part[chunk][c][s].  TAIL (wave-uniform: the wave holds iid n - 1 or lies beyond it): a genotype
// with iid >= n is skipped, whatever its code and the LUT say.
template <typename T, int KP, bool TAIL>
__device__ __forceinline__ void tdot_snp(uint32_t w, const T* __restrict__ l, const T (&v)[KP][kLaneIids], int nv,
                                         T (&acc)[KP]) {
#pragma unroll
    for (int c = 0; c < KP; c++) acc[c] = (T)0;
#pragma unroll
    for (int j = 0; j < kLaneIids; j++) {
        const T z = sel4(l[0], l[1], l[2], l[3], (w >> (2 * j)) & 3u);
#pragma unroll
        for (int c = 0; c < KP; c++) {
            const T r = fma_t(z, v[c][j], acc[c]);
            acc[c] = (!TAIL || j < nv) ? r : acc[c];
        }
    }
}

template <typename T, int KP>
__global__ __launch_bounds__(kBlock) void k_packed_tdot(const uint8_t* __restrict__ packed, uint64_t pitch, uint64_t n,
                                                        uint64_t m, const T* __restrict__ lut,
                                                        const T* __restrict__ V, uint64_t ldv,
                                                        T* __restrict__ part, uint64_t tiles) {
    __shared__ T red[kWaves][kTdotSub][KP];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t chunk = blockIdx.x / tiles, tile = blockIdx.x - chunk * tiles;
    const uint64_t s_begin = tile * kTdotSnps, s_end = min(s_begin + kTdotSnps, m);
    const uint64_t i_wave = chunk * kChunk + (uint64_t)wave * kSpan;      // wave-uniform
    const uint64_t i_lane = i_wave + (uint64_t)lane * kLaneIids;
    const bool wave_on = i_wave < n;                                        // wave-uniform
    const bool tail = i_wave + kSpan > n;                                   // wave-uniform
    // waves of this chunk that hold iids (block-uniform): only their sums are folded
    const int waves_on = (int)min<uint64_t>(kWaves, (n - chunk * kChunk + kSpan - 1) / kSpan);
    const int nv = i_lane >= n ? 0 : (int)min<uint64_t>(kLaneIids, n - i_lane);
    T v[KP][kLaneIids];
#pragma unroll
    for (int c = 0; c < KP; c++)
#pragma unroll
        for (int j = 0; j < kLaneIids; j++) v[c][j] = j < nv ? V[(uint64_t)c * ldv + i_lane + j] : (T)0;
    // a lane without iids reads no code word (its word may lie past the pitch)
    const uint32_t* col = reinterpret_cast<const uint32_t*>(packed) + i_lane / kLaneIids;
    const uint64_t wpitch = pitch / 4;
    for (uint64_t s0 = s_begin; s0 < s_end; s0 += kTdotSub) {
        const int cnt = (int)min<uint64_t>(kTdotSub, s_end - s0);
        if (wave_on) {
            for (int b = 0; b < cnt; b += kLoads) {
                uint32_t w[kLoads];
#pragma unroll
                for (int u = 0; u < kLoads; u++) w[u] = (b + u < cnt && nv > 0) ? col[(s0 + b + u) * wpitch] : 0u;
#pragma unroll
                for (int u = 0; u < kLoads; u++) {
                    if (b + u >= cnt) break;
                    const T* l = lut + 4 * (s0 + b + u);
                    T acc[KP];
                    if (tail) tdot_snp<T, KP, true>(w[u], l, v, nv, acc);
                    else tdot_snp<T, KP, false>(w[u], l, v, nv, acc);
#pragma unroll
                    for (int c = 0; c < KP; c++) acc[c] = wave_sum(acc[c]);
                    if (lane == 0) {
#pragma unroll
                        for (int c = 0; c < KP; c++) red[wave][b + u][c] = acc[c];
                    }
                }
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * KP; e += kBlock) {
            const int c = e / cnt, q = e - c * cnt;
            T sum = red[0][q][c];
            for (int x = 1; x < waves_on; x++) sum += red[x][q][c];
            part[(chunk * KP + c) * m + s0 + q] = sum;
        }
        __syncthreads();
    }
}

// G[s, c] = the chunks' partials added in chunk order, in f64, rounded once
template <typename T>
__global__ __launch_bounds__(kBlock) void k_tdot_reduce(const T* __restrict__ part, uint64_t chunks, uint64_t kp,
                                                        uint64_t m, T* __restrict__ G, uint64_t ldg) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= kp * m) return;
    const uint64_t c = e / m, s = e - c * m;
    double sum = 0.0;
    for (uint64_t q = 0; q < chunks; q++) sum += (double)part[(q * kp + c) * m + s];
    G[c * ldg + s] = (T)sum;
}

// ------------------------------------------------------------------ Z W
// Workgroup = (four iid spans of 1024, one SNP segment of kSeg); wave w owns span 4 blockIdx + w,
// lane l the 16 iids of code word l with 16 x KP accumulators.  Per SNP: one code word per lane, the
// LUT and W[s, :] wave-uniform.  The segment's sums go to the slab part[segment][c][i] (rows of
// n_pad = round_up(n, 16) elements, so every lane with an iid stores its 16 whole).
template <typename T, int KP>
__global__ __launch_bounds__(kBlock) void k_packed_dot(const uint8_t* __restrict__ packed, uint64_t pitch, uint64_t n,
                                                       uint64_t m, const T* __restrict__ lut,
                                                       const T* __restrict__ W, uint64_t ldw, T* __restrict__ part,
                                                       uint64_t n_pad, uint64_t span_blocks) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t seg = blockIdx.x / span_blocks, sb = blockIdx.x - seg * span_blocks;
    const uint64_t i_lane = (sb * kWaves + wave) * kSpan + (uint64_t)lane * kLaneIids;
    if (i_lane >= n) return;  // no barrier below; a lane without iids reads no code word
    const uint64_t s_begin = seg * kSeg, s_end = min(s_begin + kSeg, m);
    const uint32_t* col = reinterpret_cast<const uint32_t*>(packed) + i_lane / kLaneIids;
    const uint64_t wpitch = pitch / 4;
    T acc[KP][kLaneIids];
#pragma unroll
    for (int c = 0; c < KP; c++)
#pragma unroll
        for (int j = 0; j < kLaneIids; j++) acc[c][j] = (T)0;
    for (uint64_t s0 = s_begin; s0 < s_end; s0 += kLoads) {
        const int cnt = (int)min<uint64_t>(kLoads, s_end - s0);
        uint32_t w[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; u++) w[u] = u < cnt ? col[(s0 + u) * wpitch] : 0u;
#pragma unroll
        for (int u = 0; u < kLoads; u++) {
            if (u >= cnt) break;
            const uint64_t s = s0 + u;
            const T l0 = lut[4 * s], l1 = lut[4 * s + 1], l2 = lut[4 * s + 2], l3 = lut[4 * s + 3];
            T wc[KP];
#pragma unroll
            for (int c = 0; c < KP; c++) wc[c] = W[(uint64_t)c * ldw + s];
#pragma unroll
            for (int j = 0; j < kLaneIids; j++) {
                const T z = sel4(l0, l1, l2, l3, (w[u] >> (2 * j)) & 3u);
#pragma unroll
                for (int c = 0; c < KP; c++) acc[c][j] = fma_t(z, wc[c], acc[c][j]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < KP; c++) {
        // 64-byte aligned: n_pad and i_lane are multiples of 16 elements
        T* o = (T*)__builtin_assume_aligned(part + (seg * KP + c) * n_pad + i_lane, 64);
#pragma unroll
        for (int j = 0; j < kLaneIids; j++) o[j] = acc[c][j];
    }
}

// Y[i, c] = ((Y[i, c] or 0) + p_0) + p_1 + ... in dtype, p_j the segments' partials in order: the
// fold a sequence of accumulating calls over segment-multiple chunks performs too, add by add
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dot_reduce(const T* __restrict__ part, uint64_t segs, uint64_t kp,
                                                       uint64_t n, uint64_t n_pad, T* __restrict__ Y, uint64_t ldy,
                                                       int accumulate) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= kp * n) return;
    const uint64_t c = e / n, i = e - c * n;
    T y = accumulate ? Y[c * ldy + i] : (T)0;
    for (uint64_t q = 0; q < segs; q++) y = y + part[(q * kp + c) * n_pad + i];
    Y[c * ldy + i] = y;
}

// largest instantiated panel <= left (1, 2, 4, 8): any k is served by repeated panels
template <typename T>
int panel_width(uint64_t left) {
    int kp = kPanel<T>;
    while ((uint64_t)kp > left) kp >>= 1;
    return kp;
}

// the kernel of panel width kp (only the widths up to the dtype's kPanel are instantiated)
template <typename T, typename... A>
void tdot_panel(int kp, unsigned grid, hipStream_t st, A... a) {
    if constexpr (kPanel<T> >= 8) {
        if (kp == 8) return (void)k_packed_tdot<T, 8><<<grid, kBlock, 0, st>>>(a...);
    }
    if (kp == 4) k_packed_tdot<T, 4><<<grid, kBlock, 0, st>>>(a...);
    else if (kp == 2) k_packed_tdot<T, 2><<<grid, kBlock, 0, st>>>(a...);
    else k_packed_tdot<T, 1><<<grid, kBlock, 0, st>>>(a...);
}
template <typename T, typename... A>
void dot_panel(int kp, unsigned grid, hipStream_t st, A... a) {
    if constexpr (kPanel<T> >= 8) {
        if (kp == 8) return (void)k_packed_dot<T, 8><<<grid, kBlock, 0, st>>>(a...);
    }
    if (kp == 4) k_packed_dot<T, 4><<<grid, kBlock, 0, st>>>(a...);
    else if (kp == 2) k_packed_dot<T, 2><<<grid, kBlock, 0, st>>>(a...);
    else k_packed_dot<T, 1><<<grid, kBlock, 0, st>>>(a...);
}

template <typename T>
void tdot_t(Device& d, const uint8_t* packed, uint64_t pitch, uint64_t n, uint64_t m, const T* lut, const T* V,
            uint64_t ldv, uint64_t k, T* G, uint64_t ldg, hipStream_t st) {
    const uint64_t chunks = ceil_div(n, kChunk);
    // SNPs per launch: whole tiles, the slab part[chunks][kp][mt] within kSlabBytes (a SNP's row does
    // not depend on the split)
    const uint64_t fit = kSlabBytes / (chunks * kPanel<T> * sizeof(T)) / kTdotSnps * kTdotSnps;
    const uint64_t step = std::max<uint64_t>(kTdotSnps, fit);
    T* part = (T*)d.get(Device::S_MATVEC, chunks * kPanel<T> * std::min(step, m) * sizeof(T));
    for (uint64_t c0 = 0; c0 < k;) {
        const int kp = panel_width<T>(k - c0);
        for (uint64_t s0 = 0; s0 < m; s0 += step) {
            const uint64_t mt = std::min(step, m - s0), tiles = ceil_div(mt, kTdotSnps);
            const uint8_t* P = packed + s0 * pitch;
            const T* L = lut + 4 * s0;
            const T* Vp = V + c0 * ldv;
            tdot_panel<T>(kp, (unsigned)(chunks * tiles), st, P, pitch, n, mt, L, Vp, ldv, part, tiles);
            SNPMI_HIP(hipGetLastError());
            k_tdot_reduce<T><<<(unsigned)ceil_div((uint64_t)kp * mt, kBlock), kBlock, 0, st>>>(
                part, chunks, (uint64_t)kp, mt, G + c0 * ldg + s0, ldg);
            SNPMI_HIP(hipGetLastError());
        }
        c0 += kp;
    }
}

template <typename T>
void dot_t(Device& d, const uint8_t* packed, uint64_t pitch, uint64_t n, uint64_t m, const T* lut, const T* W,
           uint64_t ldw, uint64_t k, T* Y, uint64_t ldy, int accumulate, hipStream_t st) {
    const uint64_t n_pad = round_up(n, kLaneIids), span_blocks = ceil_div(n, kChunk), segs = ceil_div(m, kSeg);
    // segments per launch: the slab part[segments][kp][n_pad] within kSlabBytes; the groups are folded
    // one after the other into Y, which continues the same global fold
    const uint64_t group = std::max<uint64_t>(1, kSlabBytes / (kPanel<T> * n_pad * sizeof(T)));
    T* part = (T*)d.get(Device::S_MATVEC, std::min(group, std::max<uint64_t>(segs, 1)) * kPanel<T> * n_pad * sizeof(T));
    for (uint64_t c0 = 0; c0 < k;) {
        const int kp = panel_width<T>(k - c0);
        const unsigned rgrid = (unsigned)ceil_div((uint64_t)kp * n, kBlock);
        if (segs == 0) {  // no SNPs: zeros (callers pass accumulate == 0 here)
            k_dot_reduce<T><<<rgrid, kBlock, 0, st>>>(part, 0, (uint64_t)kp, n, n_pad, Y + c0 * ldy, ldy, 0);
            SNPMI_HIP(hipGetLastError());
        }
        for (uint64_t g0 = 0; g0 < segs; g0 += group) {
            const uint64_t gs = std::min(group, segs - g0), s0 = g0 * kSeg, mt = std::min(gs * kSeg, m - s0);
            const uint8_t* P = packed + s0 * pitch;
            const T* L = lut + 4 * s0;
            const T* Wp = W + c0 * ldw + s0;
            dot_panel<T>(kp, (unsigned)(gs * span_blocks), st, P, pitch, n, mt, L, Wp, ldw, part, n_pad, span_blocks);
            SNPMI_HIP(hipGetLastError());
            k_dot_reduce<T><<<rgrid, kBlock, 0, st>>>(part, gs, (uint64_t)kp, n, n_pad, Y + c0 * ldy, ldy,
                                                      (accumulate || g0 > 0) ? 1 : 0);
            SNPMI_HIP(hipGetLastError());
        }
        c0 += kp;
    }
}

void check_packed(const void* packed, uint64_t pitch, uint64_t n, uint64_t m, const void* lut, int dtype) {
    SNPMI_REQUIRE(dtype == SNPMI_DT_F32 || dtype == SNPMI_DT_F64, SNPMI_E_ARG, "dtype must be f32 or f64");
    SNPMI_REQUIRE(pitch % 64 == 0 && pitch >= ceil_div(n, 4), SNPMI_E_ARG, "pitch must be snpmi_packed_pitch");
    SNPMI_REQUIRE((packed != nullptr && lut != nullptr) || n == 0 || m == 0, SNPMI_E_ARG, "packed or lut is NULL");
    // one launch's grid and the kernels' 64-bit indices bound the shape far above any real one
    SNPMI_REQUIRE(n < (1ull << 40) && m < (1ull << 40), SNPMI_E_ARG, "shape too large");
}

}  // namespace
}  // namespace snpmi

using namespace snpmi;

extern "C" {

int snpmi_dev_packed_tdot(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, const void* lut,
                          int dtype, const void* V, uint64_t ldv, uint64_t k, void* G, uint64_t ldg) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(call_mutex());  // the partials' scratch slot
        check_packed(packed, pitch, n_iid, n_sid, lut, dtype);
        SNPMI_REQUIRE(ldv >= n_iid, SNPMI_E_ARG, "ldv is below n_iid");
        SNPMI_REQUIRE(ldg >= n_sid, SNPMI_E_ARG, "ldg is below n_sid");
        if (n_iid == 0 || n_sid == 0 || k == 0) return;
        SNPMI_REQUIRE(G != nullptr && (V != nullptr || n_iid == 0), SNPMI_E_ARG, "V or G is NULL");
        Device& d = device();
        if (dtype == SNPMI_DT_F32)
            tdot_t<float>(d, packed, pitch, n_iid, n_sid, (const float*)lut, (const float*)V, ldv, k, (float*)G, ldg,
                          stream());
        else
            tdot_t<double>(d, packed, pitch, n_iid, n_sid, (const double*)lut, (const double*)V, ldv, k, (double*)G,
                           ldg, stream());
    });
}

int snpmi_dev_packed_dot(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, const void* lut,
                         int dtype, const void* W, uint64_t ldw, uint64_t k, void* Y, uint64_t ldy, int accumulate) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(call_mutex());  // the partials' scratch slot
        check_packed(packed, pitch, n_iid, n_sid, lut, dtype);
        SNPMI_REQUIRE(ldw >= n_sid, SNPMI_E_ARG, "ldw is below n_sid");
        SNPMI_REQUIRE(ldy >= n_iid, SNPMI_E_ARG, "ldy is below n_iid");
        if (n_iid == 0 || k == 0 || (n_sid == 0 && accumulate)) return;
        SNPMI_REQUIRE(Y != nullptr && (W != nullptr || n_sid == 0), SNPMI_E_ARG, "W or Y is NULL");
        Device& d = device();
        if (dtype == SNPMI_DT_F32)
            dot_t<float>(d, packed, pitch, n_iid, n_sid, (const float*)lut, (const float*)W, ldw, k, (float*)Y, ldy,
                         accumulate, stream());
        else
            dot_t<double>(d, packed, pitch, n_iid, n_sid, (const double*)lut, (const double*)W, ldw, k, (double*)Y,
                          ldy, accumulate, stream());
    });
}

}  // extern "C"
