// SNP pairs straight from the 2-bit codes (gfx950): the value of pair (a, b) at iid i is
// lut0[4 a + code0(i, a)] * lut1[4 b + code1(i, b)], one IEEE multiply in dtype -- the columns of the
// reference's Pairs reader (snpreader/pairs.py:135-152), which multiplies two standardized SnpData on
// the host.
//   k_pair_values_f   a pair list -> values, F order (the k_decode_f store pattern)
//   k_pair_values_c   the same, C order (correct, no rate asked of it)
//   k_pair_tdot       G = Zp^T V over ALL pairs of two SNP blocks; no pair column is written
// Plain VALU code, vector stores only, no atomics; every sum has one fixed order, so results are the
// same bits on every run.  Built with -ffp-contract=off like the rest of the library: the pair value
// is rounded in dtype before the spelled-out FMA takes it.
#include "snpmi_internal.hpp"

namespace snpmi {
namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kLaneIids = 16;                      // one 32-bit code word of each SNP per lane
constexpr uint64_t kSpan = kWave * kLaneIids;      // iids of one wave: 1024 (256 B of codes per SNP)
constexpr uint64_t kChunk = kWaves * kSpan;        // tdot: iids of one workgroup per step of its chunk loop: 4096
constexpr int kValuesItems = 4;                    // values, F order: (pair, 1024-iid span) items per wave per iteration
constexpr int kPairTA = 8;                         // tdot: left SNPs of a workgroup's tile
constexpr int kPairTB = 32;                        // tdot: right SNPs of a workgroup's tile
constexpr int kLoads = 8;                          // tdot: right code words in flight per lane
static_assert(kPairTA * kPairTB == kBlock, "one thread per pair of the tile folds the waves' sums");
// tdot: widest column panel per dtype (16 iids x panel values of V in 64 VGPRs), and the left SNPs
// whose 16 decoded values a lane holds while it walks the tile's right SNPs (64 VGPRs)
template <typename T>
constexpr int kPairPanel = sizeof(T) == 4 ? 4 : 2;
template <typename T>
constexpr int kPairHeld = sizeof(T) == 4 ? 4 : 2;

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef double f64x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the 4-entry LUT select of kernels.hip: three v_cndmask, no divergent branch
template <typename T>
__device__ __forceinline__ T sel4(const T* __restrict__ l, uint32_t c) {
    const T l0 = l[0], l1 = l[1], l2 = l[2], l3 = l[3];
    const bool b0 = (c & 1u) != 0, b1 = (c & 2u) != 0;
    const T lo = b0 ? l1 : l0;
    const T hi = b0 ? l3 : l2;
    return b1 ? hi : lo;
}
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

template <typename V>
__device__ __forceinline__ void store_nt(V* p, const V& v) {
    __builtin_nontemporal_store(v, p);
}

// One side of a pair: packed codes [.][pitch] and the value table [.][4]
template <typename T>
struct Side {
    const uint8_t* packed;
    uint64_t pitch;
    const T* lut;
};

// ------------------------------------------------------------------ values, F order
// k_decode_f with two code words: wave work item = (pair c, span of 1024 iids).  Each lane loads the
// one dword (16 iids) of either SNP; the codes are redistributed with ds_bpermute (__shfl) so every
// store instruction writes 1 KiB contiguous (f32: 4 rounds of 16-B stores; f64: 8 rounds), U items
// per wave per iteration with all 2 U loads issued first, non-temporal stores, XCD-sliced item order
// (the grid is a multiple of 8).  An element is sel4(table 0) * sel4(table 1): the
// product a 16-entry table of the pair would hold, bit for bit, at 7 VALU per element against the 15
// selects of a 16-way register table.  Nothing is stored at or beyond iid n, so the
// unused codes of a column's last byte and the pad bytes never reach the output.
template <typename T, int U>
__global__ __launch_bounds__(kBlock) void k_pair_values_f(Side<T> s0, Side<T> s1, uint64_t n,
                                                          const uint32_t* __restrict__ idx0,
                                                          const uint32_t* __restrict__ idx1, uint64_t pairs,
                                                          T* __restrict__ out, uint64_t ld) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t spans = (n + kSpan - 1) / kSpan;
    const uint64_t total = spans * pairs;
    const uint64_t groups = (total + U - 1) / U;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    const uint64_t lb = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    for (uint64_t gi = lb * kWaves + threadIdx.x / kWave; gi < groups; gi += nwaves) {
        uint32_t w0[U], w1[U];
        uint64_t av[U], bv[U], cv[U], qv[U];
        bool val[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t it = gi * U + u;
            val[u] = it < total;  // wave-uniform
            const uint64_t c = val[u] ? it / spans : 0, q = it - c * spans;
            cv[u] = c;
            qv[u] = q;
            av[u] = val[u] ? idx0[c] : 0;
            bv[u] = val[u] ? idx1[c] : 0;
            // a lane without iids reads no code word (its word may lie past the pitch)
            const bool ok = val[u] && (q * kSpan + (uint64_t)kLaneIids * lane < n);
            w0[u] = ok ? reinterpret_cast<const uint32_t*>(s0.packed + av[u] * s0.pitch)[q * kWave + lane] : 0u;
            w1[u] = ok ? reinterpret_cast<const uint32_t*>(s1.packed + bv[u] * s1.pitch)[q * kWave + lane] : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (!val[u]) continue;
            const uint64_t i0 = qv[u] * kSpan;
            const T* la = s0.lut + 4 * av[u];
            const T* lb4 = s1.lut + 4 * bv[u];
            const T a0 = la[0], a1 = la[1], a2 = la[2], a3 = la[3];
            const T b0 = lb4[0], b1 = lb4[1], b2 = lb4[2], b3 = lb4[3];
            T* o = out + cv[u] * ld + i0;
            if constexpr (sizeof(T) == 4) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int from = r * 16 + (lane >> 2), sh = 8 * (lane & 3);
                    const uint32_t x = (__shfl(w0[u], from, kWave) >> sh) & 0xffu;
                    const uint32_t y = (__shfl(w1[u], from, kWave) >> sh) & 0xffu;
                    const uint64_t i = i0 + r * 256 + 4 * lane;
                    f32x4_t v;
                    v.x = sel4(a0, a1, a2, a3, x & 3u) * sel4(b0, b1, b2, b3, y & 3u);
                    v.y = sel4(a0, a1, a2, a3, (x >> 2) & 3u) * sel4(b0, b1, b2, b3, (y >> 2) & 3u);
                    v.z = sel4(a0, a1, a2, a3, (x >> 4) & 3u) * sel4(b0, b1, b2, b3, (y >> 4) & 3u);
                    v.w = sel4(a0, a1, a2, a3, x >> 6) * sel4(b0, b1, b2, b3, y >> 6);
                    if (i + 4 <= n) {
                        store_nt(reinterpret_cast<f32x4_t*>(o + r * 256 + 4 * lane), v);
                    } else {
                        for (int t = 0; t < 4; t++)
                            if (i + t < n) o[r * 256 + 4 * lane + t] = v[t];
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    const int from = r * 8 + (lane >> 3), sh = 8 * ((lane >> 1) & 3) + 4 * (lane & 1);
                    const uint32_t x = (__shfl(w0[u], from, kWave) >> sh) & 0xfu;
                    const uint32_t y = (__shfl(w1[u], from, kWave) >> sh) & 0xfu;
                    const uint64_t i = i0 + r * 128 + 2 * lane;
                    f64x2_t v;
                    v.x = sel4(a0, a1, a2, a3, x & 3u) * sel4(b0, b1, b2, b3, y & 3u);
                    v.y = sel4(a0, a1, a2, a3, x >> 2) * sel4(b0, b1, b2, b3, y >> 2);
                    if (i + 2 <= n) {
                        store_nt(reinterpret_cast<f64x2_t*>(o + r * 128 + 2 * lane), v);
                    } else if (i < n) {
                        o[r * 128 + 2 * lane] = v.x;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------ values, C order
// one thread per element, the pairs of a row across the lanes
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pair_values_c(Side<T> s0, Side<T> s1, uint64_t n,
                                                          const uint32_t* __restrict__ idx0,
                                                          const uint32_t* __restrict__ idx1, uint64_t pairs,
                                                          T* __restrict__ out, uint64_t ld) {
    const uint64_t total = n * pairs, step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += step) {
        const uint64_t i = e / pairs, c = e - i * pairs;
        const uint64_t a = idx0[c], b = idx1[c];
        const uint32_t sh = 2 * (uint32_t)(i & 3);
        const uint32_t x = (s0.packed[a * s0.pitch + i / 4] >> sh) & 3u;
        const uint32_t y = (s1.packed[b * s1.pitch + i / 4] >> sh) & 3u;
        out[i * ld + c] = s0.lut[4 * a + x] * s1.lut[4 * b + y];
    }
}

// ------------------------------------------------------------------ Zp^T V over a rectangle of pairs
// Workgroup = one tile of kPairTA x kPairTB SNPs, all iids: it walks the iid chunks of 4096 in order.
// In a chunk wave w owns iids [chunk + 1024 w, + 1024), lane l the 16 of them in code word l of every
// SNP.  The lane's 16 x KP values of V are loaded once per chunk; the 16 decoded values of RA left
// SNPs are held while the lane walks the tile's right SNPs, each decoded once per held group.  Per
// pair and column: p = za * zb rounded in T, then one FMA chain over the lane's 16 iids from zero,
// the wave's 64 lanes by the xor butterfly, and the chunk's waves in wave order through LDS (thread t
// = pair (t / kPairTB, t % kPairTB) of the tile).  The chunks' sums are added in chunk order in f64
// in that thread's registers and rounded once.  So a pair's row depends on its two SNPs, their tables
// and V alone -- not on its place in the tile or on the rectangle.
// A genotype with iid >= n counts as zero on both sides whatever its codes and the tables say, so its
// term is fma(0, 0, acc) = acc.  Tiles with no b >= b_lo[a] for any of their a's return at once.
template <typename T, int KP>
__global__ __launch_bounds__(kBlock) void k_pair_tdot(Side<T> A, uint64_t n_a, Side<T> B, uint64_t n_b, uint64_t n,
                                                      const int64_t* __restrict__ row_off,
                                                      const uint32_t* __restrict__ b_lo, const T* __restrict__ V,
                                                      uint64_t ldv, T* __restrict__ G, uint64_t ldg, uint64_t tiles_b) {
    constexpr int RA = kPairHeld<T>;
    __shared__ T red[kWaves][kBlock][KP];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t ta = blockIdx.x / tiles_b, tb = blockIdx.x - ta * tiles_b;
    const uint64_t a0 = ta * kPairTA, b0 = tb * kPairTB;
    const int na = (int)min<uint64_t>(kPairTA, n_a - a0), nb = (int)min<uint64_t>(kPairTB, n_b - b0);
    bool any = false;  // block-uniform
    for (int a = 0; a < na; a++) any = any || (b_lo ? (uint64_t)b_lo[a0 + a] : 0) < b0 + nb;
    if (!any) return;
    const int pa = threadIdx.x / kPairTB, pb = threadIdx.x - pa * kPairTB;  // this thread's pair in the folds
    const bool mine = pa < na && pb < nb;
    double sum[KP];
#pragma unroll
    for (int c = 0; c < KP; c++) sum[c] = 0.0;
    const uint64_t wpa = A.pitch / 4, wpb = B.pitch / 4;
    const uint64_t chunks = (n + kChunk - 1) / kChunk;
    for (uint64_t chunk = 0; chunk < chunks; chunk++) {
        const uint64_t i_wave = chunk * kChunk + (uint64_t)wave * kSpan;  // wave-uniform
        const uint64_t i_lane = i_wave + (uint64_t)lane * kLaneIids;
        const int nv = i_lane >= n ? 0 : (int)min<uint64_t>(kLaneIids, n - i_lane);
        // waves of this chunk that hold iids (block-uniform): only their sums are folded
        const int waves_on = (int)min<uint64_t>(kWaves, (n - chunk * kChunk + kSpan - 1) / kSpan);
        if (i_wave < n) {
            T v[KP][kLaneIids];
#pragma unroll
            for (int c = 0; c < KP; c++)
#pragma unroll
                for (int j = 0; j < kLaneIids; j++) v[c][j] = j < nv ? V[(uint64_t)c * ldv + i_lane + j] : (T)0;
            // a lane without iids reads no code word (its word may lie past the pitch)
            const uint32_t* col_a = reinterpret_cast<const uint32_t*>(A.packed) + i_lane / kLaneIids;
            const uint32_t* col_b = reinterpret_cast<const uint32_t*>(B.packed) + i_lane / kLaneIids;
            for (int ag = 0; ag < na; ag += RA) {
                T za[RA][kLaneIids];
#pragma unroll
                for (int r = 0; r < RA; r++) {
                    const bool on = ag + r < na;  // block-uniform
                    const uint32_t w = (on && nv > 0) ? col_a[(a0 + ag + r) * wpa] : 0u;
                    const T* l = A.lut + 4 * (a0 + (on ? ag + r : 0));
#pragma unroll
                    for (int j = 0; j < kLaneIids; j++) {
                        const T z = sel4(l, (w >> (2 * j)) & 3u);
                        za[r][j] = j < nv ? z : (T)0;
                    }
                }
                for (int bq = 0; bq < nb; bq += kLoads) {
                    uint32_t w[kLoads];
#pragma unroll
                    for (int u = 0; u < kLoads; u++) w[u] = (bq + u < nb && nv > 0) ? col_b[(b0 + bq + u) * wpb] : 0u;
#pragma unroll
                    for (int u = 0; u < kLoads; u++) {
                        if (bq + u >= nb) break;
                        const T* l = B.lut + 4 * (b0 + bq + u);
                        T zb[kLaneIids];
#pragma unroll
                        for (int j = 0; j < kLaneIids; j++) {
                            const T z = sel4(l, (w[u] >> (2 * j)) & 3u);
                            zb[j] = j < nv ? z : (T)0;
                        }
#pragma unroll
                        for (int r = 0; r < RA; r++) {
                            if (ag + r >= na) break;
                            T acc[KP];
#pragma unroll
                            for (int c = 0; c < KP; c++) acc[c] = (T)0;
#pragma unroll
                            for (int j = 0; j < kLaneIids; j++) {
                                const T p = za[r][j] * zb[j];  // the pair's value, rounded in T
#pragma unroll
                                for (int c = 0; c < KP; c++) acc[c] = fma_t(p, v[c][j], acc[c]);
                            }
#pragma unroll
                            for (int c = 0; c < KP; c++) acc[c] = wave_sum(acc[c]);
                            if (lane == 0) {
#pragma unroll
                                for (int c = 0; c < KP; c++) red[wave][(ag + r) * kPairTB + bq + u][c] = acc[c];
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int c = 0; c < KP; c++) {
                T s = red[0][threadIdx.x][c];
                for (int x = 1; x < waves_on; x++) s += red[x][threadIdx.x][c];
                sum[c] += (double)s;
            }
        }
        __syncthreads();
    }
    if (!mine) return;
    const uint64_t a = a0 + pa, b = b0 + pb;
    if (b < (b_lo ? (uint64_t)b_lo[a] : 0)) return;
    const int64_t row = (row_off ? row_off[a] : (int64_t)(a * n_b)) + (int64_t)b;
#pragma unroll
    for (int c = 0; c < KP; c++) G[(uint64_t)c * ldg + (uint64_t)row] = (T)sum[c];
}

unsigned grid_cap(uint64_t blocks, uint64_t cap) { return (unsigned)std::max<uint64_t>(1, std::min(blocks, cap)); }

template <typename T>
void values_t(const Side<T>& s0, const Side<T>& s1, uint64_t n, const uint32_t* idx0, const uint32_t* idx1,
              uint64_t pairs, int order_c, T* out, uint64_t ld, hipStream_t st) {
    if (order_c) {
        k_pair_values_c<T><<<grid_cap(ceil_div(n * pairs, kBlock), 256 * 64), kBlock, 0, st>>>(s0, s1, n, idx0, idx1,
                                                                                              pairs, out, ld);
    } else {
        // the decode's grid: kValuesItems items per wave, 8x more blocks than the resident waves hold,
        // a multiple of 8 for the XCD-sliced item order
        const uint64_t waves = ceil_div(ceil_div(n, kSpan) * pairs, kValuesItems);
        const unsigned g8 = (unsigned)round_up(grid_cap(ceil_div(waves, kWaves), 256 * 16 * 8), 8);
        k_pair_values_f<T, kValuesItems><<<g8, kBlock, 0, st>>>(s0, s1, n, idx0, idx1, pairs, out, ld);
    }
    SNPMI_HIP(hipGetLastError());
}

// largest instantiated panel <= left (1, 2, 4): any k is served by repeated panels
template <typename T>
int panel_width(uint64_t left) {
    int kp = kPairPanel<T>;
    while ((uint64_t)kp > left) kp >>= 1;
    return kp;
}

template <typename T>
void tdot_t(const Side<T>& A, uint64_t n_a, const Side<T>& B, uint64_t n_b, uint64_t n, const int64_t* row_off,
            const uint32_t* b_lo, const T* V, uint64_t ldv, uint64_t k, T* G, uint64_t ldg, hipStream_t st) {
    const uint64_t tiles_b = ceil_div(n_b, kPairTB);
    // rows of tiles per launch: one launch's grid stays below 2^31 blocks
    const uint64_t rows = std::max<uint64_t>(1, (1ull << 30) / tiles_b);
    for (uint64_t c0 = 0; c0 < k;) {
        const int kp = panel_width<T>(k - c0);
        for (uint64_t t0 = 0; t0 < ceil_div(n_a, kPairTA); t0 += rows) {
            const uint64_t a0 = t0 * kPairTA, na = std::min(rows * kPairTA, n_a - a0);
            const unsigned grid = (unsigned)(ceil_div(na, kPairTA) * tiles_b);
            Side<T> At = {A.packed + a0 * A.pitch, A.pitch, A.lut + 4 * a0};
            const uint32_t* lo = b_lo ? b_lo + a0 : nullptr;
            // without a table the row of (a, b) is a n_b + b: the launch's first row moves G instead
            const int64_t* ro = row_off ? row_off + a0 : nullptr;
            T* Gp = G + c0 * ldg + (row_off ? 0 : a0 * n_b);
            const T* Vp = V + c0 * ldv;
            if constexpr (kPairPanel<T> >= 4) {
                if (kp == 4) k_pair_tdot<T, 4><<<grid, kBlock, 0, st>>>(At, na, B, n_b, n, ro, lo, Vp, ldv, Gp, ldg, tiles_b);
            }
            if (kp == 2) k_pair_tdot<T, 2><<<grid, kBlock, 0, st>>>(At, na, B, n_b, n, ro, lo, Vp, ldv, Gp, ldg, tiles_b);
            else if (kp == 1) k_pair_tdot<T, 1><<<grid, kBlock, 0, st>>>(At, na, B, n_b, n, ro, lo, Vp, ldv, Gp, ldg, tiles_b);
            SNPMI_HIP(hipGetLastError());
        }
        c0 += kp;
    }
}

void check_side(const void* packed, uint64_t pitch, const void* lut, uint64_t n, bool used, const char* what) {
    SNPMI_REQUIRE(pitch % 64 == 0 && pitch >= ceil_div(n, 4), SNPMI_E_ARG,
                  std::string(what) + ": pitch must be snpmi_packed_pitch");
    SNPMI_REQUIRE((packed != nullptr && lut != nullptr) || !used, SNPMI_E_ARG, std::string(what) + ": packed or lut is NULL");
}

}  // namespace
}  // namespace snpmi

using namespace snpmi;

extern "C" {

int snpmi_dev_pair_values(const uint8_t* packed0, uint64_t pitch0, const void* lut0, const uint8_t* packed1,
                          uint64_t pitch1, const void* lut1, uint64_t n_iid, const uint32_t* idx0,
                          const uint32_t* idx1, uint64_t n_pairs, int dtype, int order_c, void* out, uint64_t ld) {
    return guarded([&] {
        SNPMI_REQUIRE(dtype == SNPMI_DT_F32 || dtype == SNPMI_DT_F64, SNPMI_E_ARG, "dtype must be f32 or f64");
        const bool used = n_iid != 0 && n_pairs != 0;
        check_side(packed0, pitch0, lut0, n_iid, used, "side 0");
        check_side(packed1, pitch1, lut1, n_iid, used, "side 1");
        if (!order_c) SNPMI_REQUIRE(ld % 16 == 0 && ld >= n_iid, SNPMI_E_ARG, "F-order ld must be >= n_iid, % 16");
        else SNPMI_REQUIRE(ld >= n_pairs, SNPMI_E_ARG, "C-order ld must be >= n_pairs");
        // the kernels' 64-bit indices bound the shape far above any real one
        SNPMI_REQUIRE(n_iid < (1ull << 40) && n_pairs < (1ull << 40), SNPMI_E_ARG, "shape too large");
        if (!used) return;
        SNPMI_REQUIRE(idx0 != nullptr && idx1 != nullptr && out != nullptr, SNPMI_E_ARG, "idx0, idx1 or out is NULL");
        SNPMI_REQUIRE(order_c || reinterpret_cast<uintptr_t>(out) % 16 == 0, SNPMI_E_ARG, "F-order out must be 16-byte aligned");
        device();
        if (dtype == SNPMI_DT_F32)
            values_t<float>({packed0, pitch0, (const float*)lut0}, {packed1, pitch1, (const float*)lut1}, n_iid, idx0,
                            idx1, n_pairs, order_c, (float*)out, ld, stream());
        else
            values_t<double>({packed0, pitch0, (const double*)lut0}, {packed1, pitch1, (const double*)lut1}, n_iid,
                             idx0, idx1, n_pairs, order_c, (double*)out, ld, stream());
    });
}

int snpmi_dev_pair_tdot(const uint8_t* packed_a, uint64_t pitch_a, const void* lut_a, uint64_t n_a,
                        const uint8_t* packed_b, uint64_t pitch_b, const void* lut_b, uint64_t n_b, uint64_t n_iid,
                        const int64_t* row_off, const uint32_t* b_lo, int dtype, const void* V, uint64_t ldv,
                        uint64_t k, void* G, uint64_t ldg) {
    return guarded([&] {
        SNPMI_REQUIRE(dtype == SNPMI_DT_F32 || dtype == SNPMI_DT_F64, SNPMI_E_ARG, "dtype must be f32 or f64");
        const bool used = n_iid != 0 && n_a != 0 && n_b != 0 && k != 0;
        check_side(packed_a, pitch_a, lut_a, n_iid, used, "side a");
        check_side(packed_b, pitch_b, lut_b, n_iid, used, "side b");
        SNPMI_REQUIRE(n_iid < (1ull << 40) && n_a < (1ull << 31) && n_b < (1ull << 31), SNPMI_E_ARG, "shape too large");
        SNPMI_REQUIRE(ldv >= n_iid, SNPMI_E_ARG, "ldv is below n_iid");
        // without row_off the rectangle's own n_a n_b rows are written; with it the caller's table
        // places them and the caller guarantees that every written row is below ldg (include/snpmi.h)
        SNPMI_REQUIRE(ldg >= n_a * n_b || row_off != nullptr, SNPMI_E_ARG, "ldg is below n_a * n_b");
        if (n_a == 0 || n_b == 0 || k == 0) return;
        SNPMI_REQUIRE(G != nullptr && (V != nullptr || n_iid == 0), SNPMI_E_ARG, "V or G is NULL");
        device();
        if (dtype == SNPMI_DT_F32)
            tdot_t<float>({packed_a, pitch_a, (const float*)lut_a}, n_a, {packed_b, pitch_b, (const float*)lut_b}, n_b,
                          n_iid, row_off, b_lo, (const float*)V, ldv, k, (float*)G, ldg, stream());
        else
            tdot_t<double>({packed_a, pitch_a, (const double*)lut_a}, n_a, {packed_b, pitch_b, (const double*)lut_b},
                           n_b, n_iid, row_off, b_lo, (const double*)V, ldv, k, (double*)G, ldg, stream());
    });
}

}  // extern "C"
