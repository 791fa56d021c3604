// SnpGen on the GPU (reference snpreader/snpgen.py:115-189): the reference's seeded generator,
// bit for bit.  Every SNP batch is one MT19937 stream (numpy's legacy RandomState, seeded with
// init_genrand(seed + batch * block_size)) consumed in a fixed order, so a batch is the unit of
// parallelism: ONE 256-thread workgroup per stream, and one launch (k_snpgen) per group of batches.
//
// A workgroup owns one scratch slot and is dealt batches round-robin (no workgroup ever waits on
// another).  For its batch it runs the reference's rejection rounds itself, with no host round trip:
//
//   generate  The 624-word state lives in LDS; the workgroup draws the round's B*(1+3n) doubles in
//             tiles of 256 (one per lane), regenerating the state when a tile runs past its end.
//             The first B doubles pick each SNP's MAF (searchsorted over the cdf), kept as 53-bit
//             integer thresholds; every later double becomes ONE bit (draw < MAF, or draw < 0.218
//             for the missing mask), and each wave stores its 64 bits as one word of the slot's bit
//             array, in the stream's native [iid][allele][sid] / [iid][sid] order.
//   count     per-SNP minor-allele sums c_j of the round, read back from the bit array.
//   plan      legality 1 <= c_j <= n, a prefix over the legal SNPs, their destination columns.
//   emit      transposes the newly placed columns that the caller asked for from the bit array into
//             packed 2-bit codes, straight into the caller's [n_sel][pitch] output.
//
// The stream simply continues into the next round while the batch is not full.  Scratch is per
// workgroup slot (about 3nB bits + 16 B per SNP of the batch), never per batch or per request;
// the number of slots is what the scratch budget and the device hold.
#include <algorithm>
#include <cmath>

#include "mt19937.hpp"
#include "snpmi_internal.hpp"

namespace snpmi {
namespace {

constexpr uint32_t kSmallB = 256;            // below: thresholds replicated in LDS (no per-lane modulo)
constexpr uint64_t kDefaultScratch = 1ull << 30;
constexpr uint32_t kMaxRounds = 4096;        // a batch that is not full by then is an error, not a hang
constexpr uint64_t kGroupPairs = 1ull << 22; // requested columns per launch (bounds the index tables)

__global__ __launch_bounds__(kGenBlock) void k_mt_sample(uint32_t seed, uint64_t count, double* out) {
    __shared__ __attribute__((aligned(8))) uint32_t key[kMtN];
    mt_seed(key, seed);
    uint32_t pos = kMtN;
    for (uint64_t p0 = 0; p0 < count; p0 += kGenBlock) {
        const uint32_t cnt = (uint32_t)min((uint64_t)kGenBlock, count - p0);
        const uint64_t v = mt_take(key, pos, cnt);
        if (threadIdx.x < cnt) out[p0 + threadIdx.x] = (double)v * 0x1p-53;
    }
}

struct GenTables {          // the same for every batch of a call
    const double* cdf;      // [n_pts] normalised cumulative MAF weights
    const uint64_t* thr_tab;  // [n_pts] ceil(MAF * 2^53)
    int n_pts;
    uint64_t thr_miss;      // ceil(0.218 * 2^53)
};

// One round's B*(1+3n) draws.  bw: bit q = draw B+q of the round.  Ends with a barrier.
__device__ __forceinline__ void gen_round(uint32_t* key, uint32_t& pos, uint64_t* thr_l, const GenTables& t,
                                          uint64_t n, uint32_t B, uint64_t* thr_g, uint64_t* bw) {
    const uint32_t l = threadIdx.x;
    // the round's first B doubles: SNP j's MAF = x[#{cdf <= u_j}], kept as the threshold
    // ceil(MAF * 2^53) (v / 2^53 < MAF  <=>  v < that, both sides exact)
    for (uint32_t j0 = 0; j0 < B; j0 += kGenBlock) {
        const uint32_t cnt = min(kGenBlock, B - j0);
        const uint64_t v = mt_take(key, pos, cnt);
        if (l < cnt) {
            const double u = (double)v * 0x1p-53;
            int lo = 0, hi = t.n_pts;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (t.cdf[mid] <= u) lo = mid + 1;
                else hi = mid;
            }
            thr_g[j0 + l] = t.thr_tab[min(lo, t.n_pts - 1)];
        }
    }
    __syncthreads();  // the thresholds are read back by other lanes below
    const bool small = B < kSmallB;
    if (small) {
        for (uint32_t x = l; x < 2 * kSmallB; x += kGenBlock) thr_l[x] = thr_g[x % B];
        __syncthreads();
    }
    // 2nB allele draws [iid][allele][sid], then nB missing draws [iid][sid]: one bit each
    const uint64_t na = 2 * n * B, total = 3 * n * B;
    const uint32_t step = kGenBlock % B;
    uint32_t jb = 0;  // q0 % B
    for (uint64_t q0 = 0; q0 < total; q0 += kGenBlock) {
        const uint32_t cnt = (uint32_t)min((uint64_t)kGenBlock, total - q0);
        const uint64_t v = mt_take(key, pos, cnt);
        uint64_t T = t.thr_miss;
        if (q0 + l < na) {
            uint32_t j = jb + l;
            if (small) {
                T = thr_l[j];
            } else {
                if (j >= B) j -= B;
                T = thr_g[j];
            }
        }
        const unsigned long long word = __ballot(l < cnt && v < T);
        if ((l & 63u) == 0 && l < cnt) bw[(q0 >> 6) + (l >> 6)] = word;
        jb += step;
        if (jb >= B) jb -= B;
    }
    __syncthreads();  // the bits are read back by other lanes
}

__device__ __forceinline__ uint32_t bit_at(const uint64_t* bw, uint64_t q) {
    return (uint32_t)(bw[q >> 6] >> (q & 63u)) & 1u;
}

// value of (iid i, SNP j) of the round: 0/1/2, or 3 = missing
__device__ __forceinline__ uint32_t round_value(const uint64_t* bw, uint64_t n, uint64_t B, uint64_t i, uint64_t j) {
    const uint64_t a = i * 2 * B + j;
    if (bit_at(bw, 2 * n * B + i * B + j)) return 3;
    return bit_at(bw, a) + bit_at(bw, a + B);
}

// cnt <= 32 bits from bit q on (the bit arrays keep one slack word, so the second load is in bounds)
__device__ __forceinline__ uint32_t bits_at(const uint64_t* bw, uint64_t q, uint32_t cnt) {
    const uint32_t s = (uint32_t)(q & 63u);
    uint64_t x = bw[q >> 6] >> s;
    if (s) x |= bw[(q >> 6) + 1] << (64 - s);
    return (uint32_t)x & (cnt >= 32 ? 0xffffffffu : (1u << cnt) - 1u);
}

// bit i -> bits 2i and 2i+1
__device__ __forceinline__ uint64_t spread_pairs(uint32_t m) {
    uint64_t x = m;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x | (x << 1);
}

// One-SNP batches (B = 1, the default from 50001 iids on): iid i's alleles are bits 2i, 2i+1 and
// its missing flag bit 2n+i, so sums and codes come from whole words.
// sum of the non-missing values of iids [32k, 32k+32)
__device__ __forceinline__ uint32_t b1_sum32(const uint64_t* bw, uint64_t n, uint64_t k) {
    const uint64_t i0 = k * 32;
    const uint32_t valid = (uint32_t)min((uint64_t)32, n - i0);
    uint64_t keep = ~spread_pairs(bits_at(bw, 2 * n + i0, valid));
    if (valid < 32) keep &= (1ull << (2 * valid)) - 1ull;
    return (uint32_t)__popcll(bw[k] & keep);
}
// packed byte of iids [4*byte, 4*byte+4)
__device__ __forceinline__ uint32_t b1_code(const uint64_t* bw, uint64_t n, uint64_t byte) {
    const uint32_t valid = (uint32_t)min((uint64_t)4, n - byte * 4);
    const uint32_t a = bits_at(bw, 8 * byte, 2 * valid), m = bits_at(bw, 2 * n + 4 * byte, valid);
    uint32_t code = 0;
    for (uint32_t k = 0; k < valid; k++) {
        const uint32_t v = ((a >> (2 * k)) & 1u) + ((a >> (2 * k + 1)) & 1u);
        code |= ((m >> k) & 1u ? 1u : v == 0 ? 0u : v + 1u) << (2 * k);
    }
    return code;
}

// The requested columns of one batch, sorted by the batch's own column: pairs [p0, p1) of
// (loc = column of the batch, outc = column of the caller's output).
struct Wanted {
    const uint32_t* loc;
    const uint64_t* outc;
    uint64_t p0, p1;
};

// One workgroup slot: takes batches until none are left.  Thread layout of count / emit: jt (a power
// of two <= 64) SNPs x 256/jt iid slices, so a batch of one SNP (the default at >= 50001 iids) still
// uses the whole workgroup.
// codes (count_A1 = False): 0 -> 00, missing -> 01, 1 -> 10, 2 -> 11; pad iids of the last byte 0
__global__ __launch_bounds__(kGenBlock) void k_snpgen(uint32_t n_batches, const uint32_t* seeds, const uint64_t* off,
                                                      const uint32_t* loc, const uint64_t* outc, uint64_t n, uint32_t B,
                                                      uint32_t jt, GenTables tab, uint64_t* thr, uint64_t* bits,
                                                      uint64_t W, uint32_t* csum, uint32_t* src, uint8_t* out,
                                                      uint64_t pitch, unsigned long long* totals) {
    __shared__ __attribute__((aligned(8))) uint32_t key[kMtN];
    __shared__ uint64_t thr_l[2 * kSmallB];
    __shared__ uint32_t acc[64];
    __shared__ uint32_t wsum[kGenBlock / 64];
    const uint32_t l = threadIdx.x, lane = l & 63u, wave = l >> 6;
    const uint32_t jj = l & (jt - 1), sl = l / jt, nsl = kGenBlock / jt;
    const uint64_t slot = blockIdx.x;
    uint64_t* thr_g = thr + slot * B;
    uint64_t* bw = bits + slot * W;
    uint32_t* cs = csum + slot * B;
    uint32_t* sc = src + slot * B;
    const uint64_t nb = (n + 3) / 4;
    // Batches are dealt to the slots round-robin.  Every loop that holds a barrier has scalar
    // (workgroup-uniform) control, and no lane-specific code sits at its ends, so all lanes reach
    // each barrier the same number of times.
    uint32_t all_rounds = 0, all_failed = 0;
    for (uint32_t b = blockIdx.x; b < n_batches; b += gridDim.x) {
        const Wanted want{loc, outc, off[b], off[b + 1]};
        mt_seed(key, seeds[b]);
        uint32_t pos = kMtN, fill = 0, rounds = 0;
        while (fill < B && rounds < kMaxRounds) {
            gen_round(key, pos, thr_l, tab, n, B, thr_g, bw);
            // ---- count: c_j = sum over the non-missing iids
            for (uint32_t jbase = 0; jbase < B; jbase += jt) {
                const uint32_t j = jbase + jj;
                if (l < 64) acc[l] = 0;
                __syncthreads();
                uint32_t sum = 0;
                if (B == 1) {
                    for (uint64_t k = l; k * 32 < n; k += kGenBlock) sum += b1_sum32(bw, n, k);
                } else if (j < B) {
#pragma unroll 4
                    for (uint64_t i = sl; i < n; i += nsl) {
                        const uint32_t v = round_value(bw, n, B, i, j);
                        sum += v == 3 ? 0 : v;
                    }
                }
                if (sum) atomicAdd(&acc[jj], sum);
                __syncthreads();
                if (l < jt && j < B) cs[j] = acc[l];
                __syncthreads();
            }
            // ---- plan: the legal SNPs, in order, fill the batch's next free columns
            uint32_t run = fill;  // (< 2B < 2^32)
            for (uint32_t j0 = 0; j0 < B && run < B; j0 += kGenBlock) {
                const uint32_t j = j0 + l;
                const uint32_t c = j < B ? cs[j] : 0;
                const bool legal = c >= 1 && c <= n;
                const unsigned long long m = __ballot(legal);
                if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
                __syncthreads();
                uint32_t before = 0, tot = 0;
                for (uint32_t k = 0; k < kGenBlock / 64; k++) {
                    if (k < wave) before += wsum[k];
                    tot += wsum[k];
                }
                const uint32_t d = run + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (legal && d < B) sc[d] = j;
                // (the same in every lane; read into an SGPR so the loops around stay scalar)
                run += (uint32_t)__builtin_amdgcn_readfirstlane((int)tot);
                __syncthreads();
            }
            const uint32_t nf = min(run, B);
            // ---- emit: the new columns the caller asked for, transposed into packed codes
            for (uint32_t d = fill + jj; d < nf; d += jt) {
                uint64_t lo = want.p0, hi = want.p1;
                while (lo < hi) {
                    const uint64_t mid = (lo + hi) >> 1;
                    if (want.loc[mid] < d) lo = mid + 1;
                    else hi = mid;
                }
                if (lo >= want.p1 || want.loc[lo] != d) continue;
                const uint64_t j = sc[d];
                for (uint64_t byte = sl; byte < pitch; byte += nsl) {
                    uint32_t code = 0;
                    if (byte < nb && B == 1)
                        code = b1_code(bw, n, byte);
                    else if (byte < nb)
                        for (uint32_t k = 0; k < 4; k++) {
                            const uint64_t i = byte * 4 + k;
                            if (i < n) {
                                const uint32_t v = round_value(bw, n, B, i, j);
                                code |= (v == 3 ? 1u : v == 0 ? 0u : v + 1u) << (2 * k);
                            }
                        }
                    for (uint64_t p = lo; p < want.p1 && want.loc[p] == d; p++)
                        out[want.outc[p] * pitch + byte] = (uint8_t)code;
                }
            }
            fill = nf;
            rounds++;
            __syncthreads();  // the next round overwrites the bits, thresholds and sums read above
        }
        all_rounds += rounds;
        all_failed += fill < B ? 1u : 0u;
    }
    if (l == 0) {
        atomicAdd(&totals[0], (unsigned long long)all_rounds);
        if (all_failed) atomicAdd(&totals[1], (unsigned long long)all_failed);
    }
}

thread_local uint64_t g_batch_rounds = 0;  // generator rounds (summed over the batches) of the last call

uint64_t threshold_of(double p) { return (uint64_t)std::ceil(std::ldexp(p, 53)); }

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

void snpgen_bed(uint8_t* packed, uint64_t pitch, uint64_t n, uint64_t seed, uint64_t B, const uint64_t* sid_idx,
                uint64_t n_sel, const double* maf_x, const double* maf_cdf, int n_pts, uint64_t scratch_bytes) {
    const uint64_t nb = ceil_div(n, 4);
    SNPMI_REQUIRE(n >= 1 && n < (1ull << 31), SNPMI_E_ARG, "SnpGen needs 1 <= iid_count < 2**31");
    SNPMI_REQUIRE(B >= 1 && B < (1ull << 31), SNPMI_E_ARG, "SnpGen needs 1 <= block_size < 2**31");
    SNPMI_REQUIRE(n * B < (1ull << 58), SNPMI_E_ARG, "SnpGen batch too large");
    SNPMI_REQUIRE(pitch >= nb, SNPMI_E_ARG, "pitch is smaller than a column");
    SNPMI_REQUIRE(n_pts > 0 && n_pts <= 1024 && maf_x && maf_cdf, SNPMI_E_ARG, "bad MAF table");
    g_batch_rounds = 0;
    if (n_sel == 0) return;
    SNPMI_REQUIRE(packed != nullptr && sid_idx != nullptr, SNPMI_E_ARG, "NULL argument");
    // every batch touched, once: the requested columns sorted by (batch, column of the batch)
    std::vector<Want> want(n_sel);
    for (uint64_t k = 0; k < n_sel; k++) want[k] = {sid_idx[k] / B, (uint32_t)(sid_idx[k] % B), k};
    std::sort(want.begin(), want.end(), [](const Want& a, const Want& b) {
        return a.batch != b.batch ? a.batch < b.batch : a.loc != b.loc ? a.loc < b.loc : a.outc < b.outc;
    });
    // all seeds are checked before any launch
    SNPMI_REQUIRE(seed <= 0xffffffffull && want.back().batch <= (0xffffffffull - seed) / B, SNPMI_E_ARG,
                  "Seed must be between 0 and 2**32 - 1");
    std::vector<uint64_t> thr_tab(n_pts);
    for (int k = 0; k < n_pts; k++) {
        SNPMI_REQUIRE(maf_x[k] >= 0.0 && maf_x[k] <= 1.0, SNPMI_E_ARG, "MAF outside [0, 1]");
        thr_tab[k] = threshold_of(maf_x[k]);
    }

    Device& d = device();
    hipStream_t st = d.stream;
    auto al = [](uint64_t x) { return round_up(x, 256); };
    // scratch slots: one per workgroup; more than the device holds at once (8 per CU) buy nothing
    const uint64_t W = ceil_div(3 * n * B, 64) + 1;
    const uint64_t per_slot = al(W * 8) + al(B * 8) + 2 * al(B * 4);
    const uint64_t budget = scratch_bytes ? scratch_bytes : kDefaultScratch;
    const uint64_t max_slots = std::max<uint64_t>(1, std::min<uint64_t>(budget / per_slot,
                                                                        8 * (uint64_t)std::max(d.cu_count, 1)));
    DevBuf scratch, tables;
    SNPMI_HIP(hipMalloc((void**)&scratch.p, max_slots * per_slot));
    // slots index their arrays by slot * B (or * W): the aligned sizes above only bound the total
    uint64_t* bits = (uint64_t*)scratch.p;
    uint64_t* thr = (uint64_t*)(scratch.p + max_slots * al(W * 8));
    uint32_t* csum = (uint32_t*)(scratch.p + max_slots * (al(W * 8) + al(B * 8)));
    uint32_t* src = (uint32_t*)(scratch.p + max_slots * (al(W * 8) + al(B * 8) + al(B * 4)));

    // index tables of one launch: at most kGroupPairs requested columns (or one batch's)
    const uint64_t cap_pairs = std::min<uint64_t>(n_sel, kGroupPairs);
    std::vector<uint32_t> h_seeds, h_loc;
    std::vector<uint64_t> h_off, h_outc;
    uint64_t tab_bytes = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t o = tab_bytes;
        tab_bytes += al(bytes);
        return o;
    };
    // sized for the largest launch: pairs <= max(cap_pairs, largest batch's), batches <= pairs
    uint64_t largest = 0;
    for (uint64_t i = 0, j; i < n_sel; i = j) {
        for (j = i; j < n_sel && want[j].batch == want[i].batch; j++) {}
        largest = std::max(largest, j - i);
    }
    const uint64_t max_pairs = std::max(cap_pairs, largest);
    const uint64_t o_seeds = take(max_pairs * 4), o_off = take((max_pairs + 1) * 8), o_loc = take(max_pairs * 4),
                   o_outc = take(max_pairs * 8), o_tot = take(2 * 8), o_cdf = take((uint64_t)n_pts * 8),
                   o_tab = take((uint64_t)n_pts * 8);
    SNPMI_HIP(hipMalloc((void**)&tables.p, tab_bytes));
    uint32_t* seeds_d = (uint32_t*)(tables.p + o_seeds);
    uint64_t* off_d = (uint64_t*)(tables.p + o_off);
    uint32_t* loc_d = (uint32_t*)(tables.p + o_loc);
    uint64_t* outc_d = (uint64_t*)(tables.p + o_outc);
    unsigned long long* totals = (unsigned long long*)(tables.p + o_tot);
    double* cdf_d = (double*)(tables.p + o_cdf);
    uint64_t* tab_d = (uint64_t*)(tables.p + o_tab);
    SNPMI_HIP(hipMemcpyAsync(cdf_d, maf_cdf, (size_t)n_pts * 8, hipMemcpyHostToDevice, st));
    SNPMI_HIP(hipMemcpyAsync(tab_d, thr_tab.data(), (size_t)n_pts * 8, hipMemcpyHostToDevice, st));
    const GenTables gt{cdf_d, tab_d, n_pts, threshold_of(0.218)};
    uint32_t jt = 1;
    while (jt < 64 && jt < B) jt *= 2;

    uint64_t failed = 0;
    for (uint64_t i0 = 0; i0 < n_sel;) {
        // this launch's batches: whole batches while the pairs fit (at least one batch)
        h_seeds.clear();
        h_off.clear();
        h_loc.clear();
        h_outc.clear();
        uint64_t i = i0;
        while (i < n_sel) {
            uint64_t j = i;
            while (j < n_sel && want[j].batch == want[i].batch) j++;
            if (!h_seeds.empty() && (j - i0) > cap_pairs) break;
            h_seeds.push_back((uint32_t)(seed + want[i].batch * B));
            h_off.push_back(i - i0);
            for (uint64_t k = i; k < j; k++) {
                h_loc.push_back(want[k].loc);
                h_outc.push_back(want[k].outc);
            }
            i = j;
        }
        h_off.push_back(i - i0);
        const uint64_t nbat = h_seeds.size(), npairs = i - i0;
        SNPMI_HIP(hipMemcpyAsync(seeds_d, h_seeds.data(), nbat * 4, hipMemcpyHostToDevice, st));
        SNPMI_HIP(hipMemcpyAsync(off_d, h_off.data(), (nbat + 1) * 8, hipMemcpyHostToDevice, st));
        SNPMI_HIP(hipMemcpyAsync(loc_d, h_loc.data(), npairs * 4, hipMemcpyHostToDevice, st));
        SNPMI_HIP(hipMemcpyAsync(outc_d, h_outc.data(), npairs * 8, hipMemcpyHostToDevice, st));
        SNPMI_HIP(hipMemsetAsync(totals, 0, 2 * 8, st));
        const uint32_t grid = (uint32_t)std::min<uint64_t>(nbat, max_slots);
        k_snpgen<<<grid, kGenBlock, 0, st>>>((uint32_t)nbat, seeds_d, off_d, loc_d, outc_d, n, (uint32_t)B, jt, gt, thr,
                                             bits, W, csum, src, packed, pitch, totals);
        SNPMI_HIP(hipGetLastError());
        unsigned long long h_tot[2] = {0, 0};  // rounds run, batches left unfilled
        SNPMI_HIP(hipMemcpyAsync(h_tot, totals, 2 * 8, hipMemcpyDeviceToHost, st));
        SNPMI_HIP(hipStreamSynchronize(st));  // the host lists are refilled for the next launch
        g_batch_rounds += h_tot[0];
        failed += h_tot[1];
        i0 = i;
    }
    SNPMI_REQUIRE(failed == 0, SNPMI_E_ARG, "SnpGen: a batch did not fill within 4096 rounds (MAF table without legal SNPs)");
}

}  // namespace
}  // namespace snpmi

using namespace snpmi;

extern "C" {

int snpmi_dev_snpgen_bed(uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t seed, uint64_t block_size,
                         const uint64_t* sid_idx, uint64_t n_sel, const double* maf_x, const double* maf_cdf, int n_pts,
                         uint64_t scratch_bytes) {
    return guarded([&] {
        snpgen_bed(packed, pitch, n_iid, seed, block_size, sid_idx, n_sel, maf_x, maf_cdf, n_pts, scratch_bytes);
    });
}

int snpmi_dev_snpgen_rounds(uint64_t* batch_rounds) {
    return guarded([&] {
        SNPMI_REQUIRE(batch_rounds != nullptr, SNPMI_E_ARG, "batch_rounds is NULL");
        *batch_rounds = g_batch_rounds;
    });
}

int snpmi_dev_mt19937_random_sample(uint32_t seed32, uint64_t count, double* out_dev) {
    return guarded([&] {
        if (count == 0) return;
        SNPMI_REQUIRE(out_dev != nullptr, SNPMI_E_ARG, "out is NULL");
        Device& d = device();
        k_mt_sample<<<1, kGenBlock, 0, d.stream>>>(seed32, count, out_dev);
        SNPMI_HIP(hipGetLastError());
        SNPMI_HIP(hipStreamSynchronize(d.stream));
    });
}

}  // extern "C"
