// BGEN (reference distreader/bgen.py, which wraps the cbgen C library): the host-side walk of a
// file's variant index, and the decode of inflated layout-2 genotype blocks into distributions.
//
// Host (no device work), snpmi_bgen_open / snpmi_bgen_index: the file is mmapped and walked once per
// call, variant by variant, stepping over every genotype block.  A layout-2 file is
//
//   u32 offset | header: u32 LH, u32 M, u32 N, 4 B magic, LH - 20 B free, u32 flags
//              | sample block (flags bit 31): u32 LSI, u32 N, N x (u16 len, bytes)
//   at offset + 4, M variants: u16 len, id | u16 len, rsid | u16 len, chrom | u32 position | u16 K |
//              K x (u32 len, allele) | u32 C | [u32 D when compressed] | stored bytes
//
// flags bits 0-1: 0 = stored as is (C bytes, D = C), 1 = zlib (C - 4 bytes inflate to D), 2 = zstd;
// bits 2-5: the layout.  open counts (variants, samples, widest strings), index fills arrays the
// caller allocated from those counts: strings as fixed-width NUL-padded rows (NumPy 'S<width>').
// Inflating the blocks is the caller's (Python's zlib): the library links no compression library.
//
// Device, snpmi_dev_bgen_decode_*: an inflated block of N diploid, unphased, biallelic samples is
//
//   u32 N | u16 K = 2 | u8 min ploidy = 2 | u8 max ploidy = 2 | N x u8 (bit 7: missing, low 6: ploidy)
//         | u8 phased = 0 | u8 B | N pairs of B-bit little-endian integers (a, b), bit-packed
//
// so 10 + N + ceil(2 B N / 8) bytes; the caller has checked all of that and placed every block on an
// 8-byte boundary of one buffer with 16 spare bytes behind the last.  Sample i of a block gives, with
// D = 2^B - 1,  p0 = a / D,  p1 = b / D,  p2 = (D - (a + b)) / D  in f64 (a + b < 2^33 and D - (a + b)
// are exact, so each value is one IEEE division: singly rounded), or three quiet NaNs when missing;
// a float32 output is that f64 value rounded once.
//
// The pair of sample i is the 2 B <= 64 bits at bit 8 (10 + N) + 2 B i of the block: any bit of any
// byte, up to 9 bytes wide.  It is cut from the two aligned 64-bit words around it (the second may
// lie behind the block: the spare bytes), never with an unaligned load.
//
//   k_bgen_f<VEC>   F order (three planes).  VEC: a lane decodes 16 B of consecutive rows of one
//                   column and stores 16 B to each plane -- when the output base is 16-B aligned and
//                   rows is a multiple of 16 B, so that every column of every plane starts aligned;
//                   else one row per lane, 4- or 8-byte stores, consecutive lanes consecutive rows.
//   k_bgen_c        C order (triples along each row of SNPs) through a padded LDS tile of 64 rows x
//                   32 columns x 3: decoded with the lanes along the block's samples, stored with
//                   the lanes along a row's 96 consecutive values.  Every tile edge is masked.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

#include "snpmi_internal.hpp"

namespace snpmi {
namespace {

// ------------------------------------------------------------------ host: the index walk
struct FileMap {
    int fd = -1;
    const uint8_t* p = nullptr;
    size_t size = 0;
    ~FileMap() {
        if (p && size) munmap((void*)p, size);
        if (fd >= 0) close(fd);
    }
};

void open_map(FileMap& f, const char* path) {
    SNPMI_REQUIRE(path != nullptr, SNPMI_E_ARG, "path is NULL");
    f.fd = open(path, O_RDONLY);
    SNPMI_REQUIRE(f.fd >= 0, SNPMI_E_IO, std::string("cannot open ") + path);
    struct stat st;
    SNPMI_REQUIRE(fstat(f.fd, &st) == 0, SNPMI_E_IO, std::string("cannot stat ") + path);
    f.size = (size_t)st.st_size;
    if (f.size == 0) return;
    void* m = mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, f.fd, 0);
    SNPMI_REQUIRE(m != MAP_FAILED, SNPMI_E_IO, std::string("mmap failed: ") + path);
    f.p = (const uint8_t*)m;
    (void)madvise(m, f.size, MADV_RANDOM);  // the walk touches a few bytes per variant
}

// a cursor that refuses to leave the file
struct Cursor {
    const FileMap& f;
    const char* path;
    uint64_t at;
    std::string what;  // what is being read, for the message
    void need(uint64_t bytes) const {
        if (bytes > f.size || at > f.size - bytes)
            throw Error(SNPMI_E_FORMAT, std::string("BGEN file is truncated: ") + what + " at offset " +
                                            std::to_string(at) + " needs " + std::to_string(bytes) +
                                            " bytes, the file has " + std::to_string(f.size) + " (" + path + ")");
    }
    uint32_t u16() {
        need(2);
        const uint32_t v = (uint32_t)f.p[at] | (uint32_t)f.p[at + 1] << 8;
        at += 2;
        return v;
    }
    uint32_t u32() {
        need(4);
        const uint32_t v = (uint32_t)f.p[at] | (uint32_t)f.p[at + 1] << 8 | (uint32_t)f.p[at + 2] << 16 |
                           (uint32_t)f.p[at + 3] << 24;
        at += 4;
        return v;
    }
    const uint8_t* bytes(uint64_t n) {
        need(n);
        const uint8_t* r = f.p + at;
        at += n;
        return r;
    }
};

struct Header {
    uint64_t first, m, n, flags, sample_at;  // sample_at: offset of the sample block's N, 0 = none
};

Header read_header(Cursor& c) {
    c.what = "the header";
    c.at = 0;
    Header h{};
    const uint64_t offset = c.u32(), lh = c.u32();
    h.m = c.u32();
    h.n = c.u32();
    const uint8_t* magic = c.bytes(4);
    const bool named = magic[0] == 'b' && magic[1] == 'g' && magic[2] == 'e' && magic[3] == 'n';
    const bool zeros = !magic[0] && !magic[1] && !magic[2] && !magic[3];
    SNPMI_REQUIRE(named || zeros, SNPMI_E_FORMAT, std::string("not a BGEN file (magic number): ") + c.path);
    SNPMI_REQUIRE(lh >= 20 && lh <= offset, SNPMI_E_FORMAT, std::string("BGEN header length is inconsistent: ") + c.path);
    c.bytes(lh - 20);
    h.flags = c.u32();
    h.first = offset + 4;
    const uint64_t comp = h.flags & 3, layout = (h.flags >> 2) & 15;
    SNPMI_REQUIRE(layout == 2, SNPMI_E_FORMAT,
                  "BGEN layout " + std::to_string(layout) + " is not supported (layout 2 only): " + c.path);
    SNPMI_REQUIRE(comp <= 1, SNPMI_E_FORMAT,
                  comp == 2 ? std::string("BGEN zstd compression is not supported (none or zlib only): ") + c.path
                            : std::string("BGEN compression flag 3 is undefined: ") + c.path);
    if (h.flags >> 31) {
        c.what = "the sample identifier block";
        c.u32();  // its length
        h.sample_at = c.at;
        const uint64_t ns = c.u32();
        SNPMI_REQUIRE(ns == h.n, SNPMI_E_FORMAT,
                      "BGEN sample block lists " + std::to_string(ns) + " samples, the header " + std::to_string(h.n) +
                          ": " + c.path);
    }
    return h;
}

void put(char* dst, uint64_t row, uint64_t width, const uint8_t* s, uint64_t len) {
    char* d = dst + row * width;
    len = std::min(len, width);
    std::memcpy(d, s, len);
    if (len < width) std::memset(d + len, 0, width - len);
}

// widths: sample, id, rsid, chrom, alleles (the K alleles joined with commas); any array may be NULL
struct IndexOut {
    uint64_t* rec = nullptr;  // [M][5]: data offset, stored bytes, inflated bytes, position, K
    char* str[5] = {};
    uint64_t w[5] = {};
};

// One pass over one mapping: fills `o` (when given) and the widest strings `wmax`.  `expect` (with
// `o`): the {variants, samples} the caller sized o's arrays for; a header that says otherwise is
// refused before anything is written.
Header walk(const char* path, const IndexOut* o, uint64_t* wmax, uint64_t* file_size, const uint64_t* expect = nullptr) {
    FileMap f;
    open_map(f, path);
    Cursor c{f, path, 0, ""};
    const Header h = read_header(c);
    SNPMI_REQUIRE(o == nullptr || (expect != nullptr && h.m == expect[0] && h.n == expect[1]), SNPMI_E_FORMAT,
                  std::string("BGEN counts changed while reading ") + path);
    if (file_size) *file_size = f.size;
    if (h.sample_at) {
        c.at = h.sample_at + 4;
        c.what = "the sample identifier block";
        for (uint64_t i = 0; i < h.n; i++) {
            const uint64_t len = c.u16();
            const uint8_t* s = c.bytes(len);
            wmax[0] = std::max(wmax[0], len);
            if (o && o->str[0]) put(o->str[0], i, o->w[0], s, len);
        }
    }
    SNPMI_REQUIRE(c.at <= h.first, SNPMI_E_FORMAT, std::string("BGEN header and sample block overrun the offset: ") + path);
    c.at = h.first;
    const bool compressed = (h.flags & 3) != 0;
    std::string alleles;
    for (uint64_t v = 0; v < h.m; v++) {
        c.what = "variant " + std::to_string(v);
        for (int k = 1; k <= 3; k++) {  // id, rsid, chrom
            const uint64_t len = c.u16();
            const uint8_t* s = c.bytes(len);
            wmax[k] = std::max(wmax[k], len);
            if (o && o->str[k]) put(o->str[k], v, o->w[k], s, len);
        }
        const uint64_t pos = c.u32(), K = c.u16();
        alleles.clear();
        for (uint64_t a = 0; a < K; a++) {
            const uint64_t len = c.u32();
            const uint8_t* s = c.bytes(len);
            if (a) alleles.push_back(',');
            alleles.append((const char*)s, len);
        }
        wmax[4] = std::max<uint64_t>(wmax[4], alleles.size());
        if (o && o->str[4]) put(o->str[4], v, o->w[4], (const uint8_t*)alleles.data(), alleles.size());
        c.what = "the genotype block of variant " + std::to_string(v);
        uint64_t stored = c.u32(), inflated = stored;
        if (compressed) {
            SNPMI_REQUIRE(stored >= 4, SNPMI_E_FORMAT, "BGEN " + c.what + " is shorter than its length field: " + path);
            inflated = c.u32();
            stored -= 4;
        }
        if (o && o->rec) {
            uint64_t* r = o->rec + v * 5;
            r[0] = c.at, r[1] = stored, r[2] = inflated, r[3] = pos, r[4] = K;
        }
        c.bytes(stored);
    }
    return h;
}

// ------------------------------------------------------------------ device: the decode
constexpr int kBlock = 256;
constexpr int kTileRows = 64, kTileCols = 32;

struct BgenCol {
    uint64_t off;  // of the block in the staged buffer (a multiple of 8)
    uint32_t bits, n;
};

template <typename T>
__device__ __forceinline__ T bgen_nan();
template <>
__device__ __forceinline__ double bgen_nan<double>() {
    return __longlong_as_double(0x7ff8000000000000ll);
}
template <>
__device__ __forceinline__ float bgen_nan<float>() {
    return __uint_as_float(0x7fc00000u);
}

// the three values of sample i of the block at blk (8-byte aligned)
template <typename T>
__device__ __forceinline__ void bgen_triple(const uint8_t* __restrict__ blk, uint32_t bits, uint32_t n, uint64_t i,
                                            T& p0, T& p1, T& p2) {
    if (blk[8 + i] & 0x80) {
        p0 = p1 = p2 = bgen_nan<T>();
        return;
    }
    const uint64_t bit = 8ull * (10ull + n) + 2ull * bits * i;
    const uint64_t* w = reinterpret_cast<const uint64_t*>(blk) + (bit >> 6);
    const uint32_t sh = (uint32_t)(bit & 63);
    const uint64_t lo = w[0], hi = w[1];
    const uint64_t pair = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    const uint64_t mask = (1ull << bits) - 1;  // bits <= 32
    const uint64_t a = pair & mask, b = (pair >> bits) & mask;
    const double D = (double)mask;
    p0 = (T)((double)a / D);
    p1 = (T)((double)b / D);
    p2 = (T)((D - (double)(a + b)) / D);
}

// F order: element (r, s, k) at out[r + ld_s * s + ld_k * k]; idx (may be NULL): row r is sample idx[r]
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_bgen_f(const uint8_t* __restrict__ blocks, const BgenCol* __restrict__ tab,
                                                   const uint64_t* __restrict__ idx, uint64_t rows, uint64_t cols,
                                                   T* __restrict__ out, uint64_t ld_s, uint64_t ld_k) {
    constexpr uint64_t V = VEC ? 16 / sizeof(T) : 1;
    using Vec = T __attribute__((ext_vector_type(16 / sizeof(T))));
    const uint64_t groups = rows / V;  // VEC: rows % V == 0
    for (uint64_t s = blockIdx.y; s < cols; s += gridDim.y) {
        const BgenCol c = tab[s];
        const uint8_t* blk = blocks + c.off;
        T* o = out + s * ld_s;
        for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * kBlock) {
            const uint64_t r = g * V;
            if constexpr (VEC) {
                Vec v0, v1, v2;
#pragma unroll
                for (uint64_t e = 0; e < V; e++) {
                    T a, b, d;
                    bgen_triple<T>(blk, c.bits, c.n, idx ? idx[r + e] : r + e, a, b, d);
                    v0[e] = a, v1[e] = b, v2[e] = d;
                }
                *reinterpret_cast<Vec*>(o + r) = v0;
                *reinterpret_cast<Vec*>(o + ld_k + r) = v1;
                *reinterpret_cast<Vec*>(o + 2 * ld_k + r) = v2;
            } else {
                T a, b, d;
                bgen_triple<T>(blk, c.bits, c.n, idx ? idx[r] : r, a, b, d);
                o[r] = a, o[ld_k + r] = b, o[2 * ld_k + r] = d;
            }
        }
    }
}

// C order: element (r, s, k) at out[r * ld_r + 3 * s + k]
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bgen_c(const uint8_t* __restrict__ blocks, const BgenCol* __restrict__ tab,
                                                   const uint64_t* __restrict__ idx, uint64_t rows, uint64_t cols,
                                                   T* __restrict__ out, uint64_t ld_r) {
    constexpr int W = 3 * kTileCols;
    __shared__ T tile[kTileRows][W + 1];
    const uint64_t tr = (rows + kTileRows - 1) / kTileRows, tc = (cols + kTileCols - 1) / kTileCols;
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    for (uint64_t b = blockIdx.x; b < tr * tc; b += gridDim.x) {
        const uint64_t r0 = (b % tr) * kTileRows, s0 = (b / tr) * kTileCols;
        const uint64_t r = r0 + x;
        const uint64_t i = r < rows ? (idx ? idx[r] : r) : 0;
        for (int q = y; q < kTileCols; q += kBlock / 64) {
            const uint64_t s = s0 + q;
            if (r < rows && s < cols) {
                const BgenCol c = tab[s];
                T p0, p1, p2;
                bgen_triple<T>(blocks + c.off, c.bits, c.n, i, p0, p1, p2);
                tile[x][3 * q] = p0, tile[x][3 * q + 1] = p1, tile[x][3 * q + 2] = p2;
            }
        }
        __syncthreads();
        const uint64_t width = 3 * min((uint64_t)kTileCols, cols - s0), height = min((uint64_t)kTileRows, rows - r0);
        for (uint32_t e = threadIdx.x; e < kTileRows * W; e += kBlock) {
            const uint32_t tr_ = e / W, tw = e - tr_ * W;
            if (tr_ < height && tw < width) out[(r0 + tr_) * ld_r + 3 * s0 + tw] = tile[tr_][tw];
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

constexpr uint64_t kMaxBlocks = 256 * 8 * 4;  // ~8 blocks of 256 threads per CU, the rest by grid stride

template <typename T>
void bgen_decode(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* table, uint64_t cols,
                 const uint64_t* iid_idx, uint64_t rows, T* out, uint64_t cols_total, uint64_t col0, int out_c) {
    std::lock_guard<std::recursive_mutex> lk(call_mutex());
    SNPMI_REQUIRE(rows < (1ull << 40) && cols_total < (1ull << 40), SNPMI_E_ARG, "BGEN output too large");
    SNPMI_REQUIRE(col0 <= cols_total && cols <= cols_total - col0, SNPMI_E_INDEX, "SNP range outside the output array");
    if (rows == 0 || cols == 0) return;
    SNPMI_REQUIRE(blocks != nullptr && table != nullptr && out != nullptr, SNPMI_E_ARG, "NULL argument");
    Device& d = device();
    SNPMI_REQUIRE(is_device_ptr(d, blocks) && is_device_ptr(d, out), SNPMI_E_ARG, "blocks and out must be device memory");
    SNPMI_REQUIRE(reinterpret_cast<uintptr_t>(blocks) % 8 == 0, SNPMI_E_ARG, "blocks must be 8-byte aligned");
    hipStream_t st = d.stream;
    // every read of the kernel is inside [blocks, blocks + blocks_bytes): a block's two-word windows
    // end less than 16 bytes behind it
    std::vector<BgenCol> tab(cols);
    uint64_t n_min = ~0ull;
    for (uint64_t s = 0; s < cols; s++) {
        const uint64_t off = table[3 * s], bits = table[3 * s + 1], n = table[3 * s + 2];
        SNPMI_REQUIRE(bits >= 1 && bits <= 32, SNPMI_E_ARG, "BGEN bit depth must be 1 ... 32");
        SNPMI_REQUIRE(n < (1ull << 32), SNPMI_E_ARG, "BGEN block has too many samples");
        const uint64_t len = 10 + n + (2 * bits * n + 7) / 8;
        SNPMI_REQUIRE(off % 8 == 0 && off <= blocks_bytes && len + 16 <= blocks_bytes - off, SNPMI_E_INDEX,
                      "BGEN block (with its 16 spare bytes) outside the staged buffer");
        tab[s] = {off, (uint32_t)bits, (uint32_t)n};
        n_min = std::min(n_min, n);
    }
    // the gather index: a host or a device array; checked on the host either way
    std::vector<uint64_t> idx_host;
    const uint64_t* idx_dev = nullptr;
    DevBuf scratch;
    const uint64_t tab_bytes = round_up(cols * sizeof(BgenCol), 256);
    SNPMI_HIP(hipMalloc((void**)&scratch.p, tab_bytes + (iid_idx ? rows * 8 : 0)));
    if (iid_idx) {
        const uint64_t* h = iid_idx;
        if (is_device_ptr(d, iid_idx)) {
            idx_host.resize(rows);
            SNPMI_HIP(hipMemcpy(idx_host.data(), iid_idx, rows * 8, hipMemcpyDeviceToHost));
            h = idx_host.data();
        }
        for (uint64_t r = 0; r < rows; r++)
            SNPMI_REQUIRE(h[r] < n_min, SNPMI_E_INDEX, "iid index outside the BGEN block's samples");
        SNPMI_HIP(hipMemcpy(scratch.p + tab_bytes, h, rows * 8, hipMemcpyHostToDevice));
        idx_dev = (const uint64_t*)(scratch.p + tab_bytes);
    } else {
        SNPMI_REQUIRE(rows <= n_min, SNPMI_E_INDEX, "more rows than the BGEN block has samples");
    }
    // (synchronous copies: the host tables are free to go as soon as this call returns or throws)
    SNPMI_HIP(hipMemcpy(scratch.p, tab.data(), cols * sizeof(BgenCol), hipMemcpyHostToDevice));
    const BgenCol* tab_dev = (const BgenCol*)scratch.p;
    if (out_c) {
        const uint64_t tiles = ceil_div(rows, kTileRows) * ceil_div(cols, kTileCols);
        k_bgen_c<T><<<(unsigned)std::min(tiles, kMaxBlocks), kBlock, 0, st>>>(blocks, tab_dev, idx_dev, rows, cols,
                                                                             out + 3 * col0, 3 * cols_total);
    } else {
        constexpr uint64_t V = 16 / sizeof(T);
        T* o = out + col0 * rows;
        const bool vec = rows % V == 0 && reinterpret_cast<uintptr_t>(o) % 16 == 0;
        const unsigned gy = (unsigned)std::min<uint64_t>(cols, 65535);
        const uint64_t groups = vec ? rows / V : rows;
        const dim3 g((unsigned)std::min<uint64_t>(ceil_div(groups, kBlock), std::max<uint64_t>(1, kMaxBlocks / gy)), gy);
        if (vec) k_bgen_f<T, true><<<g, kBlock, 0, st>>>(blocks, tab_dev, idx_dev, rows, cols, o, rows, rows * cols_total);
        else k_bgen_f<T, false><<<g, kBlock, 0, st>>>(blocks, tab_dev, idx_dev, rows, cols, o, rows, rows * cols_total);
    }
    SNPMI_HIP(hipGetLastError());
    SNPMI_HIP(hipStreamSynchronize(st));  // the tables are freed on return
}

}  // namespace
}  // namespace snpmi

using namespace snpmi;

extern "C" {

int snpmi_bgen_open(const char* path, uint64_t* info) {
    return guarded([&] {
        SNPMI_REQUIRE(info != nullptr, SNPMI_E_ARG, "info is NULL");
        uint64_t w[5] = {}, size = 0;
        const Header h = walk(path, nullptr, w, &size);
        info[0] = h.m, info[1] = h.n, info[2] = h.flags, info[3] = h.first, info[4] = h.sample_at ? 1 : 0;
        for (int k = 0; k < 5; k++) info[5 + k] = w[k];
        info[10] = size;
    });
}

int snpmi_bgen_index(const char* path, uint64_t n_variants, uint64_t n_samples, uint64_t* rec, char* samples,
                     uint64_t w_sample, char* ids, uint64_t w_id, char* rsids, uint64_t w_rsid, char* chroms,
                     uint64_t w_chrom, char* alleles, uint64_t w_alleles) {
    return guarded([&] {
        IndexOut o;
        o.rec = rec;
        char* const str[5] = {samples, ids, rsids, chroms, alleles};
        const uint64_t w[5] = {w_sample, w_id, w_rsid, w_chrom, w_alleles};
        for (int k = 0; k < 5; k++) o.str[k] = w[k] ? str[k] : nullptr, o.w[k] = w[k];
        // the arrays were sized from snpmi_bgen_open's counts: the walk refuses a header that says otherwise
        const uint64_t expect[2] = {n_variants, n_samples};
        uint64_t wmax[5] = {};
        walk(path, &o, wmax, nullptr, expect);
    });
}

int snpmi_dev_bgen_decode_f32(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* col_table, uint64_t cols,
                              const uint64_t* iid_idx, uint64_t rows, float* out, uint64_t cols_total, uint64_t col0,
                              int out_order_c) {
    return guarded([&] { bgen_decode(blocks, blocks_bytes, col_table, cols, iid_idx, rows, out, cols_total, col0, out_order_c); });
}
int snpmi_dev_bgen_decode_f64(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* col_table, uint64_t cols,
                              const uint64_t* iid_idx, uint64_t rows, double* out, uint64_t cols_total, uint64_t col0,
                              int out_order_c) {
    return guarded([&] { bgen_decode(blocks, blocks_bytes, col_table, cols, iid_idx, rows, out, cols_total, col0, out_order_c); });
}

}  // extern "C"
