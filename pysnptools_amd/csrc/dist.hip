// Genotype distributions <-> SNP values (gfx950): the conversions of the reference's
// snpreader/_dist2snp.py:47-52 and distreader/_snp2dist.py:41-54, and the GRM route of a
// distribution array (snpmi_grm_add_dist_*).
//
//   k_d2s_vec_f / k_d2s_vec_c   dist -> dosage, same order in and out: 16-B loads and stores, a scalar
//                               head and tail per column / row (12 or 24 B read, 4 or 8 B written per value)
//   k_d2s_scalar                the same when base or stride are not 16-B aligned with each other
//   k_d2s_tile                  F -> C and C -> F through a padded 64 x 64 LDS tile, masked at every edge
//   k_s2d_f / k_s2d_c           value -> one-hot triple (NaN triple when the value is no genotype)
//
// A distribution array is [rows][cols_total][3]: in F order three planes of rows x cols_total, in C
// order triples along each row.  Both are read through one strided view (DistSrc), which also
// describes the staged slabs of a host array.
#include <algorithm>

#include "snpmi_internal.hpp"

namespace snpmi {
namespace {

constexpr int kBlock = 256;

// element (i, s, k) of the SNP range at p[i * si + s * sj + k * sk]
template <typename T>
struct DistSrc {
    const T* p;
    uint64_t si, sj, sk;
};

// weights = array([0, .5, 1], T) * max_weight (_dist2snp.py:47)
template <typename T>
struct Weights {
    T w0, w1, w2;
};

// (val * weights).sum(axis=-1) as NumPy adds the three terms: ((0 + p0 w0) + p1 w1) + p2 w2.  The sum
// starts from +0 (three products of -0 sum to +0, as NumPy's do), every product is kept (a NaN or
// infinite p0 reaches the sum) and nothing is contracted (-ffp-contract=off).
template <typename T>
__device__ __forceinline__ T dosage(T p0, T p1, T p2, const Weights<T>& w) {
    return (((T)0 + p0 * w.w0) + p1 * w.w1) + p2 * w.w2;
}

template <typename T>
using Vec16 = T __attribute__((ext_vector_type(16 / sizeof(T))));

// F -> F.  Column s of plane k starts at p + s * sj + k * sk and the output column at out + s * ldo;
// the host has checked that, `head` elements into every column, all four are 16-B aligned.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_d2s_vec_f(DistSrc<T> src, uint64_t rows, uint64_t cols, Weights<T> w,
                                                      T* __restrict__ out, uint64_t ldo, uint32_t head) {
    constexpr uint64_t V = 16 / sizeof(T);
    using Vec = Vec16<T>;
    const uint64_t nv = (rows - head) / V, tail0 = head + nv * V;
    for (uint64_t s = blockIdx.y; s < cols; s += gridDim.y) {
        const T* c0 = src.p + s * src.sj;
        const T* c1 = c0 + src.sk;
        const T* c2 = c1 + src.sk;
        T* o = out + s * ldo;
        for (uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x; v < nv; v += (uint64_t)gridDim.x * kBlock) {
            const uint64_t i = head + v * V;
            const Vec a = *reinterpret_cast<const Vec*>(c0 + i);
            const Vec b = *reinterpret_cast<const Vec*>(c1 + i);
            const Vec c = *reinterpret_cast<const Vec*>(c2 + i);
            Vec r;
#pragma unroll
            for (uint64_t e = 0; e < V; e++) r[e] = dosage(a[e], b[e], c[e], w);
            *reinterpret_cast<Vec*>(o + i) = r;
        }
        if (blockIdx.x == 0) {  // fewer than 2 V elements: [0, head) and [tail0, rows)
            const uint64_t t = threadIdx.x;
            const uint64_t i = t < head ? t : tail0 + (t - head);
            if (i < rows) o[i] = dosage(c0[i], c1[i], c2[i], w);
        }
    }
}

// C -> C.  Row i's triples start at p + i * si and the output row at out + i * ldo; `head` values
// (3 * head source elements) into every row both are 16-B aligned.  One thread: three loads of
// 16 B = V triples, one store of V values.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_d2s_vec_c(DistSrc<T> src, uint64_t rows, uint64_t cols, Weights<T> w,
                                                      T* __restrict__ out, uint64_t ldo, uint32_t head) {
    constexpr uint64_t V = 16 / sizeof(T);
    using Vec = Vec16<T>;
    const uint64_t nv = (cols - head) / V, tail0 = head + nv * V;
    for (uint64_t i = blockIdx.y; i < rows; i += gridDim.y) {
        const T* r = src.p + i * src.si;
        T* o = out + i * ldo;
        for (uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x; v < nv; v += (uint64_t)gridDim.x * kBlock) {
            const uint64_t s = head + v * V;
            const Vec* in = reinterpret_cast<const Vec*>(r + 3 * s);
            const Vec x[3] = {in[0], in[1], in[2]};
            T f[3 * V];
#pragma unroll
            for (uint64_t e = 0; e < 3 * V; e++) f[e] = x[e / V][e % V];
            Vec y;
#pragma unroll
            for (uint64_t e = 0; e < V; e++) y[e] = dosage(f[3 * e], f[3 * e + 1], f[3 * e + 2], w);
            *reinterpret_cast<Vec*>(o + s) = y;
        }
        if (blockIdx.x == 0) {
            const uint64_t t = threadIdx.x;
            const uint64_t s = t < head ? t : tail0 + (t - head);
            if (s < cols) o[s] = dosage(r[3 * s], r[3 * s + 1], r[3 * s + 2], w);
        }
    }
}

// Same order in and out, any alignment: lanes along the order's fast axis (rows in F, SNPs in C)
template <typename T, bool ORDER_C>
__global__ __launch_bounds__(kBlock) void k_d2s_scalar(DistSrc<T> src, uint64_t rows, uint64_t cols, Weights<T> w,
                                                       T* __restrict__ out, uint64_t oi, uint64_t oj) {
    const uint64_t fast = ORDER_C ? cols : rows, slow = ORDER_C ? rows : cols;
    for (uint64_t u = blockIdx.y; u < slow; u += gridDim.y)
        for (uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x; f < fast; f += (uint64_t)gridDim.x * kBlock) {
            const uint64_t i = ORDER_C ? u : f, s = ORDER_C ? f : u;
            const T* e = src.p + i * src.si + s * src.sj;
            out[i * oi + s * oj] = dosage(e[0], e[src.sk], e[2 * src.sk], w);
        }
}

// F -> C (SRC_C = false) and C -> F: the dosages of a 64 x 64 tile are computed with the lanes along
// the source's fast axis, cross a padded LDS tile, and are stored with the lanes along the
// output's.  Every tile edge is masked.
template <typename T, bool SRC_C>
__global__ __launch_bounds__(kBlock) void k_d2s_tile(DistSrc<T> src, uint64_t rows, uint64_t cols, Weights<T> w,
                                                     T* __restrict__ out, uint64_t oi, uint64_t oj) {
    __shared__ T tile[64][65];
    const uint64_t tr = (rows + 63) / 64, tc = (cols + 63) / 64;
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    for (uint64_t b = blockIdx.x; b < tr * tc; b += gridDim.x) {
        const uint64_t i0 = (b % tr) * 64, s0 = (b / tr) * 64;
        for (int q = y; q < 64; q += 4) {
            const uint64_t i = i0 + (SRC_C ? q : x), s = s0 + (SRC_C ? x : q);
            if (i < rows && s < cols) {
                const T* e = src.p + i * src.si + s * src.sj;
                tile[q][x] = dosage(e[0], e[src.sk], e[2 * src.sk], w);
            }
        }
        __syncthreads();
        for (int q = y; q < 64; q += 4) {
            const uint64_t i = i0 + (SRC_C ? x : q), s = s0 + (SRC_C ? q : x);
            if (i < rows && s < cols) out[i * oi + s * oj] = tile[x][q];
        }
        __syncthreads();
    }
}

// _snp2dist.py:41-54: slot c of the triple is 1 where val * factor == c, else 0; a value matching
// no c (NaN included) gives a NaN triple
template <typename T>
__device__ __forceinline__ void one_hot(T v, T factor, T& d0, T& d1, T& d2) {
    const T x = v * factor;
    const bool m0 = x == (T)0, m1 = x == (T)1, m2 = x == (T)2;
    const T miss = (T)__builtin_nan("");
    const bool any = m0 || m1 || m2;
    d0 = any ? (m0 ? (T)1 : (T)0) : miss;
    d1 = any ? (m1 ? (T)1 : (T)0) : miss;
    d2 = any ? (m2 ? (T)1 : (T)0) : miss;
}

// F order: element t of val -> out[t], out[t + count], out[t + 2 count].  VEC: 16-B accesses (the
// host has checked val, out and count for it); else scalar.
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_s2d_f(const T* __restrict__ val, uint64_t count, T factor,
                                                  T* __restrict__ out) {
    constexpr uint64_t V = VEC ? 16 / sizeof(T) : 1;
    for (uint64_t t = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * V; t < count;
         t += (uint64_t)gridDim.x * kBlock * V) {
        if constexpr (VEC) {
            using Vec = Vec16<T>;
            const Vec v = *reinterpret_cast<const Vec*>(val + t);
            Vec d0, d1, d2;
#pragma unroll
            for (uint64_t e = 0; e < V; e++) {
                T a, b, c;
                one_hot(v[e], factor, a, b, c);
                d0[e] = a, d1[e] = b, d2[e] = c;
            }
            *reinterpret_cast<Vec*>(out + t) = d0;
            *reinterpret_cast<Vec*>(out + count + t) = d1;
            *reinterpret_cast<Vec*>(out + 2 * count + t) = d2;
        } else {
            one_hot(val[t], factor, out[t], out[count + t], out[2 * count + t]);
        }
    }
}

// C order: element t of val -> out[3 t .. 3 t + 2].  VEC: V values in, three 16-B stores out, and a
// scalar tail of count % V values.
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_s2d_c(const T* __restrict__ val, uint64_t count, T factor,
                                                  T* __restrict__ out) {
    constexpr uint64_t V = VEC ? 16 / sizeof(T) : 1;
    const uint64_t body = count / V * V;
    for (uint64_t t = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * V; t < body;
         t += (uint64_t)gridDim.x * kBlock * V) {
        if constexpr (VEC) {
            using Vec = Vec16<T>;
            const Vec v = *reinterpret_cast<const Vec*>(val + t);
            T f[3 * V];
#pragma unroll
            for (uint64_t e = 0; e < V; e++) one_hot(v[e], factor, f[3 * e], f[3 * e + 1], f[3 * e + 2]);
            Vec* o = reinterpret_cast<Vec*>(out + 3 * t);
#pragma unroll
            for (uint64_t q = 0; q < 3; q++) {
                Vec y;
#pragma unroll
                for (uint64_t e = 0; e < V; e++) y[e] = f[q * V + e];
                o[q] = y;
            }
        } else {
            one_hot(val[t], factor, out[3 * t], out[3 * t + 1], out[3 * t + 2]);
        }
    }
    if (VEC && blockIdx.x == 0 && body + threadIdx.x < count) {
        const uint64_t t = body + threadIdx.x;
        one_hot(val[t], factor, out[3 * t], out[3 * t + 1], out[3 * t + 2]);
    }
}

inline unsigned grid_for(uint64_t work, uint64_t per_block, uint64_t cap) {
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(1, ceil_div(work, per_block)), std::max<uint64_t>(cap, 1));
}

// ~8 blocks of 256 threads per CU in flight, the rest of the work by grid stride
constexpr uint64_t kMaxBlocks = 256 * 8 * 4;

template <typename T>
inline uint64_t elem_mod16(const T* p) {
    return (reinterpret_cast<uintptr_t>(p) / sizeof(T)) % (16 / sizeof(T));
}

// Dosages of the rows x cols range `src` describes (order_c: its order) -> out[i * oi + s * oj]
// (out_c: lanes along s, i.e. oj == 1).
template <typename T>
void launch_dist_to_snp(DistSrc<T> src, int order_c, uint64_t rows, uint64_t cols, const Weights<T>& w, T* out,
                        uint64_t oi, uint64_t oj, int out_c, hipStream_t st) {
    if (rows == 0 || cols == 0) return;
    constexpr uint64_t V = 16 / sizeof(T);
    if ((order_c != 0) != (out_c != 0)) {
        const unsigned g = grid_for(ceil_div(rows, 64) * ceil_div(cols, 64), 1, kMaxBlocks);
        if (order_c) k_d2s_tile<T, true><<<g, kBlock, 0, st>>>(src, rows, cols, w, out, oi, oj);
        else k_d2s_tile<T, false><<<g, kBlock, 0, st>>>(src, rows, cols, w, out, oi, oj);
        SNPMI_HIP(hipGetLastError());
        return;
    }
    // same order: `fast` values per line, `slow` lines `lin` (source) and `lout` (output) apart
    uint64_t fast = order_c ? cols : rows, slow = order_c ? rows : cols;
    uint64_t lin = order_c ? src.si : src.sj, lout = order_c ? oi : oj;
    const uint64_t in_per_value = order_c ? 3 : 1;
    if (lin == fast * in_per_value && lout == fast) {  // the lines abut on both sides: one long line
        fast *= slow;
        slow = 1;
        if (order_c) rows = 1, cols = fast;
        else rows = fast, cols = 1;
    }
    // 16-B accesses when, `head` values into a line, the output and every source run are aligned,
    // and the line strides keep that so for every line
    const uint32_t head = (uint32_t)std::min<uint64_t>((V - elem_mod16(out)) % V, fast);
    bool vec = slow == 1 || (lin % V == 0 && lout % V == 0);
    if (order_c) vec = vec && (elem_mod16(src.p) + 3 * head) % V == 0;
    else
        for (int k = 0; k < 3; k++) vec = vec && (elem_mod16(src.p + k * src.sk) + head) % V == 0;
    const unsigned gy = (unsigned)std::min<uint64_t>(slow, 65535);
    if (vec) {
        const dim3 g(grid_for(fast / V, kBlock, std::max<uint64_t>(1, kMaxBlocks / gy)), gy);
        if (order_c) k_d2s_vec_c<T><<<g, kBlock, 0, st>>>(src, rows, cols, w, out, lout, head);
        else k_d2s_vec_f<T><<<g, kBlock, 0, st>>>(src, rows, cols, w, out, lout, head);
    } else {
        const dim3 g(grid_for(fast, kBlock, std::max<uint64_t>(1, kMaxBlocks / gy)), gy);
        if (order_c) k_d2s_scalar<T, true><<<g, kBlock, 0, st>>>(src, rows, cols, w, out, oi, oj);
        else k_d2s_scalar<T, false><<<g, kBlock, 0, st>>>(src, rows, cols, w, out, oi, oj);
    }
    SNPMI_HIP(hipGetLastError());
}

template <typename T>
void launch_snp_to_dist(const T* val, uint64_t count, int order_c, T factor, T* out, hipStream_t st) {
    if (count == 0) return;
    constexpr uint64_t V = 16 / sizeof(T);
    const bool aligned = elem_mod16(val) == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    if (order_c) {
        if (aligned) k_s2d_c<T, true><<<grid_for(count / V + 1, kBlock, kMaxBlocks), kBlock, 0, st>>>(val, count, factor, out);
        else k_s2d_c<T, false><<<grid_for(count, kBlock, kMaxBlocks), kBlock, 0, st>>>(val, count, factor, out);
    } else if (aligned && count % V == 0) {
        k_s2d_f<T, true><<<grid_for(count / V, kBlock, kMaxBlocks), kBlock, 0, st>>>(val, count, factor, out);
    } else {
        k_s2d_f<T, false><<<grid_for(count, kBlock, kMaxBlocks), kBlock, 0, st>>>(val, count, factor, out);
    }
    SNPMI_HIP(hipGetLastError());
}

template <typename T>
struct DT;
template <>
struct DT<float> {
    static constexpr int v = SNPMI_DT_F32;
};
template <>
struct DT<double> {
    static constexpr int v = SNPMI_DT_F64;
};

template <typename T>
Weights<T> weights_of(double max_weight) {
    const T mw = (T)max_weight;
    return {(T)0 * mw, (T)0.5 * mw, (T)1 * mw};
}

// staged bytes per chunk of a host distribution array (and per chunk of a host output)
constexpr uint64_t kStageBytes = 256ull << 20;

// SNPs [c0, c0 + cc) of the SNP range [col0, ...) of `dist` as a source view.  Device arrays are
// viewed in place.  Of a host array only the wanted slabs are uploaded (on the compute stream, ahead
// of the kernel that reads them): three contiguous rows x cc runs in F order, one 2-D copy of
// rows x 3 cc with the array's row pitch in C order.
template <typename T>
DistSrc<T> dist_view(Device& d, const T* dist, bool dev, uint64_t rows, uint64_t cols_total, uint64_t col, uint64_t cc,
                     int order_c) {
    if (dev) {
        if (order_c) return {dist + col * 3, 3 * cols_total, 3, 1};
        return {dist + col * rows, 1, rows, rows * cols_total};
    }
    if (order_c) {
        T* s = (T*)d.get(Device::S_DIST, rows * 3 * cc * sizeof(T));
        SNPMI_HIP(hipMemcpy2DAsync(s, 3 * cc * sizeof(T), dist + col * 3, 3 * cols_total * sizeof(T), 3 * cc * sizeof(T),
                                   rows, hipMemcpyHostToDevice, d.stream));
        return {s, 3 * cc, 3, 1};
    }
    const uint64_t plane = round_up(rows * cc, 64);  // 16-B aligned planes
    T* s = (T*)d.get(Device::S_DIST, 3 * plane * sizeof(T));
    for (uint64_t k = 0; k < 3; k++)
        SNPMI_HIP(hipMemcpyAsync(s + k * plane, dist + (k * cols_total + col) * rows, rows * cc * sizeof(T),
                                 hipMemcpyHostToDevice, d.stream));
    return {s, 1, rows, plane};
}

template <typename T>
void check_range(const T* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols) {
    SNPMI_REQUIRE(col0 <= cols_total && cols <= cols_total - col0, SNPMI_E_INDEX, "SNP range outside the dist array");
    SNPMI_REQUIRE(dist != nullptr || rows == 0 || cols == 0, SNPMI_E_ARG, "dist is NULL");
    SNPMI_REQUIRE(rows < (1ull << 40) && cols_total < (1ull << 40), SNPMI_E_ARG, "dist array too large");
}

template <typename T>
void dist_to_snp_impl(const T* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols, int order_c,
                      double max_weight, T* out, int out_c) {
    std::lock_guard<std::recursive_mutex> lk(call_mutex());
    check_range(dist, rows, cols_total, col0, cols);
    if (rows == 0 || cols == 0) return;
    SNPMI_REQUIRE(out != nullptr, SNPMI_E_ARG, "out is NULL");
    Device& d = device();
    const bool dev_in = is_device_ptr(d, dist), dev_out = is_device_ptr(d, out);
    const Weights<T> w = weights_of<T>(max_weight);
    // one chunk when both sides are in HBM; else SNP chunks of bounded staging
    const uint64_t per_snp = rows * sizeof(T) * ((dev_in ? 0 : 3) + (dev_out ? 0 : 1));
    const uint64_t step = per_snp ? std::max<uint64_t>(1, kStageBytes / per_snp) : cols;
    for (uint64_t c0 = 0; c0 < cols; c0 += step) {
        const uint64_t cc = std::min(step, cols - c0);
        const DistSrc<T> src = dist_view(d, dist, dev_in, rows, cols_total, col0 + c0, cc, order_c);
        if (dev_out) {
            launch_dist_to_snp(src, order_c, rows, cc, w, out + (out_c ? c0 : c0 * rows), out_c ? cols : 1,
                               out_c ? 1 : rows, out_c, d.stream);
            continue;
        }
        T* o = (T*)d.get(Device::S_DIST_OUT, rows * cc * sizeof(T));
        launch_dist_to_snp(src, order_c, rows, cc, w, o, out_c ? cc : 1, out_c ? 1 : rows, out_c, d.stream);
        if (out_c)
            SNPMI_HIP(hipMemcpy2DAsync(out + c0, cols * sizeof(T), o, cc * sizeof(T), cc * sizeof(T), rows,
                                       hipMemcpyDeviceToHost, d.stream));
        else
            SNPMI_HIP(hipMemcpyAsync(out + c0 * rows, o, rows * cc * sizeof(T), hipMemcpyDeviceToHost, d.stream));
    }
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

template <typename T>
void snp_to_dist_impl(const T* val, uint64_t rows, uint64_t cols, int order_c, double max_weight, T* out) {
    std::lock_guard<std::recursive_mutex> lk(call_mutex());
    if (rows == 0 || cols == 0) return;
    SNPMI_REQUIRE(val != nullptr && out != nullptr, SNPMI_E_ARG, "NULL argument");
    SNPMI_REQUIRE(rows < (1ull << 40) && cols < (1ull << 40), SNPMI_E_ARG, "value array too large");
    Device& d = device();
    const bool dev_in = is_device_ptr(d, val), dev_out = is_device_ptr(d, out);
    const T factor = (T)(2.0 / max_weight);
    const uint64_t count = rows * cols;
    if (dev_in && dev_out) {
        launch_snp_to_dist(val, count, order_c, factor, out, d.stream);
        SNPMI_HIP(hipStreamSynchronize(d.stream));
        return;
    }
    // a host side: chunks of whole lines (SNPs in F order, iids in C), each one a contiguous run of
    // val; its triples are contiguous in C order and three runs (one per plane) in F order
    const uint64_t line = order_c ? cols : rows, lines = order_c ? rows : cols;
    const uint64_t step = std::max<uint64_t>(1, kStageBytes / (4 * line * sizeof(T)));
    for (uint64_t l0 = 0; l0 < lines; l0 += step) {
        const uint64_t cnt = std::min(step, lines - l0) * line, t0 = l0 * line;
        const T* v = val + t0;
        if (!dev_in) {
            T* s = (T*)d.get(Device::S_DIST, cnt * sizeof(T));
            SNPMI_HIP(hipMemcpyAsync(s, v, cnt * sizeof(T), hipMemcpyHostToDevice, d.stream));
            v = s;
        }
        T* o = (T*)d.get(Device::S_DIST_OUT, 3 * cnt * sizeof(T));
        launch_snp_to_dist(v, cnt, order_c, factor, o, d.stream);
        if (order_c) {
            SNPMI_HIP(hipMemcpyAsync(out + 3 * t0, o, 3 * cnt * sizeof(T), hipMemcpyDefault, d.stream));
        } else {
            for (uint64_t k = 0; k < 3; k++)  // the chunk's planes are cnt apart, the array's count
                SNPMI_HIP(hipMemcpyAsync(out + k * count + t0, o + k * cnt, cnt * sizeof(T), hipMemcpyDefault,
                                         d.stream));
        }
    }
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

template <typename T>
void grm_add_dist_impl(const T* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols, int order_c,
                       double max_weight, const StdArgs& sa, T* stats) {
    std::lock_guard<std::recursive_mutex> lk(call_mutex());
    check_range(dist, rows, cols_total, col0, cols);
    uint64_t ldz = 0;
    T* Z = (T*)grm_session_operand(DT<T>::v, rows, cols, &ldz);
    if (rows == 0 || cols == 0) return;
    SNPMI_REQUIRE(sa.kind == SNPMI_STD_NONE || stats != nullptr, SNPMI_E_ARG, "stats is NULL");
    Device& d = device();
    const bool dev_in = is_device_ptr(d, dist);
    const Weights<T> w = weights_of<T>(max_weight);
    // rows [rows, ldz) of Z are never written here and never read by the standardize or the SYRKs
    const uint64_t step = dev_in ? cols : std::max<uint64_t>(1, kStageBytes / (3 * rows * sizeof(T)));
    for (uint64_t c0 = 0; c0 < cols; c0 += step) {
        const uint64_t cc = std::min(step, cols - c0);
        const DistSrc<T> src = dist_view(d, dist, dev_in, rows, cols_total, col0 + c0, cc, order_c);
        launch_dist_to_snp(src, order_c, rows, cc, w, Z + c0 * ldz, 1, ldz, 0, d.stream);
    }
    grm_session_add_operand(DT<T>::v, Z, ldz, cols, sa, stats);
}

}  // namespace
}  // namespace snpmi

using namespace snpmi;

extern "C" {

int snpmi_dist_to_snp_f32(const float* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols,
                          int order_c, double max_weight, float* out, int out_order_c) {
    return guarded([&] { dist_to_snp_impl(dist, rows, cols_total, col0, cols, order_c, max_weight, out, out_order_c); });
}
int snpmi_dist_to_snp_f64(const double* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols,
                          int order_c, double max_weight, double* out, int out_order_c) {
    return guarded([&] { dist_to_snp_impl(dist, rows, cols_total, col0, cols, order_c, max_weight, out, out_order_c); });
}
int snpmi_snp_to_dist_f32(const float* val, uint64_t rows, uint64_t cols, int order_c, double max_weight, float* out) {
    return guarded([&] { snp_to_dist_impl(val, rows, cols, order_c, max_weight, out); });
}
int snpmi_snp_to_dist_f64(const double* val, uint64_t rows, uint64_t cols, int order_c, double max_weight,
                          double* out) {
    return guarded([&] { snp_to_dist_impl(val, rows, cols, order_c, max_weight, out); });
}
#define SNPMI_GRM_ADD_DIST(SUFFIX, T)                                                                               \
    int snpmi_grm_add_dist_##SUFFIX(const T* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols, \
                                    int order_c, double max_weight, int std_kind, double a, double b, int use_stats, \
                                    T* stats) {                                                                      \
        return guarded([&] {                                                                                         \
            grm_add_dist_impl(dist, rows, cols_total, col0, cols, order_c, max_weight,                               \
                              StdArgs{std_kind, a, b, use_stats}, stats);                                            \
        });                                                                                                          \
    }
SNPMI_GRM_ADD_DIST(f32, float)
SNPMI_GRM_ADD_DIST(f64, double)

}  // extern "C"
