// Memory-bound kernels of the two-operand ("rect") GRM, K[rows, cols] computed directly (gfx950):
//   k_rect_extract       the rectangle's dense 256 x 256 blocks -> K_out[n_r][n_c]
//   k_rect_diag_save /   exact f32 diagonal of the positions with rows[r] == cols[c], around one
//   k_rect_diag_patch    launch (the sums of squares come from kernels.hip k_diag_sq)
// The block layout is the two-operand SYRK kernels' (syrk.hip, syrk_crt.hip): block (bi, bj) at
// slot bj * nba + bi, row-major.  Reference call site: kernelreader/snpkernel.py:84-88.
#include <algorithm>

#include "snpmi_internal.hpp"

namespace snpmi {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ uint64_t rect_offset(uint64_t nba, uint64_t r, uint64_t c) {
    return ((c / 256) * nba + r / 256) * 65536 + (r % 256) * 256 + (c % 256);
}

// the outer range [o0, o0 + no) of the output's slow axis (rows in C order, columns in F order),
// written contiguously
template <typename T>
__global__ __launch_bounds__(kBlock) void k_rect_extract(const T* __restrict__ blocks, uint64_t nba, uint64_t inner,
                                                         uint64_t o0, uint64_t no, int out_c, double scale,
                                                         T* __restrict__ out) {
    const uint64_t total = no * inner;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o = o0 + t / inner, in = t % inner;
        const uint64_t r = out_c ? o : in, c = out_c ? in : o;
        T v = blocks[rect_offset(nba, r, c)];
        if (scale != 1.0) v = (T)((double)v * scale);
        out[t] = v;
    }
}

// pair p = (r, c) with rows[r] == cols[c]: a diagonal element of K inside the rectangle
__global__ __launch_bounds__(kBlock) void k_rect_diag_save(const float* __restrict__ blocks, uint64_t nba,
                                                           const uint32_t* __restrict__ pairs, uint64_t npairs,
                                                           int accumulate, double* __restrict__ saved) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npairs; p += (uint64_t)gridDim.x * blockDim.x)
        saved[p] = accumulate ? (double)blocks[rect_offset(nba, pairs[2 * p], pairs[2 * p + 1])] : 0.0;
}

__global__ __launch_bounds__(kBlock) void k_rect_diag_patch(float* __restrict__ blocks, uint64_t nba,
                                                            const uint32_t* __restrict__ pairs, uint64_t npairs,
                                                            const double* __restrict__ saved,
                                                            const double* __restrict__ sq) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npairs; p += (uint64_t)gridDim.x * blockDim.x)
        blocks[rect_offset(nba, pairs[2 * p], pairs[2 * p + 1])] = (float)(saved[p] + sq[pairs[2 * p]]);
}

inline unsigned grid_for(uint64_t work, uint64_t per_block, unsigned cap) {
    const uint64_t g = std::max<uint64_t>(1, ceil_div(work, per_block));
    return (unsigned)std::min<uint64_t>(g, cap);
}

}  // namespace

void launch_rect_extract(const void* blocks, int dtype, uint64_t nba, uint64_t inner, uint64_t o0, uint64_t no,
                         int order_c, double scale, void* out, hipStream_t st) {
    if (no * inner == 0) return;
    const unsigned g = grid_for(no * inner, kBlock * 4, 1u << 20);
    if (dtype == SNPMI_DT_F64)
        k_rect_extract<double><<<g, kBlock, 0, st>>>((const double*)blocks, nba, inner, o0, no, order_c, scale, (double*)out);
    else
        k_rect_extract<float><<<g, kBlock, 0, st>>>((const float*)blocks, nba, inner, o0, no, order_c, scale, (float*)out);
    SNPMI_HIP(hipGetLastError());
}

void launch_rect_diag_save(const float* blocks, uint64_t nba, const uint32_t* pairs, uint64_t npairs, int accumulate,
                           double* saved, hipStream_t st) {
    if (npairs == 0) return;
    k_rect_diag_save<<<grid_for(npairs, kBlock, 65536), kBlock, 0, st>>>(blocks, nba, pairs, npairs, accumulate, saved);
    SNPMI_HIP(hipGetLastError());
}

void launch_rect_diag_patch(float* blocks, uint64_t nba, const uint32_t* pairs, uint64_t npairs, const double* saved,
                            const double* sq, hipStream_t st) {
    if (npairs == 0) return;
    k_rect_diag_patch<<<grid_for(npairs, kBlock, 65536), kBlock, 0, st>>>(blocks, nba, pairs, npairs, saved, sq);
    SNPMI_HIP(hipGetLastError());
}

}  // namespace snpmi
