// Device helpers shared by the SYRK kernels of syrk.hip and syrk_crt.hip: which block of K a
// workgroup computes, and the in-group iid order of the bf16 / fp16 / int8 LDS images.
#pragma once
#include "snpmi_internal.hpp"

namespace snpmi {

// upper-triangle index L = tj (tj + 1) / 2 + ti  ->  (ti, tj), ti <= tj
__device__ __forceinline__ void tile_coords(uint64_t L, uint32_t& ti, uint32_t& tj) {
    uint64_t j = (uint64_t)((sqrt(8.0 * (double)L + 1.0) - 1.0) * 0.5);
    while ((j + 1) * (j + 2) / 2 <= L) j++;
    while (j * (j + 1) / 2 > L) j--;
    tj = (uint32_t)j;
    ti = (uint32_t)(L - j * (j + 1) / 2);
}

// position of iid p of a 16-iid group in the LDS rows the v_perm loaders build (a 4x4 transpose,
// an involution; syrk.hip "Cheap expansion")
__device__ __forceinline__ int pi16(int p) { return 4 * (p & 3) + (p >> 2); }

// Block (bi, bj) of workgroup wg = wg0 + x (the launch's first block + the workgroup's index in
// it), in one of the three orders the SYRK grids use:
//   RECT       every block of the two-operand rectangle, bi fastest inside bj (rb.nba block rows);
//   use_table  entry wg of a bi | bj << 16 table (supertile_order, or a cfg5 part's part_layout);
//   otherwise  the upper triangle, column by column (tile_coords).
// The caller decides use_table, so a kernel whose test is a template constant keeps it one.  wg0
// and x stay apart so that each branch forms its own sum, as the CRT kernels did before they
// shared this function (with one sum ahead of the branches their scalar registers are
// renumbered); a kernel that already holds the sum passes it as wg0, with x = 0.
template <bool RECT>
__device__ __forceinline__ void block_coords(uint64_t wg0, uint32_t x, bool use_table, const uint32_t* table,
                                             const RectArg<RECT>& rb, uint32_t& bi, uint32_t& bj) {
    if constexpr (RECT) {
        bi = (uint32_t)((wg0 + x) % rb.nba);
        bj = (uint32_t)((wg0 + x) / rb.nba);
    } else if (use_table) {
        const uint32_t c = table[wg0 + x];
        bi = c & 0xffffu;
        bj = c >> 16;
    } else {
        tile_coords(wg0 + x, bi, bj);
    }
}

}  // namespace snpmi
