/*
 * snpmi.h -- C ABI of libsnpmi.so, the MI355X-native (gfx950, HIP) implementation of
 * PySnpTools' BED decode -> slice -> standardize -> SnpKernel GRM path.
 *
 * The reference crosses into native code through the Rust/PyO3 module `bed_reader`
 * and NumPy BLAS; every host entry point below replaces one of those call sites
 * (paths relative to /root/reference/pysnptools):
 *
 *   snpmi_bed_check              bed_reader.open_bed(...) format check    snpreader/bed.py:137-145
 *   snpmi_bed_read_{f32,f64,i8}  open_bed(...).read(index,order,dtype)     snpreader/bed.py:337-343
 *   snpmi_standardize_{f32,f64}  bed_reader.standardize_f32/f64(...)       standardizer/standardizer.py:114,120
 *   snpmi_subset_*               bed_reader.subset_f64_f64/f32_f64/f32_f32 util/__init__.py:341-375
 *   snpmi_bed_read_standardize_* Bed.read() + SnpData.standardize() fused  snpreader/snpreader.py:606-621
 *   snpmi_grm_bed_{f32,f64}      SnpReader._read_kernel block loop         snpreader/snpreader.py:623-668
 *   snpmi_grm_dense_{f32,f64}    SnpData._read_kernel (val.dot(val.T))     snpreader/snpdata.py:190-214
 *   snpmi_diag_k_to_n_{f32,f64}  DiagKtoN._standardize_kernel              standardizer/diag_K_to_N.py:54-64
 *
 * Conventions (mirroring bed-reader's):
 *   - The caller owns every host buffer; outputs are written in place.  Index arrays are
 *     NumPy `uintp` (== uint64_t on LP64).  A NULL index array means "all, in order".
 *   - `order_c` = 1 for C order (row-major, SNP fastest), 0 for F order (iid fastest).
 *   - `stats` arrays are C-order [n_sid][2] = (mean, std) in the value dtype.
 *   - Missing values decode to NaN (float) or -127 (int8).  count_a1 selects the A1 LUT
 *     {2,NaN,1,0} instead of {0,NaN,1,2}.
 *   - Every function returns 0 on success or one of the SNPMI_E_* codes; the message of
 *     the calling thread's last failure is available from snpmi_last_error().
 *   - `num_threads` sizes the host-side gather pool only; all arithmetic runs on the GPU.
 *     There is no CPU fallback: without a HIP device every compute entry point fails
 *     with SNPMI_E_HIP.
 *   - K outputs are n_out x n_out, symmetric; order_c selects the layout of non-square
 *     subsets produced by snpmi_kernel_subset_*.
 *   - Value and K buffers (`out`, `val`, `K_out`, `K`, subset in/out) may be HOST memory or
 *     DEVICE memory of the current device (snpmi_dev_alloc / hipMalloc; HIP unified
 *     addressing tells them apart).  Device buffers are computed on in place or written
 *     directly, with no host staging: this is the array-module seam of the reference
 *     (util/__init__.py:652-730, ARRAY_MODULE=cupy keeps SnpData/KernelData values on the GPU),
 *     used by pysnptools_amd.hbm.  Stats and index arrays are always host memory.  A device
 *     buffer of another device fails with SNPMI_E_ARG.
 *
 * Deliberate semantics where the reference's two paths differ (the reference calls bed-reader's
 * native standardize by default, standardizer.py:114,120, but none of its fixtures pins the
 * native behaviour below; these follow the reference's Python path, standardizer.py:136-211,
 * which its goldens do pin -- "parity unpinned" against bed-reader itself):
 *   - a SNP with no observed value (n = 0) trains NaN stats and standardizes to an all-zero
 *     column; bed-reader's native code would raise NoIndividuals.
 *   - Beta with a trained/given mean outside [0, 2]: maf = mean/2 (folded to <= 0.5) leaves
 *     [0, 1] and the weight is 0 -- scipy.stats.beta.pdf's value there -- so the column
 *     standardizes to zeros; bed-reader would raise IllegalSnpMean.
 *   - f32 stats and LUTs are computed in f64 and rounded once (the one-pass formula in f32
 *     arithmetic misses the reference Python path by 1.47e-5 on N300); bed-reader's f32 native
 *     path has no fixture.  The claim is "matches the reference Python path", not bed-reader.
 */
#ifndef SNPMI_H
#define SNPMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNPMI_OK 0
#define SNPMI_E_ARG 1     /* bad argument (shape, dtype, order, NULL pointer)        */
#define SNPMI_E_INDEX 2   /* iid/sid index out of range                              */
#define SNPMI_E_FORMAT 3  /* not a SNP-major .bed file, or size mismatch             */
#define SNPMI_E_IO 4      /* open/read/mmap failure                                  */
#define SNPMI_E_HIP 5     /* HIP runtime error (includes "no device")                */
#define SNPMI_E_NOMEM 6   /* device or pinned allocation failed                      */
#define SNPMI_E_RCCL 7    /* RCCL error                                              */

/* standardizer kinds (standardizer/{identity,unit,beta}.py) */
#define SNPMI_STD_NONE 0  /* raw values (Identity)                                   */
#define SNPMI_STD_UNIT 1  /* (x - mean) / std, NaN -> 0                              */
#define SNPMI_STD_BETA 2  /* (x - mean) * BetaPDF(maf; a, b), NaN -> 0               */

/* dtypes for the device-resident API */
#define SNPMI_DT_F32 0
#define SNPMI_DT_F64 1
#define SNPMI_DT_I8 2

/* ---------------------------------------------------------------- runtime */
const char* snpmi_last_error(void);
int snpmi_version(void);
int snpmi_device_count(int* count);
int snpmi_set_device(int device);            /* device used by later calls of this thread */
int snpmi_get_device(int* device);
int snpmi_release_cache(void);               /* free cached device/pinned scratch          */
int snpmi_device_info(int device, char* name, size_t name_len, uint64_t* total_mem, int* cu_count);
/* the box a measurement ran on: 16-byte device UUID, PCI domain / bus / device, max SCLK (kHz) */
int snpmi_device_ids(int dev, uint8_t* uuid16, int* pci, int* clock_khz);
/* select a kernel variant by name; 0 = default.  Public switches: "f64" (0 = f64 GRMs as int8
 * residues + CRT, 1 = on the f64 MFMA), "seg" (SNPs per f32 GRM accumulation chain, default 12288,
 * 0 = one chain per launch).  The rest ("decode", "syrk", "part_order" (1 = the cfg5 part
 * kernel in triangular block order), ...) are A/B hooks for benches. */
int snpmi_set_kernel_variant(const char* kernel, int variant);
int snpmi_get_kernel_variant(const char* kernel, int* variant);  /* current value of a hook above */

/* ---------------------------------------------------------------- BED reading (bed-reader read_*) */
int snpmi_bed_check(const char* path, uint64_t n_iid, uint64_t n_sid);
int snpmi_bed_read_f32(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                       const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx,
                       uint64_t n_out_sid, int order_c, float* out, int num_threads);
int snpmi_bed_read_f64(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                       const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx,
                       uint64_t n_out_sid, int order_c, double* out, int num_threads);
int snpmi_bed_read_i8(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                      const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx,
                      uint64_t n_out_sid, int order_c, int8_t* out, int num_threads);

/* ---------------------------------------------------------------- .fam/.bim metadata (host, threaded)
 * Replaces the text parsing behind bed-reader open_bed's properties (fid/iid/sid/chromosome/
 * cm_position/bp_position; snpreader/bed.py:137-194).  Lines are split on whitespace, blank
 * lines skipped.  scan: number of rows and the widest field of columns 0..n_cols-1 (every line
 * must have >= min_fields fields, else SNPMI_E_FORMAT).  strings: column `col` as fixed-width
 * NUL-padded rows of `width` bytes.  f64: column `col` parsed as a float (SNPMI_E_FORMAT if
 * it is not one).  No GPU is needed. */
int snpmi_text_scan(const char* path, int min_fields, int n_cols, uint64_t* n_rows, uint64_t* widths,
                    int num_threads);
int snpmi_text_strings(const char* path, int col, uint64_t n_rows, uint64_t width, char* out, int num_threads);
int snpmi_text_f64(const char* path, int col, uint64_t n_rows, double* out, int num_threads);

/* ---------------------------------------------------------------- BED writing (bed-reader to_bed body)
 * Replaces the genotype half of `to_bed(filepath, val, properties, count_A1, ...)`
 * (snpreader/bed.py:300-314); the .fam/.bim text is written by the host.  val is
 * n_iid x n_sid (F or C order); values must be 0, 1, 2 or missing (NaN; -127 for int8),
 * anything else -> SNPMI_E_ARG (ValueError) and no file is left behind. */
int snpmi_bed_write_f32(const char* path, const float* val, uint64_t n_iid, uint64_t n_sid, int order_c,
                        int count_a1, int num_threads);
int snpmi_bed_write_f64(const char* path, const double* val, uint64_t n_iid, uint64_t n_sid, int order_c,
                        int count_a1, int num_threads);
int snpmi_bed_write_i8(const char* path, const int8_t* val, uint64_t n_iid, uint64_t n_sid, int order_c,
                       int count_a1, int num_threads);

/* ---------------------------------------------------------------- standardize (bed-reader standardize_*) */
int snpmi_standardize_f32(float* val, uint64_t rows, uint64_t cols, int order_c, int is_beta,
                          double a, double b, int apply_in_place, int use_stats, float* stats,
                          int num_threads);
int snpmi_standardize_f64(double* val, uint64_t rows, uint64_t cols, int order_c, int is_beta,
                          double a, double b, int apply_in_place, int use_stats, double* stats,
                          int num_threads);

/* ---------------------------------------------------------------- subset (bed-reader subset_*) */
/* out[i,j,q] = val[row_idx[i], col_idx[j], q]; val is rows x cols x k in in_order_c. */
int snpmi_subset_f64_f64(const double* val, uint64_t rows, uint64_t cols, uint64_t k, int in_order_c,
                         const uint64_t* row_idx, uint64_t n_rows, const uint64_t* col_idx,
                         uint64_t n_cols, int out_order_c, double* out, int num_threads);
int snpmi_subset_f32_f64(const float* val, uint64_t rows, uint64_t cols, uint64_t k, int in_order_c,
                         const uint64_t* row_idx, uint64_t n_rows, const uint64_t* col_idx,
                         uint64_t n_cols, int out_order_c, double* out, int num_threads);
int snpmi_subset_f32_f32(const float* val, uint64_t rows, uint64_t cols, uint64_t k, int in_order_c,
                         const uint64_t* row_idx, uint64_t n_rows, const uint64_t* col_idx,
                         uint64_t n_cols, int out_order_c, float* out, int num_threads);

/* ---------------------------------------------------------------- fused read + standardize */
int snpmi_bed_read_standardize_f32(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                                   const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx,
                                   uint64_t n_out_sid, int order_c, int std_kind, double a, double b,
                                   int use_stats, float* stats, float* out, int num_threads);
int snpmi_bed_read_standardize_f64(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                                   const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx,
                                   uint64_t n_out_sid, int order_c, int std_kind, double a, double b,
                                   int use_stats, double* stats, double* out, int num_threads);

/* ---------------------------------------------------------------- GRM (SnpKernel) */
/* K_out: n_out_iid x n_out_iid (symmetric).  stats: [n_out_sid][2] in/out (in if use_stats).
 * diag_k_to_n != 0 additionally applies DiagKtoN on the device and returns the factor. */
int snpmi_grm_bed_f32(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                      const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx,
                      uint64_t n_out_sid, int std_kind, double a, double b, int use_stats,
                      float* stats, int diag_k_to_n, double* factor, float* K_out, int num_threads);
int snpmi_grm_bed_f64(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                      const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx,
                      uint64_t n_out_sid, int std_kind, double a, double b, int use_stats,
                      double* stats, int diag_k_to_n, double* factor, double* K_out, int num_threads);
int snpmi_grm_dense_f32(const float* val, uint64_t rows, uint64_t cols, int order_c, int std_kind,
                        double a, double b, int use_stats, float* stats, int diag_k_to_n,
                        double* factor, float* K_out);
int snpmi_grm_dense_f64(const double* val, uint64_t rows, uint64_t cols, int order_c, int std_kind,
                        double a, double b, int use_stats, double* stats, int diag_k_to_n,
                        double* factor, double* K_out);
/* GRM over several .bed files that share the iids -- DistributedBed / _MergeSIDs pieces,
 * per-chromosome shards (distributedbed.py:16-207, pstreader/_mergecols.py:117-159, reached
 * from SnpReader._read_kernel snpreader.py:623-668 on a merged reader).  begin ->
 * add_bed (any number; stats per file as in snpmi_grm_bed_*) -> end (DiagKtoN + copy-out).
 * For one process per GPU, add this rank's files, then all-reduce the session tiles
 * (snpmi_grm_session_tiles + snpmi_rccl_allreduce_sum) before end. */
int snpmi_grm_begin(uint64_t n_out_iid, int dtype);
int snpmi_grm_add_bed_f32(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                          const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx,
                          uint64_t n_out_sid, int std_kind, double a, double b, int use_stats,
                          float* stats, int num_threads);
int snpmi_grm_add_bed_f64(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                          const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx,
                          uint64_t n_out_sid, int std_kind, double a, double b, int use_stats,
                          double* stats, int num_threads);
/* snpmi_grm_add_bed_{f32,f64} as the session's LAST add (a rank's SNP span of a .bed) + the K-tile
 * collective (1 = reduce onto root, 2 = all-reduce, 0 = none), overlapped on the file stream's last
 * chunk as in snpmi_grm_add_packed_reduce_*: shard.grm_sharded under RCCL (snpreader.py:623-668
 * per rank, then the sum over ranks).  Same K bit for bit as the add followed by the collective. */
int snpmi_grm_add_bed_reduce_f32(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1, const uint64_t* iid_idx,
                                 uint64_t n_out_iid, const uint64_t* sid_idx, uint64_t n_out_sid, int std_kind,
                                 double a, double b, int use_stats, float* stats, int num_threads, int collective,
                                 int root, int parts);
int snpmi_grm_add_bed_reduce_f64(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1, const uint64_t* iid_idx,
                                 uint64_t n_out_iid, const uint64_t* sid_idx, uint64_t n_out_sid, int std_kind,
                                 double a, double b, int use_stats, double* stats, int num_threads, int collective,
                                 int root, int parts);
/* add Z Z^T of an already standardized rows x cols block (F or C order) to the session */
int snpmi_grm_add_dense_f32(const float* val, uint64_t rows, uint64_t cols, int order_c);
int snpmi_grm_add_dense_f64(const double* val, uint64_t rows, uint64_t cols, int order_c);
/* add packed SNP columns already in HBM ([n_sid][pitch] bytes, pitch = snpmi_packed_pitch(n_iid),
 * every iid of the session) -- the per-rank shard of shard.grm_sharded / bench.py's cfg4 leg
 * (the block loop of snpreader.py:651-655 over a device-resident BED body).  The library runs
 * one stats + one SYRK launch per <= 65536 SNPs.  stats [n_sid][2]: host memory (synchronous) or
 * device memory (the call only enqueues on the library stream). */
int snpmi_grm_add_packed_f32(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, int count_a1,
                             int std_kind, double a, double b, int use_stats, float* stats);
int snpmi_grm_add_packed_f64(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, int count_a1,
                             int std_kind, double a, double b, int use_stats, double* stats);
/* snpmi_grm_add_packed_f32 (the session's LAST add) + the K-tile collective of the SNP-sharded
 * GRM (snpmi_rccl_reduce_sum / _allreduce_sum; collective 1 = reduce onto root, 2 = all-reduce,
 * 0 = none), overlapped: the last SNP chunk's SYRK runs as `parts` column groups of the triangle
 * (same K bit for bit) and each finished group's contiguous tile range is summed on the aux stream
 * under the next group's SYRK; the compute stream waits for the last sum.  Host stats (or a path
 * without column groups) run the add and then the collective, unoverlapped.  syrk_done (optional hipEvent_t from snpmi_event_create) is
 * recorded after the last group's SYRK.  Replaces the add + reduce pair of shard.ShardedGrm
 * (the rank loop of snpreader.py:651-655 followed by the sum over ranks). */
int snpmi_grm_add_packed_reduce_f32(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                                    int count_a1, int std_kind, double a, double b, int use_stats, float* stats,
                                    int collective, int root, int parts, void* syrk_done);
/* f64: the groups are the int8-CRT path's residue chunks of the last launch (cut at block-column
 * boundaries; `parts` is ignored) */
int snpmi_grm_add_packed_reduce_f64(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                                    int count_a1, int std_kind, double a, double b, int use_stats, double* stats,
                                    int collective, int root, int parts, void* syrk_done);
int snpmi_grm_session_tiles(void** tiles, uint64_t* count);   /* device tiles + element count */
/* The session's K-tile collective over the ranks (1 = reduce onto root, 2 = all-reduce), without
 * an add: the same RCCL calls, in the same order, as snpmi_grm_add_*_reduce_* with the same
 * `parts` -- a rank that owns no SNPs (or added its SNPs unoverlapped) joins the others' ranged sums
 * with this call.  The calls depend only on n, dtype, parts and the kernel configuration, never on
 * a rank's SNP count.  Replaces the sum over ranks after the block loop of snpreader.py:651-655. */
int snpmi_grm_session_sum(int collective, int root, int parts);
/* K_out NULL: end the session without a result (a non-root rank after snpmi_rccl_reduce_sum) */
int snpmi_grm_end(int diag_k_to_n, double* factor, void* K_out);
int snpmi_diag_k_to_n_f32(float* K, uint64_t n, double* factor);
/* SNP-side DiagKtoN (standardizer/diag_K_to_N.py:75-95): factor = rows / sum(val^2) (f64
 * accumulation); val *= sqrt(factor) unless |factor - 1| <= 1e-15.  val is any contiguous
 * rows x cols array (order does not matter). */
int snpmi_diag_k_to_n_snps_f32(float* val, uint64_t rows, uint64_t cols, double* factor);
int snpmi_diag_k_to_n_snps_f64(double* val, uint64_t rows, uint64_t cols, double* factor);
/* val[i] *= scale for a contiguous host array (DiagKtoNTrained.standardize, diag_K_to_N.py:101-159) */
int snpmi_scale_f32(float* val, uint64_t count, double scale);
int snpmi_scale_f64(double* val, uint64_t count, double scale);
int snpmi_diag_k_to_n_f64(double* K, uint64_t n, double* factor);

/* ---------------------------------------------------------------- genotype distributions (dist.hip)
 * A distribution array is rows x cols_total x 3 (iid, SNP, probability of 0 / 1 / 2 copies), host
 * memory or device memory of the current device.  F order: element (i, s, k) at
 * i + rows * s + rows * cols_total * k (three planes); C order: at (i * cols_total + s) * 3 + k.
 * The calls below work on the SNPs [col0, col0 + cols) of it; of a host array only those slabs
 * are uploaded, in SNP chunks of bounded scratch. */
/* Expected values, replacing `(distdata.val * weights).sum(axis=-1)` of snpreader/_dist2snp.py:47-52:
 * with w = {0, .5, 1} * max_weight in T, out[i, s] = ((0 + p0 w0) + p1 w1) + p2 w2 in T, bit for
 * bit NumPy's sum (NaN when any component is; +0 when all three products are -0).  out is tight
 * rows x cols in out_order_c. */
int snpmi_dist_to_snp_f32(const float* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols,
                          int order_c, double max_weight, float* out, int out_order_c);
int snpmi_dist_to_snp_f64(const double* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols,
                          int order_c, double max_weight, double* out, int out_order_c);
/* One-hot distributions of SNP values, replacing _snpval_to_distval of distreader/_snp2dist.py:41-54:
 * out[i, s, c] = 1 where (T)(val * (T)(2 / max_weight)) == c, else 0; a value that matches no c
 * (NaN included) gives NaN in all three.  out is rows x cols x 3 in val's order. */
int snpmi_snp_to_dist_f32(const float* val, uint64_t rows, uint64_t cols, int order_c, double max_weight, float* out);
int snpmi_snp_to_dist_f64(const double* val, uint64_t rows, uint64_t cols, int order_c, double max_weight,
                          double* out);
/* Inside a GRM session of `rows` iids: expected values of the SNP range written straight into the
 * library's dense operand, standardized there (stats [cols][2], host: read if use_stats, else
 * written) and Z Z^T added to the session -- one block of the loop of snpreader.py:651-655 over
 * `dist.as_snp()`, replacing its read (_dist2snp.py:47-52), standardize and `K += Z.dot(Z.T)`. */
int snpmi_grm_add_dist_f32(const float* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols,
                           int order_c, double max_weight, int std_kind, double a, double b, int use_stats,
                           float* stats);
int snpmi_grm_add_dist_f64(const double* dist, uint64_t rows, uint64_t cols_total, uint64_t col0, uint64_t cols,
                           int order_c, double max_weight, int std_kind, double a, double b, int use_stats,
                           double* stats);

/* ---------------------------------------------------------------- device-resident API
 * Buffers below are device pointers from snpmi_dev_alloc; work is enqueued on the
 * library's per-device stream (use snpmi_stream_sync / events).  Packed BED data on the
 * device is [n_sid][pitch] bytes with pitch % 64 == 0 (snpmi_packed_pitch). */
uint64_t snpmi_packed_pitch(uint64_t n_iid);
int snpmi_dev_alloc(void** ptr, uint64_t bytes);
int snpmi_dev_free(void* ptr);
/* page-locked host memory (the staging side of streamed SNP blocks) */
int snpmi_host_alloc(void** ptr, uint64_t bytes);
int snpmi_host_free(void* ptr);
int snpmi_dev_memset(void* ptr, int value, uint64_t bytes);
int snpmi_memcpy_h2d(void* dst, const void* src, uint64_t bytes);
int snpmi_memcpy_d2h(void* dst, const void* src, uint64_t bytes);
/* device -> device on the library stream (asynchronous; bench.py's measured copy peak) */
int snpmi_dev_memcpy_d2d(void* dst, const void* src, uint64_t bytes);
/* device -> device, `rows` rows of `width` bytes at the two pitches (asynchronous, the calling
 * thread's stream): drops the pad rows of a 16-aligned F-order decode without leaving HBM */
int snpmi_dev_memcpy_2d(void* dst, uint64_t dpitch, const void* src, uint64_t spitch, uint64_t width, uint64_t rows);
int snpmi_stream_sync(void);
int snpmi_event_create(void** ev);
int snpmi_event_destroy(void* ev);
int snpmi_event_record(void* ev);
int snpmi_event_elapsed_ms(void* start, void* stop, float* ms);
/* Streaming: the library keeps TWO streams per device -- compute (every kernel above) and copy
 * (DMA).  The file-backed entry points pipeline their chunks across them (H2D of chunk c+1 and
 * D2H of chunk c-1 overlap the kernels of chunk c); these calls let a caller build the same
 * pipeline over its own pinned buffers (snpmi_host_alloc).  on_copy: 0 = compute, 1 = copy.
 * kind: 0 = host->device, 1 = device->host, 2 = device->device.  snpmi_stream_sync waits for
 * both streams. */
int snpmi_memcpy_async(void* dst, const void* src, uint64_t bytes, int kind, int on_copy);
/* on_copy above may also be 2: the aux compute stream.  snpmi_set_stream(which) makes the calling
 * thread's stateless device calls (snpmi_dev_snp_stats / _decode / _decode_standardize /
 * _grm_extract / _memset / _memcpy_d2d, snpmi_event_record, the RCCL calls) enqueue on the compute
 * stream (0, the default) or on the aux stream (2), so a caller can run block k+1's stats beside
 * block k's decode (bench.py --overlap-stats); order the two with snpmi_event_record_on /
 * snpmi_stream_wait_event.  The file-backed and GRM-session entry points always use the compute
 * stream. */
int snpmi_set_stream(int which);
int snpmi_event_record_on(void* ev, int on_copy);
int snpmi_stream_wait_event(void* ev, int on_copy);   /* that stream waits for ev (no host wait) */
int snpmi_event_sync(void* ev);

/* counter-based synthetic genotypes (SnpGen MAF curve, snpreader/snpgen.py:140-151) */
int snpmi_dev_synth_bed(uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t sid0, uint64_t n_sid,
                        uint64_t seed, double miss_rate, const double* maf_x, const double* maf_cdf,
                        int n_pts);
/* the same workload on host threads (streamed cfg5 legs): SNPs [sid0, sid0+n_sid) with the MAF
 * table of snpmi_dev_synth_bed, one 32-bit hash per genotype (a different stream than the device
 * generator, same distribution) */
int snpmi_host_synth_bed(uint8_t* dst, uint64_t pitch, uint64_t n_iid, uint64_t sid0, uint64_t n_sid, uint64_t seed,
                         double miss_rate, const double* maf_x, const double* maf_cdf, int n_pts, int num_threads);
/* SnpGen (snpreader/snpgen.py:164-189): the requested SNPs' packed codes (count_A1 = False), all
 * iids, column k of the output = SNP sid_idx[k]; every batch touched is generated once per call, bit for
 * bit the reference's values. packed: device, [n_sel][pitch] bytes (pitch >= ceil(n_iid / 4); pad
 * bytes are zeroed).  sid_idx (any order, repeats allowed), maf_x and maf_cdf (the MAF points and
 * the normalised cumulative weights of RandomState.choice) are host arrays.  A batch seed
 * seed + (sid / block_size) * block_size above 2**32 - 1 is SNPMI_E_ARG, checked before any
 * launch.  Device scratch is per generator workgroup (about 3 * n_iid * block_size bits), as many
 * workgroups as fit scratch_bytes (0 = 1 GiB; at least one, at most 8 per CU): it does not grow
 * with the request.  A batch that is not full after 4096 rounds (a MAF table that yields no legal
 * SNP) is SNPMI_E_ARG.  Synchronous. */
int snpmi_dev_snpgen_bed(uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t seed, uint64_t block_size,
                         const uint64_t* sid_idx, uint64_t n_sel, const double* maf_x, const double* maf_cdf,
                         int n_pts, uint64_t scratch_bytes);
/* generator workgroups (batches x rounds) the calling thread's last snpmi_dev_snpgen_bed ran; each
 * consumed 2 * block_size * (1 + 3 * n_iid) words of its stream (tools/bench_snpgen.py's rate) */
int snpmi_dev_snpgen_rounds(uint64_t* batch_rounds);
/* the raw stream, for pinning it to numpy: count doubles of RandomState(seed32).random_sample into
 * device memory (one workgroup; synchronous) */
int snpmi_dev_mt19937_random_sample(uint32_t seed32, uint64_t count, double* out_dev);
/* DistGen (distreader/distgen.py:110-165): the requested SNPs' genotype distributions, all iids,
 * bit for bit the reference's values (a float32 output is the float64 value rounded once).  out:
 * device, tight n_iid x n_sel x 3 in C order (out_order_c) or NumPy's F order of the 3-D array
 * (strides 1, n_iid, n_iid * n_sel elements); column k = SNP sid_idx[k].  sid_idx (any order,
 * repeats allowed) is a host array.  SNP s is column s % block_size of batch s / block_size, one
 * MT19937 stream seeded with seed + batch * block_size, always of block_size SNPs; a batch seed
 * above 2^32 - 1 is SNPMI_E_ARG, checked for every batch before any launch.  Every batch touched is
 * generated once per call, by one workgroup, with no device scratch beyond the column tables.
 * n_iid == 0 or n_sel == 0 launches nothing.  Synchronous. */
int snpmi_dev_distgen_f32(float* out, uint64_t n_iid, uint64_t seed, uint64_t block_size, const uint64_t* sid_idx,
                          uint64_t n_sel, int out_order_c);
int snpmi_dev_distgen_f64(double* out, uint64_t n_iid, uint64_t seed, uint64_t block_size, const uint64_t* sid_idx,
                          uint64_t n_sel, int out_order_c);
/* BGEN (distreader/bgen.py; the reference reads through the cbgen library).  Host side, no device:
 * one walk of the file's variant index per call, stepping over the genotype blocks.  Layout 2 with
 * compression none or zlib only (layout 1, zstd: SNPMI_E_FORMAT, as is a file that ends early,
 * naming the variant and offset).  snpmi_bgen_open fills info[11]: variants, samples, the header's
 * flags, the first variant's offset, 1 if the file has a sample identifier block, the widest
 * sample / id / rsid / chromosome / alleles string in bytes (a variant's K alleles are joined with
 * commas), the file size.  snpmi_bgen_index fills arrays sized from those: rec[variant][5] = file
 * offset of the stored genotype bytes, their count, the inflated length, the position, K; and the
 * strings as fixed-width NUL-padded rows (NumPy 'S<width>'; an array whose width is 0 is not
 * written, samples also when the file has no sample block). */
int snpmi_bgen_open(const char* path, uint64_t* info);
int snpmi_bgen_index(const char* path, uint64_t n_variants, uint64_t n_samples, uint64_t* rec, char* samples,
                     uint64_t w_sample, char* ids, uint64_t w_id, char* rsids, uint64_t w_rsid, char* chroms,
                     uint64_t w_chrom, char* alleles, uint64_t w_alleles);
/* Inflated layout-2 genotype blocks (diploid, unphased, biallelic: the caller has checked every
 * block's header and length 10 + N + ceil(2 B N / 8)) -> distributions.  blocks: device, 8-byte
 * aligned, blocks_bytes long; col_table: host, [cols][3] = byte offset of output column s's block
 * (a multiple of 8, with 16 readable bytes behind the block), its bit depth B (1 ... 32) and its
 * sample count N; two columns may name one block.  Row r is sample iid_idx[r] (host or device
 * array, every entry below every N) or, iid_idx NULL, sample r (rows <= every N).  With D = 2^B - 1
 * and (a, b) the sample's two B-bit integers: p0 = a / D, p1 = b / D, p2 = (D - (a + b)) / D, each
 * one f64 division (a float32 output is that value rounded once); three quiet NaNs where the
 * sample's missing bit is set.  out: device, the SNPs [col0, col0 + cols) of a tight rows x
 * cols_total x 3 array in the layouts above (dist.hip).  rows == 0 or cols == 0 launches nothing.
 * Synchronous. */
int snpmi_dev_bgen_decode_f32(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* col_table, uint64_t cols,
                              const uint64_t* iid_idx, uint64_t rows, float* out, uint64_t cols_total, uint64_t col0,
                              int out_order_c);
int snpmi_dev_bgen_decode_f64(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* col_table, uint64_t cols,
                              const uint64_t* iid_idx, uint64_t rows, double* out, uint64_t cols_total, uint64_t col0,
                              int out_order_c);
/* zlib streams inflated in device memory, one wave per stream (csrc/inflate.hip; the decoder is
 * csrc/inflate_core.hpp, no compression library is linked).  src, dst: device; table: host,
 * [streams][4] = byte offset of the stream in src (any alignment), its stored length, byte offset
 * of its output in dst (a multiple of 8; dst itself 8-byte aligned) and the length D it must
 * inflate to.  Before any launch every range is checked to lie inside its buffer (SNPMI_E_INDEX)
 * and the dst ranges to be aligned and disjoint (SNPMI_E_ARG).  status: a HOST array of `streams`
 * words, filled before the call returns: 0, or why stream s was refused -- 1 bad zlib header,
 * 2 input exhausted, 3 reserved block type, 4 stored LEN / NLEN mismatch, 5 bad code-length set,
 * 6 invalid length or distance symbol, 7 distance beyond the bytes produced so far, 8 output would
 * exceed D, 9 stream ended with fewer than D bytes, 10 Adler-32 mismatch.  A refused stream never
 * reads outside its stored range nor writes outside its D bytes (whose content is then undefined),
 * and does not disturb the others.  Bytes behind the Adler-32 trailer are ignored, as
 * zlib.decompress ignores them.  streams == 0 launches nothing.  Synchronous. */
int snpmi_dev_inflate(const uint8_t* src, uint64_t src_bytes, uint8_t* dst, uint64_t dst_bytes, const uint64_t* table,
                      uint64_t streams, uint32_t* status);
/* What the host checks of an inflated layout-2 genotype block, read in device memory.  blocks:
 * device, 8-byte aligned; table: host, [blocks_n][2] = byte offset (a multiple of 8) and length of
 * each block, inside blocks_bytes (SNPMI_E_INDEX).  rec: HOST, [blocks_n][10] = 0, or 1 when the
 * block is shorter than 10 + n_samples bytes (then only N, K and the header ploidies are read, if
 * it has 8 bytes); the bit depth byte; the block's N; K; the header's min and max ploidy; min and
 * max of the low six bits of the n_samples ploidy bytes (255 and 0 when n_samples is 0); the phased
 * byte; 10 + n_samples + ceil(2 * bits * n_samples / 8).  Synchronous. */
int snpmi_dev_bgen_check(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* table, uint64_t blocks_n,
                         uint64_t n_samples, uint64_t* rec);
/* snpmi_dev_inflate's decoder on one stream in host memory: no device is touched.  *status as
 * above; dst[0, D) is written only.  For tests, fuzzing and sanitizer runs without a GPU. */
int snpmi_inflate_host(const uint8_t* src, uint64_t stored, uint8_t* dst, uint64_t D, uint32_t* status);
/* selected .bed columns (all iids) into a host buffer at `pitch` bytes per column (zero pad) --
 * the gather half of the file readers (bed.py:337-343), for the cfg5 plan's per-rank shares */
int snpmi_bed_gather_packed(const char* path, uint64_t n_iid, uint64_t n_sid, const uint64_t* sid_idx, uint64_t n_sel,
                            uint64_t pitch, uint8_t* dst, int num_threads);
/* per-SNP code counts -> stats [n_sid][2] (dtype) and value LUT [n_sid][4] (dtype) */
int snpmi_dev_snp_stats(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                        int count_a1, int std_kind, double a, double b, int use_stats, int dtype,
                        void* stats, void* lut);
/* packed + LUT -> values, column j at out + j*ld (F) or row i at out + i*ld (C) */
int snpmi_dev_decode(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                     const void* lut, int dtype, int order_c, void* out, uint64_t ld);
/* fused per-SNP stats + decode (f32, F order): one pass per column, LUT/stats written too */
int snpmi_dev_decode_standardize(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                                 int count_a1, int std_kind, double a, double b, int use_stats, int dtype,
                                 void* stats, void* lut, void* out, uint64_t ld);
/* values (dtype, F: column j at val + j*ld with ld % 16 == 0; C: row i at val + i*ld) -> packed
 * codes; *bad_values (if non-NULL; synchronises) = number of waves that saw a value outside
 * {0,1,2,missing} (0 = all valid) */
int snpmi_dev_encode(const void* val, int dtype, int order_c, uint64_t ld, uint64_t n_iid, uint64_t n_sid,
                     int count_a1, uint8_t* packed, uint64_t pitch, uint64_t* bad_values);
/* iid gather: dst column j = src column j restricted to iids idx[0..n_out) */
int snpmi_dev_repack(const uint8_t* src, uint64_t src_pitch, uint64_t n_src_iid, const uint64_t* idx,
                     uint64_t n_out_iid, uint64_t n_sid, uint8_t* dst, uint64_t dst_pitch);
/* Products of the standardized genotypes with tall matrices, straight from the packed codes:
 * Z[i, s] = lut[4 s + code(i, s)] (the LUT of snpmi_dev_snp_stats) is never written anywhere.
 *   snpmi_dev_packed_tdot:  G = Z^T V   (n_sid x k)
 *   snpmi_dev_packed_dot:   Y = Z W, or Y += Z W with accumulate != 0   (n_iid x k)
 * so K V = Z (Z^T V) takes two calls and no K.  The reference has no call site for these: its
 * callers use NumPy on SnpData.val (snps.val.T.dot(y)).
 * Layout: every pointer is a device pointer; lut is [n_sid][4] of dtype (f32 / f64); a tall matrix
 * with k columns is F order, column c at base + c * ld elements, ld >= its row count (V, Y: n_iid;
 * G, W: n_sid), so the G of one call is the W of the other.  Elements between the row count and ld
 * are neither read nor written.  k is any count: wider matrices are served in column panels.
 * Errors (SNPMI_E_ARG before any launch): an ld below the row count, pitch % 64 != 0, pitch <
 * ceil(n_iid / 4), another dtype.  n_iid == 0, n_sid == 0 or k == 0 launch nothing, except that the
 * dot with n_sid == 0 and accumulate == 0 writes zeros.
 * The calls run on the calling thread's stream and keep no state; their partial sums live in the
 * library's cached scratch (snpmi_release_cache).
 * iids: genotypes of iids >= n_iid are not added, whatever the unused codes of a column's last byte,
 * its pad bytes up to pitch and the LUT hold.
 * NaN: the products are IEEE FMAs, so a NaN LUT entry (the missing code under no standardization)
 * gives what NumPy gives: NaN in the tdot row of a SNP with a missing genotype and in every dot row
 * of an iid that has one, whatever V or W hold there; finite values everywhere else.
 * Determinism: no atomics, one fixed order per sum, the same bits on every run.
 *   tdot: a SNP's row depends on that SNP's codes, its LUT and V alone, not on the other SNPs of the
 *     call.  Per column a lane adds its 16 iids, a wave its 64 lanes, a workgroup its 4 waves (4096
 *     iids, in dtype); the 4096-iid chunks are then added in chunk order in f64 and rounded once.
 *   dot: the SNPs are cut into segments of 256 from the call's first SNP; a segment's sum p_j is one
 *     chain in dtype from zero, and Y = (((Y or 0) + p_0) + p_1) + ... in dtype, in segment order.
 *     The accumulate form starts that fold from the value Y holds, so calls over consecutive SNP
 *     chunks, each but the last a multiple of 256 SNPs, perform add by add the fold of one call over
 *     all of them: the same bits.  (Y is stored in dtype between calls, so the fold across segments
 *     cannot be kept in f64; in f32 a term passes through at most 256 + n_sid / 256 roundings, below
 *     the 16384 of the f32 GRM's chains up to 4.1 million SNPs.) */
int snpmi_dev_packed_tdot(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, const void* lut,
                          int dtype, const void* V, uint64_t ldv, uint64_t k, void* G, uint64_t ldg);
int snpmi_dev_packed_dot(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, const void* lut,
                         int dtype, const void* W, uint64_t ldw, uint64_t k, void* Y, uint64_t ldy, int accumulate);
/* SNP pairs straight from the packed codes: the value of pair (a, b) at iid i is
 *   Zp[i, (a, b)] = lut0[4 a + code0(i, a)] * lut1[4 b + code1(i, b)],
 * ONE IEEE multiply in dtype (f32 / f64) of two table entries (the LUTs of snpmi_dev_snp_stats), so
 * the value is defined bit for bit by the two tables.  These are the columns of the reference's
 * Pairs reader (snpreader/pairs.py:135-152), which multiplies two standardized SnpData on the host.
 *   snpmi_dev_pair_values:  the values of a pair list               (n_iid x n_pairs)
 *   snpmi_dev_pair_tdot:    G = Zp^T V over all pairs of two blocks (no pair column is written)
 * Layout: every pointer is a device pointer.  A side is packed codes [.][pitch] (4-byte aligned,
 * pitch % 64 == 0) with its table [.][4] of dtype; the two sides may be the same buffers, and may
 * have different pitches.
 * Errors (SNPMI_E_ARG before any launch, the output untouched): an ld that is too small (below),
 * pitch % 64 != 0, a pitch below ceil(n_iid / 4), another dtype.
 * Both run on the calling thread's stream and keep no state (not even scratch).
 * iids: genotypes of iids >= n_iid never reach an output, whatever the unused codes of a column's
 * last byte, its pad bytes up to pitch and the tables hold.
 * NaN: as NumPy's elementwise product -- a NaN table entry (the missing code under no
 * standardization) gives a NaN value whatever the other factor is, zero included; in the tdot a NaN
 * value gives NaN in every column of that pair's row, whatever V holds, and no other row.
 * Determinism: no atomics, one fixed order per sum, the same bits on every run.
 *
 * pair_values: out[i, c] = lut0[4 idx0[c] + code0(i, idx0[c])] * lut1[4 idx1[c] + code1(i, idx1[c])]
 * for c < n_pairs.  idx0 / idx1 index the SNPs of side 0 / side 1 (the caller keeps them inside its
 * buffers); they may repeat, be equal (a square) and come in any order.  F order (order_c == 0):
 * column c at out + c * ld elements, ld >= n_iid and ld % 16 == 0, out 16-byte aligned -- the rule
 * of snpmi_dev_decode, for the same 16-byte stores; C order: row i at out + i * ld, ld >= n_pairs.
 * Elements between the row count and ld are not written.  n_iid == 0 or n_pairs == 0 launches
 * nothing.
 *
 * pair_tdot: side a has n_a SNPs, side b n_b.  For every a < n_a and every b with b_lo[a] <= b < n_b
 *   G[row_off[a] + b, c] = sum_i Zp[i, (a, b)] V[i, c]        c < k
 * row_off == NULL means a * n_b, b_lo == NULL means 0; rows of G no (a, b) maps to are not written.
 * So a rectangle of a block pair lands in the reader's pair order, the triangular diagonal blocks
 * (b_lo skips b <= a, or b < a with singles) included, without a scatter pass.  row_off[a] + b may be
 * negative only for b < b_lo[a]: the caller guarantees that, and that every written row is below ldg.
 * V (n_iid rows, ldv >= n_iid) and G are F-order tall matrices as in snpmi_dev_packed_tdot: column c
 * at base + c * ld elements.  With row_off == NULL, ldg >= n_a * n_b (else SNPMI_E_ARG).  k is any
 * count, served in column panels of 4 / 2 / 1 (f32) or 2 / 1 (f64).  n_a, n_b or k == 0 launch
 * nothing; n_iid == 0 writes zeros to the rows the call owns.
 * Summation: the pair's value is rounded in dtype first (it equals what pair_values writes) and is
 * then multiplied into V by FMA.  Per column a lane adds its 16 iids, a wave its 64 lanes, a
 * workgroup its 4 waves (4096 iids, in dtype); the 4096-iid chunks are then added in chunk order in
 * f64 and rounded once -- the scheme of snpmi_dev_packed_tdot.  A pair's row depends on its two
 * SNPs, their tables and V alone: not on the rectangle, on its neighbours or on the tile (8 x 32
 * SNPs per workgroup) it fell into. */
int snpmi_dev_pair_values(const uint8_t* packed0, uint64_t pitch0, const void* lut0, const uint8_t* packed1,
                          uint64_t pitch1, const void* lut1, uint64_t n_iid, const uint32_t* idx0,
                          const uint32_t* idx1, uint64_t n_pairs, int dtype, int order_c, void* out, uint64_t ld);
int snpmi_dev_pair_tdot(const uint8_t* packed_a, uint64_t pitch_a, const void* lut_a, uint64_t n_a,
                        const uint8_t* packed_b, uint64_t pitch_b, const void* lut_b, uint64_t n_b, uint64_t n_iid,
                        const int64_t* row_off, const uint32_t* b_lo, int dtype, const void* V, uint64_t ldv,
                        uint64_t k, void* G, uint64_t ldg);
/* GRM tiles: K_tiles holds the upper-triangle 128x128 tiles of an n x n K
 * (snpmi_grm_tile_bytes); accumulate != 0 adds to it. */
uint64_t snpmi_grm_tile_bytes(uint64_t n_iid, int dtype);
int snpmi_dev_syrk_packed(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                          const void* lut, int dtype, void* K_tiles, int accumulate);
/* Rect GRM: K[rows, cols] = Z[rows] Z[cols]^T computed directly, without the whole K -- the
 * test x train kernel of SnpKernel(snps, std)[test_idx, train_idx].read(), which the reference
 * slices out of the N x N K (kernelreader/snpkernel.py:84-88, "could be done with less memory by
 * working in blocks").  The result is held as ceil(n_rows/256) x ceil(n_cols/256) dense row-major
 * 256x256 blocks, block (bi, bj) at slot bj * ceil(n_rows/256) + bi (snpmi_grm_rect_bytes).
 * Limits (SNPMI_E_ARG before any launch): < 65536 blocks per side, < 2^29 blocks, each operand's
 * pitch % 64 == 0 and covering round_up(n, 256) iids.
 * snpmi_dev_syrk_rect: one launch over two packed device operands (same SNP rows, same LUT
 * [n_sid][4] of dtype); pairs (host, n_pairs x (r, c), may be NULL): positions that are diagonal
 * elements of K, which in f32 get the exact f64 diagonal as the whole-K path's do
 * (snpmi_rect_diag_pairs builds the list from two index lists, NULL = identity; it needs no device).
 * snpmi_dev_rect_extract: blocks -> K_out[n_rows][n_cols] (order_c 0/1, times scale; host or device). */
uint64_t snpmi_grm_rect_bytes(uint64_t n_rows, uint64_t n_cols, int dtype);
int snpmi_rect_diag_pairs(const uint64_t* row_idx, uint64_t n_rows, const uint64_t* col_idx, uint64_t n_cols,
                          uint32_t* pairs, uint64_t cap, uint64_t* count);
int snpmi_dev_syrk_rect(const uint8_t* packed_a, uint64_t pitch_a, uint64_t n_a, const uint8_t* packed_b,
                        uint64_t pitch_b, uint64_t n_b, uint64_t n_sid, const void* lut, int dtype, void* blocks,
                        int accumulate, const uint32_t* pairs, uint64_t n_pairs);
int snpmi_dev_rect_extract(const void* blocks, uint64_t n_rows, uint64_t n_cols, int dtype, int order_c, double scale,
                           void* K_out);
/* Rect session (beside snpmi_grm_begin / add / end): begin(n_rows, n_cols, dtype), any number of
 * adds, end(scale, order_c, K_out; host or device, NULL = abort).  Every add standardizes with
 * stats over ALL n_iid (add_bed: all n_out_iid selected) iids of the reader -- what
 * SnpKernel(reader, std)[rows, cols] means -- and then takes rows row_idx / cols col_idx of them
 * (host arrays, unsorted and repeated entries allowed, an entry >= n is SNPMI_E_INDEX; NULL = all
 * iids in order, read in place without a repack).  add_packed: device codes as
 * snpmi_grm_add_packed_*; add_bed: arguments as snpmi_grm_add_bed_*, the same SNP chunks. */
int snpmi_grm_rect_begin(uint64_t n_rows, uint64_t n_cols, int dtype);
int snpmi_grm_rect_add_packed_f32(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, int count_a1,
                                  int std_kind, double a, double b, int use_stats, float* stats,
                                  const uint64_t* row_idx, const uint64_t* col_idx);
int snpmi_grm_rect_add_packed_f64(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, int count_a1,
                                  int std_kind, double a, double b, int use_stats, double* stats,
                                  const uint64_t* row_idx, const uint64_t* col_idx);
int snpmi_grm_rect_add_bed_f32(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1, const uint64_t* iid_idx,
                               uint64_t n_out_iid, const uint64_t* sid_idx, uint64_t n_out_sid, int std_kind, double a,
                               double b, int use_stats, float* stats, int num_threads, const uint64_t* row_idx,
                               const uint64_t* col_idx);
int snpmi_grm_rect_add_bed_f64(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1, const uint64_t* iid_idx,
                               uint64_t n_out_iid, const uint64_t* sid_idx, uint64_t n_out_sid, int std_kind, double a,
                               double b, int use_stats, double* stats, int num_threads, const uint64_t* row_idx,
                               const uint64_t* col_idx);
int snpmi_grm_rect_end(double scale, int order_c, void* K_out);
/* cfg5 mode (K too large to replicate): the upper triangle of the n x n K as 256x256
 * blocks, grouped into S x S-block supertiles (S = 16 once there are >= 4 supertiles per part,
 * else the largest power of two that gives as many) dealt round-robin in triangular supertile
 * order: supertile T = J(J+1)/2 + I belongs to part T mod part_world.  Part `part_rank` stores its
 * n_local blocks densely, each a full row-major 256x256 f32 block at blocks + b*65536, in its
 * walk order (its supertiles in T order, inside each block column by block column);
 * snpmi_grm_part_coords gives block b's (row0, col0), snpmi_grm_part_coords_all all of them
 * ([n_local][2]).  Every rank reads all SNPs; no reduction is needed.  The K sub-matrices the
 * reference's KernelReader serves (kernelreader.py:245-302) are read back from these blocks. */
uint64_t snpmi_grm_part_blocks(uint64_t n_iid, int part_rank, int part_world);
int snpmi_grm_part_coords(uint64_t n_iid, int part_rank, int part_world, uint64_t local_block,
                          uint64_t* row0, uint64_t* col0);
int snpmi_grm_part_coords_all(uint64_t n_iid, int part_rank, int part_world, uint64_t* coords);
int snpmi_dev_syrk_packed_part(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                               const void* lut, int part_rank, int part_world, void* blocks, int accumulate);
/* the same in float64 (the reference's default GRM dtype, snpreader.py:528,623): f64 LUT [n_sid][4],
 * blocks of 256x256 f64; computed on the int8 MFMA as exact residue products + CRT */
int snpmi_dev_syrk_packed_part_f64(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                                   const double* lut, int part_rank, int part_world, double* blocks, int accumulate);
/* cfg5 from a .bed file (SnpReader._read_kernel, snpreader.py:623-668, with K partitioned as
 * above): this rank streams every selected SNP, standardizes it with stats over all selected
 * iids (stats in/out as snpmi_grm_bed_f32), accumulates only its own blocks and writes them to
 * blocks_out[snpmi_grm_part_blocks][256][256] (rows/cols past n are padding).  blocks_out may be
 * host memory (copied out at the end) or device memory (accumulated in place: K stays in HBM). */
int snpmi_grm_part_bed_f32(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                           const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx, uint64_t n_out_sid,
                           int std_kind, double a, double b, int use_stats, float* stats, int part_rank,
                           int part_world, float* blocks_out, int num_threads);
int snpmi_grm_part_bed_f64(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1,
                           const uint64_t* iid_idx, uint64_t n_out_iid, const uint64_t* sid_idx, uint64_t n_out_sid,
                           int std_kind, double a, double b, int use_stats, double* stats, int part_rank,
                           int part_world, double* blocks_out, int num_threads);
/* K[ri[r], ci[c]] (ri/ci host arrays, NULL = identity; order_c: out row-major) restricted to the
 * blocks part `part_rank` owns, 0 elsewhere, times `scale` (DiagKtoN) -- summed over the parts the
 * sub-matrix; out host or device.  The reader of a partitioned K (shard.PartitionedKernel, the
 * KernelReader._read of kernelreader.py:245-302 / snpkernel.py:78-101 for a K that is not
 * replicated).  IndexError for indices >= n. */
int snpmi_grm_part_extract_f32(const float* blocks, uint64_t n_iid, int part_rank, int part_world, const uint64_t* ri,
                               uint64_t nr, const uint64_t* ci, uint64_t nc, int order_c, double scale, float* out);
int snpmi_grm_part_extract_f64(const double* blocks, uint64_t n_iid, int part_rank, int part_world, const uint64_t* ri,
                               uint64_t nr, const uint64_t* ci, uint64_t nc, int order_c, double scale, double* out);
/* this part's share of trace(K) (DiagKtoN over a partitioned K, diag_K_to_N.py:54-59) */
int snpmi_grm_part_trace_f32(const float* blocks, uint64_t n_iid, int part_rank, int part_world, double* trace);
int snpmi_grm_part_trace_f64(const double* blocks, uint64_t n_iid, int part_rank, int part_world, double* trace);
/* free / total HBM of the current device (hipMemGetInfo): whether a replicated K fits */
int snpmi_device_memory(uint64_t* free_bytes, uint64_t* total_bytes);
/* K_tiles (+)= Z Z^T of a dense device operand: Z is [n_sid][ldz] of dtype, F order (column s, one
 * SNP, at Z + s * ldz; its first n_iid rows are the values).  ldz % 4 == 0, and ldz >=
 * round_up(n_iid, 256) for f32 at n_iid >= 4096, ldz >= round_up(n_iid, 128) otherwise: the kernels
 * read whole iid panels.  Rows n_iid..ldz-1 must be readable; their contents (NaN included) never
 * reach K[0..n_iid) and never move the fp16 range check.  K_tiles: snpmi_grm_tile_bytes(n_iid,
 * dtype); accumulate != 0 adds to it, 0 overwrites it (n_sid == 0: zeroes it). */
int snpmi_dev_syrk_dense(const void* Z, uint64_t ldz, uint64_t n_iid, uint64_t n_sid, int dtype,
                         void* K_tiles, int accumulate);
/* tiles -> K[ri[r], ci[c]] (ri/ci NULL = identity), scaled by `scale` */
int snpmi_dev_grm_extract(const void* K_tiles, uint64_t n_iid, int dtype, const uint64_t* ri, uint64_t nr,
                          const uint64_t* ci, uint64_t nc, int order_c, double scale, void* out);
int snpmi_dev_grm_trace(const void* K_tiles, uint64_t n_iid, int dtype, double* trace);
/* float64 GRMs run on the int8 MFMA as residues modulo the first R of 15 coprime moduli, R chosen
 * per SNP block on the device from the block's own bound max_i sum_s q_is^2:
 * sum of R and number of such blocks on this device since the last reset (synchronous). */
int snpmi_crt_moduli_stats(uint64_t* sum_r, uint64_t* launches, int reset);
/* per 256-block: each block (bi, bj) runs only the moduli with P_R > 2 sqrt(M_bi M_bj), M_p = the
 * largest sum_s q_is^2 of its iid panel p (Cauchy-Schwarz per block; K is the same bits as with the
 * launch-wide R): sum of R_b and number of blocks since the last reset (synchronous). */
int snpmi_crt_block_moduli_stats(uint64_t* sum_rb, uint64_t* blocks, int reset);

/* ---------------------------------------------------------------- RCCL (one process per GPU) */
int snpmi_rccl_unique_id(uint8_t* id, uint64_t id_len);   /* id_len >= 128 */
int snpmi_rccl_init(int nranks, int rank, const uint8_t* id, uint64_t id_len);
int snpmi_rccl_allreduce_sum(void* buf, uint64_t count, int dtype);
/* In-place sum of the K tiles onto rank `root` only (the caller of read_kernel holds K:
 * snpreader.py:623-668 returns K to its one process); ncclReduce moves half the bytes of the
 * all-reduce over xGMI.  buf on non-root ranks is left unspecified. */
int snpmi_rccl_reduce_sum(void* buf, uint64_t count, int dtype, int root);
/* cfg5: every rank contributes bytes_per_rank bytes; recv gets them concatenated in rank
 * order (send may alias recv + rank * bytes_per_rank) */
int snpmi_rccl_allgather(const void* send, void* recv, uint64_t bytes_per_rank);
/* host-value all-reduce (op 0 = sum, 1 = max) of f64 scalars, synchronous; barrier = 1-elem sum */
int snpmi_rccl_host_allreduce_f64(double* values, uint64_t count, int op);
int snpmi_rccl_barrier(void);
int snpmi_rccl_comm_count(int* count);                    /* ncclCommCount: ranks in the communicator */
int snpmi_rccl_destroy(void);
/* Collective trace of this process (lock-free; callable from another thread while one sits in a
 * collective): out[0..11] = calls, all-reduces, reduces, all-gathers, host all-reduces (barriers /
 * max), bytes enqueued, signature of the (kind, count, root) sequence (FNV-1a: the same calls in the
 * same order give the same value on every rank), last kind (1 all-reduce, 2 reduce, 3 all-gather,
 * 4 host), last count, 1 while inside a blocking host all-reduce, completed host all-reduces,
 * communicator present.  n = entries wanted (<= 12). */
int snpmi_rccl_trace(uint64_t* out, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif /* SNPMI_H */
