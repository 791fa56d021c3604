// libsnpmi C ABI (include/snpmi.h): host orchestration of the BED -> GRM path on one GPU.
//
// Data flow of every file-backed entry point (one SNP chunk at a time):
//   mmap(.bed) --gather selected columns, pitch-padded--> pinned host buffer
//     --H2D--> packed codes in HBM --[k_repack: iid subset]--> k_snp_stats (stats + LUT)
//     --> k_decode_f/c (values)  or  MFMA SYRK into upper-triangle K tiles
//     --> D2H into the caller's NumPy buffer.
// The packed codes are 16x (f32) / 32x (f64) smaller than the values, so only packed bytes
// cross PCIe on the way in.
#include <fcntl.h>
#include <immintrin.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <vector>

#include "snpmi_internal.hpp"

#include <type_traits>

namespace snpmi {

// ====================================================================== errors / devices
static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }

static std::mutex g_dev_mutex;
static std::vector<Device*> g_devices;
static thread_local int g_cur_dev = -1;

static int default_device() {
    const char* e = std::getenv("PST_DEVICE");
    return e ? std::atoi(e) : 0;
}

static int num_devices() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

Device& device() {
    if (g_cur_dev < 0) g_cur_dev = default_device();
    std::lock_guard<std::mutex> lk(g_dev_mutex);
    const int n = num_devices();
    SNPMI_REQUIRE(n > 0, SNPMI_E_HIP, "no HIP device available (libsnpmi has no CPU fallback)");
    SNPMI_REQUIRE(g_cur_dev < n, SNPMI_E_ARG, "device index out of range");
    if ((int)g_devices.size() < n) g_devices.resize(n, nullptr);
    Device*& d = g_devices[g_cur_dev];
    SNPMI_HIP(hipSetDevice(g_cur_dev));
    if (!d) {
        d = new Device();
        d->id = g_cur_dev;
        SNPMI_HIP(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        SNPMI_HIP(hipStreamCreateWithFlags(&d->copy, hipStreamNonBlocking));
        SNPMI_HIP(hipStreamCreateWithFlags(&d->aux, hipStreamNonBlocking));
        for (hipEvent_t* set : {d->staged, d->consumed, d->produced, d->bounce})
            for (int s = 0; s < 2; s++) SNPMI_HIP(hipEventCreateWithFlags(&set[s], hipEventDisableTiming));
        for (int s = 0; s < kPieces; s++) SNPMI_HIP(hipEventCreateWithFlags(&d->piece[s], hipEventDisableTiming));
        SNPMI_HIP(hipEventCreateWithFlags(&d->fence, hipEventDisableTiming));
        hipDeviceProp_t p;
        SNPMI_HIP(hipGetDeviceProperties(&p, g_cur_dev));
        d->cu_count = p.multiProcessorCount;
    }
    return *d;
}

static thread_local int g_sel_stream = 0;  // snpmi_set_stream: 0 compute, 2 aux

hipStream_t stream() {
    Device& d = device();
    return g_sel_stream == 2 ? d.aux : d.stream;
}

void* Device::get(Slot s, size_t bytes) {
    if (bytes == 0) bytes = 256;
    if (cap[s] < bytes) {
        if (buf[s]) SNPMI_HIP(hipFree(buf[s]));
        buf[s] = nullptr;
        cap[s] = 0;
        size_t want = round_up(bytes, 1 << 20);
        if (hipMalloc(&buf[s], want) != hipSuccess) {
            (void)hipGetLastError();
            buf[s] = nullptr;
            throw Error(SNPMI_E_NOMEM, "hipMalloc of " + std::to_string(want) + " bytes failed");
        }
        cap[s] = want;
    }
    return buf[s];
}

void Device::release() {
    for (int s = 0; s < S_NUM; s++) {
        if (buf[s]) (void)hipFree(buf[s]);
        buf[s] = nullptr;
        cap[s] = 0;
    }
    for (int x = 0; x < 2; x++) {
        if (order_tab[x]) (void)hipFree(order_tab[x]);
        order_tab[x] = nullptr;
        order_nb[x] = 0;
    }
    if (part_tab) (void)hipFree(part_tab);
    part_tab = nullptr;
    for (int i = 0; i < 3; i++) part_key[i] = 0;
}

// pinned staging (two slots so a chunk can be gathered while the previous one uploads)
static std::mutex g_pin_mutex;
constexpr int kPinSlots = 6 + kPieces;  // 0: encoder, 2: stats, 4/5: D2H bounce, 6..: H2D piece ring
static void* g_pin[kPinSlots] = {};
static size_t g_pin_cap[kPinSlots] = {};

void* pinned(int slot, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_pin_mutex);
    if (g_pin_cap[slot] < bytes) {
        if (g_pin[slot]) (void)hipHostFree(g_pin[slot]);
        g_pin[slot] = nullptr;
        g_pin_cap[slot] = 0;
        size_t want = round_up(bytes, 1 << 20);
        if (hipHostMalloc(&g_pin[slot], want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            throw Error(SNPMI_E_NOMEM, "pinned allocation failed");
        }
        g_pin_cap[slot] = want;
    }
    return g_pin[slot];
}

void release_pinned() {
    std::lock_guard<std::mutex> lk(g_pin_mutex);
    for (int s = 0; s < kPinSlots; s++) {
        if (g_pin[s]) (void)hipHostFree(g_pin[s]);
        g_pin[s] = nullptr;
        g_pin_cap[s] = 0;
    }
}

// one API call at a time per process: scratch slots and the stream are shared
static std::recursive_mutex g_call_mutex;
std::recursive_mutex& call_mutex() { return g_call_mutex; }

// ====================================================================== host helpers
static int resolve_threads(int num_threads) {
    if (num_threads > 0) return std::min(num_threads, 64);
    unsigned hc = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(hc, 16u));
}

template <class F>
static void parallel_for(uint64_t n, int nthreads, F&& fn, uint64_t grain = 64) {
    if (n == 0) return;
    nthreads = (int)std::min<uint64_t>((uint64_t)nthreads, n);
    if (nthreads <= 1 || n < grain) {
        for (uint64_t i = 0; i < n; i++) fn(i);
        return;
    }
    std::atomic<uint64_t> next(0);
    std::vector<std::thread> th;
    th.reserve(nthreads);
    for (int t = 0; t < nthreads; t++)
        th.emplace_back([&] {
            for (;;) {
                uint64_t s = next.fetch_add(grain);
                if (s >= n) break;
                uint64_t e = std::min(n, s + grain);
                for (uint64_t i = s; i < e; i++) fn(i);
            }
        });
    for (auto& t : th) t.join();
}

// Device -> pageable host copy of `rows` rows of `width` bytes (device pitch spitch, host
// pitch dpitch) on the COPY stream, ordered after the compute stream's work so far (or after
// `after`).  A plain hipMemcpy to pageable memory runs at ~16 GB/s (the runtime's own bounce +
// a single-threaded copy); here 256 MiB pieces DMA into two pinned bounce buffers while host
// threads copy the previous piece out, so PCIe and the host copy overlap -- and, because the
// DMA sits on its own stream, kernels enqueued before this call keep running beside it.
static void d2h_rows(Device& d, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows,
                     int nthreads, hipEvent_t after = nullptr) {
    if (rows == 0 || width == 0) return;
    if (!after) {
        SNPMI_HIP(hipEventRecord(d.fence, d.stream));
        after = d.fence;
    }
    SNPMI_HIP(hipStreamWaitEvent(d.copy, after, 0));
    const size_t total = width * rows;
    if (total < (32u << 20)) {
        SNPMI_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToHost, d.copy));
        SNPMI_HIP(hipStreamSynchronize(d.copy));
        return;
    }
    const size_t per = std::max<size_t>(1, (256u << 20) / width);
    uint8_t* bounce[2] = {(uint8_t*)pinned(4, per * width), (uint8_t*)pinned(5, per * width)};
    hipEvent_t* ev = d.bounce;
    auto drain = [&](size_t r0, size_t nr, int slot) {
        SNPMI_HIP(hipEventSynchronize(ev[slot]));
        const uint8_t* b = bounce[slot];
        uint8_t* o = (uint8_t*)dst + r0 * dpitch;
        if (dpitch == width) {
            const size_t bytes = nr * width, per_t = round_up(ceil_div(bytes, (size_t)nthreads), 4096);
            parallel_for(
                ceil_div(bytes, per_t), nthreads,
                [&](uint64_t q) {
                    const size_t a = q * per_t, e = std::min(bytes, a + per_t);
                    std::memcpy(o + a, b + a, e - a);
                },
                1);
        } else {
            parallel_for(
                nr, nthreads, [&](uint64_t r) { std::memcpy(o + r * dpitch, b + r * width, width); },
                std::max<uint64_t>(1, (1u << 20) / width));
        }
    };
    size_t prev_r0 = 0, prev_n = 0;
    int i = 0;
    for (size_t r0 = 0; r0 < rows; r0 += per, i++) {
        const size_t nr = std::min(per, rows - r0);
        const int slot = i & 1;
        SNPMI_HIP(hipMemcpy2DAsync(bounce[slot], width, (const uint8_t*)src + r0 * spitch, spitch, width, nr,
                                   hipMemcpyDeviceToHost, d.copy));
        SNPMI_HIP(hipEventRecord(ev[slot], d.copy));
        if (i > 0) drain(prev_r0, prev_n, slot ^ 1);
        prev_r0 = r0;
        prev_n = nr;
    }
    drain(prev_r0, prev_n, (i - 1) & 1);
}

// contiguous byte range as rows of 4 MiB (+ a tail) through the pipelined copy above.  (The
// same bounce for host->device measured no faster than the runtime's pageable H2D: the
// source pages are already resident, while a D2H into fresh NumPy memory pays page faults
// that the threaded copy-out spreads over cores.)
static void d2h_bytes(Device& d, void* dst, const void* src, size_t bytes, int nthreads) {
    const size_t w = 4u << 20, rows = bytes / w, tail = bytes - rows * w;
    d2h_rows(d, dst, w, src, w, w, rows, nthreads);
    if (tail) d2h_rows(d, (uint8_t*)dst + rows * w, tail, (const uint8_t*)src + rows * w, tail, tail, 1, nthreads);
}

struct BedMap {
    int fd = -1;
    const uint8_t* base = nullptr;
    size_t size = 0;
    uint64_t bpc = 0;
    ~BedMap() {
        // unmapping a page-cache mapping of a few GB tears down ~1M page-table entries (~4 ms at
        // 1.25 GB, measured between the last SYRK and the K extraction, profiles/r03h): every
        // gather from it has returned, so a large mapping goes away off the call's critical path
        if (base && size >= (64u << 20)) {
            std::thread([p = (void*)base, n = size] { munmap(p, n); }).detach();
        } else if (base) {
            munmap((void*)base, size);
        }
        if (fd >= 0) close(fd);
    }
    const uint8_t* column(uint64_t s) const { return base + 3 + s * bpc; }
};

// bed-reader's open_bed format check (magic 6C 1B 01 = SNP-major) + size check.
static void open_bed(BedMap& m, const char* path, uint64_t n_iid, uint64_t n_sid) {
    SNPMI_REQUIRE(path != nullptr, SNPMI_E_ARG, "path is NULL");
    m.fd = open(path, O_RDONLY);
    SNPMI_REQUIRE(m.fd >= 0, SNPMI_E_IO, std::string("cannot open ") + path);
    struct stat st;
    SNPMI_REQUIRE(fstat(m.fd, &st) == 0, SNPMI_E_IO, std::string("cannot stat ") + path);
    m.size = (size_t)st.st_size;
    m.bpc = ceil_div(n_iid, 4);
    SNPMI_REQUIRE(m.size >= 3, SNPMI_E_FORMAT, std::string("file too short to be a .bed file: ") + path);
    void* p = mmap(nullptr, m.size, PROT_READ, MAP_SHARED, m.fd, 0);
    SNPMI_REQUIRE(p != MAP_FAILED, SNPMI_E_IO, std::string("mmap failed: ") + path);
    m.base = (const uint8_t*)p;
    SNPMI_REQUIRE(m.base[0] == 0x6C && m.base[1] == 0x1B, SNPMI_E_FORMAT,
                  std::string("not a PLINK .bed file (bad magic): ") + path);
    SNPMI_REQUIRE(m.base[2] == 0x01, SNPMI_E_FORMAT,
                  std::string("only SNP-major .bed files are supported: ") + path);
    SNPMI_REQUIRE(m.size == 3 + n_sid * m.bpc, SNPMI_E_FORMAT,
                  std::string(".bed size does not match .fam/.bim counts: ") + path);
    (void)madvise(p, m.size, MADV_SEQUENTIAL);
}

static void check_index(const uint64_t* idx, uint64_t n, uint64_t bound, const char* what) {
    if (!idx) return;
    for (uint64_t i = 0; i < n; i++)
        SNPMI_REQUIRE(idx[i] < bound, SNPMI_E_INDEX,
                      std::string(what) + " index " + std::to_string(idx[i]) + " out of range (count " +
                          std::to_string(bound) + ")");
}

// The .bed selection block from the ABI's loose arguments: the only place where "a NULL index list
// selects everything" becomes a count.
static BedSel bed_sel(const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1, const uint64_t* iid_idx,
                      uint64_t n_out_iid, const uint64_t* sid_idx, uint64_t n_out_sid, int num_threads) {
    return {path, n_iid, n_sid, count_a1, iid_idx, sid_idx, num_threads,
            iid_idx ? n_out_iid : n_iid, sid_idx ? n_out_sid : n_sid};
}
// open the selection's file and range-check its index lists
static void open_sel(BedMap& m, const BedSel& s) {
    open_bed(m, s.path, s.n_iid, s.n_sid);
    check_index(s.iid_idx, s.n_out, s.n_iid, "iid");
    check_index(s.sid_idx, s.m_out, s.n_sid, "sid");
}

static bool is_identity(const uint64_t* idx, uint64_t n, uint64_t bound) {
    if (!idx) return true;
    if (n != bound) return false;
    for (uint64_t i = 0; i < n; i++)
        if (idx[i] != i) return false;
    return true;
}

// Gather SNP columns [c0, c0+cnt) of the selection into `dst` with `pitch` bytes each.
// g_gather 0 (default): memcpy from the mmap; 1: pread() per column into the pinned piece.  A/B on
// a 50k x 100k file in the page cache (tools/exp_gather.py, profiles/r03j): the full 1.25 GB read
// into HBM at 37-47 GB/s of packed codes with the mmap vs 32-35 GB/s with pread, so the mmap stays
static int g_gather = 0;
static void gather_columns(const BedMap& m, const uint64_t* sid_idx, uint64_t c0, uint64_t cnt, uint64_t pitch,
                           uint8_t* dst, int nthreads) {
    const bool use_pread = g_gather == 1;
    parallel_for(cnt, nthreads, [&](uint64_t j) {
        const uint64_t s = sid_idx ? sid_idx[c0 + j] : c0 + j;
        uint8_t* d = dst + j * pitch;
        if (use_pread) {
            size_t got = 0;
            while (got < m.bpc) {
                const ssize_t r = pread(m.fd, d + got, m.bpc - got, (off_t)(3 + s * m.bpc + got));
                if (r <= 0) break;
                got += (size_t)r;
            }
            if (got < m.bpc) std::memcpy(d + got, m.column(s) + got, m.bpc - got);  // short read: the mapping
        } else {
            std::memcpy(d, m.column(s), m.bpc);
        }
        if (pitch > m.bpc) std::memset(d + m.bpc, 0, pitch - m.bpc);
    });
}

// Device-side iid selection state for one call.
struct IidPlan {
    uint64_t n_in, n_out, pitch_in, pitch_out;
    bool repack;
    uint64_t* idx_dev = nullptr;
    RepackPlan plan;                // gather plan of k_repack_lds / k_repack_win
};

static IidPlan plan_iids(Device& d, const BedSel& s) {
    IidPlan p;
    p.n_in = s.n_iid;
    p.n_out = s.n_out;
    p.pitch_in = packed_pitch(s.n_iid);
    p.pitch_out = packed_pitch(p.n_out);
    p.repack = !is_identity(s.iid_idx, p.n_out, s.n_iid);
    if (p.repack && p.n_out) {
        p.idx_dev = (uint64_t*)d.get(Device::S_IDX, p.n_out * 8);
        SNPMI_HIP(hipMemcpyAsync(p.idx_dev, s.iid_idx, p.n_out * 8, hipMemcpyHostToDevice, d.stream));
        uint32_t* plan = (uint32_t*)d.get(Device::S_IDX32, repack_plan_entries(p.n_out) * 4);
        uint32_t* win = (uint32_t*)d.get(Device::S_WIN, repack_win_entries(p.n_out) * 4);
        p.plan = launch_repack_plan(p.idx_dev, p.n_out, p.n_in, plan, win, d.stream);
    }
    return p;
}

// Upload SNP chunk [c0, c0+cnt) and return the device packed buffer for the selected iids.
// Chunks alternate between two device buffers (slot = chunk parity).  The H2D runs on the copy
// stream: it waits only for the kernels that last read this device slot (chunk c-2, event
// `consumed`), so the upload of chunk c overlaps the kernels of chunk c-1.  The compute stream
// waits on `staged` before touching the chunk.  Callers record consumed[slot] on the compute
// stream after the chunk's last kernel (chunk_done).
//
// The host side goes through a ring of kPieces pinned pieces of <= kPieceBytes (not one pinned
// buffer per chunk): the host gathers piece q+1 from the mmap while piece q crosses PCIe, and
// only 4 x 32 MiB is ever pinned -- a first call no longer pays for pinning two chunk-sized
// buffers (~0.5 GB at 50k iids), and ranks sharing a host hold less locked memory.  The host
// blocks only when the ring is full, i.e. until chunk c-2's kernels are done.
static const uint8_t* stage_chunk(Device& d, const BedMap& m, const uint64_t* sid_idx, uint64_t c0, uint64_t cnt,
                                  const IidPlan& p, int nthreads, int slot) {
    uint8_t* dev = (uint8_t*)d.get(slot ? Device::S_PACKED_B : Device::S_PACKED, cnt * p.pitch_in);
    SNPMI_HIP(hipStreamWaitEvent(d.copy, d.consumed[slot], 0));
    const uint64_t per = std::max<uint64_t>(1, kPieceBytes / p.pitch_in);
    for (uint64_t q0 = 0; q0 < cnt; q0 += per) {
        const uint64_t qn = std::min(per, cnt - q0);
        const int ps = (int)(d.piece_next++ % kPieces);
        SNPMI_HIP(hipEventSynchronize(d.piece[ps]));  // this pinned piece's previous H2D has finished
        uint8_t* host = (uint8_t*)pinned(6 + ps, std::min(cnt, per) * p.pitch_in);
        gather_columns(m, sid_idx, c0 + q0, qn, p.pitch_in, host, nthreads);
        SNPMI_HIP(hipMemcpyAsync(dev + q0 * p.pitch_in, host, qn * p.pitch_in, hipMemcpyHostToDevice, d.copy));
        SNPMI_HIP(hipEventRecord(d.piece[ps], d.copy));
    }
    SNPMI_HIP(hipEventRecord(d.staged[slot], d.copy));
    SNPMI_HIP(hipStreamWaitEvent(d.stream, d.staged[slot], 0));
    if (!p.repack) return dev;
    uint8_t* dev2 = (uint8_t*)d.get(Device::S_PACKED2, cnt * p.pitch_out);
    launch_repack(dev, p.pitch_in, p.n_in, p.idx_dev, p.plan, p.n_out, cnt, dev2, p.pitch_out, d.stream);
    return dev2;
}

static void chunk_done(Device& d, int slot) { SNPMI_HIP(hipEventRecord(d.consumed[slot], d.stream)); }

// Value / K buffers may be HOST or DEVICE memory (unified virtual addressing): a pointer into a
// snpmi_dev_alloc / hipMalloc allocation of the current device is computed on in place or
// written directly, without the host staging -- the device-resident SnpData / KernelData of
// pysnptools_amd.hbm (the reference's array-module seam, util/__init__.py:652-730).  Stats
// arrays stay host memory.
bool is_device_ptr(Device& d, const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable host memory is unknown to HIP
        return false;
    }
    if (at.type != hipMemoryTypeDevice) return false;
    SNPMI_REQUIRE(at.device == d.id, SNPMI_E_ARG,
                  "device buffer belongs to device " + std::to_string(at.device) + ", the call runs on device " +
                      std::to_string(d.id));
    return true;
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
template <>
struct DT<int8_t> {
    static constexpr int v = SNPMI_DT_I8;
};

static uint64_t chunk_snps(uint64_t per_snp_bytes, uint64_t budget = 1ull << 30) {
    uint64_t c = std::max<uint64_t>(1, budget / std::max<uint64_t>(per_snp_bytes, 1));
    return std::min<uint64_t>(c, 1ull << 16);
}

// ====================================================================== BED read (+ standardize)
// out_optional: the caller's own output counts (n_out_iid, n_out_sid, whatever the index lists) hold a 0
template <typename T>
static void bed_read_impl(const BedSel& s, int order_c, const StdArgs& sa, T* stats, T* out, bool out_optional) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    SNPMI_REQUIRE(out != nullptr || out_optional, SNPMI_E_ARG, "out is NULL");
    BedMap m;
    open_sel(m, s);
    const uint64_t n_out = s.n_out, m_out = s.m_out;
    if (m_out == 0) return;
    Device& d = device();
    const int nthreads = resolve_threads(s.num_threads);
    IidPlan p = plan_iids(d, s);
    const int dt = DT<T>::v;
    const bool dev_out = is_device_ptr(d, out);
    // device output: decode straight into it when its columns (F) meet the 16-B vector-store
    // alignment of k_decode_f, else through the block buffer + a device-to-device copy; C order
    // always straight (k_decode_c_reg checks alignment itself, k_decode_c has none)
    const bool direct = dev_out && (order_c || (reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
                                                (n_out * sizeof(T)) % 16 == 0));
    const uint64_t ldF = round_up(std::max<uint64_t>(n_out, 1), 16);
    const uint64_t C = chunk_snps(p.pitch_in + p.pitch_out + ldF * sizeof(T));
    const bool stats_out = sa.kind != SNPMI_STD_NONE && !sa.use_stats;
    // Three-stage pipeline over SNP chunks, two slots each: host gather + H2D (copy stream) of
    // chunk c, stats + decode of chunk c (compute stream), D2H + host copy-out of chunk c-1 (copy
    // stream, after `produced`).  PCIe runs both directions at once and the kernels of chunk c
    // hide under the copy-out of chunk c-1.
    struct Pending {
        uint64_t c0 = 0, cnt = 0, ldc = 0;
        int slot = 0;
        T* dev_out = nullptr;
        T* st_dev = nullptr;
        bool valid = false;
    } pending;
    auto drain = [&](const Pending& q) {
        if (n_out > 0 && dev_out && !direct) {
            SNPMI_HIP(hipStreamWaitEvent(d.copy, d.produced[q.slot], 0));
            SNPMI_HIP(hipMemcpy2DAsync(out + q.c0 * n_out, n_out * sizeof(T), q.dev_out, ldF * sizeof(T),
                                       n_out * sizeof(T), q.cnt, hipMemcpyDeviceToDevice, d.copy));
            SNPMI_HIP(hipStreamSynchronize(d.copy));  // the block buffer slot is reused two chunks on
        } else if (n_out > 0 && !dev_out) {
            if (!order_c)
                d2h_rows(d, out + q.c0 * n_out, n_out * sizeof(T), q.dev_out, ldF * sizeof(T), n_out * sizeof(T),
                         q.cnt, nthreads, d.produced[q.slot]);
            else
                d2h_rows(d, out + q.c0, m_out * sizeof(T), q.dev_out, q.ldc * sizeof(T), q.cnt * sizeof(T), n_out,
                         nthreads, d.produced[q.slot]);
        }
    };
    // per-SNP stats stay on the device for the whole call and cross PCIe once each way (a per-chunk
    // D2H on the copy stream would wait for that chunk's kernels and stall the next upload)
    T* st_all = (T*)d.get(Device::S_STATS, m_out * 2 * sizeof(T));
    if (sa.kind != SNPMI_STD_NONE && sa.use_stats)
        SNPMI_HIP(hipMemcpyAsync(st_all, stats, m_out * 2 * sizeof(T), hipMemcpyHostToDevice, d.stream));
    for (uint64_t c0 = 0, ci = 0; c0 < m_out; c0 += C, ci++) {
        const uint64_t cnt = std::min(C, m_out - c0);
        const int slot = (int)(ci & 1);
        const uint8_t* packed = stage_chunk(d, m, s.sid_idx, c0, cnt, p, nthreads, slot);
        T* lut = (T*)d.get(Device::S_LUT, cnt * 4 * sizeof(T));
        T* st_dev = st_all + 2 * c0;
        launch_snp_stats(packed, p.pitch_out, n_out, cnt, s.count_a1, sa, dt, st_dev, lut, d.stream);
        Pending q;
        q.c0 = c0;
        q.cnt = cnt;
        q.slot = slot;
        q.st_dev = st_dev;
        q.valid = true;
        if (n_out > 0 && direct) {
            if (!order_c) launch_decode(packed, p.pitch_out, n_out, cnt, lut, dt, 0, out + c0 * n_out, n_out, d.stream);
            else launch_decode(packed, p.pitch_out, n_out, cnt, lut, dt, 1, out + c0, m_out, d.stream);
        } else if (n_out > 0) {
            const Device::Slot os = slot ? Device::S_OUT_B : Device::S_OUT;
            if (!order_c) {
                q.dev_out = (T*)d.get(os, cnt * ldF * sizeof(T));
                launch_decode(packed, p.pitch_out, n_out, cnt, lut, dt, 0, q.dev_out, ldF, d.stream);
            } else {
                // rows padded to 16 B on the device (k_decode_c_reg vector stores), tight on the host
                q.ldc = sizeof(T) < 4 ? cnt : round_up(cnt, 16 / sizeof(T));
                q.dev_out = (T*)d.get(os, q.ldc * n_out * sizeof(T));
                launch_decode(packed, p.pitch_out, n_out, cnt, lut, dt, 1, q.dev_out, q.ldc, d.stream);
            }
        }
        chunk_done(d, slot);
        SNPMI_HIP(hipEventRecord(d.produced[slot], d.stream));
        if (pending.valid) drain(pending);
        pending = q;
    }
    if (pending.valid) drain(pending);
    if (stats_out) SNPMI_HIP(hipMemcpyAsync(stats, st_all, m_out * 2 * sizeof(T), hipMemcpyDeviceToHost, d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.copy));
}

// ====================================================================== BED write (to_bed body)
// Values (caller's host array, n_iid x n_sid, F or C) -> .bed file: magic + SNP-major packed
// columns of ceil(n/4) bytes.  SNP chunks go H2D, are encoded by k_encode_f/c, and come back
// as packed bytes (16x / 32x smaller) that are written with one fwrite per chunk.
template <typename T>
static void bed_write_impl(const char* path, const T* val, uint64_t n, uint64_t m, int order_c, int count_a1) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    SNPMI_REQUIRE(path != nullptr, SNPMI_E_ARG, "path is NULL");
    SNPMI_REQUIRE(val != nullptr || n == 0 || m == 0, SNPMI_E_ARG, "val is NULL");
    Device& d = device();
    FILE* f = std::fopen(path, "wb");
    SNPMI_REQUIRE(f != nullptr, SNPMI_E_IO, std::string("cannot create ") + path);
    struct Closer {
        FILE*& f;
        const char* path;
        bool ok = false;
        ~Closer() {
            if (f) std::fclose(f);
            if (!ok) std::remove(path);
        }
    } closer{f, path};
    const uint8_t magic[3] = {0x6C, 0x1B, 0x01};
    SNPMI_REQUIRE(std::fwrite(magic, 1, 3, f) == 3, SNPMI_E_IO, std::string("write failed: ") + path);
    const uint64_t bpc = ceil_div(n, 4), pitch = packed_pitch(n);
    const int dt = DT<T>::v;
    unsigned int* bad_dev = (unsigned int*)d.get(Device::S_RED, 256);
    if (n > 0 && m > 0) {
        const uint64_t ldF = round_up(n, 16);
        const uint64_t C = order_c ? std::min<uint64_t>(round_up(chunk_snps(n * sizeof(T) + pitch), 64), 1ull << 16)
                                   : chunk_snps(ldF * sizeof(T) + pitch);
        for (uint64_t c0 = 0; c0 < m; c0 += C) {
            const uint64_t cnt = std::min(C, m - c0);
            T* dev_val = (T*)d.get(Device::S_DENSE, cnt * (order_c ? n : ldF) * sizeof(T));
            uint8_t* dev_packed = (uint8_t*)d.get(Device::S_PACKED, cnt * pitch);
            uint8_t* host = (uint8_t*)pinned(0, cnt * bpc);
            SNPMI_HIP(hipMemsetAsync(bad_dev, 0, sizeof(unsigned int), d.stream));
            if (!order_c) {
                SNPMI_HIP(hipMemcpy2DAsync(dev_val, ldF * sizeof(T), val + c0 * n, n * sizeof(T), n * sizeof(T), cnt,
                                           hipMemcpyDefault, d.stream));  // host or device values
                launch_encode(dev_val, dt, 0, ldF, n, cnt, count_a1, dev_packed, pitch, bad_dev, d.stream);
            } else {
                SNPMI_HIP(hipMemcpy2DAsync(dev_val, cnt * sizeof(T), val + c0, m * sizeof(T), cnt * sizeof(T), n,
                                           hipMemcpyDefault, d.stream));
                launch_encode(dev_val, dt, 1, cnt, n, cnt, count_a1, dev_packed, pitch, bad_dev, d.stream);
            }
            unsigned int bad = 0;
            SNPMI_HIP(hipMemcpyAsync(&bad, bad_dev, sizeof(bad), hipMemcpyDeviceToHost, d.stream));
            SNPMI_HIP(hipMemcpy2DAsync(host, bpc, dev_packed, pitch, bpc, cnt, hipMemcpyDeviceToHost, d.stream));
            SNPMI_HIP(hipStreamSynchronize(d.stream));
            SNPMI_REQUIRE(bad == 0, SNPMI_E_ARG,
                          "Expect values to be 0, 1, 2 or missing (NaN, or -127 for int8)");
            SNPMI_REQUIRE(std::fwrite(host, 1, cnt * bpc, f) == cnt * bpc, SNPMI_E_IO,
                          std::string("write failed: ") + path);
        }
    }
    SNPMI_REQUIRE(std::fclose(f) == 0, SNPMI_E_IO, std::string("write failed: ") + path);
    f = nullptr;
    closer.ok = true;
}

// ====================================================================== dense standardize / subset
template <typename T>
static void standardize_impl(T* val, uint64_t rows, uint64_t cols, int order_c, int is_beta, double a, double b,
                             int apply_in_place, int use_stats, T* stats) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    SNPMI_REQUIRE(stats != nullptr, SNPMI_E_ARG, "stats is NULL");
    if (cols == 0) return;
    Device& d = device();
    const size_t bytes = rows * cols * sizeof(T);
    const bool dev = is_device_ptr(d, val);
    // a device val is standardized in place (a scratch copy when only the stats are wanted)
    T* dv = dev && apply_in_place ? val : (T*)d.get(Device::S_DENSE, bytes);
    T* ds = (T*)d.get(Device::S_STATS, cols * 2 * sizeof(T));
    const int nthreads = resolve_threads(0);
    if (dv != val) SNPMI_HIP(hipMemcpyAsync(dv, val, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                           d.stream));
    if (use_stats) SNPMI_HIP(hipMemcpyAsync(ds, stats, cols * 2 * sizeof(T), hipMemcpyHostToDevice, d.stream));
    launch_dense_standardize(dv, rows, cols, order_c ? cols : rows, order_c, DT<T>::v,
                             {is_beta ? SNPMI_STD_BETA : SNPMI_STD_UNIT, a, b, use_stats}, ds, d.stream);
    if (apply_in_place && !dev) d2h_bytes(d, val, dv, bytes, nthreads);
    if (!use_stats) SNPMI_HIP(hipMemcpyAsync(stats, ds, cols * 2 * sizeof(T), hipMemcpyDeviceToHost, d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

template <typename S, typename D>
static void subset_impl(const S* val, uint64_t rows, uint64_t cols, uint64_t k, int in_c, const uint64_t* ri,
                        uint64_t nr, const uint64_t* ci, uint64_t nc, int out_c, D* out) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    SNPMI_REQUIRE(k >= 1, SNPMI_E_ARG, "k must be >= 1");
    SNPMI_REQUIRE(ri && ci, SNPMI_E_ARG, "subset needs explicit row and column indices");
    check_index(ri, nr, rows, "row");
    check_index(ci, nc, cols, "col");
    if (nr * nc == 0) return;
    Device& d = device();
    const size_t in_bytes = rows * cols * k * sizeof(S);
    const bool dev_in = is_device_ptr(d, val), dev_out = is_device_ptr(d, out);
    const S* dv = dev_in ? val : (const S*)d.get(Device::S_DENSE, in_bytes);
    uint64_t* dri = (uint64_t*)d.get(Device::S_IDX, nr * 8);
    uint64_t* dci = (uint64_t*)d.get(Device::S_IDX2, nc * 8);
    D* dout = dev_out ? out : (D*)d.get(Device::S_OUT, nr * nc * k * sizeof(D));
    if (!dev_in) SNPMI_HIP(hipMemcpyAsync((S*)dv, val, in_bytes, hipMemcpyHostToDevice, d.stream));
    SNPMI_HIP(hipMemcpyAsync(dri, ri, nr * 8, hipMemcpyHostToDevice, d.stream));
    SNPMI_HIP(hipMemcpyAsync(dci, ci, nc * 8, hipMemcpyHostToDevice, d.stream));
    launch_subset(dv, DT<S>::v, rows, cols, k, in_c, dri, nr, dci, nc, out_c, dout, DT<D>::v, d.stream);
    if (!dev_out) d2h_bytes(d, out, dout, nr * nc * k * sizeof(D), resolve_threads(0));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

// ====================================================================== GRM
// Hook "syrk" (accepted: 0, 5, 20, 36, 71) and the public switch "f64"
// (pysnptools_amd.set_grm_f64: 1 = every f64 GRM on the f64 MFMA).  The two functions below are
// the only readers; every launcher asks them for the named path (snpmi_internal.hpp F32Path /
// F64Path say what each one runs).
static int g_variant_syrk = 0;
static int g_f64_mfma = 0;
static int g_variant_syrk_split = 0;  // tuning hook: 0 = auto, 1 = off, S = force S slices
static int g_dense_codes = 1;         // tuning / test hook: 0 = dense operands never re-encoded

F32Path syrk_f32_path() {
    switch (g_variant_syrk) {
        case 0: return F32Path::H2;
        case 36: return F32Path::BF3;
        case 5: return F32Path::TILE128;
        default: return F32Path::TWO_PHASE;  // 20, 71
    }
}
F64Path syrk_f64_path() {
    switch (g_variant_syrk) {
        case 0: return g_f64_mfma ? F64Path::TWO_PHASE : F64Path::CRT;
        case 5:
        case 36: return F64Path::FUSED;
        default: return F64Path::TWO_PHASE;  // 20, 71
    }
}

static GrmDest whole_dest(void* tiles, uint64_t n) {
    const uint64_t nb = ceil_div(n, 256);
    return {tiles, nullptr, nullptr, nb * (nb + 1) / 2};
}
static GrmDest part_dest(void* blocks, uint64_t n, int rank, int world) {
    const PartTables pt = part_tables(ceil_div(n, 256), rank, world);  // tab != nullptr even for an empty part
    return {blocks, pt.tab, pt.dslot, grm_part_blocks(n, rank, world)};
}

// The f32 / f64 MFMA path at N >= 4096 / 1024: two phases per sub-block of SNPs -- k_decode_f
// writes the standardized block Z (F order, ld = round_up(N, 256)) to HBM (0.4 ms per 10k SNPs at
// N=50k), then the dense SYRK streams Z into LDS with global_load_lds and runs MFMA-only (no VALU
// in its loader): 136.7 TFLOP/s vs 130.9 for the fused LUT-expanding f32 kernel (tools/ubench.py
// syrk / syrk_dense, N=50k, 10k SNPs).  Sub-blocks keep Z <= 16 GiB.
static bool use_two_phase(int dt, uint64_t n) {
    return dt == SNPMI_DT_F32 ? syrk_f32_path() == F32Path::TWO_PHASE && n >= 4096
                              : syrk_f64_path() == F64Path::TWO_PHASE && n >= 1024;
}

template <typename T, class F>
static void for_z_blocks(Device& d, const uint8_t* packed, uint64_t pitch, uint64_t n, uint64_t m, const T* lut,
                         F&& syrk) {
    const uint64_t ldz = round_up(n, 256);
    uint64_t sub = std::min<uint64_t>(m, std::max<uint64_t>(256, (16ull << 30) / (ldz * sizeof(T))));
    sub = std::min<uint64_t>(m, std::max<uint64_t>(16, sub / 16 * 16));
    T* Z = (T*)d.get(Device::S_ZBLK, sub * ldz * sizeof(T));
    if (ldz > n)  // pad iids read by the last panel: keep them finite (they only feed K(i,j), i or j >= n)
        SNPMI_HIP(hipMemset2DAsync(Z + n, ldz * sizeof(T), 0, (ldz - n) * sizeof(T), sub, d.stream));
    for (uint64_t s0 = 0; s0 < m; s0 += sub) {
        const uint64_t cnt = std::min(sub, m - s0);
        launch_decode(packed + s0 * pitch, pitch, n, cnt, lut + 4 * s0, DT<T>::v, 0, Z, ldz, d.stream);
        syrk((const T*)Z, ldz, cnt, s0 > 0);
    }
}

// split-K slices for the default f32 chain when the 256x256-block grid leaves CUs idle in its last
// round: minimise rounds-per-slice ceil(g*S / CUs) / S, +1% per extra slice (partial sets + the
// reduce), >= 1024 SNPs per slice.  Measured (tools/ubench.py syrk, m = 20k): N=10k 213 -> 242
// TFLOP/s at S=4, N=5k 199 -> 217 at S=6 -- the slice counts this model picks.
static int bf3_split_slices(uint64_t n, uint64_t m, int cus) {
    if (g_variant_syrk_split == 1) return 1;
    if (g_variant_syrk_split > 1) return g_variant_syrk_split;
    const uint64_t nb = ceil_div(n, 256), g = nb * (nb + 1) / 2, C = (uint64_t)std::max(cus, 1);
    const double unsplit = (double)ceil_div(g, C);
    int best = 1;
    double best_cost = unsplit;
    for (int S = 2; S <= 8 && m / (uint64_t)S >= 1024; S++) {
        const double cost = (double)ceil_div(g * S, C) / S * (1.0 + 0.01 * (S - 1));
        if (cost < best_cost) {
            best = S;
            best_cost = cost;
        }
    }
    return best_cost < 0.97 * unsplit ? best : 1;
}

// bf16x3 LUT (32 B per SNP); with h2, also the fp16x2 LUT (16 B per SNP) and its range flag,
// all in one scratch slot
static const uint32_t* lut_bf3(Device& d, const float* lut, uint64_t m, H2Lut* h2 = nullptr) {
    const uint64_t e = lut_bf3_entries(m);
    uint32_t* l3 = (uint32_t*)d.get(Device::S_LUT3, e * 48 + 256);
    launch_lut_bf3(lut, m, l3, d.stream);
    if (h2) {
        uint32_t* l2 = l3 + 8 * e;
        uint32_t* flag = l2 + 4 * e;
        launch_lut_h2(lut, m, l2, flag, d.stream);
        h2->lut2 = l2;
        h2->flag = flag;
    }
    return l3;
}

// f32 segment scratch pool of the current device (syrk.hip SegFlush): kSegSlots slots of 256 KiB
// + their flags, zeroed once when the pool is first allocated (slots are released by the kernels)
SegCtx seg_ctx() {
    SegCtx c;
    c.snps = g_seg_snps > 0 ? (uint32_t)g_seg_snps : 0u;
    if (!c.snps) return c;
    Device& d = device();
    const bool fresh = d.cap[Device::S_SEG] == 0;
    const uint64_t bytes = (uint64_t)kSegSlots * kSegSlotFloats * sizeof(float) + kSegSlots * sizeof(uint32_t);
    uint8_t* base = (uint8_t*)d.get(Device::S_SEG, bytes);
    c.nslots = kSegSlots;
    c.scratch = (float*)base;
    c.flags = (uint32_t*)(base + (uint64_t)kSegSlots * kSegSlotFloats * sizeof(float));
    if (fresh) {  // once per device; complete before any stream's first SYRK can take a slot
        SNPMI_HIP(hipMemsetAsync(c.flags, 0, kSegSlots * sizeof(uint32_t), d.stream));
        SNPMI_HIP(hipStreamSynchronize(d.stream));
    }
    return c;
}

// CRT moduli counters on the device: [0] sum of the launch-wide R, [1] launches (k_crt_r); [2] sum
// of the per-block R_b, [3] blocks (k_crt)
static unsigned long long* crt_record(Device& d) {
    const bool fresh = d.cap[Device::S_CRTREC] == 0;
    auto* rec = (unsigned long long*)d.get(Device::S_CRTREC, 32);
    if (fresh) SNPMI_HIP(hipMemsetAsync(rec, 0, 32, d.stream));
    return rec;
}

// Scratch of the CRT path for `blocks` 256-blocks of output: the residues (one byte per modulus and
// element, at most 4 GiB -- then the launchers chunk), the workspace of one step of <= m SNPs and the
// moduli counters.  sum_plan cuts the collective from crt_res_bytes, as the launches do.
static uint64_t crt_res_bytes(uint64_t blocks) {
    return std::min<uint64_t>(blocks * (uint64_t)crt_moduli() * 65536, 4ull << 30);
}
struct CrtScratch {
    uint8_t* res = nullptr;
    uint64_t res_bytes = 0;
    void* ws = nullptr;
    unsigned long long* rec = nullptr;
    const int* gate() const { return ws ? (const int*)ws + 1 : nullptr; }  // the non-finite flag
};
static CrtScratch crt_scratch(Device& d, uint64_t blocks, uint64_t m, uint64_t na, uint64_t nb) {
    CrtScratch s;
    s.res_bytes = crt_res_bytes(blocks);
    s.res = (uint8_t*)d.get(Device::S_ZBLK, s.res_bytes);
    s.ws = d.get(Device::S_LUT3, crt_lut_bytes(std::min(m, crt_max_snps()), na, nb));
    s.rec = crt_record(d);
    return s;
}

// One f64 product K (+)= Za Zb^T over m SNPs, crt_max_snps() per step.  B.P == nullptr: Zb = Za and
// o is the whole K or a part (a part's residue chunks follow its layout table); else o.k holds the
// o.blocks dense blocks of the rectangle.  On the CRT path each step is the int8 residue launch
// (syrk_crt.hip), then the f64 MFMA kernel gated on the step's non-finite flag; off it (hooks "syrk"
// / "f64") every block runs on the fused f64 MFMA kernel in the same steps.
static void syrk_f64_steps(Device& d, const PackedSide& A, const PackedSide& B, uint64_t m, const double* lut,
                           const GrmDest& o, int accumulate) {
    const uint64_t step = crt_max_snps();
    const CrtScratch s = syrk_f64_path() == F64Path::CRT ? crt_scratch(d, o.blocks, m, A.n, B.n) : CrtScratch();
    for (uint64_t s0 = 0; s0 < m; s0 += step) {
        const uint64_t cnt = std::min(step, m - s0);
        const int acc = accumulate || s0 > 0;
        const PackedSide a{A.P + s0 * A.pitch, A.pitch, A.n}, b{B.P ? B.P + s0 * B.pitch : nullptr, B.pitch, B.n};
        const double* L = lut + 4 * s0;
        if (s.ws)
            launch_syrk_crt(a, b, cnt, L, (double*)o.k, acc, s.ws, s.res, s.res_bytes, s.rec, d.stream, nullptr, nullptr,
                            o.tab, o.blocks);
        if (b.P) launch_syrk_rect_f64(a.P, a.pitch, a.n, b.P, b.pitch, b.n, cnt, L, (double*)o.k, acc, d.stream, s.gate());
        else launch_syrk_packed(a.P, a.pitch, a.n, cnt, L, SNPMI_DT_F64, o, acc, d.stream, s.gate());
    }
}

// The MFMA paths of both dtypes (everything but the CRT path).  f32 default: the fp16x2 / bf16x3
// chain (309 TFLOP/s for bf16x3 alone at N=50k, 10k SNPs vs 136 for the f32-MFMA two-phase path --
// tools/ubench.py syrk); otherwise the two-phase path or the fused kernels.  Two things differ by
// destination: a part's grid is never split along K, and it has its own dense launcher.
static void syrk_packed_mfma(Device& d, const uint8_t* packed, uint64_t pitch, uint64_t n, uint64_t m,
                             const void* lut, int dt, const GrmDest& o, int accumulate) {
    const F32Path p32 = syrk_f32_path();
    if (dt == SNPMI_DT_F32 && (p32 == F32Path::H2 || p32 == F32Path::BF3)) {
        H2Lut h2;
        const bool h = p32 == F32Path::H2 && m > 0;
        const uint32_t* l3 = lut_bf3(d, (const float*)lut, m, h ? &h2 : nullptr);
        const int S = o.tab ? 1 : bf3_split_slices(n, m, d.cu_count);
        if (S > 1) {
            float* part = (float*)d.get(Device::S_ZBLK, (uint64_t)S * n_tiles_upper(n) * kTile * kTile * sizeof(float));
            launch_syrk_packed_bf3_split(packed, pitch, n, m, l3, S, part, (float*)o.k, accumulate, d.stream,
                                         h ? &h2 : nullptr);
        } else {
            launch_syrk_packed_bf3(packed, pitch, n, m, l3, o, accumulate, d.stream, h ? &h2 : nullptr);
        }
        return;
    }
    if (!use_two_phase(dt, n) || m == 0) {
        launch_syrk_packed(packed, pitch, n, m, lut, dt, o, accumulate, d.stream);
        return;
    }
    auto run = [&](const void* Z, uint64_t ldz, uint64_t cnt, bool more) {
        if (o.tab) launch_syrk_dense_part((const float*)Z, ldz, n, cnt, o, accumulate || more, d.stream);
        else launch_syrk_dense(Z, ldz, n, cnt, dt, o.k, accumulate || more, d.stream);
    };
    if (dt == SNPMI_DT_F32) for_z_blocks(d, packed, pitch, n, m, (const float*)lut, run);
    else for_z_blocks(d, packed, pitch, n, m, (const double*)lut, run);
}

// K (+)= Z Z^T of a packed SNP block into the whole K or one part: f64 in the steps of
// syrk_f64_steps (the whole K only on the CRT path; a part -- cfg5 in the reference's default dtype --
// always, its dense launcher being f32 only), else the MFMA paths, for f32 inside the exact diagonal
// (hook "diag")
static void syrk_packed_auto(Device& d, const uint8_t* packed, uint64_t pitch, uint64_t n, uint64_t m,
                             const void* lut, int dt, const GrmDest& o, int accumulate) {
    const bool part64 = dt == SNPMI_DT_F64 && o.tab;
    if (part64) {
        if (o.blocks == 0) return;
        SNPMI_REQUIRE(4 * o.blocks < (1ull << 31), SNPMI_E_ARG, "too many GRM blocks for one launch");
        SNPMI_REQUIRE(pitch % 64 == 0 && pitch * 4 >= ceil_div(n, 256) * 256, SNPMI_E_ARG,
                      "packed pitch must cover round_up(n, 256) iids");
        if (m == 0) {
            if (!accumulate) SNPMI_HIP(hipMemsetAsync(o.k, 0, o.blocks * 256 * 256 * sizeof(double), d.stream));
            return;
        }
    }
    if (part64 || (dt == SNPMI_DT_F64 && syrk_f64_path() == F64Path::CRT && m > 0 && n > 0)) {
        syrk_f64_steps(d, {packed, pitch, n}, {nullptr, 0, 0}, m, (const double*)lut, o, accumulate);
        return;
    }
    if (dt == SNPMI_DT_F32 && g_diag_exact && m > 0 && n > 0) {
        double* diag = (double*)d.get(Device::S_DIAG, diag_scratch_bytes(n, m));
        launch_diag_begin((const float*)o.k, n, o.dslot, accumulate, diag, d.stream);
        syrk_packed_mfma(d, packed, pitch, n, m, lut, dt, o, accumulate);
        launch_diag_end(packed, pitch, n, m, (const float*)lut, (float*)o.k, o.dslot, diag, d.stream);
        return;
    }
    syrk_packed_mfma(d, packed, pitch, n, m, lut, dt, o, accumulate);
}

// Finish a GRM held as tiles on the device: optional DiagKtoN, then K (n x n) to the host,
// extracted in row blocks so the device never needs a second full-size K.
template <typename T>
static void grm_finish(Device& d, const T* tiles, uint64_t n, int diag_k_to_n, double* factor, T* K_out) {
    double scale = 1.0;
    if (diag_k_to_n) {
        double* tr = (double*)d.get(Device::S_RED, 64);
        launch_grm_trace(tiles, n, DT<T>::v, tr, d.stream);
        double trace = 0;
        SNPMI_HIP(hipMemcpyAsync(&trace, tr, 8, hipMemcpyDeviceToHost, d.stream));
        SNPMI_HIP(hipStreamSynchronize(d.stream));
        const double f = (double)n / trace;
        if (factor) *factor = f;
        if (std::fabs(f - 1.0) > 1e-15) scale = f;  // diag_K_to_N.py:56-59
    }
    if (n == 0) return;
    const bool dev = is_device_ptr(d, K_out);
    const uint64_t rows_per = dev ? n : std::max<uint64_t>(1, std::min<uint64_t>(n, (1ull << 30) / (n * sizeof(T))));
    for (uint64_t r0 = 0; r0 < n; r0 += rows_per) {
        const uint64_t nr = std::min(rows_per, n - r0);
        // a device K_out is written in one extraction launch, no host copy; a host K_out goes
        // through 1 GiB row blocks (d2h_rows returns once the block has landed, so the next
        // extraction may reuse the staging buffer)
        T* dk = dev ? K_out : (T*)d.get(Device::S_K, nr * n * sizeof(T));
        launch_grm_extract_rows(tiles, n, DT<T>::v, r0, nr, scale, dk, d.stream);
        if (!dev) d2h_rows(d, K_out + r0 * n, n * sizeof(T), dk, n * sizeof(T), n * sizeof(T), nr, resolve_threads(0));
    }
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

// Stream the SNP columns of one .bed through stats and `syrk(packed, pitch, n, cnt, lut,
// accumulate)` (first = overwrite).  Returns true if anything was written.
template <typename T, class Syrk>
static bool grm_stream_bed(Device& d, bool first, const BedSel& s, const StdArgs& sa, T* stats, Syrk&& syrk) {
    BedMap m;
    open_sel(m, s);
    const uint64_t n_out = s.n_out, m_out = s.m_out;
    const int std_kind = sa.kind, use_stats = sa.use_stats;
    SNPMI_REQUIRE(stats != nullptr || std_kind == SNPMI_STD_NONE || m_out == 0, SNPMI_E_ARG, "stats is NULL");
    const int nthreads = resolve_threads(s.num_threads);
    const int dt = DT<T>::v;
    IidPlan p = plan_iids(d, s);
    // ~0.5 GiB of packed codes per chunk keeps >= 2 chunks in flight for cfg4-sized inputs
    const uint64_t C = chunk_snps(p.pitch_in + p.pitch_out, 1ull << 29);
    const bool has_stats = std_kind != SNPMI_STD_NONE && m_out > 0 && n_out > 0;
    // stats of every chunk stay on the device (16 B per SNP) and cross PCIe once, before / after
    // the chunk loop: a per-chunk stats D2H on the compute stream shares a DMA engine with the
    // next chunk's H2D and held that upload until the chunk's SYRK had finished (profiles/r03h)
    T* st_host = has_stats ? (T*)pinned(2, m_out * 2 * sizeof(T)) : nullptr;
    T* st_all = (T*)d.get(Device::S_STATS, std::max<uint64_t>(m_out, 1) * 2 * sizeof(T));
    if (has_stats && use_stats) {
        std::memcpy(st_host, stats, m_out * 2 * sizeof(T));
        SNPMI_HIP(hipMemcpyAsync(st_all, st_host, m_out * 2 * sizeof(T), hipMemcpyHostToDevice, d.stream));
    }
    bool wrote = false;
    // the first chunk is an eighth of the others: its gather + upload is the one that cannot hide
    // under a SYRK, the later ones stage while the previous chunk computes
    const uint64_t C1 = std::max<uint64_t>(std::min<uint64_t>(C, 2048), C / 8);
    if (m_out > C1 && n_out > 0) {  // size both device slots for a full chunk up front: no regrowth
        const uint64_t cmax = std::min(C, m_out);  // (a free + alloc) between the first two chunks
        SNPMI_HIP(hipStreamSynchronize(d.copy));
        for (int slot = 0; slot < 2; slot++) (void)d.get(slot ? Device::S_PACKED_B : Device::S_PACKED, cmax * p.pitch_in);
        if (p.repack) (void)d.get(Device::S_PACKED2, cmax * p.pitch_out);
    }
    for (uint64_t c0 = 0, ci = 0; c0 < m_out && n_out > 0; ci++) {
        const uint64_t cnt = std::min(ci == 0 ? C1 : C, m_out - c0);
        const uint8_t* packed = stage_chunk(d, m, s.sid_idx, c0, cnt, p, nthreads, (int)(ci & 1));
        T* lut = (T*)d.get(Device::S_LUT, std::min(C, m_out) * 4 * sizeof(T));
        T* st_dev = st_all + 2 * c0;
        launch_snp_stats(packed, p.pitch_out, n_out, cnt, s.count_a1, sa, dt, st_dev, lut, d.stream);
        syrk(packed, p.pitch_out, n_out, cnt, (const T*)lut, !(first && !wrote));
        wrote = true;
        chunk_done(d, (int)(ci & 1));
        c0 += cnt;
    }
    if (has_stats && !use_stats && n_out > 0)
        SNPMI_HIP(hipMemcpyAsync(st_host, st_all, m_out * 2 * sizeof(T), hipMemcpyDeviceToHost, d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.copy));
    if (has_stats && !use_stats && n_out > 0) std::memcpy(stats, st_host, m_out * 2 * sizeof(T));
    if (n_out == 0 && std_kind != SNPMI_STD_NONE && !use_stats) {
        for (uint64_t j = 0; j < m_out; j++) stats[2 * j] = stats[2 * j + 1] = (T)NAN;
    }
    return wrote;
}

// Accumulate the SNP columns of one .bed into the replicated upper-triangle tiles.
template <typename T>
static bool grm_add_bed(Device& d, T* tiles, bool first, const BedSel& s, const StdArgs& sa, T* stats) {
    return grm_stream_bed<T>(d, first, s, sa, stats,
                             [&](const uint8_t* packed, uint64_t pitch, uint64_t n, uint64_t cnt, const T* lut, bool acc) {
                                 syrk_packed_auto(d, packed, pitch, n, cnt, lut, DT<T>::v, whole_dest(tiles, n), acc);
                             });
}

template <typename T>
static void grm_bed_impl(const BedSel& s, const StdArgs& sa, T* stats, int diag_k_to_n, double* factor, T* K_out) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    SNPMI_REQUIRE(K_out != nullptr || s.n_out == 0, SNPMI_E_ARG, "K_out is NULL");
    Device& d = device();
    const uint64_t tile_bytes = n_tiles_upper(s.n_out) * kTile * kTile * sizeof(T);
    T* tiles = (T*)d.get(Device::S_TILES, tile_bytes);
    if (!grm_add_bed<T>(d, tiles, true, s, sa, stats)) SNPMI_HIP(hipMemsetAsync(tiles, 0, tile_bytes, d.stream));
    grm_finish(d, tiles, s.n_out, diag_k_to_n, factor, K_out);
}

// ---------------------------------------------------------------------- GRM session (several .bed files)
struct GrmSession {
    bool active = false;
    bool wrote = false;
    uint64_t n = 0;
    int dtype = SNPMI_DT_F32;
};
static GrmSession g_session;

static void* session_tiles(Device& d) {
    return d.get(Device::S_SESSION, n_tiles_upper(g_session.n) * kTile * kTile * dtype_size(g_session.dtype));
}

// What an add asks of the open session, in the order every entry point reports it: that there is
// one, that it has the add's dtype, that it has the add's iid count.  The reduce forms check their
// collective arguments between the dtype and the iid count (check_reduce_args), hence the pieces.
static void session_check_open() {
    SNPMI_REQUIRE(g_session.active, SNPMI_E_ARG, "no GRM session (call snpmi_grm_begin)");
}
static void session_check_dtype(int dtype) {
    session_check_open();
    SNPMI_REQUIRE(g_session.dtype == dtype, SNPMI_E_ARG, "dtype differs from snpmi_grm_begin");
}
static void session_check_iids(uint64_t n) {
    SNPMI_REQUIRE(n == g_session.n, SNPMI_E_ARG, "iid count differs from snpmi_grm_begin");
}
static void session_check(int dtype, uint64_t n) {
    session_check_dtype(dtype);
    session_check_iids(n);
}
template <typename T>
static void session_check(uint64_t n) {
    session_check(DT<T>::v, n);
}

// The argument checks several entry points share; a site whose text has always differed passes it.
static bool part_ok(int rank, int world) { return world >= 1 && rank >= 0 && rank < world; }
static void check_part(int rank, int world, const char* msg = "bad partition") {
    SNPMI_REQUIRE(part_ok(rank, world), SNPMI_E_ARG, msg);
}
static void check_pitch(uint64_t pitch, uint64_t n, const char* msg = "pitch must be snpmi_packed_pitch") {
    SNPMI_REQUIRE(pitch % 64 == 0 && pitch >= ceil_div(n, 4), SNPMI_E_ARG, msg);
}

// supertile block order of the dense fp16x2 SYRK, kept on the device per (nb, xcd); built once
// (blocking copy from a local vector), callers hold g_call_mutex
static const uint32_t* dense_order(Device& d, uint64_t nb, bool xcd) {
    if (d.order_nb[xcd] != nb || !d.order_tab[xcd]) {
        std::vector<uint32_t> tab;
        supertile_order(nb, xcd, tab);
        if (d.order_tab[xcd]) SNPMI_HIP(hipFree(d.order_tab[xcd]));
        d.order_tab[xcd] = nullptr;
        d.order_nb[xcd] = 0;
        if (hipMalloc(&d.order_tab[xcd], tab.size() * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            throw Error(SNPMI_E_NOMEM, "hipMalloc of the block order table failed");
        }
        SNPMI_HIP(hipMemcpy(d.order_tab[xcd], tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        d.order_nb[xcd] = nb;
    }
    return d.order_tab[xcd];
}

// the packed fp16x2 SYRK's block order (syrk.hip): the same supertile table, cached per nb
const uint32_t* packed_block_order(uint64_t nb) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    return dense_order(device(), nb, false);
}

// the cfg5 part layout of part `rank` of `world` on the current device (syrk.hip part_layout):
// one allocation = the layout table (u32 per local block) + the diagonal-slot table (i32 per block
// column) + the block-slot table (i32 per upper-triangle block), cached per (nb, rank, world)
PartTables part_tables(uint64_t nb, int rank, int world) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    Device& d = device();
    const uint64_t key[3] = {nb, (uint64_t)rank, (uint64_t)world};
    const uint64_t ntab = grm_part_blocks(nb * 256, rank, world), off = round_up(std::max<uint64_t>(ntab, 1), 64);
    const uint64_t off2 = off + round_up(std::max<uint64_t>(nb, 1), 64), total = nb * (nb + 1) / 2;
    if (!d.part_tab || d.part_key[0] != key[0] || d.part_key[1] != key[1] || d.part_key[2] != key[2]) {
        std::vector<uint32_t> tab;
        part_layout(nb, rank, world, tab);
        SNPMI_REQUIRE(tab.size() == ntab, SNPMI_E_ARG, "part layout size mismatch");
        std::vector<int32_t> dslot(nb, -1), lslot(total, -1);
        for (uint64_t w = 0; w < tab.size(); w++) {
            const uint64_t bi = tab[w] & 0xffffu, bj = tab[w] >> 16;
            if (bi == bj) dslot[bj] = (int32_t)w;
            lslot[bj * (bj + 1) / 2 + bi] = (int32_t)w;
        }
        std::vector<uint32_t> buf(off2 + total);
        std::copy(tab.begin(), tab.end(), buf.begin());
        std::memcpy(buf.data() + off, dslot.data(), nb * sizeof(int32_t));
        std::memcpy(buf.data() + off2, lslot.data(), total * sizeof(int32_t));
        if (d.part_tab) SNPMI_HIP(hipFree(d.part_tab));
        d.part_tab = nullptr;
        for (int i = 0; i < 3; i++) d.part_key[i] = 0;
        if (hipMalloc(&d.part_tab, buf.size() * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            d.part_tab = nullptr;
            throw Error(SNPMI_E_NOMEM, "hipMalloc of the part layout table failed");
        }
        SNPMI_HIP(hipMemcpy(d.part_tab, buf.data(), buf.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        for (int i = 0; i < 3; i++) d.part_key[i] = key[i];
    }
    PartTables t;
    t.tab = (const uint32_t*)d.part_tab;
    t.dslot = (const int32_t*)((const uint32_t*)d.part_tab + off);
    t.lslot = (const int32_t*)((const uint32_t*)d.part_tab + off2);
    return t;
}

// dense GRM operand on the device.  f32 on the default path: genotype-valued columns are re-encoded
// as codes (hook "dense_codes"); else n >= 4096 takes the fp16x2 split kernel in SNP chunks of
// bounded stage-image scratch (falls back to the f32-MFMA k_syrk256d on the device-side range
// flag, or when the scratch cannot be allocated).  Everything else: launch_syrk_dense.
static void syrk_dense_auto(Device& d, const void* Z, uint64_t ldz, uint64_t n, uint64_t m, int dt, void* tiles,
                            int accumulate) {
    const bool h2_path = dt == SNPMI_DT_F32 && syrk_f32_path() == F32Path::H2 && m > 0;
    if (h2_path && g_dense_codes) {
        // genotype-valued columns (<= 4 distinct values each, e.g. a standardized SnpData): exact
        // re-encoding as codes + LUT, then the packed fp16x2 SYRK; one host sync for the flag
        const uint64_t pitch = packed_pitch(n);
        uint8_t* packed = (uint8_t*)d.get(Device::S_DPACK, m * pitch);
        float* lut = (float*)d.get(Device::S_DLUT, m * 16 + 256);
        unsigned int* flag = (unsigned int*)(lut + 4 * m);
        launch_dense_codes((const float*)Z, ldz, n, m, packed, pitch, lut, flag, d.stream);
        unsigned int f = 1;
        SNPMI_HIP(hipMemcpyAsync(&f, flag, sizeof(f), hipMemcpyDeviceToHost, d.stream));
        SNPMI_HIP(hipStreamSynchronize(d.stream));
        if (f == 0) {
            syrk_packed_auto(d, packed, pitch, n, m, lut, dt, whole_dest(tiles, n), accumulate);
            return;
        }
    }
    if (h2_path && n >= 4096 && ldz % 256 == 0) {
        // the blocks of n, not of ldz: the launch, the stage images and the kernel all count
        // ceil(n / 256), and a longer ldz (allowed: rows past n are never used) must not change them
        const uint64_t nb = ceil_div(n, 256);
        const uint64_t scratch = round_up(dense_h2_scratch_bytes(n, m), 256);
        uint16_t* img = nullptr;
        try {
            img = (uint16_t*)d.get(Device::S_H2, scratch + 256);
        } catch (const Error& e) {
            if (e.code != SNPMI_E_NOMEM) throw;
            img = nullptr;  // HBM is full: the f32-MFMA kernel needs no scratch
        }
        if (img) {
            uint32_t* flag = (uint32_t*)((uint8_t*)img + scratch);
            launch_syrk_dense_h2((const float*)Z, ldz, n, m, img, flag, dense_order(d, nb, false), (float*)tiles,
                                 accumulate, d.stream);
            return;
        }
    }
    launch_syrk_dense(Z, ldz, n, m, dt, tiles, accumulate, d.stream);
}

// A dense operand (rows = iids, cols = SNPs; F or C order, host or device memory) as the F-order Z
// of the SYRKs in S_DENSE, *ldz = round_up(rows, 256): the 256-iid panels of the glds SYRK
template <typename T>
static T* dense_upload(Device& d, const T* val, uint64_t rows, uint64_t cols, int order_c, uint64_t* ldz) {
    const uint64_t ld = round_up(std::max<uint64_t>(rows, 1), 256);
    T* Z = (T*)d.get(Device::S_DENSE, ld * std::max<uint64_t>(cols, 1) * sizeof(T));
    *ldz = ld;
    if (cols == 0 || rows == 0) return Z;
    if (!order_c) {
        SNPMI_HIP(hipMemcpy2DAsync(Z, ld * sizeof(T), val, rows * sizeof(T), rows * sizeof(T), cols, hipMemcpyDefault,
                                   d.stream));  // host or device val
    } else if (is_device_ptr(d, val)) {
        launch_transpose_to_f(val, rows, cols, DT<T>::v, Z, ld, d.stream);
    } else {
        T* Zc = (T*)d.get(Device::S_DENSE2, rows * cols * sizeof(T));
        SNPMI_HIP(hipMemcpyAsync(Zc, val, rows * cols * sizeof(T), hipMemcpyHostToDevice, d.stream));
        launch_transpose_to_f(Zc, rows, cols, DT<T>::v, Z, ld, d.stream);
    }
    return Z;
}

// Standardize the F-order operand Z in place with host stats [cols][2]: sent first if given, brought
// back if computed (enqueued; the caller synchronises).  standardize_impl keeps its own sequence:
// its value copy-out sits between the launch and the stats copy.
static void dense_standardize(Device& d, void* Z, uint64_t rows, uint64_t cols, uint64_t ldz, int dtype,
                              const StdArgs& sa, void* stats) {
    const size_t sb = cols * 2 * dtype_size(dtype);
    void* ds = d.get(Device::S_STATS, sb);
    if (sa.use_stats) SNPMI_HIP(hipMemcpyAsync(ds, stats, sb, hipMemcpyHostToDevice, d.stream));
    launch_dense_standardize(Z, rows, cols, ldz, 0, dtype, sa, ds, d.stream);
    if (!sa.use_stats) SNPMI_HIP(hipMemcpyAsync(stats, ds, sb, hipMemcpyDeviceToHost, d.stream));
}

template <typename T>
static void grm_dense_impl(const T* val, uint64_t rows, uint64_t cols, int order_c, const StdArgs& sa, T* stats,
                           int diag_k_to_n, double* factor, T* K_out) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    SNPMI_REQUIRE(K_out != nullptr || rows == 0, SNPMI_E_ARG, "K_out is NULL");
    Device& d = device();
    const int dt = DT<T>::v;
    uint64_t ldz = 0;
    T* Z = dense_upload(d, val, rows, cols, order_c, &ldz);
    if (sa.kind != SNPMI_STD_NONE && cols > 0) dense_standardize(d, Z, rows, cols, ldz, dt, sa, stats);
    const uint64_t tile_bytes = n_tiles_upper(rows) * kTile * kTile * sizeof(T);
    T* tiles = (T*)d.get(Device::S_TILES, tile_bytes);
    if (rows > 0) syrk_dense_auto(d, Z, ldz, rows, cols, dt, tiles, 0);
    grm_finish(d, tiles, rows, diag_k_to_n, factor, K_out);
}

template <typename T>
static void diag_k_to_n_impl(T* K, uint64_t n, double* factor) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    if (n == 0) return;
    Device& d = device();
    const bool dev = is_device_ptr(d, K);  // device K: traced and scaled in place
    T* dk = dev ? K : (T*)d.get(Device::S_K, n * n * sizeof(T));
    double* tr = (double*)d.get(Device::S_RED, 64);
    if (!dev) SNPMI_HIP(hipMemcpyAsync(dk, K, n * n * sizeof(T), hipMemcpyHostToDevice, d.stream));
    launch_dense_trace(dk, n, DT<T>::v, tr, d.stream);
    double trace = 0;
    SNPMI_HIP(hipMemcpyAsync(&trace, tr, 8, hipMemcpyDeviceToHost, d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
    const double f = (double)n / trace;
    if (factor) *factor = f;
    if (std::fabs(f - 1.0) > 1e-15) {
        launch_dense_scale(dk, n * n, DT<T>::v, f, d.stream);
        if (!dev) SNPMI_HIP(hipMemcpyAsync(K, dk, n * n * sizeof(T), hipMemcpyDeviceToHost, d.stream));
        SNPMI_HIP(hipStreamSynchronize(d.stream));
    }
}

// SNP-side DiagKtoN (diag_K_to_N.py:75-95): factor = rows / sum(val^2); val *= sqrt(factor)
// when |factor - 1| > 1e-15.  scale_only: val *= scale (trained DiagKtoN / kernel rescale).
template <typename T>
static void snp_scale_impl(T* val, uint64_t count, double rows, int scale_only, double scale, double* factor) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    if (count == 0) {
        if (factor) *factor = rows / 0.0;
        return;
    }
    Device& d = device();
    const bool dev = is_device_ptr(d, val);  // device val: scaled in place
    T* dv = dev ? val : (T*)d.get(Device::S_DENSE, count * sizeof(T));
    if (!dev) SNPMI_HIP(hipMemcpyAsync(dv, val, count * sizeof(T), hipMemcpyHostToDevice, d.stream));
    double s = scale;
    if (!scale_only) {
        double* ss = (double*)d.get(Device::S_RED, 64);
        launch_sumsq(dv, count, DT<T>::v, ss, d.stream);
        double sum = 0;
        SNPMI_HIP(hipMemcpyAsync(&sum, ss, 8, hipMemcpyDeviceToHost, d.stream));
        SNPMI_HIP(hipStreamSynchronize(d.stream));
        const double f = rows / sum;
        if (factor) *factor = f;
        if (!(std::fabs(f - 1.0) > 1e-15)) return;
        s = std::sqrt(f);
    }
    launch_dense_scale(dv, count, DT<T>::v, s, d.stream);
    if (dev) SNPMI_HIP(hipStreamSynchronize(d.stream));
    else d2h_bytes(d, val, dv, count * sizeof(T), resolve_threads(0));
}

// Z Z^T of an already standardized dense block (rows = iids, cols = SNPs, F or C) added to the
// session's tiles: the generic SnpReader._read_kernel block loop (snpreader.py:651-655) for
// readers/standardizers the fused BED path does not cover, with K kept in HBM.
template <typename T>
static void grm_add_dense_impl(const T* val, uint64_t rows, uint64_t cols, int order_c) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    session_check<T>(rows);
    SNPMI_REQUIRE(val != nullptr || rows == 0 || cols == 0, SNPMI_E_ARG, "val is NULL");
    if (rows == 0 || cols == 0) return;
    Device& d = device();
    T* tiles = (T*)session_tiles(d);
    uint64_t ldz = 0;
    const T* Z = dense_upload(d, val, rows, cols, order_c, &ldz);
    syrk_dense_auto(d, Z, ldz, rows, cols, DT<T>::v, tiles, g_session.wrote ? 1 : 0);
    g_session.wrote = true;
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

// dist.hip (snpmi_grm_add_dist_*): the session's operand buffer, and the add of a block converted
// into it -- grm_dense_impl's standardize + SYRK on the session's tiles
void* grm_session_operand(int dtype, uint64_t rows, uint64_t cols, uint64_t* ldz) {
    session_check(dtype, rows);
    *ldz = round_up(std::max<uint64_t>(rows, 1), 256);
    return device().get(Device::S_DENSE, *ldz * std::max<uint64_t>(cols, 1) * dtype_size(dtype));
}

void grm_session_add_operand(int dtype, void* Z, uint64_t ldz, uint64_t cols, const StdArgs& sa, void* stats) {
    Device& d = device();
    const uint64_t n = g_session.n;
    if (sa.kind != SNPMI_STD_NONE) dense_standardize(d, Z, n, cols, ldz, dtype, sa, stats);
    syrk_dense_auto(d, Z, ldz, n, cols, dtype, session_tiles(d), g_session.wrote ? 1 : 0);
    g_session.wrote = true;
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

// Packed SNP columns already in HBM (PackedSnps: [m][pitch] bytes, every iid of the reader): the
// argument checks every add of them shares, their chunks and the per-chunk stats + LUT.
static void check_packed_args(const PackedSnps& ps, const StdArgs& sa, const void* stats) {
    check_pitch(ps.pitch, ps.n);
    SNPMI_REQUIRE(sa.kind >= SNPMI_STD_NONE && sa.kind <= SNPMI_STD_BETA, SNPMI_E_ARG, "bad standardizer kind");
    SNPMI_REQUIRE(stats != nullptr || sa.kind == SNPMI_STD_NONE || ps.m == 0, SNPMI_E_ARG, "stats is NULL");
}
// equal chunks of <= 2^16 SNPs (the int32 / CRT accumulation cap), multiples of 256
static uint64_t packed_chunk_snps(uint64_t m) {
    const uint64_t nchunk = m ? ceil_div(m, 1ull << 16) : 1;
    return std::min<uint64_t>(1ull << 16, round_up(ceil_div(m, nchunk), 256));
}
// Per chunk one stats launch (LUT) and `mul(src, cnt, lut, last)`, so a rank's whole SNP shard
// accumulates in registers over up to 65536 SNPs per K-tile round trip instead of one per 10k block
// (the reference's block_size bounds host memory, snpreader.py:651).  stats may be host memory
// (copied synchronously) or device memory (the call then only enqueues).
template <typename T, class Mul>
static void for_packed_chunks(Device& d, const PackedSnps& ps, const StdArgs& sa, T* stats, Mul&& mul) {
    const uint64_t m = ps.m;
    if (m == 0 || ps.n == 0) return;
    SNPMI_REQUIRE(ps.P != nullptr && is_device_ptr(d, ps.P), SNPMI_E_ARG,
                  "packed must be device memory of the current device");
    const bool host_stats = stats && sa.kind != SNPMI_STD_NONE && !is_device_ptr(d, stats);
    const uint64_t step = packed_chunk_snps(m);
    for (uint64_t s0 = 0; s0 < m; s0 += step) {
        const uint64_t cnt = std::min(step, m - s0);
        const uint8_t* src = ps.P + s0 * ps.pitch;
        T* lut = (T*)d.get(Device::S_LUT, cnt * 4 * sizeof(T));
        T* st = (stats && !host_stats) ? stats + 2 * s0 : (T*)d.get(Device::S_STATS, cnt * 2 * sizeof(T));
        if (host_stats && sa.use_stats)
            SNPMI_HIP(hipMemcpyAsync(st, stats + 2 * s0, cnt * 2 * sizeof(T), hipMemcpyHostToDevice, d.stream));
        launch_snp_stats(src, ps.pitch, ps.n, cnt, ps.count_a1, sa, DT<T>::v, st, lut, d.stream);
        mul(src, cnt, (const T*)lut, s0 + cnt == m);
        if (host_stats && !sa.use_stats) {
            SNPMI_HIP(hipMemcpyAsync(stats + 2 * s0, st, cnt * 2 * sizeof(T), hipMemcpyDeviceToHost, d.stream));
            SNPMI_HIP(hipStreamSynchronize(d.stream));  // S_STATS is reused by the next chunk
        }
    }
    if (host_stats) SNPMI_HIP(hipStreamSynchronize(d.stream));
}

template <typename T>
static void check_session_packed(const PackedSnps& ps, const StdArgs& sa, const T* stats) {
    session_check<T>(ps.n);
    check_packed_args(ps, sa, stats);
    SNPMI_REQUIRE(ps.P != nullptr || ps.m == 0 || ps.n == 0, SNPMI_E_ARG, "packed is NULL");
}
// one chunk into the session's tiles
template <typename T>
static void session_add_chunk(Device& d, const uint8_t* src, uint64_t pitch, uint64_t cnt, const T* lut) {
    syrk_packed_auto(d, src, pitch, g_session.n, cnt, lut, DT<T>::v, whole_dest(session_tiles(d), g_session.n),
                     g_session.wrote ? 1 : 0);
    g_session.wrote = true;
}

// the chunks added to the session
template <typename T>
static void grm_add_packed_impl(const PackedSnps& ps, const StdArgs& sa, T* stats) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    check_session_packed(ps, sa, stats);
    Device& d = device();
    for_packed_chunks(d, ps, sa, stats, [&](const uint8_t* src, uint64_t cnt, const T* lut, bool) {
        session_add_chunk(d, src, ps.pitch, cnt, lut);
    });
}
// Column groups of the upper triangle for an overlapped collective: ranges [L0, L1) of 256-block
// indices covering whole supertile columns (16 block columns).  The last group holds ~1/4 of the
// blocks (its sum is the exposed tail), the others split the first ~3/4 evenly; every group
// boundary costs about one round of workgroups (~4 ms at 50k iids, profiles/r04l), so the bench
// uses 2 groups.
struct ColGroup {
    uint64_t L0, L1;  // 256-block index range (supertile table and triangular order alike)
    uint64_t c0, c1;  // block columns [c0, c1)
};
static std::vector<ColGroup> column_groups(uint64_t nb, int parts) {
    const uint64_t ns = ceil_div(nb, 16);
    auto B = [&](uint64_t c) { c = std::min(c, nb); return c * (c + 1) / 2; };
    const uint64_t P = (uint64_t)std::max<int64_t>(1, std::min<int64_t>(parts, (int64_t)ns));
    std::vector<ColGroup> out;
    uint64_t J = 0;
    for (uint64_t p = 0; p < P && J < ns; p++) {
        const uint64_t target = p + 1 == P ? B(nb) : (uint64_t)((double)B(nb) * 0.75 * (double)(p + 1) / (double)(P - 1));
        uint64_t J1 = J + 1;
        while (J1 < ns && B(16 * J1) < target) J1++;
        if (p + 1 == P) J1 = ns;
        out.push_back({B(16 * J), B(16 * J1), std::min(16 * J, nb), std::min(16 * J1, nb)});
        J = J1;
    }
    return out;
}

// snpmi_grm_add_packed_f32 followed by the K-tile collective (collective 1 = ncclReduce onto
// root, 2 = ncclAllReduce, 0 = none), overlapped: the last SNP chunk's SYRK runs as `parts` column
// groups of the triangle (launch_syrk_packed_h2_cols, the same K bit for bit), and as soon as a
// group's SYRK and diagonal write-back are done its contiguous range of tiles is summed over the
// ranks on the aux stream while the next group's SYRK runs.  The compute stream waits for the last
// sum before the call returns, so later work sees the combined K.  Paths without column groups
// (split-K grids, the tuning variants, the f32 MFMA fallbacks) run the SYRK whole and sum after it.
// syrk_done (optional hipEvent_t) is recorded on the compute stream after the last group's SYRK.
static int g_last_groups = 0;  // column groups of the last overlapped collective (read-only hook "overlap_groups")

// Events of one overlapped collective: compute-stream events the aux stream waits on before each
// group's sum, then one aux event the compute stream waits on; destroyed at the end.
// The RCCL calls of the last K-tile collective (read-only hooks "overlap_calls" / "overlap_sig":
// their number and a hash of their element ranges -- tests check every rank issues the same ones)
static int g_last_sum_calls = 0;
static uint64_t g_last_sum_sig = 0;
static int g_last_sum_sig31 = 0;  // its low 31 bits, as the hook reports them

struct OverlapSums {
    Device& d;
    int collective, root, dtype;
    std::vector<hipEvent_t> evs;
    OverlapSums(Device& dev, int coll, int rt, int dt) : d(dev), collective(coll), root(rt), dtype(dt) {
        g_last_sum_calls = 0;
        set_sig(1469598103934665603ull);
    }
    static void set_sig(uint64_t s) {
        g_last_sum_sig = s;
        g_last_sum_sig31 = (int)(s & 0x7fffffff);
    }
    ~OverlapSums() {
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
    }
    hipEvent_t event() {
        hipEvent_t e;
        SNPMI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        evs.push_back(e);
        return e;
    }
    // the tiles of 128-tile columns [t0, t1) are final on the compute stream: sum them on aux
    void range(void* tiles, uint64_t n, uint64_t t0, uint64_t t1) {
        if (!collective) return;
        const uint64_t nt = n_tiles_1d(n);
        auto T = [&](uint64_t t) { t = std::min(t, nt); return t * (t + 1) / 2 * (uint64_t)(kTile * kTile); };
        const uint64_t e0 = T(t0), e1 = T(t1);
        if (e1 <= e0) return;
        g_last_sum_calls++;
        set_sig((g_last_sum_sig ^ (e0 * 0x9E3779B97F4A7C15ull + e1)) * 1099511628211ull);
        hipEvent_t e = event();
        SNPMI_HIP(hipEventRecord(e, d.stream));
        SNPMI_HIP(hipStreamWaitEvent(d.aux, e, 0));
        rccl_sum_on((uint8_t*)tiles + e0 * dtype_size(dtype), e1 - e0, dtype, root, d.aux);
    }
    void join() {
        if (!collective) return;
        hipEvent_t e = event();
        SNPMI_HIP(hipEventRecord(e, d.aux));
        SNPMI_HIP(hipStreamWaitEvent(d.stream, e, 0));
    }
};

// Whether the last SYRK of an f32 GRM can run as column groups (launch_syrk_packed_h2_cols) --
// decided from state every rank shares (n, parts, the kernel configuration), never from the rank's
// own SNP count: ranks whose spans differ by a SNP, or that own none, must issue the same RCCL
// calls.  The split-K check uses the largest chunk: a chunk of fewer SNPs only narrows
// the slice counts bf3_split_slices may choose, so "no split at 65536" holds for every chunk.
static bool f32_groupable(Device& d, uint64_t n, int parts) {
    return n > 0 && syrk_f32_path() == F32Path::H2 && g_diag_exact && parts > 1 &&
           bf3_split_slices(n, 1ull << 16, d.cu_count) == 1 && ceil_div(n, 256) < 65536;
}

// The K-tile collective of one session as RCCL calls: 128-tile column ranges [t0, t1) of the
// triangle, each one in-place sum.  f32: the column groups of the overlapped SYRK; f64 on the CRT
// path: its column-aligned residue chunks; otherwise one range over the whole triangle.  Every path
// that sums a session's tiles (overlapped or not, with or without SNPs on this rank) issues exactly
// these calls, in this order.
struct SumPlan {
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    bool grouped = false;  // the ranges are the overlapped SYRK's groups
};
static SumPlan sum_plan(Device& d, uint64_t n, int dtype, int parts) {
    SumPlan p;
    if (dtype == SNPMI_DT_F32 && f32_groupable(d, n, parts)) {
        for (const auto& g : column_groups(ceil_div(n, 256), parts)) p.ranges.push_back({2 * g.c0, 2 * g.c1});
        p.grouped = true;
    } else if (dtype == SNPMI_DT_F64 && syrk_f64_path() == F64Path::CRT && n > 0) {
        for (const auto& c : crt_column_chunks(n, crt_res_bytes(whole_dest(nullptr, n).blocks)))
            p.ranges.push_back({2 * c.first, 2 * c.second});
        p.grouped = true;
    } else {
        p.ranges.push_back({0, n_tiles_1d(n)});
    }
    return p;
}

// The plan's sums after everything enqueued so far on the compute stream (aux stream, then the
// compute stream waits for the last one)
static void sum_by_plan(Device& d, const SumPlan& p, void* tiles, uint64_t n, int collective, int rt, int dtype) {
    OverlapSums sums(d, collective, rt, dtype);
    for (const auto& r : p.ranges) sums.range(tiles, n, r.first, r.second);
    sums.join();
}

// The overlapped last SYRK of an f32 GRM: `cnt` SNPs (device codes + f32 LUT) added into `tiles`
// in column groups (launch_syrk_packed_h2_cols, K bit-identical to one launch) with the exact
// diagonal written back per group, each group's tiles summed over the ranks on the aux stream
// under the next group's SYRK.  Returns the group count.
static int grouped_reduce_f32(Device& d, const uint8_t* src, uint64_t pitch, uint64_t n, uint64_t cnt,
                              const float* lut, float* tiles, int acc, int collective, int rt, int parts,
                              hipEvent_t syrk_done) {
    H2Lut h2;
    const uint32_t* l3 = lut_bf3(d, lut, cnt, &h2);
    double* diag = (double*)d.get(Device::S_DIAG, diag_scratch_bytes(n, cnt));
    launch_diag_begin(tiles, n, nullptr, acc, diag, d.stream);
    launch_diag_sq(src, pitch, n, cnt, lut, diag, d.stream);
    const auto groups = column_groups(ceil_div(n, 256), parts);
    OverlapSums sums(d, collective, rt, SNPMI_DT_F32);
    for (const auto& gr : groups) {
        launch_syrk_packed_h2_cols(src, pitch, n, cnt, l3, tiles, acc, d.stream, &h2, gr.L0, gr.L1);
        // block columns [c0, c1): diagonal iids [256 c0, 256 c1), 128-tile columns [2 c0, 2 c1)
        launch_diag_patch(tiles, n, 256 * gr.c0, 256 * gr.c1, nullptr, diag, d.stream);
        sums.range(tiles, n, 2 * gr.c0, 2 * gr.c1);
    }
    if (syrk_done) SNPMI_HIP(hipEventRecord(syrk_done, d.stream));
    sums.join();
    return (int)groups.size();
}

// f64 counterpart: the groups are the CRT path's residue chunks of the last <= crt_max_snps() SNPs
// (launch_syrk_crt cuts them at block-column boundaries when given after_chunk; ~5 at 50k
// iids, so no extra launch boundary), each chunk's f64 tiles summed on the aux stream once its
// CRT reconstruction is done.  The f64-MFMA fallback of a non-finite LUT (gated on the device
// flag) runs before the chunks, so every sum sees final tiles.
static int crt_reduce_f64(Device& d, const uint8_t* src, uint64_t pitch, uint64_t n, uint64_t cnt, const double* lut,
                          double* tiles, int acc, int collective, int rt, hipEvent_t syrk_done) {
    const uint64_t step = crt_max_snps();
    const GrmDest o = whole_dest(tiles, n);
    if (cnt > step) {  // the leading SNPs the plain way, the last <= step overlapped
        const uint64_t lead = ((cnt - 1) / step) * step;
        syrk_f64_steps(d, {src, pitch, n}, {nullptr, 0, 0}, lead, lut, o, acc);
        src += lead * pitch;
        lut += 4 * lead;
        cnt -= lead;
        acc = 1;
    }
    const CrtScratch s = crt_scratch(d, o.blocks, cnt, n, 0);
    const SumPlan plan = sum_plan(d, n, SNPMI_DT_F64, 1);
    OverlapSums sums(d, collective, rt, SNPMI_DT_F64);
    size_t groups = 0;
    const std::function<void()> pre = [&] {
        launch_syrk_packed(src, pitch, n, cnt, lut, SNPMI_DT_F64, o, acc, d.stream, s.gate());
    };
    const std::function<void(uint64_t, uint64_t)> after = [&](uint64_t c0, uint64_t c1) {
        SNPMI_REQUIRE(groups < plan.ranges.size() && plan.ranges[groups] == std::make_pair(2 * c0, 2 * c1),
                      SNPMI_E_ARG, "CRT chunks differ from the collective plan");
        groups++;
        sums.range(tiles, n, 2 * c0, 2 * c1);
    };
    launch_syrk_crt({src, pitch, n}, {nullptr, 0, 0}, cnt, lut, tiles, acc, s.ws, s.res, s.res_bytes, s.rec, d.stream,
                    &pre, &after);
    SNPMI_REQUIRE(groups == plan.ranges.size(), SNPMI_E_ARG, "CRT chunks differ from the collective plan");
    if (syrk_done) SNPMI_HIP(hipEventRecord(syrk_done, d.stream));
    sums.join();
    return (int)groups;
}

// the session's collective after an unoverlapped add (or on a rank without SNPs): the same RCCL
// calls as the overlapped path (sum_plan); zeros join the sum if nothing was added
template <typename T>
static void session_sum_planned(Device& d, int collective, int rt, int parts, hipEvent_t syrk_done) {
    T* t = (T*)session_tiles(d);
    const uint64_t count = n_tiles_upper(g_session.n) * kTile * kTile;
    if (!g_session.wrote) {
        SNPMI_HIP(hipMemsetAsync(t, 0, count * sizeof(T), d.stream));
        g_session.wrote = true;
    }
    if (syrk_done) SNPMI_HIP(hipEventRecord(syrk_done, d.stream));
    if (collective) sum_by_plan(d, sum_plan(d, g_session.n, DT<T>::v, parts), t, g_session.n, collective, rt, DT<T>::v);
}

template <typename T>
static void check_reduce_args(int collective, int parts) {
    session_check_dtype(DT<T>::v);
    SNPMI_REQUIRE(collective >= 0 && collective <= 2, SNPMI_E_ARG, "collective must be 0 (none), 1 (reduce), 2 (all-reduce)");
    SNPMI_REQUIRE(collective == 0 || rccl_ready(), SNPMI_E_ARG, "RCCL communicator not initialised");
    SNPMI_REQUIRE(parts >= 1, SNPMI_E_ARG, "parts must be >= 1");
}

// snpmi_grm_add_packed_{f32,f64} (the session's last add) + the K-tile collective, overlapped:
// the last SNP chunk of for_packed_chunks runs through grouped_reduce_f32 /
// crt_reduce_f64.  Host stats, or a path without groups, add first and sum after.
template <typename T>
static void grm_add_packed_reduce_impl(const PackedSnps& ps, const StdArgs& sa, T* stats, int collective, int root,
                                       int parts, hipEvent_t syrk_done) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    check_reduce_args<T>(collective, parts);
    Device& d = device();
    const int rt = collective == 1 ? root : -1;
    const uint64_t n = ps.n, pitch = ps.pitch;
    const bool grouped = ps.m > 0 && n > 0 && n == g_session.n && sum_plan(d, n, DT<T>::v, parts).grouped &&
                         (sa.kind == SNPMI_STD_NONE || (stats && is_device_ptr(d, stats)));
    g_last_groups = 1;
    if (!grouped) {
        grm_add_packed_impl<T>(ps, sa, stats);
        session_sum_planned<T>(d, collective, rt, parts, syrk_done);
        return;
    }
    check_packed_args(ps, sa, stats);
    for_packed_chunks(d, ps, sa, stats, [&](const uint8_t* src, uint64_t cnt, const T* lut, bool last) {
        if (!last) return session_add_chunk(d, src, pitch, cnt, lut);
        T* tiles = (T*)session_tiles(d);
        const int acc = g_session.wrote ? 1 : 0;
        g_session.wrote = true;
        if constexpr (std::is_same<T, double>::value)
            g_last_groups = crt_reduce_f64(d, src, pitch, n, cnt, lut, tiles, acc, collective, rt, syrk_done);
        else
            g_last_groups = grouped_reduce_f32(d, src, pitch, n, cnt, lut, tiles, acc, collective, rt, parts, syrk_done);
    });
}

// snpmi_grm_add_bed_{f32,f64} (the session's last add: a rank's SNP span of a .bed) + the K-tile
// collective, overlapped the same way on the file stream's last chunk.
template <typename T>
static void grm_add_bed_reduce_impl(const BedSel& s, const StdArgs& sa, T* stats, int collective, int root,
                                    int parts) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    check_reduce_args<T>(collective, parts);
    session_check_iids(s.n_out);
    Device& d = device();
    const int rt = collective == 1 ? root : -1;
    const uint64_t n = g_session.n, total = s.m_out;
    T* tiles = (T*)session_tiles(d);
    uint64_t done = 0;
    int groups = 1;
    const SumPlan plan = sum_plan(d, n, DT<T>::v, parts);
    const bool wrote = grm_stream_bed<T>(
        d, !g_session.wrote, s, sa, stats,
        [&](const uint8_t* packed, uint64_t pitch, uint64_t nn, uint64_t cnt, const T* lut, bool acc) {
            done += cnt;
            const bool last = done == total;
            if (last && plan.grouped) {
                if constexpr (std::is_same<T, double>::value)
                    groups = crt_reduce_f64(d, packed, pitch, nn, cnt, lut, tiles, acc, collective, rt, nullptr);
                else
                    groups = grouped_reduce_f32(d, packed, pitch, nn, cnt, lut, tiles, acc, collective, rt, parts,
                                                nullptr);
                return;
            }
            syrk_packed_auto(d, packed, pitch, nn, cnt, lut, DT<T>::v, whole_dest(tiles, nn), acc);
            if (last && collective) sum_by_plan(d, plan, tiles, n, collective, rt, DT<T>::v);
        });
    g_last_groups = groups;
    if (wrote && done == total) {
        g_session.wrote = true;
        return;  // the last chunk summed the tiles
    }
    session_sum_planned<T>(d, collective, rt, parts, nullptr);  // no SNP on this rank: zeros join the sum
}

// ---------------------------------------------------------------------- rect GRM: K[rows, cols] directly
// K[rows, cols] = Z[rows] Z[cols]^T without the whole K (the reference slices the N x N K,
// kernelreader/snpkernel.py:84-88).  Each SNP chunk is repacked to the rows and to the cols
// (launch_repack; an identity side is read in place) and the two-operand kernels write the
// ceil(n_r / 256) x ceil(n_c / 256) dense blocks.  Stats and the LUT come from all the reader's iids.

// positions (r, c) with rows[r] == cols[c]: the diagonal elements of K inside the rectangle
// (idx == nullptr: the identity list).  Repeats give every combination.
static void rect_diag_pairs(const uint64_t* ri, uint64_t nr, const uint64_t* ci, uint64_t nc,
                            std::vector<uint32_t>& pairs) {
    pairs.clear();
    if (nr == 0 || nc == 0) return;
    SNPMI_REQUIRE(nr < (1ull << 32) && nc < (1ull << 32), SNPMI_E_ARG, "rect GRM: too many rows / cols");
    if (!ci) {
        for (uint64_t r = 0; r < nr; r++) {
            const uint64_t i = ri ? ri[r] : r;
            if (i < nc) pairs.push_back((uint32_t)r), pairs.push_back((uint32_t)i);
        }
        return;
    }
    std::vector<uint32_t> order(nc);
    for (uint64_t c = 0; c < nc; c++) order[c] = (uint32_t)c;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ci[x] < ci[y]; });
    for (uint64_t r = 0; r < nr; r++) {
        const uint64_t i = ri ? ri[r] : r;
        auto it = std::lower_bound(order.begin(), order.end(), i, [&](uint32_t x, uint64_t v) { return ci[x] < v; });
        for (; it != order.end() && ci[*it] == i; ++it) pairs.push_back((uint32_t)r), pairs.push_back(*it);
    }
}

// one side (rows or cols) of a rect call: its index list on the device and the repack plan
struct RectSide {
    uint64_t n = 0, n_src = 0, pitch = 0;
    bool identity = true;
    uint64_t* idx_dev = nullptr;
    RepackPlan plan;
    Device::Slot dst = Device::S_RECT_A;
};

static RectSide rect_side(Device& d, const uint64_t* idx, uint64_t n_sel, uint64_t n_src, int which) {
    RectSide s;
    SNPMI_REQUIRE(idx || n_sel == n_src || n_sel == 0, SNPMI_E_ARG, "rect GRM: a NULL index list means all iids");
    for (uint64_t k = 0; idx && k < n_sel; k++) SNPMI_REQUIRE(idx[k] < n_src, SNPMI_E_INDEX, "iid index out of range");
    s.n = n_sel;
    s.n_src = n_src;
    s.pitch = packed_pitch(n_sel);
    s.identity = n_sel == n_src && is_identity(idx, n_sel, n_src);
    s.dst = which ? Device::S_RECT_B : Device::S_RECT_A;
    if (!s.identity && n_sel) {
        s.idx_dev = (uint64_t*)d.get(which ? Device::S_RECT_IDX_B : Device::S_RECT_IDX_A, n_sel * 8);
        SNPMI_HIP(hipMemcpyAsync(s.idx_dev, idx, n_sel * 8, hipMemcpyHostToDevice, d.stream));
        uint32_t* plan = (uint32_t*)d.get(which ? Device::S_RECT_PLAN_B : Device::S_RECT_PLAN_A,
                                          repack_plan_entries(n_sel) * 4);
        uint32_t* win = (uint32_t*)d.get(which ? Device::S_RECT_WIN_B : Device::S_RECT_WIN_A,
                                         repack_win_entries(n_sel) * 4);
        s.plan = launch_repack_plan(s.idx_dev, n_sel, n_src, plan, win, d.stream);
        SNPMI_HIP(hipStreamSynchronize(d.stream));  // idx is the caller's host memory
    }
    return s;
}

// the side's operand for one SNP chunk: the chunk itself (identity) or its repack
static const uint8_t* rect_operand(Device& d, const RectSide& s, const uint8_t* packed, uint64_t pitch, uint64_t cnt,
                                   uint64_t* pitch_out) {
    if (s.identity) {
        *pitch_out = pitch;
        return packed;
    }
    uint8_t* dst = (uint8_t*)d.get(s.dst, cnt * s.pitch);
    launch_repack(packed, pitch, s.n_src, s.idx_dev, s.plan, s.n, cnt, dst, s.pitch, d.stream);
    *pitch_out = s.pitch;
    return dst;
}

// diagonal pairs on the device: npairs x (r, c) u32, then npairs f64 of saved values
struct RectPairs {
    const uint32_t* pairs = nullptr;
    double* saved = nullptr;
    uint64_t n = 0;
};
static RectPairs rect_pairs_upload(Device& d, const uint32_t* host_pairs, uint64_t npairs) {
    RectPairs p;
    if (npairs == 0) return p;
    uint8_t* base = (uint8_t*)d.get(Device::S_RECT_PAIRS, npairs * 16);
    SNPMI_HIP(hipMemcpyAsync(base, host_pairs, npairs * 8, hipMemcpyHostToDevice, d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
    p.pairs = (const uint32_t*)base;
    p.saved = (double*)(base + npairs * 8);
    p.n = npairs;
    return p;
}

// blocks (+)= Za Zb^T of one SNP block: f64 in the steps of syrk_f64_steps, f32 on the fp16x2 /
// bf16x3 chain with the exact diagonal
// of the matched positions (hook "diag"), as syrk_packed_auto does for the whole K
static void syrk_rect_auto(Device& d, const uint8_t* Pa, uint64_t pitch_a, uint64_t na, const uint8_t* Pb,
                           uint64_t pitch_b, uint64_t nb, uint64_t m, const void* lut, int dt, void* blocks,
                           int accumulate, const RectPairs& dp) {
    const uint64_t g = rect_blocks(na, pitch_a, nb, pitch_b);
    if (g == 0) return;
    if (m == 0) {
        if (!accumulate) SNPMI_HIP(hipMemsetAsync(blocks, 0, g * 65536 * dtype_size(dt), d.stream));
        return;
    }
    if (dt == SNPMI_DT_F64) {
        syrk_f64_steps(d, {Pa, pitch_a, na}, {Pb, pitch_b, nb}, m, (const double*)lut, {blocks, nullptr, nullptr, g},
                       accumulate);
        return;
    }
    H2Lut h2;
    const bool h = syrk_f32_path() == F32Path::H2;
    const uint32_t* l3 = lut_bf3(d, (const float*)lut, m, h ? &h2 : nullptr);
    const bool exact = g_diag_exact && dp.n > 0;
    if (exact) launch_rect_diag_save((const float*)blocks, ceil_div(na, 256), dp.pairs, dp.n, accumulate, dp.saved, d.stream);
    launch_syrk_rect_f32(Pa, pitch_a, na, Pb, pitch_b, nb, m, l3, h ? &h2 : nullptr, (float*)blocks, accumulate, d.stream);
    if (exact) {
        double* sq = (double*)d.get(Device::S_DIAG, diag_scratch_bytes(na, m));
        SNPMI_HIP(hipMemsetAsync(sq, 0, round_up(na, 16) * sizeof(double), d.stream));
        launch_diag_sq(Pa, pitch_a, na, m, (const float*)lut, sq, d.stream);
        launch_rect_diag_patch((float*)blocks, ceil_div(na, 256), dp.pairs, dp.n, dp.saved, sq, d.stream);
    }
}

static uint64_t rect_bytes(uint64_t nr, uint64_t nc, int dt) {
    return ceil_div(nr, 256) * ceil_div(nc, 256) * 65536 * dtype_size(dt);
}

// blocks -> K_out[n_r][n_c] (host or device), modelled on grm_finish: one launch for a device
// K_out, <= 1 GiB staging blocks of the slow axis for a host K_out
template <typename T>
static void rect_extract(Device& d, const T* blocks, uint64_t nr, uint64_t nc, int order_c, double scale, T* K_out) {
    if (nr * nc == 0) return;
    const uint64_t outer = order_c ? nr : nc, inner = order_c ? nc : nr, nba = ceil_div(nr, 256);
    const bool dev = is_device_ptr(d, K_out);
    const uint64_t per = dev ? outer : std::max<uint64_t>(1, std::min<uint64_t>(outer, (1ull << 30) / (inner * sizeof(T))));
    for (uint64_t o0 = 0; o0 < outer; o0 += per) {
        const uint64_t no = std::min(per, outer - o0);
        T* dk = dev ? K_out : (T*)d.get(Device::S_K, no * inner * sizeof(T));
        launch_rect_extract(blocks, DT<T>::v, nba, inner, o0, no, order_c, scale, dk, d.stream);
        if (!dev)
            d2h_rows(d, K_out + o0 * inner, inner * sizeof(T), dk, inner * sizeof(T), inner * sizeof(T), no,
                     resolve_threads(0));
    }
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

struct RectSession {
    bool active = false;
    bool wrote = false;
    uint64_t nr = 0, nc = 0;
    int dtype = SNPMI_DT_F32;
};
static RectSession g_rect;

static void* rect_session_blocks(Device& d) { return d.get(Device::S_RECT, rect_bytes(g_rect.nr, g_rect.nc, g_rect.dtype)); }

template <typename T>
static void rect_check_session(uint64_t n, const uint64_t* row_idx, const uint64_t* col_idx) {
    SNPMI_REQUIRE(g_rect.active, SNPMI_E_ARG, "no rect GRM session (call snpmi_grm_rect_begin)");
    SNPMI_REQUIRE(g_rect.dtype == DT<T>::v, SNPMI_E_ARG, "dtype differs from snpmi_grm_rect_begin");
    SNPMI_REQUIRE(row_idx || g_rect.nr == n || g_rect.nr == 0, SNPMI_E_ARG, "row count differs from snpmi_grm_rect_begin");
    SNPMI_REQUIRE(col_idx || g_rect.nc == n || g_rect.nc == 0, SNPMI_E_ARG, "col count differs from snpmi_grm_rect_begin");
}

// the sides, the diagonal pairs and the per-chunk multiply of one add call
struct RectAdd {
    RectSide rows, cols;
    RectPairs dp;
    void* blocks = nullptr;
};
template <typename T>
static RectAdd rect_add_begin(Device& d, uint64_t n, const uint64_t* row_idx, const uint64_t* col_idx) {
    RectAdd a;
    a.rows = rect_side(d, row_idx, g_rect.nr, n, 0);
    a.cols = rect_side(d, col_idx, g_rect.nc, n, 1);
    (void)rect_blocks(g_rect.nr, a.rows.pitch, g_rect.nc, a.cols.pitch);
    if (DT<T>::v == SNPMI_DT_F32 && g_diag_exact) {
        std::vector<uint32_t> pairs;
        rect_diag_pairs(row_idx, g_rect.nr, col_idx, g_rect.nc, pairs);
        a.dp = rect_pairs_upload(d, pairs.data(), pairs.size() / 2);
    }
    a.blocks = rect_session_blocks(d);
    return a;
}
template <typename T>
static void rect_add_chunk(Device& d, const RectAdd& a, const uint8_t* packed, uint64_t pitch, uint64_t cnt,
                           const T* lut) {
    if (g_rect.nr == 0 || g_rect.nc == 0 || cnt == 0) return;
    uint64_t pa = 0, pb = 0;
    const uint8_t* A = rect_operand(d, a.rows, packed, pitch, cnt, &pa);
    const uint8_t* B = rect_operand(d, a.cols, packed, pitch, cnt, &pb);
    syrk_rect_auto(d, A, pa, g_rect.nr, B, pb, g_rect.nc, cnt, lut, DT<T>::v, a.blocks, g_rect.wrote ? 1 : 0, a.dp);
    g_rect.wrote = true;
}

template <typename T>
static void rect_add_packed_impl(const PackedSnps& ps, const StdArgs& sa, T* stats, const uint64_t* row_idx,
                                 const uint64_t* col_idx) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    rect_check_session<T>(ps.n, row_idx, col_idx);
    check_packed_args(ps, sa, stats);
    Device& d = device();
    const RectAdd ra = rect_add_begin<T>(d, ps.n, row_idx, col_idx);
    // the chunks of snpmi_grm_add_packed_*: the same launch boundaries as the whole-K session
    for_packed_chunks(d, ps, sa, stats, [&](const uint8_t* src, uint64_t cnt, const T* lut, bool) {
        rect_add_chunk<T>(d, ra, src, ps.pitch, cnt, lut);
    });
    if (ps.m > 0 && ps.n > 0) SNPMI_HIP(hipStreamSynchronize(d.stream));
}

template <typename T>
static void rect_add_bed_impl(const BedSel& s, const StdArgs& sa, T* stats, const uint64_t* row_idx,
                              const uint64_t* col_idx) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    rect_check_session<T>(s.n_out, row_idx, col_idx);
    Device& d = device();
    const RectAdd ra = rect_add_begin<T>(d, s.n_out, row_idx, col_idx);
    grm_stream_bed<T>(d, false, s, sa, stats,
                      [&](const uint8_t* packed, uint64_t pitch, uint64_t nn, uint64_t cnt, const T* lut, bool) {
                          rect_add_chunk<T>(d, ra, packed, pitch, cnt, lut);
                      });
}

// ---------------------------------------------------------------------- partitioned GRM (cfg5)
// K too large to replicate: part `rank` of `world` owns the 256x256 blocks of its layout table
// (syrk.hip part_layout, part_tables above) and nothing else of K.

// host copy of the last part layout asked for (snpmi_grm_part_coords is called per block)
static std::mutex g_layout_mutex;
static std::vector<uint32_t> g_layout;
static uint64_t g_layout_key[3] = {~0ull, 0, 0};
static const std::vector<uint32_t>& host_layout(uint64_t nb, int rank, int world) {
    if (g_layout_key[0] != nb || g_layout_key[1] != (uint64_t)rank || g_layout_key[2] != (uint64_t)world) {
        part_layout(nb, rank, world, g_layout);
        g_layout_key[0] = nb;
        g_layout_key[1] = (uint64_t)rank;
        g_layout_key[2] = (uint64_t)world;
    }
    return g_layout;
}

// From a file: rank part_rank of part_world streams EVERY SNP of the .bed (stats need all iids of
// a SNP; each rank computes them itself -- no exchange) and accumulates only its own blocks
// (snpmi_grm_part_coords) in HBM, then copies them to blocks_out (n_local x 65536 values,
// row-major blocks; may be a memory-mapped file).
template <typename T>
static void grm_part_bed_impl(const BedSel& s, const StdArgs& sa, T* stats, int part_rank, int part_world,
                              T* blocks_out) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    check_part(part_rank, part_world, "bad rank / world");
    const uint64_t nloc = grm_part_blocks(s.n_out, part_rank, part_world);
    SNPMI_REQUIRE(blocks_out != nullptr || nloc == 0, SNPMI_E_ARG, "blocks_out is NULL");
    Device& d = device();
    const uint64_t bytes = std::max<uint64_t>(nloc, 1) * 256 * 256 * sizeof(T);
    // blocks_out in device memory: the SYRK accumulates into it directly (K stays in HBM, no
    // scratch, no copy-out); host memory: scratch tiles + a pinned-bounce copy at the end
    const bool dev_out = nloc && is_device_ptr(d, blocks_out);
    T* blocks = dev_out ? blocks_out : (T*)d.get(Device::S_TILES, bytes);
    const bool wrote = grm_stream_bed<T>(
        d, true, s, sa, stats,
        [&](const uint8_t* packed, uint64_t pitch, uint64_t n, uint64_t cnt, const T* lut, bool acc) {
            syrk_packed_auto(d, packed, pitch, n, cnt, lut, DT<T>::v, part_dest(blocks, n, part_rank, part_world), acc);
        });
    if (!wrote) SNPMI_HIP(hipMemsetAsync(blocks, 0, dev_out ? nloc * 256 * 256 * sizeof(T) : bytes, d.stream));
    const size_t bb = 256 * 256 * sizeof(T);  // one block per "row" of the pinned-bounce copy
    if (nloc && !dev_out) d2h_rows(d, blocks_out, bb, blocks, bb, bb, nloc, resolve_threads(s.num_threads));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

// snpmi_dev_syrk_packed_part{,_f64}: one SNP block already in HBM into a part's blocks
static void dev_syrk_packed_part(int dtype, const uint8_t* packed, uint64_t pitch, uint64_t n, uint64_t m,
                                 const void* lut, int part_rank, int part_world, void* blocks, int accumulate) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);  // shared scratch slots
    check_part(part_rank, part_world);
    check_pitch(pitch, n);
    syrk_packed_auto(device(), packed, pitch, n, m, lut, dtype, part_dest(blocks, n, part_rank, part_world), accumulate);
}

// K[ri, ci] restricted to part `part_rank`'s blocks (the rest 0): the parts' outputs summed over
// the ranks are the sub-matrix (snpmi_grm_part_extract_*, the PartitionedKernel reader)
template <typename T>
static void part_extract_impl(const T* blocks, uint64_t n, int part_rank, int part_world, const uint64_t* ri,
                              uint64_t nr, const uint64_t* ci, uint64_t nc, int order_c, double scale, T* out) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    check_part(part_rank, part_world);
    SNPMI_REQUIRE(out != nullptr || nr * nc == 0, SNPMI_E_ARG, "out is NULL");
    Device& d = device();
    const uint64_t nloc = grm_part_blocks(n, part_rank, part_world);
    SNPMI_REQUIRE(nloc == 0 || (blocks && is_device_ptr(d, blocks)), SNPMI_E_ARG,
                  "blocks must be device memory of the current device");
    for (uint64_t k = 0; ri && k < nr; k++) SNPMI_REQUIRE(ri[k] < n, SNPMI_E_INDEX, "iid0 index out of range");
    for (uint64_t k = 0; ci && k < nc; k++) SNPMI_REQUIRE(ci[k] < n, SNPMI_E_INDEX, "iid1 index out of range");
    SNPMI_REQUIRE(ri || nr <= n, SNPMI_E_INDEX, "iid0 count exceeds n");
    SNPMI_REQUIRE(ci || nc <= n, SNPMI_E_INDEX, "iid1 count exceeds n");
    if (nr * nc == 0) return;
    const PartTables pt = part_tables(ceil_div(n, 256), part_rank, part_world);
    uint64_t* dri = nullptr;
    uint64_t* dci = nullptr;
    if (ri) {
        dri = (uint64_t*)d.get(Device::S_IDX, nr * 8);
        SNPMI_HIP(hipMemcpyAsync(dri, ri, nr * 8, hipMemcpyHostToDevice, d.stream));
    }
    if (ci) {
        dci = (uint64_t*)d.get(Device::S_IDX2, nc * 8);
        SNPMI_HIP(hipMemcpyAsync(dci, ci, nc * 8, hipMemcpyHostToDevice, d.stream));
    }
    const bool dev = is_device_ptr(d, out);
    T* o = dev ? out : (T*)d.get(Device::S_K, nr * nc * sizeof(T));
    launch_part_extract(blocks, pt.lslot, DT<T>::v, dri, nr, dci, nc, order_c, scale, o, d.stream);
    if (!dev) SNPMI_HIP(hipMemcpyAsync(out, o, nr * nc * sizeof(T), hipMemcpyDeviceToHost, d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}

template <typename T>
static void part_trace_impl(const T* blocks, uint64_t n, int part_rank, int part_world, double* trace) {
    std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
    check_part(part_rank, part_world);
    SNPMI_REQUIRE(trace != nullptr, SNPMI_E_ARG, "trace is NULL");
    Device& d = device();
    *trace = 0.0;
    if (n == 0 || grm_part_blocks(n, part_rank, part_world) == 0) return;
    SNPMI_REQUIRE(blocks && is_device_ptr(d, blocks), SNPMI_E_ARG, "blocks must be device memory of the current device");
    const PartTables pt = part_tables(ceil_div(n, 256), part_rank, part_world);
    double* tr = (double*)d.get(Device::S_RED, 64);
    launch_part_trace(blocks, pt.dslot, n, DT<T>::v, tr, d.stream);
    SNPMI_HIP(hipMemcpyAsync(trace, tr, 8, hipMemcpyDeviceToHost, d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
}
}  // namespace snpmi

// ====================================================================== exported C ABI
using namespace snpmi;

extern "C" {

const char* snpmi_last_error(void) { return g_last_error.c_str(); }
int snpmi_version(void) { return 1; }

int snpmi_device_count(int* count) {
    return guarded([&] {
        SNPMI_REQUIRE(count != nullptr, SNPMI_E_ARG, "count is NULL");
        *count = num_devices();
        (void)hipGetLastError();
    });
}

int snpmi_set_device(int dev) {
    return guarded([&] {
        SNPMI_REQUIRE(dev >= 0 && dev < num_devices(), SNPMI_E_ARG, "device index out of range");
        g_cur_dev = dev;
        (void)device();
    });
}

int snpmi_get_device(int* dev) {
    return guarded([&] {
        SNPMI_REQUIRE(dev != nullptr, SNPMI_E_ARG, "dev is NULL");
        *dev = g_cur_dev < 0 ? default_device() : g_cur_dev;
    });
}

int snpmi_release_cache(void) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
        std::lock_guard<std::mutex> lk2(g_dev_mutex);
        for (Device* d : g_devices)
            if (d) {
                SNPMI_HIP(hipSetDevice(d->id));
                SNPMI_HIP(hipStreamSynchronize(d->stream));
                d->release();
            }
        release_pinned();
    });
}

int snpmi_device_info(int dev, char* name, size_t name_len, uint64_t* total_mem, int* cu_count) {
    return guarded([&] {
        hipDeviceProp_t p;
        SNPMI_HIP(hipGetDeviceProperties(&p, dev));
        if (name && name_len) {
            std::strncpy(name, p.gcnArchName, name_len - 1);
            name[name_len - 1] = 0;
        }
        if (total_mem) *total_mem = p.totalGlobalMem;
        if (cu_count) *cu_count = p.multiProcessorCount;
    });
}

int snpmi_device_ids(int dev, uint8_t* uuid16, int* pci, int* clock_khz) {
    return guarded([&] {
        hipDeviceProp_t p;
        SNPMI_HIP(hipGetDeviceProperties(&p, dev));
        if (uuid16) std::memcpy(uuid16, p.uuid.bytes, 16);
        if (pci) {
            pci[0] = p.pciDomainID;
            pci[1] = p.pciBusID;
            pci[2] = p.pciDeviceID;
        }
        if (clock_khz) *clock_khz = p.clockRate;
    });
}

// The tuning / test hooks: name, where the value lives, what a set does with a value.  ANY keeps
// it, BOOL stores value != 0, CLAMP0 stores max(value, 0), RANGE / LIST reject a value outside
// [lo, hi] / {list} with `what` (the stored value is then unchanged), READ_ONLY rejects every set.
struct Hook {
    const char* name;
    int* value;
    enum Kind { ANY, BOOL, CLAMP0, RANGE, LIST, READ_ONLY } kind;
    int lo, hi;  // RANGE
    std::vector<int> list;
    const char* what;  // RANGE / LIST: the accepted values, for the error message
};
static const std::vector<Hook>& hooks() {
    static const std::vector<Hook> table = {
        // launch_snp_stats: 6 = one wave per SNP, 7 / 9 = 4 / 16 loads in flight, 8 = 2 waves per SNP;
        // launch_decode: 2 = no 16-B row-tile kernel, 3 = the 64x64 LDS-tile kernel;
        // launch_decode_std_fused: 1 = the two-kernel form; launch_repack_plan: 8 = no windows,
        // 9 / 10 = chunks of 16384 / 4096 codes, 11 = two columns per group, 17 = dword-per-lane gather
        {"decode", &g_variant_decode, Hook::ANY, 0, 0, {}, nullptr},
        // dense standardize: 0 = k_std_cols_f / k_std_cols_c16, 1 = round 3's kernels
        {"std", &g_variant_std, Hook::ANY, 0, 0, {}, nullptr},
        // 1 = exact f64 diagonal around every f32 SYRK (k_diag_*), 0 = the SYRK's own diagonal
        {"diag", &g_diag_exact, Hook::BOOL, 0, 0, {}, nullptr},
        // whole-K extraction: 0 = k_grm_extract_sym, 1 = k_grm_extract_rows, 2-4 = other block
        // shapes, 5-7 = the pipelined kernel in three shapes
        {"extract", &g_variant_extract, Hook::ANY, 0, 0, {}, nullptr},
        // the shipped default chain and the kernels it falls back to (syrk_f32_path / syrk_f64_path):
        // 0 = default; 36 = the bf16x3 kernel alone (fp16x2 range fallback), f64 fused; 20 = 71 = the
        // two-phase f32 / f64 MFMA kernels (dense-operand range fallback; the CRT path's non-finite
        // fallback is the fused f64 kernel); 5 = the fused 128x128 kernels at every N.  The shipped
        // forms' own A/B switches are the hooks "h2" and "crt".
        {"syrk", &g_variant_syrk, Hook::LIST, 0, 0, {0, 5, 20, 36, 71}, "syrk variant: a shipped kernel (0, 5, 20, 36, 71)"},
        // split-K of the default f32 chain: 0 = auto (bf3_split_slices), 1 = off, S = S slices
        {"syrk_split", &g_variant_syrk_split, Hook::ANY, 0, 0, {}, nullptr},
        // dense fp16x2 SYRK: SNPs per stage-image chunk, 0 = by scratch size
        {"dense_chunk", &g_dense_chunk, Hook::CLAMP0, 0, 0, {}, nullptr},
        // 1 = genotype-valued dense operands are re-encoded as codes + LUT, 0 = never
        {"dense_codes", &g_dense_codes, Hook::ANY, 0, 0, {}, nullptr},
        // SNPs per f32 accumulation segment (SegFlush), 0 = one chain per launch
        {"seg", &g_seg_snps, Hook::CLAMP0, 0, 0, {}, nullptr},
        // host gather of .bed columns: 0 = memcpy from the mmap, 1 = pread
        {"gather", &g_gather, Hook::ANY, 0, 0, {}, nullptr},
        {"h2", &g_h2_kernel, Hook::RANGE, 0, 1, {}, "h2 SYRK: 0 = k_syrk_h2, 1 = k_syrk_h2s"},
        {"crt", &g_crt_kernel, Hook::RANGE, 0, 2, {},
         "crt residue SYRK: 0 = k_syrk_i8r, 1 = k_syrk_i8w, 2 = k_syrk_i8w without its read order / wave priorities"},
        {"crt_block", &g_crt_block, Hook::RANGE, 0, 1, {}, "crt moduli: 0 = launch-wide R, 1 = per 256-block"},
        {"f64", &g_f64_mfma, Hook::RANGE, 0, 1, {}, "f64 GRM path: 0 = int8 residues + CRT, 1 = f64 MFMA"},
        // the last K-tile collective: column groups, RCCL calls, 31 bits of the hash of their ranges
        {"overlap_groups", &g_last_groups, Hook::READ_ONLY, 0, 0, {}, nullptr},
        {"overlap_calls", &g_last_sum_calls, Hook::READ_ONLY, 0, 0, {}, nullptr},
        {"overlap_sig", &g_last_sum_sig31, Hook::READ_ONLY, 0, 0, {}, nullptr},
    };
    return table;
}
static const Hook& find_hook(const char* name) {
    for (const Hook& h : hooks())
        if (std::strcmp(name, h.name) == 0) return h;
    throw Error(SNPMI_E_ARG, std::string("unknown kernel ") + name);
}

int snpmi_set_kernel_variant(const char* kernel, int variant) {
    return guarded([&] {
        SNPMI_REQUIRE(kernel != nullptr, SNPMI_E_ARG, "kernel name is NULL");
        const Hook& h = find_hook(kernel);
        const bool ok = h.kind == Hook::RANGE  ? variant >= h.lo && variant <= h.hi
                        : h.kind == Hook::LIST ? std::find(h.list.begin(), h.list.end(), variant) != h.list.end()
                                               : h.kind != Hook::READ_ONLY;
        SNPMI_REQUIRE(ok, SNPMI_E_ARG,
                      h.what ? std::string(h.what) + " (got " + std::to_string(variant) + ")"
                             : std::string("unknown kernel ") + kernel);
        *h.value = h.kind == Hook::BOOL ? variant != 0 : h.kind == Hook::CLAMP0 ? std::max(variant, 0) : variant;
    });
}

int snpmi_get_kernel_variant(const char* kernel, int* variant) {
    return guarded([&] {
        SNPMI_REQUIRE(kernel != nullptr && variant != nullptr, SNPMI_E_ARG, "kernel name or output is NULL");
        *variant = *find_hook(kernel).value;
    });
}

// The ABI spells a .bed selection, packed SNPs in HBM and the standardizer settings as loose
// parameters, under the same names in every entry point (include/snpmi.h).  The parameter lists,
// and the blocks built from them at this boundary:
#define SNPMI_BED_PARAMS                                                                             \
    const char* path, uint64_t n_iid, uint64_t n_sid, int count_a1, const uint64_t* iid_idx, uint64_t n_out_iid, \
        const uint64_t* sid_idx, uint64_t n_out_sid
#define SNPMI_BED_SEL bed_sel(path, n_iid, n_sid, count_a1, iid_idx, n_out_iid, sid_idx, n_out_sid, num_threads)
#define SNPMI_PACKED_PARAMS const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, int count_a1
#define SNPMI_PACKED_SNPS (PackedSnps{{packed, pitch, n_iid}, n_sid, count_a1})
#define SNPMI_STD_PARAMS(T) int std_kind, double a, double b, int use_stats, T* stats
#define SNPMI_STD_ARGS (StdArgs{std_kind, a, b, use_stats})
// Entry points whose _f32 / _f64 (/ _i8) forms differ only in the value type come from one macro.

int snpmi_bed_check(const char* path, uint64_t n_iid, uint64_t n_sid) {
    return guarded([&] {
        BedMap m;
        open_bed(m, path, n_iid, n_sid);
    });
}

#define SNPMI_BED_READ(SUFFIX, T)                                                                                  \
    int snpmi_bed_read_##SUFFIX(SNPMI_BED_PARAMS, int order_c, T* out, int num_threads) {                          \
        return guarded([&] {                                                                                       \
            bed_read_impl<T>(SNPMI_BED_SEL, order_c, {SNPMI_STD_NONE, 0.0, 0.0, 0}, (T*)nullptr, out,              \
                             n_out_iid == 0 || n_out_sid == 0);                                                    \
        });                                                                                                        \
    }
SNPMI_BED_READ(f32, float)
SNPMI_BED_READ(f64, double)
SNPMI_BED_READ(i8, int8_t)

#define SNPMI_BED_READ_STD(SUFFIX, T)                                                                              \
    int snpmi_bed_read_standardize_##SUFFIX(SNPMI_BED_PARAMS, int order_c, SNPMI_STD_PARAMS(T), T* out,            \
                                            int num_threads) {                                                     \
        return guarded([&] {                                                                                       \
            SNPMI_REQUIRE(std_kind == SNPMI_STD_NONE || stats != nullptr, SNPMI_E_ARG, "stats is NULL");          \
            bed_read_impl<T>(SNPMI_BED_SEL, order_c, SNPMI_STD_ARGS, stats, out,                                   \
                             n_out_iid == 0 || n_out_sid == 0);                                                    \
        });                                                                                                        \
    }
SNPMI_BED_READ_STD(f32, float)
SNPMI_BED_READ_STD(f64, double)

#define SNPMI_BED_WRITE(SUFFIX, T)                                                                                 \
    int snpmi_bed_write_##SUFFIX(const char* path, const T* val, uint64_t n_iid, uint64_t n_sid, int order_c,    \
                                 int count_a1, int) {                                                               \
        return guarded([&] { bed_write_impl<T>(path, val, n_iid, n_sid, order_c, count_a1); });                   \
    }
SNPMI_BED_WRITE(f32, float)
SNPMI_BED_WRITE(f64, double)
SNPMI_BED_WRITE(i8, int8_t)

int snpmi_dev_encode(const void* val, int dtype, int order_c, uint64_t ld, uint64_t n_iid, uint64_t n_sid,
                     int count_a1, uint8_t* packed, uint64_t pitch, uint64_t* bad_values) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);  // shared scratch slots
        check_pitch(pitch, n_iid, "pitch must be a multiple of 64 >= ceil(n/4)");
        SNPMI_REQUIRE(order_c || ld % 16 == 0, SNPMI_E_ARG, "F-order ld must be a multiple of 16");
        SNPMI_REQUIRE(order_c ? ld >= n_sid : ld >= n_iid, SNPMI_E_ARG, "ld too small");
        Device& d = device();
        unsigned int* bad_dev = (unsigned int*)d.get(Device::S_RED, 256);
        SNPMI_HIP(hipMemsetAsync(bad_dev, 0, sizeof(unsigned int), d.stream));
        launch_encode(val, dtype, order_c, ld, n_iid, n_sid, count_a1, packed, pitch, bad_dev, d.stream);
        if (bad_values) {
            unsigned int bad = 0;
            SNPMI_HIP(hipMemcpyAsync(&bad, bad_dev, sizeof(bad), hipMemcpyDeviceToHost, d.stream));
            SNPMI_HIP(hipStreamSynchronize(d.stream));
            *bad_values = bad;
        }
    });
}

int snpmi_grm_begin(uint64_t n_out_iid, int dtype) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
        SNPMI_REQUIRE(dtype == SNPMI_DT_F32 || dtype == SNPMI_DT_F64, SNPMI_E_ARG, "GRM dtype must be f32 or f64");
        Device& d = device();
        g_session = GrmSession{true, false, n_out_iid, dtype};
        (void)session_tiles(d);
    });
}

// PARTS: the one thing the pair differs in -- the f64 reduce forms take parts < 1 as 1 (the CRT
// path's own residue chunks are the groups), the f32 forms reject it
#define SNPMI_GRM_ADD(SUFFIX, T, PARTS)                                                                             \
    int snpmi_grm_add_bed_##SUFFIX(SNPMI_BED_PARAMS, SNPMI_STD_PARAMS(T), int num_threads) {                        \
        return guarded([&] {                                                                                         \
            std::lock_guard<std::recursive_mutex> lk(g_call_mutex);                                                  \
            const BedSel s = SNPMI_BED_SEL;                                                                          \
            session_check<T>(s.n_out);                                                                               \
            Device& d = device();                                                                                    \
            T* tiles = (T*)session_tiles(d);                                                                         \
            if (grm_add_bed<T>(d, tiles, !g_session.wrote, s, SNPMI_STD_ARGS, stats)) g_session.wrote = true;        \
        });                                                                                                          \
    }                                                                                                                \
    int snpmi_grm_add_bed_reduce_##SUFFIX(SNPMI_BED_PARAMS, SNPMI_STD_PARAMS(T), int num_threads, int collective,   \
                                          int root, int parts) {                                                     \
        return guarded([&] {                                                                                         \
            grm_add_bed_reduce_impl<T>(SNPMI_BED_SEL, SNPMI_STD_ARGS, stats, collective, root, PARTS);               \
        });                                                                                                          \
    }                                                                                                                \
    int snpmi_grm_add_packed_##SUFFIX(SNPMI_PACKED_PARAMS, SNPMI_STD_PARAMS(T)) {                                   \
        return guarded([&] { grm_add_packed_impl<T>(SNPMI_PACKED_SNPS, SNPMI_STD_ARGS, stats); });                   \
    }                                                                                                                \
    int snpmi_grm_add_packed_reduce_##SUFFIX(SNPMI_PACKED_PARAMS, SNPMI_STD_PARAMS(T), int collective, int root,    \
                                             int parts, void* syrk_done) {                                           \
        return guarded([&] {                                                                                         \
            grm_add_packed_reduce_impl<T>(SNPMI_PACKED_SNPS, SNPMI_STD_ARGS, stats, collective, root, PARTS,         \
                                          (hipEvent_t)syrk_done);                                                    \
        });                                                                                                          \
    }                                                                                                                \
    int snpmi_grm_add_dense_##SUFFIX(const T* val, uint64_t rows, uint64_t cols, int order_c) {                     \
        return guarded([&] { grm_add_dense_impl<T>(val, rows, cols, order_c); });                                    \
    }
SNPMI_GRM_ADD(f32, float, parts)
SNPMI_GRM_ADD(f64, double, std::max(parts, 1))

int snpmi_grm_session_tiles(void** tiles, uint64_t* count) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
        session_check_open();
        Device& d = device();
        void* t = session_tiles(d);
        const uint64_t cnt = n_tiles_upper(g_session.n) * kTile * kTile;
        if (!g_session.wrote) {
            SNPMI_HIP(hipMemsetAsync(t, 0, cnt * dtype_size(g_session.dtype), d.stream));
            SNPMI_HIP(hipStreamSynchronize(d.stream));
            g_session.wrote = true;
        }
        if (tiles) *tiles = t;
        if (count) *count = cnt;
    });
}

int snpmi_grm_session_sum(int collective, int root, int parts) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
        session_check_open();
        Device& d = device();
        const int rt = collective == 1 ? root : -1;
        g_last_groups = 1;
        if (g_session.dtype == SNPMI_DT_F64) {
            check_reduce_args<double>(collective, parts);
            session_sum_planned<double>(d, collective, rt, parts, nullptr);
        } else {
            check_reduce_args<float>(collective, parts);
            session_sum_planned<float>(d, collective, rt, parts, nullptr);
        }
    });
}

int snpmi_grm_end(int diag_k_to_n, double* factor, void* K_out) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
        session_check_open();
        Device& d = device();
        g_session.active = false;
        if (!K_out) {  // end without a result (a non-root rank after an RCCL reduce, an aborted GRM)
            SNPMI_HIP(hipStreamSynchronize(d.stream));
            if (factor) *factor = NAN;
            return;
        }
        void* t = session_tiles(d);
        if (!g_session.wrote)
            SNPMI_HIP(hipMemsetAsync(t, 0, n_tiles_upper(g_session.n) * kTile * kTile * dtype_size(g_session.dtype),
                                     d.stream));
        if (g_session.dtype == SNPMI_DT_F32)
            grm_finish(d, (const float*)t, g_session.n, diag_k_to_n, factor, (float*)K_out);
        else
            grm_finish(d, (const double*)t, g_session.n, diag_k_to_n, factor, (double*)K_out);
    });
}

// ---- rect GRM (K[rows, cols] directly)
uint64_t snpmi_grm_rect_bytes(uint64_t n_rows, uint64_t n_cols, int dtype) { return rect_bytes(n_rows, n_cols, dtype); }

int snpmi_rect_diag_pairs(const uint64_t* row_idx, uint64_t n_rows, const uint64_t* col_idx, uint64_t n_cols,
                          uint32_t* pairs, uint64_t cap, uint64_t* count) {
    return guarded([&] {
        SNPMI_REQUIRE(count != nullptr, SNPMI_E_ARG, "count is NULL");
        std::vector<uint32_t> v;
        rect_diag_pairs(row_idx, n_rows, col_idx, n_cols, v);
        *count = v.size() / 2;
        if (pairs) std::memcpy(pairs, v.data(), std::min<uint64_t>(cap, v.size() / 2) * 8);
    });
}

int snpmi_dev_syrk_rect(const uint8_t* packed_a, uint64_t pitch_a, uint64_t n_a, const uint8_t* packed_b,
                        uint64_t pitch_b, uint64_t n_b, uint64_t n_sid, const void* lut, int dtype, void* blocks,
                        int accumulate, const uint32_t* pairs, uint64_t n_pairs) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);  // shared scratch slots
        SNPMI_REQUIRE(dtype == SNPMI_DT_F32 || dtype == SNPMI_DT_F64, SNPMI_E_ARG, "GRM dtype must be f32/f64");
        Device& d = device();
        for (uint64_t k = 0; k < n_pairs; k++)
            SNPMI_REQUIRE(pairs && pairs[2 * k] < n_a && pairs[2 * k + 1] < n_b, SNPMI_E_INDEX, "diagonal pair out of range");
        (void)rect_blocks(n_a, pitch_a, n_b, pitch_b);
        const RectPairs dp = dtype == SNPMI_DT_F32 ? rect_pairs_upload(d, pairs, n_pairs) : RectPairs();
        syrk_rect_auto(d, packed_a, pitch_a, n_a, packed_b, pitch_b, n_b, n_sid, lut, dtype, blocks, accumulate, dp);
    });
}

int snpmi_dev_rect_extract(const void* blocks, uint64_t n_rows, uint64_t n_cols, int dtype, int order_c, double scale,
                           void* K_out) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);  // shared scratch slots
        SNPMI_REQUIRE(dtype == SNPMI_DT_F32 || dtype == SNPMI_DT_F64, SNPMI_E_ARG, "GRM dtype must be f32/f64");
        SNPMI_REQUIRE(K_out != nullptr || n_rows * n_cols == 0, SNPMI_E_ARG, "K_out is NULL");
        Device& d = device();
        if (dtype == SNPMI_DT_F32) rect_extract(d, (const float*)blocks, n_rows, n_cols, order_c, scale, (float*)K_out);
        else rect_extract(d, (const double*)blocks, n_rows, n_cols, order_c, scale, (double*)K_out);
    });
}

int snpmi_grm_rect_begin(uint64_t n_rows, uint64_t n_cols, int dtype) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
        SNPMI_REQUIRE(dtype == SNPMI_DT_F32 || dtype == SNPMI_DT_F64, SNPMI_E_ARG, "GRM dtype must be f32 or f64");
        SNPMI_REQUIRE(ceil_div(n_rows, 256) < 65536 && ceil_div(n_cols, 256) < 65536 &&
                          ceil_div(n_rows, 256) * ceil_div(n_cols, 256) < (1ull << 29),
                      SNPMI_E_ARG, "rect GRM: too many 256-iid blocks");
        Device& d = device();
        g_rect = RectSession{true, false, n_rows, n_cols, dtype};
        (void)rect_session_blocks(d);
    });
}

#define SNPMI_GRM_RECT_ADD(SUFFIX, T)                                                                               \
    int snpmi_grm_rect_add_packed_##SUFFIX(SNPMI_PACKED_PARAMS, SNPMI_STD_PARAMS(T), const uint64_t* row_idx,       \
                                           const uint64_t* col_idx) {                                                \
        return guarded([&] { rect_add_packed_impl<T>(SNPMI_PACKED_SNPS, SNPMI_STD_ARGS, stats, row_idx, col_idx); }); \
    }                                                                                                                \
    int snpmi_grm_rect_add_bed_##SUFFIX(SNPMI_BED_PARAMS, SNPMI_STD_PARAMS(T), int num_threads,                     \
                                        const uint64_t* row_idx, const uint64_t* col_idx) {                         \
        return guarded([&] { rect_add_bed_impl<T>(SNPMI_BED_SEL, SNPMI_STD_ARGS, stats, row_idx, col_idx); });       \
    }
SNPMI_GRM_RECT_ADD(f32, float)
SNPMI_GRM_RECT_ADD(f64, double)

int snpmi_grm_rect_end(double scale, int order_c, void* K_out) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
        SNPMI_REQUIRE(g_rect.active, SNPMI_E_ARG, "no rect GRM session (call snpmi_grm_rect_begin)");
        Device& d = device();
        g_rect.active = false;
        if (!K_out || g_rect.nr * g_rect.nc == 0) {  // an aborted session, or an empty result
            SNPMI_HIP(hipStreamSynchronize(d.stream));
            return;
        }
        void* t = rect_session_blocks(d);
        if (!g_rect.wrote)
            SNPMI_HIP(hipMemsetAsync(t, 0, rect_bytes(g_rect.nr, g_rect.nc, g_rect.dtype), d.stream));
        if (g_rect.dtype == SNPMI_DT_F32)
            rect_extract(d, (const float*)t, g_rect.nr, g_rect.nc, order_c, scale, (float*)K_out);
        else
            rect_extract(d, (const double*)t, g_rect.nr, g_rect.nc, order_c, scale, (double*)K_out);
    });
}

#define SNPMI_DENSE(SUFFIX, T)                                                                                      \
    int snpmi_standardize_##SUFFIX(T* val, uint64_t rows, uint64_t cols, int order_c, int is_beta, double a,        \
                                   double b, int apply_in_place, int use_stats, T* stats, int) {                    \
        return guarded([&] {                                                                                         \
            standardize_impl<T>(val, rows, cols, order_c, is_beta, a, b, apply_in_place, use_stats, stats);          \
        });                                                                                                          \
    }                                                                                                                \
    int snpmi_grm_bed_##SUFFIX(SNPMI_BED_PARAMS, SNPMI_STD_PARAMS(T), int diag, double* factor, T* K_out,           \
                               int num_threads) {                                                                    \
        return guarded([&] { grm_bed_impl<T>(SNPMI_BED_SEL, SNPMI_STD_ARGS, stats, diag, factor, K_out); });         \
    }                                                                                                                \
    int snpmi_grm_dense_##SUFFIX(const T* val, uint64_t rows, uint64_t cols, int order_c, SNPMI_STD_PARAMS(T),      \
                                 int diag, double* factor, T* K_out) {                                               \
        return guarded([&] {                                                                                         \
            grm_dense_impl<T>(val, rows, cols, order_c, SNPMI_STD_ARGS, stats, diag, factor, K_out);                 \
        });                                                                                                          \
    }                                                                                                                \
    int snpmi_diag_k_to_n_snps_##SUFFIX(T* val, uint64_t rows, uint64_t cols, double* factor) {                     \
        return guarded([&] { snp_scale_impl<T>(val, rows * cols, (double)rows, 0, 1.0, factor); });                  \
    }                                                                                                                \
    int snpmi_scale_##SUFFIX(T* val, uint64_t count, double scale) {                                                \
        return guarded([&] { snp_scale_impl<T>(val, count, 0.0, 1, scale, nullptr); });                              \
    }                                                                                                                \
    int snpmi_diag_k_to_n_##SUFFIX(T* K, uint64_t n, double* factor) {                                              \
        return guarded([&] { diag_k_to_n_impl<T>(K, n, factor); });                                                  \
    }
SNPMI_DENSE(f32, float)
SNPMI_DENSE(f64, double)

#define SNPMI_SUBSET(SUFFIX, S, D)                                                                                  \
    int snpmi_subset_##SUFFIX(const S* val, uint64_t rows, uint64_t cols, uint64_t k, int in_c, const uint64_t* ri, \
                              uint64_t nr, const uint64_t* ci, uint64_t nc, int out_c, D* out, int) {               \
        return guarded([&] { subset_impl<S, D>(val, rows, cols, k, in_c, ri, nr, ci, nc, out_c, out); });            \
    }
SNPMI_SUBSET(f64_f64, double, double)
SNPMI_SUBSET(f32_f64, float, double)
SNPMI_SUBSET(f32_f32, float, float)

// ---------------------------------------------------------------------- device-resident API
uint64_t snpmi_packed_pitch(uint64_t n_iid) { return packed_pitch(n_iid); }
uint64_t snpmi_grm_tile_bytes(uint64_t n_iid, int dtype) {
    return n_tiles_upper(n_iid) * kTile * kTile * dtype_size(dtype);
}

int snpmi_dev_alloc(void** ptr, uint64_t bytes) {
    return guarded([&] {
        SNPMI_REQUIRE(ptr != nullptr, SNPMI_E_ARG, "ptr is NULL");
        (void)device();
        if (hipMalloc(ptr, bytes ? bytes : 256) != hipSuccess) {
            (void)hipGetLastError();
            throw Error(SNPMI_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
        }
    });
}
int snpmi_host_alloc(void** ptr, uint64_t bytes) {
    return guarded([&] {
        SNPMI_REQUIRE(ptr != nullptr, SNPMI_E_ARG, "ptr is NULL");
        (void)device();
        if (hipHostMalloc(ptr, bytes ? bytes : 256, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            throw Error(SNPMI_E_NOMEM, "hipHostMalloc of " + std::to_string(bytes) + " bytes failed");
        }
    });
}
int snpmi_host_free(void* ptr) {
    return guarded([&] {
        (void)device();
        SNPMI_HIP(hipHostFree(ptr));
    });
}
int snpmi_dev_free(void* ptr) {
    return guarded([&] {
        (void)device();
        SNPMI_HIP(hipFree(ptr));
    });
}
int snpmi_dev_memset(void* ptr, int value, uint64_t bytes) {
    return guarded([&] { SNPMI_HIP(hipMemsetAsync(ptr, value, bytes, stream())); });
}
int snpmi_memcpy_h2d(void* dst, const void* src, uint64_t bytes) {
    return guarded([&] {
        SNPMI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream()));
        SNPMI_HIP(hipStreamSynchronize(stream()));
    });
}
int snpmi_memcpy_d2h(void* dst, const void* src, uint64_t bytes) {
    return guarded([&] {
        SNPMI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream()));
        SNPMI_HIP(hipStreamSynchronize(stream()));
    });
}
int snpmi_dev_memcpy_2d(void* dst, uint64_t dpitch, const void* src, uint64_t spitch, uint64_t width, uint64_t rows) {
    return guarded([&] {
        SNPMI_REQUIRE(dpitch >= width && spitch >= width, SNPMI_E_ARG, "a pitch is smaller than the row width");
        if (width == 0 || rows == 0) return;
        SNPMI_REQUIRE(dst != nullptr && src != nullptr, SNPMI_E_ARG, "NULL argument");
        SNPMI_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice, stream()));
    });
}

int snpmi_dev_memcpy_d2d(void* dst, const void* src, uint64_t bytes) {
    return guarded([&] {
        const bool aligned = reinterpret_cast<uintptr_t>(dst) % 16 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0;
        const uint64_t body = aligned ? bytes / 16 * 16 : 0;
        if (body) launch_copy16(src, dst, body, stream());
        if (bytes > body)
            SNPMI_HIP(hipMemcpyAsync((uint8_t*)dst + body, (const uint8_t*)src + body, bytes - body,
                                     hipMemcpyDeviceToDevice, stream()));
    });
}
int snpmi_stream_sync(void) {
    return guarded([&] {
        Device& d = device();
        SNPMI_HIP(hipStreamSynchronize(d.stream));
        SNPMI_HIP(hipStreamSynchronize(d.copy));
        SNPMI_HIP(hipStreamSynchronize(d.aux));
    });
}

int snpmi_set_stream(int which) {
    return guarded([&] {
        SNPMI_REQUIRE(which == 0 || which == 2, SNPMI_E_ARG, "stream must be 0 (compute) or 2 (aux)");
        g_sel_stream = which;
    });
}

int snpmi_device_memory(uint64_t* free_bytes, uint64_t* total_bytes) {
    return guarded([&] {
        device();
        size_t f = 0, t = 0;
        SNPMI_HIP(hipMemGetInfo(&f, &t));
        if (free_bytes) *free_bytes = f;
        if (total_bytes) *total_bytes = t;
    });
}

// ---------------------------------------------------------------------- copy stream (streaming API)
static hipStream_t pick_stream(Device& d, int on_copy) {
    return on_copy == 1 ? d.copy : on_copy == 2 ? d.aux : d.stream;
}

int snpmi_memcpy_async(void* dst, const void* src, uint64_t bytes, int kind, int on_copy) {
    return guarded([&] {
        SNPMI_REQUIRE(kind >= 0 && kind <= 2, SNPMI_E_ARG, "kind must be 0 (H2D), 1 (D2H) or 2 (D2D)");
        Device& d = device();
        const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost
                                                                              : hipMemcpyDeviceToDevice;
        if (bytes) SNPMI_HIP(hipMemcpyAsync(dst, src, bytes, k, pick_stream(d, on_copy)));
    });
}
int snpmi_event_record_on(void* ev, int on_copy) {
    return guarded([&] {
        Device& d = device();
        SNPMI_HIP(hipEventRecord((hipEvent_t)ev, pick_stream(d, on_copy)));
    });
}
int snpmi_stream_wait_event(void* ev, int on_copy) {
    return guarded([&] {
        Device& d = device();
        SNPMI_HIP(hipStreamWaitEvent(pick_stream(d, on_copy), (hipEvent_t)ev, 0));
    });
}
int snpmi_event_sync(void* ev) {
    return guarded([&] { SNPMI_HIP(hipEventSynchronize((hipEvent_t)ev)); });
}
int snpmi_event_create(void** ev) {
    return guarded([&] {
        (void)device();
        SNPMI_HIP(hipEventCreate((hipEvent_t*)ev));
    });
}
int snpmi_event_destroy(void* ev) {
    return guarded([&] { SNPMI_HIP(hipEventDestroy((hipEvent_t)ev)); });
}
int snpmi_event_record(void* ev) {
    return guarded([&] { SNPMI_HIP(hipEventRecord((hipEvent_t)ev, stream())); });
}
int snpmi_event_elapsed_ms(void* start, void* stop, float* ms) {
    return guarded([&] {
        SNPMI_HIP(hipEventSynchronize((hipEvent_t)stop));
        SNPMI_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    });
}

int snpmi_dev_synth_bed(uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t sid0, uint64_t n_sid, uint64_t seed,
                        double miss_rate, const double* maf_x, const double* maf_cdf, int n_pts) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);  // shared scratch slots
        SNPMI_REQUIRE(pitch % 4 == 0 && pitch >= ceil_div(n_iid, 4), SNPMI_E_ARG, "bad pitch");
        SNPMI_REQUIRE(n_pts > 0 && n_pts <= 1024, SNPMI_E_ARG, "bad MAF table");
        Device& d = device();
        double* tab = (double*)d.get(Device::S_RED, 2 * n_pts * sizeof(double));
        SNPMI_HIP(hipMemcpyAsync(tab, maf_x, n_pts * 8, hipMemcpyHostToDevice, d.stream));
        SNPMI_HIP(hipMemcpyAsync(tab + n_pts, maf_cdf, n_pts * 8, hipMemcpyHostToDevice, d.stream));
        launch_synth(packed, pitch, n_iid, sid0, n_sid, seed, miss_rate, tab, tab + n_pts, n_pts, d.stream);
        SNPMI_HIP(hipStreamSynchronize(d.stream));
    });
}

// ---------------------------------------------------------------------- host-side synthetic source
// A stand-in for "gather the selected .bed columns from the page cache into pinned memory" when a
// workload is too large to write to disk (cfg5: 125 GB of packed codes): the streamed GRM legs
// generate each SNP block on host threads while the GPU works on the previous one.  Per SNP the
// MAF comes from the same counter hash and MAF table as k_synth; per genotype one 32-bit hash
// (lowbias32 of seed/SNP key ^ iid * golden ratio) split into missing / hom-alt / het / hom-ref
// with the joint probabilities miss, (1-miss) p^2, (1-miss) 2p(1-p), rest -- k_synth's
// distribution, a cheaper stream (AVX2 when the host has it).  Restated in NumPy by
// tests/test_host_synth.py.
namespace {
inline uint64_t h_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
inline uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
struct SynthCol {
    uint32_t kb, thm, t3, t2;
};
inline uint32_t synth_code(uint32_t u, const SynthCol& c) {
    const uint32_t a = u - c.thm;
    return u < c.thm ? 1u : a < c.t3 ? 3u : a - c.t3 < c.t2 ? 2u : 0u;
}
// packed words [d0, d0+nw) of one column (16 iids per word; iids >= n are 0)
void synth_words_scalar(uint32_t* w, uint64_t d0, uint64_t nw, uint64_t n, const SynthCol& c) {
    for (uint64_t q = 0; q < nw; q++) {
        uint32_t x = 0;
        for (uint32_t k = 0; k < 16; k++) {
            const uint64_t i = 16 * (d0 + q) + k;
            if (i >= n) break;
            x |= synth_code(lowbias32(c.kb ^ ((uint32_t)i * 0x9E3779B9u)), c) << (2 * k);
        }
        w[q] = x;
    }
}
__attribute__((target("avx2"))) void synth_words_avx2(uint32_t* w, uint64_t d0, uint64_t nw, uint64_t n,
                                                      const SynthCol& c) {
    const __m256i sgn = _mm256_set1_epi32((int)0x80000000u);
    const __m256i vkb = _mm256_set1_epi32((int)c.kb), G = _mm256_set1_epi32((int)0x9E3779B9u);
    const __m256i M1 = _mm256_set1_epi32(0x7feb352d), M2 = _mm256_set1_epi32((int)0x846ca68bu);
    const __m256i thm_s = _mm256_set1_epi32((int)(c.thm ^ 0x80000000u)), t3_s = _mm256_set1_epi32((int)(c.t3 ^ 0x80000000u)),
                  t2_s = _mm256_set1_epi32((int)(c.t2 ^ 0x80000000u)), thm = _mm256_set1_epi32((int)c.thm),
                  t3 = _mm256_set1_epi32((int)c.t3), two = _mm256_set1_epi32(2), three = _mm256_set1_epi32(3),
                  one = _mm256_set1_epi32(1);
    const __m256i lane = _mm256_setr_epi32(0, 16, 32, 48, 64, 80, 96, 112);
    const uint64_t full = std::min<uint64_t>(nw, n / 16 > d0 ? n / 16 - d0 : 0);  // words with 16 real iids
    uint64_t q = 0;
    for (; q + 8 <= full; q += 8) {
        __m256i i = _mm256_add_epi32(_mm256_set1_epi32((int)(uint32_t)(16 * (d0 + q))), lane);
        __m256i x = _mm256_setzero_si256();
        for (int k = 0; k < 16; k++) {
            __m256i h = _mm256_xor_si256(vkb, _mm256_mullo_epi32(i, G));
            h = _mm256_xor_si256(h, _mm256_srli_epi32(h, 16));
            h = _mm256_mullo_epi32(h, M1);
            h = _mm256_xor_si256(h, _mm256_srli_epi32(h, 15));
            h = _mm256_mullo_epi32(h, M2);
            h = _mm256_xor_si256(h, _mm256_srli_epi32(h, 16));
            const __m256i miss = _mm256_cmpgt_epi32(thm_s, _mm256_xor_si256(h, sgn));  // u < thm (unsigned)
            const __m256i a = _mm256_sub_epi32(h, thm);
            const __m256i hom = _mm256_cmpgt_epi32(t3_s, _mm256_xor_si256(a, sgn));
            const __m256i het = _mm256_cmpgt_epi32(t2_s, _mm256_xor_si256(_mm256_sub_epi32(a, t3), sgn));
            __m256i code = _mm256_and_si256(het, two);
            code = _mm256_blendv_epi8(code, three, hom);
            code = _mm256_blendv_epi8(code, one, miss);
            x = _mm256_or_si256(x, _mm256_sll_epi32(code, _mm_cvtsi32_si128(2 * k)));
            i = _mm256_add_epi32(i, one);
        }
        _mm256_storeu_si256((__m256i*)(w + q), x);
    }
    if (q < nw) synth_words_scalar(w + q, d0 + q, nw - q, n, c);
}
}  // namespace

int snpmi_host_synth_bed(uint8_t* dst, uint64_t pitch, uint64_t n_iid, uint64_t sid0, uint64_t n_sid, uint64_t seed,
                         double miss_rate, const double* maf_x, const double* maf_cdf, int n_pts, int num_threads) {
    return guarded([&] {
        SNPMI_REQUIRE(dst != nullptr || n_sid == 0, SNPMI_E_ARG, "dst is NULL");
        SNPMI_REQUIRE(pitch % 4 == 0 && pitch >= ceil_div(n_iid, 4), SNPMI_E_ARG, "bad pitch");
        SNPMI_REQUIRE(n_pts > 0 && n_pts <= 1024 && maf_x && maf_cdf, SNPMI_E_ARG, "bad MAF table");
        SNPMI_REQUIRE(n_iid < (1ull << 32), SNPMI_E_ARG, "host synth: n_iid must be < 2^32");
        const bool avx2 = __builtin_cpu_supports("avx2");
        const uint64_t nd = pitch / 4, per = 2048;  // words per work item (32 KiB of codes)
        const uint64_t items_per_col = ceil_div(nd, per);
        const double sc = 4294967296.0;
        auto thr = [&](double t) { return t >= sc ? 0xFFFFFFFFu : (uint32_t)t; };
        parallel_for(
            n_sid * items_per_col, resolve_threads(num_threads),
            [&](uint64_t it) {
                const uint64_t j = it / items_per_col, d0 = (it % items_per_col) * per;
                const uint64_t sid = sid0 + j;
                const uint64_t h = h_splitmix64(seed * 0xD1B54A32D192ED03ull ^ (sid + 1) * 0x8CB92BA72F3D8DD7ull);
                const double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);
                int lo = 0, hi = n_pts - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (u > maf_cdf[mid]) lo = mid + 1;
                    else hi = mid;
                }
                const double maf = maf_x[lo], keep = 1.0 - miss_rate;
                SynthCol c;
                c.kb = (uint32_t)(h_splitmix64((seed + 0x632BE59BD9B4E019ull) ^ (sid * 0x9E6C63D0676A9A99ull)) >> 32);
                c.thm = thr(miss_rate * sc);
                c.t3 = thr(keep * maf * maf * sc);
                c.t2 = thr(keep * 2.0 * maf * (1.0 - maf) * sc);
                uint32_t* w = reinterpret_cast<uint32_t*>(dst + j * pitch) + d0;
                const uint64_t nw = std::min(per, nd - d0);
                if (avx2) synth_words_avx2(w, d0, nw, n_iid, c);
                else synth_words_scalar(w, d0, nw, n_iid, c);
            },
            4);
    });
}

// selected .bed columns (all iids, ceil(n/4) bytes each, zero-padded to `pitch`) into a host
// buffer -- the host half of stage_chunk, for callers that run their own upload (the cfg5 plan:
// each rank gathers only its share of a SNP block, shard.PartitionedGrm)
int snpmi_bed_gather_packed(const char* path, uint64_t n_iid, uint64_t n_sid, const uint64_t* sid_idx, uint64_t n_sel,
                            uint64_t pitch, uint8_t* dst, int num_threads) {
    return guarded([&] {
        BedMap m;
        open_bed(m, path, n_iid, n_sid);
        SNPMI_REQUIRE(pitch >= m.bpc, SNPMI_E_ARG, "pitch is smaller than a column");
        SNPMI_REQUIRE(dst != nullptr || n_sel == 0, SNPMI_E_ARG, "dst is NULL");
        check_index(sid_idx, n_sel, n_sid, "sid");
        gather_columns(m, sid_idx, 0, n_sel, pitch, dst, resolve_threads(num_threads));
    });
}

int snpmi_dev_snp_stats(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, int count_a1,
                        int std_kind, double a, double b, int use_stats, int dtype, void* stats, void* lut) {
    return guarded([&] {
        check_pitch(pitch, n_iid);
        launch_snp_stats(packed, pitch, n_iid, n_sid, count_a1, SNPMI_STD_ARGS, dtype, stats, lut, stream());
    });
}

int snpmi_dev_decode(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, const void* lut,
                     int dtype, int order_c, void* out, uint64_t ld) {
    return guarded([&] {
        check_pitch(pitch, n_iid);
        if (!order_c) SNPMI_REQUIRE(ld % 16 == 0 && ld >= n_iid, SNPMI_E_ARG, "F-order ld must be >= n_iid, % 16");
        else SNPMI_REQUIRE(ld >= n_sid, SNPMI_E_ARG, "C-order ld must be >= n_sid");
        launch_decode(packed, pitch, n_iid, n_sid, lut, dtype, order_c, out, ld, stream());
    });
}

int snpmi_dev_decode_standardize(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                                 int count_a1, int std_kind, double a, double b, int use_stats, int dtype,
                                 void* stats, void* lut, void* out, uint64_t ld) {
    return guarded([&] {
        SNPMI_REQUIRE(dtype == SNPMI_DT_F32, SNPMI_E_ARG, "fused decode+standardize is f32 only");
        check_pitch(pitch, n_iid);
        SNPMI_REQUIRE(ld % 16 == 0 && ld >= n_iid, SNPMI_E_ARG, "F-order ld must be >= n_iid, % 16");
        launch_decode_std_fused(packed, pitch, n_iid, n_sid, count_a1, SNPMI_STD_ARGS, stats, lut, out, ld, stream());
    });
}

int snpmi_dev_repack(const uint8_t* src, uint64_t src_pitch, uint64_t n_src, const uint64_t* idx, uint64_t n_out,
                     uint64_t n_sid, uint8_t* dst, uint64_t dst_pitch) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);  // shared scratch slots
        check_pitch(dst_pitch, n_out, "bad dst pitch");
        Device& d = device();
        uint32_t* plan = (uint32_t*)d.get(Device::S_IDX32, repack_plan_entries(n_out) * 4);
        uint32_t* win = (uint32_t*)d.get(Device::S_WIN, repack_win_entries(n_out) * 4);
        const RepackPlan P = launch_repack_plan(idx, n_out, n_src, plan, win, d.stream);
        launch_repack(src, src_pitch, n_src, idx, P, n_out, n_sid, dst, dst_pitch, d.stream);
    });
}

int snpmi_dev_syrk_packed(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, const void* lut,
                          int dtype, void* K_tiles, int accumulate) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);  // shared scratch slots
        SNPMI_REQUIRE(dtype == SNPMI_DT_F32 || dtype == SNPMI_DT_F64, SNPMI_E_ARG, "GRM dtype must be f32/f64");
        check_pitch(pitch, n_iid);
        syrk_packed_auto(device(), packed, pitch, n_iid, n_sid, lut, dtype, whole_dest(K_tiles, n_iid), accumulate);
    });
}

int snpmi_dev_syrk_dense(const void* Z, uint64_t ldz, uint64_t n_iid, uint64_t n_sid, int dtype, void* K_tiles,
                         int accumulate) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);  // shared scratch slots
        SNPMI_REQUIRE(dtype == SNPMI_DT_F32 || dtype == SNPMI_DT_F64, SNPMI_E_ARG, "GRM dtype must be f32/f64");
        syrk_dense_auto(device(), Z, ldz, n_iid, n_sid, dtype, K_tiles, accumulate);
    });
}

int snpmi_dev_grm_extract(const void* K_tiles, uint64_t n_iid, int dtype, const uint64_t* ri, uint64_t nr,
                          const uint64_t* ci, uint64_t nc, int order_c, double scale, void* out) {
    return guarded([&] {
        // the whole K (K symmetric, so either order): the tile-blocked extraction
        if (!ri && !ci && nr == n_iid && nc == n_iid)
            launch_grm_extract_rows(K_tiles, n_iid, dtype, 0, n_iid, scale, out, stream());
        else
            launch_grm_extract(K_tiles, n_iid, dtype, ri, nr, ci, nc, order_c, scale, out, stream());
    });
}

static void crt_stats(uint64_t* a, uint64_t* b, int reset, int which) {
    Device& d = device();
    unsigned long long h[2] = {0, 0};
    unsigned long long* rec = crt_record(d) + 2 * which;
    SNPMI_HIP(hipMemcpyAsync(h, rec, sizeof(h), hipMemcpyDeviceToHost, d.stream));
    if (reset) SNPMI_HIP(hipMemsetAsync(rec, 0, sizeof(h), d.stream));
    SNPMI_HIP(hipStreamSynchronize(d.stream));
    *a = h[0];
    *b = h[1];
}

int snpmi_crt_moduli_stats(uint64_t* sum_r, uint64_t* launches, int reset) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
        SNPMI_REQUIRE(sum_r != nullptr && launches != nullptr, SNPMI_E_ARG, "NULL output");
        crt_stats(sum_r, launches, reset, 0);
    });
}

int snpmi_crt_block_moduli_stats(uint64_t* sum_rb, uint64_t* blocks, int reset) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);
        SNPMI_REQUIRE(sum_rb != nullptr && blocks != nullptr, SNPMI_E_ARG, "NULL output");
        crt_stats(sum_rb, blocks, reset, 1);
    });
}

int snpmi_dev_grm_trace(const void* K_tiles, uint64_t n_iid, int dtype, double* trace) {
    return guarded([&] {
        std::lock_guard<std::recursive_mutex> lk(g_call_mutex);  // shared scratch slots
        Device& d = device();
        double* tr = (double*)d.get(Device::S_RED, 64);
        launch_grm_trace(K_tiles, n_iid, dtype, tr, d.stream);
        SNPMI_HIP(hipMemcpyAsync(trace, tr, 8, hipMemcpyDeviceToHost, d.stream));
        SNPMI_HIP(hipStreamSynchronize(d.stream));
    });
}

// ---- partitioned GRM (cfg5: each rank holds its own 256x256 blocks of K)
uint64_t snpmi_grm_part_blocks(uint64_t n_iid, int part_rank, int part_world) {
    return part_ok(part_rank, part_world) ? grm_part_blocks(n_iid, part_rank, part_world) : 0;
}

int snpmi_grm_part_coords(uint64_t n_iid, int part_rank, int part_world, uint64_t local_block, uint64_t* row0,
                          uint64_t* col0) {
    return guarded([&] {
        check_part(part_rank, part_world);
        std::lock_guard<std::mutex> lk(g_layout_mutex);
        const auto& tab = host_layout(ceil_div(n_iid, 256), part_rank, part_world);
        SNPMI_REQUIRE(local_block < tab.size(), SNPMI_E_INDEX, "block out of range");
        if (row0) *row0 = (uint64_t)(tab[local_block] & 0xffffu) * 256;
        if (col0) *col0 = (uint64_t)(tab[local_block] >> 16) * 256;
    });
}

int snpmi_grm_part_coords_all(uint64_t n_iid, int part_rank, int part_world, uint64_t* coords) {
    return guarded([&] {
        check_part(part_rank, part_world);
        std::lock_guard<std::mutex> lk(g_layout_mutex);
        const auto& tab = host_layout(ceil_div(n_iid, 256), part_rank, part_world);
        SNPMI_REQUIRE(coords != nullptr || tab.empty(), SNPMI_E_ARG, "coords is NULL");
        for (uint64_t w = 0; w < tab.size(); w++) {
            coords[2 * w] = (uint64_t)(tab[w] & 0xffffu) * 256;
            coords[2 * w + 1] = (uint64_t)(tab[w] >> 16) * 256;
        }
    });
}

#define SNPMI_GRM_PART(SUFFIX, T)                                                                                   \
    int snpmi_grm_part_bed_##SUFFIX(SNPMI_BED_PARAMS, SNPMI_STD_PARAMS(T), int part_rank, int part_world,           \
                                    T* blocks_out, int num_threads) {                                                \
        return guarded([&] {                                                                                         \
            grm_part_bed_impl<T>(SNPMI_BED_SEL, SNPMI_STD_ARGS, stats, part_rank, part_world, blocks_out);           \
        });                                                                                                          \
    }                                                                                                                \
    int snpmi_grm_part_extract_##SUFFIX(const T* blocks, uint64_t n_iid, int part_rank, int part_world,             \
                                        const uint64_t* ri, uint64_t nr, const uint64_t* ci, uint64_t nc,           \
                                        int order_c, double scale, T* out) {                                         \
        return guarded([&] {                                                                                         \
            part_extract_impl<T>(blocks, n_iid, part_rank, part_world, ri, nr, ci, nc, order_c, scale, out);         \
        });                                                                                                          \
    }                                                                                                                \
    int snpmi_grm_part_trace_##SUFFIX(const T* blocks, uint64_t n_iid, int part_rank, int part_world,               \
                                      double* trace) {                                                               \
        return guarded([&] { part_trace_impl<T>(blocks, n_iid, part_rank, part_world, trace); });                    \
    }
SNPMI_GRM_PART(f32, float)
SNPMI_GRM_PART(f64, double)

// (the pair differs in its pointer types: the f32 form predates the typed one)
int snpmi_dev_syrk_packed_part(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid, const void* lut,
                               int part_rank, int part_world, void* blocks, int accumulate) {
    return guarded([&] {
        dev_syrk_packed_part(SNPMI_DT_F32, packed, pitch, n_iid, n_sid, lut, part_rank, part_world, blocks, accumulate);
    });
}
int snpmi_dev_syrk_packed_part_f64(const uint8_t* packed, uint64_t pitch, uint64_t n_iid, uint64_t n_sid,
                                   const double* lut, int part_rank, int part_world, double* blocks, int accumulate) {
    return guarded([&] {
        dev_syrk_packed_part(SNPMI_DT_F64, packed, pitch, n_iid, n_sid, lut, part_rank, part_world, blocks, accumulate);
    });
}

}  // extern "C"
