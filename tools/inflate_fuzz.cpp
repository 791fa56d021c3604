// Host fuzzing of the inflate decoder core (pysnptools_amd/csrc/inflate_core.hpp): plain C++, no
// libsnpmi, no Python, no GPU.  Build with the host compiler and the sanitizers, then run:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o inflate_fuzz tools/inflate_fuzz.cpp
//   ./inflate_fuzz [--rounds N] [--seed S] case0.bin case1.bin ...
//
// Each case file is a u64 (little endian) D followed by one zlib stream that inflates to D bytes
// (tools/inflate_fuzz_cases.py writes the test suite's valid streams that way).  Run on them:
//   * the stream as it is: status 0
//   * seeded mutations: 1 ... 4 flipped bits, a truncation, a splice of the head of one stream with
//     the tail of another, each with D as given, D - 1, D + 1, 0 or a random D
//   * purely random bytes, half of them behind a valid zlib header
// Every run reads its source from a heap block of exactly `stored` bytes (AddressSanitizer sees one
// byte too far) and writes into D bytes ringed by 64 guard bytes each side, which are compared
// afterwards; a status outside the known ones, a guard byte changed or a valid stream refused ends
// the program with exit status 1.  That every run returns at all is the evidence for "each loop
// iteration consumes input or ends the stream".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../pysnptools_amd/csrc/inflate_core.hpp"

namespace zc = inflate_core;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return g_state * 0x2545f4914f6cdd1dull;
}

struct Case {
    std::vector<uint8_t> stream;
    uint64_t D;
};

static constexpr size_t kGuard = 64;
static uint64_t g_runs = 0, g_by_status[zc::STATUS_COUNT] = {};
static std::unique_ptr<zc::Scratch> g_scratch(new zc::Scratch);

static uint32_t run(const std::vector<uint8_t>& stream, uint64_t D, const char* what) {
    // a heap block of exactly the stream's size: a read one byte beyond it is a sanitizer report
    uint8_t* src = new uint8_t[stream.size()];
    if (!stream.empty()) std::memcpy(src, stream.data(), stream.size());
    std::vector<uint8_t> room(kGuard + D + kGuard, 0xa5);
    std::memset(g_scratch.get(), 0xcc, sizeof(zc::Scratch));  // no state survives from the run before
    const uint32_t st = zc::inflate_zlib<zc::HostLanes>(src, stream.size(), room.data() + kGuard, D, *g_scratch);
    bool ok = st < zc::STATUS_COUNT;
    for (size_t i = 0; i < kGuard; i++) ok = ok && room[i] == 0xa5 && room[kGuard + D + i] == 0xa5;
    delete[] src;
    if (!ok) {
        std::fprintf(stderr, "FAIL (%s): status %u, stored %zu, D %" PRIu64 "\n", what, st, stream.size(), D);
        std::exit(1);
    }
    g_runs++;
    g_by_status[st]++;
    return st;
}

static uint64_t pick_d(uint64_t D) {
    switch (rnd() % 6) {
        case 0: return D ? D - 1 : 0;
        case 1: return D + 1;
        case 2: return 0;
        case 3: return rnd() % (2 * D + 2);
        default: return D;
    }
}

int main(int argc, char** argv) {
    uint64_t rounds = 2000;
    std::vector<Case> cases;
    for (int a = 1; a < argc; a++) {
        if (!std::strcmp(argv[a], "--rounds") && a + 1 < argc) rounds = std::strtoull(argv[++a], nullptr, 10);
        else if (!std::strcmp(argv[a], "--seed") && a + 1 < argc) g_state ^= std::strtoull(argv[++a], nullptr, 10) * 2 + 1;
        else {
            FILE* f = std::fopen(argv[a], "rb");
            if (!f) {
                std::fprintf(stderr, "cannot open %s\n", argv[a]);
                return 2;
            }
            std::vector<uint8_t> all;
            uint8_t buf[65536];
            for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + n);
            std::fclose(f);
            if (all.size() < 8) {
                std::fprintf(stderr, "%s is shorter than its length field\n", argv[a]);
                return 2;
            }
            Case c;
            c.D = 0;
            for (int k = 7; k >= 0; k--) c.D = c.D << 8 | all[k];
            c.stream.assign(all.begin() + 8, all.end());
            if (c.D >= zc::kMaxOut || c.stream.size() >= zc::kMaxStored) {
                std::fprintf(stderr, "%s is too long\n", argv[a]);
                return 2;
            }
            if (run(c.stream, c.D, argv[a]) != zc::OK) {
                std::fprintf(stderr, "FAIL: the valid stream %s is refused\n", argv[a]);
                return 1;
            }
            cases.push_back(std::move(c));
        }
    }
    std::printf("%zu valid streams inflate\n", cases.size());
    for (size_t ci = 0; ci < cases.size(); ci++) {
        const Case& c = cases[ci];
        for (uint64_t r = 0; r < rounds; r++) {
            std::vector<uint8_t> m = c.stream;
            const char* what = "bit flips";
            switch (r % 3) {
                case 0:
                    for (uint64_t k = 1 + rnd() % 4; k && !m.empty(); k--) m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8));
                    break;
                case 1:
                    what = "truncation";
                    m.resize(rnd() % (m.size() + 1));
                    break;
                default: {
                    what = "splice";
                    const Case& o = cases[rnd() % cases.size()];
                    m.resize(rnd() % (m.size() + 1));
                    const size_t from = rnd() % (o.stream.size() + 1);
                    m.insert(m.end(), o.stream.begin() + from, o.stream.end());
                }
            }
            run(m, pick_d(c.D), what);
        }
    }
    const uint64_t randoms = rounds * (cases.empty() ? 50 : cases.size());
    for (uint64_t r = 0; r < randoms; r++) {
        std::vector<uint8_t> m(rnd() % 600);
        for (auto& b : m) b = (uint8_t)rnd();
        if ((r & 1) && m.size() >= 2) m[0] = 0x78, m[1] = 0x9c;
        run(m, rnd() % 70000, "random bytes");
    }
    std::printf("%" PRIu64 " runs, guards intact; by status:", g_runs);
    for (uint32_t s = 0; s < zc::STATUS_COUNT; s++) std::printf(" %u:%" PRIu64, s, g_by_status[s]);
    std::printf("\n");
    return 0;
}
