// The zlib / deflate decoder core: one stream in, exactly D bytes out or a status.  Written from the
// format rules alone; no compression library's source, none is linked.
//
// One body serves the device (csrc/inflate.hip: one wave per stream, the Scratch in the wave's LDS)
// and plain host C++ (snpmi_inflate_host, tools/inflate_fuzz.cpp: no hipcc needed).  It is written
// for LANES cooperating lanes that run it in lockstep: everything that steers the decode (the bit
// buffer, positions, the symbol walk) is the same value in every lane, and the bulk work -- the
// refill of the input chunk, the table fills, the match copies, the stores to dst and the Adler-32
// sums -- is strided over the lanes, `for (i = lane; i < n; i += LANES)`.  The lanes policy P gives
//
//   P::LANES, P::lane()   64 and the lane id on the device; 1 and 0 on the host
//   P::sync()             the lanes' earlier Scratch accesses are ordered before their later ones
//   P::sum(v)             the sum of v over the lanes, in every lane
//   P::uni(v)             v, known to be the same in every lane (the device moves it to an SGPR)
//
// Safety, for arbitrary input bytes (checked by tools/inflate_fuzz.cpp under ASan + UBSan):
//   * src is read only at [src, src + stored): refill_chunk() and stored_block() compare every
//     index with `stored`; bytes behind the end read as 0
//   * dst is written only at [dst, dst + D), and only by flush(): a literal or a copy that would
//     carry pos past D ends the stream first (OUTPUT_OVERFLOW)
//   * nothing is ever read back from dst: matches are served from the 32 KiB window in Scratch,
//     and a distance above the bytes produced so far (or above 32768) ends the stream
//   * every loop iteration consumes at least one input bit or ends the stream, and the stream ends
//     with INPUT_EXHAUSTED once the bit position has passed 8 * stored (checked once per symbol)
//   * no loop waits for anything another wave does
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define INFL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define INFL_HD inline
#endif

namespace inflate_core {

enum Status : uint32_t {
    OK = 0,
    BAD_HEADER = 1,        // CM != 8, CINFO > 7, FCHECK, FDICT set
    INPUT_EXHAUSTED = 2,   // the bit position passed 8 * stored
    BAD_BLOCK_TYPE = 3,    // BTYPE 3
    STORED_LEN = 4,        // NLEN != ~LEN
    BAD_CODE_LENGTHS = 5,  // oversubscribed / incomplete set, HLIT > 286, HDIST > 30, bad repeat, no code for 256
    BAD_SYMBOL = 6,        // a bit pattern no code owns, length symbol 286 / 287, distance symbol 30 / 31
    BAD_DISTANCE = 7,      // a distance beyond the bytes produced so far
    OUTPUT_OVERFLOW = 8,   // the stream holds more than D bytes
    OUTPUT_SHORT = 9,      // the stream ended with fewer than D bytes
    BAD_ADLER = 10,        // the Adler-32 trailer disagrees
    STATUS_COUNT = 11
};

constexpr uint32_t kWin = 32768, kWinMask = kWin - 1;  // the deflate window, a ring
constexpr uint32_t kChunk = 512;                       // input bytes staged at a time
constexpr uint32_t kFlush = 512;                       // output bytes stored (and summed) at a time
constexpr uint32_t kLitBits = 10, kDistBits = 8;       // index bits of the two lookup tables
constexpr uint32_t kAdler = 65521;
constexpr uint64_t kMaxStored = 1ull << 28, kMaxOut = 1ull << 31;  // so that positions fit 32 bits

// Everything a stream needs besides registers: 37,632 bytes (the device keeps it in LDS).
struct Scratch {
    alignas(8) uint8_t win[kWin];       // output byte p at win[p & kWinMask]
    alignas(8) uint8_t inbuf[kChunk];   // stream bytes [bufbase, bufbase + kChunk), 0 behind the end
    uint16_t ltab[1u << kLitBits];      // literal/length: (symbol << 4 | code length) by the next bits, 0 = walk
    uint16_t dtab[1u << kDistBits];     // distance (and, while a dynamic header is read, the code-length code)
    uint16_t lsym[288], dsym[32];       // symbols in canonical order, for the bit-by-bit walk
    uint16_t lcount[16], dcount[16];    // codes per length
    uint16_t code[320];                 // build: each symbol's code
    uint16_t first[16], nxt[16], offs[16];
    uint8_t lens[320];                  // code lengths: HLIT literal/length ones, then HDIST distance ones
    uint8_t clens[32];                  // the 19 lengths of the code-length code
};

struct HostLanes {
    static constexpr uint32_t LANES = 1;
    static INFL_HD uint32_t lane() { return 0; }
    static INFL_HD void sync() {}
    static INFL_HD uint32_t sum(uint32_t v) { return v; }
    static INFL_HD uint32_t uni(uint32_t v) { return v; }
};

template <class P>
struct Inflater {
    const uint8_t* src;
    uint8_t* dst;
    Scratch& s;
    uint32_t stored, D;
    bool dst8;            // dst is 8-byte aligned: whole flushes go out as 64-bit stores
    uint64_t bitbuf = 0;  // the next nbits bits of the stream, LSB first
    uint32_t nbits = 0;
    uint32_t inpos = 0;                  // stream bytes taken into bitbuf
    uint32_t bufbase = 0u - kChunk;      // no chunk staged yet
    uint32_t pos = 0, flushed = 0;       // bytes produced / stored to dst (flushed <= pos <= D)
    uint32_t a1 = 1, a2 = 0;             // Adler-32 of the flushed bytes
    bool fixed_ready = false;            // the tables hold the fixed codes

    INFL_HD Inflater(const uint8_t* src_, uint64_t stored_, uint8_t* dst_, uint64_t D_, Scratch& s_)
        : src(src_), dst(dst_), s(s_), stored((uint32_t)stored_), D((uint32_t)D_),
          dst8((reinterpret_cast<uintptr_t>(dst_) & 7) == 0) {}

    // ------------------------------------------------------------------ input
    INFL_HD void refill_chunk(uint32_t at) {
        P::sync();
        bufbase = at & ~(kChunk - 1);
        for (uint32_t i = P::lane(); i < kChunk; i += P::LANES) {
            const uint32_t k = bufbase + i;
            s.inbuf[i] = k < stored ? src[k] : (uint8_t)0;
        }
        P::sync();
    }
    INFL_HD void stage(uint32_t at) {
        if ((uint32_t)(at - bufbase) >= kChunk) refill_chunk(at);
    }
    // at least 32 bits in bitbuf (inpos is a multiple of 4 whenever nbits <= 32 here)
    INFL_HD void refill() {
        if (nbits <= 32) {
            stage(inpos);
            const uint32_t w = P::uni(*reinterpret_cast<const uint32_t*>(&s.inbuf[inpos - bufbase]));
            bitbuf |= (uint64_t)w << nbits;
            nbits += 32;
            inpos += 4;
        }
    }
    INFL_HD void drop(uint32_t n) {
        bitbuf >>= n;
        nbits -= n;
    }
    INFL_HD uint32_t bits(uint32_t n) {  // n <= 16, n <= nbits
        const uint32_t v = (uint32_t)bitbuf & ((1u << n) - 1);
        drop(n);
        return v;
    }
    INFL_HD uint32_t byte_pos() const { return inpos - (nbits >> 3); }  // after align()
    INFL_HD void align() { drop(nbits & 7); }
    INFL_HD bool exhausted() const { return inpos * 8 - nbits > stored * 8; }
    INFL_HD bool short_of(uint32_t n) const { return inpos * 8 - nbits + n > stored * 8; }  // fewer than n bits left
    // restart the bit buffer at stream byte `at`
    INFL_HD void seek(uint32_t at) {
        bitbuf = 0, nbits = 0, inpos = at;
        while (inpos & 3) {
            stage(inpos);
            bitbuf |= (uint64_t)P::uni(s.inbuf[inpos - bufbase]) << nbits;
            nbits += 8;
            inpos++;
        }
    }

    // ------------------------------------------------------------------ output
    // store bytes [flushed, flushed + n) of the window to dst and fold them into the Adler-32
    INFL_HD void flush(uint32_t n) {
        P::sync();
        uint32_t sa = 0, sw = 0;
        if (n == kFlush && dst8) {  // flushed is a multiple of kFlush: no wrap inside, 8-byte aligned
            const uint32_t w0 = flushed & kWinMask;
            for (uint32_t g = P::lane(); g < kFlush / 8; g += P::LANES) {
                const uint64_t v = *reinterpret_cast<const uint64_t*>(&s.win[w0 + 8 * g]);
                *reinterpret_cast<uint64_t*>(dst + flushed + 8 * g) = v;
                for (uint32_t k = 0; k < 8; k++) {
                    const uint32_t b = (uint32_t)(v >> (8 * k)) & 0xff;
                    sa += b;
                    sw += (kFlush - (8 * g + k)) * b;
                }
            }
        } else {
            for (uint32_t i = P::lane(); i < n; i += P::LANES) {
                const uint32_t b = s.win[(flushed + i) & kWinMask];
                dst[flushed + i] = (uint8_t)b;
                sa += b;
                sw += (n - i) * b;
            }
        }
        sa = P::sum(sa), sw = P::sum(sw);  // <= 512 * 255 and <= 512 * 512 * 255
        a2 = (a2 + n * a1 + sw) % kAdler;
        a1 = (a1 + sa) % kAdler;
        flushed += n;
    }
    INFL_HD void flush_full() {
        while (pos - flushed >= kFlush) flush(kFlush);
    }
    // len bytes from dist back (1 <= dist <= pos, dist <= 32768, pos + len <= D).  Byte j of the
    // copy is byte j % dist of the dist bytes before pos: only bytes produced before this copy are
    // read, so the lanes need no order among themselves whatever the overlap.
    INFL_HD void copy_match(uint32_t len, uint32_t dist) {
        P::sync();
        const uint32_t from = pos - dist;
        if (dist >= len) {
            for (uint32_t j = P::lane(); j < len; j += P::LANES)
                s.win[(pos + j) & kWinMask] = s.win[(from + j) & kWinMask];
        } else {
            for (uint32_t j = P::lane(); j < len; j += P::LANES)
                s.win[(pos + j) & kWinMask] = s.win[(from + j % dist) & kWinMask];
        }
        pos += len;
    }

    // ------------------------------------------------------------------ code tables
    static INFL_HD uint32_t reverse16(uint32_t c) {
        c = ((c & 0x5555u) << 1) | ((c >> 1) & 0x5555u);
        c = ((c & 0x3333u) << 2) | ((c >> 2) & 0x3333u);
        c = ((c & 0x0f0fu) << 4) | ((c >> 4) & 0x0f0fu);
        return ((c & 0x00ffu) << 8) | ((c >> 8) & 0x00ffu);
    }
    // Canonical codes of lens[0, n) into tab (1 << tb entries), cnt and sym.  Returns -1 for an
    // oversubscribed set, 1 for an incomplete one (tables built), 0 for a complete one; maxlen = the
    // longest code (0: no code at all).
    INFL_HD int build(const uint8_t* lens, uint32_t n, uint16_t* tab, uint32_t tb, uint16_t* cnt, uint16_t* sym,
                      uint32_t& maxlen) {
        P::sync();
        for (uint32_t i = P::lane(); i < (1u << tb); i += P::LANES) tab[i] = 0;
        for (uint32_t l = P::lane(); l < 16; l += P::LANES) {
            uint32_t c = 0;
            for (uint32_t i = 0; i < n; i++) c += lens[i] == l;
            cnt[l] = (uint16_t)(l ? c : 0);
        }
        P::sync();
        int32_t left = 1;
        uint32_t code = 0, off = 0;
        maxlen = 0;
        for (uint32_t l = 1; l < 16; l++) {
            const uint32_t c = P::uni(cnt[l]);
            left = (left << 1) - (int32_t)c;
            if (left < 0) return -1;
            if (c) maxlen = l;
            if (P::lane() == 0) s.first[l] = s.nxt[l] = (uint16_t)code, s.offs[l] = (uint16_t)off;
            code = (code + c) << 1;  // next[len + 1] = (next[len] + count[len]) << 1
            off += c;
        }
        P::sync();
        if (P::lane() == 0) {  // codes go to the symbols in symbol order
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t l = lens[i];
                if (l) s.code[i] = s.nxt[l]++;
            }
        }
        P::sync();
        for (uint32_t i = P::lane(); i < n; i += P::LANES) {
            const uint32_t l = lens[i];
            if (!l) continue;
            const uint32_t c = s.code[i];
            sym[s.offs[l] + (c - s.first[l])] = (uint16_t)i;
            if (l <= tb) {
                const uint16_t e = (uint16_t)(i << 4 | l);
                for (uint32_t k = reverse16(c) >> (16 - l); k < (1u << tb); k += 1u << l) tab[k] = e;
            }
        }
        P::sync();
        return left > 0 ? 1 : 0;
    }
    // the next symbol of a code (at least 15 bits are in bitbuf), or -1 when no code owns the bits
    INFL_HD int32_t decode(const uint16_t* tab, uint32_t tb, const uint16_t* cnt, const uint16_t* sym) {
        const uint32_t e = P::uni(tab[(uint32_t)bitbuf & ((1u << tb) - 1)]);
        if (e) {
            drop(e & 15);
            return (int32_t)(e >> 4);
        }
        // bit by bit, the code's most significant bit first
        uint32_t code = 0, first = 0, index = 0, b = (uint32_t)bitbuf;
        for (uint32_t l = 1; l < 16; l++) {
            code |= b & 1;
            b >>= 1;
            const uint32_t c = P::uni(cnt[l]);
            if (code < first + c) {
                drop(l);
                return (int32_t)P::uni(sym[index + (code - first)]);
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        return -1;
    }

    INFL_HD uint32_t fixed_tables() {
        if (fixed_ready) return OK;
        P::sync();
        for (uint32_t i = P::lane(); i < 320; i += P::LANES)
            s.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
        uint32_t m;
        build(s.lens, 288, s.ltab, kLitBits, s.lcount, s.lsym, m);
        build(s.lens + 288, 32, s.dtab, kDistBits, s.dcount, s.dsym, m);
        fixed_ready = true;
        return OK;
    }

    INFL_HD uint32_t dynamic_tables() {
        fixed_ready = false;
        refill();
        const uint32_t hlit = bits(5) + 257, hdist = bits(5) + 1, hclen = bits(4) + 4;
        if (hlit > 286 || hdist > 30) return BAD_CODE_LENGTHS;
        P::sync();
        if (P::lane() == 0)
            for (uint32_t i = 0; i < 19; i++) s.clens[i] = 0;
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (uint32_t i = 0; i < hclen; i++) {
            refill();
            const uint32_t v = bits(3);
            if (P::lane() == 0) s.clens[order[i]] = (uint8_t)v;
        }
        if (exhausted()) return INPUT_EXHAUSTED;
        uint32_t m;
        if (build(s.clens, 19, s.dtab, 7, s.dcount, s.dsym, m) != 0) return BAD_CODE_LENGTHS;
        const uint32_t total = hlit + hdist;
        uint32_t i = 0, prev = 0;
        while (i < total) {
            refill();
            const int32_t c = decode(s.dtab, 7, s.dcount, s.dsym);
            if (c < 0) return BAD_CODE_LENGTHS;  // (a complete code owns every bit pattern)
            uint32_t rep = 1, v = (uint32_t)c;
            if (c == 16) v = prev, rep = 3 + bits(2);
            else if (c == 17) v = 0, rep = 3 + bits(3);
            else if (c == 18) v = 0, rep = 11 + bits(7);
            if (exhausted()) return INPUT_EXHAUSTED;
            if ((c == 16 && i == 0) || rep > total - i) return BAD_CODE_LENGTHS;
            for (uint32_t k = P::lane(); k < rep; k += P::LANES) s.lens[i + k] = (uint8_t)v;
            i += rep;
            prev = v;
        }
        if (exhausted()) return INPUT_EXHAUSTED;
        P::sync();
        if (P::uni(s.lens[256]) == 0) return BAD_CODE_LENGTHS;
        int r = build(s.lens, hlit, s.ltab, kLitBits, s.lcount, s.lsym, m);
        if (r < 0 || (r > 0 && m != 1)) return BAD_CODE_LENGTHS;  // incomplete: only a single 1-bit code
        r = build(s.lens + hlit, hdist, s.dtab, kDistBits, s.dcount, s.dsym, m);
        if (r < 0 || (r > 0 && m > 1)) return BAD_CODE_LENGTHS;   // ... or, for distances, no code at all
        return OK;
    }

    // ------------------------------------------------------------------ blocks
    INFL_HD uint32_t stored_block() {
        align();
        refill();
        const uint32_t len = bits(16), nlen = bits(16);
        if (exhausted()) return INPUT_EXHAUSTED;
        if ((len ^ 0xffffu) != nlen) return STORED_LEN;
        const uint32_t at = byte_pos();  // at <= stored: not exhausted
        if (len > stored - at) return INPUT_EXHAUSTED;
        if (len > D - pos) return OUTPUT_OVERFLOW;
        for (uint32_t done = 0; done < len;) {
            const uint32_t n = len - done < 256 ? len - done : 256;
            P::sync();
            for (uint32_t j = P::lane(); j < n; j += P::LANES) s.win[(pos + j) & kWinMask] = src[at + done + j];
            pos += n;
            done += n;
            flush_full();
        }
        seek(at + len);
        return OK;
    }

    INFL_HD uint32_t coded_block() {
        for (;;) {
            refill();
            const int32_t sym = decode(s.ltab, kLitBits, s.lcount, s.lsym);
            if (sym < 0) return short_of(15) ? INPUT_EXHAUSTED : BAD_SYMBOL;
            // a symbol's bits are all taken before it is judged: a stream that ends inside one is
            // INPUT_EXHAUSTED, whatever the zeros behind its end would have meant
            uint32_t bad = OK, len = 0, dist = 0;
            if (sym > 256) {
                // lengths 257 ... 285: bases 3 ... 10 (no extra bits), then four symbols per extra-bit
                // count: 11, 13, 15, 17 (1) ... 131, 163, 195, 227 (5); 285 is 258
                const uint32_t ls = (uint32_t)sym - 257;
                if (ls >= 29) bad = BAD_SYMBOL;
                else {
                    if (ls < 8) len = 3 + ls;
                    else if (ls == 28) len = 258;
                    else {
                        const uint32_t e = (ls >> 2) - 1;
                        len = 3 + ((4 + (ls & 3)) << e) + bits(e);
                    }
                    refill();
                    const int32_t ds = decode(s.dtab, kDistBits, s.dcount, s.dsym);
                    if (ds < 0) return short_of(15) ? INPUT_EXHAUSTED : BAD_SYMBOL;
                    // distances 0 ... 29: 1 ... 4 (no extra bits), then two symbols per extra-bit
                    // count: 5, 7 (1), 9, 13 (2) ... 16385, 24577 (13)
                    if (ds >= 30) bad = BAD_SYMBOL;
                    else if (ds < 4) dist = 1 + (uint32_t)ds;
                    else {
                        const uint32_t e = ((uint32_t)ds >> 1) - 1;
                        dist = 1 + ((2 + ((uint32_t)ds & 1)) << e) + bits(e);
                    }
                }
            }
            if (exhausted()) return INPUT_EXHAUSTED;
            if (bad != OK) return bad;
            if (sym < 256) {
                if (pos >= D) return OUTPUT_OVERFLOW;
                if (P::lane() == 0) s.win[pos & kWinMask] = (uint8_t)sym;
                pos++;
            } else if (sym == 256) {
                return OK;
            } else {
                if (dist > pos) return BAD_DISTANCE;  // (dist <= 32768 by construction)
                if (len > D - pos) return OUTPUT_OVERFLOW;
                copy_match(len, dist);
            }
            flush_full();
        }
    }

    INFL_HD uint32_t run() {
        refill();
        const uint32_t cmf = bits(8), flg = bits(8);
        if (exhausted()) return INPUT_EXHAUSTED;
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (cmf * 256 + flg) % 31 != 0 || (flg & 32)) return BAD_HEADER;
        uint32_t last;
        do {
            refill();
            last = bits(1);
            const uint32_t type = bits(2);
            if (exhausted()) return INPUT_EXHAUSTED;
            uint32_t st;
            if (type == 0) st = stored_block();
            else if (type == 3) st = BAD_BLOCK_TYPE;
            else {
                st = type == 1 ? fixed_tables() : dynamic_tables();
                if (st == OK) st = coded_block();
            }
            if (st != OK) return st;
        } while (!last);
        align();
        refill();
        uint32_t want = 0;
        for (int k = 0; k < 4; k++) {
            if (k == 2) refill();
            want = want << 8 | bits(8);
        }
        if (exhausted()) return INPUT_EXHAUSTED;
        if (pos != D) return OUTPUT_SHORT;
        if (pos > flushed) flush(pos - flushed);
        // bytes behind the trailer are ignored, as zlib.decompress ignores them
        return want == (a2 << 16 | a1) ? OK : BAD_ADLER;
    }
};

// One zlib stream src[0, stored) into exactly dst[0, D): 0 or a Status.  stored < kMaxStored and
// D < kMaxOut are the caller's to check.
template <class P>
INFL_HD uint32_t inflate_zlib(const uint8_t* src, uint64_t stored, uint8_t* dst, uint64_t D, Scratch& s) {
    Inflater<P> z(src, stored, dst, D, s);
    return z.run();
}

}  // namespace inflate_core
