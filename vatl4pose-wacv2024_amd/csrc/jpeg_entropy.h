// Host half of the hybrid JPEG decoder: marker parser + Huffman decoder of baseline sequential streams (ITU-T T.81, SOF0, 8 bit).
//   alphapose/datasets/coco_video.py `_read_rgb` -> Pillow -> libjpeg: the serial part of what that call does.
// Plain C++ with no HIP and no global state (jpeg.hip includes it; tools/jpeg_entropy_check.cpp builds it alone under the host
// sanitizers).  The input is file bytes, so NOTHING here trusts it: every stream read goes through `Bits` / `Reader`, which never
// step past `end`, every coefficient write is inside the block the caller counted, and every index taken from the stream
// (table ids, sampling factors, run lengths, symbol sizes) is range-checked.  A bad stream is an error code + message, never a fault.
//
// Output: int16 coefficients in NATURAL order, not dequantised, per component in block-raster order over the component's padded
// block grid (de-interleaved from MCU order) — the layout jpeg.hip's IDCT kernel walks; the quantiser tables per component in natural order;
// and the frame descriptor below.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace vatl {
namespace jpeg {

// the frame descriptor: int32[kDescInts], laid out as include/vatl_hip.h documents it (VATL_JPEG_DESC_INTS; jpeg.hip static_asserts the
// length and the refusal codes below against that header, tests/test_jpeg_tables.py the header against vatl_hip.JPEG_REFUSALS)
enum { kAdmitted = 0, kRefusal, kHeight, kWidth, kComponents, kSampling /* 1: all 1x1, 2: luma 2x2 */, kMcusX, kMcusY, kBw0, kBh0, kBwC, kBhC,
       kBlocks /* all components */, kRestart, kScanOffset /* byte offset of the entropy-coded segment */, kReserved, kDescInts };

// why the probe refuses a stream (descriptor[kRefusal]; 0 = admitted)
enum Refusal { kOk = 0, kNotJpeg, kBadHeader, kNotBaseline, kPrecision, kComponentCount, kSamplingFactors, kTooSmall, kMultipleScans, kColourSpace, kQuantPrecision, kTooLarge };

constexpr int64_t kMaxPixels = 1LL << 26;     // frames above this (8192 x 8192) are refused: 192 MB of coefficients at 4:2:0

// decode errors (negative like the library's VATL_E* codes; -1 is VATL_EINVAL)
enum { kErrArg = -1, kErrStream = -3 };

static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Msg {                       // caller-owned message buffer (the library passes its thread-local one)
    char* buf;
    int cap;
    int set(int code, const char* fmt, ...) const {
        if (buf && cap > 0) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(buf, (size_t)cap, fmt, ap);
            va_end(ap);
        }
        return code;
    }
};

constexpr int kLookBits = 9;

struct Huff {
    bool present = false;
    uint16_t look[1 << kLookBits];   // (length << 8) | symbol for codes of <= kLookBits bits; 0: longer
    int32_t maxcode[18];             // largest code of each length (-1: none), [17] = sentinel
    int32_t valoff[17];              // symbol index = code + valoff[length]
    uint8_t vals[256];
    int nvals = 0;
    // AC tables: where a code AND the magnitude bits behind it fit the look-ahead, the whole coefficient in one probe —
    // (value << 8) | (zero run << 4) | (bits used); 0: take the two-step path.  Most coefficients of a photograph are this short.
    int16_t fast[1 << kLookBits];
};

struct Component { int id = 0, h = 0, v = 0, tq = 0, td = 0, ta = 0; };

struct Header {
    int32_t desc[kDescInts];
    Component comp[4];
    uint16_t qt[4][64];              // natural order
    bool qt_present[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    bool saw_sof = false, saw_jfif = false, saw_adobe = false;
    int adobe_transform = 0;
    const uint8_t* scan = nullptr;   // first byte of the entropy-coded segment (set when admitted)
};

// ---------------------------------------------------------------------------------------------------------------------
// marker segments
// ---------------------------------------------------------------------------------------------------------------------

struct Reader {                    // bounds-checked big-endian reads; `ok` goes false (and stays) on the first read past the end
    const uint8_t* p;
    const uint8_t* end;
    bool ok = true;
    int64_t left() const { return end - p; }
    int u8() { if (p < end) return *p++; ok = false; return 0; }
    int u16() { const int a = u8(); return (a << 8) | u8(); }
    void skip(int64_t n) { if (n < 0 || n > left()) { ok = false; p = end; } else p += n; }
};

inline bool build_huff(Huff& h, const uint8_t counts[16], const uint8_t* syms, int nsyms) {
    int total = 0;
    for (int i = 0; i < 16; ++i) total += counts[i];
    if (total > 256 || total != nsyms) return false;
    memset(h.look, 0, sizeof(h.look));
    memcpy(h.vals, syms, (size_t)total);
    h.nvals = total;
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int n = counts[len - 1];
        h.valoff[len] = k - code;
        if (n) {
            if (code + n > (1 << len)) return false;                 // more codes than the length has: not a prefix code
            if (len <= kLookBits)
                for (int i = 0; i < n; ++i) {
                    const int first = (code + i) << (kLookBits - len), span = 1 << (kLookBits - len);
                    for (int j = 0; j < span; ++j) h.look[first + j] = (uint16_t)((len << 8) | syms[k + i]);
                }
            code += n; k += n;
            h.maxcode[len] = code - 1;
        } else h.maxcode[len] = -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    for (int i = 0; i < (1 << kLookBits); ++i) {
        h.fast[i] = 0;
        const int len = h.look[i] >> 8, run = (h.look[i] & 255) >> 4, mag = h.look[i] & 15;
        if (len && mag && len + mag <= kLookBits) {
            const int v = ((i << len) & ((1 << kLookBits) - 1)) >> (kLookBits - mag);
            const int value = v < (1 << (mag - 1)) ? v - (1 << mag) + 1 : v;
            if (value >= -128 && value <= 127)                                               // the upper byte is signed: a size-8 symbol on a 1-bit code
                h.fast[i] = (int16_t)(value * 256 + run * 16 + len + mag);                   // (values 128 .. 255) takes the two-step path
        }
    }
    h.present = true;
    return true;
}

// Parses the marker segments up to and including the first SOS header.  Returns 0 with the descriptor filled — admitted or refused
// with a reason in `msg` — and r.p at the first entropy-coded byte; a stream that is no JPEG or whose header is cut short is a refusal too.
inline int parse_header(const uint8_t* data, int64_t n, Header& H, const Msg& msg) {
    memset(H.desc, 0, sizeof(H.desc));
    auto refuse = [&](int why) { H.desc[kAdmitted] = 0; H.desc[kRefusal] = why; return 0; };
    if (!data || n < 4 || data[0] != 0xFF || data[1] != 0xD8) { msg.set(0, "not a JPEG stream (no SOI marker)"); return refuse(kNotJpeg); }
    Reader r{data + 2, data + n};
    for (;;) {
        int b = r.u8();
        if (!r.ok) { msg.set(0, "header ends before a scan starts"); return refuse(kBadHeader); }
        if (b != 0xFF) continue;                                     // (garbage between segments: skipped like libjpeg's next_marker)
        int m = r.u8();
        while (m == 0xFF && r.ok) m = r.u8();                        // fill bytes
        if (!r.ok) { msg.set(0, "header ends before a scan starts"); return refuse(kBadHeader); }
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // stand-alone markers
        if (m == 0xD9) { msg.set(0, "EOI before any scan"); return refuse(kBadHeader); }
        const int len = r.u16();
        if (!r.ok || len < 2 || len - 2 > r.left()) { msg.set(0, "marker segment 0x%02X runs past the end of the stream", m); return refuse(kBadHeader); }
        Reader s{r.p, r.p + (len - 2)};
        r.skip(len - 2);
        if (m == 0xC0 || (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC)) {
            if (m != 0xC0) {
                msg.set(0, "%s (SOF%d): only baseline sequential Huffman streams are decoded on the device",
                        m == 0xC2 ? "progressive" : m == 0xC1 ? "extended sequential" : m >= 0xC9 ? "arithmetic-coded" : "not baseline", m - 0xC0);
                return refuse(kNotBaseline);
            }
            if (H.saw_sof) { msg.set(0, "two frame headers"); return refuse(kBadHeader); }
            const int prec = s.u8(), h = s.u16(), w = s.u16(), nc = s.u8();
            if (!s.ok) { msg.set(0, "frame header cut short"); return refuse(kBadHeader); }
            if (prec != 8) { msg.set(0, "%d-bit samples", prec); return refuse(kPrecision); }
            if (nc != 1 && nc != 3) { msg.set(0, "%d components (1 or 3 are decoded on the device)", nc); return refuse(kComponentCount); }
            if (h == 0 || w == 0) { msg.set(0, "frame of %dx%d (a height of 0 is defined by a later DNL marker)", h, w); return refuse(kBadHeader); }
            for (int c = 0; c < nc; ++c) {
                H.comp[c].id = s.u8();
                const int hv = s.u8();
                H.comp[c].h = hv >> 4; H.comp[c].v = hv & 15;
                H.comp[c].tq = s.u8();
                if (H.comp[c].tq > 3) { msg.set(0, "quantiser table index %d", H.comp[c].tq); return refuse(kBadHeader); }
            }
            if (!s.ok) { msg.set(0, "frame header cut short"); return refuse(kBadHeader); }
            int samp = 0;
            if (nc == 1) samp = (H.comp[0].h == 1 && H.comp[0].v == 1) ? 1 : 0;
            else if (H.comp[1].h == 1 && H.comp[1].v == 1 && H.comp[2].h == 1 && H.comp[2].v == 1)
                samp = (H.comp[0].h == 1 && H.comp[0].v == 1) ? 1 : (H.comp[0].h == 2 && H.comp[0].v == 2) ? 2 : 0;
            H.desc[kHeight] = h; H.desc[kWidth] = w; H.desc[kComponents] = nc; H.desc[kSampling] = samp;
            if (!samp) {
                msg.set(0, "sampling %dx%d,%dx%d,%dx%d (4:4:4 and 4:2:0 are decoded on the device)", H.comp[0].h, H.comp[0].v, H.comp[1].h, H.comp[1].v, H.comp[2].h, H.comp[2].v);
                return refuse(kSamplingFactors);
            }
            if (h < 8 || w < 8) { msg.set(0, "frame of %dx%d: height and width under 8 are not decoded on the device", h, w); return refuse(kTooSmall); }
            if ((int64_t)h * w > kMaxPixels) { msg.set(0, "frame of %dx%d: more than 2^26 pixels are not decoded on the device", h, w); return refuse(kTooLarge); }
            const int mcu = 8 * samp, mx = (w + mcu - 1) / mcu, my = (h + mcu - 1) / mcu;
            H.desc[kMcusX] = mx; H.desc[kMcusY] = my;
            H.desc[kBw0] = mx * samp; H.desc[kBh0] = my * samp;
            H.desc[kBwC] = nc == 3 ? mx : 0; H.desc[kBhC] = nc == 3 ? my : 0;
            const int64_t blocks = (int64_t)H.desc[kBw0] * H.desc[kBh0] + 2LL * H.desc[kBwC] * H.desc[kBhC];    // <= 1.5 * 8192^2: fits
            H.desc[kBlocks] = (int32_t)blocks;
            H.saw_sof = true;
        } else if (m == 0xC4) {                                      // DHT
            while (s.left() > 0) {
                const int tc_th = s.u8();
                uint8_t counts[16];
                int total = 0;
                for (int i = 0; i < 16; ++i) { counts[i] = (uint8_t)s.u8(); total += counts[i]; }
                if (!s.ok || (tc_th >> 4) > 1 || (tc_th & 15) > 3 || total > 256 || total > s.left()) { msg.set(0, "bad Huffman table definition"); return refuse(kBadHeader); }
                Huff& t = (tc_th >> 4) ? H.ac[tc_th & 15] : H.dc[tc_th & 15];
                if (!build_huff(t, counts, s.p, total)) { msg.set(0, "Huffman table is not a prefix code"); return refuse(kBadHeader); }
                s.skip(total);
            }
        } else if (m == 0xDB) {                                      // DQT
            while (s.left() > 0) {
                const int pq_tq = s.u8();
                if ((pq_tq & 15) > 3) { msg.set(0, "quantiser table index %d", pq_tq & 15); return refuse(kBadHeader); }
                if (pq_tq >> 4) { msg.set(0, "16-bit quantiser table"); return refuse(kQuantPrecision); }
                if (s.left() < 64) { msg.set(0, "quantiser table cut short"); return refuse(kBadHeader); }
                for (int i = 0; i < 64; ++i) H.qt[pq_tq & 15][kNatural[i]] = (uint16_t)s.u8();
                H.qt_present[pq_tq & 15] = true;
            }
        } else if (m == 0xDD) {                                      // DRI
            const int ri = s.u16();
            if (!s.ok) { msg.set(0, "restart interval cut short"); return refuse(kBadHeader); }
            H.desc[kRestart] = ri;
        } else if (m == 0xE0) {
            if (s.left() >= 5 && !memcmp(s.p, "JFIF\0", 5)) H.saw_jfif = true;
        } else if (m == 0xEE) {
            if (s.left() >= 12 && !memcmp(s.p, "Adobe", 5)) { H.saw_adobe = true; H.adobe_transform = s.p[11]; }
        } else if (m == 0xDA) {                                      // SOS
            if (!H.saw_sof) { msg.set(0, "scan before the frame header"); return refuse(kBadHeader); }
            const int nc = H.desc[kComponents], ns = s.u8();
            if (!s.ok || ns < 1 || ns > 4 || s.left() < 2 * ns + 3) { msg.set(0, "scan header cut short"); return refuse(kBadHeader); }
            if (ns != nc) { msg.set(0, "first scan holds %d of %d components: several scans are not decoded on the device", ns, nc); return refuse(kMultipleScans); }
            for (int c = 0; c < ns; ++c) {
                const int id = s.u8(), tdta = s.u8();
                if (id != H.comp[c].id) { msg.set(0, "scan components out of frame order"); return refuse(kMultipleScans); }
                H.comp[c].td = tdta >> 4; H.comp[c].ta = tdta & 15;
                if (H.comp[c].td > 3 || H.comp[c].ta > 3) { msg.set(0, "Huffman table index out of range"); return refuse(kBadHeader); }
            }
            const int ss = s.u8(), se = s.u8(), ahal = s.u8();
            if (ss != 0 || se != 63 || ahal != 0) { msg.set(0, "spectral selection %d..%d / approximation 0x%02X in a baseline scan", ss, se, ahal); return refuse(kNotBaseline); }
            // libjpeg's colour-space guess for three components (jdapimin.c default_decompress_parms): Pillow converts only YCbCr
            if (nc == 3 && !H.saw_jfif) {
                const bool rgb_ids = H.comp[0].id == 'R' && H.comp[1].id == 'G' && H.comp[2].id == 'B';
                if (H.saw_adobe ? H.adobe_transform != 1 : rgb_ids) { msg.set(0, "three components that are not YCbCr"); return refuse(kColourSpace); }
            }
            H.desc[kScanOffset] = (int32_t)((r.p - data) < 0x7fffffff ? (r.p - data) : 0x7fffffff);
            // a block costs two bits at the very least (a 1-bit DC code and a 1-bit end-of-block): a header that declares more blocks than the
            // scan can hold must not size anybody's buffers
            if ((int64_t)H.desc[kBlocks] > 4 * (int64_t)((data + n) - r.p)) {
                msg.set(0, "%d blocks declared, %lld bytes of scan: too short for its frame", H.desc[kBlocks], (long long)((data + n) - r.p));
                return refuse(kBadHeader);
            }
            H.desc[kAdmitted] = 1;
            if (msg.buf && msg.cap > 0) msg.buf[0] = 0;
            H.scan = r.p;
            return 0;
        }
        // everything else (APPn, COM, DNL, ...): skipped
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// entropy-coded segment
// ---------------------------------------------------------------------------------------------------------------------

struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;              // the low `n` bits are the unread bits, oldest highest
    int n = 0;
    int pad = 0;                   // how many of them (the youngest) are zeros invented past a marker / the end of the stream

    // >= 57 bits afterwards.  Stuffed FF00 -> FF; any other FFxx is a marker: it stays unread and zeros are fed instead.
    void fill() {
        if (end - p >= 8 && n <= 56) {                               // up to 7 bytes at once when none of the next 8 is 0xFF
            uint64_t x;
            memcpy(&x, p, 8);
            x = __builtin_bswap64(x);
            const uint64_t y = ~x;                                   // a 0xFF byte of x is a zero byte of y
            if (!((y - 0x0101010101010101ull) & ~y & 0x8080808080808080ull)) {
                const int k = (64 - n) >> 3 > 7 ? 7 : (64 - n) >> 3;   // 1 .. 7 whole bytes
                acc = (acc << (8 * k)) | (x >> (64 - 8 * k));
                n += 8 * k; p += k;
            }
        }
        while (n <= 56) {
            unsigned b = 0;
            if (p < end) {
                b = *p;
                if (b != 0xFF) ++p;
                else if (end - p >= 2 && p[1] == 0x00) p += 2;
                else { b = 0; pad += 8; }                            // a marker (or a lone FF at the very end)
            } else pad += 8;
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)((acc >> (n - k)) & ((1u << k) - 1u)); }      // 1 <= k <= 16 <= n
    void drop(int k) { n -= k; }
    bool overrun() const { return n < pad; }                         // bits were consumed that the stream does not hold
    void restart() { acc = 0; n = 0; pad = 0; }
};

// -> symbol, or -1 when no code of the table matches.  Needs >= 16 unread bits.
inline int decode_symbol(Bits& b, const Huff& h) {
    const unsigned e = h.look[b.peek(kLookBits)];
    if (e) { b.drop((int)(e >> 8)); return (int)(e & 255u); }
    const int code16 = (int)b.peek(16);
    for (int len = kLookBits + 1; len <= 16; ++len) {
        const int code = code16 >> (16 - len);
        if (code <= h.maxcode[len]) {
            const int idx = code + h.valoff[len];
            if (idx < 0 || idx >= h.nvals) return -1;
            b.drop(len);
            return h.vals[idx];
        }
    }
    return -1;
}

inline int extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }      // 1 <= s <= 15

// One 8x8 block into out[64] (natural order; the caller zeroed it).  0, or -1 with the reason in *why.
inline int decode_block(Bits& b, const Huff& dc, const Huff& ac, int& pred, int16_t* out, const char** why) {
    if (b.n < 32) b.fill();                                          // a symbol takes <= 16 code bits + <= 15 magnitude bits
    int s = decode_symbol(b, dc);
    if (s < 0 || s > 15) { *why = "bad DC code"; return -1; }
    if (s) { const unsigned v = b.peek(s); b.drop(s); pred += extend(v, s); }
    pred = (int16_t)pred;                                            // a valid stream stays inside 12 bits; a corrupt one wraps instead of growing
    out[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        if (b.n < 32) b.fill();
        const int f = ac.fast[b.peek(kLookBits)];
        if (f) {                                                     // run, size and value in one probe
            k += (f >> 4) & 15;
            if (k > 63) { *why = "zero run past coefficient 63"; return -1; }
            b.drop(f & 15);
            out[kNatural[k++]] = (int16_t)(f >> 8);
            continue;
        }
        const int rs = decode_symbol(b, ac);
        if (rs < 0) { *why = "bad AC code"; return -1; }
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) { *why = "zero run past coefficient 63"; return -1; }
            const unsigned v = b.peek(s); b.drop(s);
            out[kNatural[k]] = (int16_t)extend(v, s);
            ++k;
        } else if (r == 15) {
            k += 16;
            if (k > 64) { *why = "zero run past coefficient 63"; return -1; }
        } else break;                                                // EOB (r < 15 with s == 0 ends the block like libjpeg's baseline decoder)
    }
    if (b.overrun()) { *why = "entropy-coded data ends early"; return -1; }
    return 0;
}

// Bytes -> coefficients (coef[0 .. 64 * blocks), zero-filled first), per-component quantiser tables qt[3][64] and the descriptor.
// 0 on success; kErrArg for a capacity that is too small / a refused stream, kErrStream for a corrupt one.
inline int entropy_decode(const uint8_t* data, int64_t n, int16_t* coef, int64_t coef_capacity, uint16_t* qt, int32_t* desc, const Msg& msg) {
    if (!data || !coef || !qt || !desc || n < 0) return msg.set(kErrArg, "jpeg entropy decode: null pointer");
    Header H;
    parse_header(data, n, H, msg);
    memcpy(desc, H.desc, sizeof(H.desc));
    if (!H.desc[kAdmitted]) return kErrArg;                          // (msg holds the probe's reason)
    const int nc = H.desc[kComponents], samp = H.desc[kSampling];
    const int64_t blocks = H.desc[kBlocks];
    if (coef_capacity < blocks * 64) return msg.set(kErrArg, "jpeg entropy decode: %lld coefficients do not fit a capacity of %lld", (long long)(blocks * 64), (long long)coef_capacity);
    for (int c = 0; c < nc; ++c) {
        if (!H.qt_present[H.comp[c].tq]) return msg.set(kErrStream, "jpeg: quantiser table %d is not defined", H.comp[c].tq);
        if (!H.dc[H.comp[c].td].present || !H.ac[H.comp[c].ta].present) return msg.set(kErrStream, "jpeg: Huffman table %d/%d is not defined", H.comp[c].td, H.comp[c].ta);
    }
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) qt[c * 64 + i] = c < nc ? H.qt[H.comp[c].tq][i] : 0;
    memset(coef, 0, (size_t)blocks * 64 * sizeof(int16_t));

    const int bw[3] = {H.desc[kBw0], H.desc[kBwC], H.desc[kBwC]};
    const int64_t first[3] = {0, (int64_t)H.desc[kBw0] * H.desc[kBh0], (int64_t)H.desc[kBw0] * H.desc[kBh0] + (int64_t)H.desc[kBwC] * H.desc[kBhC]};
    const int per[3] = {samp, 1, 1};                                 // blocks per MCU along each axis
    const int mx = H.desc[kMcusX], my = H.desc[kMcusY], ri = H.desc[kRestart];
    Bits b{H.scan, data + n};
    int pred[3] = {0, 0, 0};
    int64_t mcu = 0;
    const int64_t mcus = (int64_t)mx * my;
    const char* why = "";
    for (int y = 0; y < my; ++y)
        for (int x = 0; x < mx; ++x, ++mcu) {
            if (ri && mcu && mcu % ri == 0) {                        // RSTm sits byte-aligned right behind the interval's last bits
                const uint8_t* p = b.p;
                while (b.end - p >= 2 && p[0] == 0xFF && p[1] == 0xFF) ++p;
                const int want = 0xD0 + (int)((mcu / ri - 1) & 7);
                if (b.n - b.pad >= 8 || b.end - p < 2 || p[0] != 0xFF || p[1] != want)
                    return msg.set(kErrStream, "jpeg: restart marker RST%d missing before MCU %lld of %lld", want - 0xD0, (long long)mcu, (long long)mcus);
                b.p = p + 2;
                b.restart();
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < nc; ++c)
                for (int v = 0; v < per[c]; ++v)
                    for (int h = 0; h < per[c]; ++h) {
                        const int64_t blk = first[c] + (int64_t)(y * per[c] + v) * bw[c] + (x * per[c] + h);     // < blocks: (y, x) < (my, mx), bw = mx * per
                        if (decode_block(b, H.dc[H.comp[c].td], H.ac[H.comp[c].ta], pred[c], coef + blk * 64, &why))
                            return msg.set(kErrStream, "jpeg: %s in MCU %lld of %lld", why, (long long)mcu, (long long)mcus);
                    }
        }
    return 0;
}

}  // namespace jpeg
}  // namespace vatl
