// Device Huffman decoding of baseline JPEG streams, the parts that host and device share:
//   * `pack`: the host's whole share of that path — marker parsing (jpeg_entropy.h's parse_header: the same streams are admitted),
//     removal of the byte stuffing, the restart-marker check and the tables in the form the kernels probe.  Plain C++ like
//     jpeg_entropy.h: no HIP, no global state, every read and write bounds-checked, a bad stream is an error code + message.
//   * `lane_decode`: what ONE lane of csrc/jpeg_huffman.hip does with one subsequence of the scan.  It is written once, here, so that
//     tools/jpeg_pack_check.cpp runs the very code of the kernels on the CPU under the host sanitizers.
//
// The scheme (Weissenberger & Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018): the unstuffed scan of every SEGMENT
// (the whole scan, or one restart interval) is cut into subsequences of kSubBytes.  The decoder's state at a subsequence boundary is
// (bit position, block-in-MCU index c, zig-zag slot z); a block is 64 slots whatever it codes (end-of-block jumps to 64), so the
// number of slots consumed since the segment's start gives the block, its component and the coefficient.  A subsequence decoded from
// a wrong state falls in step with the right one after a few codes (JPEG's Huffman codes self-synchronise), so: decode every
// subsequence from a guess, hand each exit state to the next subsequence and decode again where the entry state changed, until
// nothing changes; the first subsequence of a segment always starts from the true state (0, 0, 0), so after r rounds the first r
// subsequences are exact and the fixed point is THE decode, however long it takes to reach.
#pragma once
#include "jpeg_entropy.h"

#if defined(__HIPCC__)
#define VATL_HD __host__ __device__ __forceinline__
#else
#define VATL_HD inline
#endif

namespace vatl {
namespace jpeg {

constexpr int kSubBytes = 128;                  // one lane's share of the scan
constexpr int kSubBits = kSubBytes * 8;
constexpr int kSubWords = kSubBytes / 4;
constexpr int kSubsPerBlock = 256;              // lanes of a thread block: 32 KiB of scan
constexpr int kRowPitch32 = kSubWords + 1;      // dwords per subsequence in LDS: lane l's k-th dword lies on bank (33 l + k) mod 32 — lanes that read the same k never collide
constexpr int kSegCols = 4;                     // segment row: byte offset in the frame's packed scan, real bit length, first MCU, MCU count
// A lane walks a whole segment in the worst case (no self-synchronisation at all), once to find the states and once to write: ONE lane
// writes 2.0 MB/s of quality-100 noise and does both passes at 1.25 MB/s (tools/jpeg_lane_rate.hip, profiles/jpeg_huffman_notes.md), so
// a segment at the cap takes 0.39 s to write and 0.63 s in all.
constexpr int64_t kMaxSegmentBytes = 768LL << 10;
constexpr int kSegmentTooLong = kTooLarge + 1;  // refusal reason of `pack` alone (VATL_JPEG_SEGMENT_TOO_LONG): the probe admits such a stream, the host decoder takes it

// one Huffman table as the kernels stage it in LDS: jpeg_entropy.h's Huff without the one-probe `fast` table
struct HuffDev {
    uint16_t look[1 << kLookBits];
    int32_t maxcode[18];
    int32_t valoff[17];
    int32_t nvals;
    uint8_t vals[256];
};
constexpr int kHuffDevBytes = (int)sizeof(HuffDev);
constexpr int kHuffPerFrame = 6;                // [component][0: DC, 1: AC]
static_assert(kHuffDevBytes % 4 == 0, "HuffDev is staged as dwords");

// per-frame status of the device decode (VATL_JHUFF_* of include/vatl_hip.h)
enum { kStOk = 0, kStBadDc, kStBadAc, kStZeroRun, kStEndsEarly, kStBlocksShort, kStRestartUnread };

// boundary state: bits 0..4 the bit offset past the subsequence's end, 5..7 the block-in-MCU index, 8..13 the zig-zag slot; bit 15:
// no valid state (an invalid code was met on the way).  The upper half of the word a subsequence stores is the slots it consumed.
constexpr uint32_t kStateInvalid = 0x8000u;
VATL_HD uint32_t make_state(int prel, int c, int z) { return (uint32_t)(prel | (c << 5) | (z << 8)); }

// the 32 bits at bit position q of a scan kept as BIG-ENDIAN dwords with kRowPitch32 dwords per subsequence (q < 2^31 - 64)
VATL_HD uint32_t window(const uint32_t* words, int q) {
    const int w = q >> 5, sh = q & 31;
    const uint32_t hi = words[w + w / kSubWords], lo = words[(w + 1) + (w + 1) / kSubWords];
    return sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
}

// extend() and kNatural[] of jpeg_entropy.h for code that also runs on the device
VATL_HD int extend_bits(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }      // 1 <= s <= 15
VATL_HD int natural_of(int z) {
    constexpr uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return nat[z & 63];
}

// decode_symbol of jpeg_entropy.h on a 32-bit window: -> symbol and its code length, or -1
VATL_HD int device_symbol(uint32_t win, const HuffDev& h, int& len) {
    const unsigned e = h.look[win >> (32 - kLookBits)];
    if (e) { len = (int)(e >> 8); return (int)(e & 255u); }
    const int code16 = (int)(win >> 16);
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int code = code16 >> (16 - l);
        if (code <= h.maxcode[l]) {
            const int idx = code + h.valoff[l];
            if (idx < 0 || idx >= h.nvals || idx >= 256) return -1;
            len = l;
            return h.vals[idx];
        }
    }
    return -1;
}

// where the write pass puts coefficients: the frame's geometry and the bounds of its own coefficients
struct LaneOut {
    int16_t* coef;               // the frame's first coefficient
    int64_t frame_blocks;        // stores go to [0, 64 * frame_blocks)
    int64_t first_block;         // MCU-order index of the segment's first block in the frame: first MCU * blocks per MCU
    int samp, mcus_x, bw0, bwc;
    int64_t n0, nc;              // luma / chroma block counts
};

// MCU-order block index -> the block's place in the frame's coefficient layout (per component, block raster), or -1
VATL_HD int64_t block_address(const LaneOut& o, int64_t B, int bpm) {
    const int64_t m = B / bpm;
    const int ci = (int)(B - m * bpm), per2 = o.samp * o.samp;
    const int64_t y = m / o.mcus_x, x = m - y * o.mcus_x;
    int64_t blk;
    if (ci < per2) {
        const int v = ci / o.samp, h = ci - v * o.samp;
        blk = (y * o.samp + v) * o.bw0 + (x * o.samp + h);
    } else
        blk = o.n0 + (int64_t)(ci - per2) * o.nc + y * o.bwc + x;
    return blk >= 0 && blk < o.frame_blocks ? blk : -1;
}

struct LaneResult {
    uint32_t word;               // (slots consumed << 16) | exit state
    int status;                  // WRITE only: kSt*
    int remaining;               // WRITE only: real bits left in the segment when its last block ended, or -1 (it did not end here)
};

// One lane, one subsequence.  `words`: the staged scan (see `window`); the subsequence covers bits [q0, q0 + kSubBits) of it, the
// segment's real bits end at qend_seg (anything from there on is padding).  `entry`: the boundary state to start from.  `tables`:
// the frame's kHuffPerFrame tables.  `bpm`: blocks per MCU.
// WRITE = false: the speculative pass — an invalid code is normal and gives kStateInvalid; nothing is stored anywhere.
// WRITE = true: the entry state is the true one and `nstart` the slots consumed since the segment's start; the non-zero coefficients are
// stored (DC as its difference), decoding stops at `seg_slots`, and the conditions jpeg_entropy.h's decode_block rejects are reported.
// The loop runs once per code and a code takes a bit at least: kSubBits trips at the most.
template <bool WRITE>
VATL_HD LaneResult lane_decode(const uint32_t* words, int q0, int qend_seg, uint32_t entry, const HuffDev* tables, int bpm, int64_t nstart, int64_t seg_slots,
                               const LaneOut* out) {
    LaneResult r{kStateInvalid, kStOk, -1};
    if (entry & kStateInvalid) return r;
    int q = q0 + (int)(entry & 31u), c = (int)((entry >> 5) & 7u), z = (int)((entry >> 8) & 63u);
    if (c >= bpm) return r;
    const int sub_end = q0 + kSubBits, qend = sub_end < qend_seg ? sub_end : qend_seg;
    const int per2 = bpm == 1 ? 1 : bpm - 2;
    int64_t n = nstart;
    int slots = 0;
    if (WRITE && n >= seg_slots) return r;
    for (int it = 0; it < kSubBits && q < qend; ++it) {
        const int comp = c < per2 ? 0 : c - per2 + 1;
        const uint32_t win = window(words, q);
        int len = 0, znew, value = 0, zat = z;
        if (z == 0) {
            const int s = device_symbol(win, tables[comp * 2], len);
            if (s < 0 || s > 15) { if (WRITE) r.status = kStBadDc; return r; }
            if (s) { value = extend_bits((win << len) >> (32 - s), s); len += s; }
            znew = 1;
        } else {
            const int rs = device_symbol(win, tables[comp * 2 + 1], len);
            if (rs < 0) { if (WRITE) r.status = kStBadAc; return r; }
            const int run = rs >> 4, s = rs & 15;
            if (s) {
                zat = z + run;
                if (zat > 63) { if (WRITE) r.status = kStZeroRun; return r; }
                value = extend_bits((win << len) >> (32 - s), s);
                len += s;
                znew = zat + 1;
            } else if (run == 15) {
                znew = z + 16;
                if (znew > 64) { if (WRITE) r.status = kStZeroRun; return r; }
            } else znew = 64;
        }
        q += len;
        if (WRITE) {
            if (q > qend_seg) { r.status = kStEndsEarly; return r; }
            if (value) {
                const int64_t blk = block_address(*out, out->first_block + (n >> 6), bpm);
                if (blk >= 0) out->coef[blk * 64 + natural_of(zat)] = (int16_t)value;
            }
            n += znew - z;
        }
        slots += znew - z;
        z = znew;
        if (z == 64) {
            z = 0;
            c = c + 1 == bpm ? 0 : c + 1;
            if (WRITE && n >= seg_slots) { r.remaining = qend_seg - q; return r; }
        }
    }
    const int prel = q > sub_end ? q - sub_end : 0;
    r.word = ((uint32_t)(slots > 0xffff ? 0xffff : slots) << 16) | make_state(prel > 31 ? 31 : prel, c, z);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// host: bytes -> packed frame
// ---------------------------------------------------------------------------------------------------------------------

inline void huff_to_dev(const Huff& h, HuffDev& d) {
    memset(&d, 0, sizeof(d));
    memcpy(d.look, h.look, sizeof(d.look));
    memcpy(d.maxcode, h.maxcode, sizeof(d.maxcode));
    memcpy(d.valoff + 1, h.valoff + 1, sizeof(int32_t) * 16);        // ([0] is never set or read)
    d.nvals = h.nvals;
    memcpy(d.vals, h.vals, (size_t)h.nvals);
}

// how many restart intervals (segments) the admitted header H declares
inline int64_t segment_count(const Header& H) {
    const int64_t mcus = (int64_t)H.desc[kMcusX] * H.desc[kMcusY], ri = H.desc[kRestart];
    return ri > 0 && ri < mcus ? (mcus + ri - 1) / ri : 1;
}

// Capacities that `pack` needs for this stream: scan bytes (an upper bound) and segment rows.  0, or kErrArg for a refused stream.
inline int pack_size(const uint8_t* data, int64_t n, int64_t* scan_capacity, int64_t* segment_rows, const Msg& msg) {
    if (!data || !scan_capacity || !segment_rows || n < 0) return msg.set(kErrArg, "jpeg pack: null pointer");
    Header H;
    parse_header(data, n, H, msg);
    if (!H.desc[kAdmitted]) return kErrArg;
    const int64_t segs = segment_count(H);
    *segment_rows = segs;
    *scan_capacity = ((data + n) - H.scan) + segs * kSubBytes;       // every segment is padded to whole subsequences, an empty one gets one
    return 0;
}

// File bytes -> scan[0 .. used[0]) (stuffing removed, cut at the markers, every segment zero-padded to whole subsequences), segment
// rows[0 .. used[1]) of kSegCols int32, huff (kHuffPerFrame HuffDev), qt[3][64] and the descriptor — qt and desc as entropy_decode
// gives them.  0 on success; kErrArg for a refused stream (desc holds the reason; a segment above kMaxSegmentBytes is refused here
// with kSegmentTooLong) or capacities too small, kErrStream for a missing table or restart marker.
inline int pack(const uint8_t* data, int64_t n, uint8_t* scan, int64_t scan_capacity, int32_t* rows, int64_t row_capacity, uint8_t* huff, uint16_t* qt,
                int32_t* desc, int64_t* used, const Msg& msg) {
    if (!data || !scan || !rows || !huff || !qt || !desc || !used || n < 0) return msg.set(kErrArg, "jpeg pack: null pointer");
    Header H;
    parse_header(data, n, H, msg);
    memcpy(desc, H.desc, sizeof(H.desc));
    if (!H.desc[kAdmitted]) return kErrArg;
    const int nc = H.desc[kComponents];
    for (int c = 0; c < nc; ++c) {
        if (!H.qt_present[H.comp[c].tq]) return msg.set(kErrStream, "jpeg: quantiser table %d is not defined", H.comp[c].tq);
        if (!H.dc[H.comp[c].td].present || !H.ac[H.comp[c].ta].present) return msg.set(kErrStream, "jpeg: Huffman table %d/%d is not defined", H.comp[c].td, H.comp[c].ta);
    }
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) qt[c * 64 + i] = c < nc ? H.qt[H.comp[c].tq][i] : 0;
    for (int c = 0; c < 3; ++c) {
        HuffDev d[2];
        huff_to_dev(H.dc[H.comp[c < nc ? c : 0].td], d[0]);
        huff_to_dev(H.ac[H.comp[c < nc ? c : 0].ta], d[1]);
        memcpy(huff + (size_t)c * 2 * sizeof(HuffDev), d, sizeof(d));
    }
    const int64_t segs = segment_count(H), mcus = (int64_t)H.desc[kMcusX] * H.desc[kMcusY];
    const int64_t ri = segs > 1 ? H.desc[kRestart] : mcus;
    if (row_capacity < segs) return msg.set(kErrArg, "jpeg pack: %lld segments do not fit %lld rows", (long long)segs, (long long)row_capacity);
    const uint8_t* p = H.scan;
    const uint8_t* const end = data + n;
    int64_t at = 0;                                                  // bytes of `scan` written
    for (int64_t s = 0; s < segs; ++s) {
        const int64_t first = at;
        while (p < end) {                                            // up to the first marker (or a lone FF at the very end), like Bits::fill
            const uint8_t b = *p;
            if (b == 0xFF) {
                if (end - p >= 2 && p[1] == 0x00) p += 2; else break;
            } else ++p;
            if (at >= scan_capacity || at >= 0x7fff0000) return msg.set(kErrArg, "jpeg pack: the scan does not fit %lld bytes", (long long)scan_capacity);   // (rows hold int32 offsets)
            scan[at++] = b;
        }
        const int64_t bytes = at - first;
        if (bytes > kMaxSegmentBytes) {
            desc[kAdmitted] = 0; desc[kRefusal] = kSegmentTooLong;
            return msg.set(kErrArg, "a segment of %lld bytes between restart markers: more than %lld are not Huffman-decoded on the device", (long long)bytes, (long long)kMaxSegmentBytes);
        }
        const int64_t padded = bytes ? (bytes + kSubBytes - 1) / kSubBytes * kSubBytes : kSubBytes;
        if (first + padded > scan_capacity) return msg.set(kErrArg, "jpeg pack: the scan does not fit %lld bytes", (long long)scan_capacity);
        memset(scan + at, 0, (size_t)(first + padded - at));
        at = first + padded;
        int32_t* row = rows + s * kSegCols;
        row[0] = (int32_t)first; row[1] = (int32_t)(bytes * 8); row[2] = (int32_t)(s * ri); row[3] = (int32_t)(s + 1 < segs ? ri : mcus - s * ri);
        if (s + 1 < segs) {                                          // RSTm right here, FF fill bytes allowed, the number counted modulo 8: entropy_decode's rule
            while (end - p >= 2 && p[0] == 0xFF && p[1] == 0xFF) ++p;
            const int want = 0xD0 + (int)(s & 7);
            if (end - p < 2 || p[0] != 0xFF || p[1] != want)
                return msg.set(kErrStream, "jpeg: restart marker RST%d missing before MCU %lld of %lld", want - 0xD0, (long long)((s + 1) * ri), (long long)mcus);
            p += 2;
        }
    }
    used[0] = at; used[1] = segs;
    return 0;
}

}  // namespace jpeg
}  // namespace vatl
