// Stand-alone run of the host half of the device Huffman decoder (csrc/jpeg_pack.h `pack`) AND of the code one lane of
// csrc/jpeg_huffman.hip runs (`lane_decode`, the same source) for the host sanitizers — CPU only, no HIP, no Python:
//
//   python tools/make_jpeg_golden.py --dump-streams /tmp/jpeg_streams
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ivatl4pose-wacv2024_amd/csrc \
//       tools/jpeg_pack_check.cpp -o /tmp/jpeg_pack_check -lpthread
//   /tmp/jpeg_pack_check /tmp/jpeg_streams/*.bin
//
// Every file is packed from a heap copy of EXACTLY the stream's length into buffers of EXACTLY the sizes `pack_size` asks for, once on
// the main thread and once on eight threads at the same time, whose results must agree.  What packs is then decoded the way the
// kernels do it — every subsequence from a guess, exit states handed on until nothing changes, prefix sum, write pass, DC pass,
// closing checks — with the scan staged like the kernels' LDS image in a buffer of exactly that size, and the outcome must be the
// host decoder's: the same coefficients where `entropy_decode` succeeds, a non-zero status where it fails.
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "jpeg_pack.h"

using namespace vatl::jpeg;

struct Packed {
    int rc = 0, admitted = 0;
    std::vector<uint8_t> scan, huff;
    std::vector<int32_t> rows;
    std::vector<uint16_t> qt;
    std::vector<int32_t> desc;
    bool operator==(const Packed& o) const { return rc == o.rc && admitted == o.admitted && scan == o.scan && huff == o.huff && rows == o.rows && qt == o.qt && desc == o.desc; }
};

static Packed run_pack(const std::vector<uint8_t>& file) {
    Packed r;
    uint8_t* data = (uint8_t*)malloc(file.size() ? file.size() : 1);          // exact size: no slack behind the stream
    memcpy(data, file.data(), file.size());
    char text[256] = "";
    Msg msg{text, (int)sizeof(text)};
    int64_t cap = 0, nrows = 0;
    r.rc = pack_size(data, (int64_t)file.size(), &cap, &nrows, msg);
    if (r.rc == 0) {
        r.admitted = 1;
        r.scan.assign((size_t)cap, 0xa5); r.rows.assign((size_t)nrows * kSegCols, -1); r.huff.assign((size_t)kHuffPerFrame * kHuffDevBytes, 0);
        r.qt.assign(3 * 64, 0); r.desc.assign(kDescInts, 0);
        int64_t used[2] = {0, 0};
        r.rc = pack(data, (int64_t)file.size(), r.scan.data(), cap, r.rows.data(), nrows, r.huff.data(), r.qt.data(), r.desc.data(), used, msg);
        if (r.rc == 0) { r.scan.resize((size_t)used[0]); r.rows.resize((size_t)used[1] * kSegCols); }
        else { r.scan.clear(); r.rows.clear(); if (!r.desc[kAdmitted]) r.admitted = 0; }          // (a segment above the cap: refused by pack alone)
    }
    free(data);
    return r;
}

// the kernels' schedule on one thread: -> status, coefficients in `coef` (sized by the descriptor)
static int emulate(const Packed& P, std::vector<int16_t>& coef) {
    const int32_t* d = P.desc.data();
    const int64_t subs = (int64_t)P.scan.size() / kSubBytes, nsegs = (int64_t)P.rows.size() / kSegCols;
    const int bpm = d[kComponents] == 1 ? 1 : d[kSampling] * d[kSampling] + 2;
    std::vector<uint32_t> words((size_t)(subs + 1) * kRowPitch32, 0);          // the kernels' LDS image, for the whole frame
    for (int64_t g = 0; g < subs * kSubWords; ++g) {
        const uint8_t* b = P.scan.data() + g * 4;
        words[(size_t)(g + g / kSubWords)] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
    }
    std::vector<HuffDev> tables(kHuffPerFrame);
    memcpy(tables.data(), P.huff.data(), P.huff.size());
    coef.assign((size_t)d[kBlocks] * 64, 0);
    LaneOut o;
    o.coef = coef.data(); o.frame_blocks = d[kBlocks]; o.samp = bpm == 6 ? 2 : 1; o.mcus_x = d[kMcusX]; o.bw0 = d[kBw0]; o.bwc = d[kBwC];
    o.n0 = (int64_t)d[kBw0] * d[kBh0]; o.nc = (int64_t)d[kBwC] * d[kBhC];
    int status = 0;
    const int per[3] = {o.samp, 1, 1};
    for (int64_t s = 0; s < nsegs; ++s) {
        const int32_t* row = P.rows.data() + s * kSegCols;
        const int64_t sub0 = row[0] / kSubBytes, sub1 = s + 1 < nsegs ? row[kSegCols] / kSubBytes : subs, n = sub1 - sub0;
        const int qend = (int)(sub0 * kSubBits + row[1]);
        std::vector<uint32_t> x((size_t)n), last((size_t)n, 0u);
        for (int64_t i = 0; i < n; ++i) x[(size_t)i] = lane_decode<false>(words.data(), (int)((sub0 + i) * kSubBits), qend, 0u, tables.data(), bpm, 0, 0, nullptr).word;
        for (int64_t round = 0; round <= n; ++round) {                        // all lanes read, then all lanes write: one round of the kernels
            bool any = false;
            std::vector<uint32_t> next = x;
            for (int64_t i = 1; i < n; ++i) {
                const uint32_t in = x[(size_t)i - 1] & 0xffffu;
                if (in == last[(size_t)i]) continue;
                next[(size_t)i] = lane_decode<false>(words.data(), (int)((sub0 + i) * kSubBits), qend, in, tables.data(), bpm, 0, 0, nullptr).word;
                last[(size_t)i] = in;
                any = true;
            }
            x.swap(next);
            if (!any) break;
        }
        int64_t nstart = 0;
        int remaining = -1;
        o.first_block = (int64_t)row[2] * bpm;
        for (int64_t i = 0; i < n; ++i) {
            const LaneResult r = lane_decode<true>(words.data(), (int)((sub0 + i) * kSubBits), qend, i ? x[(size_t)i - 1] & 0xffffu : 0u, tables.data(), bpm, nstart,
                                                   (int64_t)row[3] * bpm * 64, &o);
            if (r.status > status) status = r.status;
            if (r.remaining >= 0) remaining = r.remaining;
            nstart += x[(size_t)i] >> 16;
        }
        if (remaining < 0) status = status > kStBlocksShort ? status : kStBlocksShort;
        else if (s + 1 < nsegs && remaining >= 8) status = status > kStRestartUnread ? status : kStRestartUnread;
        for (int c = 0; c < d[kComponents]; ++c) {                             // DC: wrapping running sum in MCU order
            uint16_t pred = 0;
            const int64_t first = c == 0 ? 0 : o.n0 + (c - 1) * o.nc, bw = c == 0 ? o.bw0 : o.bwc;
            for (int64_t k = 0; k < (int64_t)row[3] * per[c] * per[c]; ++k) {
                const int64_t m = row[2] + k / (per[c] * per[c]), j = k % (per[c] * per[c]), y = m / o.mcus_x, xx = m % o.mcus_x;
                const int64_t blk = first + (y * per[c] + j / per[c]) * bw + xx * per[c] + j % per[c];
                if (blk < 0 || blk >= o.frame_blocks) continue;
                pred = (uint16_t)(pred + (uint16_t)coef[(size_t)blk * 64]);
                coef[(size_t)blk * 64] = (int16_t)pred;
            }
        }
    }
    return status;
}

int main(int argc, char** argv) {
    int refused = 0, packed = 0, pack_errors = 0, agree_ok = 0, agree_bad = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> file;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + n);
        fclose(f);
        const Packed one = run_pack(file);
        std::vector<Packed> many(8);
        std::vector<std::thread> pool;
        for (int t = 0; t < 8; ++t) pool.emplace_back([&, t] { many[t] = run_pack(file); });
        for (auto& th : pool) th.join();
        for (const Packed& m : many)
            if (!(m == one)) { fprintf(stderr, "%s: threads disagree\n", argv[a]); return 3; }
        if (!one.admitted) { ++refused; continue; }
        // the yardstick: the host decoder on the same bytes
        char text[256] = "";
        Msg msg{text, (int)sizeof(text)};
        std::vector<int16_t> want((size_t)one.desc[kBlocks] * 64, 0);
        uint16_t qt[3 * 64];
        int32_t desc[kDescInts];
        const int host = entropy_decode(file.data(), (int64_t)file.size(), want.data(), (int64_t)want.size(), qt, desc, msg);
        if (one.rc != 0) {
            ++pack_errors;
            if (host == 0) { fprintf(stderr, "%s: pack failed (%d) on a stream the host decoder takes\n", argv[a], one.rc); return 4; }
            continue;
        }
        ++packed;
        if (memcmp(qt, one.qt.data(), sizeof(qt)) || memcmp(desc, one.desc.data(), sizeof(desc))) { fprintf(stderr, "%s: qt / descriptor differ\n", argv[a]); return 5; }
        std::vector<int16_t> got;
        const int status = emulate(one, got);
        if ((status == 0) != (host == 0)) { fprintf(stderr, "%s: status %d, host decoder %d (%s)\n", argv[a], status, host, text); return 6; }
        if (host == 0 && got != want) { fprintf(stderr, "%s: coefficients differ\n", argv[a]); return 7; }
        if (host == 0) ++agree_ok; else ++agree_bad;
    }
    printf("%d streams: %d refused, %d failed to pack (the host decoder rejects them too), %d packed — %d decode to the host decoder's coefficients, "
           "%d are rejected by both; no sanitizer report\n", argc - 1, refused, pack_errors, packed, agree_ok, agree_bad);
    return 0;
}
