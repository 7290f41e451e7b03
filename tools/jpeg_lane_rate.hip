// The single-lane decode rate behind csrc/jpeg_pack.h's kMaxSegmentBytes (profiles/jpeg_huffman_notes.md) — a measurement, not part of the library:
//
//   python tools/jpeg_decode_bench.py --dump-noise-frame /tmp/noise_q100.jpg        # the 256x256 quality-100 noise frame of tests/test_gpu_jpeg_huffman.py
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Ivatl4pose-wacv2024_amd/csrc tools/jpeg_lane_rate.hip -o /tmp/jpeg_lane_rate
//   /tmp/jpeg_lane_rate /tmp/noise_q100.jpg
//
// The worst case of csrc/jpeg_huffman.hip is a segment in which nothing synchronises: one lane at a time decodes, subsequence after
// subsequence, once to find the states (lane_decode<false>) and once to write (lane_decode<true>).  This program packs the file's
// one segment with `pack`, stages a thread block's scan and the tables in LDS as the kernels do, and lets lane 0 alone do exactly that
// — first the write pass by itself (entry states and slot offsets from a host decode), then the state pass — and prints both rates
// and the rate of the two together, which is the one the cap is sized by.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_pack.h"

using namespace vatl::jpeg;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

constexpr int kLdsWords = (kSubsPerBlock + 1) * kRowPitch32;

// mode 0: the write pass (entry[i], nstart[i] given); mode 1: the state pass (every subsequence from its predecessor's exit)
__global__ __launch_bounds__(kSubsPerBlock) void walk(const uint32_t* scan_be, const uint32_t* huff, const uint32_t* entry, const uint32_t* nstart, int64_t subs,
                                                     long long qend_total, int bpm, int64_t seg_slots, LaneOut o, int mode, int* result) {
    __shared__ uint32_t words[kLdsWords];
    __shared__ uint32_t tabs[kHuffPerFrame * kHuffDevBytes / 4];
    for (int g = threadIdx.x; g < kHuffPerFrame * kHuffDevBytes / 4; g += kSubsPerBlock) tabs[g] = huff[g];
    const HuffDev* tables = reinterpret_cast<const HuffDev*>(tabs);
    uint32_t state = 0;
    int status = 0, remaining = -1;
    for (int64_t tb = 0; tb * kSubsPerBlock < subs; ++tb) {
        __syncthreads();
        for (int g = threadIdx.x; g < kSubsPerBlock * kSubWords + kSubWords; g += kSubsPerBlock) {
            const int64_t idx = tb * kSubsPerBlock * kSubWords + g;
            words[g + g / kSubWords] = idx < subs * kSubWords ? scan_be[idx] : 0u;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const long long qe = qend_total - tb * (long long)kSubsPerBlock * kSubBits;
            const int qend = (int)(qe > (1LL << 30) ? (1LL << 30) : qe);
            for (int i = 0; i < kSubsPerBlock && tb * kSubsPerBlock + i < subs; ++i) {
                const int64_t g = tb * kSubsPerBlock + i;
                if (mode == 0) {
                    const LaneResult r = lane_decode<true>(words, i * kSubBits, qend, entry[g], tables, bpm, nstart[g], seg_slots, &o);
                    if (r.status > status) status = r.status;
                    if (r.remaining >= 0) remaining = r.remaining;
                } else
                    state = lane_decode<false>(words, i * kSubBits, qend, state, tables, bpm, 0, 0, nullptr).word & 0xffffu;
            }
        }
    }
    if (threadIdx.x == 0) { result[0] = status; result[1] = mode == 0 ? remaining : (int)state; }
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: jpeg_lane_rate FILE.jpg\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> file;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + n);
    fclose(f);
    char text[256] = "";
    Msg msg{text, (int)sizeof(text)};
    int64_t cap = 0, nrows = 0, used[2] = {0, 0};
    if (pack_size(file.data(), (int64_t)file.size(), &cap, &nrows, msg)) { printf("refused: %s\n", text); return 2; }
    std::vector<uint8_t> scan((size_t)cap), huff((size_t)kHuffPerFrame * kHuffDevBytes);
    std::vector<int32_t> rows((size_t)nrows * kSegCols);
    uint16_t qt[3 * 64];
    int32_t desc[kDescInts];
    if (pack(file.data(), (int64_t)file.size(), scan.data(), cap, rows.data(), nrows, huff.data(), qt, desc, used, msg)) { printf("pack: %s\n", text); return 2; }
    if (used[1] != 1) { printf("a stream without restart markers is expected (one segment)\n"); return 2; }
    const int64_t subs = used[0] / kSubBytes, blocks = desc[kBlocks];
    const int bpm = desc[kComponents] == 1 ? 1 : desc[kSampling] * desc[kSampling] + 2;
    std::vector<uint32_t> be((size_t)subs * kSubWords), image((size_t)(subs + 1) * kRowPitch32, 0);
    for (int64_t g = 0; g < subs * kSubWords; ++g) {
        const uint8_t* b = scan.data() + g * 4;
        be[(size_t)g] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
        image[(size_t)(g + g / kSubWords)] = be[(size_t)g];
    }
    // the true chain on the host: every subsequence's entry state and slot offset
    std::vector<HuffDev> tables(kHuffPerFrame);
    memcpy(tables.data(), huff.data(), huff.size());
    std::vector<uint32_t> entry((size_t)subs), nstart((size_t)subs);
    uint32_t state = 0, slots = 0;
    for (int64_t i = 0; i < subs; ++i) {
        entry[(size_t)i] = state; nstart[(size_t)i] = slots;
        const uint32_t w = lane_decode<false>(image.data(), (int)(i * kSubBits), rows[1], state, tables.data(), bpm, 0, 0, nullptr).word;
        state = w & 0xffffu; slots += w >> 16;
    }
    uint32_t *dscan, *dhuff, *dentry, *dnstart;
    int16_t* dcoef;
    int* dres;
    CK(hipMalloc(&dscan, be.size() * 4)); CK(hipMalloc(&dhuff, huff.size())); CK(hipMalloc(&dentry, entry.size() * 4)); CK(hipMalloc(&dnstart, nstart.size() * 4));
    CK(hipMalloc(&dcoef, (size_t)blocks * 128)); CK(hipMalloc(&dres, 8));
    CK(hipMemcpy(dscan, be.data(), be.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dhuff, huff.data(), huff.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(dentry, entry.data(), entry.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dnstart, nstart.data(), nstart.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dcoef, 0, (size_t)blocks * 128));
    LaneOut o;
    o.coef = dcoef; o.frame_blocks = blocks; o.first_block = 0; o.samp = bpm == 6 ? 2 : 1; o.mcus_x = desc[kMcusX]; o.bw0 = desc[kBw0]; o.bwc = desc[kBwC];
    o.n0 = (int64_t)desc[kBw0] * desc[kBh0]; o.nc = (int64_t)desc[kBwC] * desc[kBhC];
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    const double bytes = rows[1] / 8.0;
    double ms[2] = {0, 0};
    for (int rep = 0; rep < 3; ++rep)                                 // the first repeat is the warm-up
        for (int mode = 0; mode < 2; ++mode) {
            CK(hipEventRecord(a));
            hipLaunchKernelGGL(walk, dim3(1), dim3(kSubsPerBlock), 0, 0, dscan, dhuff, dentry, dnstart, subs, (long long)rows[1], bpm, (int64_t)rows[3] * bpm * 64, o, mode, dres);
            CK(hipEventRecord(b)); CK(hipEventSynchronize(b)); CK(hipGetLastError());
            float t = 0;
            CK(hipEventElapsedTime(&t, a, b));
            int res[2];
            CK(hipMemcpy(res, dres, 8, hipMemcpyDeviceToHost));
            if (mode == 0 && (res[0] != 0 || res[1] < 0)) { printf("write pass: status %d, segment end %d\n", res[0], res[1]); return 3; }
            if (mode == 1 && (uint32_t)res[1] != state) { printf("state pass: exit state %d, host %u\n", res[1], state); return 3; }
            if (rep) printf("repeat %d  %s: %.0f scan bytes in %.3f ms = %.3f MB/s\n", rep, mode == 0 ? "write pass, one lane" : "state pass, one lane", bytes, t, bytes / (t * 1e3));
            if (rep == 2) ms[mode] = t;
        }
    printf("both passes, one lane: %.3f MB/s; a segment of %lld bytes (kMaxSegmentBytes) takes %.2f s\n", bytes / ((ms[0] + ms[1]) * 1e3), (long long)kMaxSegmentBytes,
           kMaxSegmentBytes / (bytes / ((ms[0] + ms[1]) * 1e-3)));
    return 0;
}
