// Baseline JPEG Huffman decoding on the device: packed scans of a BATCH of frames (jpeg_pack.h `pack`: stuffing removed, cut
// at the restart markers) -> the int16 coefficient blocks vatl_jpeg_pixels reads, bit for bit those of jpeg_entropy.h's host decoder.
// The frames this project reads carry no restart markers, so the parallelism is not "one thread per restart interval": the scan is cut
// into 128-byte subsequences, one lane each, and the lanes find their true entry states through the self-synchronisation of JPEG's
// Huffman codes (the scheme and what one lane does: jpeg_pack.h; the kernels below are the schedule around `lane_decode`).
//   sync     256 lanes = 256 consecutive subsequences of ONE frame (32 KiB of scan + the frame's six tables in LDS).  Rounds: a lane whose
//            entry state (its left neighbour's exit) changed decodes again; the loop ends on a block-wide "nothing changed" and is bounded by
//            the block's lane count.  Across block boundaries the same step is one LAUNCH per round: a block reads the exit state its left
//            neighbour published in the previous launch (double-buffered: nothing is read that the same launch writes) and returns at once
//            if that is the state it already used.  The host fixes the launch count from the sizes — the most thread blocks any segment
//            spans — so after launch r the first r + 1 blocks of every segment hold true states and the last launch leaves THE decode.
//            No block waits for another one anywhere.
//   offsets  exclusive prefix sum, per segment, of the slots each subsequence consumed: every lane's absolute position.
//   write    each lane decodes its subsequence once more from its true state and stores the non-zero coefficients (2-byte scattered stores,
//            fire and forget: nothing waits on them) — DC as its difference — and reports what decode_block rejects.
//   dc       per segment and component, a wrapping int16 running sum over the DC differences in MCU order; the segment's closing checks.
// Nothing here has been profiled with counters; profiles/jpeg_huffman_notes.md has the phase times.
#include "common.h"
#include "jpeg_pack.h"

namespace vatl {

using namespace jpeg;

// one int64 row per frame (+ a closing row with the totals in kTb0 / kSeg0 / kCoef0): vatl_hip.jpeg_huffman_batch builds it, include/vatl_hip.h documents it
enum { kTb0 = 0, kSubs, kSeg0, kSegs, kCoef0, kHBlocks, kHComps, kHSamp, kHMcusX, kHMcusY, kHBw0, kHBh0, kHBwc, kHBhc, kHuffCols = 16 };
constexpr int kLdsWords = (kSubsPerBlock + 1) * kRowPitch32;
constexpr int kBlockWords = kSubsPerBlock * kSubWords;
constexpr int kActiveSlots = 64;

static_assert(kStBadDc == VATL_JHUFF_BAD_DC && kStBadAc == VATL_JHUFF_BAD_AC && kStZeroRun == VATL_JHUFF_ZERO_RUN && kStEndsEarly == VATL_JHUFF_ENDS_EARLY &&
              kStBlocksShort == VATL_JHUFF_BLOCKS_SHORT && kStRestartUnread == VATL_JHUFF_RESTART_UNREAD && kSegmentTooLong == VATL_JPEG_SEGMENT_TOO_LONG, "vatl_hip.h: status codes");
static_assert(kSubBytes == VATL_JHUFF_SUB_BYTES && kSubsPerBlock == VATL_JHUFF_BLOCK_SUBS && kHuffPerFrame * kHuffDevBytes == VATL_JHUFF_HUFF_BYTES &&
              kHuffCols == VATL_JHUFF_TABLE_COLS && kActiveSlots == VATL_JHUFF_ACTIVE_WORDS, "vatl_hip.h: sizes");

struct JhParams {
    const uint32_t* scan;         // frame f's packed scan starts at dword table[f][kTb0] * kBlockWords
    const int32_t* rows;          // (segments, kSegCols), offsets relative to the frame's scan
    const uint32_t* huff;         // (frames, kHuffPerFrame) HuffDev
    const long long* table;       // (frames + 1, kHuffCols)
    int16_t* coef;
    int32_t* status;
    uint32_t* state;              // per subsequence: (slots << 16) | exit state
    uint32_t* nstart;             // per subsequence: slots consumed in its segment before it
    uint32_t* edge;               // [2][thread blocks]: the exit state of each block's last lane, per launch parity
    uint32_t* used;               // [thread blocks]: the left neighbour's state the block decoded from
    int32_t* seg_rem;             // [segments]: real bits left when the segment's last block ended, -1: it never did
    uint32_t* active;             // [kActiveSlots]: blocks that did work in each sync launch
    long long scan_words, coef_elems, tbs, segments;
    int frames, round;
};

__device__ __forceinline__ int frame_of_col(const long long* table, int frames, int col, long long v) {
    int lo = 0, hi = frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(long long)mid * kHuffCols + col] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// what a lane knows about its subsequence
struct Lane {
    bool live, first;             // inside the frame; the first subsequence of its segment
    long long seg;                // row of the segment (global)
    int qend_seg;                 // LDS bit position where the segment's real bits end
    int bpm;
    long long seg_sub0, seg_subs; // the segment's first subsequence in the frame and how many it has
};

__device__ __forceinline__ Lane find_lane(const JhParams& p, const long long* t, long long tb_in_frame, int lane) {
    Lane L{};
    const long long sub = tb_in_frame * kSubsPerBlock + lane, nsegs = t[kSegs], seg0 = t[kSeg0];
    L.bpm = t[kHComps] == 1 ? 1 : (int)(t[kHSamp] * t[kHSamp]) + 2;
    L.live = sub >= 0 && sub < t[kSubs] && nsegs > 0 && seg0 >= 0 && seg0 + nsegs <= p.segments && (L.bpm == 1 || L.bpm == 3 || L.bpm == 6);
    if (!L.live) return L;
    long long lo = 0, hi = nsegs - 1;                                 // the last row that starts at or before this subsequence
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if ((long long)p.rows[(seg0 + mid) * kSegCols] <= sub * kSubBytes) lo = mid; else hi = mid - 1;
    }
    L.seg = seg0 + lo;
    const int32_t* row = p.rows + L.seg * kSegCols;
    L.seg_sub0 = row[0] / kSubBytes;
    L.seg_subs = (lo + 1 < nsegs ? (long long)row[kSegCols] / kSubBytes : t[kSubs]) - L.seg_sub0;
    L.first = sub == L.seg_sub0;
    long long qe = (L.seg_sub0 - tb_in_frame * kSubsPerBlock) * kSubBits + row[1];
    qe = qe < -(1LL << 30) ? -(1LL << 30) : qe > (1LL << 30) ? (1LL << 30) : qe;
    L.qend_seg = (int)qe;
    if (sub < L.seg_sub0 || row[1] < 0) L.live = false;              // (rows out of order: not ours to decode)
    return L;
}

// the block's 32 KiB of scan as big-endian dwords, kRowPitch32 per subsequence, zero behind the frame's own bytes; and the frame's tables
__device__ __forceinline__ void stage(const JhParams& p, const long long* t, int f, long long tb_in_frame, uint32_t* words, uint32_t* tabs) {
    const long long frame_words = t[kSubs] * kSubWords, base = t[kTb0] * kBlockWords;
    for (int g = threadIdx.x; g < kBlockWords + kSubWords; g += kSubsPerBlock) {
        const long long idx = tb_in_frame * kBlockWords + g;
        uint32_t v = 0;
        if (idx >= 0 && idx < frame_words && base >= 0 && base + idx < p.scan_words) v = __builtin_bswap32(p.scan[base + idx]);
        words[g + g / kSubWords] = v;
    }
    const uint32_t* src = p.huff + (long long)f * (kHuffPerFrame * kHuffDevBytes / 4);
    for (int g = threadIdx.x; g < kHuffPerFrame * kHuffDevBytes / 4; g += kSubsPerBlock) tabs[g] = src[g];
}

__global__ __launch_bounds__(kSubsPerBlock) void jh_sync_kernel(JhParams p) {
    __shared__ uint32_t words[kLdsWords];
    __shared__ uint32_t tabs[kHuffPerFrame * kHuffDevBytes / 4];
    __shared__ uint32_t xs[kSubsPerBlock];
    const long long tb = blockIdx.x;
    const int lane = threadIdx.x, par = p.round & 1;
    const int f = frame_of_col(p.table, p.frames, kTb0, tb);
    const long long* t = p.table + (long long)f * kHuffCols;
    const long long tb_in_frame = tb - t[kTb0];
    // the left neighbour's exit state: the guess in the first launch, what it published in the previous one afterwards
    const uint32_t edge_in = (tb_in_frame == 0 || p.round == 0) ? 0u : p.edge[(long long)(par ^ 1) * p.tbs + tb - 1];
    if (p.round > 0 && edge_in == p.used[tb]) {                      // nothing new: this block's states stand (uniform over the block)
        if (lane == 0) p.edge[(long long)par * p.tbs + tb] = p.edge[(long long)(par ^ 1) * p.tbs + tb];
        return;
    }
    stage(p, t, f, tb_in_frame, words, tabs);
    const Lane L = find_lane(p, t, tb_in_frame, lane);
    const HuffDev* tables = reinterpret_cast<const HuffDev*>(tabs);
    const long long g = tb * kSubsPerBlock + lane;
    __syncthreads();
    uint32_t last_in, out = kStateInvalid;
    if (p.round == 0) {
        last_in = 0;
        if (L.live) out = lane_decode<false>(words, lane * kSubBits, L.qend_seg, 0u, tables, L.bpm, 0, 0, nullptr).word;
    } else {
        out = p.state[g];
        last_in = L.first ? 0u : lane > 0 ? (p.state[g - 1] & 0xffffu) : p.used[tb];
    }
    xs[lane] = out;
    __syncthreads();
    for (int r = 0; r <= kSubsPerBlock; ++r) {                       // after round r the block's first r lanes are final: at most kSubsPerBlock rounds change anything
        const uint32_t in = L.first ? 0u : lane > 0 ? (xs[lane - 1] & 0xffffu) : edge_in;
        const bool again = L.live && in != last_in;
        if (again) {
            out = lane_decode<false>(words, lane * kSubBits, L.qend_seg, in, tables, L.bpm, 0, 0, nullptr).word;
            last_in = in;
        }
        __syncthreads();                                             // every lane has read its neighbour
        if (again) xs[lane] = out;
        if (!__syncthreads_or(again)) break;
    }
    p.state[g] = xs[lane];
    if (lane == 0) {
        p.edge[(long long)par * p.tbs + tb] = xs[kSubsPerBlock - 1] & 0xffffu;
        p.used[tb] = edge_in;
        atomicAdd(&p.active[min(p.round, kActiveSlots - 1)], 1u);
    }
}

// inclusive sum over the block's 256 values (sh: 256 words); every thread also gets the total
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < kSubsPerBlock; off <<= 1) {
        const uint32_t add = tid >= off ? sh[tid - off] : 0u;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const uint32_t r = sh[tid];
    total = sh[kSubsPerBlock - 1];
    __syncthreads();
    return r;
}

// one block per segment: nstart of its subsequences.  The sum saturates (a stream that claims more slots than 2^32 is damaged; the write
// pass stops at the segment's own slot count anyway).
__global__ __launch_bounds__(kSubsPerBlock) void jh_offsets_kernel(JhParams p) {
    __shared__ uint32_t sh[kSubsPerBlock];
    const long long seg = blockIdx.x;
    const int f = frame_of_col(p.table, p.frames, kSeg0, seg);
    const long long* t = p.table + (long long)f * kHuffCols;
    const long long local = seg - t[kSeg0];
    if (local < 0 || local >= t[kSegs] || t[kSeg0] + t[kSegs] > p.segments) return;
    const int32_t* row = p.rows + seg * kSegCols;
    const long long sub0 = row[0] / kSubBytes, sub1 = local + 1 < t[kSegs] ? (long long)row[kSegCols] / kSubBytes : t[kSubs];
    const long long first = t[kTb0] * kSubsPerBlock + sub0, subs = sub1 - sub0;
    if (sub0 < 0 || subs <= 0 || sub1 > t[kSubs] || first + subs > p.tbs * kSubsPerBlock) return;
    unsigned long long carry = 0;
    for (long long i0 = 0; i0 < subs; i0 += kSubsPerBlock) {         // ceil(subs / 256) trips
        const long long i = i0 + threadIdx.x;
        const uint32_t n = i < subs ? p.state[first + i] >> 16 : 0u;
        uint32_t total;
        const uint32_t incl = block_scan(n, sh, total);
        const unsigned long long at = carry + incl - n;
        if (i < subs) p.nstart[first + i] = at > 0xffffffffull ? 0xffffffffu : (uint32_t)at;
        carry += total;
    }
}

__global__ __launch_bounds__(kSubsPerBlock) void jh_write_kernel(JhParams p) {
    __shared__ uint32_t words[kLdsWords];
    __shared__ uint32_t tabs[kHuffPerFrame * kHuffDevBytes / 4];
    const long long tb = blockIdx.x;
    const int lane = threadIdx.x;
    const int f = frame_of_col(p.table, p.frames, kTb0, tb);
    const long long* t = p.table + (long long)f * kHuffCols;
    const long long tb_in_frame = tb - t[kTb0];
    stage(p, t, f, tb_in_frame, words, tabs);
    const Lane L = find_lane(p, t, tb_in_frame, lane);
    __syncthreads();
    if (!L.live) return;
    const long long g = tb * kSubsPerBlock + lane;
    const uint32_t entry = L.first ? 0u : (p.state[g - 1] & 0xffffu);            // (not first: g - 1 is a subsequence of the same frame)
    const int32_t* row = p.rows + L.seg * kSegCols;
    LaneOut o;
    const long long c0 = t[kCoef0], fb = t[kHBlocks];
    if (c0 < 0 || fb <= 0 || (c0 + fb) * 64 > p.coef_elems || row[2] < 0 || row[3] < 0) return;    // the frame's coefficients must lie inside the buffer the caller states
    o.coef = p.coef + c0 * 64;
    o.frame_blocks = fb;
    o.first_block = (long long)row[2] * L.bpm;
    o.samp = L.bpm == 6 ? 2 : 1;
    o.mcus_x = max((int)t[kHMcusX], 1);
    o.bw0 = (int)t[kHBw0]; o.bwc = (int)t[kHBwc];
    o.n0 = t[kHBw0] * t[kHBh0]; o.nc = t[kHBwc] * t[kHBhc];
    const LaneResult r = lane_decode<true>(words, lane * kSubBits, L.qend_seg, entry, reinterpret_cast<const HuffDev*>(tabs), L.bpm, (long long)p.nstart[g],
                                           (long long)row[3] * L.bpm * 64, &o);
    if (r.status) atomicMax(&p.status[f], r.status);
    if (r.remaining >= 0) p.seg_rem[L.seg] = r.remaining;            // one lane per segment gets here: the one in which its slot count is reached
}

// grid: 3 blocks per segment, one per component.  A block walks the component's blocks of the segment in MCU order, 256 at a time.
__global__ __launch_bounds__(kSubsPerBlock) void jh_dc_kernel(JhParams p) {
    __shared__ uint32_t sh[kSubsPerBlock];
    const long long seg = blockIdx.x / 3;
    const int comp = blockIdx.x % 3;
    const int f = frame_of_col(p.table, p.frames, kSeg0, seg);
    const long long* t = p.table + (long long)f * kHuffCols;
    const long long local = seg - t[kSeg0];
    if (local < 0 || local >= t[kSegs] || t[kSeg0] + t[kSegs] > p.segments) return;
    const int32_t* row = p.rows + seg * kSegCols;
    if (comp == 0 && threadIdx.x == 0) {                             // the host decoder's checks between segments, from the final states
        const int rem = p.seg_rem[seg];
        if (rem < 0) atomicMax(&p.status[f], (int)kStBlocksShort);
        else if (local + 1 < t[kSegs] && rem >= 8) atomicMax(&p.status[f], (int)kStRestartUnread);
    }
    const int comps = (int)t[kHComps], samp = comps == 1 ? 1 : (int)t[kHSamp];
    if (comp >= comps || (samp != 1 && samp != 2) || row[2] < 0 || row[3] < 0) return;
    const long long c0 = t[kCoef0], fb = t[kHBlocks];
    if (c0 < 0 || fb <= 0 || (c0 + fb) * 64 > p.coef_elems) return;
    int16_t* coef = p.coef + c0 * 64;
    const int per = comp == 0 ? samp : 1, per2 = per * per;
    const long long mx = max(t[kHMcusX], 1LL), bw = comp == 0 ? t[kHBw0] : t[kHBwc];
    const long long comp_first = comp == 0 ? 0 : t[kHBw0] * t[kHBh0] + (comp - 1) * t[kHBwc] * t[kHBhc];
    const long long count = (long long)row[3] * per2;
    uint32_t carry = 0;
    for (long long k0 = 0; k0 < count; k0 += kSubsPerBlock) {        // ceil(count / 256) trips
        const long long k = k0 + threadIdx.x, m = row[2] + k / per2;
        const int j = (int)(k % per2), v = j / per, h = j % per;
        const long long y = m / mx, x = m - y * mx;
        const long long blk = comp_first + (y * per + v) * bw + (x * per + h);
        const bool ok = k < count && blk >= 0 && blk < fb;
        uint32_t total;
        const uint32_t incl = block_scan(ok ? (uint32_t)(uint16_t)coef[blk * 64] : 0u, sh, total);
        if (ok) coef[blk * 64] = (int16_t)(uint16_t)(carry + incl);  // modulo 2^16: the host's pred = (int16_t)pred
        carry += total;
    }
}

}  // namespace vatl

using namespace vatl;

static jpeg::Msg pack_error_msg() { return jpeg::Msg{err_buf(), 512}; }

extern "C" int vatl_jpeg_pack_size(const uint8_t* data, int64_t nbytes, int64_t* scan_capacity, int64_t* segment_rows) {
    return jpeg::pack_size(data, nbytes, scan_capacity, segment_rows, pack_error_msg());
}

extern "C" int vatl_jpeg_pack(const uint8_t* data, int64_t nbytes, uint8_t* scan, int64_t scan_capacity, int32_t* segments, int64_t segment_capacity,
                              uint8_t* huff, uint16_t* qt, int32_t* desc, int64_t* used) {
    return jpeg::pack(data, nbytes, scan, scan_capacity, segments, segment_capacity, huff, qt, desc, used, pack_error_msg());
}

// dwords: state + nstart per subsequence, edge[2] + used per thread block, seg_rem per segment, the launch activity counters
static int64_t workspace_words(int64_t tbs, int64_t segments) { return 2 * tbs * kSubsPerBlock + 3 * tbs + segments + kActiveSlots; }

extern "C" int64_t vatl_jpeg_huffman_workspace_bytes(int64_t thread_blocks, int64_t segments) {
    if (thread_blocks <= 0 || segments <= 0 || thread_blocks > (1LL << 22) || segments > (1LL << 28)) return 0;
    return 4 * workspace_words(thread_blocks, segments);
}

extern "C" int vatl_jpeg_huffman(const uint8_t* scan, const int32_t* segments, const uint8_t* huff, const int64_t* table, int frames, int64_t thread_blocks,
                                 int64_t segment_rows, int launches, int16_t* coef, int64_t coef_elems, int32_t* status, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
    if (frames == 0) return 0;
    if (!scan || !segments || !huff || !table || !coef || !status || !workspace) return fail(VATL_EINVAL, "vatl_jpeg_huffman: null pointer");
    const int64_t need = vatl_jpeg_huffman_workspace_bytes(thread_blocks, segment_rows);
    if (frames < 0 || need == 0 || workspace_bytes < need || coef_elems <= 0 || launches < 1 || launches > thread_blocks || 3 * segment_rows >= (1LL << 31))
        return fail(VATL_EINVAL, "vatl_jpeg_huffman: frames=%d thread_blocks=%lld segments=%lld launches=%d coef_elems=%lld workspace=%lld (needs %lld)", frames,
                    (long long)thread_blocks, (long long)segment_rows, launches, (long long)coef_elems, (long long)workspace_bytes, (long long)need);
    if (((uintptr_t)scan & 3) || ((uintptr_t)huff & 3) || ((uintptr_t)workspace & 3) || ((uintptr_t)coef & 1))
        return fail(VATL_EINVAL, "vatl_jpeg_huffman: scan / huff / workspace must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* w = (uint32_t*)workspace;
    JhParams p{};
    p.scan = (const uint32_t*)scan; p.rows = segments; p.huff = (const uint32_t*)huff; p.table = (const long long*)table;
    p.coef = coef; p.status = status;
    p.state = w; p.nstart = p.state + thread_blocks * kSubsPerBlock; p.edge = p.nstart + thread_blocks * kSubsPerBlock; p.used = p.edge + 2 * thread_blocks;
    p.seg_rem = (int32_t*)(p.used + thread_blocks); p.active = (uint32_t*)(p.seg_rem + segment_rows);
    p.scan_words = thread_blocks * kBlockWords; p.coef_elems = coef_elems; p.tbs = thread_blocks; p.segments = segment_rows; p.frames = frames;
    if (hipMemsetAsync(coef, 0, (size_t)coef_elems * sizeof(int16_t), s) != hipSuccess || hipMemsetAsync(status, 0, (size_t)frames * sizeof(int32_t), s) != hipSuccess ||
        hipMemsetAsync(p.edge, 0, (size_t)(3 * thread_blocks) * 4, s) != hipSuccess || hipMemsetAsync(p.seg_rem, 0xff, (size_t)segment_rows * 4, s) != hipSuccess ||
        hipMemsetAsync(p.active, 0, kActiveSlots * 4, s) != hipSuccess)
        return fail(VATL_ELAUNCH, "vatl_jpeg_huffman: hipMemsetAsync failed");
    for (int r = 0; r < launches; ++r) {
        p.round = r;
        hipLaunchKernelGGL(jh_sync_kernel, dim3((unsigned)thread_blocks), dim3(kSubsPerBlock), 0, s, p);
    }
    hipLaunchKernelGGL(jh_offsets_kernel, dim3((unsigned)segment_rows), dim3(kSubsPerBlock), 0, s, p);
    hipLaunchKernelGGL(jh_write_kernel, dim3((unsigned)thread_blocks), dim3(kSubsPerBlock), 0, s, p);
    hipLaunchKernelGGL(jh_dc_kernel, dim3((unsigned)(3 * segment_rows)), dim3(kSubsPerBlock), 0, s, p);
    return check_launch("vatl_jpeg_huffman");
}
