// Hybrid JPEG decoder — the data-parallel half on the device (crop-producer row):
//   alphapose/datasets/coco_video.py `_read_rgb` (Pillow -> libjpeg-turbo; the reference: posetrack21.py:141 cv2.imread)
// The host keeps marker parsing and Huffman decoding (jpeg_entropy.h); a BATCH of frames' coefficient blocks then becomes packed RGB
// in the frame arena that vatl_crop_warp_affine reads, in two launches for the whole batch:
//   A  dequantise + 8x8 inverse DCT of every block of every component of every frame -> uint8 component planes padded to whole blocks
//   B  chroma upsampling + YCbCr -> RGB + store at each frame's byte offset in the arena
// The arithmetic is libjpeg-turbo's JDCT_ISLOW (jidctint.c), h2v2 "fancy" upsampling (jdsample.c) and ycc_rgb_convert (jdcolor.c) —
// what Pillow runs by default — restated in 32-bit integers, so the bytes are those of the host path bit for bit (tests/golden/jpeg.npz).
// The two launches together take 8 us per 1280x720 frame against 1.4 ms of Huffman decoding on the host (profiles/jpeg_decode_notes.md; no
// counters were taken, so what bounds each kernel is not known): they are not where the hybrid path's time goes and are written for
// exactness and for bounds safety first — a frame look-up and a 64-bit division per pixel group, chroma re-read per pixel through a
// clamped index, every index derived from the frame table checked against the buffer sizes the caller states.
#include "common.h"
#include "jpeg_entropy.h"

namespace vatl {

// one row per frame (+ a closing row that holds the totals in kBlock0 / kGroup0); int64 columns — vatl_hip.jpeg_decode_batch builds it (JPEG_TABLE_COLS columns), include/vatl_hip.h documents it
enum { kBlock0 = 0, kGroup0, kArenaOff, kFh, kFw, kFcomp, kFsamp, kFbw0, kFbh0, kFbwc, kFbhc, kTableCols = 12 };

struct JpegParams {
    const int16_t* coef;          // 64 per block, frames back to back
    const uint16_t* qt;           // (frames, 3, 64) natural order
    const long long* table;       // (frames + 1, kTableCols)
    uint8_t* planes;              // 64 bytes per block: same offsets as coef
    uint8_t* arena;
    long long blocks, groups, arena_bytes;
    int frames;
};

// the frame whose [table[f][col], table[f+1][col]) holds v (v < the closing row's value)
__device__ __forceinline__ int frame_of(const long long* table, int frames, int col, long long v) {
    int lo = 0, hi = frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(long long)mid * kTableCols + col] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// jidctint.c jpeg_idct_islow: one 1-D pass over eight (dequantised) inputs
__device__ __forceinline__ void idct8(const int i[8], int o[8], int shift) {
    int z1 = (i[2] + i[6]) * 4433;
    const int t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
    const int t0 = (i[0] + i[4]) << 13, t1 = (i[0] - i[4]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const int r = 1 << (shift - 1);
    o[0] = (t10 + a3 + r) >> shift; o[7] = (t10 - a3 + r) >> shift;
    o[1] = (t11 + a2 + r) >> shift; o[6] = (t11 - a2 + r) >> shift;
    o[2] = (t12 + a1 + r) >> shift; o[5] = (t12 - a1 + r) >> shift;
    o[3] = (t13 + a0 + r) >> shift; o[4] = (t13 - a0 + r) >> shift;
}

constexpr int kIdctBlocks = 32;      // 8x8 blocks per workgroup: eight lanes each
constexpr int kRowPitch = 9;         // LDS row pitch in ints: the column pass (lanes along a row) and the row pass (lanes down a column) both hit 8 distinct banks

// Stage A.  Lane l of a block's eight loads coefficient row l (16 bytes: the eight lanes read the block's 128 contiguous bytes), multiplies by the
// quantiser row and parks it in LDS; then it is column l of pass 1 and row l of pass 2, and stores its row of eight samples as one 8-byte word.
__global__ __launch_bounds__(kIdctBlocks * 8) void jpeg_idct_kernel(JpegParams p) {
    __shared__ int ws[kIdctBlocks][8 * kRowPitch];
    const int slot = threadIdx.x >> 3, l = threadIdx.x & 7;
    const long long g = (long long)blockIdx.x * kIdctBlocks + slot;
    const bool live = g < p.blocks;
    int f = 0, comp = 0, bw = 1;
    long long local = 0, comp_first = 0;
    if (live) {
        f = frame_of(p.table, p.frames, kBlock0, g);
        const long long* t = p.table + (long long)f * kTableCols;
        local = g - t[kBlock0];
        const long long n0 = t[kFbw0] * t[kFbh0], nc = t[kFbwc] * t[kFbhc];
        bw = (int)t[kFbw0];
        if (local >= n0) {                                           // a chroma block (local < n0 + 2 nc by the table's own sums; comp is clamped all the same)
            comp = nc > 0 && local - n0 >= nc ? 2 : 1;
            comp_first = n0 + (comp - 1) * nc;
            bw = (int)t[kFbwc];
        }
        int v[8];
        const int4 raw = *reinterpret_cast<const int4*>(p.coef + g * 64 + l * 8);
        const int4 q = *reinterpret_cast<const int4*>(p.qt + ((long long)f * 3 + comp) * 64 + l * 8);
        const int rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = (int)(short)(rw[k] & 0xffff) * (qw[k] & 0xffff);
            v[2 * k + 1] = (rw[k] >> 16) * (int)((unsigned)qw[k] >> 16);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[slot][l * kRowPitch + k] = v[k];
    }
    __syncthreads();
    if (live) {                                                      // pass 1: down column l
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = ws[slot][k * kRowPitch + l];
        idct8(in, out, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[slot][k * kRowPitch + l] = out[k];      // (only this lane touches column l: no barrier between its reads and writes)
    }
    __syncthreads();
    if (live) {                                                      // pass 2: along row l
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = ws[slot][l * kRowPitch + k];
        idct8(in, out, 18);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (unsigned)min(max(out[k] + 128, 0), 255) << (8 * k);
            hi |= (unsigned)min(max(out[k + 4] + 128, 0), 255) << (8 * k);
        }
        const long long within = local - comp_first;
        bw = max(bw, 1);
        const long long by = within / bw, bx = within - by * bw;
        // the component's plane is (8 bh, 8 bw) row-major right behind the planes before it: block-relative byte < 64 * blocks of the frame
        const long long at = (p.table[(long long)f * kTableCols + kBlock0] + comp_first) * 64 + (by * 8 + l) * (8LL * bw) + bx * 8;
        if (at >= 0 && at + 8 <= p.blocks * 64) *reinterpret_cast<uint2*>(p.planes + at) = make_uint2(lo, hi);
    }
}

struct FrameView {
    const uint8_t* planes;        // all frames' planes; y / cb / cr are byte offsets into it, every read is clamped to [0, limit]
    long long y, cb, cr, limit;
    int h, w, samp, comps, pitch0, pitchc, dw, dh;
    __device__ __forceinline__ int at(long long i) const { return planes[min(max(i, 0LL), limit)]; }
};

// h2v2 fancy upsampling of one chroma sample (jdsample.c h2v2_fancy_upsample): 3/4 near + 1/4 far row, then 3/4 + 1/4 along the row
__device__ __forceinline__ int chroma420(const FrameView& v, long long c, int yy, int xx) {
    const int r = yy >> 1, x = xx >> 1;
    const int rf = (yy & 1) ? min(r + 1, v.dh - 1) : max(r - 1, 0);
    const long long near = c + (long long)r * v.pitchc + x, far = c + (long long)rf * v.pitchc + x;
    const int s = 3 * v.at(near) + v.at(far);
    if (xx & 1) {
        if (x == v.dw - 1) return (4 * s + 7) >> 4;
        return (3 * s + 3 * v.at(near + 1) + v.at(far + 1) + 7) >> 4;
    }
    if (x == 0) return (4 * s + 8) >> 4;
    return (3 * s + 3 * v.at(near - 1) + v.at(far - 1) + 8) >> 4;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

// pixel q (row-major over the (h, w) frame) -> its three bytes, R lowest (jdcolor.c ycc_rgb_convert)
__device__ __forceinline__ unsigned pixel_rgb(const FrameView& v, long long q) {
    const int yy = (int)(q / v.w), xx = (int)(q - (long long)yy * v.w);
    const int y = v.at(v.y + (long long)yy * v.pitch0 + xx);
    if (v.comps == 1) return (unsigned)y * 0x010101u;
    int cb, cr;
    if (v.samp == 2) {
        cb = chroma420(v, v.cb, yy, xx);
        cr = chroma420(v, v.cr, yy, xx);
    } else {
        cb = v.at(v.cb + (long long)yy * v.pitchc + xx);
        cr = v.at(v.cr + (long long)yy * v.pitchc + xx);
    }
    cb -= 128; cr -= 128;
    const unsigned r = clamp255(y + ((91881 * cr + 32768) >> 16));
    const unsigned g = clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    const unsigned b = clamp255(y + ((116130 * cb + 32768) >> 16));
    return r | (g << 8) | (b << 16);
}

// Stage B.  A frame starts at any byte of the arena (offsets are sums of h*w*3), so the unit of work is not four pixels but the
// 12 bytes of three ALIGNED dwords: group k of a frame covers arena bytes [base + 12 k, base + 12 k + 12), base = the frame's offset
// rounded down to a dword.  Those bytes belong to five consecutive pixels at the most (four when the offset is aligned); a group
// that lies wholly inside the frame is three dword stores, the frame's first and last group store the bytes that are the frame's one
// by one (the neighbouring frame's last / first group writes the other bytes of those dwords).
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(JpegParams p) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= p.groups) return;
    const int f = frame_of(p.table, p.frames, kGroup0, g);
    const long long* t = p.table + (long long)f * kTableCols;
    const long long k = g - t[kGroup0], off = t[kArenaOff];
    FrameView v;
    v.planes = p.planes; v.limit = p.blocks * 64 - 1;
    v.h = (int)t[kFh]; v.w = max((int)t[kFw], 1); v.comps = (int)t[kFcomp]; v.samp = (int)t[kFsamp];
    v.pitch0 = (int)t[kFbw0] * 8; v.pitchc = (int)t[kFbwc] * 8;
    v.dw = (v.w + 1) >> 1; v.dh = (v.h + 1) >> 1;
    v.y = t[kBlock0] * 64;
    v.cb = v.y + t[kFbw0] * t[kFbh0] * 64;
    v.cr = v.cb + t[kFbwc] * t[kFbhc] * 64;
    const long long npix = (long long)v.h * v.w, nbytes = 3 * npix;
    const int mis = (int)(off & 3);
    const long long j0 = 12 * k - mis;                               // frame byte of the group's first arena byte (-3 .. -1 in the first group when mis != 0)
    const long long q0 = j0 >= 0 ? j0 / 3 : -1;                      // first pixel the group touches
    const int lead = (int)(j0 - 3 * q0);                             // 0 .. 2: bytes of pixel q0 that lie before the group
    unsigned px[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const long long q = q0 + i;
        px[i] = (q >= 0 && q < npix && (i < 4 || lead)) ? pixel_rgb(v, q) : 0u;
    }
    // the 15 bytes as one little-endian number, shifted down by `lead` bytes -> the group's three dwords
    const unsigned w4[4] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8), px[4]};
    unsigned wd[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) wd[d] = (unsigned)((((unsigned long long)w4[d + 1] << 32) | w4[d]) >> (8 * lead));
    const long long a0 = (off - mis) + 12 * k;                       // arena byte of the group: a multiple of 4
    if (a0 < 0 || a0 >= p.arena_bytes) return;
    uint8_t* dst = p.arena + a0;
    if (j0 >= 0 && j0 + 12 <= nbytes && a0 + 12 <= p.arena_bytes) {
        unsigned* d32 = reinterpret_cast<unsigned*>(dst);
        d32[0] = wd[0]; d32[1] = wd[1]; d32[2] = wd[2];
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const long long j = j0 + i;
            if (j >= 0 && j < nbytes && a0 + i < p.arena_bytes) dst[i] = (uint8_t)(wd[i >> 2] >> (8 * (i & 3)));
        }
    }
}

}  // namespace vatl

using namespace vatl;

static jpeg::Msg last_error_msg() { return jpeg::Msg{err_buf(), 512}; }

// the public header's numbers are jpeg_entropy.h's
static_assert(jpeg::kDescInts == VATL_JPEG_DESC_INTS && jpeg::kErrArg == VATL_EINVAL && jpeg::kErrStream == VATL_ESTREAM, "vatl_hip.h: descriptor / error codes");
static_assert(jpeg::kNotJpeg == VATL_JPEG_NOT_JPEG && jpeg::kBadHeader == VATL_JPEG_BAD_HEADER && jpeg::kNotBaseline == VATL_JPEG_NOT_BASELINE &&
              jpeg::kPrecision == VATL_JPEG_PRECISION && jpeg::kComponentCount == VATL_JPEG_COMPONENTS && jpeg::kSamplingFactors == VATL_JPEG_SAMPLING &&
              jpeg::kTooSmall == VATL_JPEG_TOO_SMALL && jpeg::kMultipleScans == VATL_JPEG_MULTIPLE_SCANS && jpeg::kColourSpace == VATL_JPEG_COLOUR_SPACE &&
              jpeg::kQuantPrecision == VATL_JPEG_QUANT_PRECISION && jpeg::kTooLarge == VATL_JPEG_TOO_LARGE, "vatl_hip.h: refusal codes");

extern "C" int vatl_jpeg_probe(const uint8_t* data, int64_t nbytes, int32_t* desc) {
    if (!data || !desc || nbytes < 0) return fail(VATL_EINVAL, "vatl_jpeg_probe: null pointer");
    jpeg::Header H;
    jpeg::parse_header(data, nbytes, H, last_error_msg());
    for (int i = 0; i < jpeg::kDescInts; ++i) desc[i] = H.desc[i];
    return 0;
}

extern "C" int vatl_jpeg_entropy_decode(const uint8_t* data, int64_t nbytes, int16_t* coef, int64_t coef_capacity, uint16_t* qt, int32_t* desc) {
    return jpeg::entropy_decode(data, nbytes, coef, coef_capacity, qt, desc, last_error_msg());
}

extern "C" int vatl_jpeg_pixels(const int16_t* coef, const uint16_t* qt, const int64_t* table, int frames, int64_t blocks, int64_t groups,
                                uint8_t* planes, uint8_t* arena, int64_t arena_bytes, void* stream) {
    if (frames == 0) return 0;
    if (!coef || !qt || !table || !planes || !arena) return fail(VATL_EINVAL, "vatl_jpeg_pixels: null pointer");
    if (frames < 0 || blocks <= 0 || groups <= 0 || arena_bytes <= 0 || blocks > (1LL << 31) || groups > (1LL << 38))           // (grids of < 2^31 workgroups)
        return fail(VATL_EINVAL, "vatl_jpeg_pixels: frames=%d blocks=%lld groups=%lld arena_bytes=%lld", frames, (long long)blocks, (long long)groups, (long long)arena_bytes);
    if (((uintptr_t)coef & 15) || ((uintptr_t)qt & 15) || ((uintptr_t)planes & 7) || ((uintptr_t)arena & 3))
        return fail(VATL_EINVAL, "vatl_jpeg_pixels: coef / qt must be 16-byte, planes 8-byte, arena 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    JpegParams p{coef, qt, (const long long*)table, planes, arena, blocks, groups, arena_bytes, frames};
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)cdiv(blocks, kIdctBlocks)), dim3(kIdctBlocks * 8), 0, s, p);
    hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((unsigned)cdiv(groups, 256)), dim3(256), 0, s, p);
    return check_launch("vatl_jpeg_pixels");
}
