// Ordered dx of the deformable convolution's backward: the same per-term arithmetic as deform_columns_bwd_kernel's float atomics
// (deform_conv.hip), summed in ONE fixed order, so that its bits do not change from run to run.  The contribution rows exist already —
// dcol[p][t * C + c] — so what is built here is the inverted index (deform_index.h) and the pass that sums through it:
//   deform_index_walk_kernel<false>   count: per (output pixel, tap, group) the corners with w[k] * m != 0 — the test of the atomic
//                                     kernel — are counted into their list (integer atomics);
//   deform_index_scan_kernel          exclusive scan of the counts, one block per image (an image's lists live in its own region);
//   deform_index_walk_kernel<true>    fill: the same walk stores {key, wk} through integer cursors;
//   deform_index_sort_kernel          every list sorted in place by key, by its owner thread (keys are unique: the order in which the
//                                     cursors handed out the slots leaves no trace);
//   deform_dx_sum_kernel              dx[q][c] = ((+0 + dcol * wk) + dcol * wk) + ... in ascending key order, product and sum each
//                                     rounded once; every element of dx gets one plain store.
// Separate launches on the caller's stream: no flag, ticket or wait between blocks.  Every loop bound comes from the count array,
// which this call zeroes and writes, and every workspace byte that is read was written by this call first.  The sampling rules are
// deform_sample.h's, through deform_tap.  d_offset / d_mask come from deform_columns_bwd_kernel<false>: the code of the atomic entry.
#include "deform_tap.h"   // first: the HIP runtime, which deform_sample.h's host / device macro needs
#include "deform_index.h"

namespace vatl {

struct DeformIndex {
    int* count; int* start; int* cursor;     // one int per list (q * dg + g)
    DeformEntry* entries;                    // image n's lists: entries + n * cap, list l at start[l], count[l] entries
    long long cap;
};

// one thread per (output pixel, tap, deformable group); count and fill see the same corners with the same wk
template <bool kFill>
__global__ void deform_index_walk_kernel(DeformGeom q, DeformIndex ix) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= q.P * 9 * q.dg) return;
    const int g = (int)(e % q.dg);
    const int t = (int)((e / q.dg) % 9);
    const long long p = e / (9 * q.dg);
    const DeformTap d = deform_tap(q, p, t, g);
    if (!d.s.valid) return;
    const long long per_image = (long long)q.Ho * q.Wo;
    const long long n = p / per_image;
    const int p_local = (int)(p - n * per_image);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float wk = d.s.w[k] * d.m;
        if (wk != 0.f) {
            const long long list = (d.base + d.s.idx[k]) * q.dg + g;
            if (!kFill) {
                atomicAdd(ix.count + list, 1);
            } else {
                const int at = atomicAdd(ix.cursor + list, 1);
                if (at >= 0 && at < ix.cap) ix.entries[n * ix.cap + at] = DeformEntry{deform_key_pack(p_local, t, k), wk};
            }
        }
    }
}

// block b scans the `per_image` counts of image b: thread i sums the run [i * run, (i + 1) * run), the block scans the 1024 sums in
// LDS, the thread then writes its run's exclusive prefixes into start and cursor
constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kScanThreads) void deform_index_scan_kernel(DeformIndex ix, int per_image) {
    __shared__ int sums[kScanThreads];
    const long long first = (long long)blockIdx.x * per_image;
    const int run = (per_image + kScanThreads - 1) / kScanThreads;
    const int lo = min(per_image, (int)threadIdx.x * run), hi = min(per_image, lo + run);
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += ix.count[first + i];
    sums[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {
        const int add = (int)threadIdx.x >= o ? sums[threadIdx.x - o] : 0;
        __syncthreads();
        sums[threadIdx.x] += add;
        __syncthreads();
    }
    int at = sums[threadIdx.x] - mine;
    for (int i = lo; i < hi; ++i) {
        ix.start[first + i] = at;
        ix.cursor[first + i] = at;
        at += ix.count[first + i];
    }
}

__global__ void deform_index_sort_kernel(DeformIndex ix, long long lists, int per_image) {
    const long long l = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (l >= lists) return;
    deform_sort_list(ix.entries + (l / per_image) * ix.cap + ix.start[l], ix.count[l]);
}

// one thread per (input pixel, 4-channel run): the lanes of a deformable group read the same entries (a broadcast) and 16 contiguous
// bytes each of the dcol row the entry names
__global__ void deform_dx_sum_kernel(const float* __restrict__ dcol, int col_stride, DeformGeom q, DeformIndex ix, float* __restrict__ dx) {
#pragma clang fp contract(off)   // acc + (v * wk): two roundings per term, as v * wk into a float atomic has
    const int C4 = q.C >> 2;
    const long long pixels = (long long)q.N * q.H * q.W;
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= pixels * C4) return;
    const long long pix = i / C4;
    const int cc = (int)(i - pix * C4) * 4;
    const long long n = pix / ((long long)q.H * q.W);
    const long long list = pix * q.dg + cc / q.Cg;
    const DeformEntry* e = ix.entries + n * ix.cap + ix.start[list];
    const int len = ix.count[list];
    const float* rows = dcol + n * q.Ho * q.Wo * col_stride + cc;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < len; ++j) {
        const DeformEntry en = e[j];
        const f32x4 v = *reinterpret_cast<const f32x4*>(rows + (long long)deform_key_pixel(en.key) * col_stride + deform_key_tap(en.key) * q.C);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float term = v[c] * en.wk;
            acc[c] = acc[c] + term;
        }
    }
    *reinterpret_cast<f32x4*>(dx + pix * q.C + cc) = acc;
}

}  // namespace vatl

using namespace vatl;

extern "C" int64_t vatl_deform_dx_index_bytes(int N, int H, int W, int stride, int deform_groups) {
    DeformIndexLayout l;
    const int rc = deform_index_layout(N, H, W, stride, deform_groups, &l);
    if (rc == 1) return fail(VATL_EINVAL, "deform_dx_index_bytes: N %d, H %d, W %d, stride %d (1, 2), %d deformable groups (1, 2, 4) not served", N, H, W, stride, deform_groups);
    if (rc) return fail(VATL_EINVAL, "deform_dx_index_bytes: the index exceeds 2^30 entries; split the batch");
    return l.bytes;
}

extern "C" int vatl_deform_columns_bwd_ordered(const float* dcol, int col_stride, const float* x, const float* offset, int offset_stride,
                                               const float* mask_or_null, int mask_stride, int mask_is_logits, float* dx, float* d_offset,
                                               int d_offset_stride, float* d_mask_or_null, int d_mask_stride, int N, int H, int W, int C,
                                               int stride, int deform_groups, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "deform_columns_bwd_ordered";
    DeformGeom q{};
    if (int rc = deform_bwd_check(who, q, dcol, col_stride, x, offset, offset_stride, mask_or_null, mask_stride, mask_is_logits, dx, d_offset, d_offset_stride,
                                  d_mask_or_null, d_mask_stride, N, H, W, C, stride, deform_groups))
        return rc;
    DeformIndexLayout l;
    if (deform_index_layout(N, H, W, stride, deform_groups, &l)) return fail(VATL_EINVAL, "%s: the index exceeds 2^30 entries; split the batch", who);
    if (!workspace || ((uintptr_t)workspace & 15)) return fail(VATL_EINVAL, "%s: workspace null or not 16-byte aligned", who);
    if (workspace_bytes < l.bytes)
        return fail(VATL_EINVAL, "%s: workspace of %lld bytes, vatl_deform_dx_index_bytes asks for %lld", who, (long long)workspace_bytes, l.bytes);
    char* ws = static_cast<char*>(workspace);
    DeformIndex ix{reinterpret_cast<int*>(ws + l.count_off), reinterpret_cast<int*>(ws + l.start_off), reinterpret_cast<int*>(ws + l.cursor_off),
                   reinterpret_cast<DeformEntry*>(ws + l.entries_off), l.cap};
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ix.count, 0, (size_t)l.lists * sizeof(int), st) != hipSuccess) return fail(VATL_ELAUNCH, "%s: memset failed", who);
    const dim3 walk((unsigned)((q.P * 9 * q.dg + 255) / 256));
    hipLaunchKernelGGL(deform_index_walk_kernel<false>, walk, dim3(256), 0, st, q, ix);
    hipLaunchKernelGGL(deform_index_scan_kernel, dim3((unsigned)N), dim3(kScanThreads), 0, st, ix, (int)l.lists_per_image);
    hipLaunchKernelGGL(deform_index_walk_kernel<true>, walk, dim3(256), 0, st, q, ix);
    hipLaunchKernelGGL(deform_index_sort_kernel, dim3((unsigned)((l.lists + 255) / 256)), dim3(256), 0, st, ix, l.lists, (int)l.lists_per_image);
    const long long runs = (long long)N * H * W * (C / 4);
    hipLaunchKernelGGL(deform_dx_sum_kernel, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, st, dcol, col_stride, q, ix, dx);
    deform_bwd_launch(false, dcol, col_stride, x, q, dx, d_offset, d_offset_stride, d_mask_or_null, d_mask_stride, st);
    return check_launch(who);
}
