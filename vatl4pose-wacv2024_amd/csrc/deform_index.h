// Inverted index behind the ordered (bit-reproducible) dx of the deformable convolution (csrc/deform_dx_ordered.hip): everything that
// is plain arithmetic — the entry and its key, the in-place sort of a list, the layout of the workspace with its sizes and overflow
// guards.  Plain C++ for host and device: the kernels compile it, and so does the stand-alone CPU check
// (tools/deform_index_check.cpp) that runs it under the host sanitizers.
//
//   list     one per (input pixel q = n*H*W + y*W + x, deformable group g): the corners of sampling taps that land on q with a
//            weight w[k] * m != 0.  Image n's lists live in image n's own region of the entry array.
//   entry    {key, wk}: key = (p_local * 9 + t) * 4 + k with p_local the output pixel's row-major index inside its image, t the tap
//            and k the corner; wk = w[k] * m, rounded once.  Keys inside a list are unique.
//   order    ascending key: dx[q][c] = (((+0 + dcol[p0][t0*C + c] * wk0) + dcol[p1][t1*C + c] * wk1) + ...), product and sum each
//            rounded once.
#pragma once
#include "deform_sample.h"

namespace vatl {

struct DeformEntry {
    int key;
    float wk;
};

constexpr long long kDeformIndexLimit = 1LL << 30;      // no count, offset or key of the index reaches 2^30

VATL_HD int deform_key_pack(int p_local, int t, int k) { return (p_local * 9 + t) * 4 + k; }
VATL_HD int deform_key_pixel(int key) { return key / 36; }
VATL_HD int deform_key_tap(int key) { return (key >> 2) % 9; }
VATL_HD int deform_key_corner(int key) { return key & 3; }

// In-place heap sort by key, ascending: O(n log n) for every input, no recursion, no scratch.  Keys are unique inside a list, so the
// result does not depend on the algorithm (or on the order the entries arrived in).
VATL_HD void deform_sift_down(DeformEntry* a, int root, int n) {
    const DeformEntry v = a[root];
    for (;;) {
        int child = 2 * root + 1;
        if (child >= n) break;
        if (child + 1 < n && a[child + 1].key > a[child].key) ++child;
        if (a[child].key <= v.key) break;
        a[root] = a[child];
        root = child;
    }
    a[root] = v;
}

VATL_HD void deform_sort_list(DeformEntry* a, int n) {
    for (int i = n / 2 - 1; i >= 0; --i) deform_sift_down(a, i, n);
    for (int end = n - 1; end > 0; --end) {
        const DeformEntry top = a[0];
        a[0] = a[end];
        a[end] = top;
        deform_sift_down(a, 0, end);
    }
}

// Workspace: [count | start | cursor] (one int per list each, N * H * W * dg lists), padded to 16 bytes, then the entries: image n's at
// entry n * cap, cap = 4 * Ho * Wo * 9 * dg (every corner of every tap of the image's output pixels: the worst case).
struct DeformIndexLayout {
    long long lists_per_image, lists;     // H * W * dg, N * H * W * dg
    long long cap;                        // entries per image
    long long count_off, start_off, cursor_off, entries_off;      // byte offsets
    long long bytes;
};

// 0 = fine; 1 = an argument the kernels do not serve; 2 = a count, an offset or a key would reach 2^30
VATL_HD int deform_index_layout(int N, int H, int W, int stride, int dg, DeformIndexLayout* out) {
    if (N <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2) || (dg != 1 && dg != 2 && dg != 4)) return 1;
    const long long ho = (H - 1) / stride + 1, wo = (W - 1) / stride + 1;
    DeformIndexLayout l;
    l.lists_per_image = (long long)H * W * dg;
    if (l.lists_per_image >= kDeformIndexLimit) return 2;
    l.lists = l.lists_per_image * N;
    l.cap = ho * wo * 36 * dg;                                    // ho * wo <= H * W < 2^30: no overflow in 64 bits
    if (l.lists >= kDeformIndexLimit || l.cap >= kDeformIndexLimit || l.cap * N >= kDeformIndexLimit) return 2;
    l.count_off = 0;
    l.start_off = l.lists * 4;
    l.cursor_off = l.lists * 8;
    l.entries_off = (l.lists * 12 + 15) / 16 * 16;
    l.bytes = l.entries_off + l.cap * N * (long long)sizeof(DeformEntry);
    *out = l;
    return 0;
}

}  // namespace vatl
