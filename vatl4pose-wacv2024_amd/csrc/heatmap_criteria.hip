// Heat-map criteria beside HP, each reading the (N,J,H,W) fp32 heat-maps once:
//   THC           compute_thc + neighbour rule     active_learning/ActiveLearning.py:345-363, 747-760
//   TPC           compute_tpc + neighbour rule     ActiveLearning.py:333-344, 736-745
//   MPE / Margin  compute_mpe / compute_margin     ActiveLearning.py:762-788  (skimage.feature.peak_local_max(min_distance=5,
//                                                  num_peaks=5) + scipy softmax / entropy)
//   Entropy       compute_entropy                  ActiveLearning.py:790-796  (scipy.stats.entropy of the flattened map)
#include "scorer_common.h"

namespace vatl {

// --------------------------------------------------------------------------
// THC: one block per pair of heat-map stacks (J*H*W floats each)
// --------------------------------------------------------------------------
template <int NORM>
__global__ __launch_bounds__(256) void thc_pairs_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        long long sa, long long sb, float* __restrict__ out, int J, int n) {
    const float* pa = a + (long long)blockIdx.x * sa;
    const float* pb = b + (long long)blockIdx.x * sb;
    const int tid = threadIdx.x;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    const int n4 = n >> 2;
    for (int q = tid; q < n4; q += 256) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(pa + 4 * q);
        const f32x4 y = *reinterpret_cast<const f32x4*>(pb + 4 * q);
        const float d0 = x[0] - y[0], d1 = x[1] - y[1], d2 = x[2] - y[2], d3 = x[3] - y[3];
        if (NORM == 1) { acc0 += fabsf(d0); acc1 += fabsf(d1); acc2 += fabsf(d2); acc3 += fabsf(d3); }
        else           { acc0 += d0 * d0;   acc1 += d1 * d1;   acc2 += d2 * d2;   acc3 += d3 * d3; }
    }
    for (int q = 4 * n4 + tid; q < n; q += 256) {
        const float d = pa[q] - pb[q];
        acc0 += NORM == 1 ? fabsf(d) : d * d;
    }
    __shared__ double part[4];
    block4_put(part, wave_sum((double)acc0 + (double)acc1 + (double)acc2 + (double)acc3));
    __syncthreads();
    if (tid == 0) out[blockIdx.x] = (float)(block4_sum(part) / (double)J);
}

__global__ void thc_combine_kernel(const float* __restrict__ pair, const uint8_t* __restrict__ is_prev,
                                   const uint8_t* __restrict__ is_next, float* __restrict__ thc, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const bool hp = is_prev[i] != 0 && i > 0, hn = is_next[i] != 0 && i < N - 1;
    float t = 0.f;
    if (hp) t += pair[i - 1];
    if (hn) t += pair[i];
    if (hp != hn) t *= 2.f;                                     // exactly one neighbour: doubled
    thc[i] = t;
}

// --------------------------------------------------------------------------
// TPC: one thread per item.  adj_prev[i] / adj_next[i] are the neighbours' heat-maps
// decoded with item i's box (vatl_decode_argmax_affine on shifted views).
// --------------------------------------------------------------------------
__device__ __forceinline__ int moved_joints(const float* a, const float* b, int J, double thresh) {
    int c = 0;
    for (int j = 0; j < J; ++j) {
        const float dx = a[2 * j] - b[2 * j], dy = a[2 * j + 1] - b[2 * j + 1];
        const float d = sqrtf(dx * dx + dy * dy);             // np.linalg.norm on float32 rows
        c += ((double)d > thresh) ? 1 : 0;
    }
    return c;
}

__global__ void tpc_stream_kernel(const float* __restrict__ cur, const float* __restrict__ adj_prev, const float* __restrict__ adj_next,
                                  const float* __restrict__ bbox, const uint8_t* __restrict__ is_prev, const uint8_t* __restrict__ is_next,
                                  float* __restrict__ tpc, int N, int J) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double w = (double)bbox[4 * i + 2] - (double)bbox[4 * i + 0], h = (double)bbox[4 * i + 3] - (double)bbox[4 * i + 1];
    const double thresh = 0.01 * sqrt(w * h);
    const bool hp = is_prev[i] != 0 && i > 0, hn = is_next[i] != 0 && i < N - 1;
    int t = 0;
    if (hp) t += moved_joints(cur + (long long)i * J * 2, adj_prev + (long long)i * J * 2, J, thresh);
    if (hn) t += moved_joints(cur + (long long)i * J * 2, adj_next + (long long)i * J * 2, J, thresh);
    if (hp != hn) t *= 2;
    tpc[i] = (float)t;
}

// --------------------------------------------------------------------------
// peaks5 with MPE and Margin: one block (or one wave) per plane
// --------------------------------------------------------------------------
// arg-max of per-thread (value, index) pairs over the block, to every thread; sval / sidx are free again on return
__device__ __forceinline__ void block_argmax_reduce(float& bv, int& bi, float* sval, int* sidx) {
    wave_argmax<false>(bv, bi);
    block4_put(sval, bv); block4_put(sidx, bi);
    __syncthreads();
    block4_argmax<false>(sval, sidx, bv, bi);
    __syncthreads();
}

// Block-wide arg-max over (value desc, index asc); -inf entries never win.  Returns the flat index or -1.
__device__ __forceinline__ int block_argmax(const float* v, int n, float* sval, int* sidx, float& best_val) {
    float bv = -INFINITY; int bi = 0x7FFFFFFF;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float x = v[i];
        if (x > bv) { bv = x; bi = i; }                        // strided scan keeps the lowest index among equals per thread
    }
    block_argmax_reduce(bv, bi, sval, sidx);
    best_val = bv;
    return bv == -INFINITY ? -1 : bi;
}

// a plane's peaks and its MPE and Margin terms (one thread)
__device__ __forceinline__ void store_peaks5(float* peak_val, int32_t* peak_idx, int32_t* npeaks,
                                             float* mpe, float* margin, long long plane, const float* pv, const int* pi, int n) {
    npeaks[plane] = n;
    for (int k = 0; k < 5; ++k) { peak_val[plane * 5 + k] = k < n ? pv[k] : 0.f; peak_idx[plane * 5 + k] = k < n ? pi[k] : -1; }
    float e = 0.f;
    if (n > 0) {                                            // entropy(softmax(peaks)), float32 like scipy on a float32 array
        float ex[5], s = 0.f;
        for (int k = 0; k < n; ++k) { ex[k] = expf(pv[k] - pv[0]); s += ex[k]; }
        float q[5], qs = 0.f;
        for (int k = 0; k < n; ++k) { q[k] = ex[k] / s; qs += q[k]; }
        for (int k = 0; k < n; ++k) { const float p = q[k] / qs; e += p > 0.f ? -p * logf(p) : 0.f; }
    }
    mpe[plane] = e;
    margin[plane] = n > 1 ? fabsf(pv[0] - pv[1]) : 0.f;
}

// peak_local_max(plane, min_distance = D, num_peaks = 5): (2D+1)^2 maximum filter with replicated edges, strictly
// above the plane minimum, D-wide border excluded, greedy spacing (Chebyshev distance < D rejected) in descending
// intensity / ascending index order, first five kept.  Also the per-plane MPE and Margin terms.  The plane lives in LDS.
__global__ __launch_bounds__(256) void peaks5_kernel(const float* __restrict__ hm, float* __restrict__ peak_val, int32_t* __restrict__ peak_idx,
                                                     int32_t* __restrict__ npeaks, float* __restrict__ mpe, float* __restrict__ margin,
                                                     int H, int W, int D) {
    extern __shared__ float sm[];
    float* img = sm;                 // plane, later the candidate values (-inf = not a candidate)
    float* tmp = sm + H * W;         // row-filtered plane
    __shared__ float sval[4]; __shared__ int sidx[4];
    const int HW = H * W;
    const float* src = hm + (long long)blockIdx.x * HW;
    float mn = INFINITY;
    for (int i = threadIdx.x; i < HW; i += 256) { const float v = src[i]; img[i] = v; mn = fminf(mn, v); }
    block4_put(sval, -wave_max(-mn));
    __syncthreads();
    mn = fminf(fminf(sval[0], sval[1]), fminf(sval[2], sval[3]));
    __syncthreads();
    // separable (2D+1)^2 maximum filter with replicated edges (= maximum over the in-range part of the window).
    // Row pass: each thread produces 4 consecutive outputs from one sliding window (4 + 2D reads instead of 4 (2D+1)).
    const float inv_w = 1.0f / (float)W;
    const int W4 = (W + 3) >> 2;
    const float inv_w4 = 1.0f / (float)W4;
    for (int q = threadIdx.x; q < H * W4; q += 256) {
        const int y = fast_div(q, inv_w4), x = 4 * (q - y * W4);
        const float* row = img + y * W;
        float core = -INFINITY;                                   // columns x+3-D .. x+D are common to all four windows
        for (int xx = max(x + 3 - D, 0); xx <= min(x + D, W - 1); ++xx) core = fmaxf(core, row[xx]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (x + e >= W) break;
            float m = core;
            for (int xx = max(x + e - D, 0); xx < max(x + 3 - D, 0); ++xx) m = fmaxf(m, row[xx]);          // left extras
            for (int xx = min(x + D, W - 1) + 1; xx <= min(x + e + D, W - 1); ++xx) m = fmaxf(m, row[xx]);   // right extras
            tmp[y * W + x + e] = m;
        }
    }
    __syncthreads();
    // Column pass, same sliding scheme over 4 consecutive rows of one column
    const int H4 = (H + 3) >> 2;
    for (int q = threadIdx.x; q < H4 * W; q += 256) {
        const int yb = fast_div(q, inv_w), x = q - yb * W;
        const int y = 4 * yb;
        float core = -INFINITY;
        for (int yy = max(y + 3 - D, 0); yy <= min(y + D, H - 1); ++yy) core = fmaxf(core, tmp[yy * W + x]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int yo = y + e;
            if (yo >= H) break;
            float m = core;
            for (int yy = max(yo - D, 0); yy < max(y + 3 - D, 0); ++yy) m = fmaxf(m, tmp[yy * W + x]);
            for (int yy = min(y + D, H - 1) + 1; yy <= min(yo + D, H - 1); ++yy) m = fmaxf(m, tmp[yy * W + x]);
            const float v = img[yo * W + x];
            const bool inside = yo >= D && yo < H - D && x >= D && x < W - D;
            img[yo * W + x] = (inside && v == m && v > mn) ? v : -INFINITY;     // each thread rewrites only what it alone reads
        }
    }
    __syncthreads();
    // Candidates are few (a handful per plane): compact them into a list and let the greedy selection run over the
    // list; a plateau-ridden plane with more than CAP candidates falls back to arg-max passes over the whole plane.
    constexpr int CAP = 256;
    __shared__ float cval[CAP]; __shared__ int cidx[CAP]; __shared__ int ccount;
    if (threadIdx.x == 0) ccount = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < HW; i += 256) {
        const float v = img[i];
        if (v != -INFINITY) { const int slot = atomicAdd(&ccount, 1); if (slot < CAP) { cval[slot] = v; cidx[slot] = i; } }
    }
    __syncthreads();
    const int nc = ccount;
    float pv[5]; int pi[5]; int n = 0;
    if (nc <= CAP) {
        for (int k = 0; k < 5; ++k) {                            // ordered by (value desc, flat index asc): slot order is irrelevant
            float bv = -INFINITY; int bi = 0x7FFFFFFF;
            for (int t = threadIdx.x; t < nc; t += 256) argmax_merge<false>(bv, bi, cval[t], cidx[t]);
            block_argmax_reduce(bv, bi, sval, sidx);
            if (bv == -INFINITY) break;
            pv[n] = bv; pi[n] = bi; ++n;
            const int by = bi / W, bx = bi - by * W;
            for (int t = threadIdx.x; t < nc; t += 256) {        // reject everything at Chebyshev distance < D (itself included)
                const int yy = fast_div(cidx[t], inv_w), xx = cidx[t] - yy * W;
                if (abs(yy - by) < D && abs(xx - bx) < D) cval[t] = -INFINITY;
            }
            __syncthreads();
        }
    } else {
        for (int k = 0; k < 5; ++k) {
            float bv;
            const int bi = block_argmax(img, HW, sval, sidx, bv);
            if (bi < 0) break;
            pv[n] = bv; pi[n] = bi; ++n;
            const int by = bi / W, bx = bi - by * W;
            const int side = 2 * D - 1;
            for (int t = threadIdx.x; t < side * side; t += 256) {
                const int yy = by - (D - 1) + t / side, xx = bx - (D - 1) + t % side;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) img[yy * W + xx] = -INFINITY;
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) store_peaks5(peak_val, peak_idx, npeaks, mpe, margin, (long long)blockIdx.x, pv, pi, n);
}

// The same function for the shipped heat-map size (64 x 48) and min_distance (5: ActiveLearning.py:773,784) with ONE WAVE per
// plane and no block barriers: lane = row, the row's 48 values live in registers.  The 11 x 11 maximum filter is two in-register
// passes of the doubling scheme (windows of 2, 4, 8, then 8 + 4 overlapping = 11: 4 max operations per pixel and pass instead of
// 10), the COLUMN pass on a transposed copy of the plane — written row-wise to a wave-private LDS tile (pitch W + 4 floats:
// conflict-free both ways), read column-wise (lane = column), filtered, written back and read row-wise again.  Same window maxima
// as the block kernel (max is associative; fmaxf treats a NaN as missing in any order), same candidates, same greedy selection.
// The block kernel spends its time in 17 barriers and an LDS compaction per plane.
template <int W>
__global__ __launch_bounds__(256) void peaks5_wave_kernel(const float* __restrict__ hm, float* __restrict__ peak_val, int32_t* __restrict__ peak_idx,
                                                          int32_t* __restrict__ npeaks, float* __restrict__ mpe, float* __restrict__ margin,
                                                          long long planes) {
    constexpr int D = 5, H = 64;
    static_assert(W % 4 == 0 && W > 2 * D && W <= 64, "row of W floats per lane");
    constexpr int P = W + 4;
    extern __shared__ __attribute__((aligned(16))) float tile_all[];
    const int lane = threadIdx.x & 63;
    float* tile = tile_all + (threadIdx.x >> 6) * (H * P);
    const long long plane = wave_plane();
    if (plane >= planes) return;
    const float* src = hm + plane * (H * W) + lane * W;
    float v[W];
#pragma unroll
    for (int k = 0; k < W / 4; ++k) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(src + 4 * k);
        v[4 * k] = t[0]; v[4 * k + 1] = t[1]; v[4 * k + 2] = t[2]; v[4 * k + 3] = t[3];
        *reinterpret_cast<f32x4*>(tile + lane * P + 4 * k) = t;
    }
    float mn = v[0];
#pragma unroll
    for (int x = 1; x < W; ++x) mn = fminf(mn, v[x]);
    mn = -wave_max(-mn);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // column pass (lane = column x < W): c[y] = max over rows y - 5 .. y + 5 inside the plane
    if (lane < W) {
        float c[H];
#pragma unroll
        for (int y = 0; y < H; ++y) c[y] = tile[y * P + lane];
        float a2[H], a4[H], a8[H];                         // maxima of the windows [y, y + 2), [y, y + 4), [y, y + 8) clipped at the last row
#pragma unroll
        for (int y = 0; y < H; ++y) a2[y] = y + 1 < H ? fmaxf(c[y], c[y + 1]) : c[y];
#pragma unroll
        for (int y = 0; y < H; ++y) a4[y] = y + 2 < H ? fmaxf(a2[y], a2[y + 2]) : a2[y];
#pragma unroll
        for (int y = 0; y < H; ++y) a8[y] = y + 4 < H ? fmaxf(a4[y], a4[y + 4]) : a4[y];
#pragma unroll
        for (int y = 0; y < H; ++y) {
            // rows y - 5 .. y + 5 = [s, s + 8) U [y + 2, y + 6) with s = y - 5; at the top the window starts at row 0 and is shorter
            float m;
            if (y >= D) m = y + 2 < H ? fmaxf(a8[y - D], a4[y + 2]) : a8[y - D];
            else if (y + D + 1 >= 8) m = fmaxf(a8[0], a4[y + 2]);                  // [0, 8) U [y + 2, y + 6)   (y = 2 .. 4)
            else m = fmaxf(a4[0], a4[y + 2]);                                       // [0, 4) U [y + 2, y + 6)   (y = 0, 1: windows of 6 / 7 rows)
            tile[y * P + lane] = m;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // row pass (lane = row y) on the column maxima
    float h[W];
#pragma unroll
    for (int k = 0; k < W / 4; ++k) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(tile + lane * P + 4 * k);
        h[4 * k] = t[0]; h[4 * k + 1] = t[1]; h[4 * k + 2] = t[2]; h[4 * k + 3] = t[3];
    }
    float cand[W];
    {
        float b2[W], b4[W], b8[W];
#pragma unroll
        for (int x = 0; x < W; ++x) b2[x] = x + 1 < W ? fmaxf(h[x], h[x + 1]) : h[x];
#pragma unroll
        for (int x = 0; x < W; ++x) b4[x] = x + 2 < W ? fmaxf(b2[x], b2[x + 2]) : b2[x];
#pragma unroll
        for (int x = 0; x < W; ++x) b8[x] = x + 4 < W ? fmaxf(b4[x], b4[x + 4]) : b4[x];
        const bool row_in = lane >= D && lane < H - D;
#pragma unroll
        for (int x = D; x < W - D; ++x) {                  // candidates exist inside the border only: there the window is never clipped on the left
            const float m = fmaxf(b8[x - D], b4[x + 2]);
            cand[x] = (row_in && v[x] == m && v[x] > mn) ? v[x] : -INFINITY;
        }
#pragma unroll
        for (int x = 0; x < D; ++x) { cand[x] = -INFINITY; cand[W - 1 - x] = -INFINITY; }
    }
    float pv[5]; int pi[5]; int n = 0;
    // Greedy selection.  A plane has few candidates (maxima of 11 x 11 windows: typically 10 - 25): they are compacted into a list of at most
    // 64 — one per lane, in LDS where the tile was — and the five rounds run on ONE value per lane (wave arg-max + one distance test) instead
    // of re-scanning 48 registers per lane and round.  Planes with more than 64 candidates (plateaus of equal values) take the register scan
    // below.  Same order either way: value descending, flat index ascending.
    int mine = 0;
#pragma unroll
    for (int x = D; x < W - D; ++x) mine += cand[x] > -INFINITY ? 1 : 0;
    int incl = mine;                                       // inclusive prefix sum over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    const int total = __shfl(incl, 63, 64);
    if (total <= 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                   // every lane has read its row of the tile
        int pos = incl - mine;
#pragma unroll
        for (int x = D; x < W - D; ++x)
            if (cand[x] > -INFINITY) { tile[pos] = cand[x]; reinterpret_cast<int*>(tile)[64 + pos] = lane * W + x; ++pos; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float cv = lane < total ? tile[lane] : -INFINITY;
        const int ci = lane < total ? reinterpret_cast<const int*>(tile)[64 + lane] : 0x7FFFFFFF;
        const int cy = ci / W, cx = ci - cy * W;
#pragma unroll 1
        for (int k = 0; k < 5; ++k) {
            float bv = cv; int bi = cv > -INFINITY ? ci : 0x7FFFFFFF;
            wave_argmax<false>(bv, bi);
            if (bv == -INFINITY) break;
            pv[n] = bv; pi[n] = bi; ++n;
            const int by = bi / W, bx = bi - by * W;
            if (abs(cy - by) < D && abs(cx - bx) < D) cv = -INFINITY;
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < 5; ++k) {
            float bv = -INFINITY; int bi = 0x7FFFFFFF;
#pragma unroll
            for (int x = 0; x < W; ++x)
                if (cand[x] > bv) { bv = cand[x]; bi = lane * W + x; }          // ascending x: the first maximum of the row
            wave_argmax<false>(bv, bi);
            if (bv == -INFINITY) break;
            pv[n] = bv; pi[n] = bi; ++n;
            const int by = bi / W, bx = bi - by * W;
            if (abs(lane - by) < D) {
#pragma unroll
                for (int x = 0; x < W; ++x)
                    if (abs(x - bx) < D) cand[x] = -INFINITY;
            }
        }
    }
    if (lane == 0) store_peaks5(peak_val, peak_idx, npeaks, mpe, margin, plane, pv, pi, n);
}

// --------------------------------------------------------------------------
// Entropy: scipy.stats.entropy(plane.flatten()): p = h / sum(h), then the sum of entr(p); a zero sum gives nan like numpy's 0/0 and x/0
// --------------------------------------------------------------------------
// scipy.special.entr: -p ln p (p > 0), 0 (p == 0), -inf (p < 0), nan (nan)
__device__ __forceinline__ float entr(float p) {
    if (p > 0.f) return -p * logf(p);
    if (p == 0.f) return 0.f;
    if (p < 0.f) return -INFINITY;
    return p;
}

__global__ __launch_bounds__(256) void plane_entropy_kernel(const float* __restrict__ hm, float* __restrict__ out, int HW) {
    const float* gsrc = hm + (long long)blockIdx.x * HW;
    extern __shared__ __attribute__((aligned(16))) float plane[];   // read from HBM once; each thread re-reads only what it wrote
    __shared__ double sh[4];
    double s = 0.0;
    if ((HW & 3) == 0) {                               // 16-byte loads
        for (int i = threadIdx.x; i < (HW >> 2); i += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(gsrc + 4 * i);
            *reinterpret_cast<f32x4*>(plane + 4 * i) = v;
            s += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
        }
    } else {
        for (int i = threadIdx.x; i < HW; i += 256) { const float v = gsrc[i]; plane[i] = v; s += (double)v; }
    }
    const float* src = plane;
    const int step = (HW & 3) == 0 ? 4 : 1;            // pass 2 walks the elements this thread staged
    block4_put(sh, wave_sum(s));
    __syncthreads();
    const float total = (float)block4_sum(sh);
    __syncthreads();
    double e = 0.0;
    for (int i0 = threadIdx.x * step; i0 < HW; i0 += 256 * step)
        for (int i = i0; i < i0 + step; ++i) e += (double)entr(src[i] / total);
    block4_put(sh, wave_sum(e));
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (float)block4_sum(sh);
}

// one wave per plane (scorer_common.h): same arithmetic
template <int NV>
__global__ __launch_bounds__(256) void plane_entropy_wave_kernel(const float* __restrict__ hm, float* __restrict__ out, int planes) {
    const int lane = threadIdx.x & 63;
    const long long plane = wave_plane();
    if (plane >= planes) return;
    f32x4 v[NV];
    load_plane<NV>(hm + plane * (64LL * NV * 4), lane, v);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) s += ((double)v[k][0] + (double)v[k][1]) + ((double)v[k][2] + (double)v[k][3]);
    const float total = (float)wave_sum(s);
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) e += (double)entr(v[k][c] / total);
    e = wave_sum(e);
    if (lane == 0) out[plane] = (float)e;
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_thc_pairs(const float* a, const float* b, int64_t stride_a, int64_t stride_b, float* out,
                              int P, int J, int HW, int norm, void* stream) {
    if (norm != 1 && norm != 2) return fail(VATL_EINVAL, "thc_pairs: norm must be 1 (L1) or 2 (L2)");
    if (P <= 0) return 0;
    if (!a || !b || !out) return fail(VATL_EINVAL, "thc_pairs: null pointer");
    if (((uintptr_t)a | (uintptr_t)b) & 15 || (stride_a & 3) || (stride_b & 3))
        return fail(VATL_EINVAL, "thc_pairs: operands must be 16-byte aligned");
    if (norm == 1) hipLaunchKernelGGL(thc_pairs_kernel<1>, dim3(P), dim3(256), 0, (hipStream_t)stream, a, b, (long long)stride_a, (long long)stride_b, out, J, J * HW);
    else           hipLaunchKernelGGL(thc_pairs_kernel<2>, dim3(P), dim3(256), 0, (hipStream_t)stream, a, b, (long long)stride_a, (long long)stride_b, out, J, J * HW);
    return check_launch("thc_pairs");
}

extern "C" int vatl_thc_combine(const float* pair, const uint8_t* is_prev, const uint8_t* is_next, float* thc, int N, void* stream) {
    if (N <= 0) return 0;
    if (!is_prev || !is_next || !thc || (N > 1 && !pair)) return fail(VATL_EINVAL, "thc_combine: null pointer");
    hipLaunchKernelGGL(thc_combine_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, pair, is_prev, is_next, thc, N);
    return check_launch("thc_combine");
}

extern "C" int vatl_tpc_stream(const float* cur, const float* adj_prev, const float* adj_next, const float* bbox,
                               const uint8_t* is_prev, const uint8_t* is_next, float* tpc, int N, int J, void* stream) {
    if (N <= 0) return 0;
    if (!cur || !bbox || !is_prev || !is_next || !tpc || (N > 1 && (!adj_prev || !adj_next))) return fail(VATL_EINVAL, "tpc_stream: null pointer");
    hipLaunchKernelGGL(tpc_stream_kernel, dim3(cdiv(N, 128)), dim3(128), 0, (hipStream_t)stream, cur, adj_prev, adj_next, bbox, is_prev, is_next, tpc, N, J);
    return check_launch("tpc_stream");
}

extern "C" int vatl_peaks5(const float* hm, float* peak_val, int32_t* peak_idx, int32_t* npeaks, float* mpe, float* margin,
                           int N, int J, int H, int W, int min_distance, void* stream) {
    if (N <= 0) return 0;
    if (!hm || !peak_val || !peak_idx || !npeaks || !mpe || !margin) return fail(VATL_EINVAL, "peaks5: null pointer");
    if (min_distance < 1 || H <= 2 * min_distance || W <= 2 * min_distance) return fail(VATL_EINVAL, "peaks5: %dx%d plane too small for min_distance %d", H, W, min_distance);
    if (H == 64 && W == 48 && min_distance == 5 && (((uintptr_t)hm) & 15) == 0) {      // the shipped heat-map size: one wave per plane
        const long long planes = (long long)N * J;
        hipLaunchKernelGGL(peaks5_wave_kernel<48>, dim3((unsigned)cdiv(planes, 4)), dim3(256), 4 * 64 * (48 + 4) * sizeof(float), (hipStream_t)stream, hm, peak_val,
                           peak_idx, npeaks, mpe, margin, planes);
        return check_launch("peaks5");
    }
    const size_t smem = 2 * (size_t)H * W * sizeof(float);
    if (smem > 60 * 1024) return fail(VATL_EINVAL, "peaks5: heat-map %dx%d too large for the LDS tile", H, W);
    hipLaunchKernelGGL(peaks5_kernel, dim3((unsigned)(N * J)), dim3(256), smem, (hipStream_t)stream, hm, peak_val, peak_idx, npeaks, mpe, margin, H, W, min_distance);
    return check_launch("peaks5");
}

extern "C" int vatl_plane_entropy(const float* hm, float* out, int N, int J, int H, int W, void* stream) {
    if (N <= 0) return 0;
    if (!hm || !out) return fail(VATL_EINVAL, "plane_entropy: null pointer");
    const size_t smem = (size_t)H * W * sizeof(float);
    if (smem > 60 * 1024) return fail(VATL_EINVAL, "plane_entropy: heat-map %dx%d too large for the LDS tile", H, W);
    const long long planes = (long long)N * J;
    const int nv = wave_route_nv(hm, planes, H, W);
    if (nv == 12) hipLaunchKernelGGL(plane_entropy_wave_kernel<12>, dim3(cdiv(planes, 4)), dim3(256), 0, (hipStream_t)stream, hm, out, (int)planes);
    else if (nv == 27) hipLaunchKernelGGL(plane_entropy_wave_kernel<27>, dim3(cdiv(planes, 4)), dim3(256), 0, (hipStream_t)stream, hm, out, (int)planes);
    else hipLaunchKernelGGL(plane_entropy_kernel, dim3((unsigned)(N * J)), dim3(256), smem, (hipStream_t)stream, hm, out, H * W);
    return check_launch("plane_entropy");
}
