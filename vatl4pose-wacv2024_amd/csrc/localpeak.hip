// Local peaks of the (N,J,H,W) fp32 heat-maps: localpeak_mean / localpeak_values, active_learning/local_peak.py:5-22.
// A pixel is a local maximum when it equals the maximum of its 3x3 neighbourhood with a zero halo (scipy mode='constant', cval=0); the
// kept peaks are those >= order * the largest of them.  One block per (item, joint) plane; per-plane (sum, count) of the kept peaks go
// to a workspace and a second kernel forms the per-item mean in joint order (deterministic).
#include "scorer_common.h"

namespace vatl {

// maximum of the 3x3 ring and centre whose rows start at up / mid / dn (the centre is mid[1])
__device__ __forceinline__ float max3x3(const float* up, const float* mid, const float* dn) {
    float m = fmaxf(fmaxf(up[0], up[1]), up[2]);
    m = fmaxf(m, fmaxf(mid[0], mid[2]));
    return fmaxf(m, fmaxf(fmaxf(dn[0], dn[1]), dn[2]));
}
// the same around the pixel c of an LDS tile of pitch PW
__device__ __forceinline__ float tile_max3x3(const float* c, int PW) { return max3x3(c - PW - 1, c - 1, c + PW - 1); }

// plane into the (H+2) x (W+2) LDS tile with its zero halo, any width: scalar loads
__device__ __forceinline__ void stage_tile(const float* src, float* tile, int H, int W) {
    const int PW = W + 2, PN = (H + 2) * PW;
    for (int q = threadIdx.x; q < PN; q += 256) {
        const int y = q / PW - 1, x = q % PW - 1;
        tile[q] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? src[y * W + x] : 0.f;
    }
}

// a plane's (sum, count) of kept peaks (one thread)
__device__ __forceinline__ void store_plane_result(double* ws, int32_t* count_out, double sum, int count) {
    ws[2 * (long long)blockIdx.x] = sum;
    ws[2 * (long long)blockIdx.x + 1] = (double)count;
    if (count_out) count_out[blockIdx.x] = count;
}

// four-wave blocks: per-thread (sum, count) -> the plane's result
__device__ __forceinline__ void reduce_plane_result(double* ws, int32_t* count_out, float s, int cnt, double* wsum, int* wcnt) {
    block4_put(wsum, wave_sum((double)s)); block4_put(wcnt, wave_sum(cnt));
    __syncthreads();
    if (threadIdx.x == 0) store_plane_result(ws, count_out, block4_sum(wsum), block4_sum(wcnt));
}

// W % 4 == 0 planes that the register kernel below does not take: 16-byte loads into the LDS tile, 1x4 strips per thread
__global__ __launch_bounds__(256) void localpeak_plane_kernel(const float* __restrict__ hm, double* __restrict__ ws, int32_t* __restrict__ count_out,
                                                              int H, int W, float order) {
    extern __shared__ __attribute__((aligned(16))) float tile[];        // (H+2) x (W+2), zero halo
    __shared__ float wmax[4];
    __shared__ int wcnt[4];
    __shared__ double wsum[4];
    const int tid = threadIdx.x;
    const int HW = H * W, PW = W + 2;
    const float* src = hm + (long long)blockIdx.x * HW;
    // interior: 16-byte global loads (W % 4 == 0: a float4 never straddles rows); halo: zeros
    const int n4 = HW >> 2, W4 = W >> 2;
    const float inv_w4 = 1.0f / (float)W4;
    for (int q = tid; q < n4; q += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
        const int y = fast_div(q, inv_w4), x = 4 * (q - y * W4);
        float* d = tile + (y + 1) * PW + x + 1;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    for (int q = tid; q < PW; q += 256) { tile[q] = 0.f; tile[(H + 1) * PW + q] = 0.f; }
    for (int q = tid; q < H; q += 256) { tile[(q + 1) * PW] = 0.f; tile[(q + 1) * PW + W + 1] = 0.f; }
    __syncthreads();
    // pass 1: local maxima and the largest of them.  Each thread owns 1x4 strips: 18 LDS reads serve four pixels.  Peak flags are
    // kept in a per-thread bit set for pass 2.
    float pmax = -INFINITY;
    unsigned long long flags = 0ull;                           // strip k of this thread, pixel e  ->  bit 4k + e   (n4 <= 16 * 256)
    int k = 0;
    for (int q = tid; q < n4; q += 256, ++k) {
        const int y = fast_div(q, inv_w4), x = 4 * (q - y * W4);
        const float* c = tile + (y + 1) * PW + (x + 1);
        float up[6], mid[6], dn[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) { up[e] = c[-PW - 1 + e]; mid[e] = c[-1 + e]; dn[e] = c[PW - 1 + e]; }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = mid[e + 1];
            if (v >= max3x3(up + e, mid + e, dn + e)) { pmax = fmaxf(pmax, v); flags |= 1ull << (4 * k + e); }
        }
    }
    block4_put(wmax, wave_max(pmax));
    __syncthreads();
    pmax = block4_max(wmax);
    // pass 2: keep peaks >= order * largest peak
    const float thr = pmax * order;
    float s = 0.f;
    int cnt = 0;
    if (pmax > -INFINITY && flags) {
        k = 0;
        for (int q = tid; q < n4; q += 256, ++k) {
            const unsigned f = (unsigned)(flags >> (4 * k)) & 15u;
            if (!f) continue;
            const int y = fast_div(q, inv_w4), x = 4 * (q - y * W4);
            const float* c = tile + (y + 1) * PW + (x + 1);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((f >> e) & 1u) { const float v = c[e]; if (v >= thr) { s += v; ++cnt; } }
        }
    }
    reduce_plane_result(ws, count_out, s, cnt, wsum, wcnt);
}

// Register-tile variant for W % 4 == 0 (every shipped heat-map size): the plane never touches LDS.  A thread owns a 4-column x
// RPT-row patch: RPT + 2 float4 row loads (the two halo rows come out of L1/L2), the 3x3 maximum is a vertical max3 in registers
// followed by a horizontal max3 whose outer columns come from the neighbouring lanes (one shuffle each way per row).  Lanes
// are laid out [row group][float4 column] with whole row groups per wave, so a neighbour is always lane +- 1 of the same wave.
// Rows / columns outside the plane read as 0.  Up to 16 waves per block, so its combines loop over the waves.
template <int RPT>
__global__ __launch_bounds__(1024) void localpeak_plane_reg_kernel(const float* __restrict__ hm, double* __restrict__ ws, int32_t* __restrict__ count_out,
                                                                   int H, int W, float order) {
    __shared__ float wmax[16];
    __shared__ int wcnt[16];
    __shared__ double wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int W4 = W >> 2, gpw = 64 / W4;                     // float4 columns per row, row groups per wave
    const int g = lane / W4, c4 = lane - g * W4;
    const bool on = g < gpw;
    const int row0 = (wave * gpw + g) * RPT;                  // first row of this thread's patch
    const float* src = hm + (long long)blockIdx.x * H * W + 4 * c4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 v[RPT + 2];
#pragma unroll
    for (int r = 0; r < RPT + 2; ++r) {
        const int y = row0 - 1 + r;
        v[r] = (on && y >= 0 && y < H) ? *reinterpret_cast<const f32x4*>(src + (long long)y * W) : zero;
    }
    float pmax = -INFINITY;
    unsigned long long flags = 0ull;                          // row r, column e of the patch -> bit 4 r + e
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        f32x4 vm;
#pragma unroll
        for (int e = 0; e < 4; ++e) vm[e] = fmaxf(fmaxf(v[r][e], v[r + 1][e]), v[r + 2][e]);
        float left = __shfl_up(vm[3], 1, 64), right = __shfl_down(vm[0], 1, 64);
        if (c4 == 0) left = 0.f;
        if (c4 == W4 - 1) right = 0.f;
        const float L[4] = {fmaxf(fmaxf(left, vm[0]), vm[1]), fmaxf(fmaxf(vm[0], vm[1]), vm[2]), fmaxf(fmaxf(vm[1], vm[2]), vm[3]),
                            fmaxf(fmaxf(vm[2], vm[3]), right)};
        const bool live = on && row0 + r < H;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float c = v[r + 1][e];
            if (live && c >= L[e]) { pmax = fmaxf(pmax, c); flags |= 1ull << (4 * r + e); }
        }
    }
    pmax = wave_max(pmax);
    if (lane == 0) wmax[wave] = pmax;
    __syncthreads();
    pmax = wmax[0];
    for (int w = 1; w < nw; ++w) pmax = fmaxf(pmax, wmax[w]);
    // pass 2: keep peaks >= order * largest peak (values still in registers)
    const float thr = pmax * order;
    float s = 0.f;
    int cnt = 0;
    if (pmax > -INFINITY && flags) {
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((flags >> (4 * r + e)) & 1ull) { const float c = v[r + 1][e]; if (c >= thr) { s += c; ++cnt; } }
    }
    const double ds = wave_sum((double)s);
    cnt = wave_sum(cnt);
    if (lane == 0) { wsum[wave] = ds; wcnt[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        int c = 0;
        for (int w = 0; w < nw; ++w) { t += wsum[w]; c += wcnt[w]; }
        store_plane_result(ws, count_out, t, c);
    }
}

// any width (the per-item API accepts arbitrary planes): scalar loads, one pixel per thread step
__global__ __launch_bounds__(256) void localpeak_plane_generic_kernel(const float* __restrict__ hm, double* __restrict__ ws, int32_t* __restrict__ count_out,
                                                              int H, int W, float order) {
    extern __shared__ __attribute__((aligned(16))) float tile[];        // (H+2) x (W+2)
    __shared__ float wmax[4];
    __shared__ int wcnt[4];
    __shared__ double wsum[4];
    const int tid = threadIdx.x;
    const int HW = H * W, PW = W + 2;
    stage_tile(hm + (long long)blockIdx.x * HW, tile, H, W);
    __syncthreads();
    // pass 1: largest local maximum; the peak flag is kept in a per-thread bit set so that pass 2 does not redo the nine reads
    float pmax = -INFINITY;
    unsigned long long flags = 0ull;                           // element q = tid + 256 k  ->  bit k  (HW <= 64 * 256)
    int k = 0;
    for (int q = tid; q < HW; q += 256, ++k) {
        const int y = q / W, x = q - y * W;
        const float* c = tile + (y + 1) * PW + (x + 1);
        const float v = c[0];
        if (v >= tile_max3x3(c, PW)) { pmax = fmaxf(pmax, v); flags |= 1ull << k; }
    }
    block4_put(wmax, wave_max(pmax));
    __syncthreads();
    pmax = block4_max(wmax);
    // pass 2: keep peaks >= order * largest peak
    const float thr = pmax * order;
    float s = 0.f;
    int cnt = 0;
    if (pmax > -INFINITY) {
        k = 0;
        for (int q = tid; q < HW; q += 256, ++k) {
            if (!((flags >> k) & 1ull)) continue;
            const int y = q / W, x = q - y * W;
            const float v = tile[(y + 1) * PW + (x + 1)];
            if (v >= thr) { s += v; ++cnt; }
        }
    }
    reduce_plane_result(ws, count_out, s, cnt, wsum, wcnt);
}

__global__ void localpeak_finish_kernel(const double* __restrict__ ws, float* __restrict__ mean_out, int N, int J) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double tot = 0.0, cnt = 0.0;
    for (int j = 0; j < J; ++j) { tot += ws[2 * ((long long)i * J + j)]; cnt += ws[2 * ((long long)i * J + j) + 1]; }
    mean_out[i] = cnt > 0.0 ? (float)(tot / cnt) : __builtin_nanf("");
}

// kept-peak mask of localpeak_values, any plane size (no bound on H * W, so no per-thread flag set: pass 2 tests the pixel again)
__global__ __launch_bounds__(256) void localpeak_mask_kernel(const float* __restrict__ hm, uint8_t* __restrict__ mask, int H, int W, float order) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    __shared__ float wmax[4];
    const int tid = threadIdx.x;
    const int HW = H * W, PW = W + 2;
    stage_tile(hm + (long long)blockIdx.x * HW, tile, H, W);
    __syncthreads();
    float pmax = -INFINITY;
    for (int q = tid; q < HW; q += 256) {
        const int y = q / W, x = q - y * W;
        const float* c = tile + (y + 1) * PW + (x + 1);
        if (c[0] >= tile_max3x3(c, PW)) pmax = fmaxf(pmax, c[0]);
    }
    block4_put(wmax, wave_max(pmax));
    __syncthreads();
    pmax = block4_max(wmax);
    const float thr = pmax * order;
    for (int q = tid; q < HW; q += 256) {
        const int y = q / W, x = q - y * W;
        const float* c = tile + (y + 1) * PW + (x + 1);
        mask[(long long)blockIdx.x * HW + q] = (pmax > -INFINITY && c[0] >= tile_max3x3(c, PW) && c[0] >= thr) ? 1 : 0;
    }
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_localpeak_mean(const float* hm, float* mean, int32_t* count, double* workspace, int N, int J, int H, int W, float order,
                                   void* stream) {
    if (N <= 0) return 0;
    if (!hm || !mean || !workspace) return fail(VATL_EINVAL, "localpeak_mean: null pointer");
    const size_t smem = (size_t)(H + 2) * (W + 2) * sizeof(float);
    if (smem > 60 * 1024 || (long long)H * W > 64 * 256) return fail(VATL_EINVAL, "localpeak_mean: heat-map %dx%d too large for the LDS tile", H, W);
    const int W4 = W >> 2, gpw = W4 > 0 ? 64 / W4 : 0;
    const int reg_waves = gpw > 0 ? cdiv(H, 16 * gpw) : 1 << 30;     // register-tile kernel: 16 rows per thread, whole row groups per wave
    if (W & 3) hipLaunchKernelGGL(localpeak_plane_generic_kernel, dim3((unsigned)(N * J)), dim3(256), smem, (hipStream_t)stream, hm, workspace, count, H, W, order);
    else if (reg_waves <= 16 && (((uintptr_t)hm) & 15) == 0)
        hipLaunchKernelGGL(localpeak_plane_reg_kernel<16>, dim3((unsigned)(N * J)), dim3(64 * reg_waves), 0, (hipStream_t)stream, hm, workspace, count, H, W, order);
    else       hipLaunchKernelGGL(localpeak_plane_kernel, dim3((unsigned)(N * J)), dim3(256), smem, (hipStream_t)stream, hm, workspace, count, H, W, order);
    hipLaunchKernelGGL(localpeak_finish_kernel, dim3(cdiv(N, 128)), dim3(128), 0, (hipStream_t)stream, workspace, mean, N, J);
    return check_launch("localpeak_mean");
}

extern "C" int vatl_localpeak_mask(const float* hm, uint8_t* mask, int planes, int H, int W, float order, void* stream) {
    if (planes <= 0) return 0;
    if (!hm || !mask) return fail(VATL_EINVAL, "localpeak_mask: null pointer");
    const size_t smem = (size_t)(H + 2) * (W + 2) * sizeof(float);
    if (smem > 60 * 1024) return fail(VATL_EINVAL, "localpeak_mask: map %dx%d too large for the LDS tile", H, W);
    hipLaunchKernelGGL(localpeak_mask_kernel, dim3(planes), dim3(256), smem, (hipStream_t)stream, hm, mask, H, W, order);
    return check_launch("localpeak_mask");
}
