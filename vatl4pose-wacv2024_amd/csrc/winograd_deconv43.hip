// ConvTranspose2d(4, 2, 1) forward as Winograd F(4x3, 2x2) on the gfx950 fp32 matrix cores (inference).
//
// Each of the four sub-pixel phases of the transposed conv is a 2x2 convolution of the input (conv_winograd.hip).  There a 3x3 tile of
// phase outputs comes from a 4x4 input tile: 16 multiplies per 9 outputs, and the flagship's grids (8x6, 16x12, 32x24) need 9x6, 18x12
// and 33x24 tiles of coverage.  Here the tile is 4 rows x 3 columns from a 5x4 input tile — F(4,2) vertically on the points
// (0, 1, -1, 2, inf), the same F(3,2) horizontally: 20 multiplies per 12 outputs (1.667 against 1.778), 20 positions that split 5-5-5-5
// over four waves, and tiles that cover those grids exactly: 16.7 % / 16.7 % / 9.1 % fewer MFMAs for deconv1 / 2 / 3.
//
//     Y = A4^T [ (G4 g G3^T) .* (B4^T d B3) ] A3        U = G4 g G3^T: 20 values per filter, packed once (winograd_pack.h: wino43_pack_block)
//
// About twice the rounding error of F(3x3,2x2) (the factors 2, 3, 8 of the vertical transform); tests hold both to the same float64 bound.
//
// The matrices, the block (32 tiles x 64 output channels, wave nu = column position nu x all five row positions), the row transform and the MFMA
// group are winograd43.h's, shared with winograd_s2_43.hip; the stage and its offsets winograd_stage.h's; the tile order tile_order.h's.  This file's:
//   * one phase per block — the tile unit is (phase, 64 channels) — with that phase's padding and filter;
//   * per 8-channel step a wave reads its two columns of the five staged rows (10 ds_read_b128) and issues 40 MFMAs 32x32x2 (20 per 32-channel
//     half, the two filter-fragment sets of 20 registers alternating between the halves one group ahead);
//   * output transform: the xi sum (5 -> 4 rows) in registers, the nu sum (4 -> 3 columns) through LDS — [4 nu][4 rows][32 tiles][32 channels]
//     is exactly the two stage buffers — one 32-channel half at a time; a thread owns (tile, channel quad) and walks the four rows, so a
//     wave reads 1 KB contiguous per (nu, row) and stores 128-byte NHWC channel runs with scale / bias / ReLU into the phase's pixels of the
//     2H x 2W output.  (winograd_s2_43.hip has the same transform as text: as one function called from both, this kernel spills a register.)
// The per-output arithmetic depends only on the tile's own pixels: results do not depend on the batch position.
#include "common.h"
#include "buffer.h"
#include "tile_order.h"
#include "winograd43.h"

#include <algorithm>
#include <atomic>

namespace vatl {

struct Deconv43Params {
    const float* x;
    const float* u;
    const float* scale;
    const float* bias;
    float* y;
    int N, H, W, Cin, Cout;
    int TH, TW, tpi, Mtiles;          // tiles per image column / row / image (H / 4, W / 3), tiles in the launch
    int m_tiles, n_tiles;             // 32-tile groups, 64-channel filter tiles
    int relu;
    int stages;                       // Cin / 16
    int rn;                           // filter slices (phase, 64 channels) per group of the tile order
    long long u_phase_floats;
    unsigned x_bytes, u_bytes, y_bytes;
    FastDivU d_TH, d_TW, d_tpi, d_grp, d_rn, d_rn_last, d_ntiles;
};

// (body in a __device__ function, as winograd_body: with the DMA builtin inside the __global__ function hipcc drops the kernel's host stub)
__device__ __forceinline__ void winograd_deconv43_body(const Deconv43Params& p, float* smem) {
    constexpr int NW = 4;
    float* Rs = smem;                                      // [2][5 rows][3 arrays x 33 entries + zero entry][16 channels], chunk-swizzled
    const int tid = threadIdx.x, lane = tid & 63, nu = __builtin_amdgcn_readfirstlane(tid >> 6);

    // tile order (tile_order.h): slice = (phase, 64 output channels)
    int m_tile, unit;
    grouped_tile(p, xcd_contiguous_index(blockIdx.x, gridDim.x), p.n_tiles * 4, m_tile, unit);
    const int phase = fdiv(unit, p.d_ntiles), n_tile = unit - phase * p.n_tiles;
    const int m0 = m_tile * W_TB, n0 = n_tile * 64;
    const int py = phase >> 1, px = phase & 1;
    const int pad_y = 1 - py, pad_x = 1 - px;

    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t ur = buf_rsrc(p.u + (long long)phase * p.u_phase_floats, p.u_bytes);

    // ---- U fragments: [n_tile][step][position xi * 4 + nu][half][lane][4] -------------------------------------------------------------
    const int steps = p.stages * 2;
    const unsigned ubase = (unsigned)(((n_tile * steps) * 20 + nu) * 2 * 64 + lane) << 4;      // bytes; + step * 40 KB + xi * 8 KB + half * 1 KB
    auto u_load = [&](f32x4 (&dst)[5], int step_, int half) {
        const int step = min(step_, steps - 1);            // past the last step: the last step's fragments again, no per-lane select
        const unsigned off = ubase + (unsigned)half * 1024u + (unsigned)step * 40960u;
#pragma unroll
        for (int xi = 0; xi < 5; ++xi) dst[xi] = buf_load4(ur, off + xi * 8192u);
    };
    f32x4 ua[5], ub[5];
    u_load(ua, 0, 0);

    // ---- staging by LDS-DMA (winograd_stage.h): five input rows 4 ty - pad_y + i of the dense image -----------------------------------------
    unsigned goff[W43_NLD];
#pragma unroll
    for (int u = 0; u < W43_NLD; ++u)
        goff[u] = wino_piece_offset<W43Stage, 3, 4, false>(p, (nu + NW * u) * 64 + lane, m0, p.Mtiles, pad_y, pad_x, p.H, p.W);
    auto stage_dma = [&](int buf, int st) {
#pragma unroll
        for (int u = 0; u < W43_NLD; ++u)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void*)(Rs + buf * W43Stage::FLOATS + (nu + NW * u) * 256), 16,
                                                     goff[u] + (unsigned)st * (W_CK * 4), 0, 0, 0);
    };
    stage_dma(0, 0);
    if (p.stages > 1) stage_dma(1, 1);

    // ---- fragment addressing: lane = (tile l & 31, channel quad l >> 5); this wave's column combination is d[ja] + sgn * d[jb]
    // (B3^T rows: d0 - d2, d1 + d2, d2 - d1, d1 - d3).  ca / cb: float index (relative to a stage's input row, first 8-channel step) of the
    // two columns of the lane's tile; the second step is the same index ^ 8; a column outside the image = the row's zero entry.
    const int h = lane >> 5;
    const float sgn = nu == 1 ? 1.f : -1.f;
    int ca, cb;
    {
        const int tl = lane & 31;
        const int m = min(m0 + tl, p.Mtiles - 1);
        const int gr = fdiv(m, p.d_TW), tx = m - gr * p.TW;
        ca = wino_frag_col<3>(w43_col_a(nu), tl, h, tx, pad_x, p.W);
        cb = wino_frag_col<3>(w43_col_b(nu), tl, h, tx, pad_x, p.W);
    }

    f32x16 accs[2][5];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int xi = 0; xi < 5; ++xi)
#pragma unroll
            for (int e = 0; e < 16; ++e) accs[hh][xi][e] = 0.f;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's DMA pieces have landed
    __syncthreads();

    // The two fragment sets alternate between the halves with a look-ahead of one group of 20 MFMAs: (step 0, half 0) = ua [requested in the
    // stage before], (step 0, half 1) = ub, (step 1, half 0) = ua, ...  The scheduler barriers keep the requests where they are written.
    for (int st = 0; st < p.stages; ++st) {
        const int buf = st & 1;
        const float* Rb = Rs + buf * W43Stage::FLOATS;
        f32x4 v[5];
        u_load(ub, 2 * st, 1);
        __builtin_amdgcn_sched_barrier(0);
        w43_make_v<5>(v, Rb, ca, cb, sgn, 0);
        w43_mfma_group<5>(accs[0], v, ua);
        __builtin_amdgcn_sched_barrier(0);
        u_load(ua, 2 * st + 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        w43_mfma_group<5>(accs[1], v, ub);
        __builtin_amdgcn_sched_barrier(0);
        u_load(ub, 2 * st + 1, 1);
        if (st + 1 < p.stages && st > 0) stage_dma(buf ^ 1, st + 1);       // (behind the fragments of this stage's second step: loads retire in order)
        __builtin_amdgcn_sched_barrier(0);
        w43_make_v<5>(v, Rb, ca, cb, sgn, 8);
        w43_mfma_group<5>(accs[0], v, ua);
        __builtin_amdgcn_sched_barrier(0);
        u_load(ua, 2 * st + 2, 0);
        __builtin_amdgcn_sched_barrier(0);
        w43_mfma_group<5>(accs[1], v, ub);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of the next stage have landed
        __syncthreads();
    }

    // ---- output transform ---------------------------------------------------------------------------------------------------------------
    // thread = (tile tid >> 3, channel quad tid & 7); its 4 x 3 output pixels are base + a * row stride + b * column stride
    const __amdgpu_buffer_rsrc_t yr = buf_rsrc(p.y, p.y_bytes);
    const int c4 = tid & 7, tl = tid >> 3;
    const int OW = 2 * p.W;
    const unsigned cstep = (unsigned)(2 * p.Cout) << 2, rstep = (unsigned)(2 * OW * p.Cout) << 2;      // bytes between the phase's neighbouring columns / rows
    const bool valid = m0 + tl < p.Mtiles;
    unsigned obase;
    {
        const int m = min(m0 + tl, p.Mtiles - 1);
        const int b = fdiv(m, p.d_tpi), r = m - b * p.tpi;
        const int ty = fdiv(r, p.d_TW), tx = r - ty * p.TW;
        obase = (unsigned)(((b * 2 * p.H + 8 * ty + py) * OW + 6 * tx + px) * p.Cout + n0 + c4 * 4) << 2;
    }
    const float lo = p.relu ? 0.f : -INFINITY;
    float* Ps = smem;                                      // [nu][row a][tile][32 channels]
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {                       // one filter half at a time through the same LDS tiles
        const int n = n0 + 32 * hh + c4 * 4;
        f32x4 sc = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
        if (p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + n);       // requested before the accumulators go through LDS
        if (p.bias) bi = *reinterpret_cast<const f32x4*>(p.bias + n);
        // xi sum in registers (rows of A4^T): P0 = M0 + M1 + M2 + M3, P1 = M1 - M2 + 2 M3, P2 = M1 + M2 + 4 M3, P3 = M1 - M2 + 8 M3 + M4
        {
            const int cl = lane & 31;
            f32x16 (&ac)[5] = accs[hh];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                const float sum = ac[1][e] + ac[2][e], dif = ac[1][e] - ac[2][e], m3 = ac[3][e];
                Ps[((nu * 4 + 0) * W_TB + row) * 32 + cl] = ac[0][e] + sum + m3;
                Ps[((nu * 4 + 1) * W_TB + row) * 32 + cl] = dif + 2.f * m3;
                Ps[((nu * 4 + 2) * W_TB + row) * 32 + cl] = sum + 4.f * m3;
                Ps[((nu * 4 + 3) * W_TB + row) * 32 + cl] = dif + 8.f * m3 + ac[4][e];
            }
        }
        lds_barrier();
        // nu sum (rows of A3^T) per (tile, output row a, channel quad); 16-byte stores of NHWC channel runs
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            f32x4 pq[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) pq[k] = *reinterpret_cast<const f32x4*>(&Ps[((k * 4 + a) * W_TB + tl) * 32 + c4 * 4]);
            f32x4 yv[3];
            yv[0] = pq[0] + pq[1] + pq[2];
            yv[1] = pq[1] - pq[2];
            yv[2] = pq[1] + pq[2] + pq[3];
            if (valid) {
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    f32x4 o;
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] = fmaxf(yv[b][c] * sc[c] + bi[c], lo);
                    buf_store4(yr, obase + (unsigned)hh * 128u + (unsigned)a * rstep + (unsigned)b * cstep, o);
                }
            }
        }
        if (hh == 0) lds_barrier();                        // the second half's tiles go where this one's were read (the stores stay in flight)
    }
}

__global__ __launch_bounds__(256, 2) void winograd_deconv43_kernel(Deconv43Params p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    winograd_deconv43_body(p, smem);
}

static std::atomic<unsigned> g_d43_lds_done;

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_deconv4x4s2_winograd43_supported(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
    if (H % 4 != 0 || W % 3 != 0 || Cin % 16 != 0 || Cout % 64 != 0) return 0;
    const w43_count n = N;
    return w43_in_range(n * (H / 4) * (W / 3), n * H * W * Cin, 4 * n * H * W * Cout, (w43_count)20 * Cout * Cin, Cin, Cout / 64 * 4) ? 1 : 0;
}

extern "C" int vatl_deconv4x4s2_winograd43_fwd(const float* x, const float* u, const float* scale, const float* bias, float* y, int N, int H, int W,
                                               int Cin, int Cout, int relu, void* stream) {
    if (!x || !u || !y) return fail(VATL_EINVAL, "deconv4x4s2_winograd43_fwd: null pointer");
    if (!vatl_deconv4x4s2_winograd43_supported(N, H, W, Cin, Cout))
        return fail(VATL_EINVAL, "deconv4x4s2_winograd43_fwd: %d x %dx%d x %d -> %d is outside H %% 4 == 0, W %% 3 == 0, Cin %% 16 == 0, Cout %% 64 == 0 and 32-bit offsets",
                    N, H, W, Cin, Cout);
    Deconv43Params p{};
    p.x = x; p.u = u; p.scale = scale; p.bias = bias; p.y = y;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.relu = relu;
    p.TH = H / 4; p.TW = W / 3; p.tpi = p.TH * p.TW;
    p.Mtiles = N * p.tpi;
    p.m_tiles = cdiv(p.Mtiles, W_TB);
    p.n_tiles = Cout / 64;
    p.stages = Cin / W_CK;
    p.u_phase_floats = 20LL * Cout * Cin;
    p.x_bytes = (unsigned)((long long)N * H * W * Cin * 4);
    p.y_bytes = (unsigned)(4LL * N * H * W * Cout * 4);
    p.u_bytes = (unsigned)(p.u_phase_floats * 4);
    // a slice (phase, 64 channels) is Cin * 5 KB; the slices of a group (<= 2 MB, at least two) stay in an XCD's L2 over the sweep of the m-tiles
    const int units = p.n_tiles * 4;
    set_grouped_order(p, units, std::max(1, std::min(units, std::max(2, 2048 / (5 * Cin)))));
    p.d_TH = make_fastdiv(p.TH); p.d_TW = make_fastdiv(p.TW); p.d_tpi = make_fastdiv(p.tpi); p.d_ntiles = make_fastdiv(p.n_tiles);
    if (int rc = ensure_dynamic_lds((const void*)winograd_deconv43_kernel, W43_LDS_BYTES, g_d43_lds_done, "winograd_deconv43")) return rc;
    hipLaunchKernelGGL(winograd_deconv43_kernel, dim3((unsigned)(p.m_tiles * units)), dim3(256), W43_LDS_BYTES, (hipStream_t)stream, p);
    meter_add(1, 2.0 * ((double)p.m_tiles * W_TB) * 20.0 * (double)Cin * (double)Cout * 4.0);
    meter_route(kRouteWinoDeconv43);
    return check_launch("winograd_deconv43");
}
