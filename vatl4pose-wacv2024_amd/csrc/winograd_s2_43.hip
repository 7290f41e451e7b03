// 3x3 / stride 2 / pad 1 convolution forward as Winograd F(4x3, 2x2) summed over the four input phases (inference; Bottleneck.conv2 of the first
// block of ResNet stages 2 - 4).
//
// Pad the filter to 4x4 with a zero last row and column and write its tap r = 2a + b: y[o] = sum_b sum_a g_b[a] P_b[o + a] with the input phase
// P_b[i] = x[2i + b - 1] (zero outside the image) and g_b[a] = w[2a + b].  In 2-D that is four 2x2-tap stride-1 correlations — phase (by, bx):
// P[i][j] = x[2i + by - 1][2j + bx - 1], g[a][b] = w[2a + by][2b + bx] — each one exactly the F(4x3, 2x2) problem of winograd_deconv43.hip (a 4-row x
// 3-column output tile from a 5x4 tile of the phase image, the same B4^T, B3^T, G4, G3, A4^T, A3^T).  All four produce the SAME output tile through the
// same output transform, so their transform-domain products add into one accumulator set: the reduction runs over (phase, input channel), one
// launch, no partial sums in memory, one output transform per tile.
//
// The single-tap phases have g[1] = 0 and G4's last row is [0 1]: for the two by = 1 phases the transformed filter is identically zero at row position
// xi = 4.  That half of the reduction runs with four row positions (16 MFMAs per group instead of 20, four fragment loads, the fifth input row neither
// staged nor read): 20 + 20 + 16 + 16 = 72 multiplies per 12 outputs against the direct sum's 108 (1.5x fewer MFMAs), and the 32x24 / 16x12 / 8x6 output
// grids of the 256x192 networks are whole tiles.  (For the bx = 1 phases column position nu = 3 is zero as well; that would only idle one wave of a block
// that runs in lock-step and is not exploited.)
//
// The block is winograd_deconv43_body's; what the two share is in winograd43.h (matrices, row transform, MFMA group, host range check),
// winograd_stage.h (the stage and its offsets) and tile_order.h.  What differs:
//   * no phase in the tile unit: a block is (m-tile, 64-channel filter tile) and walks 4 * Cin / 16 stages — phase (0,0), (0,1) with five row positions,
//     then (1,0), (1,1) with four (the position count is a compile-time parameter of the stage body).
//   * the phase image is a stride-2 view: its pixel (yy, xx) = 4 ty + i - pad_y, 3 tx + r - pad_x (pad = 1 - b, inside for 0 <= yy < H / 2,
//     0 <= xx < W / 2) is image pixel (2 yy + pad_y, 2 xx + pad_x).  Which pieces are outside the image — and which of two tiles a shared column-array
//     entry serves at a row end — depends on the phase, and the descriptor's range check does not catch them (they land in a neighbouring row or image).
//     The eight staging offsets and the two fragment-read column indices of a lane are therefore recomputed at the three phase changes of a block
//     (the offsets one stage ahead, with the DMA that uses them) instead of kept four-fold in registers.
//   * the filter stream of a block is contiguous: [n / 64][by = 0: bx, step = c / 8, 20 positions | by = 1: bx, step, 16 positions][n / 32 % 2][lane][c % 4]
//     (winograd_pack.h: wino_s2_43_pack_block), U = G4 g G3^T in float64 rounded once.
//   * epilogue: dense NHWC output, scale / bias / ReLU, no residual.
// The executed FLOPs, 2 * (tiles rounded up to 32) * 72 * Cin * Cout, are booked in the meter's DIRECT class: the launch is reached through conv2d_fwd, whose
// time the benchmark books under its implicit-GEMM group; in the Winograd class they would add FLOPs without time to the other group's fraction.
// The per-output arithmetic depends only on the tile's own pixels: results do not depend on the batch position.
#include "common.h"
#include "buffer.h"
#include "tile_order.h"
#include "winograd43.h"

#include <algorithm>
#include <atomic>
#include <type_traits>

namespace vatl {

struct S2W43Params {
    const float* x;
    const float* u;
    const float* scale;
    const float* bias;
    float* y;
    int N, H, W, Cin, Cout;
    int OH, OW;                       // output grid = grid of every phase image's valid pixels (H / 2, W / 2)
    int TH, TW, tpi, Mtiles;          // tiles per image column / row / image (OH / 4, OW / 3), tiles in the launch
    int m_tiles, n_tiles;             // 32-tile groups, 64-channel filter tiles
    int relu;
    int sp;                           // stages per phase: Cin / 16
    int rn;                           // filter tiles per group of the tile order
    unsigned x_bytes, u_bytes, y_bytes;
    FastDivU d_TH, d_TW, d_tpi, d_grp, d_rn, d_rn_last;
};

constexpr int S2W_ROW4_DMA = 4 * W43Stage::ROWE * 4 / 64;      // first DMA instruction of the fifth input row
static_assert(4 * W43Stage::ROWE * 4 % 64 == 0, "the fifth input row starts a DMA instruction");

// (body in a __device__ function, as winograd_body: with the DMA builtin inside the __global__ function hipcc drops the kernel's host stub)
__device__ __forceinline__ void winograd_s2_43_body(const S2W43Params& p, float* smem) {
    constexpr int NW = 4;
    float* Rs = smem;                                      // [2][5 rows][3 arrays x 33 entries + zero entry][16 channels], chunk-swizzled
    const int tid = threadIdx.x, lane = tid & 63, nu = __builtin_amdgcn_readfirstlane(tid >> 6);

    // tile order (tile_order.h): slice = 64-channel filter tile
    int m_tile, n_tile;
    grouped_tile(p, xcd_contiguous_index(blockIdx.x, gridDim.x), p.n_tiles, m_tile, n_tile);
    const int m0 = m_tile * W_TB, n0 = n_tile * 64;

    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t ur = buf_rsrc(p.u, p.u_bytes);

    // ---- U fragments: [n_tile][by = 0: 2 * steps x 20 positions | by = 1: 2 * steps x 16 positions][half][lane][4], position = xi * 4 + nu ----------
    const int steps = p.sp * 2;                            // 8-channel steps per phase
    const int gsteps = 4 * steps, gsteps5 = 2 * steps;     // steps of the block; of them with five row positions
    const unsigned ubase = (unsigned)n_tile * (unsigned)steps * 147456u + ((unsigned)((nu * 2) * 64 + lane) << 4);     // bytes; + xi * 8 KB + half * 1 KB
    auto u_load = [&](auto np, f32x4 (&dst)[5], int gstep_, int half) {
        constexpr int NP = decltype(np)::value;
        const int g = min(gstep_, gsteps - 1);             // past the last step: the last step's fragments again, no per-lane select
        const unsigned soff = g < gsteps5 ? (unsigned)g * 40960u : (unsigned)gsteps5 * 40960u + (unsigned)(g - gsteps5) * 32768u;
        const unsigned off = ubase + (unsigned)half * 1024u + soff;
#pragma unroll
        for (int xi = 0; xi < NP; ++xi) dst[xi] = buf_load4(ur, off + xi * 8192u);
    };
    f32x4 ua[5], ub[5];
    u_load(std::integral_constant<int, 5>{}, ua, 0, 0);

    // ---- staging by LDS-DMA (winograd_stage.h) from the stride-2 view of the phase image (pad_y, pad_x) = (1 - by, 1 - bx) --------------------------
    unsigned goff[W43_NLD];
    // (m0 and the lane go through an empty asm: without it the compiler hoists the phase-independent part of every call out of the stage loops
    // and keeps it in registers the loop does not have)
    auto set_goff = [&](int pad_y, int pad_x) {
        int m0 = m_tile * W_TB, ln = lane;
        asm volatile("" : "+s"(m0), "+v"(ln));
#pragma unroll
        for (int u = 0; u < W43_NLD; ++u) {
            __builtin_amdgcn_sched_barrier(0);             // one offset at a time: the accumulators and a fragment set are live around the later calls
            goff[u] = wino_piece_offset<W43Stage, 3, 4, true>(p, (nu + NW * u) * 64 + ln, m0, p.Mtiles, pad_y, pad_x, p.OH, p.OW);
        }
    };
    // st: stage inside the phase the offsets were made for; rows5: that phase has five row positions (else the fifth input row is not staged)
    auto stage_dma = [&](int buf, int st, bool rows5) {
        unsigned so = (unsigned)st * (W_CK * 4);
        asm volatile("" : "+s"(so));                       // (opaque: otherwise the loop keeps a second, advancing copy of the eight offsets)
#pragma unroll
        for (int u = 0; u < W43_NLD; ++u) {
            if (!rows5 && nu + NW * u >= S2W_ROW4_DMA) continue;           // (wave-uniform)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void*)(Rs + buf * W43Stage::FLOATS + (nu + NW * u) * 256), 16,
                                                     goff[u] + so, 0, 0, 0);
        }
    };
    set_goff(1, 1);
    stage_dma(0, 0, true);

    // ---- fragment addressing: lane = (tile l & 31, channel quad l >> 5); this wave's column combination is d[ja] + sgn * d[jb]
    // (B3^T rows: d0 - d2, d1 + d2, d2 - d1, d1 - d3).  ca / cb: float index (relative to a stage's input row, first 8-channel step) of the
    // two columns of the lane's tile; the second step is the same index ^ 8; a column outside the phase image = the row's zero entry.
    const float sgn = nu == 1 ? 1.f : -1.f;
    int ca, cb;
    auto set_cols = [&](int pad_x) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int tl = ln & 31, h = ln >> 5;
        const int m = min(m0 + tl, p.Mtiles - 1);
        const int gr = fdiv(m, p.d_TW), tx = m - gr * p.TW;
        ca = wino_frag_col<3>(w43_col_a(nu), tl, h, tx, pad_x, p.OW);
        cb = wino_frag_col<3>(w43_col_b(nu), tl, h, tx, pad_x, p.OW);
    };

    f32x16 accs[2][5];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int xi = 0; xi < 5; ++xi)
#pragma unroll
            for (int e = 0; e < 16; ++e) accs[hh][xi][e] = 0.f;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's DMA pieces have landed
    __syncthreads();

    // One phase: its Cin / 16 stages.  The two fragment sets alternate between the halves with a look-ahead of one group of MFMAs, as in winograd_deconv43_body;
    // the scheduler barriers keep the requests where they are written.  gs0: the phase's first stage in the block's count (fragment steps and the stage buffer
    // follow it).  The DMA issued in a stage fills the other buffer for the next stage; in a phase's last stage that is the next phase's first one, so the
    // offsets change before it.  (A fragment request that crosses into the four-position half with NP = 5 reads one fragment it does not use.)
    auto run_phase = [&](auto np, int ph, int gs0) {
        constexpr int NP = decltype(np)::value;
        set_cols(1 - (ph & 1));
        for (int st = 0; st < p.sp; ++st) {
            const int gs = gs0 + st, buf = gs & 1;
            const float* Rb = Rs + buf * W43Stage::FLOATS;
            const bool wrap = st + 1 == p.sp;
            if (wrap && ph < 3) set_goff(1 - ((ph + 1) >> 1), 1 - ((ph + 1) & 1));
            f32x4 v[5];
            u_load(np, ub, 2 * gs, 1);
            __builtin_amdgcn_sched_barrier(0);
            w43_make_v<NP>(v, Rb, ca, cb, sgn, 0);
            w43_mfma_group<NP>(accs[0], v, ua);
            __builtin_amdgcn_sched_barrier(0);
            u_load(np, ua, 2 * gs + 1, 0);
            __builtin_amdgcn_sched_barrier(0);
            w43_mfma_group<NP>(accs[1], v, ub);
            __builtin_amdgcn_sched_barrier(0);
            u_load(np, ub, 2 * gs + 1, 1);
            if (!(wrap && ph == 3)) stage_dma(buf ^ 1, wrap ? 0 : st + 1, wrap ? ph + 1 < 2 : ph < 2);      // (behind the fragments of this stage's second step: loads retire in order)
            __builtin_amdgcn_sched_barrier(0);
            w43_make_v<NP>(v, Rb, ca, cb, sgn, 8);
            w43_mfma_group<NP>(accs[0], v, ua);
            __builtin_amdgcn_sched_barrier(0);
            u_load(np, ua, 2 * gs + 2, 0);
            __builtin_amdgcn_sched_barrier(0);
            w43_mfma_group<NP>(accs[1], v, ub);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of the next stage have landed
            __syncthreads();
        }
    };
    run_phase(std::integral_constant<int, 5>{}, 0, 0);
    run_phase(std::integral_constant<int, 5>{}, 1, p.sp);
    run_phase(std::integral_constant<int, 4>{}, 2, 2 * p.sp);
    run_phase(std::integral_constant<int, 4>{}, 3, 3 * p.sp);

    // ---- output transform (winograd_deconv43_body's as text, see there; dense output) -----------------------------------------------------
    // thread = (tile tid >> 3, channel quad tid & 7); its 4 x 3 output pixels are base + a * row stride + b * column stride
    const __amdgpu_buffer_rsrc_t yr = buf_rsrc(p.y, p.y_bytes);
    const int c4 = tid & 7, tl = tid >> 3;
    const unsigned cstep = (unsigned)p.Cout << 2, rstep = (unsigned)(p.OW * p.Cout) << 2;      // bytes between neighbouring columns / rows
    const bool valid = m0 + tl < p.Mtiles;
    unsigned obase;
    {
        const int m = min(m0 + tl, p.Mtiles - 1);
        const int b = fdiv(m, p.d_tpi), r = m - b * p.tpi;
        const int ty = fdiv(r, p.d_TW), tx = r - ty * p.TW;
        obase = (unsigned)(((b * p.OH + 4 * ty) * p.OW + 3 * tx) * p.Cout + n0 + c4 * 4) << 2;
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

__global__ __launch_bounds__(256, 2) void winograd_s2_43_kernel(S2W43Params p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    winograd_s2_43_body(p, smem);
}

static std::atomic<unsigned> g_s2w43_lds_done;

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_conv3x3s2_winograd43_supported(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
    if (H % 8 != 0 || W % 6 != 0 || Cin % 16 != 0 || Cout % 64 != 0) return 0;         // H, W even, (H / 2) % 4 == 0, (W / 2) % 3 == 0
    const w43_count n = N;
    return w43_in_range(n * (H / 8) * (W / 6), n * H * W * Cin, n * (H / 2) * (W / 2) * Cout, (w43_count)72 * Cout * Cin, Cin, Cout / 64) ? 1 : 0;
}

extern "C" int vatl_conv3x3s2_winograd43_fwd(const float* x, const float* u, const float* scale, const float* bias, float* y, int N, int H, int W,
                                             int Cin, int Cout, int relu, void* stream) {
    if (!x || !u || !y) return fail(VATL_EINVAL, "conv3x3s2_winograd43_fwd: null pointer");
    if (!vatl_conv3x3s2_winograd43_supported(N, H, W, Cin, Cout))
        return fail(VATL_EINVAL, "conv3x3s2_winograd43_fwd: %d x %dx%d x %d -> %d is outside H %% 8 == 0, W %% 6 == 0, Cin %% 16 == 0, Cout %% 64 == 0 and 32-bit offsets",
                    N, H, W, Cin, Cout);
    S2W43Params p{};
    p.x = x; p.u = u; p.scale = scale; p.bias = bias; p.y = y;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.relu = relu;
    p.OH = H / 2; p.OW = W / 2;
    p.TH = p.OH / 4; p.TW = p.OW / 3; p.tpi = p.TH * p.TW;
    p.Mtiles = N * p.tpi;
    p.m_tiles = cdiv(p.Mtiles, W_TB);
    p.n_tiles = Cout / 64;
    p.sp = Cin / W_CK;
    p.x_bytes = (unsigned)((long long)N * H * W * Cin * 4);
    p.y_bytes = (unsigned)((long long)N * p.OH * p.OW * Cout * 4);
    p.u_bytes = (unsigned)(72LL * Cout * Cin * 4);
    // a filter tile (64 channels, all four phases) is Cin * 18 KB; the tiles of a group (<= 2 MB, at least two) stay in an XCD's L2 over the sweep of the m-tiles
    set_grouped_order(p, p.n_tiles, std::max(1, std::min(p.n_tiles, std::max(2, 2048 / (18 * Cin)))));
    p.d_TH = make_fastdiv(p.TH); p.d_TW = make_fastdiv(p.TW); p.d_tpi = make_fastdiv(p.tpi);
    if (int rc = ensure_dynamic_lds((const void*)winograd_s2_43_kernel, W43_LDS_BYTES, g_s2w43_lds_done, "winograd_s2_43")) return rc;
    hipLaunchKernelGGL(winograd_s2_43_kernel, dim3((unsigned)(p.m_tiles * p.n_tiles)), dim3(256), W43_LDS_BYTES, (hipStream_t)stream, p);
    meter_add(0, 2.0 * ((double)p.m_tiles * W_TB) * 72.0 * (double)Cin * (double)Cout);
    meter_route(kRouteWinoS2_43);
    return check_launch("winograd_s2_43");
}
