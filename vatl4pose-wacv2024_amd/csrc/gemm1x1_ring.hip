// The LDS-DMA ring GEMM for the long-K 1x1 layers: kernel, launcher, the gate dispatch() asks (ring_wanted) and knob 27.
#include "conv_igemm.h"
#include "tile_order.h"
#include "tune.h"

namespace vatl {

// ---------------------------------------------------------------------------------------------------------
// Long-K 1x1 / stride-1 layers (K >= 512, and the dual-source conv3 + projection): a plain GEMM Y[M][N] = A[M][K] W[N][K]^T on
// 128 x 128 tiles with an LDS-DMA OPERAND RING.  The r01 ablation of the tiled kernel puts 12 % of its time on staging (global
// loads + ds_write: 138 -> 150 TFLOP/s without them), and fp32 MFMAs do not overlap vector instructions on a SIMD.  Here:
//  * stages of 16 k (two 8-deep fragment groups) = (128 + 128) rows x 64 bytes = 16 KB; a ring of four = 64 KB per block, two blocks
//    per CU.  While stage s is multiplied, stages s+1 .. s+3 are in flight (look-ahead 3, against 1 for VAR 5, conv_igemm_dma_kernel);
//  * both operands are staged by buffer_load ... lds only (no staging registers, no ds_write).  A lane's source offset is fixed for
//    the tile (row * K + chunk); the stage advance is the SGPR soffset s * 64.  The k-loop is MFMAs, ds_read_b128, four DMA
//    instructions per wave and stage, scalar ops, one counted s_waitcnt and one barrier per stage;
//  * LDS rows are 64 bytes (4 chunks of 16 B); chunk c of tile row r lives at position c ^ ((r >> 2) & 3), applied on the SOURCE
//    side (the DMA destination is lane-linear).  Each 16-lane service group of a ds_read_b128 fragment read ({0-3, 12-15, 20-27},
//    {4-11, 16-19, 28-31}, same + 32) covers rows with four different (r >> 2) & 3 and four different r & 3: all 16 slots of a
//    256-byte bank row, conflict-free;
//  * tail rows (m >= M) read row M-1 (in range; their outputs are dropped by the descriptor: offsets >= M * Cout * 4);
//  * the epilogue writes straight from the accumulator layout (a half wave stores a 128-byte channel run per row, as
//    conv1x1_rows256_kernel), the residual is requested two stages before the end.
// Dual source: stages 0 .. 2 k1 - 1 read x (one row per output pixel), the rest read x2 at the row's strided pixel.
// Same k order as conv_igemm_kernel (lanes 0-31: k = 8g + t, lanes 32-63: k = 8g + 4 + t, groups ascending; x before x2) and the
// same epilogue arithmetic: bit-identical results.
// ---------------------------------------------------------------------------------------------------------
constexpr int RING_BK = 16;                       // k per stage
constexpr int RING_NS = 4;                        // stages in the ring
constexpr int RING_STAGE = 256 * RING_BK;         // floats per stage: 128 A rows, then 128 B rows
constexpr int RING_BYTES = RING_NS * RING_STAGE * (int)sizeof(float);

template <int N>
__device__ __forceinline__ void ring_wait_vm() {  // s_waitcnt vmcnt(N) with a compile-time N (the DMA requests are not in hipcc's own bookkeeping)
    static_assert(N == 0 || N == 4 || N == 8 || N == 32 || N == 36, "add the count here");
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 32) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(36)" ::: "memory");
}

template <bool DUAL, bool RES>
__device__ __forceinline__ void gemm1x1_ring_body(const ConvParams& p, float* smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;      // 2 x 2 waves of 64 x 64

    // tile order of conv_igemm_kernel (order 0): each XCD a contiguous run, n-tile fastest
    const int t = xcd_contiguous_index(blockIdx.x, gridDim.x);
    const int m_tile = t / p.n_tiles, n_tile = t - m_tile * p.n_tiles;
    const int m0 = m_tile * 128, n0 = n_tile * 128;

    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t wr = buf_rsrc(p.w, p.w_bytes);
    const __amdgpu_buffer_rsrc_t xr2 = buf_rsrc(DUAL ? p.x2 : p.x, DUAL ? p.x2_bytes : p.x_bytes);

    // ---- loader: DMA instruction u (0, 1) of wave w fills tile rows (4u + w) * 16 .. + 15 of A and of B; lane -> (row lane >> 2,
    // position lane & 3), which receives the row's chunk (lane & 3) ^ ((row >> 2) & 3) = (lane & 3) ^ ((lane >> 4) & 3)
    const int lchk = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned aoff[2], boff[2], aoff2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int row = (4 * u + wave) * 16 + (lane >> 2);
        const int m = min(m0 + row, p.M - 1);
        aoff[u] = (unsigned)m * (unsigned)(p.Cin * 4) + (unsigned)lchk * 16u;
        aoff2[u] = 0;
        if (DUAL) {
            const int b = fdiv(m, p.d_HoWo);
            const int rem = m - b * p.Ho * p.Wo;
            const int oy = fdiv(rem, p.d_Wo);
            const int ox = rem - oy * p.Wo;
            aoff2[u] = (unsigned)((b * p.H2 + oy * p.stride2) * p.W2 + ox * p.stride2) * (unsigned)(p.C2 * 4) + (unsigned)lchk * 16u;
        }
        boff[u] = (unsigned)(n0 + row) * (unsigned)(p.K * 4) + (unsigned)lchk * 16u;
    }
    const int S = p.ktiles * 2;                   // stages (a multiple of 4: ring_wanted)
    const int S1 = DUAL ? p.k1 * 2 : S;           // stages that read x
    // DMA of stage s into ring slot buf: offsets fixed per tile, the stage in soffset; src (compile-time) 1 = the stage reads x2
    auto issue = [&](auto src, int buf, int s) {
        float* st = smem + buf * RING_STAGE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            lds_void* da = (lds_void*)(st + (4 * u + wave) * 256);
            if constexpr (DUAL && decltype(src)::value == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(xr2, da, 16, aoff2[u], (unsigned)(s - S1) * 64u, 0, 0);
            else                                             __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, da, 16, aoff[u], (unsigned)s * 64u, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void*)(st + 128 * RING_BK + (4 * u + wave) * 256), 16, boff[u], (unsigned)s * 64u, 0, 0);
    };

    // ---- fragments: row frow (+ 32 i) of the wave's 64, logical chunk 2g + h, at position (2g + h) ^ ((frow >> 2) & 3)
    const int frow = lane & 31, h = lane >> 5;
    const int fsw = (frow >> 2) & 3;
    const float* Ard[2];
    const float* Brd[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        Ard[g] = smem + (wm * 64 + frow) * RING_BK + (((2 * g + h) ^ fsw) << 2);
        Brd[g] = smem + 128 * RING_BK + (wn * 64 + frow) * RING_BK + (((2 * g + h) ^ fsw) << 2);
    }

    // ---- epilogue operands, requested up front (scale / bias) or two stages before the end (residual)
    const unsigned rowb = (unsigned)p.Cout * 4u;
    const unsigned ylane = (unsigned)(m0 + wm * 64 + 4 * h) * rowb + (unsigned)(n0 + wn * 64 + frow) * 4u;   // acc element e of tile (i, j): + row (32 i + (e & 3) + 8 (e >> 2)), + 128 j bytes
    float sc[2], bi[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + frow;
        sc[j] = p.scale ? p.scale[n] : 1.f;
        bi[j] = p.bias ? p.bias[n] : 0.f;
    }
    const __amdgpu_buffer_rsrc_t yr = buf_rsrc(p.y, p.y_bytes);
    const __amdgpu_buffer_rsrc_t rr = buf_rsrc(RES ? p.res : p.y, RES ? p.y_bytes : 0u);
    float rs[2][2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) rs[i][j][e] = 0.f;
    auto res_load = [&](int i) {                  // 32 loads: the residual of row half i
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                rs[i][j][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                  rr, ylane + (unsigned)(32 * i + (e & 3) + 8 * (e >> 2)) * rowb + (unsigned)j * 128u, 0, 0));
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // One stage.  KIND 0: steady state (stages s+1, s+2 in flight behind s: vmcnt(8)), then the request of stage s+3 into the
    // slot every wave finished reading before this barrier (stage s-1's); 1: s = S-3, requests the residual's first row half
    // instead; 2: s = S-2 (stage S-1 and that half younger); 3: s = S-1 (only that half younger), requests the second half.
    // VMEM operations retire in order, so each count waits for this wave's pieces of stage s exactly.
    auto stage = [&](auto slot, auto kind, auto src, int s) {
        constexpr int B = decltype(slot)::value, KIND = decltype(kind)::value;
        if constexpr (KIND <= 1) ring_wait_vm<8>();
        else if constexpr (KIND == 2) ring_wait_vm<RES ? 36 : 4>();
        else ring_wait_vm<RES ? 32 : 0>();
        __builtin_amdgcn_s_barrier();             // every wave's pieces of stage s have landed; every wave is done reading slot (s - 1) % 4
        asm volatile("" ::: "memory");
        f32x4 af[2][2], bf[2][2];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[g][i] = *reinterpret_cast<const f32x4*>(Ard[g] + B * RING_STAGE + i * 32 * RING_BK);
                bf[g][i] = *reinterpret_cast<const f32x4*>(Brd[g] + B * RING_STAGE + i * 32 * RING_BK);
            }
        if constexpr (KIND == 0) issue(src, (B + 3) & 3, s + 3);
        if constexpr (RES && KIND == 1) res_load(0);
        if constexpr (RES && KIND == 3) res_load(1);
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g][i][tt], bf[g][j][tt], acc[i][j], 0, 0, 0);
        // pin the order: both groups' fragment reads first (separate registers: the second group's reads must not wait for the
        // first group's MFMAs), then the four DMA requests one behind each of the first MFMAs, then the rest of the MFMAs
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
        if constexpr (KIND == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 28, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    using C0 = std::integral_constant<int, 0>;
    using C1 = std::integral_constant<int, 1>;
    using C2 = std::integral_constant<int, 2>;
    using C3 = std::integral_constant<int, 3>;

    using X2 = std::integral_constant<int, DUAL ? 1 : 0>;   // source of the stages past S1 (x itself for the plain form)
    auto group = [&](auto src, int s) {           // four steady-state stages whose requests all read one source
        stage(C0{}, C0{}, src, s);
        stage(C1{}, C0{}, src, s + 1);
        stage(C2{}, C0{}, src, s + 2);
        stage(C3{}, C0{}, src, s + 3);
    };

    issue(C0{}, 0, 0);                            // (S1 >= 4: the first three stages read x)
    issue(C0{}, 1, 1);
    issue(C0{}, 2, 2);
    int s = 0;
    if constexpr (DUAL) {
        for (; s < S1 - 4; s += 4) group(C0{}, s);
        stage(C0{}, C0{}, C0{}, s);               // the group whose requests cross from x to x2 (S1 - 1 | S1 .. S1 + 2)
        stage(C1{}, C0{}, X2{}, s + 1);
        stage(C2{}, C0{}, X2{}, s + 2);
        stage(C3{}, C0{}, X2{}, s + 3);
        s += 4;
    }
    for (; s < S - 4; s += 4) group(X2{}, s);
    stage(C0{}, C0{}, X2{}, s);                   // the last group: requests the last stage, then the residual
    stage(C1{}, C1{}, X2{}, s + 1);
    stage(C2{}, C2{}, X2{}, s + 2);
    stage(C3{}, C3{}, X2{}, s + 3);

    // ---- write-out from the accumulator layout: element e of tile (i, j) is row 32 i + (e & 3) + 8 (e >> 2) + 4 h, channel
    // 64 wn + 32 j + frow; rows >= M lie past the descriptor (dropped).  Same arithmetic as conv_epilogue.
    const float lo = p.relu ? 0.f : -INFINITY;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float v = fmaxf(acc[i][j][e] * sc[j] + bi[j] + rs[i][j][e], lo);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yr,
                                                      ylane + (unsigned)(32 * i + (e & 3) + 8 * (e >> 2)) * rowb + (unsigned)j * 128u, 0, 0);
            }
}

template <bool DUAL, bool RES>
__global__ __launch_bounds__(256, 2) void gemm1x1_ring_kernel(ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    gemm1x1_ring_body<DUAL, RES>(p, smem);
}

static std::atomic<int> g_ring{1};     // LDS-DMA ring kernel for the long-K 1x1 layers; 0 = off: vatl_tune_set(27, 0), profiling variant only (same-box A/B)
int ring_set_enable(int v) { g_ring.store(v, std::memory_order_relaxed); return 0; }

template <bool DUAL, bool RES>
static int launch_ring_impl(const ConvParams& p, hipStream_t st) {
    auto kern = gemm1x1_ring_kernel<DUAL, RES>;
    static std::atomic<unsigned> configured{0};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), RING_BYTES, configured, "gemm1x1_ring")) return rc;
    ConvParams q = p;
    q.n_tiles = p.CoutPad / 128;
    q.m_tiles = cdiv(p.M, 128);
    q.splits = 1;
    hipLaunchKernelGGL(kern, dim3((unsigned)(q.m_tiles * q.n_tiles)), dim3(256), RING_BYTES, st, q);
    meter_add(0, 2.0 * ((double)q.m_tiles * 128) * ((double)q.n_tiles * 128) * ((double)q.ktiles * BK));
    meter_route(kRouteGemm1x1Ring);
    return check_launch("gemm1x1_ring");
}

int launch_ring(const ConvParams& p, hipStream_t st) {
    if (p.x2) return launch_ring_impl<true, false>(p, st);           // (the dual form has no residual: ring_wanted)
    return p.res ? launch_ring_impl<false, true>(p, st) : launch_ring_impl<false, false>(p, st);
}

// The ring kernel serves whole 128 x 128 tiles of a stride-1 1x1 layer (or the dual-source form) with K a multiple of 64 and at least
// 16 k-tiles (12 for the dual form, whose x / x2 boundary falls on a multiple of 64 channels), NHWC output, Cout == CoutPad, no training epilogue (statistics / BatchNorm backward) and no
// split-K workspace; (M + 128) * Cout < 2^30 so that the byte offsets of the tail tile's dropped rows do not wrap.  Default schedule only
// (knob 0 = 4: the other schedules keep the tiled kernel).  The fine-tune step's data-gradient launches without a BatchNorm-backward
// epilogue are plain 1x1 GEMMs as well and take it where their shape qualifies (same bits).
bool ring_wanted(const ConvParams& p, int phases, int bn, int bm, int var) {
    if (!g_ring.load(std::memory_order_relaxed) || var != 4 || phases != 1 || bn != 128 || bm != 128) return false;
    if (p.R != 1 || p.S != 1 || p.stride != 1 || p.pad_y || p.pad_x || p.out_nchw || p.deconv || p.stats || p.bz) return false;
    if (p.osy != 1 || p.osx != 1 || p.OH != p.Ho || p.OW != p.Wo || p.H != p.Ho || p.W != p.Wo) return false;
    if (p.Cout != p.CoutPad || (p.ktiles & 1) || p.ktiles < (p.x2 ? 12 : 16)) return false;
    // dual form: the x / x2 boundary on a whole group of four stages, at least one group of each source (the prologue's three stages
    // read x), no residual (vatl_conv1x1_dual_fwd has none)
    if (p.x2 && (p.res || p.k1 < 2 || (p.k1 & 1) || p.ktiles - p.k1 < 2)) return false;
    if ((long long)(p.M + 128) * p.Cout >= (1LL << 30)) return false;
    long long ws_floats = 0;
    int sk_policy = 0;
    return splitk_workspace(&ws_floats, &sk_policy) == nullptr;
}

}  // namespace vatl
