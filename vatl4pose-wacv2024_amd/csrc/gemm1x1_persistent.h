// The persistent 1x1 GEMM family: both kernels, their launcher, knobs 7 and 10 and the gate dispatch() asks.
//
// This file is part of conv_igemm.hip's translation unit (included there, after conv_igemm_kernel), not one of its own: compiled
// alone, both kernels come out with a different instruction schedule and register assignment (hipcc 7.2: the
// optimised IR already differs in how the addresses off vatl::smem are formed, the one dynamic-LDS symbol that all kernels of a
// unit share, so these two depend on that symbol's other users).  The other kernel families keep their code in files of their own; tools/kernel_isa.py
// is the check.  Nothing here relies on being in that unit: the interface is conv_igemm.h / tune.h, as for the other families.
#pragma once
#include "conv_igemm.h"
#include "tune.h"

namespace vatl {

// ---------------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------------
// Persistent 1x1 / stride-1 kernel (a plain GEMM Y[M][N] = A[M][K] W[N][K]^T with the conv epilogue).
// The short-K 1x1 layers (conv3 / conv1 of the bottlenecks, K = 64..512) spend as long in the prologue (first
// operand loads with nothing to overlap) and in the tile write-out as in their 2-16 k-tiles (profiles/r01_notes.md,
// ablation knob 6).  Here a block stays resident, walks a run of tiles and requests the NEXT tile's first operand
// tile before the current tile's epilogue, so that latency and the write-out overlap.  Same LDS layout, fragment
// mapping, MFMA order and epilogue as conv_igemm_kernel: results are bit-identical.
// ---------------------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void gemm1x1_persistent_kernel(ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                          // [2][BM][LDK]
    float* Bs = smem + 2 * BM * LDK;           // [2][BN][LDK]
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    constexpr int LA = BM / 32, LB = BN / 32;
    constexpr int NG = BK / 8, MPG = 4 * TM * TN;
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves per block");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int lrow = tid >> 3, kq = tid & 7;
    const int wpos = (kq ^ ((lrow >> 1) & 7)) * 4;
    const int frow = lane & 31;
    int koff[BK / 8];
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) koff[g] = ((2 * g + (lane >> 5)) ^ ((frow >> 1) & 7)) * 4;
    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t wr = buf_rsrc(p.w, p.w_bytes);

    // XCD-aware runs: XCD x (= block id mod 8) owns tiles [x*per, (x+1)*per) in n-fastest order; its blocks walk the run
    // with a stride of (blocks per XCD), so the blocks that share an activation panel are on the same L2 at the same time
    const int total = p.m_tiles * p.n_tiles;
    const int per = (total + 7) >> 3, bpx = gridDim.x >> 3;
    const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int run_end = min((xcd + 1) * per, total);
    int t = xcd * per + loc;
    if (t >= run_end) return;

    unsigned aoff[LA], boff[LB];               // byte offsets of this thread's float4s at k-tile 0
    int m0, n0;
    auto setup = [&](int tile, unsigned (&ao)[LA], unsigned (&bo)[LB], int& mm0, int& nn0) {
        const int m_tile = tile / p.n_tiles, n_tile = tile - m_tile * p.n_tiles;
        mm0 = m_tile * BM; nn0 = n_tile * BN;
#pragma unroll
        for (int i = 0; i < LA; ++i) ao[i] = (unsigned)(((mm0 + lrow + 32 * i) * p.K + kq * 4) * 4);   // rows >= M: past the descriptor -> zeros
#pragma unroll
        for (int j = 0; j < LB; ++j) bo[j] = (unsigned)(((nn0 + lrow + 32 * j) * p.K + kq * 4) * 4);
    };
    f32x4 ra[LA], rb[LB];
    auto gload = [&](const unsigned (&ao)[LA], const unsigned (&bo)[LB], int kt, bool live) {
#pragma unroll
        for (int i = 0; i < LA; ++i) ra[i] = buf_load4(xr, live ? ao[i] + (unsigned)kt * (BK * 4) : OOB);
#pragma unroll
        for (int j = 0; j < LB; ++j) rb[j] = buf_load4(wr, live ? bo[j] + (unsigned)kt * (BK * 4) : OOB);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < LA; ++i) *reinterpret_cast<f32x4*>(&As[(buf * BM + lrow + 32 * i) * LDK + wpos]) = ra[i];
#pragma unroll
        for (int j = 0; j < LB; ++j) *reinterpret_cast<f32x4*>(&Bs[(buf * BN + lrow + 32 * j) * LDK + wpos]) = rb[j];
    };
    auto frag_read = [&](f32x4 (&af)[TM], f32x4 (&bf)[TN], int buf, int g) {
        const float* Ab = As + (buf * BM + wm * WM + frow) * LDK + koff[g];
        const float* Bb = Bs + (buf * BN + wn * WN + frow) * LDK + koff[g];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * LDK);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * LDK);
    };

    setup(t, aoff, boff, m0, n0);
    gload(aoff, boff, 0, true);
    lstore(0);
    __syncthreads();
    const int HoWo = p.Ho * p.Wo;
    for (;;) {
        f32x16 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        f32x4 af[2][TM], bf[2][TN];
        for (int kt = 0; kt < p.ktiles; ++kt) {
            const int buf = kt & 1;
            const bool live = kt + 1 < p.ktiles;
            frag_read(af[0], bf[0], buf, 0);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g + 1 < NG) frag_read(af[(g + 1) & 1], bf[(g + 1) & 1], buf, g + 1);
                if (g == 0) gload(aoff, boff, kt + 1, live);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g & 1][i][tt], bf[g & 1][j][tt], acc[i][j], 0, 0, 0);
                if (g + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
#pragma unroll
                for (int q = 0; q < MPG; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x016, 2, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (live) lstore(buf ^ 1);
            __syncthreads();
        }
        // request the next tile's first operand tile: in flight during this tile's epilogue
        const int tn = t + bpx;
        const bool more = tn < run_end;
        unsigned aoffn[LA], boffn[LB];
        int m0n = 0, n0n = 0;
        if (more) { setup(tn, aoffn, boffn, m0n, n0n); gload(aoffn, boffn, 0, true); }
        conv_epilogue<BM, BN, WM, WN>(p, acc, smem, m0, n0, 0, 0, wm, wn, tid, lane, HoWo);
        if (!more) break;
        __syncthreads();                       // every thread is done with the epilogue's LDS tile
        lstore(0);
        __syncthreads();
        t = tn; m0 = m0n; n0 = n0n;
#pragma unroll
        for (int i = 0; i < LA; ++i) aoff[i] = aoffn[i];
#pragma unroll
        for (int j = 0; j < LB; ++j) boff[j] = boffn[j];
    }
}

// The same persistent GEMM with a DISTANCE-2 operand stream that runs across tile boundaries.  With K = 64 .. 256 a tile has only
// 2 .. 8 k-tiles; with one k-tile of look-ahead every one of them waits for an HBM round trip that 4096 matrix-pipe cycles do
// not cover, and the pipe idles (l2.n.c3, K = 128: 61 % of peak at 3.4 TB/s — neither roof).  Here two staging register sets
// alternate: while k-tile kt is multiplied, k-tile kt+1 sits in registers waiting to be written to LDS and k-tile kt+2 is being
// requested — and "kt+2" simply continues into the NEXT tile's first two k-tiles, which therefore are in flight during the
// whole epilogue of the current tile.  Requires an even number of k-tiles (statically indexed register sets).  Same LDS
// layout, fragment mapping, MFMA order and epilogue: bit-identical to the other two kernels.
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void gemm1x1_persistent2_kernel(ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                          // [2][BM][LDK]
    float* Bs = smem + 2 * BM * LDK;           // [2][BN][LDK]
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    constexpr int LA = BM / 32, LB = BN / 32;
    constexpr int NG = BK / 8, MPG = 4 * TM * TN;
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves per block");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int lrow = tid >> 3, kq = tid & 7;
    const int wpos = (kq ^ ((lrow >> 1) & 7)) * 4;
    const int frow = lane & 31;
    int koff[BK / 8];
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) koff[g] = ((2 * g + (lane >> 5)) ^ ((frow >> 1) & 7)) * 4;
    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t wr = buf_rsrc(p.w, p.w_bytes);

    const int total = p.m_tiles * p.n_tiles;
    const int per = (total + 7) >> 3, bpx = gridDim.x >> 3;
    const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int run_end = min((xcd + 1) * per, total);
    int t = xcd * per + loc;
    if (t >= run_end) return;

    unsigned aoff[LA], boff[LB];               // byte offsets of this thread's float4s at k-tile 0
    int m0, n0;
    auto setup = [&](int tile, unsigned (&ao)[LA], unsigned (&bo)[LB], int& mm0, int& nn0) {
        const int m_tile = tile / p.n_tiles, n_tile = tile - m_tile * p.n_tiles;
        mm0 = m_tile * BM; nn0 = n_tile * BN;
#pragma unroll
        for (int i = 0; i < LA; ++i) ao[i] = (unsigned)(((mm0 + lrow + 32 * i) * p.K + kq * 4) * 4);   // rows >= M: past the descriptor -> zeros
#pragma unroll
        for (int j = 0; j < LB; ++j) bo[j] = (unsigned)(((nn0 + lrow + 32 * j) * p.K + kq * 4) * 4);
    };
    f32x4 sa[2][LA], sb[2][LB];
    auto issue = [&](f32x4 (&da)[LA], f32x4 (&db)[LB], const unsigned (&ao)[LA], const unsigned (&bo)[LB], int kt, bool live) {
#pragma unroll
        for (int i = 0; i < LA; ++i) da[i] = buf_load4(xr, live ? ao[i] + (unsigned)kt * (BK * 4) : OOB);
#pragma unroll
        for (int j = 0; j < LB; ++j) db[j] = buf_load4(wr, live ? bo[j] + (unsigned)kt * (BK * 4) : OOB);
    };
    auto stash = [&](const f32x4 (&da)[LA], const f32x4 (&db)[LB], int buf) {
#pragma unroll
        for (int i = 0; i < LA; ++i) *reinterpret_cast<f32x4*>(&As[(buf * BM + lrow + 32 * i) * LDK + wpos]) = da[i];
#pragma unroll
        for (int j = 0; j < LB; ++j) *reinterpret_cast<f32x4*>(&Bs[(buf * BN + lrow + 32 * j) * LDK + wpos]) = db[j];
    };
    auto frag_read = [&](f32x4 (&af)[TM], f32x4 (&bf)[TN], int buf, int g) {
        const float* Ab = As + (buf * BM + wm * WM + frow) * LDK + koff[g];
        const float* Bb = Bs + (buf * BN + wn * WN + frow) * LDK + koff[g];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * LDK);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * LDK);
    };

    setup(t, aoff, boff, m0, n0);
    issue(sa[0], sb[0], aoff, boff, 0, true);
    stash(sa[0], sb[0], 0);
    issue(sa[0], sb[0], aoff, boff, 1, true);          // ktiles >= 2
    __syncthreads();
    const int HoWo = p.Ho * p.Wo;
    const int KT = p.ktiles;
    for (;;) {
        f32x16 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        const int tn = t + bpx;
        const bool more = tn < run_end;
        unsigned aoffn[LA], boffn[LB];
        int m0n = 0, n0n = 0;
        setup(more ? tn : t, aoffn, boffn, m0n, n0n);
        f32x4 af[2][TM], bf[2][TN];
        // one k-tile: fragment reads + 64 MFMAs on LDS buffer `buf`, the request of a later k-tile in the first group's shadow,
        // the write of the waiting register set to the other buffer in the last group's
        auto ktile = [&](int buf, auto&& request, auto&& write_back) {
            frag_read(af[0], bf[0], buf, 0);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g + 1 < NG) frag_read(af[(g + 1) & 1], bf[(g + 1) & 1], buf, g + 1);
                if (g == 0) request();
                if (g == NG - 1) write_back();
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g & 1][i][tt], bf[g & 1][j][tt], acc[i][j], 0, 0, 0);
                if (g + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
#pragma unroll
                for (int q = 0; q < MPG; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x216, 2, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
        };
        for (int kt = 0; kt < KT; kt += 2) {
            const bool in_tile = kt + 2 < KT;              // k-tiles kt+2, kt+3 belong to this tile; else: the next tile's first two
            ktile(0, [&] { if (in_tile) issue(sa[1], sb[1], aoff, boff, kt + 2, true); else issue(sa[1], sb[1], aoffn, boffn, 0, more); },
                  [&] { stash(sa[0], sb[0], 1); });
            ktile(1, [&] { if (in_tile) issue(sa[0], sb[0], aoff, boff, kt + 3, true); else issue(sa[0], sb[0], aoffn, boffn, 1, more); },
                  [&] { if (in_tile) stash(sa[1], sb[1], 0); });
        }
#ifdef VATL_ABLATION
        if (p.ablate & 1) {                    // profiling build only: keep the accumulators alive, skip the write-out
            float sacc = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) sacc += acc[i][j][e];
            if (sacc == 12345.678f) p.y[0] = sacc;
        } else
#endif
        conv_epilogue<BM, BN, WM, WN>(p, acc, smem, m0, n0, 0, 0, wm, wn, tid, lane, HoWo);
        if (!more) break;
        __syncthreads();                       // every thread is done with the epilogue's LDS tile
        stash(sa[1], sb[1], 0);                // the next tile's k-tile 0 (requested two k-tiles ago); its k-tile 1 waits in set 0
        __syncthreads();
        t = tn; m0 = m0n; n0 = n0n;
#pragma unroll
        for (int i = 0; i < LA; ++i) aoff[i] = aoffn[i];
#pragma unroll
        for (int j = 0; j < LB; ++j) boff[j] = boffn[j];
    }
}

static std::atomic<int> g_persist_dist{2};   // vatl_tune_set(10, v): operand look-ahead of the persistent 1x1 kernel (1 or 2 k-tiles)
int persistent_set_dist(int v) { g_persist_dist.store(v, std::memory_order_relaxed); return 0; }

template <int BM, int BN, int WM, int WN, bool D2>
static int launch_persistent_impl(const ConvParams& p, hipStream_t st) {
    auto kern = gemm1x1_persistent_kernel<BM, BN, WM, WN>;
    auto kern2 = gemm1x1_persistent2_kernel<BM, BN, WM, WN>;
    constexpr int smem = conv_smem_floats(BM, BN) * (int)sizeof(float);
    static std::atomic<unsigned> configured{0};
    if (int rc = ensure_dynamic_lds(D2 ? reinterpret_cast<const void*>(kern2) : reinterpret_cast<const void*>(kern), smem, configured, "gemm1x1_persistent")) return rc;
    ConvParams q = p;
    q.n_tiles = p.CoutPad / BN;
    q.m_tiles = cdiv(p.M, BM);
    const int total = q.m_tiles * q.n_tiles;
    int grid = 512;                            // two resident blocks per CU
    if (grid > total) grid = (total + 7) / 8 * 8;
#ifdef VATL_ABLATION
    q.ablate = igemm_ablate_bits();
    if (q.ablate & 4) q.y_bytes = 0;           // every output store (and residual load) out of range: dropped, no HBM writes
    if (q.ablate & 8) q.x_bytes = 0;           // every activation load out of range: zeros, no HBM reads
    if ((q.ablate & 2) && q.ktiles > 2) { q.ktiles = 2; }
#endif
    if (D2) hipLaunchKernelGGL(kern2, dim3((unsigned)grid), dim3(256), smem, st, q);
    else    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), smem, st, q);
    meter_add(0, 2.0 * ((double)q.m_tiles * BM) * ((double)q.n_tiles * BN) * ((double)q.ktiles * BK));
    meter_route(kRoutePersistent1x1);
    return check_launch("gemm1x1_persistent");
}

int launch_persistent(const ConvParams& p, hipStream_t st) {
    const bool d2 = g_persist_dist.load(std::memory_order_relaxed) == 2 && p.ktiles >= 2 && (p.ktiles & 1) == 0;
    return d2 ? launch_persistent_impl<128, 128, 64, 64, true>(p, st) : launch_persistent_impl<128, 128, 64, 64, false>(p, st);
}

static std::atomic<int> g_persist{1};  // vatl_tune_set(7, v): persistent kernel for 1x1 layers with K <= 256 v (0 = off)
int persistent_set_kmax(int v) { g_persist.store(v, std::memory_order_relaxed); return 0; }

// short-K 1x1 / stride-1 layers on whole 128x128 tiles (dispatch() asks after it has sent the 64-row tiles elsewhere)
bool persistent_wanted(const ConvParams& p, int phases, int bn, int var) {
    const int pk = g_persist.load(std::memory_order_relaxed);
    return pk && bn == 128 && var == 4 && phases == 1 && p.R == 1 && p.S == 1 && p.stride == 1 && p.pad_y == 0 && !p.out_nchw && !p.deconv &&
           p.osy == 1 && p.osx == 1 && p.OH == p.Ho && p.OW == p.Wo && (p.Cout & 3) == 0 && p.ktiles <= pk * 8 && !p.x2 &&
           (long long)(p.M + 128) * p.K < (1LL << 30);
}

}  // namespace vatl
