// What the implicit-GEMM translation units share: the launch parameters, the tile constants, the tile write-out and the host
// functions the dispatcher (conv_igemm.hip) calls across files.  
#pragma once
#include "common.h"
#include "buffer.h"
#include "bn_epilogue.h"

namespace vatl {

struct ConvParams {
    const float* x;
    const float* w;
    const float* scale;
    const float* bias;
    const float* res;
    float* y;
    int N, H, W, Cin;
    int Cout, CoutPad;
    int R, S, stride, pad_y, pad_x;
    int Ho, Wo, M;
    int OH, OW, osy, osx, ooy, oox;   // output pixel = (oy*osy+ooy, ox*osx+oox) in an OH x OW image
    int relu, out_nchw, deconv;
    int kpr;                          // k-tiles per filter tap  (Cin/32; 1 for the stem)
    int ktiles;                       // total k-tiles
    int n_tiles, m_tiles;
    int order;                        // tile order inside an XCD's run: 0 n-tile fastest, 1 m-tile fastest
    int stagger;                      // start the second resident block of every CU half a block-time late
    int K;                            // packed K per output channel
    double* stats;                    // training: per (row block, channel) partial (sum, sum^2) of the stored tile, or NULL
    // BatchNorm-backward fusion (data-gradient launches of the fine-tune step): the tile being stored is dL/dy of a
    // Conv+BN(+ReLU) layer whose conv output is bz (same NHWC layout as y).  The epilogue applies that layer's ReLU mask
    // (bmy > 0 if given, else bz*bsc+bbi > 0 if bsc is given, else none), stores g = masked gradient and accumulates the
    // per-channel (sum g, sum g*xhat), xhat = (bz - bmu)*bis, into `stats` — the reduction pass of the BN backward.
    const float* bz;
    const float* bmy;
    const float* bsc;
    const float* bbi;
    const float* bmu;
    const float* bis;
    // dual-source 1x1 (projection shortcut fused into the block's last conv): k-tiles 0..k1-1 read x (C1 = Cin channels,
    // one row per output pixel), k-tiles k1.. read x2 (C2 channels, an H2 x W2 image sampled with stride2)
    const float* x2;
    int k1, C2, H2, W2, stride2;
    unsigned x2_bytes;
    int ablate;                       // profiling only (vatl_tune_set(6, bits), wrong results): 1 = no epilogue
    // opt-in split-K (small batches): blockIdx.z owns k-tiles [z*kt_per_split, ...) and writes a raw partial tile into
    // its slice of `part` (output layout of y, NHWC); splitk_reduce_kernel sums the slices in order and applies the epilogue
    int splits, kt_per_split;
    float* part;
    long long part_slice;
    unsigned x_bytes, w_bytes, y_bytes;   // buffer extents (hardware bounds checks: OOB loads read 0, OOB stores drop)
    FastDivU d_HoWo, d_Wo;                // m -> (image, row, column) without integer divisions (common.h: fdiv; filled in by dispatch())
};

constexpr int BK = 32;
constexpr int LDK = BK;               // LDS row = one k-tile; chunk positions XOR-swizzled (conv_igemm.hip's introduction)
// dynamic LDS of a BM x BN block: the two k-loop stages, or the epilogue's output tile if that is larger
constexpr int conv_smem_floats(int BM, int BN) { return 2 * (BM + BN) * LDK > BM * (BN + 4) ? 2 * (BM + BN) * LDK : BM * (BN + 4); }
constexpr unsigned OOB = 0xFFFFFFFFu; // byte offset guaranteed outside any descriptor of these kernels

// Epilogue shared by the conv kernels: scale/bias in registers, tile staged through LDS, then full-row 16-byte
// stores with the residual read the same way (or per-element stores for NCHW / odd channel counts).
template <int BM, int BN, int WM, int WN, int NT = 256, bool BNB = false>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, f32x16 (&acc)[WM / 32][WN / 32], float* smem, int m0, int n0,
                                              int ooy, int oox, int wm, int wn, int tid, int lane, int HoWo) {
    constexpr int TM = WM / 32, TN = WN / 32;
    // ---- epilogue -------------------------------------------------------------
    // 1. scale/bias in registers, tile -> LDS (the staging buffers are free after the
    //    loop's last barrier).  D[row = (e&3) + 8*(e>>2) + 4*(lane>>5)][col = lane&31].
    constexpr int LDC = BN + 4;
    float* Cs = smem;
    // 0. output offsets of this thread's float4 columns and the residual tile, requested BEFORE the LDS
    //    transpose so that its HBM latency hides behind the accumulator write-out and the barrier
    const __amdgpu_buffer_rsrc_t yr = buf_rsrc(p.y, p.y_bytes);
    const __amdgpu_buffer_rsrc_t rr = buf_rsrc(p.res, p.res ? p.y_bytes : 0u);
    const int OHW = p.OH * p.OW;
    const bool plain = !p.deconv && p.osy == 1 && p.osx == 1 && p.OH == p.Ho && p.OW == p.Wo;   // NHWC output row index == m
    const bool vec = !p.out_nchw && (p.Cout & 3) == 0;
    constexpr int C4 = BN / 4;                         // float4 columns per tile row
    constexpr int RPP = NT / C4;                       // tile rows per pass
    constexpr int NP = BM / RPP;                       // passes
    unsigned offv[NP];
    f32x4 rsv[NP];
    if (vec) {
        const int c4 = tid % C4, r0 = tid / C4;
        const int n = n0 + c4 * 4;
        const bool nv = n < p.Cout;
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int m = m0 + r0 + u * RPP;
            int orow = m;
            if (!plain) {
                const int b = fdiv(m, p.d_HoWo);
                const int rem = m - b * HoWo;
                const int oy = fdiv(rem, p.d_Wo);
                const int ox = rem - oy * p.Wo;
                orow = b * OHW + (oy * p.osy + ooy) * p.OW + (ox * p.osx + oox);
            }
            offv[u] = (nv && m < p.M) ? (unsigned)(orow * p.Cout + n) << 2 : OOB;
        }
        if (p.res) {
#pragma unroll
            for (int u = 0; u < NP; ++u) rsv[u] = buf_load4(rr, offv[u]);
        } else {
#pragma unroll
            for (int u = 0; u < NP; ++u) rsv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int cl = wn * WN + j * 32 + (lane & 31);
        const int n = n0 + cl;
        const bool nv = n < p.Cout;
        const float sc = (nv && p.scale) ? p.scale[n] : 1.f;
        const float bi = (nv && p.bias) ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wm * WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                Cs[row * LDC + cl] = acc[i][j][e] * sc + bi;
            }
    }
    __syncthreads();

    // 2. LDS -> HBM with full rows: (+ residual) (ReLU), branch-free through descriptors
    const float lo = p.relu ? 0.f : -INFINITY;
    if (vec) {
        const int c4 = tid % C4, r0 = tid / C4;
        f32x4 ssum = {0.f, 0.f, 0.f, 0.f}, ssq = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BNB) {
            // BatchNorm-backward fusion (separate instantiations: the extra tile of z / mask registers must not cost the
            // inference kernels their occupancy): mask the gradient tile with the consumer layer's ReLU, store g, reduce (g, g*xhat)
            const __amdgpu_buffer_rsrc_t zr = buf_rsrc(p.bz, p.y_bytes);
            const __amdgpu_buffer_rsrc_t mr = buf_rsrc(p.bmy, p.bmy ? p.y_bytes : 0u);
            const int n = n0 + c4 * 4;
            const bool nv = n < p.Cout;                    // Cout % 4 == 0 on this path: the float4 is in range or entirely out
            // (bn_epilogue.h's bn_consts, kept as text here: through the function the 128x32 instantiation spills 6 instead of 2 scalar registers)
            const f32x4 one = {1.f, 1.f, 1.f, 1.f}, nul = {0.f, 0.f, 0.f, 0.f};
            const f32x4 mu = nv ? *reinterpret_cast<const f32x4*>(p.bmu + n) : nul, is = nv ? *reinterpret_cast<const f32x4*>(p.bis + n) : nul;
            const f32x4 msc = (nv && p.bsc) ? *reinterpret_cast<const f32x4*>(p.bsc + n) : nul;
            const f32x4 mbi = (nv && p.bsc) ? *reinterpret_cast<const f32x4*>(p.bbi + n) : one;   // no mask: 0*z + 1 > 0
            f32x4 zt[NP], yt[NP];
#pragma unroll
            for (int u = 0; u < NP; ++u) zt[u] = buf_load4(zr, offv[u]);
            if (p.bmy) {
#pragma unroll
                for (int u = 0; u < NP; ++u) yt[u] = buf_load4(mr, offv[u]);
            }
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&Cs[(r0 + u * RPP) * LDC + c4 * 4]);
                // (bn_epilogue.h's bn_masked_grad, kept as text here: through the function the 128x128 instantiation takes 243 instead of 238 VGPRs
                // and its 1024 -> 256 data gradient at 120 crops measured 1.7 % slower; the bit fixture pins that the product below fuses into the sum)
                f32x4 g;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = v[c] + rsv[u][c];
                    const bool on = p.bmy ? yt[u][c] > 0.f : relu_on(zt[u][c], msc[c], mbi[c]);
                    g[c] = on ? d : 0.f;
                    ssum[c] += g[c];
                    ssq[c] += g[c] * ((zt[u][c] - mu[c]) * is[c]);       // rows >= M: d = 0 exactly
                }
                buf_store4(yr, offv[u], g);
            }
        } else {
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(&Cs[(r0 + u * RPP) * LDC + c4 * 4]);
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = fmaxf(v[c] + rsv[u][c], lo);
            buf_store4(yr, offv[u], o);
            if (p.stats) fold_stats(ssum, ssq, o);     // rows >= M hold exact zeros
        }
        }
        if (p.stats) {
            // BatchNorm batch statistics of the tile just stored (training forward): per-thread fp32 sums over NP rows,
            // combined over the RPP row groups in double, one (sum, sum^2) pair per (row block, channel) — the layout
            // bn_train_finalize_kernel reduces in a fixed order (deterministic, no atomics).
            // (every thread is done reading Cs once it is past the combine's first barrier)
            stats_block_store<NT, C4>(smem, tid, ssum, ssq, p.stats, (long long)blockIdx.y, p.m_tiles, m0 / BM, n0, p.Cout);
        }
    } else {
        // NCHW output (heat-map head) or a channel count that is not a multiple of 4:
        // one tile row per thread, lanes run along pixels (contiguous in NCHW)
        constexpr int CPP = NT / BM;                   // tile columns per pass
        const int row = tid % BM, cl0 = tid / BM;
        const int m = m0 + row;
        const bool mv = m < p.M;
        const int b = fdiv(m, p.d_HoWo);
        const int rem = m - b * HoWo;
        const int oy = fdiv(rem, p.d_Wo);
        const int ox = rem - oy * p.Wo;
        const int opix = (oy * p.osy + ooy) * p.OW + (ox * p.osx + oox);
        const int nstride = p.out_nchw ? OHW : 1;
        const int obase = p.out_nchw ? b * p.Cout * OHW + opix : (b * OHW + opix) * p.Cout;
        if (p.res) {
#pragma unroll 4
            for (int ps = 0; ps < BN / CPP; ++ps) {
                const int cl = cl0 + ps * CPP;
                const int n = n0 + cl;
                const unsigned off = (mv && n < p.Cout) ? (unsigned)(obase + n * nstride) << 2 : OOB;
                buf_store1(yr, off, fmaxf(Cs[row * LDC + cl] + buf_load1(rr, off), lo));
            }
        } else {
#pragma unroll 8
            for (int ps = 0; ps < BN / CPP; ++ps) {
                const int cl = cl0 + ps * CPP;
                const int n = n0 + cl;
                const unsigned off = (mv && n < p.Cout) ? (unsigned)(obase + n * nstride) << 2 : OOB;
                buf_store1(yr, off, fmaxf(Cs[row * LDC + cl], lo));
            }
        }
    }
}

// Host functions between the implicit-GEMM files (hidden visibility, C++ linkage: not part of the C ABI).  Each kernel family's
// file holds its kernels, its launcher, the knob it owns (tune.h) and the gate dispatch() asks, in dispatch()'s order.
#pragma GCC visibility push(hidden)
float* splitk_workspace(long long* floats, int* policy);                                  // conv_igemm.hip
int igemm_ablate_bits();                                                                  // conv_igemm.hip (knob 6; read by the profiling variant only)
bool streamk_wanted(const ConvParams& p, int phases, int bn, int bm, bool stem);          // conv_streamk.hip
template <bool BNB>
int launch_streamk(const ConvParams& p, hipStream_t st);
bool persistent_wanted(const ConvParams& p, int phases, int bn, int var);                 // gemm1x1_persistent.h (in conv_igemm.hip's unit)
int launch_persistent(const ConvParams& p, hipStream_t st);
bool ring_wanted(const ConvParams& p, int phases, int bn, int bm, int var);               // gemm1x1_ring.hip
int launch_ring(const ConvParams& p, hipStream_t st);
#pragma GCC visibility pop

}  // namespace vatl
