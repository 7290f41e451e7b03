// Tail of one bottleneck and head of the next in ONE persistent launch over 32-pixel tiles (ResNet stage 1, HRNet layer1: 64 -> 256 -> 64 channels):
//     T  = relu(scale3 * (A x W3^T) + bias3 + skip)        A: conv2 output (M, 64),  W3: 64 -> 256,  skip / T: (M, 256)        [conv3 + bn3 + add + relu, Resnet.py:120-128]
//     Y1 = relu(scale1 * (T x W1^T) + bias1)               W1: 256 -> 64                                                        [next block's conv1 + bn1 + relu, :104-108]
// T is stored (it is the next block's skip connection) but never re-read from HBM: the second GEMM takes it from LDS.  Each wave owns 64 of T's 256 channels in the first GEMM and
// exactly that K range of the second one (split K over the four waves, partial tiles summed in wave order through LDS: fixed order, batch-independent bits).
// Both filters stay in registers (64 + 64 values per lane); the A rows arrive by LDS-DMA one tile ahead, the skip rows are requested before the first GEMM and consumed after it,
// and the stores of a tile stay in flight across the barrier into the next one (counted s_waitcnt: VMEM operations retire in order).
// T has the bits of the tiled implicit GEMM (same k order); Y1 sums K in 4 x 64 pieces, so it differs from the two-launch path in the last bits (5e-7 of the plane maximum).
// Measured at 1024 crops of 64x48 pixels (tools/chain_bench.py): 2.00 ms against 2.48 - 2.64 ms for the two tiled launches; the first GEMM alone (w1 == NULL) 1.36 against 1.51 ms.
#include "common.h"
#include "buffer.h"

namespace vatl {

struct ChainParams {
    const float* a;          // (M, 64)
    const float* w3;         // packed [256][64]
    const float* scale3;
    const float* bias3;
    const float* res;        // (M, 256) or null
    float* t;                // (M, 256)
    const float* w1;         // packed [N2][256], or null: first GEMM only
    const float* scale1;
    const float* bias1;
    float* out2;             // (M, N2)
    int M, N2, relu3;
    int m_tiles;
    unsigned a_bytes, t_bytes, o_bytes, w3_bytes, w1_bytes;
};

constexpr unsigned BOOB = 0xFFFFFFFFu;

constexpr int BT_LDT = 260;                       // T tile row pitch (floats)
constexpr int BT_AS = 32 * 64;                    // one A stage: 32 rows x 64 floats, 16-byte chunks XOR-swizzled by (row & 7)
constexpr int BT_FLOATS = 2 * BT_AS + 4 * 32 * 68;      // the T tile (32 x 260 = 8320 floats) and, after it, the four partial tiles (4 x 32 x 68 = 8704) share the region

template <bool SECOND>
__global__ __launch_bounds__(256, 2) void bottleneck_chain_kernel(ChainParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                             // [2][32][64]
    float* Ts = smem + 2 * BT_AS;                 // [32][260]; after the second GEMM's reads: partial tiles [4][32][64 + 4]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, h = lane >> 5;
    const int nblk = gridDim.x, bid = blockIdx.x;

    const __amdgpu_buffer_rsrc_t ar = buf_rsrc(p.a, p.a_bytes);
    const __amdgpu_buffer_rsrc_t w3r = buf_rsrc(p.w3, p.w3_bytes);
    const __amdgpu_buffer_rsrc_t tr = buf_rsrc(p.t, p.t_bytes);
    const __amdgpu_buffer_rsrc_t rr = buf_rsrc(p.res ? p.res : p.t, p.res ? p.t_bytes : 0u);

    // filters in MFMA B-fragment order: lane (channel fr of the 32-column block, k half h) holds W[n][8 g + 4 h .. + 3]
    f32x4 w3f[2][8];                              // first GEMM: this wave's 64 output channels, K = 64
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int g = 0; g < 8; ++g) w3f[nb][g] = buf_load4(w3r, (unsigned)(((wave * 64 + nb * 32 + fr) * 64 + 8 * g + 4 * h) * 4));
    float sc3[2], bi3[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int n = wave * 64 + nb * 32 + fr;
        sc3[nb] = p.scale3 ? p.scale3[n] : 1.f;
        bi3[nb] = p.bias3 ? p.bias3[n] : 0.f;
    }
    f32x4 w1f[SECOND ? 2 : 1][8];                 // second GEMM: all 64 output channels, this wave's K range [64 wave, 64 wave + 64)
    if constexpr (SECOND) {
        const __amdgpu_buffer_rsrc_t w1r = buf_rsrc(p.w1, p.w1_bytes);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int g = 0; g < 8; ++g) w1f[nb][g] = buf_load4(w1r, (unsigned)(((nb * 32 + fr) * 256 + wave * 64 + 8 * g + 4 * h) * 4));
    }
    const float lo3 = p.relu3 ? 0.f : -INFINITY;

    // A stage by LDS-DMA: 512 16-byte pieces per tile = 2 wave instructions per wave; LDS piece q = (row q >> 4, position q & 15) receives the row's chunk (q & 15) ^ (row & 7)
    // (rows past M need no test anywhere below: their byte offsets lie past the descriptors' sizes, so the hardware drops those loads and stores)
    auto a_dma = [&](int buf, int mt) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = (wave * 2 + u) * 64 + lane;
            const int row = q >> 4, chunk = (q & 15) ^ (row & 7);
            const unsigned off = (unsigned)mt * (32u * 64u * 4u) + (unsigned)(row * 64 + chunk * 4) * 4u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ar, (lds_void*)(As + buf * BT_AS + (wave * 2 + u) * 256), 16, off, 0, 0, 0);
        }
    };

    const int c4 = tid & 63, r0 = tid >> 6;
    const unsigned tlane = (unsigned)(r0 * 256 + c4 * 4) * 4u;
    int mt = bid, buf = 0;
    if (mt < p.m_tiles) a_dma(0, mt);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (; mt < p.m_tiles; mt += nblk, buf ^= 1) {
        __syncthreads();                          // this tile's A rows have landed (waited for at the end of the pass before); T of the tile before has been consumed
        // the skip-connection rows of this tile: requested now, consumed after the first GEMM (their latency behind 64 MFMAs per wave)
        const unsigned tbase = (unsigned)mt * (32u * 1024u) + tlane;
        f32x4 rs[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) rs[u] = p.res ? buf_load4(rr, tbase + (unsigned)u * 4096u) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (mt + nblk < p.m_tiles) a_dma(buf ^ 1, mt + nblk);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[nb][e] = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 af = *reinterpret_cast<const f32x4*>(As + buf * BT_AS + fr * 64 + (((2 * g + h) ^ (fr & 7)) << 2));
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[tt], w3f[nb][g][tt], acc[nb], 0, 0, 0);
        }
        // conv3 + bn3 into the T tile
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
                Ts[row * BT_LDT + wave * 64 + nb * 32 + fr] = acc[nb][e] * sc3[nb] + bi3[nb];
            }
        __syncthreads();
        // + skip, ReLU, stored as the block output (16-byte rows) and written back to the tile for the second GEMM
        {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int row = r0 + 4 * u;
                const f32x4 v = *reinterpret_cast<const f32x4*>(&Ts[row * BT_LDT + c4 * 4]);
                f32x4 o;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = fmaxf(v[c] + rs[u][c], lo3);
                buf_store4(tr, tbase + (unsigned)u * 4096u, o);
                if constexpr (SECOND) *reinterpret_cast<f32x4*>(&Ts[row * BT_LDT + c4 * 4]) = o;
            }
        }
        if constexpr (SECOND) {
            __syncthreads();
            // second GEMM over this wave's K range: A fragments from the T tile (lane = (pixel row fr, k half h))
            f32x16 acc2[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc2[nb][e] = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 tf = *reinterpret_cast<const f32x4*>(&Ts[fr * BT_LDT + wave * 64 + 8 * g + 4 * h]);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) acc2[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(tf[tt], w1f[nb][g][tt], acc2[nb], 0, 0, 0);
            }
            __syncthreads();                      // every wave has read its K range of T: the tile region is free for the partial sums
            float* Pw = Ts + wave * (32 * 68);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
                    Pw[row * 68 + nb * 32 + fr] = acc2[nb][e];
                }
            __syncthreads();
            {
                const __amdgpu_buffer_rsrc_t orr = buf_rsrc(p.out2, p.o_bytes);
                const int q4 = tid & 15, q0 = tid >> 4;              // 16 quads x 16 rows per pass, 2 passes
                const f32x4 s1 = p.scale1 ? *reinterpret_cast<const f32x4*>(p.scale1 + q4 * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
                const f32x4 b1 = p.bias1 ? *reinterpret_cast<const f32x4*>(p.bias1 + q4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int row = q0 + 16 * u;
                    f32x4 sum = *reinterpret_cast<const f32x4*>(&Ts[row * 68 + q4 * 4]);
#pragma unroll
                    for (int w = 1; w < 4; ++w) {
                        const f32x4 q = *reinterpret_cast<const f32x4*>(&Ts[w * (32 * 68) + row * 68 + q4 * 4]);
#pragma unroll
                        for (int c = 0; c < 4; ++c) sum[c] += q[c];
                    }
                    f32x4 o;
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] = fmaxf(sum[c] * s1[c] + b1[c], 0.f);
                    buf_store4(orr, ((unsigned)(mt * 32 + row) * 64u + (unsigned)q4 * 4u) * 4u, o);
                }
            }
        }
        // the next tile's A rows were requested before this pass's stores: wait for them only (vmcnt retires in order), the stores stay in flight across the barrier
        if constexpr (SECOND) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    }
}


// ---- The two other 256-channel boundaries of stage 1 as one launch each (same idea as above: T stored once, the next block's conv1 takes it from LDS) ----
//   form P (projection block):  T = relu(bias + [conv2 output | block input] x Wdual^T)   K = 64 + 64 (the packed dual filter and folded bias of conv1x1_rows_kernel<true>),
//                               Y = relu(scale1 * (T x W1^T) + bias1)                     W1: 256 -> 64   (next block's conv1)
//   form S (step into stage 2): T = relu(scale3 * (A x W3^T) + bias3 + skip)              K = 64 (the first GEMM above),
//                               Y = relu(scale1 * (T x W1^T) + bias1)                     W1: 256 -> 128  (stage 2's first conv1)
// The plain extension of the kernel above needs 192 filter registers and does not fit two blocks per CU.  What is different here:
//   * the second GEMM is split over N, not K: wave w owns Y columns 32 w .. 32 w + 31 (S, v_mfma_f32_32x32x2_f32) or 16 w .. 16 w + 15 (P, v_mfma_f32_16x16x4_f32) and
//     reads the whole T tile from LDS.  No partial sums, no exchange, two barriers per tile.  S walks K in the order of conv1x1_rows256_kernel: Y has its bits.
//     P walks K as 16 q + 4 j + tt (j = lane / 16): fp32 rounding of the tiled GEMM's value, not its bits.
//   * the T tile is kept as four 64-column blocks [wave][32 rows][64] with the 16-byte chunks XOR-swizzled by (row & 7), the A stage's layout: the wave that computes a
//     64-column block of T is the one that brings its skip values in by LDS-DMA (S: eight 1 KB requests per wave and tile, issued before the first GEMM), so the skip
//     needs a counted s_waitcnt and no barrier, and no registers across the MFMAs.
// T has the bits of the launches replaced (same k order, same epilogue expression).  Arithmetic is per tile: a crop's bits do not depend on its batch position.
struct FormParams {
    const float* a;          // (M, 64) conv2 output
    const float* x2;         // P: (M, 64) block input
    const float* w3;         // P: packed dual [256][128]; S: packed [256][64]
    const float* scale3;
    const float* bias3;
    const float* res;        // S: (M, 256) or null
    float* t;                // (M, 256)
    const float* w1;         // packed [N2][256]
    const float* scale1;
    const float* bias1;
    float* y;                // (M, N2)
    int m_tiles, relu3;
    unsigned a_bytes, t_bytes, y_bytes;
};

// scalar + lane part of an address; opaque to the compiler, so the sums are formed where they are used and not kept in registers across the tile loop
__device__ __forceinline__ unsigned uadd(unsigned s_part, unsigned v_part) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned r;
    asm("v_add_u32 %0, %1, %2" : "=v"(r) : "s"(s_part), "v"(v_part));
    return r;
#else
    return s_part + v_part;
#endif
}

constexpr int CF_TS = 4 * 32 * 64;                // the T tile: [4 column blocks][32 rows][64], chunks swizzled

template <bool PROJ>
__global__ __launch_bounds__(256, 2) void chain_form_kernel(FormParams p) {
    constexpr int K1 = PROJ ? 128 : 64, G1 = K1 / 8, AS = 32 * K1, N2 = PROJ ? 64 : 128;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                             // [2][32][K1]
    float* Ts = smem + 2 * AS;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, h = lane >> 5;
    const int nblk = gridDim.x;

    const __amdgpu_buffer_rsrc_t ar = buf_rsrc(p.a, p.a_bytes);
    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(PROJ ? p.x2 : p.a, PROJ ? p.a_bytes : 0u);
    const __amdgpu_buffer_rsrc_t w3r = buf_rsrc(p.w3, 256u * K1 * 4u);
    const __amdgpu_buffer_rsrc_t w1r = buf_rsrc(p.w1, (unsigned)N2 * 256u * 4u);
    const __amdgpu_buffer_rsrc_t tr = buf_rsrc(p.t, p.t_bytes);
    const __amdgpu_buffer_rsrc_t rr = buf_rsrc(p.res ? p.res : p.t, p.res ? p.t_bytes : 0u);
    const __amdgpu_buffer_rsrc_t yr = buf_rsrc(p.y, p.y_bytes);

    // first GEMM: this wave's 64 channels of T, all of K1, in MFMA B-fragment order (lane = (channel fr of a 32-column block, k half h))
    f32x4 w3f[2][G1];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int g = 0; g < G1; ++g) w3f[nb][g] = buf_load4(w3r, (unsigned)(((wave * 64 + nb * 32 + fr) * K1 + 8 * g + 4 * h) * 4));
    float sc3[2], bi3[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int n = wave * 64 + nb * 32 + fr;
        sc3[nb] = p.scale3 ? p.scale3[n] : 1.f;
        bi3[nb] = p.bias3 ? p.bias3[n] : 0.f;
    }
    // second GEMM: this wave's Y columns, all 256 values of K.  S: lane (column fr, k half h) holds W1[n][8 g + 4 h ..]; P: lane (column lane & 15, k quarter j) W1[n][16 q + 4 j ..]
    const int l16 = lane & 15, j = lane >> 4;
    const int n1 = PROJ ? wave * 16 + l16 : wave * 32 + fr;
    f32x4 w1f[PROJ ? 16 : 32];
#pragma unroll
    for (int g = 0; g < (PROJ ? 16 : 32); ++g) w1f[g] = buf_load4(w1r, (unsigned)((n1 * 256 + (PROJ ? 16 * g + 4 * j : 8 * g + 4 * h)) * 4));
    const float sc1 = p.scale1 ? p.scale1[n1] : 1.f, bi1 = p.bias1 ? p.bias1[n1] : 0.f;
    const float lo3 = p.relu3 ? 0.f : -INFINITY;

    // Lane parts of the LDS and global addresses, kept few on purpose (the filters take 192 of the 256 registers); the wave- and tile-dependent parts are scalar and
    // joined by uadd() inside the loop.  LDS addresses are float indices into smem.
    const int c4 = lane, r0 = wave;               // T write-out: 64 float4 columns x 4 rows per pass, 8 passes
    int ax[4], tq[4], tw[2], tx[PROJ ? 2 : 4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ax[k] = fr * K1 + (((2 * k + h) ^ (fr & 7)) << 2);                                  // A fragment g: ax[g & 3] + 32 (g >> 2)   (chunk (2 g + h) ^ (fr & 7))
        tq[k] = 2 * AS + 4 * h * 64 + ((((fr >> 2) ^ (4 * h) ^ k) << 2) | (fr & 3));        // T element e of column block nb: tq[e & 3] + 64 ((e & 3) + 8 (e >> 2)) + 32 nb
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) tw[k] = 2 * AS + (c4 >> 4) * 2048 + (((c4 & 15) ^ (r0 | 4 * k)) << 2);       // T piece of row r0 + 4 u: tw[u & 1] + 64 r0 + 256 u
#pragma unroll
    for (int k = 0; k < (PROJ ? 2 : 4); ++k)      // T fragment.  S, g: tx[g & 3] + 32 ((g >> 2) & 1) + 2048 (g >> 3);  P, (q, rb): tx[q & 1] + 32 ((q >> 1) & 1) + 2048 (q >> 2) + 1024 rb
        tx[k] = 2 * AS + (PROJ ? l16 * 64 + (((4 * k + j) ^ (l16 & 7)) << 2) : fr * 64 + (((2 * k + h) ^ (fr & 7)) << 2));
    unsigned va[PROJ ? 4 : 2], vs[2];             // A and skip requests: byte offset of the lane's piece within the request's rows
#pragma unroll
    for (int u = 0; u < (PROJ ? 4 : 2); ++u)
        va[u] = PROJ ? (unsigned)(h * 64 + (((lane & 31) ^ (2 * u + h)) & 15) * 4) * 4u : (unsigned)(j * 64 + (l16 ^ (4 * u + j)) * 4) * 4u;
#pragma unroll
    for (int k = 0; k < 2; ++k) vs[k] = (unsigned)(j * 256 + (l16 ^ (4 * k + j)) * 4) * 4u;
    const unsigned vy = PROJ ? (unsigned)(4 * j * N2 + l16) * 4u : (unsigned)(4 * h * N2 + fr) * 4u;          // accumulator layout: rows 4 j + r (P) / (e & 3) + 8 (e >> 2) + 4 h (S)

    // A stage by LDS-DMA, one tile ahead: 16-byte pieces, LDS piece (row, position) receives the row's chunk position ^ (row & 7).  Rows past M (and the tile after the
    // last one) need no test: their byte offsets lie past the descriptors' sizes (the hardware writes zeros for those loads and drops those stores).
    auto a_dma = [&](int buf, int mt) {
#pragma unroll
        for (int u = 0; u < K1 / 32; ++u) {
            const int piece = wave * (K1 / 32) + u;                 // 1 KB of the stage: 4 rows (S) / 2 rows (P)
            lds_void* dst = (lds_void*)(As + buf * AS + piece * 256);
            const unsigned off = uadd((unsigned)mt * (32u * 64u * 4u) + (unsigned)piece * (PROJ ? 2u : 4u) * 256u, va[u]);
            if constexpr (PROJ) {                 // chunks 0 .. 15 from the conv2 output, 16 .. 31 from the block input: two requests with complementary lanes
                if ((lane & 16) == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(ar, dst, 16, off, 0, 0, 0);
                else                  __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, dst, 16, off, 0, 0, 0);
            } else {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ar, dst, 16, off, 0, 0, 0);
            }
        }
    };
    // S: the skip values of this wave's 64 columns of the tile, straight into its block of the T tile: request u brings rows 4 u .. 4 u + 3
    auto skip_dma = [&](int mt) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rr, (lds_void*)(Ts + wave * 2048 + u * 256), 16,
                                                     uadd((unsigned)mt * (32u * 1024u) + (unsigned)u * 4096u + (unsigned)wave * 256u, vs[u & 1]), 0, 0, 0);
    };

    int mt = blockIdx.x, buf = 0;
    a_dma(0, mt);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (; mt < p.m_tiles; mt += nblk, buf ^= 1) {
        lds_barrier();                            // this tile's A rows have landed (waited for at the end of the pass before); every wave is done with the T tile of the pass before
        if constexpr (!PROJ) skip_dma(mt);        // (no skip tensor: a descriptor of size 0, the requests write zeros)
        a_dma(buf ^ 1, mt + nblk);                // always issued (past the last tile: zeros into the idle stage), so the counted waits below hold on every pass
        __builtin_amdgcn_sched_barrier(0);
        // the wave's two 32-column blocks one after the other (16 accumulator registers live, not 32); bn3 (+ skip) + ReLU into the wave's block of the T tile
        const int abase = buf * AS, tqbase = wave * 2048;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int g = 0; g < G1; ++g) {
                const f32x4 af = *reinterpret_cast<const f32x4*>(smem + abase + ax[g & 3] + 32 * (g >> 2));
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[tt], w3f[nb][g][tt], acc, 0, 0, 0);
            }
            if (!PROJ && nb == 0) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");      // the skip requests are older than the two A requests: they have landed
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float* q = smem + tqbase + tq[e & 3] + 64 * ((e & 3) + 8 * (e >> 2)) + 32 * nb;
                const float v = acc[e] * sc3[nb] + bi3[nb];
                *q = fmaxf(v + (PROJ ? 0.f : *q), lo3);
            }
        }
        lds_barrier();
        // T, the block output: 16-byte pieces of whole rows
#pragma unroll
        for (int u = 0; u < 8; ++u)
            buf_store4(tr, uadd((unsigned)mt * (32u * 1024u) + (unsigned)(r0 + 4 * u) * 1024u, (unsigned)c4 * 16u),
                       *reinterpret_cast<const f32x4*>(smem + r0 * 64 + tw[u & 1] + 256 * u));
        // second GEMM: A fragments from the T tile, Y stored straight from the accumulator layout
        const unsigned ytile = (unsigned)mt * (32u * N2 * 4u) + (unsigned)wave * (PROJ ? 64u : 128u);
        if constexpr (PROJ) {
            f32x4 acc2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                f32x4 tf[2];
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) tf[rb] = *reinterpret_cast<const f32x4*>(smem + tx[q & 1] + 32 * ((q >> 1) & 1) + 2048 * (q >> 2) + 1024 * rb);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) acc2[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(tf[rb][tt], w1f[q][tt], acc2[rb], 0, 0, 0);
            }
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) buf_store1(yr, uadd(ytile + (unsigned)(rb * 16 + r) * (N2 * 4u), vy), fmaxf(acc2[rb][r] * sc1 + bi1, 0.f));
            asm volatile("s_waitcnt vmcnt(16)" ::: "memory");       // the next tile's A rows were requested before this pass's 8 + 8 stores: wait for them only
        } else {
            f32x16 acc2;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc2[e] = 0.f;
#pragma unroll
            for (int g = 0; g < 32; ++g) {
                const f32x4 tf = *reinterpret_cast<const f32x4*>(smem + tx[g & 3] + 32 * ((g >> 2) & 1) + 2048 * (g >> 3));
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(tf[tt], w1f[g][tt], acc2, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) buf_store1(yr, uadd(ytile + (unsigned)((e & 3) + 8 * (e >> 2)) * (N2 * 4u), vy), fmaxf(acc2[e] * sc1 + bi1 + 0.f, 0.f));
            asm volatile("s_waitcnt vmcnt(24)" ::: "memory");       // ... 8 + 16 stores
        }
    }
}

}  // namespace vatl

using namespace vatl;

static bool chain_shape_ok(int Cmid, int Cout, int Cnext, int64_t M) {
    return Cmid == 64 && Cout == 256 && (Cnext == 64 || Cnext == 0) && M > 0 && (M + 32) * 256 < (1LL << 30);       // 32-bit byte offsets into T, tile rounding included
}

extern "C" int vatl_bottleneck_chain_supported(int Cmid, int Cout, int Cnext, int64_t M) { return chain_shape_ok(Cmid, Cout, Cnext, M) ? 1 : 0; }

extern "C" int vatl_bottleneck_chain_fwd(const float* a, const float* w3, const float* scale3, const float* bias3, const float* skip, float* t, const float* w1,
                                         const float* scale1, const float* bias1, float* y1, int64_t M, int Cmid, int Cout, int Cnext, void* stream) {
    if (!a || !w3 || !t || (Cnext != 0) != (w1 != nullptr) || (w1 && !y1)) return fail(VATL_EINVAL, "bottleneck_chain_fwd: bad arguments");
    if (!chain_shape_ok(Cmid, Cout, Cnext, M)) return fail(VATL_EINVAL, "bottleneck_chain_fwd: serves 64 -> 256 (-> 64) channels and (M + 32) * 256 < 2^30 pixels x channels");
    ChainParams p{};
    p.a = a; p.w3 = w3; p.scale3 = scale3; p.bias3 = bias3; p.res = skip; p.t = t; p.w1 = w1; p.scale1 = scale1; p.bias1 = bias1; p.out2 = y1;
    p.M = (int)M; p.N2 = 64; p.relu3 = 1; p.m_tiles = (int)((M + 31) / 32);
    p.a_bytes = (unsigned)(M * 64 * 4); p.t_bytes = (unsigned)(M * 256 * 4); p.o_bytes = (unsigned)(M * 64 * 4); p.w3_bytes = 256 * 64 * 4; p.w1_bytes = 64 * 256 * 4;
    const int smem = BT_FLOATS * (int)sizeof(float);
    static std::atomic<unsigned> c0{0}, c1{0};
    const double padded = (double)p.m_tiles * 32.0;
    if (w1) {
        auto kern = bottleneck_chain_kernel<true>;
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, c1, "bottleneck_chain")) return rc;
        const int grid = p.m_tiles < 512 ? p.m_tiles : 512;                   // 237 registers: two blocks per CU
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, (hipStream_t)stream, p);
        meter_add(0, 2.0 * padded * 256.0 * 64.0 * 2.0);
        meter_route(kRouteChain);
    } else {
        auto kern = bottleneck_chain_kernel<false>;
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, c0, "bottleneck_chain")) return rc;
        const int grid = p.m_tiles < 512 ? p.m_tiles : 512;                   // (163 registers: a third block per CU fits and was measured: no gain)
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, (hipStream_t)stream, p);
        meter_add(0, 2.0 * padded * 256.0 * 64.0);
        meter_route(kRouteChain);
    }
    return check_launch("bottleneck_chain");
}

static bool form_shape_ok(int Cmid, int Cout, int Cnext, int want_next, int64_t M) {
    return Cmid == 64 && Cout == 256 && Cnext == want_next && M > 0 && (M + 32) * 256 < (1LL << 30);                // as chain_shape_ok
}

extern "C" int vatl_chain_proj_supported(int Cmid, int Cout, int Cnext, int64_t M) { return form_shape_ok(Cmid, Cout, Cnext, 64, M) ? 1 : 0; }
extern "C" int vatl_chain_step_supported(int Cmid, int Cout, int Cnext, int64_t M) { return form_shape_ok(Cmid, Cout, Cnext, 128, M) ? 1 : 0; }

static int chain_form_launch(bool proj, FormParams p, int64_t M, void* stream) {
    const int N2 = proj ? 64 : 128, K1 = proj ? 128 : 64;
    const char* what = proj ? "chain_proj" : "chain_step";
    p.m_tiles = (int)((M + 31) / 32);
    p.a_bytes = (unsigned)(M * 64 * 4); p.t_bytes = (unsigned)(M * 256 * 4); p.y_bytes = (unsigned)(M * N2 * 4);
    const int smem = (2 * 32 * K1 + CF_TS) * (int)sizeof(float);
    static std::atomic<unsigned> c[2] = {{0}, {0}};
    void (*kern)(FormParams) = chain_form_kernel<false>;
    if (proj) kern = chain_form_kernel<true>;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, c[proj], what)) return rc;
    const int grid = p.m_tiles < 512 ? p.m_tiles : 512;                       // two blocks per CU
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, (hipStream_t)stream, p);
    meter_add(0, 2.0 * ((double)p.m_tiles * 32.0) * 256.0 * (double)(K1 + N2));
    meter_route(proj ? kRouteChainProj : kRouteChainStep);
    return check_launch(what);
}

extern "C" int vatl_chain_proj_fwd(const float* a, const float* x2, const float* w, const float* scale, const float* bias, float* t, const float* w1, const float* scale1,
                                   const float* bias1, float* y1, int64_t M, int Cmid, int Cout, int Cnext, int relu, void* stream) {
    if (!a || !x2 || !w || !t || !w1 || !y1) return fail(VATL_EINVAL, "chain_proj_fwd: bad arguments");
    if (!form_shape_ok(Cmid, Cout, Cnext, 64, M)) return fail(VATL_EINVAL, "chain_proj_fwd: serves 64 + 64 -> 256 -> 64 channels and (M + 32) * 256 < 2^30 pixels x channels");
    FormParams p{};
    p.a = a; p.x2 = x2; p.w3 = w; p.scale3 = scale; p.bias3 = bias; p.t = t; p.w1 = w1; p.scale1 = scale1; p.bias1 = bias1; p.y = y1; p.relu3 = relu;
    return chain_form_launch(true, p, M, stream);
}

extern "C" int vatl_chain_step_fwd(const float* a, const float* w3, const float* scale3, const float* bias3, const float* skip, float* t, const float* w1,
                                   const float* scale1, const float* bias1, float* y1, int64_t M, int Cmid, int Cout, int Cnext, void* stream) {
    if (!a || !w3 || !t || !w1 || !y1) return fail(VATL_EINVAL, "chain_step_fwd: bad arguments");
    if (!form_shape_ok(Cmid, Cout, Cnext, 128, M)) return fail(VATL_EINVAL, "chain_step_fwd: serves 64 -> 256 -> 128 channels and (M + 32) * 256 < 2^30 pixels x channels");
    FormParams p{};
    p.a = a; p.w3 = w3; p.scale3 = scale3; p.bias3 = bias3; p.res = skip; p.t = t; p.w1 = w1; p.scale1 = scale1; p.bias1 = bias1; p.y = y1; p.relu3 = 1;
    return chain_form_launch(false, p, M, stream);
}
