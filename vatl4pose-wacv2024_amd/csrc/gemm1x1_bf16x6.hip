// The bf16x6 GEMM for the long-K 1x1 layers of the inference plans: fp32 operands, each product as six bf16 MFMAs.  Kernel, filter pack,
// launcher, the shape rules (vatl_gemm1x1_bf16x6_supported, and vatl_gemm1x1_bf16x6_short_supported of the short-K form) and the C entry points.
#include "conv_igemm.h"
#include "split16.h"
#include "tile_order.h"

namespace vatl {

// ---------------------------------------------------------------------------------------------------------
// Y[M][N] = A[M][K] W[N][K]^T for the shapes of gemm1x1_ring_kernel (stride-1 1x1 layers with K >= 512 and the dual-source conv3 +
// projection form, whole 128-wide N tiles, NHWC output) on the 16-bit matrix pipe with fp32 results.  split16.h cuts a float exactly
// into three bf16 pieces, a = a0 + a1 + a2, w = w0 + w1 + w2, and the product becomes the six piece products a_i w_j with i + j <= 2
// (the three dropped ones are below 2^-24 of the product).  Each piece product is exact in the fp32 accumulator.  Six
// v_mfma_f32_32x32x16_bf16 take 6/16 of the matrix-pipe cycles of the sixteen v_mfma_f32_32x32x2_f32 they replace.
//  * TWO accumulator sets: a0 w0 goes into one, the five small products (a0 w1, a1 w0, a1 w1, a0 w2, a2 w0, in this order, every
//    16-k stage) into the other, and the two are added once, in front of the epilogue.  With one set the small products are rounded
//    at the magnitude of the large sum and the network error rises to 1.06x fp32's; with two it is 0.99x (tests/probes/bf16x6_accuracy.py).
//  * the A operand stays fp32 in HBM and in LDS: the ring kernel's LDS-DMA requests and swizzle (rows of 64 bytes, chunk c of tile row r
//    at position c ^ ((r >> 2) & 3), applied on the source side).  A lane reads the eight k of its row that the MFMA wants from it
//    (chunks 2h and 2h + 1: k = 8h .. 8h + 7 of the stage, h = lane >> 5) with two ds_read_b128 — conflict-free like the ring's
//    reads, every service group shares h — and splits them in registers: per element two ANDs and two exact subtractions, per pair
//    three packs.
//  * the filter is split once, by vatl_pack_gemm1x1_bf16x6_weight, into three bf16 planes in the order the B fragments are read: per
//    (n-tile, stage) 12 KB = [plane 3][column block 4][lane 64] x 16 bytes, lane l of column block jb holding piece `plane` of
//    W[128 n_tile + 32 jb + (l & 31)][16 stage + 8 (l >> 5) + 0 .. 7].  The DMA copies it linearly, a fragment is one ds_read_b128 at
//    lane * 16: conflict-free, no swizzle.
//  * a stage is 16 k = 8 KB of A + 12 KB of B, a ring of four is 80 KB per block, two blocks per CU.  Per stage and wave 24 MFMAs, five DMA
//    requests, one counted s_waitcnt, one barrier.
//  * the k-loop is software-pipelined inside the wave: iteration s issues the 24 MFMAs of stage s from registers (A pieces and B fragments, two
//    sets) and, between them, reads the fragments of stage s + 1 from the ring and splits its A values into the other set: the split's 88 vector
//    instructions stand five to an MFMA gap, where they cost nothing (tools/probes/mfma_valu_overlap.hip), not in front of the MFMAs.
//    Ring discipline: behind the barrier of iteration s every wave's pieces of stage s + 1 have landed, and slot s % 4 is free — its fragments went
//    into registers in iteration s - 1, and the counted wait in front of the barrier also waits for those LDS reads (lgkmcnt(0)) — so the request of
//    stage s + 4 goes there.  Counted waits (per wave, oldest first; five requests a stage, VMEM retires in order):
//      prologue      [0, 1, 2, 3]                    vmcnt(15): stage 0 landed; barrier; stage 0 into set 0
//      s <= S-5      [s+1, s+2, s+3]                 vmcnt(10): stage s + 1 landed; barrier; then the request of stage s + 4
//      s  = S-4      [S-3, S-2, S-1]                 vmcnt(10); no request left
//      s  = S-3      [S-2, S-1]                      vmcnt(5)
//      s  = S-2      [S-1]                           vmcnt(0)
//      s  = S-1      nothing to read: MFMAs only, no wait, no barrier
//    Dual source: S1 = 2 k1 is a multiple of 4 (x6_shape_ok), so the four requests of a group of iterations s .. s + 3 (stages s + 4 .. s + 7) read one
//    source: x while s + 4 < S1, else x2.  The prologue's four stages read x (S1 >= 4).  The counts do not change at the crossing.
//  * the residual is read in the write-out, after the two accumulator sets are added (the registers the ring kernel keeps it in hold
//    the second set here).
// Arithmetic per output row depends on that row's inputs and the filter only: the same bits alone and in any batch position.
// Tail rows read row M-1; their stores lie past the descriptor and are dropped.  No atomics, no split-K.
// Dual source: stages 0 .. S1 - 1 = 2 k1 - 1 read x, the rest x2 at the row's strided pixel (the ring kernel's rules).
//
// SHORT (128 <= K < 512, N >= 512: conv3 of ResNet stages 2 and 3; gemm1x1_bf16x6_short_kernel): the same loop, products and order — 8 to 28
// stages — with the per-tile cost that a long loop hides taken out of the tail:
//  * scale, bias and the write-out addresses are loaded / computed in front of the k-loop;
//  * the residual tile is requested by LDS-DMA into the ring slots that fall free at the tail: iterations S-4 .. S-1 issue no operand requests, so
//    slot s % 4 is free from the barrier of iterations S-4, S-3 and S-2 on — 60 KB.  The 64 KB tile less the last eight rows of
//    either wave row (56 KB: compact row cr = 56 wm + lr, lr < 56, 512 bytes each, linear from the ring's base) goes there in 5 + 5 + 4
//    requests per wave, the 2 x 4 elements a lane owns of the other eight rows are loaded into registers in front of the loop.  The
//    write-out reads the tile with ds_read_b32 (16-byte chunk c of row cr sits at position c ^ 8 ((cr >> 2) & 1): the two half-waves
//    of a read, four rows apart, take opposite halves of the 64 banks).  The residual's HBM round trip thus runs under the last four
//    iterations' MFMAs.  Counted waits of the tail (per wave, oldest first): S-4: [S-3, S-2, S-1] -> vmcnt(10), then R0 (5); S-3: [S-2, S-1, R0]
//    -> vmcnt(10), then R1 (5); S-2: [S-1, R0, R1] -> vmcnt(10), then R2 (4); S-1: none; after the loop vmcnt(0) and one barrier.  The register
//    loads and the scale / bias loads in front of the loop share the counter: wherever the compiler puts them among the first requests, an
//    operation younger than stage s + 1's pieces can only make a counted wait stricter (vmcnt(N) leaves at most the N youngest outstanding), and
//    an older one has retired before them.
// ---------------------------------------------------------------------------------------------------------
constexpr int X6_BK = 16;                             // k per stage
constexpr int X6_NS = 4;                              // stages in the ring
constexpr int X6_A_FLOATS = 128 * X6_BK;              // 8 KB: 128 A rows of 64 bytes
constexpr int X6_B_BYTES = 3 * 128 * X6_BK * 2;       // 12 KB: three bf16 planes of 128 filter rows
constexpr int X6_STAGE = X6_A_FLOATS + X6_B_BYTES / 4;   // floats per stage
constexpr int X6_BYTES = X6_NS * X6_STAGE * (int)sizeof(float);

typedef __bf16 x6_bf16x8 __attribute__((ext_vector_type(8)));

template <int N>
__device__ __forceinline__ void x6_wait_vm() {       // s_waitcnt vmcnt(N), N a compile-time count of this wave's younger DMA requests; and every LDS read of
    static_assert(N == 0 || N == 5 || N == 10 || N == 15, "add the count here");     // the iteration before is done before the barrier that frees its slot
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory");
    else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(15) lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ f32x16 x6_mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x6_bf16x8, a), __builtin_bit_cast(x6_bf16x8, b), c, 0, 0, 0);
}

struct X6Epilogue {                                   // what the write-out needs beside the accumulators
    unsigned rowb, ylane;
    __amdgpu_buffer_rsrc_t yr, rr;
    float sc[2], bi[2], lo;
};

template <bool DUAL, bool RES, bool SHORT = false>
__device__ __forceinline__ void gemm1x1_bf16x6_body(const ConvParams& p, float* smem) {
    static_assert(!(SHORT && DUAL), "the short-K form is plain");
    constexpr bool LDSRES = SHORT && RES;             // residual through the ring slots that fall free at the tail
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;          // 2 x 2 waves of 64 x 64

    const int t = xcd_contiguous_index(blockIdx.x, gridDim.x);   // tile order of the ring kernel: n-tile fastest inside an XCD's run
    const int m_tile = t / p.n_tiles, n_tile = t - m_tile * p.n_tiles;
    const int m0 = m_tile * 128, n0 = n_tile * 128;

    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t wr = buf_rsrc(p.w, p.w_bytes);
    const __amdgpu_buffer_rsrc_t xr2 = buf_rsrc(DUAL ? p.x2 : p.x, DUAL ? p.x2_bytes : p.x_bytes);

    const int S = p.ktiles * 2;                       // stages (a multiple of 4: x6_shape_ok)
    const int S1 = DUAL ? p.k1 * 2 : S;               // stages that read x

    // ---- loader.  A: DMA instruction u (0, 1) of wave w fills tile rows (4u + w) * 16 .. + 15; lane -> (row lane >> 2, position lane & 3),
    // which receives the row's chunk (lane & 3) ^ ((row >> 2) & 3).  B: instruction u (0 .. 2) of wave w copies 1 KB piece 4u + w of the
    // stage's 12 KB, lane-linear.
    const int lchk = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned aoff[2], aoff2[2], boff[3];
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
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) boff[u] = (unsigned)(n_tile * S) * (unsigned)X6_B_BYTES + (unsigned)(4 * u + wave) * 1024u + (unsigned)lane * 16u;
    auto issue = [&](auto src, int buf, int s) {
        float* st = smem + buf * X6_STAGE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            lds_void* da = (lds_void*)(st + (4 * u + wave) * 256);
            if constexpr (DUAL && decltype(src)::value == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(xr2, da, 16, aoff2[u], (unsigned)(s - S1) * 64u, 0, 0);
            else                                             __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, da, 16, aoff[u], (unsigned)s * 64u, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void*)(st + X6_A_FLOATS + (4 * u + wave) * 256), 16, boff[u], (unsigned)s * (unsigned)X6_B_BYTES, 0, 0);
    };

    // ---- fragments.  A: row frow (+ 32 i) of the wave's 64, logical chunks 2h and 2h + 1 at positions (2h + c) ^ ((frow >> 2) & 3).
    // B: plane pl, column block 2 wn + j: 16 bytes at ((4 pl + 2 wn + j) * 64 + lane) * 16.
    const int frow = lane & 31, h = lane >> 5;
    const int fsw = (frow >> 2) & 3;
    const float* Ard[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) Ard[c] = smem + (wm * 64 + frow) * X6_BK + (((2 * h + c) ^ fsw) << 2);
    const float* Brd = smem + X6_A_FLOATS + (2 * wn * 64 + lane) * 4;

    // ---- write-out operands (SHORT: in front of the k-loop).  Element e of tile (i, j) is row 32 i + (e & 3) + 8 (e >> 2) + 4 h, channel 64 wn + 32 j + frow.
    auto epilogue_operands = [&]() {
        X6Epilogue ep;
        ep.rowb = (unsigned)p.Cout * 4u;
        ep.ylane = (unsigned)(m0 + wm * 64 + 4 * h) * ep.rowb + (unsigned)(n0 + wn * 64 + frow) * 4u;
        ep.yr = buf_rsrc(p.y, p.y_bytes);
        ep.rr = buf_rsrc(RES ? p.res : p.y, RES ? p.y_bytes : 0u);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + frow;
            ep.sc[j] = p.scale ? p.scale[n] : 1.f;
            ep.bi[j] = p.bias ? p.bias[n] : 0.f;
        }
        ep.lo = p.relu ? 0.f : -INFINITY;
        return ep;
    };
    X6Epilogue ep;
    if constexpr (SHORT) ep = epilogue_operands();
    float dres[2][4];                                 // LDSRES: residual of rows 56 .. 59 (+ 4 h) of the wave's 64, the eight rows the ring has no room for
    unsigned roff = 0;
    if constexpr (LDSRES) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) dres[j][r] = buf_load1(ep.rr, ep.ylane + (unsigned)(56 + r) * ep.rowb + (unsigned)j * 128u);
        // request u of piece Q by wave w fills compact rows 40 Q + 8 u + 2 w + (lane >> 5): 1 KB, lane-linear; the lane fetches chunk (lane & 31) ^ 8 (w >> 1)
        // (rows past M are clamped to row M - 1 like the A rows: every request stays inside the tensor, and those rows' stores are dropped)
        roff = (unsigned)n0 * 4u + (unsigned)((lane & 31) ^ ((wave >> 1) << 3)) * 16u;
    }
    const int rrow = m0 + 2 * wave + (lane >> 5);
    auto issue_res = [&](auto piece) {
        constexpr int Q = decltype(piece)::value;
#pragma unroll
        for (int u = 0; u < (Q < 2 ? 5 : 4); ++u) {
            const int cr0 = 40 * Q + 8 * u;                           // (a block of eight compact rows never straddles row 56)
            const int row0 = cr0 + (cr0 >= 56 ? 8 : 0);               // tile row of compact row cr0
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ep.rr, (lds_void*)(smem + (20 * Q + 4 * u + wave) * 256), 16,
                                                     (unsigned)min(rrow + row0, p.M - 1) * ep.rowb + roff, 0, 0, 0);
        }
    };

    f32x16 acc[2][2], sml[2][2];                      // a0 w0 | the five small products
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; sml[i][j][e] = 0.f; }

    // Operands in registers, two sets (set = stage & 1): the A pieces pa[set][piece][i] and the B fragments bw[set][plane][j].
    u32x4 pa[2][3][2], bw[2][3][2];
    auto read_a = [&](auto slot, f32x4 (&af)[2][2]) {
        constexpr int B = decltype(slot)::value;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) af[i][c] = *reinterpret_cast<const f32x4*>(Ard[c] + B * X6_STAGE + i * 32 * X6_BK);
    };
    auto read_b = [&](auto slot, int pl, u32x4 (&b)[3][2]) {
        constexpr int B = decltype(slot)::value;
#pragma unroll
        for (int j = 0; j < 2; ++j) b[pl][j] = *reinterpret_cast<const u32x4*>(Brd + B * X6_STAGE + (4 * pl + j) * 256);
    };
    auto split = [&](const f32x4 (&af)[2][2], u32x4 (&q)[3][2]) {       // split16.h: fragment dword d = k pair (2d, 2d + 1) of the lane's eight
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const split16::Pieces e = split16::split3(af[i][d >> 1][(2 * d) & 3]), o = split16::split3(af[i][d >> 1][(2 * d + 1) & 3]);
                q[0][i][d] = split16::pack_pair(e.hi, o.hi);
                q[1][i][d] = split16::pack_pair(e.mid, o.mid);
                q[2][i][d] = split16::pack_pair(e.lo, o.lo);
            }
    };

    // One iteration: the 24 MFMAs of stage s from the registers of set s & 1, and between them everything stage s + 1 needs to be in the other set.
    // KIND 0: steady state; 1: s = S-4, 2: s = S-3, 3: s = S-2 (nothing left to request); 4: s = S-1 (nothing left to read: MFMAs only, no barrier).
    // Instruction order (sched_group_barrier; the scheduler is free only inside a group): MFMA | the four A reads and the plane-0 B reads of stage s + 1 |
    // then 23 times one MFMA and either one DMA request (the first five gaps of an iteration that has requests) or five of the split's 88 instructions;
    // the plane-1 / plane-2 B reads of stage s + 1 follow the 16th / 20th MFMA, the last that reads those registers for stage s.  No split instruction
    // stands in front of the first two MFMAs: the A reads' latency runs under them.  (tools/probes/mfma_valu_overlap.hip: up to five of these per gap of
    // this MFMA cost nothing, in front of the MFMAs they cost 352 cycles; profiles/bf16x6_pipe_notes.md: one request per gap beats five in one gap.)
    auto stage = [&](auto slot, auto kind, auto src, int s) {
        constexpr int B = decltype(slot)::value, KIND = decltype(kind)::value, CUR = B & 1, NXT = CUR ^ 1;
        using Next = std::integral_constant<int, (B + 1) & 3>;
        f32x4 af[2][2];
        if constexpr (KIND <= 3) {
            if constexpr (KIND <= 1 || LDSRES) x6_wait_vm<10>();  // (LDSRES: the tail's residual requests keep two pieces behind stage s + 1, see above)
            else if constexpr (KIND == 2) x6_wait_vm<5>();
            else x6_wait_vm<0>();
            __builtin_amdgcn_s_barrier();             // every wave's pieces of stage s + 1 have landed; every wave has read slot s % 4 into registers
            asm volatile("" ::: "memory");
            read_a(Next{}, af);
            read_b(Next{}, 0, bw[NXT]);
            if constexpr (KIND == 0) issue(src, B, s + 4);
            else if constexpr (LDSRES) issue_res(std::integral_constant<int, KIND - 1>{});      // into slot B = KIND - 1 (S % 4 == 0)
        }
        auto& a = pa[CUR];
        auto& b = bw[CUR];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = x6_mfma(a[0][i], b[0][j], acc[i][j]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) sml[i][j] = x6_mfma(a[0][i], b[1][j], sml[i][j]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) sml[i][j] = x6_mfma(a[1][i], b[0][j], sml[i][j]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) sml[i][j] = x6_mfma(a[1][i], b[1][j], sml[i][j]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) sml[i][j] = x6_mfma(a[0][i], b[2][j], sml[i][j]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) sml[i][j] = x6_mfma(a[2][i], b[0][j], sml[i][j]);
        if constexpr (KIND <= 3) {
            read_b(Next{}, 1, bw[NXT]);
            read_b(Next{}, 2, bw[NXT]);
            split(af, pa[NXT]);
            __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
            constexpr int NREQ = KIND == 0 ? 5 : (LDSRES ? (KIND == 3 ? 4 : 5) : 0);      // DMA requests of this iteration
#pragma unroll
            for (int g = 1; g < 24; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                if (g <= NREQ) __builtin_amdgcn_sched_group_barrier(0x10, 1, 0);
                else if (g >= 2) __builtin_amdgcn_sched_group_barrier(0x2, 5, 0);
                if (g == 15 || g == 19) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);            // an iteration's reads and requests stay between its barrier and the next
    };
    using C0 = std::integral_constant<int, 0>;
    using C1 = std::integral_constant<int, 1>;
    using C2 = std::integral_constant<int, 2>;
    using C3 = std::integral_constant<int, 3>;
    using C4 = std::integral_constant<int, 4>;

    using X2 = std::integral_constant<int, DUAL ? 1 : 0>;   // source of the stages past S1 (x itself for the plain form)
    auto group = [&](auto src, int s) {               // four steady-state iterations; their requests (stages s + 4 .. s + 7) all read one source: S1 % 4 == 0
        stage(C0{}, C0{}, src, s);
        stage(C1{}, C0{}, src, s + 1);
        stage(C2{}, C0{}, src, s + 2);
        stage(C3{}, C0{}, src, s + 3);
    };

    issue(C0{}, 0, 0);                                // (S1 >= 4: the first four stages read x)
    issue(C0{}, 1, 1);
    issue(C0{}, 2, 2);
    issue(C0{}, 3, 3);
    {                                                 // stage 0 into set 0
        x6_wait_vm<15>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        f32x4 af[2][2];
        read_a(C0{}, af);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) read_b(C0{}, pl, bw[0]);
        split(af, pa[0]);
        __builtin_amdgcn_sched_barrier(0);
    }
    int s = 0;
    if constexpr (DUAL)
        for (; s < S1 - 4; s += 4) group(C0{}, s);    // requests up to stage S1 - 1
    for (; s < S - 4; s += 4) group(X2{}, s);
    stage(C0{}, C1{}, X2{}, s);                       // the last four: nothing left to request
    stage(C1{}, C2{}, X2{}, s + 1);
    stage(C2{}, C3{}, X2{}, s + 2);
    stage(C3{}, C4{}, X2{}, s + 3);

    // ---- write-out from the accumulator layout (the ring kernel's): element e of tile (i, j) is row 32 i + (e & 3) + 8 (e >> 2) + 4 h,
    // channel 64 wn + 32 j + frow; rows >= M lie past the descriptor (loads read 0, stores are dropped).  Same expression as conv_epilogue.
    if constexpr (!SHORT) {
        const unsigned rowb = (unsigned)p.Cout * 4u;
        const unsigned ylane = (unsigned)(m0 + wm * 64 + 4 * h) * rowb + (unsigned)(n0 + wn * 64 + frow) * 4u;
        const __amdgpu_buffer_rsrc_t yr = buf_rsrc(p.y, p.y_bytes);
        const __amdgpu_buffer_rsrc_t rr = buf_rsrc(RES ? p.res : p.y, RES ? p.y_bytes : 0u);
        float sc[2], bi[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + frow;
            sc[j] = p.scale ? p.scale[n] : 1.f;
            bi[j] = p.bias ? p.bias[n] : 0.f;
        }
        const float lo = p.relu ? 0.f : -INFINITY;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float rs[2][16];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    rs[j][e] = RES ? buf_load1(rr, ylane + (unsigned)(32 * i + (e & 3) + 8 * (e >> 2)) * rowb + (unsigned)j * 128u) : 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float a = acc[i][j][e] + sml[i][j][e];
                    const float v = fmaxf(a * sc[j] + bi[j] + rs[j][e], lo);
                    buf_store1(yr, ylane + (unsigned)(32 * i + (e & 3) + 8 * (e >> 2)) * rowb + (unsigned)j * 128u, v);
                }
        }
    } else {                                          // the same expression; operands from in front of the loop, the residual from the ring's LDS
        if constexpr (RES) {
            x6_wait_vm<0>();
            __builtin_amdgcn_s_barrier();             // every wave's pieces of the residual tile have landed
            asm volatile("" ::: "memory");
        }
        const float* resL = smem + (wm * 56 + 4 * h) * 128 + wn * 64 + frow;      // the lane's first element of the residual tile
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float rs[2][16];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if constexpr (!RES) rs[j][e] = 0.f;
                    else rs[j][e] = (i == 1 && e >= 12) ? dres[j][e - 12] : resL[(32 * i + (e & 3) + 8 * (e >> 2)) * 128 + ((j ^ h) << 5)];
                }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float a = acc[i][j][e] + sml[i][j][e];
                    const float v = fmaxf(a * ep.sc[j] + ep.bi[j] + rs[j][e], ep.lo);
                    buf_store1(ep.yr, ep.ylane + (unsigned)(32 * i + (e & 3) + 8 * (e >> 2)) * ep.rowb + (unsigned)j * 128u, v);
                }
        }
    }
}

template <bool DUAL, bool RES>
__global__ __launch_bounds__(256, 2) void gemm1x1_bf16x6_kernel(ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    gemm1x1_bf16x6_body<DUAL, RES>(p, smem);
}

template <bool RES>
__global__ __launch_bounds__(256, 2) void gemm1x1_bf16x6_short_kernel(ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    gemm1x1_bf16x6_body<false, RES, true>(p, smem);
}

// ---- filter pack: one thread per 16-byte fragment piece (see the layout above)
__global__ __launch_bounds__(256) void gemm1x1_bf16x6_pack_kernel(const float* __restrict__ w, u32x4* __restrict__ u, int K, long long units) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= units) return;
    const int S = K / X6_BK;
    const int l = (int)(idx & 63), jb = (int)((idx >> 6) & 3);
    const long long rest = idx >> 8;
    const int pl = (int)(rest % 3);
    const long long ts = rest / 3;                    // n_tile * S + stage
    const int st = (int)(ts % S), n_tile = (int)(ts / S);
    const float* src = w + (long long)(n_tile * 128 + jb * 32 + (l & 31)) * K + st * X6_BK + 8 * (l >> 5);
    float pc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const split16::Pieces q = split16::split3(src[j]);
        pc[j] = pl == 0 ? q.hi : (pl == 1 ? q.mid : q.lo);
    }
    u32x4 o;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = split16::pack_pair(pc[2 * d], pc[2 * d + 1]);
    u[idx] = o;
}

// The shapes the kernel serves — the ring kernel's, by geometry alone: whole 128-wide N tiles, K a multiple of 64 and at least 512 (plain
// form; the stage count a multiple of 4), or the dual form with the x / x2 boundary K1 on a multiple of 64, at least 64 channels on
// either side and K >= 384; (M + 128) * N < 2^30 so that the byte offsets of the tail tile's dropped rows do not wrap; the operands
// within 32-bit byte offsets.
static bool x6_shape_ok(long long M, int K, int K1, int N) {
    if (M < 1 || N < 128 || (N % 128) || K < 1 || (K % 64)) return false;
    if (K1 == 0 ? K < 512 : (K1 < 64 || (K1 % 64) || K - K1 < 64 || K < 384)) return false;
    if ((M + 128) * N >= (1LL << 30) || M * (K1 ? K1 : K) >= (1LL << 30) || 6LL * N * K >= (1LL << 31)) return false;
    return true;
}

// The short-K rule, geometry only: stride-1 1x1 layers with 128 <= K < 512, K a multiple of 64 (8 .. 28 stages, a multiple of 4), N >= 512 (narrower layers stay
// on the row-streaming kernel) and N a multiple of 256 — the widths of the conv3 layers the form was measured on (512, 1024); the kernel itself serves any whole
// number of 128-wide N tiles, but N = 640 and the like are left to the fp32 kernels until one is measured — and the 32-bit offset guards of x6_shape_ok.
static bool x6_short_shape_ok(long long M, int K, int N) {
    if (M < 1 || N < 512 || (N % 256) || K < 128 || K >= 512 || (K % 64)) return false;
    if ((M + 128) * N >= (1LL << 30) || M * K >= (1LL << 30) || 6LL * N * K >= (1LL << 31)) return false;
    return true;
}

template <bool DUAL, bool RES, bool SHORT = false>
static int launch_x6_impl(const ConvParams& p, hipStream_t st) {
    auto kern = [] {
        if constexpr (SHORT) return gemm1x1_bf16x6_short_kernel<RES>;
        else return gemm1x1_bf16x6_kernel<DUAL, RES>;
    }();
    static std::atomic<unsigned> configured{0};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), X6_BYTES, configured, SHORT ? "gemm1x1_bf16x6_short" : "gemm1x1_bf16x6")) return rc;
    ConvParams q = p;
    q.n_tiles = p.Cout / 128;
    q.m_tiles = cdiv(p.M, 128);
    q.splits = 1;
    hipLaunchKernelGGL(kern, dim3((unsigned)(q.m_tiles * q.n_tiles)), dim3(256), X6_BYTES, st, q);
    // six bf16 MFMAs in place of sixteen fp32-MFMA equivalents: the fp32-pipe time the launch occupies
    meter_add(0, (6.0 / 16.0) * 2.0 * ((double)q.m_tiles * 128) * ((double)q.n_tiles * 128) * ((double)q.ktiles * BK));
    meter_route(SHORT ? kRouteGemm1x1Bf16x6Short : kRouteGemm1x1Bf16x6);
    return check_launch(SHORT ? "gemm1x1_bf16x6_short" : "gemm1x1_bf16x6");
}

}  // namespace vatl

using namespace vatl;

extern "C" int64_t vatl_gemm1x1_bf16x6_weight_floats(int N, int K) { return 3LL * N * K / 2; }

extern "C" int vatl_pack_gemm1x1_bf16x6_weight(const float* w, float* u, int N, int K, void* stream) {
    if (!w || !u) return fail(VATL_EINVAL, "pack_gemm1x1_bf16x6_weight: null pointer");
    if (N < 128 || (N % 128) || K < 64 || (K % 64) || 6LL * N * K >= (1LL << 31))
        return fail(VATL_EINVAL, "pack_gemm1x1_bf16x6_weight: N %d must be a multiple of 128, K %d of 64, 6 N K below 2^31 bytes", N, K);
    const long long units = 6LL * N * K / 16;
    hipLaunchKernelGGL(gemm1x1_bf16x6_pack_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, reinterpret_cast<u32x4*>(u), K, units);
    return check_launch("gemm1x1_bf16x6_pack");
}

static ConvParams x6_plain_params(const float* x, const float* u, const float* scale, const float* bias, const float* residual, float* y,
                                  int N, int H, int W, int Cin, int Cout, int relu) {
    const long long M = (long long)N * H * W;
    ConvParams p{};
    p.x = x; p.w = u; p.scale = scale; p.bias = bias; p.res = residual; p.y = y;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.CoutPad = Cout;
    p.R = 1; p.S = 1; p.stride = 1;
    p.Ho = H; p.Wo = W; p.M = (int)M;
    p.OH = H; p.OW = W; p.osy = 1; p.osx = 1;
    p.relu = relu;
    p.kpr = Cin / BK; p.ktiles = p.kpr; p.K = Cin;
    p.x_bytes = (unsigned)(M * Cin * 4); p.y_bytes = (unsigned)(M * Cout * 4); p.w_bytes = (unsigned)(6LL * Cout * Cin);
    p.d_HoWo = make_fastdiv((unsigned)(H * W)); p.d_Wo = make_fastdiv((unsigned)W);
    return p;
}

extern "C" int vatl_gemm1x1_bf16x6_supported(int64_t M, int K, int K1, int N) { return x6_shape_ok(M, K, K1, N) ? 1 : 0; }

extern "C" int vatl_gemm1x1_bf16x6_fwd(const float* x, const float* u, const float* scale, const float* bias, const float* residual, float* y,
                                       int N, int H, int W, int Cin, int Cout, int stride, int relu, void* stream) {
    if (!x || !u || !y || N <= 0 || H <= 0 || W <= 0) return fail(VATL_EINVAL, "gemm1x1_bf16x6_fwd: null pointer or empty batch");
    const long long M = (long long)N * H * W;
    if (stride != 1 || !x6_shape_ok(M, Cin, 0, Cout))
        return fail(VATL_EINVAL, "gemm1x1_bf16x6_fwd: %lld x %d -> %d, stride %d is outside stride 1, K %% 64 == 0, K >= 512, N %% 128 == 0 and 32-bit offsets", M, Cin, Cout, stride);
    const ConvParams p = x6_plain_params(x, u, scale, bias, residual, y, N, H, W, Cin, Cout, relu);
    return residual ? launch_x6_impl<false, true>(p, (hipStream_t)stream) : launch_x6_impl<false, false>(p, (hipStream_t)stream);
}

extern "C" int vatl_gemm1x1_bf16x6_short_supported(int64_t M, int K, int N) { return x6_short_shape_ok(M, K, N) ? 1 : 0; }

extern "C" int vatl_gemm1x1_bf16x6_short_fwd(const float* x, const float* u, const float* scale, const float* bias, const float* residual, float* y,
                                             int N, int H, int W, int Cin, int Cout, int stride, int relu, void* stream) {
    if (!x || !u || !y || N <= 0 || H <= 0 || W <= 0) return fail(VATL_EINVAL, "gemm1x1_bf16x6_short_fwd: null pointer or empty batch");
    const long long M = (long long)N * H * W;
    if (stride != 1 || !x6_short_shape_ok(M, Cin, Cout))
        return fail(VATL_EINVAL, "gemm1x1_bf16x6_short_fwd: %lld x %d -> %d, stride %d is outside stride 1, K %% 64 == 0, 128 <= K < 512, N %% 256 == 0, N >= 512 and 32-bit offsets", M, Cin, Cout, stride);
    const ConvParams p = x6_plain_params(x, u, scale, bias, residual, y, N, H, W, Cin, Cout, relu);
    return residual ? launch_x6_impl<false, true, true>(p, (hipStream_t)stream) : launch_x6_impl<false, false, true>(p, (hipStream_t)stream);
}

extern "C" int vatl_gemm1x1_bf16x6_dual_fwd(const float* a, const float* x, const float* u, const float* bias, const float* residual, float* y,
                                            int N, int Ho, int Wo, int C1, int H2, int W2, int C2, int stride2, int Cout, int relu, void* stream) {
    if (!a || !x || !u || !y || N <= 0 || Ho <= 0 || Wo <= 0) return fail(VATL_EINVAL, "gemm1x1_bf16x6_dual_fwd: null pointer or empty batch");
    if (residual) return fail(VATL_EINVAL, "gemm1x1_bf16x6_dual_fwd: the dual form takes no residual");
    if (stride2 < 1 || (long long)(Ho - 1) * stride2 >= H2 || (long long)(Wo - 1) * stride2 >= W2)
        return fail(VATL_EINVAL, "gemm1x1_bf16x6_dual_fwd: stride %d does not map %dx%d onto %dx%d", stride2, Ho, Wo, H2, W2);
    const long long M = (long long)N * Ho * Wo, x2e = (long long)N * H2 * W2 * C2;
    if (C1 <= 0 || C2 <= 0 || !x6_shape_ok(M, C1 + C2, C1, Cout) || x2e >= (1LL << 30))
        return fail(VATL_EINVAL, "gemm1x1_bf16x6_dual_fwd: %lld x (%d + %d) -> %d is outside C1 %% 64 == 0, C2 %% 64 == 0, K >= 384, N %% 128 == 0 and 32-bit offsets", M, C1, C2, Cout);
    ConvParams p{};
    p.x = a; p.x2 = x; p.w = u; p.bias = bias; p.y = y;
    p.N = N; p.H = Ho; p.W = Wo; p.Cin = C1; p.Cout = Cout; p.CoutPad = Cout;
    p.R = 1; p.S = 1; p.stride = 1;
    p.Ho = Ho; p.Wo = Wo; p.M = (int)M;
    p.OH = Ho; p.OW = Wo; p.osy = 1; p.osx = 1;
    p.relu = relu;
    p.k1 = C1 / BK; p.C2 = C2; p.H2 = H2; p.W2 = W2; p.stride2 = stride2;
    p.kpr = (C1 + C2) / BK; p.ktiles = p.kpr; p.K = C1 + C2;
    p.x_bytes = (unsigned)(M * C1 * 4); p.x2_bytes = (unsigned)(x2e * 4); p.y_bytes = (unsigned)(M * Cout * 4); p.w_bytes = (unsigned)(6LL * Cout * p.K);
    p.d_HoWo = make_fastdiv((unsigned)(Ho * Wo)); p.d_Wo = make_fastdiv((unsigned)Wo);
    return launch_x6_impl<true, false>(p, (hipStream_t)stream);
}
