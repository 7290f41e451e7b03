// Does a SIMD's matrix pipe run one wave's MFMAs while its vector ALU runs another wave's (or the same wave's) ordinary vector instructions?
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/mfma_valu_overlap tools/probes/mfma_valu_overlap.hip && /tmp/mfma_valu_overlap
// Each block = WAVES waves on one CU (WAVES / 4 per SIMD); every wave runs ITER rounds of [MF independent MFMAs (f32 16x16x4: 32 cycles each, or 32x32x2: 64)] and
// [VA dependent-free v_fma_f32].  Reported: cycles per round per SIMD against MF x passes and VA x 4.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int MF, int VA, bool BIG, bool SPLIT>
__global__ __launch_bounds__(512) void probe(float* out, int iters) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 acc[8];
    f32x16 accb[2];
    for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 2; ++i) for (int e = 0; e < 16; ++e) accb[i][e] = 0.f;
    float v[8];
    for (int i = 0; i < 8; ++i) v[i] = (float)(lane + i);
    const float a = 1.0f + lane * 1e-3f, b = 0.5f;
    // SPLIT: even waves of a SIMD pair only do MFMAs, odd waves only vector instructions (different waves); otherwise every wave does both
    const bool do_m = !SPLIT || ((wave >> 2) & 1) == 0, do_v = !SPLIT || ((wave >> 2) & 1) == 1;
    for (int it = 0; it < iters; ++it) {
        if (do_m) {
#pragma unroll
            for (int k = 0; k < MF; ++k) {
                if constexpr (BIG) accb[k & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, accb[k & 1], 0, 0, 0);
                else acc[k & 7] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[k & 7], 0, 0, 0);
            }
        }
        if (do_v) {
#pragma unroll
            for (int k = 0; k < VA; ++k) v[k & 7] = __builtin_fmaf(v[k & 7], 1.0001f, 0.5f);
        }
    }
    float s = 0.f;
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][3] + v[i];
    s += accb[0][0] + accb[1][5];
    out[blockIdx.x * 512 + threadIdx.x] = s;
}

template <int MF, int VA, bool BIG, bool SPLIT>
static void run(const char* name, int waves) {
    float* out;
    hipMalloc(&out, 256 * 512 * sizeof(float));
    const int iters = 2000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    probe<MF, VA, BIG, SPLIT><<<256, waves * 64>>>(out, 10);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    probe<MF, VA, BIG, SPLIT><<<256, waves * 64>>>(out, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    const double wps = waves / 4.0;                                  // waves per SIMD
    const double per_round_us = ms * 1e3 / iters;
    printf("%-58s %d waves/SIMD: %8.3f us per round per wave-set\n", name, (int)wps, per_round_us);
    hipFree(out);
}

// ---- the same question for v_mfma_f32_32x32x16_bf16 (32 cycles per SIMD, of which it holds the vector issue for 8) and the REAL vector work of the bf16x6
// GEMM's stage: the three-way split of 16 floats per lane (csrc/split16.h: 32 v_and_b32, 32 v_sub_f32, 24 v_perm_b32 = 88) on random data, beside the 24 MFMAs
// of a stage on two accumulator sets of 64 registers.  A round splits x into the pieces that the NEXT round's MFMAs read (two register sets, ping-pong), so
// the split can neither be hoisted nor dropped.  MODE 0: MFMAs alone; 1: split alone; 2: the split, then the 24 MFMAs (the k-loop of gemm1x1_bf16x6_body
// before the pipelining); 3: the same wave, the split's instructions between the MFMAs, VALU_PER_GAP in each gap (sched_group_barrier); 4: MFMAs in one wave
// of a SIMD, the split in the other (8 waves).  Reported: shader cycles per round of wave 0 (s_memtime) and us per round.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct Pieces16 { u32x4 p0[2], p1[2], p2[2]; };

__device__ __forceinline__ unsigned perm_pair(float even, float odd) {
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, odd), __builtin_bit_cast(unsigned, even), 0x07060302u);
}

__device__ __forceinline__ void split16_lane(const float (&x)[16], Pieces16& q) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            float hi[2], mid[2], lo[2];
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const float a = x[8 * i + 2 * d + o];
                hi[o] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, a) & 0xFFFF0000u);
                const float r1 = a - hi[o];
                mid[o] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, r1) & 0xFFFF0000u);
                lo[o] = r1 - mid[o];
            }
            q.p0[i][d] = perm_pair(hi[0], hi[1]);
            q.p1[i][d] = perm_pair(mid[0], mid[1]);
            q.p2[i][d] = perm_pair(lo[0], lo[1]);
        }
}

__device__ __forceinline__ f32x16 mfma16(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

template <int MODE, int VALU_PER_GAP>
__global__ __launch_bounds__(512) void probe16(const float* __restrict__ in, float* out, long long* cyc, int iters) {
    const int wave = threadIdx.x >> 6;
    const bool do_m = MODE == 0 || MODE == 2 || MODE == 3 || (MODE == 4 && ((wave >> 2) & 1) == 0);
    const bool do_v = MODE == 1 || MODE == 2 || MODE == 3 || (MODE == 4 && ((wave >> 2) & 1) == 1);
    float x[16];
    for (int i = 0; i < 16; ++i) x[i] = in[(threadIdx.x * 16 + i) & 8191];
    u32x4 bw[3][2];
    for (int pl = 0; pl < 3; ++pl)
        for (int j = 0; j < 2; ++j)
            for (int d = 0; d < 4; ++d) bw[pl][j][d] = __builtin_bit_cast(unsigned, in[(threadIdx.x * 24 + pl * 8 + j * 4 + d + 4096) & 8191]) & 0x3F803F80u;
    f32x16 acc[2][2], sml[2][2];
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; sml[i][j][e] = 0.f; }
    Pieces16 P, Q;
    split16_lane(x, P);
    Q = P;
    auto round = [&](const Pieces16& cur, Pieces16& nxt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(x[i]));          // opaque: the split is this round's work
        if (do_v) split16_lane(x, nxt);
        if (do_v && !do_m) {                                                  // no MFMA reads the pieces in this wave: keep every round's split alive
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int d = 0; d < 4; ++d) asm volatile("" :: "v"(nxt.p0[i][d]), "v"(nxt.p1[i][d]), "v"(nxt.p2[i][d]));
        }
        if (do_m) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(cur.p0[i], bw[0][j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) sml[i][j] = mfma16(cur.p0[i], bw[1][j], sml[i][j]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) sml[i][j] = mfma16(cur.p1[i], bw[0][j], sml[i][j]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) sml[i][j] = mfma16(cur.p1[i], bw[1][j], sml[i][j]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) sml[i][j] = mfma16(cur.p0[i], bw[2][j], sml[i][j]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) sml[i][j] = mfma16(cur.p2[i], bw[0][j], sml[i][j]);
        }
        if constexpr (MODE == 3) {
#pragma unroll
            for (int g = 0; g < 24; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x2, VALU_PER_GAP, 0);
            }
        } else if constexpr (MODE == 2) {
            __builtin_amdgcn_sched_group_barrier(0x2, 88, 0);
            __builtin_amdgcn_sched_group_barrier(0x8, 24, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; it += 2) {
        round(P, Q);
        round(Q, P);
    }
    const long long t1 = __builtin_readcyclecounter();
    float s = 0.f;
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) s += acc[i][j][0] + sml[i][j][7];
    s += __builtin_bit_cast(float, P.p0[0][0] ^ P.p1[1][1] ^ P.p2[0][3] ^ Q.p0[1][2] ^ Q.p2[1][0]);
    out[blockIdx.x * 512 + threadIdx.x] = s;
    if (blockIdx.x == 0 && threadIdx.x == 0) cyc[0] = t1 - t0;
}

template <int MODE, int VALU_PER_GAP>
static void run16(const char* name, int waves, const float* in) {
    float* out;
    long long* cyc;
    hipMalloc(&out, 256 * 512 * sizeof(float));
    hipMalloc(&cyc, sizeof(long long));
    const int iters = 2000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    probe16<MODE, VALU_PER_GAP><<<256, waves * 64>>>(in, out, cyc, 10);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    probe16<MODE, VALU_PER_GAP><<<256, waves * 64>>>(in, out, cyc, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    long long c = 0;
    hipMemcpy(&c, cyc, sizeof(c), hipMemcpyDeviceToHost);
    printf("%-66s %d waves/SIMD: %8.1f cycles per round of a wave  %7.3f us per round\n", name, waves / 4, (double)c / iters, ms * 1e3 / iters);
    hipFree(out); hipFree(cyc);
}

static void bf16_cases() {
    std::vector<float> h(8192);
    unsigned s = 12345u;
    for (auto& v : h) {                                                     // uniform in (-2, 2), full mantissas
        s = s * 1664525u + 1013904223u;
        v = ((int)(s >> 8) - (1 << 23)) * (1.f / (1 << 22));
    }
    float* in;
    hipMalloc(&in, h.size() * sizeof(float));
    hipMemcpy(in, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    printf("-- 32x32x16 bf16 MFMA (32 cycles), 24 per round = 768 cycles alone; the bf16x6 split of 16 floats: 88 vector instructions = 352 cycles of issue\n");
    run16<0, 0>("warm-up", 8, in);
    for (int waves : {4, 8}) {
        if (waves == 4) {
            run16<0, 0>("24 MFMA alone", 4, in);
            run16<1, 0>("88-instruction split alone", 4, in);
            run16<2, 0>("split, then 24 MFMA (burst, burst), same wave", 4, in);
            run16<3, 3>("same wave, 3 split instructions in every MFMA gap (+16 behind)", 4, in);
            run16<3, 4>("same wave, 4 split instructions in every MFMA gap (22 gaps)", 4, in);
            run16<3, 5>("same wave, 5 split instructions in every MFMA gap (18 gaps)", 4, in);
        } else {
            run16<0, 0>("24 MFMA alone", 8, in);
            run16<1, 0>("88-instruction split alone", 8, in);
            run16<2, 0>("split, then 24 MFMA (burst, burst), every wave", 8, in);
            run16<3, 3>("every wave, 3 split instructions in every MFMA gap (+16 behind)", 8, in);
            run16<3, 4>("every wave, 4 split instructions in every MFMA gap (22 gaps)", 8, in);
            run16<3, 5>("every wave, 5 split instructions in every MFMA gap (18 gaps)", 8, in);
            run16<4, 0>("24 MFMA in one wave, the split in the OTHER wave of the SIMD", 8, in);
        }
    }
    hipFree(in);
}

int main() {
    bf16_cases();
    // clocks warm-up
    run<64, 0, false, false>("warm-up", 8);
    printf("-- 16x16x4 f32 MFMA (8 passes = 32 cycles), 64 per round = 2048 cycles alone; v_fma 4 cycles each\n");
    run<64, 0, false, false>("64 MFMA, 0 vector, every wave", 4);
    run<64, 0, false, false>("64 MFMA, 0 vector, every wave", 8);
    run<0, 256, false, false>("0 MFMA, 256 vector (1024 cycles), every wave", 4);
    run<0, 256, false, false>("0 MFMA, 256 vector, every wave", 8);
    run<64, 256, false, false>("64 MFMA + 256 vector in the SAME wave", 4);
    run<64, 256, false, false>("64 MFMA + 256 vector in every wave", 8);
    run<64, 256, false, true>("64 MFMA in one wave, 256 vector in the OTHER wave of the SIMD", 8);
    run<64, 512, false, true>("64 MFMA in one wave, 512 vector in the OTHER wave of the SIMD", 8);
    printf("-- 32x32x2 f32 MFMA (16 passes = 64 cycles), 32 per round = 2048 cycles alone\n");
    run<32, 0, true, false>("32 MFMA, 0 vector, every wave", 4);
    run<32, 256, true, false>("32 MFMA + 256 vector in the SAME wave", 4);
    run<32, 256, true, true>("32 MFMA in one wave, 256 vector in the OTHER wave of the SIMD", 8);
    run<32, 512, true, true>("32 MFMA in one wave, 512 vector in the OTHER wave of the SIMD", 8);
    return 0;
}
