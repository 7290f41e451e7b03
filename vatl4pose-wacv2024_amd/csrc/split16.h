// The truncating three-way split of a float into bf16 pieces, and the packing of pieces into bf16 pairs: the arithmetic of the
// bf16x6 GEMM route (gemm1x1_bf16x6.hip) and of its filter pack.  Host- and device-callable, no HIP types: tools/split16_check.cpp
// includes this file alone.
//
//   hi  = a truncated to its 8 leading significant bits (the float's bit pattern with the low 16 bits cleared);
//   mid = (a - hi) truncated the same way;   lo = (a - hi) - mid.
// Both subtractions are exact (the operands share their leading bits), and the second remainder holds at most the 8 bits that are
// left of the 24, so it is a bf16 itself: hi + mid + lo == a bit for bit, and every piece has zero low 16 bits.  That holds for
// zeros (-0 gives hi = -0, mid = lo = +0), for FLT_MAX and for every |a| >= 2^-100 (kSplitExactMin).
//
// What the route does with values outside that:
//  * an infinity: hi = a, a - hi = inf - inf = NaN, so every output of the row that reads it is NaN; a NaN stays a NaN in mid / lo
//    (its hi piece may read as an infinity when the payload sits in the low 16 bits).  Either way the row is NaN, as after fp32 inf * 0.
//  * tiny values, |a| < 2^-100: a remainder below 2^-126 is a subnormal float, whose spacing 2^-149 is finer than the bf16 subnormal
//    spacing 2^-133.  hi + mid + lo == a still holds in floats, but mid / lo may carry low bits, which pack_pair cuts off: the packed
//    pieces miss less than 2^-132 of a, and the matrix pipe may flush subnormal pieces altogether (less than 2^-125).  No three bf16
//    values can do better.  Against products that are accumulated in fp32 next to terms of ordinary size this is nothing.
//  * the kernel must run with fp32 denormals kept (hipcc's default) for the subtractions to be exact on subnormal remainders.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPLIT16_FN __host__ __device__ inline
#else
#define SPLIT16_FN inline
#endif

namespace split16 {

constexpr float kSplitExactMin = 7.8886090522101181e-31f;   // 2^-100: from here up the three pieces are bf16 values exactly

SPLIT16_FN uint32_t bits_of(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, f);
#else
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
#endif
}
SPLIT16_FN float float_of(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(float, u);
#else
    float f;
    std::memcpy(&f, &u, 4);
    return f;
#endif
}

// a with its low 16 bits cleared: the bf16 below it in magnitude (truncation), still a float
SPLIT16_FN float trunc16(float a) { return float_of(bits_of(a) & 0xFFFF0000u); }

struct Pieces {
    float hi, mid, lo;
};

SPLIT16_FN Pieces split3(float a) {
    Pieces p;
    p.hi = trunc16(a);
    const float r1 = a - p.hi;
    p.mid = trunc16(r1);
    p.lo = r1 - p.mid;
    return p;
}

// two pieces (each with zero low 16 bits) as one bf16 pair: `even` in the low half (fragment element 2d), `odd` in the high half
SPLIT16_FN uint32_t pack_pair(float even, float odd) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(bits_of(odd), bits_of(even), 0x07060302u);   // one v_perm_b32: bytes 3, 2 of odd | bytes 3, 2 of even
#else
    return (bits_of(even) >> 16) | (bits_of(odd) & 0xFFFF0000u);
#endif
}

// the bf16 bit pattern of a piece
SPLIT16_FN uint16_t bf16_bits(float piece) { return (uint16_t)(bits_of(piece) >> 16); }

}  // namespace split16
