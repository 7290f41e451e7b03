// Host check of csrc/split16.h, the split arithmetic of the bf16x6 GEMM route (stand-alone, no GPU):
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Ivatl4pose-wacv2024_amd/csrc tools/split16_check.cpp -o split16_check
//     ./split16_check          (tests/test_split16_cpu.py builds and runs it without the sanitizer flags)
// For every input: hi + mid + lo == a bit for bit (summed in either order), every piece has zero low 16 bits (|a| >= 2^-100 and zeros; below
// that the low bits the pack cuts off mid / lo amount to less than 2^-132, split16.h), |mid| <= 2^-7 |hi| and |lo| <= 2^-7 |mid| where those
// are non-zero, and pack_pair / bf16_bits put the pieces where the MFMA fragment wants them.
// Inputs: 2^24 random finite bit patterns (xorshift, fixed seed), every pattern with 13 random high bits against all low 16 bits = 0 /
// all ones, and the edge values 0, -0, 1 +- ulp, FLT_MAX, the smallest normal, the largest and smallest subnormal, each with both signs.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "split16.h"

static long g_bad = 0;

static void check(float a) {
    using namespace split16;
    const Pieces p = split3(a);
    const uint32_t ua = bits_of(a), uh = bits_of(p.hi), um = bits_of(p.mid), ul = bits_of(p.lo);
    const float back1 = (p.hi + p.mid) + p.lo, back2 = p.hi + (p.mid + p.lo);
    bool ok = (uh & 0xFFFFu) == 0;
    if (std::fabs(a) >= kSplitExactMin || a == 0.f) {
        ok = ok && (um & 0xFFFFu) == 0 && (ul & 0xFFFFu) == 0;
        ok = ok && (p.mid == 0.f || std::fabs(p.mid) <= std::ldexp(std::fabs(p.hi), -7));
        ok = ok && (p.lo == 0.f || std::fabs(p.lo) <= std::ldexp(std::fabs(p.mid), -7));
    } else {                                          // tiny values: what the pack cuts off mid / lo is below 2^-132 (split16.h)
        const double packed = (double)p.hi + (double)trunc16(p.mid) + (double)trunc16(p.lo);
        ok = ok && std::fabs((double)a - packed) < std::ldexp(1.0, -132);
    }
    ok = ok && ((bits_of(back1) == ua && bits_of(back2) == ua) || (ua == 0x80000000u && uh == ua && back1 == 0.f && back2 == 0.f));   // (-0) + (+0) = +0: the sign lives in hi
    ok = ok && pack_pair(p.hi, p.mid) == ((uh >> 16) | (um & 0xFFFF0000u)) && pack_pair(p.lo, p.hi) == ((ul >> 16) | uh);
    ok = ok && bf16_bits(p.hi) == (uint16_t)(ua >> 16);
    if (!ok && g_bad++ < 10)
        std::printf("FAIL a = %a (0x%08x): hi 0x%08x mid 0x%08x lo 0x%08x, sum 0x%08x / 0x%08x\n", (double)a, ua, uh, um, ul, bits_of(back1), bits_of(back2));
}

int main() {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 32); };
    long n = 0;
    for (long i = 0; i < (1L << 24); ++i) {
        const uint32_t u = next();
        if ((u & 0x7F800000u) == 0x7F800000u) continue;         // infinities and NaNs: documented in split16.h, not part of the identity
        check(split16::float_of(u)); ++n;
    }
    for (long i = 0; i < (1L << 13); ++i) {
        const uint32_t u = next() & 0xFFFF0000u;
        if ((u & 0x7F800000u) == 0x7F800000u) continue;
        check(split16::float_of(u)); check(split16::float_of(u | 0xFFFFu)); check(split16::float_of(u | 0x00FFu)); check(split16::float_of(u | 0xFF00u)); n += 4;
    }
    const float edges[] = {0.f, 1.f, std::nextafterf(1.f, 2.f), std::nextafterf(1.f, 0.f), FLT_MAX, FLT_MIN, std::nextafterf(FLT_MIN, 0.f),
                           split16::float_of(1u), split16::float_of(0x0000FFFFu), split16::float_of(0x00010000u), 3.14159274f, 1.0f / 3.0f};
    for (float e : edges) { check(e); check(-e); n += 2; }
    // what the header says of an infinity: the row turns into NaN through inf - inf
    const split16::Pieces inf = split16::split3(INFINITY);
    if (!(std::isinf(inf.hi) && std::isnan(inf.mid) && std::isnan(inf.lo))) { std::printf("FAIL: split3(inf) is not (inf, NaN, NaN)\n"); ++g_bad; }
    // -0 keeps its sign in hi
    if (split16::bits_of(split16::split3(-0.f).hi) != 0x80000000u) { std::printf("FAIL: split3(-0).hi is not -0\n"); ++g_bad; }
    std::printf("split16_check: %ld values, %ld failures\n", n, g_bad);
    return g_bad ? 1 : 0;
}
