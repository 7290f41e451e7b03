// Host-only check of what the two F(4x3,2x2) entry points admit (stand-alone, needs no GPU; meant to be built with a host sanitizer):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Ivatl4pose-wacv2024_amd/csrc \
//         tools/probes/wino43_range_check.hip vatl4pose-wacv2024_amd/csrc/{winograd_deconv43,winograd_s2_43,runtime}.hip -o /tmp/wino43_range_check
//   /tmp/wino43_range_check
//
// It calls vatl_deconv4x4s2_winograd43_supported / vatl_conv3x3s2_winograd43_supported over a grid of shapes that straddles every 32-bit-offset
// bound and compares with the bounds restated here in 128-bit integers, then w43_in_range (csrc/winograd43.h) one step inside and outside each
// bound.  Exit status 0 and "ok" = all agree (and the sanitizer saw no overflow on the way).
#include "winograd43.h"

#include <cstdio>

using namespace vatl;
typedef __int128 i128;

static int bad = 0;
static void expect(bool got, bool want, const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0, long long e = 0) {
    if (got != want) { std::printf("MISMATCH %s (%lld %lld %lld %lld %lld): got %d, want %d\n", what, a, b, c, d, e, (int)got, (int)want); ++bad; }
}

// the bounds of csrc/winograd43.h restated: offsets of x up to 0xFFFF0000 bytes, y < 2^32 bytes, packed filter < 2^30 bytes, tiles < 2^30,
// stages < 1024, grid < 2^31 blocks
static bool admit(i128 mt, i128 xe, i128 ye, i128 ue, int Cin, i128 units) {
    return xe * 4 <= (i128)0xFFFF0000u && ye * 4 < ((i128)1 << 32) && ue * 4 < ((i128)1 << 30) && mt < ((i128)1 << 30) && Cin / 16 < 1024 &&
           (mt + 31) / 32 * units < ((i128)1 << 31);
}

int main() {
    const int Ns[] = {-1, 0, 1, 2, 5, 1024, 65535, 65536, 1 << 20, 1 << 24, 0x7FFFFFFF};
    const int Hs[] = {0, 4, 8, 12, 16, 64, 1024, 4096, 32768};
    const int Ws[] = {0, 3, 6, 12, 24, 48, 768, 3072, 24576};
    const int Cs[] = {0, 8, 16, 48, 64, 2048, 16368, 16384, 32768};
    const int Os[] = {0, 32, 64, 192, 2048, 16384, 1 << 20};
    long checked = 0;
    for (int N : Ns) for (int H : Hs) for (int W : Ws) for (int C : Cs) for (int O : Os) {
        const bool pos = N > 0 && H > 0 && W > 0 && C > 0 && O > 0;
        const i128 n = N;
        const bool d = pos && H % 4 == 0 && W % 3 == 0 && C % 16 == 0 && O % 64 == 0 &&
                       admit(n * (H / 4) * (W / 3), n * H * W * C, 4 * n * H * W * O, (i128)20 * O * C, C, O / 64 * 4);
        expect(vatl_deconv4x4s2_winograd43_supported(N, H, W, C, O) != 0, d, "deconv4x4s2_winograd43_supported", N, H, W, C, O);
        const bool s = pos && H % 8 == 0 && W % 6 == 0 && C % 16 == 0 && O % 64 == 0 &&
                       admit(n * (H / 8) * (W / 6), n * H * W * C, n * (H / 2) * (W / 2) * O, (i128)72 * O * C, C, O / 64);
        expect(vatl_conv3x3s2_winograd43_supported(N, H, W, C, O) != 0, s, "conv3x3s2_winograd43_supported", N, H, W, C, O);
        checked += 2;
    }
    // one step inside / outside each bound of the factored check
    const long long XE = 0xFFFF0000u / 4, Y = 1LL << 30, U = 1LL << 28, MT = 1LL << 30;
    expect(w43_in_range(32, XE, Y - 1, U - 1, 16368, 4), true, "all bounds met");
    expect(w43_in_range(32, XE + 1, 1, 1, 16, 1), false, "x one element over");
    expect(w43_in_range(32, 1, Y, 1, 16, 1), false, "y at 2^30 elements");
    expect(w43_in_range(32, 1, 1, U, 16, 1), false, "u at 2^28 elements");
    expect(w43_in_range(MT - 1, 1, 1, 1, 16, 63), true, "tiles just under 2^30, grid just under 2^31");
    expect(w43_in_range(MT - 1, 1, 1, 1, 16, 64), false, "grid at 2^31 blocks");
    expect(w43_in_range(MT, 1, 1, 1, 16, 1), false, "tiles at 2^30");
    expect(w43_in_range(32, 1, 1, 1, 16384, 1), false, "1024 stages");
    std::printf("%s: %ld entry-point calls, %d mismatches\n", bad ? "FAILED" : "ok", checked, bad);
    return bad ? 1 : 0;
}
