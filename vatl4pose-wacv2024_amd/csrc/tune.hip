// vatl_tune_set: the knob switchboard of the whole library.  The storage of a knob lives with the launcher that reads it (tune.h).
#include "common.h"
#include "tune.h"

#include <cstdlib>

using namespace vatl;

extern "C" int vatl_tune_set(int knob, int value) {
    // PRODUCT KNOBS — process-global route selectors (relaxed atomics; set them before launching from several threads).  Every accepted
    // value computes the SAME BITS as the default (tests/test_gpu_conv.py, tests/test_gpu_winograd.py assert it per knob); the table in
    // include/vatl_hip.h is the contract.  Nothing else is accepted by the shipped library.
    switch (knob) {
    case 0:  if (value == 0 || value == 2 || value == 4 || value == 5) return igemm_set_schedule(value); break;
    case 1:  if (value == 0 || value == 1) return igemm_set_order(value); break;
    case 5:  if (value == 0 || value == 64 || value == 128) return igemm_set_tile_rows(value); break;
    case 7:  if (value >= 0 && value <= 64) return persistent_set_kmax(value); break;
    case 8:  if (value == 0 || value == 1) return conv3x3_halo_enable(value); break;
    case 10: if (value == 1 || value == 2) return persistent_set_dist(value); break;
    case 18: if (value >= 0 && value <= (1 << 20)) return wino_set_group_kb(value); break;
    case 21: if (value >= 1 && value <= 3) return wino_set_halves(value); break;
    case 22: if (value >= 0 && value <= 4096) return wino_set_persist(value); break;
    case 24: if (value >= 0 && value <= 3) return wino_set_persist_pf(value); break;
    case 25: if (value == 0 || value == 1) return wino_wgrad_set_table(value); break;
    default: break;
    }
#ifdef VATL_ABLATION
    // PROFILING VARIANT ONLY (build.py --ablation -> libvatl_hip_ablation.so): knobs that change the summation order (3, 9, 12, 19) or are not pinned bit-identical (23), performance-only
    // experiments (2, 16, 27) and the ablations that compute WRONG results by construction (0: 10..13, 4, 6, 17; these also need VATL_ALLOW_ABLATION=1).
    const bool wrong = (knob == 0 && value >= 10) || ((knob == 4 || knob == 6 || knob == 17) && value != 0);
    if (wrong) {
        const char* ok = getenv("VATL_ALLOW_ABLATION");
        if (!ok || ok[0] != '1') return fail(VATL_EINVAL, "tune_set: knob %d value %d is a profiling ablation (wrong results); set VATL_ALLOW_ABLATION=1", knob, value);
    }
    if (knob == 0 && value >= 10 && value <= 13) return igemm_set_schedule(value);
    if (knob == 2 && value >= 0 && value <= 200) return igemm_set_stagger(value);
    if (knob == 3 && tune_wgrad_blocks(value) == 0) return 0;
    if (knob == 4 && value >= 0 && value <= 3) return tune_wgrad_blocks(-value - 1);
    if (knob == 6 && value >= 0 && value <= 15) return igemm_set_ablate(value);
    if (knob == 9 && (value == 0 || value == 1)) return igemm_set_splitk_policy(value);
    if (knob == 12 && (value == 0 || value == 1)) return streamk_set_enable(value);
    if (knob == 16 && crop_tune_px(value) == 0) return 0;
    if (knob == 17 && value >= 0 && value <= 63) return wino_set_ablate(value);
    if (knob == 19 && value >= 1 && value <= (1 << 20)) return wino_wgrad_set_blocks(value);
    if (knob == 23 && value >= 1 && value <= 2) return wino_wgrad_set_halves(value);
    if (knob == 27 && (value == 0 || value == 1)) return ring_set_enable(value);
    return fail(VATL_EINVAL, "tune_set: unknown knob %d / value %d", knob, value);
#else
    return fail(VATL_EINVAL, "tune_set: knob %d / value %d is not a product knob (include/vatl_hip.h lists them: 0, 1, 5, 7, 8, 10, 18, 21, 22, 24, 25 — all bit-identical); "
                "knobs that change the summation order, performance experiments and profiling ablations exist only in the variant built with "
                "`build.py --ablation` (-DVATL_ABLATION)", knob, value);
#endif
}
