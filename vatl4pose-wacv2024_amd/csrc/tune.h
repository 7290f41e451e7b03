// The setters behind vatl_tune_set (tune.hip): each knob's storage lives in the file whose launcher reads it.  Every owning file
// includes this header, so the compiler checks a declaration against its definition.  Internal hooks, not part of the C ABI:
// hidden visibility, C++ linkage.  Range checks are vatl_tune_set's; a setter that checks its own value returns non-zero on refusal.
#pragma once

namespace vatl {
#pragma GCC visibility push(hidden)
int igemm_set_schedule(int v);                                 // conv_igemm.hip: knob 0
int igemm_set_order(int v);                                    //   1
int igemm_set_stagger(int v);                                  //   2
int igemm_set_tile_rows(int v);                                //   5
int igemm_set_ablate(int bits);                                //   6
int igemm_set_splitk_policy(int v);                            //   9
int persistent_set_kmax(int v);                                // gemm1x1_persistent.h: knob 7
int persistent_set_dist(int v);                                //   10
int streamk_set_enable(int v);                                 // conv_streamk.hip: knob 12
int ring_set_enable(int v);                                    // gemm1x1_ring.hip: knob 27
int conv3x3_halo_enable(int on);                               // conv3x3_halo.hip
int wino_set_ablate(int bits);                                 // conv_winograd.hip
int wino_set_group_kb(int v);
int wino_set_halves(int v);
int wino_set_persist(int v);
int wino_set_persist_pf(int v);
int wino_wgrad_set_halves(int v);                              // winograd_wgrad.hip
int wino_wgrad_set_table(int v);
int wino_wgrad_set_blocks(int v);
int tune_wgrad_blocks(int blocks);                             // conv_wgrad.hip
int crop_tune_px(int px);                                      // crop.hip
#pragma GCC visibility pop
}  // namespace vatl
