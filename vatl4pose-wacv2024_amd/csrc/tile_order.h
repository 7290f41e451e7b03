// Which tile a block computes: the XCD-contiguous block index and the grouped (m-tile, filter slice) order of the Winograd kernels.
#pragma once
#include "common.h"

namespace vatl {

// XCD-aware tile order: the hardware deals the blocks of a launch round-robin over the eight XCDs (block b runs on XCD b % 8), each with an
// L2 of its own.  This maps block b of nblk to position t of the launch's tile sequence such that every XCD gets a CONTIGUOUS run of the
// sequence — neighbours in the sequence, which share an operand panel, then run at the same time on the same L2.  Bijective for any grid
// size: the first nblk % 8 XCDs get one block more.
__device__ __forceinline__ int xcd_contiguous_index(int bid, int nblk) {
    const int xcd = bid & 7, loc = bid >> 3, q8 = nblk >> 3, r8 = nblk & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
}

// Grouped order of the Winograd kernels: position t of
//     for (group of rn filter slices) for (m-tile) for (slice in the group)        slice = what a block takes of the filter, `units` in all
// so the blocks that are resident together read the same input tiles (fetched from HBM once per group instead of once per slice) while
// the group's filter slices (sized by the launcher to <= 2 MB) stay in that XCD's L2 for the whole sweep over the m-tiles.  The last
// group may be smaller.  P: a parameter struct with m_tiles, rn and the divisors d_grp (by m_tiles * rn), d_rn, d_rn_last.
template <class P>
__device__ __forceinline__ void grouped_tile(const P& p, int t, int units, int& m_tile, int& unit) {
    const int grp = fdiv(t, p.d_grp), rem = t - grp * (p.m_tiles * p.rn);
    const bool last_grp = units - grp * p.rn < p.rn;
    const int rn_g = last_grp ? units - grp * p.rn : p.rn;
    m_tile = fdiv(rem, last_grp ? p.d_rn_last : p.d_rn);
    unit = grp * p.rn + (rem - m_tile * rn_g);
}
// ... and the launcher's side of it (p.m_tiles set before)
template <class P>
inline void set_grouped_order(P& p, int units, int rn) {
    p.rn = rn;
    p.d_grp = make_fastdiv((unsigned)(p.m_tiles * p.rn));
    p.d_rn = make_fastdiv(p.rn);
    p.d_rn_last = make_fastdiv(units % p.rn ? units % p.rn : p.rn);
}

}  // namespace vatl
