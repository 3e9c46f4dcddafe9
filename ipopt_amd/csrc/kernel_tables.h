// kernel_tables.h -- the records of the launch tables the kernels read (built on the host by launch_plan.cpp, uploaded by numeric.hip).
// Plain structs, one definition for the host-only launch plan and for the kernels.
#pragma once

namespace mi355x {

// per-front / per-child records in LAUNCH order: one 64-byte load replaces a chain of 4-5 dependent index loads at the
// head of every front kernel (each of them an HBM/MALL round trip on the critical path of a tree level)
struct FrontMeta { int s, c0, k, r0, m, aq0, aq1, ch0, ch1, alias; long long panel_off, cb_off, minv_off; int ldp, ldt;
                   long long cv, wb, gpart; int gbase, gpos, grem, gcols, split, ttab, ttab2, solo, selfasm, bigidx, tfuse, asmcut; };
// (bigidx: the front's slot in the per-big-front arrays (isg); tfuse: the contribution block is ASSEMBLED BY ITS UPDATE -- k_big_schur64 writes
//  T = sum of the children - L21 W21^T once; the assembly kernels leave the T columns alone)
// one front of a leaf chain, everything the chain kernels need of it in one record (the chain's records lie side by side: the next link's is requested a link ahead)
struct LeafLink { int s, c0, k, m, aq0, aq1, relbase, ldp, r0, pad; long long panel_off, minv_off, cb_off, cv; };
struct ChildMeta { int ch, mc, relbase, owner; long long cb_off; int ldt, aliased; long long cvbase, inv; int rlo, rhi; };      // rlo / rhi: first / last row of the PARENT's front the child's update rows map to
// one link of a chain group as seen from a later link of the same group (trailing update, fused solves)
struct GroupLink { long long panel_off, wb, minv_off, cv, tr; int c0, k, m, ldp, r0, ch0, ch1, alias; long long t_off; int ldt, s, selfasm, aq0, aq1, bigidx; };     // t_off/ldt: the link's trailing block (V.cb + t_off)

// Sync-free triangular solves along pure in-place separator chains (a run of consecutive tree levels whose fronts are all chain
// links): ONE launch per sweep for the whole run instead of 1 (forward) / 2 (backward) launches per level.  One workgroup per link
// (+ one per 64 rows beyond the chain in the forward sweep); a link's workgroup waits on a flag for each earlier (forward) / later
// (backward) link, applies that link's 64 x 64 block of the panel to its own rows, then solves with its pivot block and raises its
// own flag -- the point-to-point pipeline of a "synchronisation-free" sparse triangular solve (Liu et al., Euro-Par 2016).
struct ChainLink { long long panel_off, minv_off; int c0, k, ldp, s, r0, koff, fi, pad1; };      // links of all chains, chain by chain, bottom link first; fi: slot of the link's flags
struct ChainDesc { long long cvb; int link0, nlinks, tail, ktot, wg0f, wg0b;       // cvb: chain vector base, ktot: columns of the chain, wg0*: first workgroup (within the segment's launch)
                   int ch0, ch1, alias0, s0, init, gw0, gw1, tf0, pw0, pw1, dot0, pad0; };         // first link: children (cmeta range), in place on a child's vector, supernode; init: see launch_plan.cpp;
                                                                                       // gw0..gw1: tail flags (chwait) awaited before the first link's children are gathered; tf0: own tail flags;
                                                                                       // pw0..pw1: backward, link flags (chwait) of the parent's chain; dot0: first dot workgroup (flags, partial sums)
struct DfLevel { int b0, n16, nb, q0; };      // k_front_df: a level's bucket of one-wavefront fronts: first launch-list entry, fronts of order <= 16 (they come first), all fronts; its first virtual workgroup

}  // namespace mi355x
