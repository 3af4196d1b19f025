// hrgym_hammer_hulls.hip -- the hammering kernels (hrgym_hammer.hip: CollaborativeHammeringCart) compiled once more with the arm links' CONVEX HULLS as collision
// geometry (hrg_model_desc.robot_hulls = 1): the link x human and link x plane pairs run the hull narrowphase (GJK, lowest point), a link x {board, hammer head,
// nail head} pair of collide_hammer the hull - box penetration by MPR with that geom's own extents and pose (hrgym_hull.h), one contact per pair.  Its own
// translation unit, so the capsule-geometry hammering kernels carry none of it.
#define HRG_HAMMER 1
#define HRG_HULLS 1
#undef HRG_WG_WAVES
#define HRG_WG_WAVES 1   // as hrgym_hammer.hip: one env per workgroup
#include "hrgym_hip.hip"
