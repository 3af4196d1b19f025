// hrgym_handover_hulls.hip -- the handover kernels (hrgym_handover.hip: HumanRobotHandoverCart, RobotHumanHandoverCart) compiled once more with the arm links'
// CONVEX HULLS as collision geometry (hrg_model_desc.robot_hulls = 1): the link x human and link x plane pairs run the hull narrowphase (GJK, lowest point) and the
// link x cube pairs of pass 0 of the cube narrowphase the hull - box penetration by MPR (hrgym_hull.h), one contact per pair, in both physics passes of a cycle.
// Its own translation unit, so the capsule-geometry handover kernels carry none of it.
#define HRG_BOX 1
#define HRG_HANDOVER 1
#define HRG_HULLS 1
#ifndef HRG_BOX_WAVES
#define HRG_BOX_WAVES 2   // as hrgym_handover.hip: two waves per SIMD (the two-pass cycle body spills at three)
#endif
#include "hrgym_hip.hip"
