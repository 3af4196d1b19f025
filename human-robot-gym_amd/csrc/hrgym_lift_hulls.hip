// hrgym_lift_hulls.hip -- the lifting kernels (hrgym_lift.hip: CollaborativeLiftingCart) compiled once more with the arm links' CONVEX HULLS as collision geometry
// (hrg_model_desc.robot_hulls = 1): the link x human and link x plane pairs run the hull narrowphase (GJK, lowest point), the link x board pairs of pass 0 of the
// box narrowphase the hull - box penetration by MPR (hrgym_hull.h), one contact per pair; the table slab x board pair stays box - box.  Its own translation unit,
// so the capsule-geometry lifting kernels carry none of it.
#define HRG_BOX 1
#define HRG_LIFT 1
#define HRG_HULLS 1
#include "hrgym_hip.hip"
