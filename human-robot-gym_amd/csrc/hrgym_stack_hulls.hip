// hrgym_stack_hulls.hip -- the stacking kernels (hrgym_stack.hip: CollaborativeStackingCart) compiled once more with the arm links' CONVEX HULLS as collision
// geometry (hrg_model_desc.robot_hulls = 1): the link x human and link x plane pairs run the hull narrowphase (GJK, lowest point), a link x cube pair of
// collide_cubes the hull - box penetration by MPR against that cube (hrgym_hull.h), one contact per pair; the finger and gripper capsules stay capsules.  Its own
// translation unit, so the capsule-geometry stacking kernels carry none of it.
#define HRG_STACK 1
#define HRG_HULLS 1
#undef HRG_WG_WAVES
#define HRG_WG_WAVES 1   // as hrgym_stack.hip: one env per workgroup
#include "hrgym_hip.hip"
