// hrgym_box_hulls.hip -- the cube kernels (hrgym_box.hip: PickPlaceHumanCart and its Close / Pointing variants, HumanObjectInspectionCart, ReachHuman with its box)
// compiled once more with the arm links' CONVEX HULLS as collision geometry (hrg_model_desc.robot_hulls = 1): the link x human and link x plane pairs run the hull
// narrowphase of the ReachHuman hull variant (GJK, lowest point), the link x cube pairs the hull - cube penetration by MPR (hrgym_hull.h), one contact per pair.
// Its own translation unit, so the capsule-geometry cube kernels carry none of it.
#define HRG_BOX 1
#define HRG_HULLS 1
#include "hrgym_hip.hip"
#include "hrgym_host.h"   // hrg_run_tap, hull_centroids

// ---- test tap (include/hrgym.h: hrg_test_hull_box_queries): the MPR wave routine on its own, one query per wavefront -- tests/test_hull_box*.py compare it with
// a numpy restatement.  Link pose and the cube go through LDS as in the step kernel (kR / kp, bR / bx.pos).
struct HullBoxQuery { double R[9], p[3], bp[3], bR[9], bh[3]; int32_t hull, pad; };
__global__ __launch_bounds__(64) void hrg_test_hull_box_kernel(const double* __restrict__ verts, const int32_t* __restrict__ off, const double* __restrict__ cen,
                                                               const HullBoxQuery* __restrict__ q, int n, double* __restrict__ out) {
  const int k = (int)blockIdx.x, lane = hrg_lane();
  if (k >= n) return;
  Lds& L = g_L;
  if (lane < 9) { L.kR[0][lane] = q[k].R[lane]; L.bR[lane] = q[k].bR[lane]; }
  if (lane < 3) { L.kp[0][lane] = q[k].p[lane]; L.bx.pos[lane] = q[k].bp[lane]; }
  wave_sync();
  const int h = __builtin_amdgcn_readfirstlane(q[k].hull), o0 = __builtin_amdgcn_readfirstlane(off[h]), o1 = __builtin_amdgcn_readfirstlane(off[h + 1]);
  const double bh[3] = {q[k].bh[0], q[k].bh[1], q[k].bh[2]};
  const HullRef H = {verts + 3 * o0, o1 - o0, L.kR[0], L.kp[0]};
  double hc[3], depth, nn[3], pos[3];
  m3mulv(hc, L.kR[0], cen + 3 * h);
  v3add(hc, hc, L.kp[0]);
  const int r = mpr_hull_box_wave(H, hc, L.bR, L.bx.pos, bh, depth, nn, pos);
  if (lane == 0) {
    double* o = out + 9 * (size_t)k;
    o[0] = r == MPR_PENETRATING ? 1.0 : 0.0;
    o[1] = depth;
    for (int a = 0; a < 3; a++) { o[2 + a] = nn[a]; o[5 + a] = pos[a]; }
    o[8] = r == MPR_NOT_CONVERGED ? 0.0 : 1.0;
  }
}
extern "C" int hrg_test_hull_box_queries(const double* verts_host, const int32_t* off_host, const void* queries_host, int32_t n, double* out_host) {
  if (!verts_host || !off_host || !queries_host || !out_host || n <= 0 || off_host[0] != 0) return -1;
  for (int h = 0; h < HRG_NHULL; h++) if (!(off_host[h + 1] > off_host[h] + 3)) return -1;
  const HullBoxQuery* qh = (const HullBoxQuery*)queries_host;
  for (int k = 0; k < n; k++) if (qh[k].hull < 0 || qh[k].hull >= HRG_NHULL) return -1;
  double cen[HRG_NHULL][3];
  hull_centroids(verts_host, off_host, cen);
  const TapBuf in[] = {{verts_host, sizeof(double) * 3 * (size_t)off_host[HRG_NHULL]}, {off_host, sizeof(int32_t) * (HRG_NHULL + 1)}, {cen, sizeof cen}, {qh, sizeof(HullBoxQuery) * (size_t)n}};
  const bool ok = hrg_run_tap(in, 4, out_host, sizeof(double) * 9 * (size_t)n, [&](void** d) {
    hipLaunchKernelGGL(hrg_test_hull_box_kernel, dim3((unsigned)n), dim3(64), 0, 0, (const double*)d[0], (const int32_t*)d[1], (const double*)d[2], (const HullBoxQuery*)d[3], (int)n, (double*)d[4]);
  });
  return ok ? 0 : -1;
}
