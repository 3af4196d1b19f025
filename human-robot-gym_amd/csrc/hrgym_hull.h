// hrgym_hull.h — convex hulls of the arm links as collision geometry (hrg_model_desc.robot_hulls; robot.xml:29-55: mesh geoms, which MuJoCo convexifies).
// The whole wave works on ONE (hull, other geom) pair at a time: the support mapping -- the hull vertex farthest along a direction -- runs over the vertices
// with lanes = vertices (a hull has 122 .. 2211 of them) and a wave arg-max; the GJK iteration around it (Gilbert / Johnson / Keerthi; closest-point
// sub-problems after Ericson, Real-Time Collision Detection 5.1) is wave-uniform: every lane computes the same numbers.  Its simplex -- up to four points of the
// Minkowski difference with their witnesses -- lives in the collide part of the env's LDS image (Lds::gjk), written by lane 0 and indexed dynamically there; in
// registers it would be 36 doubles per lane behind dynamic indices (scratch), and as a real function its call made the register allocator spill 290 VGPRs
// across the whole step kernel (727 scratch loads; 4 x the step time).  Inlined with the simplex in LDS the step kernel keeps its allocation.
// Restated side by side in oracle/hrg_oracle.c (hull_support, gjk_hull_segment, hull_lowest).
#pragma once
#include "hrgym_device.h"

struct HullRef { const double* v; int n; const double* R; const double* p; };   // body-frame vertices (device memory); world pose of the body (LDS / constants)

// vertex farthest along the world direction d (the lowest index on a tie): index; world point in out.  Wave-uniform result.
DI int hull_support_wave(const HullRef& H, const double* d, double* out) {
  const int lane = hrg_lane();
  const double dl0 = H.R[0] * d[0] + H.R[3] * d[1] + H.R[6] * d[2], dl1 = H.R[1] * d[0] + H.R[4] * d[1] + H.R[7] * d[2], dl2 = H.R[2] * d[0] + H.R[5] * d[1] + H.R[8] * d[2];
  double bv = -1e300;
  int bi = 0x7fffffff;
  // four vertices per lane and trip: their twelve loads are in flight together (the table sits in L2; one wave per SIMD-slot pays the full latency per trip otherwise --
  // link 4 has 2211 vertices = 35 trips per support call, ~ 8 calls per GJK query)
  int i = lane;
#pragma unroll 1
  for (; i + 192 < H.n; i += 256) {
    double t[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { const double* v = H.v + 3 * (i + 64 * u); t[u] = v[0] * dl0 + v[1] * dl1 + v[2] * dl2; }
#pragma unroll
    for (int u = 0; u < 4; u++) if (t[u] > bv) { bv = t[u]; bi = i + 64 * u; }
  }
#pragma unroll 1
  for (; i < H.n; i += 64) {
    const double t = H.v[3 * i] * dl0 + H.v[3 * i + 1] * dl1 + H.v[3 * i + 2] * dl2;
    if (t > bv) { bv = t; bi = i; }
  }
  const double mx = wave_max(bv);
  int cand = bv == mx ? bi : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(cand, o, 64); cand = t < cand ? t : cand; }
  const int best = __builtin_amdgcn_readfirstlane(cand);
  const double vx = H.v[3 * best], vy = H.v[3 * best + 1], vz = H.v[3 * best + 2];
  out[0] = H.p[0] + H.R[0] * vx + H.R[1] * vy + H.R[2] * vz;
  out[1] = H.p[1] + H.R[3] * vx + H.R[4] * vy + H.R[5] * vz;
  out[2] = H.p[2] + H.R[6] * vx + H.R[7] * vy + H.R[8] * vz;
  return best;
}

// barycentric coordinates of the point of triangle (a, b, c) closest to the origin (Ericson 5.1.5)
DI void closest_triangle(const double* a, const double* b, const double* c, double& l0, double& l1, double& l2) {
  double ab[3], ac[3];
  v3sub(ab, b, a); v3sub(ac, c, a);
  const double d1 = -v3dot(ab, a), d2 = -v3dot(ac, a);
  const double d3 = -v3dot(ab, b), d4 = -v3dot(ac, b);
  const double d5 = -v3dot(ab, c), d6 = -v3dot(ac, c);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  if (d1 <= 0 && d2 <= 0) { l0 = 1; l1 = 0; l2 = 0; }
  else if (d3 >= 0 && d4 <= d3) { l0 = 0; l1 = 1; l2 = 0; }
  else if (vc <= 0 && d1 >= 0 && d3 <= 0) { const double v = d1 / (d1 - d3); l0 = 1 - v; l1 = v; l2 = 0; }
  else if (d6 >= 0 && d5 <= d6) { l0 = 0; l1 = 0; l2 = 1; }
  else if (vb <= 0 && d2 >= 0 && d6 <= 0) { const double w = d2 / (d2 - d6); l0 = 1 - w; l1 = 0; l2 = w; }
  else if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) { const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); l0 = 0; l1 = 1 - w; l2 = w; }
  else { const double den = 1.0 / (va + vb + vc), v = vb * den, w = vc * den; l0 = 1 - v - w; l1 = v; l2 = w; }
}

// point of the simplex (S = g_L.gjk, n points) closest to the origin: v; the simplex reduced to the vertices that carry it (n updated), their weights in
// S.lam; true when the origin is inside.  Every lane computes the same values from LDS; lane 0 writes.
DI bool simplex_closest(int& n, double* v) {
  GjkLds& S = g_L.gjk;
  const bool w0 = hrg_lane() == 0;
  if (n == 1) { if (w0) S.l[0] = 1; }
  else if (n == 2) {
    double ab[3];
    v3sub(ab, S.y[1], S.y[0]);
    const double den = v3dot(ab, ab);
    double t = den > 0 ? -v3dot(S.y[0], ab) / den : 0.0;
    t = t < 0 ? 0 : (t > 1 ? 1 : t);
    if (w0) { S.l[0] = 1 - t; S.l[1] = t; }
  } else if (n == 3) {
    double l0, l1, l2;
    closest_triangle(S.y[0], S.y[1], S.y[2], l0, l1, l2);
    if (w0) { S.l[0] = l0; S.l[1] = l1; S.l[2] = l2; }
  } else {   // tetrahedron (Ericson 5.1.6): the closest of the faces the origin lies outside of; inside all four -> the origin is in the simplex
    double best = 1e300, b0 = 0, b1 = 0, b2 = 0;
    int fb = -1;
#pragma unroll 1
    for (int f = 0; f < 4; f++) {
      // faces (0 1 2 | 3), (0 2 3 | 1), (0 3 1 | 2), (1 3 2 | 0)
      const int i0 = f == 3 ? 1 : 0, i1 = f == 0 ? 1 : (f == 1 ? 2 : 3), i2 = f == 0 ? 2 : (f == 1 ? 3 : (f == 2 ? 1 : 2)), i3 = f == 0 ? 3 : (f == 1 ? 1 : (f == 2 ? 2 : 0));
      const double *a = S.y[i0], *b = S.y[i1], *c = S.y[i2], *d = S.y[i3];
      double ab[3], ac[3], nrm[3], ad[3];
      v3sub(ab, b, a); v3sub(ac, c, a); v3cross(nrm, ab, ac); v3sub(ad, d, a);
      const double sp = -v3dot(a, nrm), sd = v3dot(ad, nrm);
      if (!(sp * sd < 0) && sd != 0) continue;
      double l0, l1, l2, q[3];
      closest_triangle(a, b, c, l0, l1, l2);
      for (int k = 0; k < 3; k++) q[k] = l0 * a[k] + l1 * b[k] + l2 * c[k];
      const double dq = v3dot(q, q);
      if (dq < best) { best = dq; fb = f; b0 = l0; b1 = l1; b2 = l2; }
    }
    if (fb < 0) { v3set(v, 0, 0, 0); return true; }
    if (w0) {
      const int i0 = fb == 3 ? 1 : 0, i1 = fb == 0 ? 1 : (fb == 1 ? 2 : 3), i2 = fb == 0 ? 2 : (fb == 1 ? 3 : (fb == 2 ? 1 : 2));
      S.l[0] = S.l[1] = S.l[2] = S.l[3] = 0;
      S.l[i0] = b0; S.l[i1] = b1; S.l[i2] = b2;
    }
  }
  wave_sync();
  int nk = 0;
  v3set(v, 0, 0, 0);
#pragma unroll 1
  for (int i = 0; i < n; i++) {
    const double li = S.l[i];
    if (!(li > 0)) continue;
    double y[3];
    v3cpy(y, S.y[i]);
    for (int k = 0; k < 3; k++) v[k] += li * y[k];
    if (w0) {
      S.lam[nk] = li;
      if (nk != i) { v3cpy(S.y[nk], y); v3cpy(S.a[nk], S.a[i]); v3cpy(S.b[nk], S.b[i]); S.ia[nk] = S.ia[i]; S.ib[nk] = S.ib[i]; }
    }
    nk++;
  }
  n = nk;
  wave_sync();
  return false;
}

// distance between the hull and the segment [s1, s2] (a capsule's axis, in LDS); witness points wa (on the hull) and wb (on the segment).  0 when they
// intersect.  Wave-uniform result.  `cutoff`: the caller only asks whether the two come closer than this -- every support point w bounds the distance from below by
// v.w / |v| (the supporting plane of the Minkowski difference), so the iteration stops at the first plane farther out than the cutoff and returns 1e300: the
// narrowphase of a pair whose bounding capsules touch but whose hull is clear ends after one or two support calls instead of converging on a distance nobody uses.
DI double gjk_hull_segment_wave(const HullRef& H, const double* s1, const double* s2, double* wa, double* wb, double cutoff = 1e300) {
  GjkLds& S = g_L.gjk;
  const bool w0 = hrg_lane() == 0;
  double v[3];
  int n = 1;
  {
    double a0[3];
    const double vx = H.v[0], vy = H.v[1], vz = H.v[2];
    a0[0] = H.p[0] + H.R[0] * vx + H.R[1] * vy + H.R[2] * vz; a0[1] = H.p[1] + H.R[3] * vx + H.R[4] * vy + H.R[5] * vz; a0[2] = H.p[2] + H.R[6] * vx + H.R[7] * vy + H.R[8] * vz;
    v3sub(v, a0, s1);
    if (w0) { v3cpy(S.y[0], v); v3cpy(S.a[0], a0); v3cpy(S.b[0], s1); S.ia[0] = 0; S.ib[0] = 0; S.lam[0] = 1; }
  }
  wave_sync();
  bool inside = false;
#pragma unroll 1
  for (int it = 0; it < 64; it++) {
    const double vv = v3dot(v, v);
    if (vv <= 1e-24) { inside = true; break; }
    const double dir[3] = {-v[0], -v[1], -v[2]};
    double a[3], w[3], b[3];
    const int ia = hull_support_wave(H, dir, a);
    const int ib = v3dot(v, s2) > v3dot(v, s1) ? 1 : 0;
    v3cpy(b, ib ? s2 : s1);
    v3sub(w, a, b);
    const double vw = v3dot(v, w);
    if (vw > 0 && vw * vw > cutoff * cutoff * vv) { v3set(wa, 0, 0, 0); v3set(wb, 0, 0, 0); return 1e300; }
    if (vv - vw <= 1e-12 * vv) break;
    bool seen = false;
    for (int q = 0; q < n; q++) if (S.ia[q] == ia && S.ib[q] == ib) seen = true;
    if (seen) break;
    if (w0) { v3cpy(S.y[n], w); v3cpy(S.a[n], a); v3cpy(S.b[n], b); S.ia[n] = ia; S.ib[n] = ib; }
    n++;
    wave_sync();
    if (simplex_closest(n, v)) { inside = true; break; }
  }
  v3set(wa, 0, 0, 0); v3set(wb, 0, 0, 0);
  if (inside) return 0.0;
#pragma unroll 1
  for (int q = 0; q < n; q++) { const double lq = S.lam[q]; for (int k = 0; k < 3; k++) { wa[k] += lq * S.a[q][k]; wb[k] += lq * S.b[q][k]; } }
  return fsqrt(v3dot(v, v));
}

// the hull against a horizontal plane -> out[3]: z = height of the lowest vertex, (x, y) = mean of the vertices within 1e-6 m of it (a link lying flat on a face
// or an edge touches in the middle of it, whichever vertex rounding makes the lowest).  Wave-uniform result.
DI void hull_lowest_wave(const HullRef& H, double* out) {
  const int lane = hrg_lane();
  const double r6 = H.R[6], r7 = H.R[7], r8 = H.R[8], pz = H.p[2];
  double zm = 1e300;
  int i = lane;
#pragma unroll 1
  for (; i + 192 < H.n; i += 256) {
    double z[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { const double* v = H.v + 3 * (i + 64 * u); z[u] = pz + r6 * v[0] + r7 * v[1] + r8 * v[2]; }
#pragma unroll
    for (int u = 0; u < 4; u++) zm = z[u] < zm ? z[u] : zm;
  }
#pragma unroll 1
  for (; i < H.n; i += 64) {
    const double z = pz + r6 * H.v[3 * i] + r7 * H.v[3 * i + 1] + r8 * H.v[3 * i + 2];
    zm = z < zm ? z : zm;
  }
  const double zmin = -wave_max(-zm);
  double sx = 0, sy = 0, cnt = 0;
#pragma unroll 2
  for (int i = lane; i < H.n; i += 64) {
    const double vx = H.v[3 * i], vy = H.v[3 * i + 1], vz = H.v[3 * i + 2];
    const double z = pz + r6 * vx + r7 * vy + r8 * vz;
    if (z <= zmin + 1e-6) { sx += H.p[0] + H.R[0] * vx + H.R[1] * vy + H.R[2] * vz; sy += H.p[1] + H.R[3] * vx + H.R[4] * vy + H.R[5] * vz; cnt += 1; }
  }
  const double tc = wave_sum(cnt);
  out[0] = wave_sum(sx) / tc; out[1] = wave_sum(sy) / tc; out[2] = zmin;
}

#if HRG_HULL_MPR
// ------------------------------------------------------------------------------------------------ hull x cube: penetration by MPR
// MuJoCo 2.1 (the version the reference pins) collides a mesh geom with a box through its convex-convex path: Minkowski Portal Refinement (Snethen, "XenoCollide",
// Game Programming Gems 7), ONE contact per pair -- depth, direction, position.  Restated here from that description, wave-uniform like the GJK above: the hull's
// support mapping is hull_support_wave (lanes = vertices), the cube's is closed form, and the portal (four points of the Minkowski difference hull - cube with their
// witnesses, plus the candidate point) lives in the collide part of the LDS union (Lds::mpr), written by lane 0, read by every lane.
#define HRG_MPR_TOLERANCE 1e-6    // mjOption.mpr_tolerance (MuJoCo 2.1 default): a support point this close to the portal's plane ends the refinement
#define HRG_MPR_ITERATIONS 50     // mjOption.mpr_iterations (MuJoCo 2.1 default): bound on every loop of the routine; beyond it the pair is "not converged"
#define HRG_MPR_EPS 2.220446049250313e-16   // zero test of the portal's sign decisions (double epsilon)
enum { MPR_SEPARATED = 0, MPR_PENETRATING = 1, MPR_NOT_CONVERGED = 2 };

// corner of the cube (rotation R row-major, centre p, half extents h) farthest along the world direction d: the sign of each component of d in the cube's frame
DI void box_support(const double* R, const double* p, const double* h, const double* d, double* out) {
  double s[3];
  for (int a = 0; a < 3; a++) s[a] = R[a] * d[0] + R[3 + a] * d[1] + R[6 + a] * d[2] >= 0 ? h[a] : -h[a];
  for (int k = 0; k < 3; k++) out[k] = p[k] + R[3 * k] * s[0] + R[3 * k + 1] * s[1] + R[3 * k + 2] * s[2];
}

// support point of the Minkowski difference hull - cube along d into portal slot k: hull vertex farthest along d minus cube corner farthest along -d
DI void mpr_support(const HullRef& H, const double* bR, const double* bp, const double* bh, const double* d, int k) {
  MprLds& P = g_L.mpr;
  double a[3], b[3];
  const double nd[3] = {-d[0], -d[1], -d[2]};
  hull_support_wave(H, d, a);
  box_support(bR, bp, bh, nd, b);
  if (hrg_lane() == 0) { v3cpy(P.a[k], a); v3cpy(P.b[k], b); for (int c = 0; c < 3; c++) P.v[k][c] = a[c] - b[c]; }
  wave_sync();
}
DI void mpr_copy(int dst, int src) {
  MprLds& P = g_L.mpr;
  if (hrg_lane() == 0) { v3cpy(P.v[dst], P.v[src]); v3cpy(P.a[dst], P.a[src]); v3cpy(P.b[dst], P.b[src]); }
  wave_sync();
}
DI void mpr_normalize(double* d) { const double l = v3norm(d); if (l > 0) v3scl(d, d, 1.0 / l); }
// normal of the portal triangle (v1, v2, v3), pointing away from v0
DI void mpr_portal_dir(double* d) {
  const MprLds& P = g_L.mpr;
  double e1[3], e2[3];
  v3sub(e1, P.v[2], P.v[1]); v3sub(e2, P.v[3], P.v[1]);
  v3cross(d, e1, e2);
  mpr_normalize(d);
}
// the candidate (slot 4) lies within the tolerance of the portal's plane along d
DI bool mpr_reached(const double* d) {
  const MprLds& P = g_L.mpr;
  const double d4 = v3dot(P.v[4], d);
  const double m = fmin(d4 - v3dot(P.v[1], d), fmin(d4 - v3dot(P.v[2], d), d4 - v3dot(P.v[3], d)));
  return m <= HRG_MPR_TOLERANCE;
}
// the candidate replaces the portal vertex on the far side of the plane through v0, v4 that keeps the origin inside the new portal's cone
DI void mpr_expand() {
  const MprLds& P = g_L.mpr;
  double c[3];
  v3cross(c, P.v[4], P.v[0]);
  int r;
  if (v3dot(P.v[1], c) > 0) r = v3dot(P.v[2], c) > 0 ? 1 : 3;
  else r = v3dot(P.v[3], c) > 0 ? 2 : 1;
  mpr_copy(r, 4);
}

// Penetration of hull H and the cube (bR, bp, bh), `hc` = world position of the hull's vertex centroid (the interior point).  MPR_PENETRATING: depth > 0, the unit
// normal n from the hull into the cube (moving the hull by -depth n separates the two), pos = half way between the two witnesses of the origin in the final portal.
// MPR is not a minimum-depth method: n is the normal of the boundary face the ray from the interior point through the origin leaves by, not of the nearest one.
// MPR_SEPARATED: the origin lies outside the Minkowski difference (or on its boundary).  MPR_NOT_CONVERGED: a loop ran out of HRG_MPR_ITERATIONS.  Wave-uniform.
DI int mpr_hull_box_wave(const HullRef& H, const double* hc, const double* bR, const double* bp, const double* bh, double& depth, double* n, double* pos) {
  MprLds& P = g_L.mpr;
  const bool w0 = hrg_lane() == 0;
  depth = 0; v3set(n, 0, 0, 0); v3set(pos, 0, 0, 0);
  // ---- phase 1: portal discovery.  v0 = an interior point of the Minkowski difference (centroid of the hull - centre of the cube)
  {
    double v0[3];
    v3sub(v0, hc, bp);
    if (v0[0] == 0 && v0[1] == 0 && v0[2] == 0) v0[0] = 10 * HRG_MPR_EPS;   // on the origin: nudged, so that the ray from it has a direction
    if (w0) { v3cpy(P.v[0], v0); v3cpy(P.a[0], hc); v3cpy(P.b[0], bp); }
    wave_sync();
  }
  double d[3];
  v3scl(d, P.v[0], -1.0);
  mpr_normalize(d);
  mpr_support(H, bR, bp, bh, d, 1);
  {
    const double t = v3dot(P.v[1], d);
    if (t < HRG_MPR_EPS) return MPR_SEPARATED;   // the farthest point towards the origin does not pass it
  }
  v3cross(d, P.v[0], P.v[1]);
  if (v3dot(d, d) < HRG_MPR_EPS) {   // the origin lies on the line v0 - v1
    const double l = v3norm(P.v[1]);
    if (!(l > 0)) return MPR_SEPARATED;   // ... on v1: the boundary, touching
    depth = l;
    v3scl(n, P.v[1], 1.0 / l);
    for (int c = 0; c < 3; c++) pos[c] = 0.5 * (P.a[1][c] + P.b[1][c]);
    return MPR_PENETRATING;
  }
  mpr_normalize(d);
  mpr_support(H, bR, bp, bh, d, 2);
  if (v3dot(P.v[2], d) < HRG_MPR_EPS) return MPR_SEPARATED;
  {
    double e1[3], e2[3];
    v3sub(e1, P.v[1], P.v[0]); v3sub(e2, P.v[2], P.v[0]);
    v3cross(d, e1, e2);
    mpr_normalize(d);
    if (v3dot(d, P.v[0]) > 0) {   // orient the portal's faces away from the origin: swap v1 and v2
      mpr_copy(4, 1); mpr_copy(1, 2); mpr_copy(2, 4);
      v3scl(d, d, -1.0);
    }
  }
  bool found = false;
#pragma unroll 1
  for (int it = 0; it < HRG_MPR_ITERATIONS; it++) {
    mpr_support(H, bR, bp, bh, d, 3);
    if (v3dot(P.v[3], d) < HRG_MPR_EPS) return MPR_SEPARATED;
    double c[3];
    v3cross(c, P.v[1], P.v[3]);
    double t = v3dot(c, P.v[0]);
    int r = 0;
    if (t < 0 && !(fabs(t) < HRG_MPR_EPS)) r = 2;   // the origin is outside the face (v1, v0, v3): v3 takes v2's place
    else {
      v3cross(c, P.v[3], P.v[2]);
      t = v3dot(c, P.v[0]);
      if (t < 0 && !(fabs(t) < HRG_MPR_EPS)) r = 1;   // ... outside (v3, v0, v2): v3 takes v1's place
    }
    if (!r) { found = true; break; }
    mpr_copy(r, 3);
    double e1[3], e2[3];
    v3sub(e1, P.v[1], P.v[0]); v3sub(e2, P.v[2], P.v[0]);
    v3cross(d, e1, e2);
    mpr_normalize(d);
  }
  if (!found) return MPR_NOT_CONVERGED;
  // ---- phase 2: refine the portal until the origin lies on its inner side (intersection) or a support point shows it outside (separation)
  found = false;
#pragma unroll 1
  for (int it = 0; it < HRG_MPR_ITERATIONS; it++) {
    mpr_portal_dir(d);
    if (v3dot(d, P.v[1]) > -HRG_MPR_EPS) { found = true; break; }
    mpr_support(H, bR, bp, bh, d, 4);
    if (v3dot(P.v[4], d) < HRG_MPR_EPS || mpr_reached(d)) return MPR_SEPARATED;
    mpr_expand();
  }
  if (!found) return MPR_NOT_CONVERGED;
  // ---- phase 3: push the portal out to the boundary along its normal; the depth is the origin's distance to the final portal triangle
  found = false;
#pragma unroll 1
  for (int it = 0; it < HRG_MPR_ITERATIONS; it++) {
    mpr_portal_dir(d);
    mpr_support(H, bR, bp, bh, d, 4);
    if (mpr_reached(d)) { found = true; break; }
    mpr_expand();
  }
  if (!found) return MPR_NOT_CONVERGED;
  // the final portal's normal is the contact normal; the depth is the extent of the Minkowski difference along it (the support point's distance: the overlap of the
  // two shapes' projections on n, how far the hull must move back along n to clear the cube), within the tolerance of the portal plane's distance from the origin
  depth = v3dot(P.v[4], d);
  if (!(depth > 0)) { depth = 0; return MPR_SEPARATED; }   // the origin on the boundary: touching, no contact at margin 0
  v3cpy(n, d);
  // position: barycentric coordinates of the origin in the tetrahedron (v0 .. v3) -- signed volumes -- applied to the witnesses on each shape, then the midpoint.
  // A flat tetrahedron falls back to the coordinates of the origin's projection along the portal's normal in the triangle (v1, v2, v3).
  double w[4], cr[3];
  v3cross(cr, P.v[1], P.v[2]); w[0] = v3dot(cr, P.v[3]);
  v3cross(cr, P.v[3], P.v[2]); w[1] = v3dot(cr, P.v[0]);
  v3cross(cr, P.v[0], P.v[1]); w[2] = v3dot(cr, P.v[3]);
  v3cross(cr, P.v[2], P.v[1]); w[3] = v3dot(cr, P.v[0]);
  double sw = w[0] + w[1] + w[2] + w[3];
  if (sw < HRG_MPR_EPS) {
    w[0] = 0;
    v3cross(cr, P.v[2], P.v[3]); w[1] = v3dot(cr, d);
    v3cross(cr, P.v[3], P.v[1]); w[2] = v3dot(cr, d);
    v3cross(cr, P.v[1], P.v[2]); w[3] = v3dot(cr, d);
    sw = w[1] + w[2] + w[3];
  }
  const double inv = 1.0 / sw;
#pragma unroll
  for (int k = 0; k < 4; k++) for (int c = 0; c < 3; c++) pos[c] += w[k] * (P.a[k][c] + P.b[k][c]);
  v3scl(pos, pos, 0.5 * inv);
  return MPR_PENETRATING;
}
#endif
