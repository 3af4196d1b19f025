"""Hull x box penetration of the cube kernels (robot_geometry="hull" for PickPlaceHumanCart and the other cube tasks): the numpy restatement of MPR
(tests/hullbox_ref.py) against closed-form answers on a unit cube and against its own certificate on the real link hulls; the library's exports and the desc
the cube tasks build with hulls.  The GPU side -- the step kernel's wave routine against this reference, the wiring, behaviour and steady state -- is
tests/test_hull_box_gpu.py."""
import numpy as np
import pytest

import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.model import load_robot_hulls
import hullbox_ref as ref

NH = CONST["HRG_NHULL"]
CUBE = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)])   # hull = the 8 corners of a unit cube (centroid at its centre)
I3 = np.eye(3)
H5 = np.full(3, 0.5)


def rot(rng):
    q = rng.randn(4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def axis_rot(axis, ang):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return I3 + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def kat_cases():
    """(name, hull R, hull p, box centre, box R, box half, expected depth or None (separated), expected normal)"""
    c = []
    # face - face: the box overlaps the cube's +x face by 0.1 (off-centre across the face), and the same along -y, +z
    c.append(("face_x", I3, np.zeros(3), np.array([0.9, 0.02, 0.03]), I3, H5, 0.1, [1, 0, 0]))
    c.append(("face_-y", I3, np.zeros(3), np.array([0.01, -0.95, -0.02]), I3, H5, 0.05, [0, -1, 0]))
    c.append(("face_z_small_box", I3, np.zeros(3), np.array([0.1, -0.1, 0.52]), I3, np.array([0.2, 0.1, 0.05]), 0.03, [0, 0, 1]))
    # edge - edge: the cube turned 45 deg about z (an edge along z at x = sqrt(2)/2), the box turned 45 deg about y (an edge along y at x = c - sqrt(2)/2)
    r2 = np.sqrt(2.0)
    c.append(("edge_edge", axis_rot([0, 0, 1], np.pi / 4), np.zeros(3), np.array([r2 - 0.08, 0, 0]), axis_rot([0, 1, 0], np.pi / 4), H5, 0.08, [1, 0, 0]))
    # vertex - face: the cube's (1, 1, 1) diagonal turned onto +x (a vertex at x = sqrt(3)/2) against an axis-aligned box face
    v = np.array([1.0, 1.0, 1.0]) / np.sqrt(3)
    ax = np.cross(v, [1, 0, 0])
    Rv = axis_rot(ax, np.arccos(v[0]))
    c.append(("vertex_face", Rv, np.zeros(3), np.array([np.sqrt(3) / 2 + 0.5 - 0.04, 0, 0]), I3, H5, 0.04, [1, 0, 0]))
    # separated: the same configurations pulled apart
    c.append(("sep_face", I3, np.zeros(3), np.array([1.1, 0, 0]), I3, H5, None, None))
    c.append(("sep_edge", axis_rot([0, 0, 1], np.pi / 4), np.zeros(3), np.array([r2 + 0.01, 0, 0]), axis_rot([0, 1, 0], np.pi / 4), H5, None, None))
    c.append(("sep_vertex", Rv, np.zeros(3), np.array([np.sqrt(3) / 2 + 0.5 + 0.002, 0, 0]), I3, H5, None, None))
    c.append(("sep_diag", I3, np.zeros(3), np.array([1.02, 1.02, 0]), I3, H5, None, None))
    # posed and rotated: the face - face and edge - edge cases carried by one rigid motion -- same depth, normal turned with them
    T, t = rot(np.random.RandomState(11)), np.array([0.3, -1.2, 0.7])
    for name, R, p, bc, bR, bh, dep, n in list(c[:1]) + list(c[3:4]):
        c.append((name + "_posed", T @ R, T @ p + t, T @ bc + t, T @ bR, bh, dep, T @ np.asarray(n, float)))
    return c


@pytest.mark.parametrize("case", kat_cases(), ids=lambda c: c[0])
def test_mpr_known_answers_on_a_unit_cube(case):
    name, R, p, bc, bR, bh, dep, n = case
    st, depth, nrm, pos = ref.mpr_penetration(CUBE, R, p, bc, bR, bh)
    if dep is None:
        assert st == ref.SEPARATED, name
        return
    assert st == ref.PENETRATING, name
    assert abs(depth - dep) <= 1e-12, (name, depth, dep)
    np.testing.assert_allclose(nrm, n, rtol=0, atol=1e-12, err_msg=name)
    # the box-face bound holds with equality where a box face carries the contact (face - face, vertex - face)
    if name.startswith(("face", "vertex")):
        ov = [ref.support_value_hull(CUBE, R, p, u) - ref.support_value_box(bc, bR, bh, u) for u in (nrm, -nrm)]
        assert depth <= min(ov) * (1 + 1e-6) + 1e-9
    # the position lies inside both shapes' overlap: between the hull's extent and the box's along the normal
    assert ref.support_value_box(bc, bR, bh, nrm) - 1e-12 <= pos @ nrm <= ref.support_value_hull(CUBE, R, p, nrm) + 1e-12


def random_real_queries(n, seed):
    """the real hulls at random poses against a 4 cm cube near their surface: (hull, R, p, box centre, box R) x n"""
    V, off = load_robot_hulls()
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        h = k % NH
        Vb = V[off[h]:off[h + 1]]
        R, p = rot(rng), rng.uniform(-0.3, 0.3, 3)
        c = (Vb @ R.T + p)[rng.randint(len(Vb))] + rng.randn(3) * 0.015
        out.append((h, R, p, c, rot(rng)))
    return out


def test_mpr_certificate_and_depth_bound_on_the_real_hulls():
    """>= 500 penetrating poses of the seven link hulls against the 4 cm cube.
    Certificate: along the returned normal n, max over the hull of n.v minus min over the box of n.c is the returned depth (the depth IS that overlap).
    Depth bound: the box's face normals bound the depth only where MPR's portal ends on a box face -- MPR follows the ray from the interior point (hull centroid -
    box centre) through the origin to the face that ray exits, not to the nearest face, and on these poses its depth exceeds the smallest face-normal overlap in about
    a quarter of the pairs by up to a few cm (reported below).  What MPR does guarantee: the final portal contains that ray's exit point, so the depth is at most
    the overlap along the ray's direction u plus the tolerance: the face-normal bound relaxed to that direction, asserted for every pair (the face-normal bound
    itself holds, with equality, on the unit-cube cases where a box face carries the contact: test_mpr_known_answers_on_a_unit_cube)."""
    V, off = load_robot_hulls()
    h2 = np.full(3, 0.02)
    npen = nsep = 0
    face_bound_viol = 0
    for h, R, p, c, bR in random_real_queries(900, 1):
        Vb = V[off[h]:off[h + 1]]
        st, depth, n, pos = ref.mpr_penetration(Vb, R, p, c, bR, h2)
        assert st != ref.NOT_CONVERGED
        if st == ref.SEPARATED:
            nsep += 1
            continue
        npen += 1
        assert depth > 0 and abs(np.linalg.norm(n) - 1) < 1e-12
        cert = ref.support_value_hull(Vb, R, p, n) - ref.support_value_box(c, bR, h2, n)
        assert abs(cert - depth) <= 1e-8, (h, cert, depth)
        u = -(R @ Vb.mean(axis=0) + p - c)
        u /= np.linalg.norm(u)
        ov_u = ref.support_value_hull(Vb, R, p, u) - ref.support_value_box(c, bR, h2, u)
        assert depth <= ov_u * (1 + 1e-6) + ref.TOL + 1e-9, (h, depth, ov_u)
        ov_face = min(min(ref.support_value_hull(Vb, R, p, s * e) - ref.support_value_box(c, bR, h2, s * e) for s in (1, -1)) for e in bR.T)
        if depth > ov_face * (1 + 1e-6) + 1e-9:
            face_bound_viol += 1
        assert ref.support_value_box(c, bR, h2, n) - 1e-9 <= pos @ n <= ref.support_value_hull(Vb, R, p, n) + 1e-9
    print(f"[hull_box] {npen} penetrating, {nsep} separated; depth above the smallest box-face overlap in {face_bound_viol} pairs")
    assert npen >= 500 and nsep > 0


def test_cube_tasks_build_a_hull_desc_and_the_library_exports_the_tap():
    from human_robot_gym_amd import _lib
    assert "hrg_test_hull_box_queries" in _lib.EXPORTS and "hrg_batch_mpr_fallbacks" in _lib.EXPORTS
    assert any(s.endswith("hrgym_box_hulls.hip") for s in (_lib.SRC_BOX_HULLS,))
    for env_id, extra in (("PickPlaceHumanCart", {}), ("HumanObjectInspectionCart", {}), ("ReachHuman", dict(reach_box=True))):
        d = hrg.build_model_desc(None, env_id=env_id, robot_geometry="hull", **extra)
        assert d.robot_hulls == 1 and d.task != CONST["HRG_TASK_REACH"]
        assert list(d.hull_off) == list(load_robot_hulls()[1])
