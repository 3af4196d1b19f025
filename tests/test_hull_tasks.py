"""robot_geometry="hull" for the handover, lifting, stacking and hammering tasks (hrg_step_kernel_ho_hull, _lift_hull, _stack_hull, _hammer_hull): the descs these
tasks build with hulls, the library's sources, the mixed batch's keyword, and the numpy MPR (tests/hullbox_ref.py) on the real link hulls against the boxes these
tasks collide with -- the lifting board, a stacking cube and the hammering task's board, handle, head and 4 mm nail head.  The GPU side is
tests/test_hull_tasks_gpu.py."""
import inspect

import numpy as np
import pytest

import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.model import load_robot_hulls
import hullbox_ref as ref
from test_hull_box import axis_rot, rot

NH = CONST["HRG_NHULL"]
TASKS = ("HumanRobotHandoverCart", "RobotHumanHandoverCart", "CollaborativeLiftingCart", "CollaborativeStackingCart", "CollaborativeHammeringCart")


def task_boxes():
    """(name, half extents) of every box an arm link meets in the five tasks, read from their descs"""
    hm = hrg.build_model_desc(None, env_id="CollaborativeHammeringCart")
    names = ("board", "handle", "head", "nail_head")
    out = [("hammer_" + names[g], np.array(hm.hm_geom_half[g][:])) for g in range(CONST["HRG_HM_NGEOM"])]
    out.append(("lifting_board", np.array(hrg.build_model_desc(None, env_id="CollaborativeLiftingCart").box_half[:])))
    out.append(("stacking_cube", np.array(hrg.build_model_desc(None, env_id="CollaborativeStackingCart").box_half[:])))
    return out


def surface_queries(n, half, seed, noise):
    """the real hulls at random poses, a box (half extents `half`, random rotation) placed so that one hull vertex lies `noise`-close to a random point of a box face
    (along its normal): (hull, R, p, box centre, box R) x n.  Every other query takes the hull's vertex nearest to that face's plane, so that the hull lies on the
    face's outer side but for that vertex (grazing: both verdicts), the others a random vertex (mostly overlapping)."""
    V, off = load_robot_hulls()
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        h = k % NH
        Vb = V[off[h]:off[h + 1]]
        R, p, bR = rot(rng), rng.uniform(-0.3, 0.3, 3), rot(rng)
        ax, sg = rng.randint(3), rng.choice((-1.0, 1.0))
        Vw = Vb @ R.T + p
        v = Vw[np.argmin(Vw @ (sg * bR[:, ax]))] if k % 2 == 0 else Vw[rng.randint(len(Vb))]
        q = rng.uniform(-1, 1, 3) * half
        q[ax] = sg * (half[ax] + rng.randn() * noise)
        out.append((h, R, p, v - bR @ q, bR))
    return out


def test_the_five_tasks_build_a_hull_desc():
    hv, ho = load_robot_hulls()
    for env_id in TASKS:
        d = hrg.build_model_desc(None, env_id=env_id, robot_geometry="hull")
        assert d.robot_hulls == 1, env_id
        assert list(d.hull_off) == list(ho), env_id
        assert np.array_equal(np.ctypeslib.as_array(d.hull_verts, shape=(int(ho[-1]) * 3,)), hv.ravel()), env_id
        assert hrg.build_model_desc(None, env_id=env_id).robot_hulls == 0, env_id   # the default stays capsules


def test_the_library_builds_the_four_new_variants():
    from human_robot_gym_amd import _lib
    for f in ("hrgym_handover_hulls.hip", "hrgym_lift_hulls.hip", "hrgym_stack_hulls.hip", "hrgym_hammer_hulls.hip"):
        assert any(s.endswith(f) for s in _lib.SOURCES), f
    assert len(set(_lib.SOURCES)) == len(_lib.SOURCES) == 12


def test_mixed_batch_takes_the_robot_geometry():
    from human_robot_gym_amd import mixed
    for fn in (mixed.make_mixed_batch, mixed.make_mixed_vec_env):
        p = inspect.signature(fn).parameters["robot_geometry"]
        assert p.default == "capsule", fn


def test_task_box_extents():
    b = dict(task_boxes())
    np.testing.assert_allclose(b["hammer_board"], [0.5, 0.2, 0.015])
    np.testing.assert_allclose(b["hammer_handle"], [0.0175, 0.0175, 0.0875])
    np.testing.assert_allclose(b["hammer_head"], [0.0616, 0.01925, 0.01925])
    np.testing.assert_allclose(b["hammer_nail_head"], [0.02, 0.02, 0.002])
    np.testing.assert_allclose(b["lifting_board"], [0.5, 0.2, 0.015])


@pytest.mark.parametrize("box", task_boxes(), ids=lambda b: b[0])
def test_mpr_certificate_and_depth_bound_on_the_task_boxes(box):
    """the bounds of test_hull_box.py::test_mpr_certificate_and_depth_bound_on_the_real_hulls at these extents: separated and penetrating placements of all seven
    hulls, shallow (3 mm) and grazing (0.3 mm: against the nail head's 2 mm half height the hull's vertex sits at its rim)"""
    name, bh = box
    V, off = load_robot_hulls()
    npen = nsep = 0
    for noise in (0.003, 0.0003):
        for h, R, p, c, bR in surface_queries(140, bh, 5 if noise > 0.001 else 6, noise):
            Vb = V[off[h]:off[h + 1]]
            st, depth, n, pos = ref.mpr_penetration(Vb, R, p, c, bR, bh)
            assert st != ref.NOT_CONVERGED, (name, h)
            if st == ref.SEPARATED:
                nsep += 1
                continue
            npen += 1
            assert depth > 0 and abs(np.linalg.norm(n) - 1) < 1e-12
            cert = ref.support_value_hull(Vb, R, p, n) - ref.support_value_box(c, bR, bh, n)
            assert abs(cert - depth) <= 1e-8, (name, h, cert, depth)
            u = -(R @ Vb.mean(axis=0) + p - c)
            u /= np.linalg.norm(u)
            ov_u = ref.support_value_hull(Vb, R, p, u) - ref.support_value_box(c, bR, bh, u)
            assert depth <= ov_u * (1 + 1e-6) + ref.TOL + 1e-9, (name, h, depth, ov_u)
            assert ref.support_value_box(c, bR, bh, n) - 1e-9 <= pos @ n <= ref.support_value_hull(Vb, R, p, n) + 1e-9
    print(f"[hull_tasks] {name}: {npen} penetrating, {nsep} separated")
    assert npen >= 60 and nsep >= 20, (npen, nsep)


@pytest.mark.parametrize("box", [b for b in task_boxes() if b[0] in ("hammer_board", "lifting_board")], ids=lambda b: b[0])
def test_link_lying_flat_on_the_board_face(box):
    """every hull laid on the board's top face with its lowest vertex 2 mm into it (the board turned about z, the link about its own vertical): the contact normal is
    the face normal and the depth is the 2 mm, to MPR's tolerance; lifted 2 mm clear of the face the pair is separated"""
    name, bh = box
    V, off = load_robot_hulls()
    rng = np.random.RandomState(9)
    tested = 0
    for h in range(NH):
        Vb = V[off[h]:off[h + 1]]
        for _ in range(4):
            bR = axis_rot([0, 0, 1], rng.uniform(-np.pi, np.pi))
            c = np.array([0.3, -0.1, 0.8])
            R = bR @ axis_rot([0, 0, 1], rng.uniform(-np.pi, np.pi)) @ axis_rot([1, 0, 0], np.pi / 2 * rng.randint(4))
            xy = rng.uniform(-0.05, 0.05, 2)
            low = (Vb @ R.T)[:, 2].min()
            cen = R @ Vb.mean(axis=0)
            p = c + bR @ np.array([xy[0], xy[1], 0.0]) - np.array([cen[0], cen[1], 0.0])
            if np.any(np.abs(((Vb @ R.T + p - c) @ bR)[:, :2]) > bh[:2]):
                continue   # the link overhangs the face: not lying on it
            tested += 1
            for lift, want in ((-0.002, ref.PENETRATING), (0.002, ref.SEPARATED)):
                p[2] = c[2] + bh[2] - low + lift
                st, depth, n, pos = ref.mpr_penetration(Vb, R, p, c, bR, bh)
                assert st == want, (name, h, lift, st)
                if want == ref.PENETRATING:
                    np.testing.assert_allclose(n, [0, 0, -1], atol=1e-6, err_msg=f"{name} hull {h}")
                    assert abs(depth - 0.002) <= 2 * ref.TOL, (name, h, depth)
    assert tested >= 14, tested
