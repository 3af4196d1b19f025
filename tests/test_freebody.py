"""The free-body contact step against an independent reference (tests/freebody_ref.py): anchors of the reference itself, teeth of the scenarios, and the
CPU oracle against the reference with the scenarios and the bound of tests/freebody_scenarios.py (the kernels: tests/test_freebody_gpu.py)."""
from dataclasses import replace

import numpy as np
import pytest

import freebody_ref as fr
import freebody_scenarios as fs

LD = np.longdouble
EPS = {np.float64: float(np.finfo(np.float64).eps), LD: float(np.finfo(LD).eps)}


def _desc(family):
    import human_robot_gym_amd as hrg
    F = fs.FAMILIES[family]
    return hrg.build_model_desc(dict(F["kw"]), n_clips=3, env_id=F["env_id"])


@pytest.fixture(scope="module")
def cube():
    return _desc("cube")


@pytest.fixture(scope="module")
def brick():
    return _desc("brick")


# ------------------------------------------------------------------------------------------------ anchors of the reference
@pytest.mark.parametrize("T", [np.float64, LD])
def test_free_fall_is_the_closed_form_of_semi_implicit_euler(cube, T):
    """No contact: v_k = v_0 + g h k and z_k = z_0 + v_0 h k + g h^2 k (k + 1) / 2, to rounding (k additions of numbers of the size of the result: k eps each)."""
    M = fr.Model.from_desc(cube, T)
    p0, v0, k = [0.3, 0.4, 3.0], [0.2, -0.1, 1.5, 0, 0, 0], 60
    p, q, v = fr.advance(M, p0, [1, 0, 0, 0], v0, k)
    g, h = M.gravity, M.h
    v_want = np.array(v0[:3], dtype=T) + g * h * k
    p_want = np.array(p0, dtype=T) + np.array(v0[:3], dtype=T) * h * k + g * h * h * T(k * (k + 1) / 2)
    assert np.abs(v[:3] - v_want).max() <= 2 * k * EPS[T] * np.abs(v_want).max()
    assert np.abs(p - p_want).max() <= 2 * k * EPS[T] * np.abs(p_want).max()
    assert np.array_equal(q, np.array([1, 0, 0, 0], dtype=T)) and not v[3:].any()


def test_a_spinning_cube_keeps_its_spin_and_turns_by_k_h_omega(cube):
    """Isotropic inertia: no torque, so w stays and the cube turns by exactly k h |w| about it (every substep multiplies by the same unit quaternion)."""
    M = fr.Model.from_desc(cube, LD)
    w = np.array([3.0, -2.0, 4.0], dtype=LD)
    k, q0 = 50, np.array([np.cos(0.3), np.sin(0.3) * 0.6, 0, np.sin(0.3) * 0.8], dtype=LD)
    p, q, v = fr.advance(M, [0, 0, 5.0], q0, [0, 0, 0, *w], k)
    wn = fr.norm(w)
    assert np.abs(v[3:] - w).max() <= 8 * k * EPS[LD] * wn       # (R diag(I) R' is the identity times I only up to rounding: a torque of a few eps)
    half = k * M.h * wn / 2
    want = fr.quat_mul(np.concatenate([[np.cos(half)], np.sin(half) * w / wn]).astype(LD), q0)
    assert fs.quat_diff(q, want) <= 8 * k * EPS[LD]


def _rest_force(M, R, r):
    """normal force of a cube lying flat r deep at rest: 4 corners x 4 edges, each D K imp |r| along its own direction n +- mu t -- the tangential parts cancel"""
    imp, K, B = fr.impedance(M, R, -r)
    mu = M.mu if R.mu is None else M.T(R.mu)
    D = 1 / ((1 - imp) / imp * (1 / M.mass) * (1 + mu * mu) * fr.pyramid_r_scale(R, mu))
    return 16 * D * K * imp * r, 16 * D * K * imp, 16 * D * B


def rest_penetration(M, R=fr.Rules()):
    """r* with m g = 16 D(r) K imp(r) r, by bisection (the force grows with r: D, imp and r all do)"""
    w = M.mass * abs(M.gravity[2])
    lo, hi = M.T(0), M.T(0.01)
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if _rest_force(M, R, mid)[0] < w else (lo, mid)
    return (lo + hi) / 2


def test_a_cube_at_rest_sits_at_the_penetration_of_the_force_balance(cube):
    """Flat on the table, 8 policy steps (0.8 s = 40 time constants of the critically damped contact).  Bound = the solve's residual carried through the force
    balance: at the last substep 16 D (K imp r - B v_z) = m (g + a_z) up to the KKT residual, so F(r) - F(r*) = m a_z + 16 D B v_z + res, and since
    F'(r) >= 16 D K imp (D and imp do not fall with r) |r - r*| <= (m |a_z| + 16 D B |v_z| + KKT_TOL (1 + m g)) / (16 D K imp) at the shallower of r, r*."""
    M = fr.Model.from_desc(cube)
    z0 = M.table_top_z + M.half[2]
    p, q, v, a = fr.advance(M, [0.5, 0.7, z0], [1, 0, 0, 0], [0] * 6, 8 * cube.n_cycles, return_warm=True)
    r, want = z0 - p[2], rest_penetration(M)
    _, stiff, damp = _rest_force(M, fr.Rules(), min(r, want))
    bound = (M.mass * abs(a[2]) + damp * abs(v[2]) + fr.KKT_TOL * (1 + M.mass * abs(M.gravity[2]))) / stiff
    print(f"[freebody] rest: r {r:.6e} r* {want:.6e} |r - r*| {abs(r - want):.2e} bound {bound:.2e} v_z {v[2]:.1e} a_z {a[2]:.1e}")
    assert 1e-5 < want < 1e-3 and abs(r - want) <= bound + 8 * EPS[np.float64] * z0    # (r is a difference of two heights near 0.84: their rounding)
    assert np.abs(v).max() < 1e-9 and np.abs(q - [1, 0, 0, 0]).max() < 1e-12


def test_angular_momentum_of_a_tumbling_brick_drifts_to_first_order(brick):
    """Explicit Euler guarantees one thing for the torque-free brick: the drift of I_world w per unit time is O(h) -- half the step, twice the substeps, half the drift (10 %)."""
    def drift(M, n):
        q0, w0 = np.array([np.cos(0.35), np.sin(0.35) * 0.6, np.sin(0.35) * 0.8, 0], dtype=LD), np.array([3.0, -2.0, 4.0], dtype=LD)
        L = lambda q, w: (fr.quat_to_mat(q) * M.inertia) @ fr.quat_to_mat(q).T @ w  # noqa: E731
        p, q, v = fr.advance(M, [0, 0, 5.0], q0, [0, 0, 0, *w0], n)
        return float(fr.norm(L(q, v[3:]) - L(q0, w0)) / fr.norm(L(q0, w0)))
    M = fr.Model.from_desc(brick, LD)
    d1, d2 = drift(M, 50), drift(replace(M, h=M.h / 2), 100)
    print(f"[freebody] angular momentum drift over 0.2 s: {d1:.3e} at h, {d2:.3e} at h/2, ratio {d2 / d1:.3f}")
    assert d1 > 1e-4 and 0.45 <= d2 / d1 <= 0.55


# ------------------------------------------------------------------------------------------------ teeth
# one rule mutated at a time.  (The second is rule 5's last line the other way round: the reference carries the code's PYRAMID_R_SCALE = 1, the mutant MuJoCo's 2 mu^2.)
MUTATIONS = dict(solimp_mid_0_4=dict(solimp_mid=0.4), pyramid_r_scale_mujoco=dict(pyramid_r_scale=fr.MUJOCO_PYRAMID_R_SCALE), contact_point_at_surface=dict(contact_at_surface=True),
                 position_from_old_velocity=dict(position_from_old_velocity=True), mu_0_9=dict(mu=0.9), tangents_turned_45_degrees=dict(tangent_angle=np.pi / 4),
                 no_gyroscopic_term=dict(gyroscopic=False))


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_every_mutated_rule_is_caught_by_a_scenario(brick, mutation):
    """The mutated reference (float64) against the reference, on the brick's scenarios and with the bound the kernels get: at least one scenario exceeds it."""
    M = fr.Model.from_desc(brick)
    caught = []
    for nm in fs.SCENARIOS:
        ref = fs.reference(brick, nm, fs.SLOTS[0], brick.n_cycles)
        state = fs.start_state(M, nm, fs.SLOTS[0])
        for k in range(len(ref)):
            state = fr.advance(M, *state, brick.n_cycles, fr.mutated(**MUTATIONS[mutation]))
            err = fs.diffs(state, ref[k][0])
            caught += [(nm, k, q, err[q] / (fs.FACTOR * ref[k][1][q])) for q in err if ref[k][1][q] <= fs.CAP[q] and err[q] > fs.FACTOR * ref[k][1][q]]
    print(f"[freebody] {mutation}: caught by {sorted({c[0] for c in caught})}, largest error / bound {max((c[3] for c in caught), default=0):.3g}")
    assert caught, f"{mutation} passes every scenario: they are too tame"


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("family", [f for f in fs.FAMILIES if f != "cube_hull"])   # (the oracle keeps capsules whatever robot_geometry says: the hull family is the kernels' alone)
def test_oracle_follows_the_reference(family):
    """Every scenario of the family on an oracle batch, through get_box / set_box (get_stack / set_stack), compared after every policy step.

    Measured (largest error / floor per family, bound 8): cube 1.58, brick 1.34, stacking 1.33, handover 1.32, lifting 1.04; in most scenarios the oracle's box is
    the float64 reference to the last bit."""
    from oracle.oracle import OracleBatch
    B, desc, names = fs.family_batch(family, OracleBatch)
    try:
        worst = fs.run_family(family, B, desc, names)
    finally:
        B.close()
    print(f"[freebody] oracle {family}: largest error / floor {max(v[0] / v[1] for x in worst.values() for v in x.values() if v[1] > 0):.2f}")
