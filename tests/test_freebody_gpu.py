"""Every kernel family's free boxes against the independent reference (tests/freebody_ref.py), with the scenarios and the bound of tests/freebody_scenarios.py.
One batch per family, one scenario per env (stacking: one per cube, four per env), zero actions, state read back after every policy step.  -m gpu.

The reference of a (model, scenario) is computed once per process (freebody_scenarios.reference caches it; the cube, its hull variant and the stacking cubes
share one model).  `pytest -s` shows every error and floor."""
import pytest

import freebody_scenarios as fs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", list(fs.FAMILIES))
def test_kernel_follows_the_reference(family):
    """Before any comparison run_family asserts the test's own side: every contact listed is (table | floor, object), so the Newton system split; no env finished,
    reached a goal or crashed; and every scenario's floor is under its cap.

    Measured on an MI355X, largest error / floor per family (bound 8) and where: cube 1.80 (quat, error 1.9e-15 at a floor of 2.3e-15), brick 1.58 (pos, 1.7e-15),
    cube + hulls 1.80 (quat), stacking 1.80 (quat, 1.1e-15 at 2.4e-15), handover 1.51 (quat, 6.3e-15 at 8.5e-15), lifting 1.15 (quat, 3.8e-16 at 3.3e-16).
    The largest floors: 3.3e-15 m, 8.5e-15, 3.0e-13 m/s.  DESIGN.md section 2b has the table."""
    from human_robot_gym_amd._lib import HipBatch
    B, desc, names = fs.family_batch(family, HipBatch)
    try:
        worst = fs.run_family(family, B, desc, names)
    finally:
        B.close()
    print(f"[freebody] hip {family}: largest error / floor {max(v[0] / v[1] for x in worst.values() for v in x.values() if v[1] > 0):.2f}")
