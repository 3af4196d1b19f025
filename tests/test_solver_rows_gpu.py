"""The constraint rows of the ReachHuman stepper in the three mixes a substep can see, HIP vs oracle through the parity harness.  -m gpu.

Friction-loss rows take their D and limit from the model's constants, and the general row set-up (impedance, D) runs only in a substep in which a joint-limit or
contact row is active.  So one batch of 8 envs (shield OFF, 4 compared steps, compare() on everything) holds all three cases side by side:
  * envs 1 and 3 fold the arm onto the table (helpers.fold_onto_table): friction rows with contact rows;
  * envs 4 and 5 hold joints 4 and 5 against their upper range limits (action +1 on both): the position controller clips its goal at the limit and the joint
    settles a fraction of a milliradian beyond it, where the limit row pushes back -- friction rows with limit rows.  In env 5 both joints are beyond at the
    start of every compared step, in env 4 joint 5;
  * envs 0, 2, 6 and 7 move freely: friction rows alone.
That each case occurred is asserted from the oracle's states and contact lists alone.  A joint needs about seventy policy steps to reach its limit and the fold
about fifty to reach the table, so the oracle rolls forward on its own first (74 steps) and the device continues from its state: only the four compared steps
run on the device."""
import numpy as np
import pytest

import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST

pytestmark = pytest.mark.gpu

N, PREROLL, STEPS = 8, 74, 4
FOLDED, LIMITED, FREE = (1, 3), (4, 5), (0, 2, 6, 7)
JOINTS = (4, 5)
GEOM_TABLE = CONST["HRG_NRCAP"] + CONST["HRG_NHB"]


def test_friction_limit_and_contact_rows_in_one_batch():
    from helpers import fold_onto_table, make_pair
    from parity import Run, field, read_blocks, write_blocks
    O, G = make_pair(N, dict(shield_type="OFF", horizon=200, done_at_collision=False), clips=hrg.synthetic_clips(1, seed=0, min_frames=200, max_frames=300))
    run = Run(O, G, "solver rows", violent="base")
    lo, hi = (np.array([O.desc.jnt_range[i][side] for i in range(CONST["HRG_NV"])]) for side in (0, 1))
    rng = np.random.RandomState(3)

    def actions(k):
        a = rng.uniform(-0.3, 0.3, (N, 7))
        a[list(FOLDED)] = fold_onto_table(rng, N)[list(FOLDED)]
        a[list(LIMITED), 5] = 1.0
        if k >= 24:   # (the shorter way to its limit: both joints arrive together)
            a[list(LIMITED), 4] = 1.0
        return a

    for k in range(PREROLL):
        O.step(actions(k))
    assert not O.done.any() and not O.info[:, 11].any()
    write_blocks(G, run.kind, *read_blocks(O, run.kind))

    beyond = np.zeros((N, len(lo)), int)
    table = np.zeros(N, int)
    for s in run.steps(STEPS, lambda k: actions(PREROLL + k)):
        assert s.chk.all(), f"{s.msg}: an env left the comparison: {np.flatnonzero(~s.chk).tolist()}"
        s.compare()
        q0, q1 = field(s.pre_states, "qpos")[:, :len(lo)], field(s.o.states, "qpos")[:, :len(lo)]
        out0, out1 = (q0 < lo) | (q0 > hi), (q1 < lo) | (q1 > hi)
        beyond += out0   # a joint beyond its range when the step begins: its limit row is a candidate in the first substep at least
        # limit rows without contact rows
        assert (s.o.ncon[list(LIMITED)] == 0).all(), s.msg
        # friction rows alone: inside every range before and after the step, no contact
        free = list(FREE)
        assert not out0[free].any() and not out1[free].any() and (s.o.ncon[free] == 0).all(), s.msg
        # contact rows: an arm link on the table (by now the folding shoulder may sit at its own limit as well)
        for e in FOLDED:
            table[e] += int((s.o.pairs[e, :s.o.ncon[e], 1] == GEOM_TABLE).sum())
        s.resync()
    assert (beyond[5][list(JOINTS)] == STEPS).all() and beyond[4][5] == STEPS, f"joints 4 and 5 were meant to sit beyond their upper limits: {beyond[list(LIMITED)].tolist()}"
    assert (table[list(FOLDED)] > 0).all(), f"the fold was meant to bring an arm link of envs {FOLDED} onto the table: {table.tolist()}"
    run.finish()
