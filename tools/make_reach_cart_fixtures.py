#!/usr/bin/env python3
"""Record what the reference's ReachHumanCartExpert computes: python tools/make_reach_cart_fixtures.py REFERENCE_CHECKOUT [OUT.npz]

Runs the reference's own class (human_robot_gym/demonstrations/experts/reach_human_cart_expert.py) on recorded inputs and writes
tests/golden/reach_cart_ref.npz: inputs, parameters, outputs.  Build machine only: no test reads the checkout.

The stand-ins are those of tools/make_expert_fixtures.py (bare package shells, a `gym` that carries `Space` and `spaces.Box`), and like there
signal_to_noise_ratio = 1: the reference's noise draws (numpy's PCG64) are not reproduced by the stepper's counter hash, and at 1 they cannot show.
Rows whose goal difference comes within 1e-9 of a clip threshold (+-action limit) are dropped and drawn again.
"""
import os
import sys

import numpy as np

from make_expert_fixtures import CART_HIGH, CART_LOW, MARGIN, ROWS, f32, install_stand_ins


def main():
    ref = os.path.abspath(sys.argv[1])
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "tests", "golden", "reach_cart_ref.npz")
    Box = install_stand_ins(ref)
    from human_robot_gym.demonstrations.experts.reach_human_cart_expert import ReachHumanCartExpert
    rng = np.random.RandomState(20250)
    ex = ReachHumanCartExpert(Box([-np.inf] * 3, [np.inf] * 3), Box(CART_LOW, CART_HIGH), signal_to_noise_ratio=1, delta_time=0.01, seed=0)
    lim = CART_HIGH[0]
    # goal differences inside and beyond the action limit: the sampling space is half a metre wide, the limit 0.1 m
    pool = f32(rng.uniform(-0.6, 0.6, (4 * ROWS, 3)) * rng.choice([1.0, 0.2, 0.02], (4 * ROWS, 1)))
    keep = np.all(np.abs(np.abs(pool) - lim) >= MARGIN, axis=1)
    gd = pool[keep][:ROWS]
    assert gd.shape == (ROWS, 3)
    act = np.array([ex(dict(goal_difference=g)) for g in gd])
    assert act.shape == (ROWS, 4) and (np.abs(gd) > lim).any(axis=1).sum() > 50 and (np.abs(gd) < lim).all(axis=1).sum() > 50
    np.savez_compressed(out, cart_goal_difference=gd, cart_action=act, cart_low=np.array(CART_LOW), cart_high=np.array(CART_HIGH),
                        dropped_share=np.float64(1.0 - keep.mean()),
                        note=np.array("outputs of human_robot_gym's ReachHumanCartExpert (signal_to_noise_ratio=1, delta_time=0.01), run with the stand-ins of "
                                      "tools/make_expert_fixtures.py; inputs f32-representable; rows within 1e-9 of a clip threshold dropped"))
    print("wrote", out, os.path.getsize(out), "bytes; dropped share", 1.0 - keep.mean())


if __name__ == "__main__":
    main()
