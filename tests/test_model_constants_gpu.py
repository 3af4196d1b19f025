"""The model constants that hrg_batch_create has the device precompute (DevModel: expressions the step kernels used to evaluate in every substep) against the same
expressions evaluated again by one wave, through hrg_debug_model_constants.  -m gpu.

The stored entries replace a substep's own arithmetic, FP64 divisions of the device included, so they must be the bits that arithmetic gives: the tap returns them
next to what the kernels' expressions (the steppers' own row_D with its impedance code, run on a position term that arrives at run time) compute, and the two sets must
be equal bit for bit.  The ReachHuman model has eight friction-loss rows at most; the hammering model adds the nail's slide joint, a ninth."""
import ctypes

import numpy as np
import pytest

import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST

pytestmark = pytest.mark.gpu

NV = CONST["HRG_NV"]
COLUMNS = {"fric_D": (CONST["HRG_MC_FRIC_D"], NV + 1), "fric_lim": (CONST["HRG_MC_FRIC_LIM"], NV + 1), "fric_imp": (CONST["HRG_MC_FRIC_IMP"], NV + 1),
           "eul_hd": (CONST["HRG_MC_EUL_HD"], NV), "eul_rhd": (CONST["HRG_MC_EUL_RHD"], 2), "eul_fingers": (CONST["HRG_MC_EUL_FINGERS"], 1),
           "rcap_mid": (CONST["HRG_MC_RCAP_MID"], 3 * CONST["HRG_NRCAP"])}


def _tap(env_id):
    """(stored, recomputed, desc): the two rows of hrg_debug_model_constants for a small batch of `env_id`"""
    from human_robot_gym_amd._lib import HipBatch
    from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
    clips = task_clips(env_id, 2, min_frames=300, max_frames=400)
    desc = hrg.build_model_desc(dict(task_env_kwargs(env_id)), n_clips=clips.n_clips, env_id=env_id)
    G = HipBatch(desc, clips, 2)
    out = np.full((2, CONST["HRG_MC_DIM"]), np.nan)
    try:
        assert G.lib.hrg_debug_model_constants(G.h, out.ctypes.data_as(ctypes.c_void_p)) == 0, G.lib.hrg_last_error().decode()
    finally:
        G.close()
    return out[0], out[1], desc


@pytest.fixture(scope="module", params=["ReachHuman", "CollaborativeHammeringCart"])
def tapped(request):
    return (request.param,) + _tap(request.param)


def test_columns_cover_the_tap():
    assert sorted(o for o, _ in COLUMNS.values()) == sorted(set(o for o, _ in COLUMNS.values()))
    assert sum(n for _, n in COLUMNS.values()) == CONST["HRG_MC_DIM"]


def test_stored_constants_are_the_bits_the_kernels_compute(tapped):
    env_id, stored, again, _ = tapped
    assert np.isfinite(stored).all() and np.isfinite(again).all()
    for name, (o, n) in COLUMNS.items():
        a, b = stored[o:o + n], again[o:o + n]
        assert (a.view(np.uint64) == b.view(np.uint64)).all(), f"{env_id} {name}: stored {a.tolist()} recomputed {b.tolist()}"


def test_friction_rows_are_the_models(tapped):
    """which rows carry a constant, and that it is the expression of the model's numbers (IEEE here, the device's division there: a few ulp)"""
    env_id, stored, _, desc = tapped
    floss = np.array(list(desc.jnt_frictionloss)[:NV] + [desc.hm_nail_frictionloss])
    invw = np.array(list(desc.dof_invweight0)[:NV] + [desc.hm_nail_invweight])
    has = (floss > 0) & (invw > 0)
    assert has[:NV].any()
    assert has[NV] == (env_id == "CollaborativeHammeringCart")
    o, n = COLUMNS["fric_D"]
    D = stored[o:o + n]
    o, n = COLUMNS["fric_lim"]
    lim = stored[o:o + n]
    o, n = COLUMNS["fric_imp"]
    imp = stored[o:o + n]
    assert (D[~has] == 0).all() and (lim[~has] == 0).all() and (imp[~has] == 0).all()
    d0 = desc.solimp[0]
    assert (imp[has] == d0).all()
    np.testing.assert_allclose(D[has], 1.0 / ((1 - d0) / d0 * invw[has]), rtol=1e-14, atol=0)
    np.testing.assert_allclose(lim[has], floss[has] / D[has], rtol=1e-14, atol=0)


def test_damping_constants_are_the_models(tapped):
    _, stored, _, desc = tapped
    damp, h = np.array(list(desc.jnt_damping)[:NV]), desc.timestep
    o, n = COLUMNS["eul_hd"]
    assert (stored[o:o + n] == h * damp).all()   # one product: no room for a difference
    fingers = (h * damp[NV - 2:] > 0).all()
    assert fingers, "both models damp the fingers: the reciprocals are in use"
    assert stored[COLUMNS["eul_fingers"][0]] == 1.0
    o, n = COLUMNS["eul_rhd"]
    np.testing.assert_allclose(stored[o:o + n], 1.0 / (h * damp[NV - 2:]), rtol=1e-15, atol=0)   # one division: within a few ulp of IEEE


def test_capsule_mid_points_are_the_models(tapped):
    _, stored, _, desc = tapped
    p1, p2 = (np.array([list(r) for r in p])[:CONST["HRG_NRCAP"]] for p in (desc.rcap_p1, desc.rcap_p2))
    o, n = COLUMNS["rcap_mid"]
    assert (stored[o:o + n].reshape(-1, 3) == 0.5 * (p1 + p2)).all()   # a sum and a halving: IEEE on both sides
    assert np.abs(p2 - p1).max() > 0
