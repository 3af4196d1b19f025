"""The primitive narrowphase of the kernels (seg_seg, seg_box, cap_box_two, box_box2 through hrg_debug_narrowphase, as each kernel variant compiles them) on the cases
of tests/narrowphase_cases.py: through the checker of tests/narrowphase_ref.py, and side by side with the oracle (equal counts, contacts in order, 1e-12 on every
number: the device's square root and division are not the host's, so nothing is compared bit for bit).  DESIGN.md section 2d."""
import ctypes
import functools

import numpy as np
import pytest

import human_robot_gym_amd as hrg
import narrowphase_cases as nc
import narrowphase_ref as nr
from human_robot_gym_amd._cstruct import CONST
from narrowphase_ref import BOXBOX, CAPBOX, SEGBOX, SEGSEG
from test_narrowphase import KIND_NAMES, judge

pytestmark = pytest.mark.gpu

SEGMENT_KINDS = (SEGSEG, SEGBOX, CAPBOX)
ALL_KINDS = SEGMENT_KINDS + (BOXBOX,)
# variant -> (env_id, build_model_desc keywords, the kinds its kernels compile)
VARIANTS = {
    "stacking": ("CollaborativeStackingCart", {}, ALL_KINDS),
    "hammering": ("CollaborativeHammeringCart", {}, ALL_KINDS),
    "lifting": ("CollaborativeLiftingCart", {}, ALL_KINDS),
    "cube, capsules": ("PickPlaceHumanCart", {}, SEGMENT_KINDS),
    "cube, hulls": ("PickPlaceHumanCart", dict(robot_geometry="hull"), SEGMENT_KINDS),
}
_batches = {}


def _batch(variant):
    if variant not in _batches:
        from human_robot_gym_amd._lib import HipBatch
        from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
        env_id, desc_kw, _ = VARIANTS[variant]
        clips = task_clips(env_id, 2, min_frames=300, max_frames=320)
        _batches[variant] = HipBatch(hrg.build_model_desc(dict(task_env_kwargs(env_id)), n_clips=clips.n_clips, env_id=env_id, **desc_kw), clips, 1)
    return _batches[variant]


def device_outputs(G, kind, Q):
    Q = np.ascontiguousarray(Q, np.float64)
    out = np.full((len(Q), nr.NP_ODIM), np.nan)
    rc = G.lib.hrg_debug_narrowphase(G.h, kind, Q.ctypes.data_as(ctypes.c_void_p), len(Q), out.ctypes.data_as(ctypes.c_void_p))
    return rc, out


@functools.lru_cache(None)
def _oracle(kind):
    from oracle import oracle
    oracle.build()
    return nc.oracle_outputs(oracle.load(), kind, nc.CASES[kind]()[1])


def test_layout_is_the_headers():
    assert (CONST["HRG_NP_SEGSEG"], CONST["HRG_NP_SEGBOX"], CONST["HRG_NP_CAPBOX"], CONST["HRG_NP_BOXBOX"]) == (SEGSEG, SEGBOX, CAPBOX, BOXBOX)
    assert (CONST["HRG_NP_QDIM"], CONST["HRG_NP_ODIM"]) == (nr.NP_QDIM, nr.NP_ODIM) and CONST["HRG_NP_MAX"] >= 2000


@pytest.mark.parametrize("variant,kind", [(v, k) for v, (_, _, kinds) in VARIANTS.items() for k in kinds], ids=lambda x: KIND_NAMES.get(x, x) if isinstance(x, int) else x)
def test_device_against_the_reference_and_the_oracle(variant, kind):
    names, Q = nc.CASES[kind]()
    rc, out = device_outputs(_batch(variant), kind, Q)
    assert rc == 0 and np.isfinite(out).all()
    V = judge(kind, Q, out, names, f"device ({variant})")
    side_by_side(kind, names, V, out, _oracle(kind), f"device ({variant})")


def side_by_side(kind, names, V, out, ref, who):
    """Device and oracle, number by number at 1e-12: equal answers and counts, the contacts in order.  Where the checker says that a witness is not unique (V.free:
    a stretch of closest pairs; a box pair with a corner on the other outline, where rounding decides under which index a candidate exists) two correct outputs
    need not name the same one: the closest pair is then left to the checker, the contacts are matched as a set.  Two segments' closest pair is conditioned as
    1 / sin^2 of their angle (V.wit_tol): measured on an MI355X, 1.6e-11 m along the segments at sin^2 = 1e-5 with the distances equal to 1e-17, and at most
    1.2e-15 on every number held to 1e-12."""
    worst = 0.0
    for name, v, o, r in zip(names, V, out, ref):
        if v.knife:
            continue
        tol = np.full(len(o), 1e-12)
        if kind in (SEGSEG, SEGBOX, CAPBOX):
            tol[1:7] = np.inf if v.free else v.wit_tol
            assert abs(np.sqrt(o[0]) - np.sqrt(r[0])) <= 1e-12, f"{who} {name}: distance {np.sqrt(o[0])!r}, the oracle's {np.sqrt(r[0])!r}"
        if kind == CAPBOX:
            assert o[7] == r[7], f"{who} {name}: answers {o[7]}, the oracle {r[7]}"
        if kind == BOXBOX:
            assert o[0] == r[0], f"{who} {name}: {int(o[0])} contacts, the oracle {int(r[0])}"
            if v.free:   # as a set: every contact of the one next to a contact of the other
                n = int(o[0])
                co, cr = o[1:1 + 7 * n].reshape(n, 7), r[1:1 + 7 * n].reshape(n, 7)
                o = o.copy()
                o[1:1 + 7 * n] = np.array([co[np.argmin(np.abs(co - c).max(1))] for c in cr]).ravel()
                assert len({int(np.argmin(np.abs(co - c).max(1))) for c in cr}) == n, f"{who} {name}: the contacts do not pair up with the oracle's"
        gap = np.abs(o - r)
        worst = max(worst, float(gap[np.isfinite(tol) & (tol <= 1e-12)].max()))
        assert (gap <= tol).all(), f"{who} {name}: device {o.tolist()} oracle {r.tolist()} (bounds {tol.tolist()})"
    print(f"[narrowphase] {who} {KIND_NAMES[kind]}: device and oracle differ by at most {worst:.3g} on the numbers held to 1e-12")


def test_the_finding_keeps_its_four_corners_on_the_device():
    names, Q = nc.box_box_cases()
    sel = [k for k, name in enumerate(names) if name.startswith("the parallelogram of the finding")]
    for variant in ("stacking", "hammering", "lifting"):
        rc, out = device_outputs(_batch(variant), BOXBOX, Q[sel])
        assert rc == 0
        for q, o in zip(Q[sel], out):
            V = nr.check_box_box(q, o)
            assert o[0] == 4 and not V.bad and V.stats["ratio"] > 1 - 1e-9, (variant, V.bad, V.stats)


def test_what_a_variant_does_not_compile_is_refused():
    UNSUPPORTED, INVALID = CONST["HRG_ERR_UNSUPPORTED"], CONST["HRG_ERR_INVALID"]
    _, Q = nc.box_box_cases()
    for variant in ("cube, capsules", "cube, hulls"):
        assert device_outputs(_batch(variant), BOXBOX, Q[:8])[0] == UNSUPPORTED
    G = _batch("stacking")
    one = np.zeros((CONST["HRG_NP_MAX"] + 1, nr.NP_QDIM))
    out = np.zeros((len(one), nr.NP_ODIM))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert G.lib.hrg_debug_narrowphase(G.h, SEGSEG, p(one), len(one), p(out)) == INVALID          # more than one launch
    assert G.lib.hrg_debug_narrowphase(G.h, SEGSEG, p(one), 0, p(out)) == INVALID
    assert G.lib.hrg_debug_narrowphase(G.h, 4, p(one), 1, p(out)) == INVALID


def test_a_partial_wave():
    """n that is no multiple of the lanes a wave serves (64, 32, 6): the last wave runs with some of its lanes idle"""
    G = _batch("stacking")
    for kind, n in ((SEGSEG, 65), (SEGBOX, 33), (CAPBOX, 1), (BOXBOX, 7)):
        names, Q = nc.CASES[kind]()
        rc, out = device_outputs(G, kind, Q[:n])
        assert rc == 0
        side_by_side(kind, names[:n], [nr.CHECK[kind](q, o) for q, o in zip(Q[:n], out)], out, _oracle(kind)[:n], f"device, {n} queries")


def teardown_module():
    for G in _batches.values():
        G.close()
    _batches.clear()
