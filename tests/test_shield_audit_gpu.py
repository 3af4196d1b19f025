"""The shield of the HIP step kernels held to the rules of DESIGN.md section 2c: the four scenario batches of tests/shield_scenarios.py on HipBatch, one shield cycle
per policy step, every cycle audited by tests/shield_audit.py from (state before, state after, reach-capsule taps).  An oracle twin is set to the GPU's state before
every cycle and gets the same actions; the test prints, per check, the largest residual of the kernels, of the oracle and between the two (the table of section 2c).
(helpers.make_pair is not used: the scenarios edit the model description after it is built.)"""
import numpy as np
import pytest

import shield_audit as A
import shield_scenarios as S

pytestmark = pytest.mark.gpu

LATE = "a joint's pieces end after T"
TWIN_EVERY = 4      # the twin is stepped and compared every cycle, audited every 4th (its residuals over every cycle are the CPU test's)


def _between(stats, key, x, y):
    stats[key] = max(stats.get(key, 0.0), float(np.max(np.abs(np.asarray(x, float) - np.asarray(y, float)) / (1.0 + np.abs(np.asarray(y, float))))))


@pytest.mark.parametrize("scn", S.SCENARIOS, ids=lambda s: s.name)
def test_hip_keeps_every_rule(scn):
    from human_robot_gym_amd._lib import HipBatch
    from oracle.oracle import OracleBatch
    d = scn.desc()
    P = A.params(d)
    assert d.n_cycles == 1
    G, O, F = HipBatch(scn.desc(), scn.clips(), scn.n), OracleBatch(scn.desc(), scn.clips(), scn.n), OracleBatch(scn.desc(), scn.clips(), scn.n)
    G.enable_taps(True)
    scn.place(G); O.reset(); scn.place(F)
    cov, cov_f = S.Coverage(scn, d), S.Coverage(scn, d)
    sg, so, sb, viol, late_g, late_o, differ = {}, {}, {}, [], [], [], []
    free = S.cycles(F, scn)
    for k, b, a, rc, hc, nh, ao, rco, hco, nho in S.cycles(G, scn, twin=O):
        viol += [dict(v, cycle=k) for v in A.audit_cycle(P, b, a, rc, hc, nh, sg, rules=A.RULES + (A.SYNC,))]
        cov.add(b, a)
        _, fb, fa = next(free)[:3]
        cov_f.add(fb, fa)
        if k % TWIN_EVERY == 0:
            late_o += [(v["env"], k) for v in A.audit_cycle(P, b, ao, rco, hco, nho, so, rules=A.RULES + (A.SYNC,)) if v["quantity"] == LATE]
            late_g += [(v["env"], k) for v in viol if v["quantity"] == LATE and v["cycle"] == k]
        # the two backends against each other, one cycle from the same state
        differ += [(k, int(e), f) for f, x, y in (("is_safe", a["is_safe"], ao["is_safe"]), ("new_goal", a["new_goal"], ao["new_goal"]), ("n_hcaps", nh, nho))
                   for e in np.nonzero(x != y)[0]]
        ss = np.linspace(0.0, 1.0, 5)[None, :] * ao["ltt"]["T"][:, None]
        for i, nm in enumerate(("q", "q'")):
            _between(sb, f"R1.ltt {nm}", A.ltt_eval(a["ltt"], ss)[i], A.ltt_eval(ao["ltt"], ss)[i])
        for f in ("path_s", "path_v", "path_a"):
            _between(sb, f"R2.{f}", a[f], ao[f])
        for f in ("des_q", "des_v", "des_a"):
            _between(sb, f"R3.{f}", a[f], ao[f])
        safe = a["is_safe"] != 0
        if safe.any():
            _between(sb, "R4.rcaps", rc[safe], rco[safe])
            _between(sb, "R5.hcaps", hc[safe][:, :nh.min()], hco[safe][:, :nh.min()])
    G.close(); O.close(); F.close()
    for name, st in (("hip", sg), ("oracle", so), ("hip - oracle", sb)):
        for key in sorted(st):
            print(f"[shield-audit-gpu] {scn.name}: {name}: {key} = {st[key]:.3g}")
    print(f"[shield-audit-gpu] {scn.name}: coverage {cov.c}")
    bad = [v for v in viol if v["rule"] != A.SYNC]
    by_rule = {r: sum(v["rule"] == r for v in bad) for r in A.RULES}
    assert not bad, f"{len(bad)} violations {by_rule}, first: {bad[:5]}"                      # the rules first: they say what is wrong, the twin only that something is
    assert not differ, f"verdict, swap or capsule count differs from the oracle twin in {len(differ)} env-cycles, first (cycle, env, field): {differ[:5]}"
    print(f"[shield-audit-gpu] {scn.name}: D28 (a joint stretched past T): {len(late_g)} env-cycles of the {scn.n * scn.cycles // TWIN_EVERY} audited on both sides")
    assert sorted(late_g) == sorted(late_o)                 # deviation D28 is the same on both sides
    assert sg["n.knife"] <= 0.01 * scn.n * scn.cycles       # verdicts on a knife edge cannot be audited: at most 1 % of the env-cycles
    assert cov.c["episode_ends"] == 0
    S.assert_coverage(scn, cov.c)
    assert cov.c == cov_f.c, "the kernels' run reaches other things than the oracle's free run"
