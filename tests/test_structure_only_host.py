"""Structure-only optimisation without a GPU: the numpy restatement of StructureOnlySolver::calc
(tests/structure_only_ref.py) against itself and the CPU oracle, and the case table the GPU tests compare against.

Every decision the reference takes on a table case stays away from its threshold, so the device (whose sums round
differently) takes the same one and no GPU test has to skip a point:
  | |b| - 0.001 | > 1e-3 * 0.001          (the gradient test, :148)
  | chi2 - new_chi2 | > 1e-6 * chi2        (the acceptance test, :179-180; a non-finite new_chi2 is far by nature)
These are conditions on the inputs (chosen here), not tolerances.
"""
import numpy as np
import pytest

import structure_only_ref as so
from g2o_amd import synth

B_MARGIN = 1e-3    # relative distance of |b| from 0.001
CHI_MARGIN = 1e-6  # |chi2 - new_chi2| relative to chi2


def _margins_ok(results, where):
    for i, r in results.items():
        for bn in r.b_norms:
            assert abs(bn - so.B_STOP) > B_MARGIN * so.B_STOP, (where, i, bn)
        for chi, new in r.chi_pairs:
            if np.isfinite(new):
                assert abs(chi - new) > CHI_MARGIN * abs(chi), (where, i, chi, new)


@pytest.mark.parametrize("key", [c.key for c in so.TABLE])
def test_case_properties_and_margins(key):
    s, new, results = so.reference(key)
    _margins_ok(results, key)
    for i, r in results.items():
        vs, row = s.row[i]
        before = so.track_chi2(s.track(i), vs.est[row])
        assert r.chi2 <= before, (key, i, r.chi2, before)               # chi2 never rises
        if vs.fixed[row]:                                               # fixed points untouched
            assert r.stop == so.FIXED and np.array_equal(r.est, vs.est[row])
            assert np.array_equal(new[vs.vtype][row], vs.est[row])
        # the accepted trials are exactly the ones that lowered chi2
        assert r.accepted == sum(1 for a, b in r.chi_pairs if np.isfinite(b) and a - b > 0), (key, i)
    for vs in s.prob.vertices:                                          # cameras / poses untouched
        if not np.any(vs.marginalized):
            assert np.array_equal(new[vs.vtype], vs.est)
    c = so.counts(results)
    assert c["accepted"] + c["rejected"] > 0
    print(key, c)


def test_table_covers_every_branch():
    seen = dict(rej_then_acc=0, exhausted=0, gradient=0, nonfinite=0, fixed=0)
    for c in so.TABLE:
        _, _, results = so.reference(c.key)
        for r in results.values():
            seen["rej_then_acc"] += r.rejected_then_accepted
            seen["exhausted"] += r.stop == so.TRIALS
            seen["gradient"] += r.stop == so.GRADIENT
            seen["nonfinite"] += r.nonfinite_trials > 0
            seen["fixed"] += r.stop == so.FIXED
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    assert any(c.max_trials in (1, 2) for c in so.TABLE)


def test_plane_case_hits_the_z0_plane():
    s, _, results = so.reference("plane")
    r = results[2]
    assert r.nonfinite_trials == 1 and r.rejected_then_accepted
    chi, new = r.chi_pairs[0]
    assert not np.isfinite(new)


def four_single_calcs(key, n=4):
    """n times calc(points, 1), each from the last one's estimates: (estimates, [results per call])."""
    c = so.CASES[key]
    s = so.Structure(c.make(), c.robust)
    est, out = None, []
    for _ in range(n):
        est, res = s.calc(1, c.max_trials, est=est)
        out.append(res)
    return s, est, out


def test_trajectories_differ():
    """calc(points, 4) carries mu over its iterations, four solve() calls restart it at 0.01 (:65-70, :86): on the
    trajectory case the two end more than 1e-4 apart (relative, in state), so the GPU test can tell them apart; the four
    single calls keep the margins too."""
    key = so.TRAJECTORY
    s, new4, _ = so.reference(key)
    _, new1, per_call = four_single_calcs(key)
    for k, res in enumerate(per_call):
        _margins_ok(res, f"{key} call {k}")
    vt = s.lm_sets[0].vtype
    rel = np.linalg.norm(new4[vt] - new1[vt]) / np.linalg.norm(new4[vt])
    print("calc(4) vs 4 x calc(1): relative state difference", rel)
    assert rel > 1e-4, rel


@pytest.mark.parametrize("which", ["ba", "se2xy"])
def test_initial_chi2_equals_oracle(oracle, which):
    if which == "ba":
        prob = synth.ba(num_cameras=6, num_points=150, obs_per_point=4, window=6)
    else:
        full = synth.slam2d(num_poses=40)
        prob = synth.Problem("se2xy", full.vertices, [e for e in full.edges if e.etype == synth.E_SE2_XY], 3, 2)
    ref = oracle.OracleGraph(prob).chi2()
    mine = so.Structure(prob).chi2()
    print(which, mine, ref)
    assert abs(mine - ref) <= 1e-9 * abs(ref), (mine, ref)


def test_ldlt_matches_solve_and_sign():
    rng = np.random.default_rng(1)
    for n in (2, 3):
        A = rng.standard_normal((n, n))
        M = A @ A.T + 0.01 * np.eye(n)
        b = rng.standard_normal(n)
        pos, solve = so.ldlt(M)
        assert pos and np.allclose(solve(b), np.linalg.solve(M, b), rtol=1e-10)
        assert not so.ldlt(-M)[0]
        bad = M.copy()
        bad[0, 0] = np.nan
        assert not so.ldlt(bad)[0]
    assert so.ldlt(np.zeros((3, 3)))[0]  # ZeroSign counts as positive (Eigen's isPositive)


def test_symbols_exported(g2o_amd_mod):
    assert "g2ohip_structure_only_calc" in g2o_amd_mod.EXPORTS
    assert hasattr(g2o_amd_mod.lib(), "g2ohip_structure_only_calc")
    assert hasattr(g2o_amd_mod.SparseOptimizer, "structure_only")
