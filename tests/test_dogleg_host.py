"""Powell's dogleg without a GPU: the two scalar decisions the device kernels and the host share
(g2ohip_dogleg_blend, g2ohip_dogleg_next_delta; common.hpp) against numpy bit for bit, and the reference loop
(tests/dogleg_ref.py over the CPU oracle) on the inputs the GPU trajectory tests compare against: it visits every
branch of optimization_algorithm_dogleg.cpp:57-208, and every decision it takes there is far from its threshold.

g2ohip_set_algorithm needs a graph handle, which needs a device: the algorithm names (dl_hip_* accepted, dl_pcg
refused) are checked in tests/test_gpu_dogleg.py.
"""
import numpy as np
import pytest

import dogleg_ref
from dogleg_ref import STEP_DL, STEP_GN, STEP_SD

# margins every compared decision keeps (conditions on the inputs, not tolerances)
RHO_MARGIN = 1e-3     # rho from 0, 0.25 and 0.75
NORM_MARGIN = 1e-6    # |hgn| and |hsd| from delta, relative
CHI_DROP = 1e-6       # chi2 falls by more than this, relative, in every compared iteration


# ---------------------------------------------------------------- the shared scalar functions
def _blend_numpy(hgn_norm, hsd_norm, hsd_sq, c, bma_sq, delta):
    """optimization_algorithm_dogleg.cpp:153-175 in IEEE doubles, one rounding per operation."""
    f = np.float64
    hgn_norm, hsd_norm, hsd_sq, c, bma_sq, delta = map(f, (hgn_norm, hsd_norm, hsd_sq, c, bma_sq, delta))
    if hgn_norm < delta:
        return STEP_GN, f(0.0), f(1.0)
    if hsd_norm > delta:
        return STEP_SD, delta / hsd_norm, f(0.0)
    disc = np.sqrt(c * c + bma_sq * (delta * delta - hsd_sq))
    if c <= 0.0:
        beta = (-c + disc) / bma_sq
    else:
        beta = (delta * delta - hsd_sq) / (c + disc)
    return STEP_DL, f(1.0) - beta, beta


def _vectors(rng, n, scale_sd):
    """A Gauss-Newton step and a shorter steepest-descent step, and the sums the blend takes."""
    hgn = rng.standard_normal(n)
    hsd = scale_sd * (hgn + 0.7 * rng.standard_normal(n))
    bma = hgn - hsd
    return (float(np.linalg.norm(hgn)), float(np.linalg.norm(hsd)), float(hsd @ hsd), float(hsd @ bma),
            float(bma @ bma))


def _blend_cases():
    rng = np.random.default_rng(5)
    cases = []
    for k in range(400):
        n = int(rng.integers(3, 40))
        hgn_n, hsd_n, hsd_sq, c, bma_sq = _vectors(rng, n, rng.uniform(0.05, 1.4))
        lo, hi = min(hgn_n, hsd_n), max(hgn_n, hsd_n)
        for delta in (hi * rng.uniform(1.01, 3.0), lo * rng.uniform(0.1, 0.99), rng.uniform(lo, hi)):
            cases.append((hgn_n, hsd_n, hsd_sq, c, bma_sq, float(delta)))
    # the boundaries: |hgn| == delta is not a GN step, |hsd| == delta is not an SD step
    hgn_n, hsd_n, hsd_sq, c, bma_sq = _vectors(rng, 12, 0.4)
    cases.append((hgn_n, hsd_n, hsd_sq, c, bma_sq, hgn_n))
    cases.append((hgn_n, hsd_n, hsd_sq, c, bma_sq, hsd_n))
    cases.append((hgn_n, hsd_n, hsd_sq, c, bma_sq, float(np.nextafter(hgn_n, np.inf))))
    cases.append((hgn_n, hsd_n, hsd_sq, c, bma_sq, float(np.nextafter(hsd_n, -np.inf))))
    # both beta branches by hand: c < 0, c == 0, c > 0 with |hsd| <= delta <= |hgn|
    for cc in (-0.3, 0.0, 0.3, 1e-300, -1e-300):
        cases.append((2.0, 0.5, 0.25, cc, 3.1, 1.25))
    return cases


def test_blend_matches_numpy_bitwise(g2o_amd_mod):
    seen, branches = set(), set()
    for case in _blend_cases():
        step, c0, c1 = g2o_amd_mod.dogleg_blend(*case)
        rs, r0, r1 = _blend_numpy(*case)
        assert step == rs, (case, step, rs)
        assert c0 == float(r0) and c1 == float(r1), (case, (c0, c1), (float(r0), float(r1)))
        seen.add(step)
        if step == STEP_DL:
            branches.add(case[3] <= 0.0)
    assert seen == {STEP_SD, STEP_GN, STEP_DL}
    assert branches == {True, False}  # both beta formulas


def test_blend_boundaries(g2o_amd_mod):
    """hgn_norm == delta is not GN (strict <), hsd_norm == delta is not SD (strict >): both are dogleg steps."""
    assert g2o_amd_mod.dogleg_blend(2.0, 0.5, 0.25, 0.1, 2.0, 2.0)[0] == STEP_DL
    assert g2o_amd_mod.dogleg_blend(2.0, 0.5, 0.25, 0.1, 2.0, 0.5)[0] == STEP_DL
    assert g2o_amd_mod.dogleg_blend(2.0, 0.5, 0.25, 0.1, 2.0, float(np.nextafter(2.0, 3.0)))[0] == STEP_GN
    assert g2o_amd_mod.dogleg_blend(2.0, 0.5, 0.25, 0.1, 2.0, float(np.nextafter(0.5, 0.0)))[0] == STEP_SD
    # at delta == |hsd| the dogleg step is the steepest-descent step itself: beta = 0
    step, c0, c1 = g2o_amd_mod.dogleg_blend(2.0, 0.5, 0.25, 0.1, 2.0, 0.5)
    assert (c0, c1) == (1.0, 0.0)


def _next_delta_numpy(delta, rho, hdl_norm):
    delta, rho, hdl_norm = np.float64(delta), np.float64(rho), np.float64(hdl_norm)
    if rho > 0.75:
        return max(delta, np.float64(3.0) * hdl_norm)
    if rho < 0.25:
        return delta * np.float64(0.5)
    return delta


def test_next_delta_matches_numpy_bitwise(g2o_amd_mod):
    rng = np.random.default_rng(6)
    rhos = np.concatenate([rng.uniform(-2, 2, 2000), [0.25, 0.75, np.nextafter(0.25, 0), np.nextafter(0.25, 1),
                                                      np.nextafter(0.75, 0), np.nextafter(0.75, 1), 0.0, -1e300,
                                                      1e300]])
    for rho in rhos.tolist():
        delta, hdl = float(10.0 ** rng.uniform(-6, 4)), float(10.0 ** rng.uniform(-6, 4))
        got = g2o_amd_mod.dogleg_next_delta(delta, rho, hdl)
        assert got == float(_next_delta_numpy(delta, rho, hdl)), (delta, rho, hdl, got)
    # exactly at the thresholds nothing changes (rho > 0.75 and rho < 0.25 are strict)
    assert g2o_amd_mod.dogleg_next_delta(1.5, 0.25, 100.0) == 1.5
    assert g2o_amd_mod.dogleg_next_delta(1.5, 0.75, 100.0) == 1.5
    assert g2o_amd_mod.dogleg_next_delta(1.5, float(np.nextafter(0.75, 1)), 100.0) == 300.0
    assert g2o_amd_mod.dogleg_next_delta(1.5, float(np.nextafter(0.75, 1)), 0.1) == 1.5  # max(delta, 3 |hdl|)
    assert g2o_amd_mod.dogleg_next_delta(1.5, float(np.nextafter(0.25, 0)), 100.0) == 0.75


# ---------------------------------------------------------------- the reference loop on the compared inputs
def _steps(its):
    return [[s for s, _ in it.trials] for it in its]


def _margins(key, its):
    for k, it in enumerate(its):
        if it.result == dogleg_ref.FAIL:
            continue
        print(f"{key} it {k}: chi2 {it.chi2_before:.9g} -> {it.chi2:.9g} tries {it.tries} delta {it.delta:.6g} "
              f"trials {[(s, float(f'{r:.4g}')) for s, r in it.trials]} lambda {it.lam:g} wasPD {it.was_pd} "
              f"rho margin {it.rho_margin:.3g} norm margin {it.norm_margin:.3g}")
        assert it.rho_margin >= RHO_MARGIN, (key, k, it.trials)
        assert it.norm_margin >= NORM_MARGIN, (key, k, it.norm_margin)
        assert it.chi2_before - it.chi2 > CHI_DROP * it.chi2_before, (key, k, it.chi2_before, it.chi2)


def test_ref_c1_small_delta(oracle):
    n, its, _ = dogleg_ref.reference("C1_d0.05", oracle)
    assert n == 8
    assert _steps(its) == [[STEP_SD]] * 2 + [[STEP_DL]] * 5 + [[STEP_GN]]
    assert all(it.was_pd and it.lam == 1e-7 for it in its)
    _margins("C1_d0.05", its)


def test_ref_c2(oracle):
    n, its, _ = dogleg_ref.reference("C2_d1", oracle)
    assert n == 6
    assert _steps(its) == [[STEP_SD]] + [[STEP_DL]] * 4 + [[STEP_GN]]
    _margins("C2_d1", its)


def test_ref_s2_default_delta(oracle):
    """Schur 3/2 from the default delta 1e4: most trials are rejected, and rejected trials only halve delta."""
    n, its, _ = dogleg_ref.reference("S2_default", oracle)
    assert n == 8
    trials = [t for it in its for t in it.trials]
    assert len(trials) == 35 and sum(1 for _, rho in trials if not rho > 0) == 27
    assert _steps(its)[0] == [STEP_GN] * 9 + [STEP_DL]
    _margins("S2_default", its)


def test_ref_s2_unit_delta(oracle):
    n, its, _ = dogleg_ref.reference("S2_d1", oracle)
    assert n == 8
    st = _steps(its)
    assert st[0] == [STEP_SD] and st[1] == [STEP_SD] and st[2] == [STEP_DL]
    # the third iteration's rho lies between 0.25 and 0.75: delta stays as it is
    assert 0.25 < its[2].trials[0][1] < 0.75 and its[2].delta == its[1].delta
    assert all(s == STEP_DL for it in st[3:] for s in it)
    assert any(it.tries > 1 for it in its[3:])  # rejected dogleg trials
    _margins("S2_d1", its)


def test_ref_c4(oracle):
    """Schur 6/3: rho of a plain GN step is about 0.5 because the model's gain counts Hpp only."""
    n, its, _ = dogleg_ref.reference("C4_d0.05", oracle)
    assert n == 5
    assert _steps(its) == [[STEP_DL]] * 4 + [[STEP_GN]]
    assert abs(its[4].trials[0][1] - 0.5) < 0.05
    _margins("C4_d0.05", its)


def test_ref_indefinite(oracle):
    """H indefinite: the damping loop climbs from 1e-7 by factors of ten until the factorization succeeds."""
    n, its, _ = dogleg_ref.reference("C1_indef-0.2", oracle)
    assert n == 3
    assert not any(it.was_pd for it in its)
    climb = [0.0] + [1e-7 * 10.0 ** k for k in range(1, 10)]
    assert np.allclose(its[0].lambdas_tried, climb, rtol=1e-12) and its[0].lambdas_tried[-1] == pytest.approx(100.0)
    assert [it.lambdas_tried[-1] for it in its] == pytest.approx([100.0, 20.0, 4.0])
    assert [it.lam for it in its] == pytest.approx([20.0, 4.0, 0.8])
    for k, it in enumerate(its):
        # -lambda_min(H) a factor 2 away from every damping value tried: no factorization sits at the edge of PD
        neg = -it.hpp_min_eig
        assert neg > 0, (k, neg)
        for lam in it.lambdas_tried:
            assert lam >= 2 * neg or lam <= neg / 2, (k, lam, neg)
            assert (lam > neg) == (lam == it.lambdas_tried[-1]), (k, lam, neg)
    _margins("C1_indef-0.2", its)


def test_ref_indefinite_fail(oracle):
    """The smallest eigenvalue is below -1e3: lambda passes maxLambda, Fail at iteration 0, optimize returns 0."""
    n, its, _ = dogleg_ref.reference("C1_indef-0.5", oracle)
    assert n == 0 and len(its) == 1
    it = its[0]
    assert it.result == dogleg_ref.FAIL and it.lam == 1e3 and not it.was_pd and it.tries == 1
    assert it.lambdas_tried[-1] == pytest.approx(1e3) and len(it.lambdas_tried) == 11
    assert -it.hpp_min_eig >= 2e3
