"""The supernodal Cholesky (csrc/cholesky.hip) called directly through g2ohip_linear_solve_ccs: front and panel
edges, accuracy against an extended-precision reference, not-positive-definite detection at every elimination position
and the forced factorization schedules. The matrices, the longdouble reference and LAPACK's fp64 figures come from
chol_cases.py; test_chol_cases.py checks on the CPU that those inputs are what they are meant to be.

Tolerances. Nothing is compared with the device's own earlier output. The normwise backward error
eta = ||b - A x|| / (||A||_2 ||x|| + ||b||) (residual in longdouble) may be at most 64 x the eta of LAPACK's fp64
Cholesky (scipy cho_factor / cho_solve) on the same system, and the relative forward error against the longdouble
solution at most 64 x LAPACK's, with a floor of 64 x 2.2e-16. The 64 is the pivot-reciprocal error chol32 was
documented with (rsq + one Newton step, ~3.75e-15) over the unit roundoff 1.1e-16, ~34, doubled because the factor
enters A as L L^T; it is not headroom for anything else. (These tests found that step behind forward errors of up to
77 x LAPACK's; chol32 now takes a third-order step and sits at 1 x in the median) Every figure is printed (CHOLFIG lines) before it is asserted.
"""
import numpy as np
import pytest

import chol_cases as cc
from test_gpu_parity import SCHEDULES

pytestmark = pytest.mark.gpu

CAP = 64.0
FWD_FLOOR = CAP * cc.EPS


def _solve(mod, A, bd, b, ccs=None, info=False):
    Ap, Ai, Ax = ccs or cc.upper_ccs(A)
    return mod.linear_solve_ccs(A.shape[0], Ap, Ai, Ax, b, block_dim=bd, info=info)


def _judge(label, A, norm2, b, x, x_ref, lapack, bad):
    """The criteria of the shape sweep for one solution; misses are appended to `bad`."""
    if not b.any():
        if x.any():
            bad.append(f"{label}: b = 0 must give x = 0 exactly, got max |x| = {np.abs(x).max():.3e}")
        return
    eta, fwd = cc.errors(A, b, x, x_ref, norm2)
    print(f"CHOLFIG {label} gpu_eta={eta:.3e} lapack_eta={lapack[0]:.3e} gpu_fwd={fwd:.3e} lapack_fwd={lapack[1]:.3e}")
    if not eta <= CAP * lapack[0]:
        bad.append(f"{label}: eta {eta:.3e} > 64 x LAPACK's {lapack[0]:.3e}")
    if not fwd <= max(CAP * lapack[1], FWD_FLOOR):
        bad.append(f"{label}: forward error {fwd:.3e} > 64 x max(LAPACK's {lapack[1]:.3e}, 2.2e-16)")


def _host_analysis(mod, m):
    bi, bj = cc.block_pattern(m["ccs"][0], m["ccs"][1], m["bd"])
    ns, nr, lv = mod.symbolic_supernodes(m["nb"], m["bd"], bi, bj)
    return dict(n=m["n"], supernodes=len(ns), levels=int(lv.max()) + 1, max_front=int((ns + nr).max()))


def _run_case(mod, name, bad, tag=""):
    """Every right-hand side of a case under the current schedule; returns (solutions, factor info)."""
    m, ref = cc.matrix(name), cc.reference(name)
    xs, info = [], None
    for k, rn in enumerate(cc.RHS_NAMES):
        b = ref["B"][:, k]
        ok, x, info = _solve(mod, m["A"], m["bd"], b, ccs=m["ccs"], info=True)
        assert ok, f"{name} {rn}: reported not positive definite"
        _judge(f"{tag}{name} {rn}", m["A"], m["norm2"], b, x, ref["X"][:, k], ref["lapack"][k], bad)
        xs.append(x)
    print(f"CHOLINFO {tag}{name} {info}")
    return xs, info


# ------------------------------------------------------------------------------------------------ a. shapes
@pytest.mark.parametrize("name", list(cc.SHAPE_CASES))
def test_shape_sweep(g2o_amd_mod, name):
    """Well-conditioned (mu = 1e-2) systems at the front-size edges, default schedule: n = 1, one block, dense fronts
    one below, on and one above multiples of the 32-column panel and the 64-row tile, block sizes 1, 2, 3, 5, 6, 7,
    chains, arrows, fans (fronts with rows below them at those edges), disconnected components with isolated blocks,
    random graphs. The factorization the call reports is the one the host analysis predicts."""
    bad = []
    _, info = _run_case(g2o_amd_mod, name, bad)
    host = _host_analysis(g2o_amd_mod, cc.matrix(name))
    assert {k: int(info[k]) for k in host} == host
    assert info["nnzL"] > 0 and info["flops"] > 0
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ b. conditioning
# The one miss, measured on an MI355X: chain(65, bd 1) at mu = 1e-10 (cond_2 = 5.8e10), b = A x0 with integer x0.
# GPU eta 1.3e-16 (LAPACK 1.7e-17, 7.2 x), GPU forward error 3.2e-7 against LAPACK's 4.9e-9: 64.8 x, cap 64.
# The cause is the elimination order, not a term of the solver. The chain is tridiagonal in its natural order, where
# LAPACK does one multiply-subtract per pivot and this right-hand side happens to come out 60 x below its own error
# for the other right-hand sides of the same matrix (2.9e-7). The same LAPACK routine on the same system gives
# 8.5e-8 in the device's nested-dissection order and a median of 9.6e-8, at most 3.3e-7, over 20 random symmetric
# permutations; a plain fp64 Cholesky in the device's order with correctly rounded pivots and triangular solves
# (neither the rsq step nor the explicit inverses) gives 2.7e-7. The device's 3.2e-7 is inside that spread.
ORDER_BOUND = {("cond-chain65-bd1-mu1e-10", "A@int")}
COND_PARAMS = [pytest.param(name, rn, marks=[pytest.mark.xfail(
    strict=True, reason="forward error 3.2e-7 = 64.8 x LAPACK's 4.9e-9 in the natural tridiagonal order; LAPACK in "
    "the device's elimination order: 8.5e-8 (see the comment above ORDER_BOUND)")] if (name, rn) in ORDER_BOUND else [])
    for name in cc.COND_CASES for rn in cc.RHS_NAMES]


@pytest.mark.parametrize("name,rhs", COND_PARAMS)
def test_conditioning_sweep(g2o_amd_mod, name, rhs):
    """cond_2(A) ~ 6e2, 6e5, 6e8, 6e10 (mu = 1e-2 ... 1e-10, LM systems at small lambda) on two arrows and a chain:
    the pivot reciprocal and the explicit inverses of the diagonal blocks must not cost more than the documented
    64 x LAPACK, in backward and in forward error (DESIGN.md records the figures)."""
    m, ref = cc.matrix(name), cc.reference(name)
    k = cc.RHS_NAMES.index(rhs)
    b = ref["B"][:, k]
    ok, x = _solve(g2o_amd_mod, m["A"], m["bd"], b, ccs=m["ccs"])
    assert ok
    bad = []
    _judge(f"{name} {rhs}", m["A"], m["norm2"], b, x, ref["X"][:, k], ref["lapack"][k], bad)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ c. not PD
def _twin_pair(mod, A, bd, norm2, k, b, label, bad):
    """The indefinite copy of A at scalar k must be refused, its positive definite twin solved to the criteria."""
    notpd, pd = cc.twins(A, k)
    ok, _ = _solve(mod, notpd, bd, b)
    if ok:
        bad.append(f"{label} k={k}: indefinite matrix reported positive definite")
    ok, x = _solve(mod, pd, bd, b)
    if not ok:
        bad.append(f"{label} k={k}: positive definite twin reported not positive definite")
        return
    ref = cc.reference_for(pd, b[:, None], norm2)
    _judge(f"{label} k={k} pd-twin", pd, norm2, b, x, ref["X"][:, 0], ref["lapack"][0], bad)


SWEEPS = [("notpd-arrow33-bd3-sep4", p, 3) for p in range(3)] + [("notpd-arrow40-bd6-sep12", p, 2) for p in range(2)] \
    + [("notpd-fan-bd3-sep11", 0, 1)]


@pytest.mark.parametrize("name,part,parts", SWEEPS)
def test_notpd_sweep(g2o_amd_mod, name, part, parts):
    """A - t e_k e_k^T for every scalar k of the 99-column arrow (every elimination position, every lane of full and
    partial 32-column blocks), every 7th k and the ends of every separator block of the 240-column arrow, and every 4th
    k of a fan whose separator pivots fail only after its children's updates: t just past the pivot's Schur complement
    is refused (the diagonal entry stays positive: only the factorization can tell), t at half of it is solved.
    A refused factorization leaves nothing behind: the unmodified matrix is solved afterwards, in the same process."""
    m, ref = cc.matrix(name), cc.reference(name)
    b = ref["B"][:, 0]
    ks = cc.notpd_indices(name)[part::parts]
    bad = []
    for k in ks:
        _twin_pair(g2o_amd_mod, m["A"], m["bd"], m["norm2"], k, b, name, bad)
    _run_case(g2o_amd_mod, name, bad, tag="after-sweep ")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(cc.fixed_notpd()))
def test_notpd_fixed(g2o_amd_mod, name):
    """1 x 1 pivots of exactly 0.0 and below it (cs_chol's d <= 0): an isolated block's cut-off last scalar beside two
    healthy components, and n = 1."""
    A, bd = cc.fixed_notpd()[name]
    ok, _ = _solve(g2o_amd_mod, A, bd, np.ones(A.shape[0]))
    assert not ok


# ------------------------------------------------------------------------------------------------ d. schedules
FACTOR_SCHEDULES = {k: dict(SCHEDULES[k]) for k in (
    "lagged_all_levels", "blocked_separate_contrib", "band_leaves", "assembly_cb_zeroed", "scatter_up_front",
    "no_leaf_absorption", "syrk_register_staged", "syrk_128x64_blocked", "syrk_128x64_deferred_l21", "deferred_l21_all",
    "deferred_l21_off", "extend_add_512")}
FACTOR_SCHEDULES["blocked_separate_contrib"]["G2OHIP_CHOL_BLOCK_MIN"] = "32"
FACTOR_SCHEDULES["assemble_in_place"] = {"G2OHIP_CHOL_PRE_MAX": "0"}
FACTOR_SCHEDULES["prescatter_all"] = {"G2OHIP_CHOL_PRE_MAX": "1000000000000"}
# arrow(60, bd 6, sep 12): a 348-column root supernode (panels past 64 columns, big panels when blocked) over two
# 6-column leaves with 78 and 84 rows below them; the random graph: 28 fronts on 5 levels, most with children
SCHEDULE_CASES = ("sched-arrow60-bd6-sep12", "sched-random-bd6-nb60")
_default_x = {}


@pytest.mark.parametrize("mode", list(FACTOR_SCHEDULES))
def test_forced_schedules(g2o_amd_mod, monkeypatch, mode):
    """Each schedule knob that acts on the factor, on systems small enough for the reference: the criteria of the
    shape sweep, the default schedule's x within 1e-12, the schedule really taken (factor info of the very call), and
    not-PD detection under it for a leaf scalar, the first and the last separator scalar."""
    bad = []
    for name in SCHEDULE_CASES:
        if name not in _default_x:
            _default_x[name] = _run_case(g2o_amd_mod, name, bad, tag="default ")
    for k, v in FACTOR_SCHEDULES[mode].items():
        monkeypatch.setenv(k, v)
    for name in SCHEDULE_CASES:
        xs, info = _run_case(g2o_amd_mod, name, bad, tag=f"{mode} ")
        x0s, info0 = _default_x[name]

        def need(cond):
            if not cond:
                bad.append(f"{mode} {name}: schedule not taken, factor info {info} (default {info0})")

        for x, x0, rn in zip(xs, x0s, cc.RHS_NAMES):
            if x0.any() and not np.linalg.norm(x - x0) <= 1e-12 * np.linalg.norm(x0):
                bad.append(f"{mode} {name} {rn}: {np.linalg.norm(x - x0) / np.linalg.norm(x0):.3e} from the default x")
        if mode in ("blocked_separate_contrib", "syrk_128x64_blocked"):
            need(info["blocked_fronts"] > 0 and info["bwd_rounds"] > 0)
        else:
            need(info["blocked_fronts"] == 0)
        if mode in ("syrk_128x64_deferred_l21", "deferred_l21_all"):
            need(info["levels"] > 1 and info["deferred_l21_fronts"] > 0)
        if mode == "deferred_l21_off":
            need(info["deferred_l21_fronts"] == 0)
        need(info["inplace_levels"] + info["prescatter_levels"] == info["levels"])
        if mode == "prescatter_all":
            need(info["inplace_levels"] == 0)
        elif mode == "assemble_in_place" and name == "sched-random-bd6-nb60":
            # levels whose fronts are mostly input entries stay pre-scattered whatever the limit (the leaves)
            need(info["inplace_levels"] > 0 and info["prescatter_levels"] < info0["prescatter_levels"])
        if mode == "no_leaf_absorption":
            need(info["supernodes"] >= info0["supernodes"])
    m, ref = cc.matrix(SCHEDULE_CASES[0]), cc.reference(SCHEDULE_CASES[0])
    for k in cc.notpd_indices(SCHEDULE_CASES[0]):
        _twin_pair(g2o_amd_mod, m["A"], m["bd"], m["norm2"], k, ref["B"][:, 0], f"{mode} {SCHEDULE_CASES[0]}", bad)
    assert not bad, "\n".join(bad)
