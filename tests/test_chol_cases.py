"""CPU checks of the inputs of test_gpu_cholesky_edges.py, so that the GPU tests cannot pass on vacuous cases: the
positive definite ones really are (and well enough conditioned for the longdouble reference to be a reference), the
indefinite ones really are (by a margin, by the longdouble factorization and by CSparse's verdict), and the shapes
reach the supernode widths and front sizes they are listed for in the symbolic analysis the device solver runs."""
import numpy as np
import pytest

import chol_cases as cc

EPS = cc.EPS
TWIN_SWEEPS = ("notpd-arrow33-bd3-sep4", "notpd-arrow40-bd6-sep12", "notpd-fan-bd3-sep11", "sched-arrow60-bd6-sep12")


def _csparse(oracle, n, ccs, b):
    """(ok, x) of the oracle's restatement of cs_cholsol (cs_amd order, `d <= 0` is not positive definite); where the
    reference's own CSparse is built, its verdict must be the same."""
    ok, x = oracle.ccs_cholsol(n, *ccs, b, 1)
    if oracle.ref_available():
        assert oracle.ccs_cholsol(n, *ccs, b, 2)[0] == ok
    return ok, x


def test_reference_factorization():
    """chol_ld / solve_factored_ld against exact arithmetic: a matrix with a known integer factor, and residuals at the
    longdouble roundoff level (three digits below fp64's) on a conditioning-sweep matrix."""
    assert np.finfo(cc.LD).eps < 2e-19  # 64-bit mantissa: the reference is worth its name
    rng = np.random.default_rng(0)
    L0 = np.tril(rng.integers(-3, 4, (40, 40))).astype(float)
    np.fill_diagonal(L0, rng.integers(1, 5, 40))
    A = L0 @ L0.T  # exact in fp64
    L = cc.chol_ld(A)
    assert np.array_equal(L.astype(float), L0)
    x0 = rng.integers(-9, 10, (40, 3)).astype(float)
    assert np.array_equal(cc.solve_factored_ld(L, A @ x0).astype(float), x0)
    assert np.array_equal(cc.solve_ld(A, A @ x0[:, 0]).astype(float), x0[:, 0])
    m, ref = cc.matrix("cond-arrow33-bd3-sep4-mu1e-08"), cc.reference("cond-arrow33-bd3-sep4-mu1e-08")
    for k in (0, 1, 3, 4):
        eta, _ = cc.errors(m["A"], ref["B"][:, k], ref["X"][:, k], ref["X"][:, k], m["norm2"])
        assert eta <= 1e-19
    assert cc.chol_ld(np.array([[1.0, 2.0], [2.0, 1.0]])) is None
    assert cc.chol_ld(np.array([[0.0]])) is None


def test_upper_ccs_and_block_pattern():
    A = np.array([[4.0, 0, 1, 0], [0, 0.0, 0, 0], [1, 0, 3, 2], [0, 0, 2, 5]])
    Ap, Ai, Ax = cc.upper_ccs(A)
    assert (Ap, Ai, Ax) == ([0, 1, 2, 4, 6], [0, 1, 0, 2, 2, 3], [4.0, 0.0, 1.0, 3.0, 2.0, 5.0])
    assert cc.block_pattern(Ap, Ai, 2) == ([0, 0, 1], [0, 1, 1])
    assert cc.block_pattern(Ap, Ai, 1) == ([0, 1, 0, 2, 2, 3], [0, 1, 2, 2, 3, 3])


@pytest.mark.parametrize("name", list(cc.CASES))
def test_pd_case(oracle, name):
    """A positive definite case: the longdouble factorization succeeds, LAPACK's fp64 Cholesky and CSparse
    agree with its solution within cond_2(A) * 2.2e-16, and cond_2(A) <= 1e12 (the reference keeps at least three more
    digits than fp64)."""
    m, ref = cc.matrix(name), cc.reference(name)
    A, B, X = m["A"], ref["B"], ref["X"]
    assert X is not None
    ev = np.linalg.eigvalsh(A)
    cond = ev[-1] / ev[0]
    assert ev[0] > 0 and cond <= 1e12
    if name in cc.COND_CASES:  # cond_2 ~ 1 / mu: the sweep reaches the conditioning it is listed for
        mu = cc.CASES[name]["mu"]
        assert 1.0 / mu <= cond <= 100.0 / mu
    # n = 1 (cond 1) is a square root and two divisions: three roundings of 1.1e-16 each, whatever the code; no fp64
    # solver can promise 2.2e-16 there, so the bound's factor is at least 1.5
    bound = max(cond, 1.5) * EPS
    for k in range(B.shape[1]):
        if not B[:, k].any():
            continue
        assert ref["lapack"][k][1] <= bound
        ok, x = _csparse(oracle, m["n"], m["ccs"], B[:, k])
        assert ok == 1
        assert cc.errors(A, B[:, k], x, X[:, k], m["norm2"])[1] <= bound


@pytest.mark.parametrize("name", TWIN_SWEEPS)
def test_indefinite_twins(oracle, name):
    m = cc.matrix(name)
    A, n = m["A"], m["n"]
    b = np.ones(n)
    ks = cc.notpd_indices(name)
    assert len(ks) == len(set(ks)) and 0 in ks and n - 1 in ks
    for k in ks:
        bad, good = cc.twins(A, k)
        assert bad[k, k] > 0 and A[k, k] * np.linalg.inv(A)[k, k] >= 1.5
        ev = np.linalg.eigvalsh(bad)
        assert ev[0] <= -1e-3 * ev[-1], (k, ev[0] / ev[-1])
        assert cc.chol_ld(bad) is None
        assert _csparse(oracle, n, cc.upper_ccs(bad), b)[0] == 0
        ev = np.linalg.eigvalsh(good)
        assert ev[0] >= 1e-4 * ev[-1], (k, ev[0] / ev[-1])
        assert cc.chol_ld(good) is not None
        assert _csparse(oracle, n, cc.upper_ccs(good), b)[0] == 1


def test_notpd_sweep_indices():
    assert cc.notpd_indices("notpd-arrow33-bd3-sep4") == list(range(99))
    ks = cc.notpd_indices("notpd-arrow40-bd6-sep12")
    assert set(range(0, 240, 7)) <= set(ks)
    assert all(b * 6 in ks and b * 6 + 5 in ks for b in range(28, 40))


@pytest.mark.parametrize("name", list(cc.fixed_notpd()))
def test_fixed_notpd(oracle, name):
    A, bd = cc.fixed_notpd()[name]
    n = A.shape[0]
    assert np.array_equal(A, A.T) and n % bd == 0
    assert cc.chol_ld(A) is None
    assert _csparse(oracle, n, cc.upper_ccs(A), np.ones(n))[0] == 0
    k = n - 1
    assert not A[k, :k].any()  # a 1 x 1 pivot: the diagonal entry itself, in any order
    assert (A[k, k] == 0.0) if name.endswith("zero") else (A[k, k] < 0.0)
    if n > 1:  # everything but that pivot is positive definite
        assert np.linalg.eigvalsh(A[:k, :k])[0] > 0


# ---------------------------------------------------------------------------------------------- shape coverage
# (ns, nr) of supernodes each shape must produce in the symbolic analysis the device solver runs: ns scalar columns,
# nr scalar rows below them (front size ns + nr), and its number of levels. The panel width is 32, the tile 64.
# The chains and arrows come out of the ordering in few supernodes (the chain's leaves are amalgamated into band-like
# halves, the arrows' chain leaves into their root): what they still reach is listed here, and the fans carry the
# fronts with rows below them at the boundaries.
SHAPES = {"single-bd1": ([(1, 0)], 1), "single-bd7": ([(7, 0)], 1)}
for _n in (31, 32, 33, 63, 64, 65, 96, 97, 129, 257):
    SHAPES[f"dense-bd1-n{_n}"] = ([(_n, 0)], 1)
for _nb in (10, 11, 21, 22):
    SHAPES[f"dense-bd3-nb{_nb}"] = ([(3 * _nb, 0)], 1)
for _nb in (9, 10):
    SHAPES[f"dense-bd7-nb{_nb}"] = ([(7 * _nb, 0)], 1)
for _bd in (1, 2, 5, 6, 7):  # a leaf of 32 blocks (ns a multiple of 32) with one block row below it
    SHAPES[f"chain-bd{_bd}-nb65"] = ([(32 * _bd, _bd), (33 * _bd, 0)], 2)
SHAPES.update({
    "arrow-bd1-sep31": ([(32, 0), (37, 32)], 3), "arrow-bd1-sep32": ([(63, 0), (6, 33)], 3),
    "arrow-bd1-sep33": ([(64, 0), (6, 34)], 3), "arrow-bd1-sep63": ([(64, 0), (30, 64)], 3),
    "arrow-bd1-sep64": ([(65, 0), (30, 65)], 3), "arrow-bd1-sep65": ([(66, 0), (30, 66)], 3),
    "arrow-bd3-sep10": ([(174, 0), (3, 33)], 2), "arrow-bd3-sep11": ([(177, 0), (3, 36)], 2),
    "arrow-bd3-sep21": ([(186, 0), (18, 66)], 3), "arrow-bd3-sep22": ([(189, 0), (18, 69)], 3),
    "arrow-bd6-sep5": ([(318, 0), (6, 36)], 2), "arrow-bd6-sep6": ([(324, 0), (6, 42)], 2),
    "arrow-bd6-sep11": ([(354, 0), (6, 72)], 2), "arrow-bd6-sep12": ([(360, 0), (6, 78)], 2),
    # disconnected: five childless roots on one level
    "components-bd3": ([(135, 0), (60, 0), (3, 0)], 1),
    "fan-bd1-sep32": ([(31, 32), (32, 32), (33, 32), (16, 32), (32, 0)], 2),
    "fan-bd1-sep33": ([(30, 33), (31, 33), (32, 33), (33, 0)], 2),
    "fan-bd1-sep64": ([(63, 64), (64, 64), (65, 64), (31, 64), (33, 64), (64, 0)], 2),
    "fan-bd3-sep11": ([(30, 33), (33, 33), (96, 0)], 2),
    "fan-bd6-sep5": ([(30, 30), (36, 30), (96, 0)], 2),
    # the schedule cases: a 348-column root (panels past 64) over leaves with rows below them; a deep tree
    "sched-arrow60-bd6-sep12": ([(348, 0), (6, 78)], 2),
})


def supernodes(g2o_amd_mod, name):
    m = cc.matrix(name)
    Ap, Ai, _ = m["ccs"]
    bi, bj = cc.block_pattern(Ap, Ai, m["bd"])
    ns, nr, lv = g2o_amd_mod.symbolic_supernodes(m["nb"], m["bd"], bi, bj)
    perm, st = g2o_amd_mod.symbolic_analyze(m["nb"], m["bd"], bi, bj)
    assert st["supernodes"] == len(ns) and st["levels"] == lv.max() + 1 and ns.sum() == m["n"]
    return list(zip(ns.tolist(), nr.tolist())), int(lv.max()) + 1


@pytest.mark.parametrize("name", list(cc.SHAPE_CASES) + ["sched-arrow60-bd6-sep12", "sched-random-bd6-nb60"])
def test_shape_coverage(g2o_amd_mod, name):
    sn, levels = supernodes(g2o_amd_mod, name)
    if name.startswith("random") or name.startswith("sched-random"):  # deep trees of many small fronts
        assert levels >= 4 and len(sn) >= 20 and sum(1 for s in sn if s[1] > 0) >= 20, (levels, sn)
        return
    want, want_levels = SHAPES[name]
    assert levels == want_levels, (levels, sn)
    assert all(w in sn for w in want), sn
    if name == "components-bd3":
        assert sn.count((3, 0)) == 3 and len(sn) == 5


def test_shape_sweep_reaches_sharp_boundaries(g2o_amd_mod):
    """Over the shape sweep: supernodes with rows below them (a panel step with a trailing part, not just a dense
    root) of ns % 32 in {31, 0, 1}, and fronts of (ns + nr) % 64 in {63, 0, 1}; the same for root fronts."""
    sn = [s for name in cc.SHAPE_CASES for s in supernodes(g2o_amd_mod, name)[0]]
    for below in (True, False):
        sel = [s for s in sn if (s[1] > 0) == below]
        assert {s[0] % 32 for s in sel} >= {31, 0, 1}
        assert {(s[0] + s[1]) % 64 for s in sel} >= {63, 0, 1}
    assert {s[0] for s in sn} >= {1, 7, 31, 32, 33, 63, 64, 65}  # less than one panel, partial last panels
    assert cc.SHAPE_CASES.keys() <= SHAPES.keys() | {"random-bd3-nb120", "random-bd6-nb120"}
