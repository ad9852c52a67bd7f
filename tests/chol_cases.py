"""Matrices, shapes and the extended-precision reference for the direct tests of the sparse Cholesky solver
(test_chol_cases.py checks the cases themselves on the CPU, test_gpu_cholesky_edges.py runs them on the device).

Reference: a column Cholesky and two triangular solves in np.longdouble (64-bit mantissa on x86, unit roundoff
5.4e-20 against fp64's 1.1e-16), each step vectorised over its column.

Matrix family: block graph Laplacians. Each edge (i, j) of a graph over nb blocks of size bd adds [[W, -W], [-W, W]]
with W = G G^T, G a bd x (bd + 2) standard normal; a block without any edge gets one W on its diagonal (else it would
be zero). The graph part of a connected component is singular, so after adding mu * trace(A) / n * I the condition
number is about 1 / mu, like a Levenberg-Marquardt system at that damping. (A A^T + n I, or a diagonally dominant
matrix scaled symmetrically, would not do: Cholesky is invariant under symmetric scaling, and those stay at a scaled
condition number of about 2.)
"""
import functools
import zlib

import numpy as np

LD = np.longdouble
EPS = 2.2e-16  # fp64 machine epsilon, as the tolerances of the GPU tests count it


# ------------------------------------------------------------------------------------------------ reference
def chol_ld(A):
    """Lower Cholesky factor of A in longdouble (left-looking, one column per step); None when a pivot is not
    positive (CSparse's `d <= 0` test)."""
    A = np.asarray(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0:
            return None
        L[j:, j] = c / np.sqrt(c[0])
    return L


def solve_factored_ld(L, B):
    """L L^T X = B in longdouble; B a vector or an n x k matrix."""
    X = np.array(B, LD)
    n = L.shape[0]
    for j in range(n):  # forward, column oriented
        X[j] = X[j] / L[j, j]
        if j + 1 < n:
            X[j + 1:] -= np.multiply.outer(L[j + 1:, j], X[j]) if X.ndim == 2 else L[j + 1:, j] * X[j]
    for j in range(n - 1, -1, -1):  # backward with L^T, column oriented
        X[j] = X[j] / L[j, j]
        if j:
            X[:j] -= np.multiply.outer(L[j, :j], X[j]) if X.ndim == 2 else L[j, :j] * X[j]
    return X


def solve_ld(A, b):
    L = chol_ld(A)
    return None if L is None else solve_factored_ld(L, b)


def errors(A, b, x, x_ref, norm2):
    """(normwise backward error ||b - A x|| / (||A||_2 ||x|| + ||b||) with the residual formed in longdouble,
    relative forward error against x_ref)."""
    xl, bl = np.asarray(x, LD), np.asarray(b, LD)
    r = bl - np.asarray(A, LD) @ xl
    den = LD(norm2) * np.linalg.norm(xl) + np.linalg.norm(bl)
    eta = float(np.linalg.norm(r) / den) if den > 0 else 0.0
    fwd = float(np.linalg.norm(xl - x_ref) / np.linalg.norm(x_ref))
    return eta, fwd


# ------------------------------------------------------------------------------------------------ structures
def chain(nb):
    return [(i, i + 1) for i in range(nb - 1)]


def arrow(nb, sep):
    """A chain on the first nb - sep blocks; each of the last sep blocks joined to every block before it: a dense root
    separator that every leaf has rows in."""
    return chain(nb - sep) + [(i, j) for j in range(nb - sep, nb) for i in range(j)]


def dense(nb):
    return [(i, j) for j in range(nb) for i in range(j)]


def random_graph(nb, density, rng):
    return [(i, j) for j in range(nb) for i in range(j) if rng.random() < density]


def fan(sep, leaves):
    """Cliques of the given widths (blocks), each joined to every block of a separator clique of sep blocks behind
    them. A leaf clique wider than an eighth of the separator is neither absorbed into the root supernode nor (but for
    the last one, when it fits) amalgamated with it, so each is a front of its own with sep block rows below it."""
    edges, base = [], 0
    for w in leaves:
        edges += [(base + i, base + j) for i, j in dense(w)]
        base += w
    return base + sep, edges + [(i, j) for j in range(base, base + sep) for i in range(j)]


def components(arrows, isolated):
    """Disjoint arrows [(nb, sep), ...] followed by `isolated` blocks without any edge."""
    edges, base = [], 0
    for nb, sep in arrows:
        edges += [(base + i, base + j) for i, j in arrow(nb, sep)]
        base += nb
    return base + isolated, edges


def graph_matrix(nb, bd, edges, mu, rng):
    n = nb * bd
    A = np.zeros((n, n))
    touched = np.zeros(nb, bool)
    for i, j in edges:
        G = rng.standard_normal((bd, bd + 2))
        W = G @ G.T
        si, sj = slice(i * bd, (i + 1) * bd), slice(j * bd, (j + 1) * bd)
        A[si, si] += W
        A[sj, sj] += W
        A[si, sj] -= W
        A[sj, si] -= W
        touched[i] = touched[j] = True
    for i in np.nonzero(~touched)[0]:
        G = rng.standard_normal((bd, bd + 2))
        A[i * bd:(i + 1) * bd, i * bd:(i + 1) * bd] += G @ G.T
    return A + mu * np.trace(A) / n * np.eye(n)


# ------------------------------------------------------------------------------------------------ packing
def upper_ccs(A):
    """Upper CCS (Ap, Ai, Ax) of the nonzero entries of the upper triangle of A; the diagonal is always stored."""
    n = A.shape[0]
    Ap, Ai, Ax = [0], [], []
    for j in range(n):
        rows = np.nonzero(A[: j + 1, j])[0]
        if not len(rows) or rows[-1] != j:
            rows = np.append(rows, j)
        Ai += rows.tolist()
        Ax += A[rows, j].tolist()
        Ap.append(len(Ai))
    return Ap, Ai, Ax


def block_pattern(Ap, Ai, bd):
    """Upper block pattern (bi, bj) of a scalar upper CCS in the order g2ohip_linear_solve_ccs lists it (first
    appearance by scalar column, then the diagonal blocks not seen): the input of the same symbolic analysis."""
    n = len(Ap) - 1
    seen, bi, bj = set(), [], []
    for j in range(n):
        for p in range(Ap[j], Ap[j + 1]):
            key = (Ai[p] // bd, j // bd)
            if Ai[p] <= j and key not in seen:
                seen.add(key)
                bi.append(key[0])
                bj.append(key[1])
    for k in range(n // bd):
        if (k, k) not in seen:
            bi.append(k)
            bj.append(k)
    return bi, bj


# ------------------------------------------------------------------------------------------------ indefinite twins
def twins(A, k):
    """(indefinite, positive definite) copies of a positive definite A that differ from it in entry (k, k) alone.
    With s = 1 / (A^-1)_kk, A - t e_k e_k^T is positive definite exactly when t < s. The indefinite copy takes
    t = (s + A_kk) / 2: its diagonal entry (A_kk - s) / 2 stays positive, only a factorization finds it. The positive
    definite twin takes t = s / 2."""
    s = 1.0 / np.linalg.inv(A)[k, k]
    bad, good = A.copy(), A.copy()
    bad[k, k] -= 0.5 * (s + A[k, k])
    good[k, k] -= 0.5 * s
    return bad, good


# ------------------------------------------------------------------------------------------------ the cases
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _case(bd, nb, edges, mu=1e-2):
    return dict(bd=bd, nb=nb, edges=edges, mu=mu)


FANS = ((1, 32, (31, 32, 33, 16)), (1, 33, (30, 31, 32)), (1, 64, (63, 64, 65, 31, 33)), (3, 11, (10, 11, 21)),
        (6, 5, (5, 6, 11)))


def _shape_cases():
    c = {"single-bd1": _case(1, 1, []), "single-bd7": _case(7, 1, [])}
    for n in (31, 32, 33, 63, 64, 65, 96, 97, 129, 257):
        c[f"dense-bd1-n{n}"] = _case(1, n, dense(n))
    for nb in (10, 11, 21, 22):
        c[f"dense-bd3-nb{nb}"] = _case(3, nb, dense(nb))
    for nb in (9, 10):
        c[f"dense-bd7-nb{nb}"] = _case(7, nb, dense(nb))
    for bd in (1, 2, 5, 6, 7):
        c[f"chain-bd{bd}-nb65"] = _case(bd, 65, chain(65))
    for sep in (31, 32, 33, 63, 64, 65):
        c[f"arrow-bd1-sep{sep}"] = _case(1, 40 + sep, arrow(40 + sep, sep))
    for sep in (10, 11, 21, 22):
        c[f"arrow-bd3-sep{sep}"] = _case(3, 50 + sep, arrow(50 + sep, sep))
    for sep in (5, 6, 11, 12):
        c[f"arrow-bd6-sep{sep}"] = _case(6, 50 + sep, arrow(50 + sep, sep))
    nb, edges = components([(20, 3), (45, 5)], 3)
    c["components-bd3"] = _case(3, nb, edges)
    # not in the issue's list: fronts with rows below them at the 32-column and 64-row boundaries (the arrows' leaves
    # are amalgamated into their root supernodes by the ordering, see test_chol_cases.py::test_shape_coverage)
    for bd, sep, leaves in FANS:
        nb, edges = fan(sep, leaves)
        c[f"fan-bd{bd}-sep{sep}"] = _case(bd, nb, edges)
    for bd in (3, 6):
        c[f"random-bd{bd}-nb120"] = _case(bd, 120, random_graph(120, 0.05, _rng(f"random-graph-{bd}")))
    return c


MUS = (1e-2, 1e-5, 1e-8, 1e-10)


def _cond_cases():
    c = {}
    for mu in MUS:
        c[f"cond-arrow65-bd6-sep6-mu{mu:g}"] = _case(6, 65, arrow(65, 6), mu)
        c[f"cond-arrow33-bd3-sep4-mu{mu:g}"] = _case(3, 33, arrow(33, 4), mu)
        c[f"cond-chain65-bd1-mu{mu:g}"] = _case(1, 65, chain(65), mu)
    return c


SHAPE_CASES = _shape_cases()   # (a) well-conditioned shape sweep
COND_CASES = _cond_cases()     # (b) conditioning sweep
OTHER_CASES = {                # (c) not-PD sweeps, (d) forced schedules
    "notpd-arrow33-bd3-sep4": _case(3, 33, arrow(33, 4)),
    "notpd-arrow40-bd6-sep12": _case(6, 40, arrow(40, 12)),
    "notpd-fan-bd3-sep11": _case(3, *fan(11, (10, 11, 21))),  # three fronts: pivots that fail after a child's update
    "sched-arrow60-bd6-sep12": _case(6, 60, arrow(60, 12)),
    "sched-random-bd6-nb60": _case(6, 60, random_graph(60, 0.08, _rng("random-graph-sched"))),
}
CASES = {**SHAPE_CASES, **COND_CASES, **OTHER_CASES}


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The case's matrix, read only: dict(A, n, bd, nb, ccs=(Ap, Ai, Ax), norm2)."""
    c = CASES[name]
    A = graph_matrix(c["nb"], c["bd"], c["edges"], c["mu"], _rng(name))
    A.setflags(write=False)
    return dict(A=A, n=A.shape[0], bd=c["bd"], nb=c["nb"], ccs=upper_ccs(A), norm2=float(np.linalg.norm(A, 2)))


def rhs(A, seed):
    """Right-hand sides as columns: random, A x0 with small-integer x0, zero, e_first, e_last."""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    B = np.zeros((n, 5))
    B[:, 0] = rng.standard_normal(n)
    B[:, 1] = A @ rng.integers(-4, 5, n).astype(float)
    B[0, 3] = 1.0
    B[n - 1, 4] = 1.0
    return B


RHS_NAMES = ("random", "A@int", "zero", "e_first", "e_last")


def reference_for(A, B, norm2):
    """dict(B, X: longdouble solutions, lapack: [(eta, fwd) per column] of scipy's fp64 cho_factor / cho_solve against
    them); X is None when the longdouble factorization fails."""
    import scipy.linalg as sla
    L = chol_ld(A)
    if L is None:
        return dict(B=B, X=None, lapack=None)
    X = solve_factored_ld(L, B)
    Xl = sla.cho_solve(sla.cho_factor(A, lower=True), B)
    lap = [errors(A, B[:, k], Xl[:, k], X[:, k], norm2) if np.any(B[:, k]) else (0.0, 0.0) for k in range(B.shape[1])]
    return dict(B=B, X=X, Xlapack=Xl, lapack=lap)


@functools.lru_cache(maxsize=None)
def reference(name):
    m = matrix(name)
    return reference_for(m["A"], rhs(m["A"], zlib.crc32(name.encode()) + 1), m["norm2"])


def notpd_indices(name):
    """Scalar indices k of the twin sweeps."""
    if name == "notpd-arrow33-bd3-sep4":
        return list(range(99))
    if name == "notpd-arrow40-bd6-sep12":
        sep = [b * 6 + e for b in range(28, 40) for e in (0, 5)]
        return sorted(set(list(range(0, 240, 7)) + sep))
    if name == "sched-arrow60-bd6-sep12":  # a leaf, the first and the last separator scalar
        return [0, 48 * 6, 60 * 6 - 1]
    if name == "notpd-fan-bd3-sep11":
        return list(range(0, 159, 4)) + [158]
    raise KeyError(name)


def fixed_notpd():
    """name -> (A, block size): matrices whose failing pivot is a 1 x 1 pivot of known value. The last scalar of the
    last isolated block of components-bd3 is cut off from its block (row and column zeroed), so its pivot is the
    diagonal entry itself in any elimination order: exactly 0.0, or negative."""
    base = matrix("components-bd3")["A"].copy()
    k = base.shape[0] - 1
    base[k, :] = 0.0
    base[:, k] = 0.0
    neg = base.copy()
    neg[k, k] = -0.5 * float(np.mean(np.diag(base)))
    return {"isolated-pivot-zero": (base, 3), "isolated-pivot-negative": (neg, 3),
            "n1-zero": (np.array([[0.0]]), 1), "n1-negative": (np.array([[-1.0]]), 1)}
