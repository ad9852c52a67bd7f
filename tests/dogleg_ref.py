"""TEST INFRASTRUCTURE — Powell's dogleg as the reference runs it, in numpy over the CPU oracle.

OptimizationAlgorithmDogleg::solve (core/optimization_algorithm_dogleg.cpp:57-208) restated line for line over
oracle_py.OracleGraph: chi2(), stage(lam) for b, x and the solver's ok, hessian_dense() for Hpp, push / update / pop /
discard_top. It shares no code with the library under test (the device loop, or g2ohip_dogleg_blend).

multiplyHessian (block_solver.h:146) multiplies by Hpp only: the vectors have vectorSize() entries, poses then
landmarks, and the landmark part of the product stays zero. So alpha = |b|^2 / (b_p^T Hpp b_p) with |b|^2 over the full
vector, and linearGain = -hdl_p^T Hpp hdl_p + 2 b . hdl with the last dot over the full vector. That is the
reference's behaviour and is reproduced as it is.

Besides the trajectory every decision's margins are recorded: how far each rho is from the thresholds 0, 0.25 and 0.75,
and how far |hgn| and |hsd| are from delta (relative). A comparison against this loop is meaningful only where those
margins are well above rounding (tests/test_dogleg_host.py asserts them for the inputs of TABLE).
"""
from __future__ import annotations

import dataclasses
import math
from typing import List

import numpy as np

from g2o_amd import synth

STEP_UNDEFINED, STEP_SD, STEP_GN, STEP_DL = 0, 1, 2, 3  # the reference's enum order
OK, TERMINATE, FAIL = 0, 1, 2


@dataclasses.dataclass
class Iteration:
    chi2_before: float
    chi2: float                 # after the iteration (activeRobustChi2 of the state it leaves)
    tries: int                  # _lastNumTries
    delta: float                # _delta after the iteration
    trials: list                # (step, rho) per trial
    lam: float                  # _currentLambda after the iteration
    was_pd: bool                # _wasPDInAllIterations
    result: int                 # OK / TERMINATE / FAIL
    lambdas_tried: list         # damping values the not-PD loop solved with (0: undamped)
    rho_margin: float           # min over trials of the distance of rho to 0, 0.25, 0.75
    norm_margin: float          # min over trials of | |hgn| - delta | / delta and | |hsd| - delta | / delta
    hpp_min_eig: float          # smallest eigenvalue of the solved system's matrix, undamped (see _system_min_eig)

    @property
    def last_step(self):
        return self.trials[-1][0] if self.trials else STEP_UNDEFINED


class Dogleg:
    """One OptimizationAlgorithmDogleg bound to an OracleGraph; solve(iteration) is one solve() call."""

    def __init__(self, graph, initial_delta=1e4, max_trials=100, initial_lambda=1e-7, lambda_factor=10.0, cfg=None):
        self.g = graph
        self.user_delta, self.max_trials = float(initial_delta), int(max_trials)
        self.initial_lambda, self.lambda_factor = float(initial_lambda), float(lambda_factor)
        self.delta, self.lam, self.was_pd = self.user_delta, self.initial_lambda, True
        self.cfg = cfg

    def _system_min_eig(self, st, Hpp, with_eig):
        """Smallest eigenvalue of the matrix the linear solver factors, without damping. Only where the not-PD branch
        matters (with_eig) and only on a graph without landmarks, where that matrix is Hpp."""
        if not with_eig or st["nl"]:
            return math.nan
        return float(np.linalg.eigvalsh(Hpp).min())

    def solve(self, iteration: int, with_eig: bool = False) -> Iteration:
        g = self.g
        if iteration == 0:  # :64-79
            self.delta, self.lam, self.was_pd = self.user_delta, self.initial_lambda, True
        chi = g.chi2()                                  # :82, :89
        st = g.stage(0.0, self.cfg)                     # :91 buildSystem (+ the undamped solve, used below)
        npose, nl = st["np"], st["nl"]
        b = st["b"]
        Hpp = _hpp(g, st)
        # :98-105
        aux = Hpp @ b[:npose]
        b_sq = float(b @ b)
        alpha = b_sq / float(aux @ b[:npose])
        hsd = alpha * b
        hsd_norm = float(np.linalg.norm(hsd))
        tried = []
        # :115-148, the Gauss-Newton solve of the first trial
        ok = False
        x = None
        while not ok:
            lam = 0.0 if self.was_pd else self.lam      # :125-126
            s = st if lam == 0.0 else g.stage(lam, self.cfg)
            tried.append(lam)
            ok = bool(s["ok"])                          # :127
            x = s["x"]
            self.was_pd = self.was_pd and ok            # :130
            if not self.was_pd:                         # :131-142
                if ok:
                    self.lam = max(1e-12, self.lam / (0.5 * self.lambda_factor))
                else:
                    self.lam *= self.lambda_factor
                    if self.lam > 1e3:
                        self.lam = 1e3
                        return Iteration(chi, chi, 1, self.delta, [], self.lam, self.was_pd, FAIL, tried, math.inf,
                                         math.inf, self._system_min_eig(st, Hpp, with_eig))
        hgn = x
        hgn_norm = float(np.linalg.norm(hgn))           # :147
        trials, rho_m, norm_m = [], math.inf, math.inf
        tries, good, new_chi = 0, False, chi
        while True:                                     # :112-204
            tries += 1
            d = self.delta
            norm_m = min(norm_m, abs(hgn_norm - d) / d)
            if hgn_norm < d:                            # :153-155
                hdl, step = hgn, STEP_GN
            else:
                norm_m = min(norm_m, abs(hsd_norm - d) / d)
                if hsd_norm > d:                        # :157-159
                    hdl, step = d / hsd_norm * hsd, STEP_SD
                else:                                   # :161-173
                    bma = hgn - hsd
                    c = float(hsd @ bma)
                    bma_sq = float(bma @ bma)
                    hsd_sq = float(hsd @ hsd)
                    if c <= 0.0:
                        beta = (-c + math.sqrt(c * c + bma_sq * (d * d - hsd_sq))) / bma_sq
                    else:
                        beta = (d * d - hsd_sq) / (c + math.sqrt(c * c + bma_sq * (d * d - hsd_sq)))
                    assert 0.0 < beta < 1.0, beta
                    hdl, step = hsd + beta * bma, STEP_DL
            # :178-180
            aux = Hpp @ hdl[:npose]
            gain = -1.0 * float(aux @ hdl[:npose]) + 2.0 * float(b @ hdl)
            g.push()                                    # :183-186
            g.update(hdl)
            t_chi = g.chi2()
            if abs(gain) < 1e-12:                       # :188-189
                gain = 1e-12
            rho = (chi - t_chi) / gain
            if rho > 0:                                 # :192-197
                g.discard_top()
                good, new_chi = True, t_chi
            else:
                g.pop()
            if rho > 0.75:                              # :199-203
                self.delta = max(self.delta, 3.0 * float(np.linalg.norm(hdl)))
            elif rho < 0.25:
                self.delta *= 0.5
            trials.append((step, rho))
            rho_m = min(rho_m, abs(rho), abs(rho - 0.25), abs(rho - 0.75))
            if good or tries >= self.max_trials:        # :204
                break
        result = TERMINATE if (tries == self.max_trials or not good) else OK
        return Iteration(chi, new_chi, tries, self.delta, trials, self.lam, self.was_pd, result, tried, rho_m, norm_m,
                         self._system_min_eig(st, Hpp, with_eig))


def _hpp(g, st):
    """Hpp of the last buildSystem, dense and symmetric (the oracle may return its upper triangle only). Hll and Hpl
    are not needed: hessian_dense gets no buffers for them."""
    npose = st["np"]
    Hpp = g.hessian_dense(npose, 0)[0]
    lower = np.tril(Hpp, -1)
    if not lower.any():
        Hpp = Hpp + np.triu(Hpp, 1).T
    return Hpp


def optimize(graph, iterations: int, with_eig: bool = False, **params):
    """SparseOptimizer::optimize's loop (sparse_optimizer.cpp:374-439) over Dogleg.solve: (return value, [Iteration]).
    A Fail returns 0, a Terminate ends the loop after its iteration."""
    alg = Dogleg(graph, **params)
    out: List[Iteration] = []
    cj = 0
    for i in range(iterations):
        it = alg.solve(i, with_eig)
        out.append(it)
        cj += 1
        if it.result != OK:
            break
    if out and out[-1].result == FAIL:
        return 0, out
    return cj, out


# ---------------------------------------------------------------- the compared inputs
def indefinite_c1(factor: float):
    """C1 (small) with the information matrix of edge 5 multiplied by `factor` (< 0): an indefinite H."""
    prob = synth.by_name("C1", "small")
    e = prob.edges[0]
    info = e.info.copy()
    info[5] *= factor
    return synth.Problem(f"{prob.name}_info5x{factor:g}", prob.vertices,
                         [synth.EdgeSet(e.etype, e.v0, e.v1, e.meas, info, e.params)], prob.pose_dim,
                         prob.landmark_dim)


@dataclasses.dataclass
class Case:
    key: str
    make: object          # () -> synth.Problem
    initial_delta: float
    iterations: int
    fixed_algo: str       # the dl_hip_fix* name matching the graph
    pd: bool = True       # H stays positive definite


TABLE = [
    Case("C1_d0.05", lambda: synth.by_name("C1", "small"), 0.05, 8, "dl_hip_fix6_6"),
    Case("C2_d1", lambda: synth.by_name("C2", "small"), 1.0, 6, "dl_hip_fix3_3"),
    Case("S2_default", lambda: synth.by_name("S2", "small"), 1e4, 8, "dl_hip_fix3_2"),
    Case("S2_d1", lambda: synth.by_name("S2", "small"), 1.0, 8, "dl_hip_fix3_2"),
    Case("C4_d0.05", lambda: synth.by_name("C4", "small"), 0.05, 5, "dl_hip_fix6_3"),
    Case("C1_indef-0.2", lambda: indefinite_c1(-0.2), 1e4, 3, "dl_hip_fix6_6", pd=False),
    Case("C1_indef-0.5", lambda: indefinite_c1(-0.5), 1e4, 1, "dl_hip_fix6_6", pd=False),
]
CASES = {c.key: c for c in TABLE}

_ref_cache: dict = {}


def reference(key: str, oracle_py):
    """(return value, [Iteration], final minimal_state) of the reference loop on a TABLE input; computed once."""
    if key not in _ref_cache:
        c = CASES[key]
        g = oracle_py.OracleGraph(c.make())
        n, its = optimize(g, c.iterations, with_eig=not c.pd, initial_delta=c.initial_delta)
        _ref_cache[key] = (n, its, g.minimal_state())
    return _ref_cache[key]
