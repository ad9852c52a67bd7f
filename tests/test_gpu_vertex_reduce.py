"""The vertex reduction (k_vertex_reduce<DIM, 1 | 4 | 8>, k_vertex_reduce_wide<DIM>, k_vertex_reduce<DIM, 64>) at every
block dimension and lane class, with degrees that are ragged against the lane count.

The engine picks the lane count from the average degree of the reduced vertex set: 64 from 128, 8 from 16, 4 from 6,
else 1. Each graph here puts that average well inside one class (the test computes it and asserts the margin) and then
holds a vertex of degree 1, one of LANES - 1, one of LANES + 1 and a hub of three times the base degree; the wide class
also one of degree 7 (fewer slots than its 8 streams) and one of 65 (one past its 64-slot stride).

  DIM 6: VertexSE3 under EdgeSE3, DIM 3: VertexSE2 under EdgeSE2 (circulant graphs, pose_edges_ref.ragged_pose_graph)
  DIM 2: XY landmarks under EdgeSE2PointXY, the number of observing poses chosen per landmark (ragged_landmark_graph)

Checked: stage(1e-3) against the numpy dense system of tests/pose_edges_ref.py (1e-9 on b, bschur and x, 1e-11 on
Hschur), two runs bit for bit, and the wide class again with G2OHIP_VR_WIDE=0 (k_vertex_reduce<DIM, 64>) in a child
process, because the library reads that variable once per process.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAM = 1e-3
# lane class -> (vertices, circulant half-width k: base degree 2k, the average degree the class must hold)
POSE_SHAPES = {1: (24, 1, (0, 4)), 4: (40, 5, (8, 12)), 8: (48, 16, (24, 64)), 64: (176, 84, (160, 1e9))}
# lane class -> (landmark degrees, poses)
LM_SHAPES = {1: ([1, 2, 3, 3, 2, 3, 9, 3, 3], 12),
             4: ([1, 3, 5, 10, 10, 9, 10, 30, 11, 10], 24),
             8: ([1, 7, 9, 32, 33, 31, 32, 96, 32, 30], 40),
             64: ([1, 7, 63, 65, 700, 170, 171, 169, 170, 172, 168, 170, 171], 90)}
CLASS_RANGE = {1: (0, 4), 4: (8, 12), 8: (24, 64), 64: (160, 1e9)}


def _lanes_of(avg):
    return 64 if avg >= 128 else (8 if avg >= 16 else (4 if avg >= 6 else 1))


def _problem(dim, lanes):
    import pose_edges_ref as R
    from g2o_amd import synth
    if dim == 2:
        degrees, npose = LM_SHAPES[lanes]
        prob = R.ragged_landmark_graph(degrees, npose, seed=lanes)
        deg = np.asarray(degrees)
    else:
        nv, k, _ = POSE_SHAPES[lanes]
        prob, deg = R.ragged_pose_graph(synth.V_SE3_QUAT if dim == 6 else synth.V_SE2, nv, k, lanes, wide=lanes == 64,
                                        seed=10 * dim + lanes)
    avg = deg.sum() / len(deg)
    lo, hi = CLASS_RANGE[lanes]
    assert lo <= avg <= hi and _lanes_of(avg) == lanes, (dim, lanes, avg)
    want = {1, lanes + 1} | ({lanes - 1} if lanes > 1 else set()) | ({7, 65} if lanes == 64 else set())
    assert want <= set(deg.tolist()) and deg.max() >= 2.5 * avg, (dim, lanes, sorted(set(deg.tolist())))
    return prob


def _check(dim, lanes):
    import g2o_amd
    import pose_edges_ref as R
    prob = _problem(dim, lanes)
    r = R.numpy_stage(prob, LAM)
    runs = [g2o_amd.SparseOptimizer(0).add_problem(prob).stage(LAM) for _ in range(2)]
    s = runs[0]
    assert s["ok"] == 1 and (s["n"], s["np"]) == (r["n"], r["np"])
    for k in ("b", "x") + (("bschur",) if dim == 2 else ()):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"dim {dim} lanes {lanes} {k}: {err:.2e}")
        assert err <= 1e-9, (dim, lanes, k, err)
    err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
    print(f"dim {dim} lanes {lanes} Hschur: {err:.2e}")
    assert err <= 1e-11, (dim, lanes, err)
    for k in ("b", "x", "Hschur", "bschur"):
        assert np.array_equal(runs[0][k], runs[1][k]), (dim, lanes, k)
    return s


@pytest.mark.parametrize("lanes", [1, 4, 8, 64])
@pytest.mark.parametrize("dim", [2, 3, 6])
def test_ragged_degrees(g2o_amd_mod, dim, lanes):
    _check(dim, lanes)


@pytest.mark.parametrize("dim", [2, 3, 6])
def test_wide_class_without_the_wide_kernel(g2o_amd_mod, monkeypatch, tmp_path, dim):
    """G2OHIP_VR_WIDE=0: the same graph through k_vertex_reduce<DIM, 64>; same checks, and b equal to the wide kernel's
    to rounding (the two sum in different orders)."""
    monkeypatch.setenv("G2OHIP_VR_WIDE", "0")
    out = tmp_path / "b.npy"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(dim), str(out)], capture_output=True, text=True,
                       timeout=120)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "child ok" in p.stdout
    monkeypatch.delenv("G2OHIP_VR_WIDE")
    b = _check(dim, 64)["b"]
    bc = np.load(out)
    assert np.linalg.norm(b - bc) <= 1e-12 * np.linalg.norm(b)


if __name__ == "__main__":  # the child of test_wide_class_without_the_wide_kernel
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    assert os.environ.get("G2OHIP_VR_WIDE") == "0"
    np.save(sys.argv[2], _check(int(sys.argv[1]), 64)["b"])
    print("child ok")
