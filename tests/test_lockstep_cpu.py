"""CPU: the host-driven lockstep L-BFGS-B loop of the scan driver (scan._lockstep, behind refine_batched and the margin's
refinement) through the library's host-only ibs_lbfgsb2_*: points advanced side by side behave exactly as each does alone."""
import numpy as np

import ibs_amd
from ibs_amd.scan import _lockstep
from tests.test_lbfgsb2 import BOX, OPTS, bumpy, quad, rosen

FUNS = [quad([[2.0, 0.3], [0.3, 1.0]], [2.0, 0.8]), rosen(), bumpy(3), rosen(1.7, (0.4, 0.2)), bumpy(1)]
X0 = np.array([[0.5, 0.5], [0.2, 0.3], [2.9, 1.5], [5.0, -3.0], [0.3, 0.2]])        # (point 3 starts outside the box: clipped)
ACTIVE = np.array([True, True, False, True, True])


def test_points_in_lockstep_run_as_each_does_alone():
    batches, visited = [], [[] for _ in FUNS]

    def evaluate(idx, X):
        batches.append(np.array(idx))
        val, jac = np.zeros(len(idx)), np.zeros((len(idx), 2))
        for q, k in enumerate(idx):
            visited[k].append(X[q].copy())
            val[q], jac[q] = FUNS[k](X[q])
        return val, jac

    r = _lockstep(evaluate, X0, ACTIVE, OPTS["maxiter"], OPTS["ftol"], OPTS["gtol"])
    alone = [ibs_amd.minimize2(f, x0, BOX, **OPTS) for f, x0 in zip(FUNS, X0)]
    running = ACTIVE.copy()
    for rnd, idx in enumerate(batches):                    # each round's batch: the still-running points in increasing order
        assert np.array_equal(idx, np.nonzero(running)[0]), (rnd, idx)
        for k in idx:
            running[k] = rnd + 1 < alone[k].nfev
    assert not running.any()
    for k, ref in enumerate(alone):
        if not ACTIVE[k]:
            assert not visited[k] and r["evals"][k] == 0 and r["task"][k] == 10 and np.isnan(r["f"][k])
            assert np.array_equal(r["x"][k], np.clip(X0[k], [b[0] for b in BOX], [b[1] for b in BOX]))
            continue
        assert ref.nfev > 1
        assert np.array_equal(np.array(visited[k]), ref.trace[:, :2])          # the same evaluation points, bit for bit
        assert r["evals"][k] == ref.nfev and r["task"][k] == ref.task
        assert np.array_equal(r["x"][k], ref.x) and r["f"][k] == ref.fun
    assert r["rounds"] == len(batches) == max(ref.nfev for k, ref in enumerate(alone) if ACTIVE[k])
    assert len(set(ref.nfev for k, ref in enumerate(alone) if ACTIVE[k])) > 1   # (the points do stop in different rounds)
