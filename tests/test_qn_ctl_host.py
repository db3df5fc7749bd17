"""The shared quasi-Newton controller (``csrc/host/qn_ctl.h``: the convergence tests, both line
searches, the failure rule, the OWLQN element rules -- the code the four device solvers run) on the
CPU: ``quasi_newton_ctl`` takes every decision from it over the cost function and history of the
reference driver ``quasi_newton``, which is written independently.  Same arithmetic, so the two
must agree bit for bit: the point reached, the whole objective history and the stop reason."""
import numpy as np
import pytest


def _system(X, y, off_diag=1.0):
    """The normal-equation system with an intercept row as the WLS driver hands it to the optimizer:
    (bBar, bbBar, ab, A packed upper by columns, aBar).  ``off_diag`` scales the covariances between
    different features (past 1 the system turns indefinite)."""
    n, nf = X.shape
    aBar, bBar, bbBar = X.mean(0), float(y.mean()), float((y * y).mean())
    cov = (X - aBar).T @ (X - aBar) / n
    cov = np.where(np.eye(nf, dtype=bool), cov, off_diag * cov)
    A = np.ones((nf + 1, nf + 1))
    A[:nf, :nf] = cov + np.outer(aBar, aBar)
    A[:nf, nf] = A[nf, :nf] = aBar
    ab = np.append(X.T @ y / n, bBar)
    i, j = np.triu_indices(nf + 1)
    order = np.argsort(i + j * (j + 1) // 2)
    return bBar, bbBar, ab, A[i[order], j[order]], aBar


def _plain(k, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((40 * k, k))
    y = X @ (rng.standard_normal(k) * (rng.random(k) > 0.3)) + 0.5 + 0.1 * rng.standard_normal(40 * k)
    return X / X.std(0), y / y.std()


def _collinear(k, mix, seed=1):
    """Columns ``mix * common + (1 - mix) * noise`` scaled over three decades, then standardized: what is
    left of the scaling is the rounding of the statistics, on a nearly singular system."""
    rng = np.random.default_rng(seed)
    n = 20 * k
    X = (mix * rng.standard_normal((n, 1)) + (1.0 - mix) * rng.standard_normal((n, k))) * np.logspace(0, 3, k)
    y = X @ (rng.standard_normal(k) / np.logspace(0, 3, k)) + 0.1 * rng.standard_normal(n)
    return X / X.std(0), y / y.std()


def _with_nan(sys_):
    bBar, bbBar, ab, A, aBar = sys_
    ab = ab.copy()
    ab[1] = np.nan
    return bBar, bbBar, ab, A, aBar


def _l1(k, v):
    return np.append(np.full(k, v), 0.0)  # the intercept carries no L1 weight


# (name, system, max_iter, tol, l1 or None)
CASES = [
    ("k5-lbfgs", _system(*_plain(5)), 100, 1e-6, None),
    ("k5-owlqn", _system(*_plain(5)), 100, 1e-6, _l1(5, 0.05)),
    ("k30-lbfgs", _system(*_plain(30)), 100, 1e-6, None),
    ("k30-owlqn", _system(*_plain(30)), 100, 1e-6, _l1(30, 0.01)),
    ("k5-lbfgs-iter0", _system(*_plain(5)), 0, 1e-6, None),
    ("k5-lbfgs-iter1", _system(*_plain(5)), 1, 1e-6, None),
    ("k5-owlqn-iter0", _system(*_plain(5)), 0, 1e-6, _l1(5, 0.05)),
    ("k5-owlqn-iter1", _system(*_plain(5)), 1, 1e-6, _l1(5, 0.05)),
    ("k60-collinear-lbfgs", _system(*_collinear(60, 0.9)), 200, 1e-6, None),
    ("k60-collinear-owlqn", _system(*_collinear(60, 0.9)), 200, 1e-6, _l1(60, 1e-4)),
    ("k20-collinear-lbfgs", _system(*_collinear(20, 0.99)), 200, 1e-6, None),
    ("k20-collinear-owlqn", _system(*_collinear(20, 0.99)), 200, 1e-6, _l1(20, 1e-4)),
    ("k12-indefinite3-lbfgs", _system(*_plain(12, 1), off_diag=3.0), 60, 1e-6, None),
    ("k12-indefinite3-owlqn", _system(*_plain(12, 1), off_diag=3.0), 60, 1e-6, _l1(12, 0.01)),
    ("k12-indefinite5-lbfgs", _system(*_plain(12, 1), off_diag=5.0), 60, 1e-6, None),
    ("k12-indefinite5-owlqn", _system(*_plain(12, 1), off_diag=5.0), 60, 1e-6, _l1(12, 0.01)),
    ("k5-nan-lbfgs", _with_nan(_system(*_plain(5))), 40, 1e-6, None),
    ("k5-nan-owlqn", _with_nan(_system(*_plain(5))), 40, 1e-6, _l1(5, 0.05)),
]


def _run(name, case):
    from net.jgp.labs.sparkdq4ml_amd.ops import native

    _, (bBar, bbBar, ab, A, aBar), max_iter, tol, l1 = case
    return getattr(native.host(), name)(bBar, bbBar, ab, A, aBar, True, max_iter, tol, l1)


@pytest.fixture(scope="module")
def reference():
    return {c[0]: _run("quasi_newton", c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_shared_controller_equals_reference_driver(case, reference):
    x, hist, why = _run("quasi_newton_ctl", case)
    rx, rhist, rwhy = reference[case[0]]
    print(case[0], rwhy, len(rhist))
    assert why == rwhy
    assert len(hist) == len(rhist)
    assert hist.tobytes() == rhist.tobytes()  # bitwise (NaNs included)
    assert np.array_equal(x, rx, equal_nan=True)


def test_cases_reach_every_reason_and_a_failed_pass(reference):
    """The case list keeps its teeth: the reference driver alone ends for each of the four reasons,
    and for each solver some fit contains a failed pass (the history repeats a value)."""
    assert {r[2] for r in reference.values()} == {"max iterations", "function values converged",
                                                  "gradient converged", "search failed"}
    for solver in ("lbfgs", "owlqn"):
        assert any(np.any(h[1:] == h[:-1]) for n, (_, h, _) in reference.items() if solver in n), solver
