"""The fused IRLS pass (csrc/hip/glm_irls.hip) against its fp64 twin, and the iteration step kernel.

Bound.  ``|got_k - ref_k| <= 1e-12 * S_k`` with ``S_k`` the fp64 sum of the absolute per-row terms of
component k: the project's bound for f64 row reductions (tests/test_gpu_rowops.py).  The reference
is the twin ``kernels.glm_pass`` on host copies of the same inputs (f32 features widen exactly); it
is compared against a 40-digit oracle in tests/test_glm_host.py.  Every comparison prints its
largest ``|d| / S`` before it asserts.

Dead rows of a selection hold NaN features and NaN labels in every case that has one: a kernel that
multiplied instead of selecting would return NaN statistics.
"""
import numpy as np
import pytest
import torch

import _glm_cases as C

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd.ops import device, kernels  # noqa: E402

DEV = "cuda"
SMALL_BLOCKS = 3
N_LAST = 64 * 4 * SMALL_BLOCKS + 7  # every wave of a SMALL_BLOCKS grid gets a superstep, then the tail
NS = (1, 63, 64, 65, 333, N_LAST)
DS = (1, 16, 17, 33, 64)  # every NT, a partial last tile, a single feature


def _t(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)


def _operands(case, dev, pad=0):
    X = _t(case["X"])
    if pad:  # padded ld: the rows of a wider buffer
        buf = torch.full((X.shape[0], X.shape[1] + pad), float("nan"), dtype=X.dtype)
        buf[:, :X.shape[1]] = X
        X = buf.to(dev)[:, :case["X"].shape[1]]
    else:
        X = X.to(dev)
    return (X, _t(case["y"]).to(dev), None if case["w"] is None else _t(case["w"]).to(dev),
            None if case["sel"] is None else _t(case["sel"], torch.bool).to(dev))


def _compare(case, mode, what, blocks=None, pad=0):
    ref = kernels.glm_pass(*_operands(case, "cpu"), case["beta"], case["family"], case["link"], mode).numpy()
    got = device.glm_pass(*_operands(case, DEV, pad), case["beta"], case["family"], case["link"], mode, blocks)
    C.check_flat(got.cpu().numpy(), ref, C.abs_sums(case, case["beta"], mode), what)
    return got


@pytest.mark.parametrize("family,link", C.PAIRS, ids=C.PAIR_IDS)
def test_every_pair(family, link):
    for xdt in (np.float32, np.float64):
        case = C.make_case(family, link, 333, 17, 7, weights=True, dead=True, xdtype=xdt)
        for mode in (C.INIT, C.STEP):
            _compare(case, mode, f"{family}/{link} {np.dtype(xdt).name} mode {mode}")
        plain = C.make_case(family, link, 333, 17, 8, xdtype=xdt)
        _compare(plain, C.STEP, f"{family}/{link} {np.dtype(xdt).name} no weights, no selection")


@pytest.mark.parametrize("d", DS)
def test_shapes(d):
    for family, link in (("binomial", "logit"), ("gamma", "inverse")):
        for n in NS:
            for xdt in (np.float32, np.float64):
                case = C.make_case(family, link, n, d, 100 + n, weights=True, dead=True, xdtype=xdt)
                tag = f"{family} d={d} n={n} {np.dtype(xdt).name}"
                _compare(case, C.STEP, tag)
                _compare(case, C.INIT, tag + " init")
        # several supersteps per wave and the tail: one block for the 13 supersteps of N_LAST
        case = C.make_case(family, link, N_LAST, d, 5, weights=True, dead=True, xdtype=np.float32)
        for blocks in (1, SMALL_BLOCKS):
            _compare(case, C.STEP, f"{family} d={d} n={N_LAST} blocks={blocks}", blocks=blocks)
        # (775 + 41 = 816 elements between the f32 rows: 16-byte aligned, so the view is read in place)
        _compare(case, C.STEP, f"{family} d={d} n={N_LAST} padded ld", pad=41)


def test_bit_identical_run_to_run():
    case = C.make_case("poisson", "log", 20000, 33, 3, weights=True, dead=True, xdtype=np.float32)
    ops = _operands(case, DEV)
    a = device.glm_pass(*ops, case["beta"], "poisson", "log", C.STEP).clone()
    b = device.glm_pass(*ops, case["beta"], "poisson", "log", C.STEP)
    assert torch.equal(a, b)


def test_validation():
    case = C.make_case("binomial", "logit", 64, 4, 1)
    X, y, w, sel = _operands(case, DEV)
    with pytest.raises(ValueError, match="does not support the log link"):
        device.glm_pass(X, y, w, sel, case["beta"], "binomial", "log", C.STEP)
    with pytest.raises(ValueError, match="1 <= d <= 64"):
        device.glm_pass(torch.zeros(65, 8, device=DEV), y[:8], None, None, np.zeros(66), "binomial", "logit", C.STEP)
    with pytest.raises(ValueError, match="beta must hold"):
        device.glm_pass(X, y, w, sel, np.zeros(3), "binomial", "logit", C.STEP)
    with pytest.raises(ValueError, match="f32 / f64"):
        device.glm_pass(X.to(torch.bfloat16), y, w, sel, case["beta"], "binomial", "logit", C.STEP)


# ---- the step kernel -------------------------------------------------------------------------------
def _step_model(sol, d, tol, init, beta, state):
    """numpy model of glm_step_kernel."""
    beta, state = beta.copy(), state.copy()
    if state[1] != 0:
        return beta, state
    dl = float(np.max(np.abs(beta - sol[:d + 1])))
    ok = sol[d + 1] == 0
    if ok:
        beta = sol[:d + 1].copy()
    if not init:
        state[0] += 1
        state[3] = dl
    if not ok:
        state[1], state[2] = 1, sol[d + 1]
    elif not init and dl < tol:
        state[1] = 1
    return beta, state


@pytest.mark.parametrize("d", (1, 5, 64))
def test_step_transitions(d):
    rng = np.random.default_rng(d)
    tol = 1e-3
    beta, state = np.zeros(d + 1), np.zeros(4)
    dbeta = torch.zeros(d + 1, dtype=torch.float64, device=DEV)
    dstate = torch.zeros(4, dtype=torch.float64, device=DEV)
    base = rng.normal(size=d + 1)
    # the starting model (tiny, yet not "converged"), two moving steps, a converging one, then steps
    # after done (one of them with a failed solve) that must change nothing
    script = [(base * 1e-9, 0.0, True), (base, 0.0, False), (base + 0.5, 0.0, False), (base + 0.5 + 1e-4, 0.0, False),
              (base + 3.0, 0.0, False), (base + 4.0, 7.0, False)]
    for vals, status, init in script:
        sol = np.concatenate([vals, [status], rng.normal(size=5)])
        beta, state = _step_model(sol, d, tol, init, beta, state)
        device.glm_step(torch.as_tensor(sol, device=DEV), d, tol, init, dbeta, dstate)
        assert np.array_equal(dbeta.cpu().numpy(), beta), (vals, status, init)
        assert np.array_equal(dstate.cpu().numpy(), state), (vals, status, init, dstate, state)
    assert state[0] == 3 and state[1] == 1 and state[2] == 0 and state[3] < tol
    # a failed solve before done: done with that status, beta kept
    beta, state = base.copy(), np.array([2.0, 0.0, 0.0, 0.5])
    dbeta, dstate = torch.as_tensor(beta, device=DEV).clone(), torch.as_tensor(state, device=DEV).clone()
    sol = np.concatenate([base + 1.0, [7.0], np.zeros(5)])
    device.glm_step(torch.as_tensor(sol, device=DEV), d, tol, False, dbeta, dstate)
    beta, state = _step_model(sol, d, tol, False, beta, state)
    assert state[1] == 1 and state[2] == 7 and state[0] == 3
    assert np.array_equal(dbeta.cpu().numpy(), beta) and np.array_equal(dstate.cpu().numpy(), state)


def test_enqueued_loop_stops_and_needs_no_host_read():
    family, link = "binomial", "logit"
    case = C.fit_case(family, link)
    X, y, w, sel = _operands(case, DEV)
    coef, icpt, its, deltas = C.oracle_irls(case["X"].T, case["y"], case["w"], family, link)
    assert C.clear_of_tol(deltas)
    loop = device.GlmLoop(X, y, w, sel, family, link, True, 0.0, 1e-6)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loop.start()
        loop.iterate(its + 6)  # more than needed: the extra iterations must be no-ops
    finally:
        torch.cuda.set_sync_debug_mode("default")
    state, beta = loop.state.cpu().numpy(), loop.beta.cpu().numpy()
    assert state[0] == its and state[1] == 1 and state[2] == 0, state
    np.testing.assert_allclose(beta, np.concatenate([coef, [icpt]]), rtol=1e-6, atol=1e-8)
    flat = loop.flat.clone()
    loop.iterate(3)
    assert np.array_equal(loop.beta.cpu().numpy(), beta) and np.array_equal(loop.state.cpu().numpy(), state)
    assert torch.equal(loop.flat, flat)  # the stale slabs fold to the last solve's statistics
