"""The fused mixture pass (csrc/hip/gmm.hip) against its fp64 twin (ops/gmm.py).

The live-row count and the ASSIGN indices equal the twin's exactly -- the inputs are asserted to keep
every live row's two largest responsibilities more than 1e-9 apart, and its exponent terms
|u_j| + 0.5 |W_j (x - mu_j)|^2 below 64 -- and every other statistic lies within tau S, S the fp64 sum
of the absolute per-row terms.  tau = 1e-12, the project's bound for f64 row reductions
(tests/test_gpu_rowops.py): tests/test_gmm_host.py measured the twin itself within 5.4e-16 S of a
40-digit oracle, well inside the 1e-13 S that tau presumes.  Per row, S is 1 for the probabilities
and 1 + |log P| for log P.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from net.jgp.labs.sparkdq4ml_amd.ops import device, gmm as G  # noqa: E402

TAU = 1e-12
CASES = [(d, k) for d in (1, 15, 16, 17, 32) for k in (2, 8, 16) if G.fused_range(d, k)]
NS = ((1, None), (63, None), (64, None), (65, None), (333, None), (64 * 4 * 3 + 7, 1), (64 * 4 * 3 + 7, 3))


def _dev(X, dtype, pad=0):
    """Feature-major device matrix of ``dtype`` with ``pad`` extra columns behind the rows (ld > n)."""
    t = torch.from_numpy(X).to(dtype)
    if pad:
        t = torch.cat([t, torch.full((t.shape[0], pad), float("nan"), dtype=dtype)], dim=1)
    return t.cuda()[:, :X.shape[1]]


def _mixture(rng, d, k):
    """Covariances A A^T + 0.5 I with |A| <= 0.5 / sqrt(d) and means in [-0.3, 0.3]: at d = 32 wider
    ones push every density of a row in [-1, 1]^d below EPS (u alone is -29 - 0.5 logdet), which
    ties all responsibilities at 1 / k and fails the two input asserts of _check_pass."""
    A = rng.uniform(-0.5, 0.5, (k, d, d)) / np.sqrt(d)
    return rng.dirichlet(np.full(k, 4.0)), rng.uniform(-0.3, 0.3, (k, d)), A @ A.transpose(0, 2, 1) + 0.5 * np.eye(d)


def _bound(X, live, prob, logp):
    """tau S of the STEP statistics from the twin's responsibilities."""
    k, d = prob.shape[0], X.shape[0]
    Xa = np.where(live[None, :], np.abs(X), 0.0)
    iu = np.triu_indices(d)
    S = np.einsum("kn,an,bn->kab", prob, Xa, Xa)[:, iu[0], iu[1]]
    return TAU * np.concatenate([prob.sum(axis=1), (prob @ Xa.T).reshape(-1), S.reshape(-1), [np.abs(logp).sum(), 0.0]])


def _check_pass(X, live, with_sel, par, blocks, dtypes=(torch.float32, torch.float64), pad=0, exact_inputs=True):
    Xn = np.where(live[None, :], X, np.nan)  # dead rows hold NaN
    sel = torch.from_numpy(live) if with_sel else None
    want = G.em_pass_host(torch.from_numpy(Xn), sel, *par, G.STEP).numpy()
    wi, wp, wl = (t.numpy() for t in G.em_pass_host(torch.from_numpy(Xn), sel, *par, G.ASSIGN))
    if exact_inputs:
        for j, (mu, cov) in enumerate(zip(par[1], par[2])):
            W, u = G.gaussian_params(mu, cov)
            z = W @ (X - mu[:, None])
            assert (abs(u) + 0.5 * (z * z).sum(axis=0))[live].max() < 64
        top = np.sort(wp, axis=0)
        assert (top[-1] - top[-2])[live].min() > 1e-9
    bound = _bound(X, live, wp, wl)
    for dtype in dtypes:
        Xd, seld = _dev(Xn, dtype, pad), None if sel is None else sel.cuda()
        got = device.gmm_pass(Xd, seld, *par, G.STEP, blocks).cpu().numpy()
        assert got[-1] == want[-1] == live.sum()
        err = np.abs(got - want)
        print(f"d={X.shape[0]} k={len(par[0])} n={X.shape[1]} {dtype}: worst error / (tau S) = {(err[:-1] / bound[:-1]).max():.3g}")
        assert (err <= bound).all()
        gi, gp, gl = (t.cpu().numpy() for t in device.gmm_pass(Xd, seld, *par, G.ASSIGN, blocks))
        np.testing.assert_array_equal(gi, wi)
        assert (np.abs(gp - wp) <= TAU).all() and (np.abs(gl - wl) <= TAU * (1.0 + np.abs(wl))).all()
        assert (gp[:, ~live] == 0).all() and (gl[~live] == 0).all()
    return wp, wl


@pytest.mark.parametrize("with_sel", [False, True], ids=["all", "sel"])
@pytest.mark.parametrize("d,k", CASES)
def test_pass_equals_twin(d, k, with_sel):
    for n, blocks in NS:
        rng = np.random.default_rng(1000 * d + 10 * k + n)
        X = rng.uniform(-1, 1, (d, n)).astype(np.float32).astype(np.float64)
        live = rng.random(n) < 0.8 if with_sel else np.ones(n, dtype=bool)
        live[0] = True
        _check_pass(X, live, with_sel, _mixture(rng, d, k), blocks, pad=11 if n == 333 else 0)  # ld = 344: aligned


def test_singular_component_and_all_eps_row():
    rng = np.random.default_rng(17)
    d, k, n = 17, 3, 200
    X = rng.uniform(-1, 1, (d, n)).astype(np.float32).astype(np.float64)
    X[:, 70] = 1e3  # every p_j is EPS: r_j = 1 / k, log P = log(k EPS)
    w, mu, cov = _mixture(rng, d, k)
    cov[1] = np.diag(np.where(np.arange(d) == 1, 0.0, rng.uniform(0.5, 1.5, d)))  # the pseudo-inverse drops feature 1
    live = np.ones(n, dtype=bool)
    wp, wl = _check_pass(X, live, False, (w, mu, cov), None, exact_inputs=False)
    assert (wp[:, 70] == 1.0 / k).all() and wl[70] == np.log(k * G.EPS)
    gi, gp, gl = device.gmm_pass(_dev(X, torch.float64), None, w, mu, cov, G.ASSIGN)
    assert gi[70] == 0 and (gp[:, 70].cpu().numpy() == 1.0 / k).all() and float(gl[70]) == np.log(k * G.EPS)


def test_two_runs_are_bit_identical():
    rng = np.random.default_rng(5)
    X = torch.from_numpy(rng.uniform(-1, 1, (17, 20000)).astype(np.float32)).cuda()
    par = _mixture(rng, 17, 8)
    assert torch.equal(device.gmm_pass(X, None, *par, G.STEP).clone(), device.gmm_pass(X, None, *par, G.STEP))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_device_fit_equals_host_loop(dtype):
    """From equal starts the device loop takes the host loop's iterations; each pass adds at most
    tau S to the statistics and EM does not expand differences near a separated optimum, so the
    parameters agree within iterations x tau x (S / sw) of their moments."""
    rng = np.random.default_rng(11)
    k, d, n = 4, 9, 3001
    lab = rng.integers(0, k, n)
    X = (rng.normal(size=(k, d))[lab] * 6 + rng.normal(size=(n, d))).T.astype(np.float32)
    Xh = torch.from_numpy(X).to(dtype)
    start = G.seed_gaussians(Xh, None, k, 3)
    want = G.fit(Xh, None, k, 30, 0.01, init=start, how="host")
    got = device.gmm_fit(Xh.cuda(), None, *start, 30, 0.01)
    assert got.iterations == want.iterations and got.route == "fused"
    _, r, _ = G.em_pass_host(Xh, None, want.weights, want.means, want.covs, G.ASSIGN)
    Xa, sw = np.abs(X.astype(np.float64)), r.numpy().sum(axis=1)
    m1 = (r.numpy() @ Xa.T) / sw[:, None]
    m2 = np.einsum("kn,an,bn->kab", r.numpy(), Xa, Xa) / sw[:, None, None]
    tol = TAU * want.iterations
    assert (np.abs(got.weights - want.weights) <= tol).all() and (np.abs(got.means - want.means) <= tol * m1).all()
    assert (np.abs(got.covs - want.covs) <= tol * (m2 + 2 * m1[:, :, None] * m1[:, None, :])).all()
    assert abs(got.log_likelihood - want.log_likelihood) <= tol * abs(want.log_likelihood)


def test_validation_errors():
    X = torch.zeros(4, 10).cuda()
    par = lambda k, d: (np.full(k, 1.0 / k), np.zeros((k, d)), np.stack([np.eye(d)] * k))  # noqa: E731
    with pytest.raises(ValueError, match="d <= 32"):
        device.gmm_pass(torch.zeros(33, 10).cuda(), None, *par(2, 33), G.STEP)
    with pytest.raises(ValueError, match="k <= 16"):
        device.gmm_pass(X, None, *par(17, 4), G.STEP)
    with pytest.raises(ValueError, match="k <= 8"):
        device.gmm_pass(torch.zeros(17, 10).cuda(), None, *par(9, 17), G.STEP)
    with pytest.raises(ValueError):
        device.gmm_pass(X, None, *par(1, 4), G.STEP)
    with pytest.raises(ValueError, match="f32 / f64"):
        device.gmm_pass(X.to(torch.bfloat16), None, *par(2, 4), G.STEP)
    with pytest.raises(ValueError, match=r"means \[k, d\]"):
        device.gmm_pass(X, None, *par(2, 5), G.STEP)
    with pytest.raises(ValueError, match="no non-zero singular values"):
        device.gmm_pass(X, None, np.full(2, 0.5), np.zeros((2, 4)), np.zeros((2, 4, 4)), G.STEP)
