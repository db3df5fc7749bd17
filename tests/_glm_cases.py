"""Shared inputs and oracles of the GLM tests (test_glm_host.py, test_gpu_glm.py, test_gpu_glm_api.py).

Nothing here imports the package's family / link tables: the numpy definitions below and the
stand-alone IRLS (``numpy.linalg.lstsq`` on sqrt(w')-scaled rows) are written out again, so a wrong
table entry in ``ops/glm.py`` or in the kernel cannot hide behind itself.
"""
import numpy as np

PAIRS = [("gaussian", "identity"), ("gaussian", "log"), ("gaussian", "inverse"), ("binomial", "logit"),
         ("poisson", "log"), ("poisson", "identity"), ("poisson", "sqrt"), ("gamma", "inverse"),
         ("gamma", "identity"), ("gamma", "log")]
PAIR_IDS = [f"{f}-{l}" for f, l in PAIRS]
INIT, STEP = 0, 1
EPS = 1e-16
TOL = 1e-12  # |got_k - ref_k| <= TOL * S_k: the project's bound for f64 row reductions


# ---- the tables, numpy ---------------------------------------------------------------------------
def np_link(link, mu):
    return {"identity": lambda: mu, "log": lambda: np.log(mu), "logit": lambda: np.log(mu / (1 - mu)),
            "inverse": lambda: 1 / mu, "sqrt": lambda: np.sqrt(mu)}[link]()


def np_unlink(link, eta):
    return {"identity": lambda: eta, "log": lambda: np.exp(eta), "logit": lambda: 1 / (1 + np.exp(-eta)),
            "inverse": lambda: 1 / eta, "sqrt": lambda: eta * eta}[link]()


def np_dlink(link, mu):
    return {"identity": lambda: np.ones_like(mu), "log": lambda: 1 / mu, "logit": lambda: 1 / (mu * (1 - mu)),
            "inverse": lambda: -1 / (mu * mu), "sqrt": lambda: 1 / (2 * np.sqrt(mu))}[link]()


def np_variance(family, mu):
    return {"gaussian": lambda: np.ones_like(mu), "binomial": lambda: mu * (1 - mu), "poisson": lambda: mu,
            "gamma": lambda: mu * mu}[family]()


def np_project(family, mu):
    big = np.finfo(np.float64).max
    if family == "gaussian":
        return np.clip(mu, -big, big)
    if family == "binomial":
        return np.clip(mu, EPS, 1 - EPS)
    return np.clip(mu, EPS, big)


def np_init(family, y, w):
    if family == "binomial":
        return (w * y + 0.5) / (w + 1)
    if family == "poisson":
        return np.maximum(y, 0.1)
    return y


def np_working(family, link, eta, y, w, mode):
    if mode == INIT:
        return np_link(link, np_init(family, y, w)), w
    mu = np_project(family, np_unlink(link, eta))
    g = np_dlink(link, mu)
    return eta + (y - mu) * g, w / (g * g * np_variance(family, mu))


def np_unit_deviance(family, y, mu, w):
    def ylog(a, b):
        return np.where(a == 0, 0.0, a * np.log(np.where(a == 0, 1.0, a) / b))
    if family == "gaussian":
        return w * (y - mu) ** 2
    if family == "binomial":
        return 2 * w * (ylog(y, mu) + ylog(1 - y, 1 - mu))
    if family == "poisson":
        return 2 * w * (ylog(y, mu) - (y - mu))
    return -2 * w * (np.log(y / mu) - (y - mu) / mu)


# ---- inputs --------------------------------------------------------------------------------------
def _eta_range(family, link):
    """(intercept, half width): eta stays in [b - c, b + c], |eta| <= 4, mu far from the clamps and
    inside the domain of the link (inverse, sqrt and a positive-mean identity need eta > 0)."""
    if link in ("inverse", "sqrt") or (link == "identity" and family in ("poisson", "gamma")):
        return 2.25, 1.5
    return 0.2, 1.5


def make_case(family, link, n, d, seed, weights=False, dead=False, xdtype=np.float64, small_noise=False):
    """Feature-major X [d, n] (|x| <= 1, rounded to ``xdtype``), label drawn from the family at the
    true coefficients, optional weights in [0.5, 2], optional selection with ~1/5 dead rows whose
    features and label are NaN.  beta = [coef(d), intercept] keeps eta inside ``_eta_range``.
    ``small_noise``: poisson / gamma labels are mu (1 + 0.01 N(0, 1)) instead of draws (IRLS with a
    non-canonical link then converges fast enough for two implementations to stop together)."""
    rng = np.random.default_rng(seed)
    b, c = _eta_range(family, link)
    X = rng.uniform(-1, 1, size=(d, n)).astype(xdtype).astype(np.float64)
    coef = rng.choice([-1.0, 1.0], size=d) * rng.uniform(0.5, 1.0, size=d) * (c / d)
    beta = np.concatenate([coef, [b]])
    eta = coef @ X + b
    mu = np_unlink(link, eta)
    if family == "gaussian":
        y = mu + (0.02 if link != "identity" else 0.3) * rng.standard_normal(n)
        if link != "identity":
            y = np.maximum(y, 0.05)  # Spark's starting model takes link(y)
    elif family == "binomial":
        y = (rng.random(n) < mu).astype(np.float64)
    elif small_noise:
        y = mu * (1 + 0.01 * rng.standard_normal(n))
    elif family == "poisson":
        y = rng.poisson(mu).astype(np.float64)
    else:
        y = rng.gamma(4.0, mu / 4.0)
    w = rng.uniform(0.5, 2.0, size=n) if weights else None
    sel = None
    if dead:
        sel = rng.random(n) >= 0.2
        if n >= 1 and not sel.any():
            sel[0] = True
        X = X.copy()
        X[:, ~sel] = np.nan
        y = y.copy()
        y[~sel] = np.nan
    return {"X": X.astype(xdtype), "y": y, "w": w, "sel": sel, "beta": beta, "family": family, "link": link}


def packed_upper(M):
    d = M.shape[0]
    return np.array([M[i, j] for j in range(d) for i in range(j + 1)], dtype=M.dtype)


def abs_sums(case, beta, mode):
    """S_k of every component of the flat statistics: the fp64 sum of the absolute per-row terms."""
    X = np.asarray(case["X"], dtype=np.float64)
    d, n = X.shape
    live = np.ones(n, bool) if case["sel"] is None else case["sel"]
    X = np.where(live, X, 0.0)
    y = np.where(live, case["y"], 1.0)
    w = np.ones(n) if case["w"] is None else case["w"]
    eta = np.asarray(beta[:d]) @ X + beta[d]
    z, wp = np_working(case["family"], case["link"], eta, y, w, mode)
    z, wp = np.where(live, z, 0.0), np.where(live, wp, 0.0)
    aw = np.abs(wp)
    ax = np.abs(X)
    return np.concatenate([[float(live.sum()), aw.sum(), (wp * wp).sum(), (aw * np.abs(z)).sum(), (aw * z * z).sum()],
                           ax @ aw, ax @ (aw * np.abs(z)), packed_upper((ax * aw) @ ax.T)])


def check_flat(got, ref, S, what):
    """Assert the bound, printing the largest |delta| / S first."""
    got, ref, S = (np.asarray(v, dtype=np.float64) for v in (got, ref, S))
    assert got.shape == ref.shape == S.shape, (what, got.shape, ref.shape, S.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite statistics"
    err = np.abs(got - ref)
    ratio = float(np.max(np.where(S > 0, err / np.where(S > 0, S, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: max |d|/S = {ratio:.3e}")
    assert np.all(err <= TOL * S), f"{what}: max |d|/S = {ratio:.3e} > {TOL}"


# ---- the stand-alone IRLS ------------------------------------------------------------------------
def oracle_irls(X, y, w, family, link, fit_icpt=True, tol=1e-6, max_iter=25, reg=0.0):
    """Spark's loop on rows X [n, d]: (coef, intercept, iterations, [max |delta| per iteration]).
    Each solve is a least-squares problem on sqrt(w')-scaled rows; ``reg`` (L2 on the coefficients,
    objective 1/(2 sum w') sum w' (z - x.beta - b)^2 + reg/2 |beta|^2) adds d rows."""
    n, d = X.shape
    w = np.ones(n) if w is None else w
    A = np.hstack([X, np.ones((n, 1))]) if fit_icpt else X

    def solve(z, wp):
        s = np.sqrt(wp)
        Ar, br = A * s[:, None], z * s
        if reg > 0:
            pen = np.zeros((d, A.shape[1]))
            pen[np.arange(d), np.arange(d)] = np.sqrt(reg * wp.sum())
            Ar, br = np.vstack([Ar, pen]), np.concatenate([br, np.zeros(d)])
        return np.linalg.lstsq(Ar, br, rcond=None)[0]

    z, wp = np_working(family, link, None, y, w, INIT)
    beta = solve(z, wp)
    deltas = []
    it = 0
    if not (family == "gaussian" and link == "identity"):
        while it < max_iter:
            z, wp = np_working(family, link, A @ beta, y, w, STEP)
            new = solve(z, wp)
            deltas.append(float(np.max(np.abs(new - beta))))
            beta = new
            it += 1
            if deltas[-1] < tol:
                break
    coef, icpt = (beta[:d], float(beta[d])) if fit_icpt else (beta, 0.0)
    return coef, icpt, it, deltas


FIT_N, FIT_D = 333, 5
# Seeds of make_case(family, link, FIT_N, FIT_D, seed, weights=True) at which the oracle's last two
# max |delta| at tol = 1e-6 are each a factor 10 away from tol (the tests assert it), so a last-ulp
# difference between two implementations cannot move numIterations.
FIT_SEEDS = {("gaussian", "identity"): 1, ("gaussian", "log"): 95, ("gaussian", "inverse"): 35,
             ("binomial", "logit"): 1, ("poisson", "log"): 1, ("poisson", "identity"): 28, ("poisson", "sqrt"): 1,
             ("gamma", "inverse"): 4, ("gamma", "identity"): 95, ("gamma", "log"): 1}


FIT_SMALL_NOISE = {("poisson", "identity"), ("poisson", "sqrt"), ("gamma", "identity"), ("gamma", "log")}


def fit_case(family, link, weights=True, seed=None):
    return make_case(family, link, FIT_N, FIT_D, FIT_SEEDS[(family, link)] if seed is None else seed, weights=weights,
                     small_noise=(family, link) in FIT_SMALL_NOISE)


def clear_of_tol(deltas, tol=1e-6):
    """The oracle's last two max |delta| are each a factor 10 away from tol."""
    return len(deltas) >= 2 and deltas[-1] < tol / 10 and deltas[-2] > tol * 10


def rows_of(case, Vectors, with_weight=True):
    """createDataFrame rows (features, label[, weight]) of a case without dead rows."""
    X = np.asarray(case["X"], dtype=np.float64)
    n = X.shape[1]
    w = np.ones(n) if case["w"] is None else case["w"]
    if with_weight:
        return [(Vectors.dense(X[:, i]), float(case["y"][i]), float(w[i])) for i in range(n)]
    return [(Vectors.dense(X[:, i]), float(case["y"][i])) for i in range(n)]
