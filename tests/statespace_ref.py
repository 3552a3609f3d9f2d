"""Float64 numpy references for the state-space (Kalman) form of a one-dimensional Matern GP: a plain sequential Kalman filter and
Rauch-Tung-Striebel smoother over the conventions of include/svgp_mi355x.h (svgp_ss_*), and the dense Cholesky exact GP they must
equal.  Families: 1 = Matern-3/2, 2 = Matern-5/2 (the C-ABI's codes)."""
import numpy as np


def model(family, variance, inv_lengthscale, dtype=np.float64):
    """-> (lam, N = F + lam I (nilpotent), Pinf), every number in dtype (float64, or longdouble for a reference of the reference)"""
    variance, inv_lengthscale = dtype(variance), dtype(inv_lengthscale)
    if family == 1:
        lam = np.sqrt(dtype(3.0)) * inv_lengthscale
        F = np.array([[0.0, 1.0], [-lam**2, -2.0 * lam]], dtype=dtype)
        Pinf = np.diag(np.array([variance, lam**2 * variance], dtype=dtype))
    elif family == 2:
        lam = np.sqrt(dtype(5.0)) * inv_lengthscale
        F = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-lam**3, -3.0 * lam**2, -3.0 * lam]], dtype=dtype)
        kap = variance * lam**2 / dtype(3.0)
        Pinf = np.array([[variance, 0.0, -kap], [0.0, kap, 0.0], [-kap, 0.0, lam**4 * variance]], dtype=dtype)
    else:
        raise ValueError("the state-space form needs a Matern-3/2 or Matern-5/2 kernel")
    return lam, F + lam * np.eye(F.shape[0], dtype=dtype), Pinf


def transition(family, variance, inv_lengthscale, dt):
    """-> (A(dt), Q(dt) = Pinf - A Pinf A')"""
    lam, N, Pinf = model(family, variance, inv_lengthscale)
    A, term = np.eye(N.shape[0]), np.eye(N.shape[0])
    for p in range(1, N.shape[0]):
        term = term @ N * (dt / p)
        A = A + term
    A = np.exp(-lam * dt) * A
    return A, Pinf - A @ Pinf @ A.T


def kalman(family, variance, inv_lengthscale, t, delta, r):
    """Sequential filter and RTS smoother over the sorted times t.  r[k] < 0: no observation at point k (a test point).
    -> (lml, smoothed latent mean (without the prior mean), smoothed latent variance)"""
    t, delta, r = (np.asarray(a, dtype=np.float64) for a in (t, delta, r))
    n = t.shape[0]
    _, N, Pinf = model(family, variance, inv_lengthscale)
    D = N.shape[0]
    ms, Ps, mp, Pp, As = np.zeros((n, D)), np.zeros((n, D, D)), np.zeros((n, D)), np.zeros((n, D, D)), np.zeros((n, D, D))
    m, P, lml = np.zeros(D), Pinf.copy(), 0.0
    for k in range(n):
        if k > 0:
            A, Q = transition(family, variance, inv_lengthscale, t[k] - t[k - 1])
            m, P = A @ m, A @ P @ A.T + Q
            As[k] = A
        mp[k], Pp[k] = m, P
        if r[k] >= 0:
            S, e = P[0, 0] + r[k], delta[k] - m[0]
            K = P[:, 0] / S
            m, P = m + K * e, P - np.outer(K, P[0, :])
            lml -= 0.5 * (np.log(2.0 * np.pi * S) + e * e / S)
        ms[k], Ps[k] = m, P
    sm, sP = ms[-1], Ps[-1]
    mean, var = np.zeros(n), np.zeros(n)
    mean[-1], var[-1] = sm[0], sP[0, 0]
    for k in range(n - 2, -1, -1):
        E = np.linalg.solve(Pp[k + 1], As[k + 1] @ Ps[k]).T
        sm = ms[k] + E @ (sm - mp[k + 1])
        sP = Ps[k] + E @ (sP - Pp[k + 1]) @ E.T
        mean[k], var[k] = sm[0], sP[0, 0]
    return lml, mean, var


def filter_lml(family, variance, inv_lengthscale, t, delta, r, dtype=np.float64):
    """The log marginal likelihood alone, by the sequential filter of kalman() without its smoother and without stored moments, every
    operation in dtype: with np.longdouble it is the float64 filter's own higher-precision check at sizes no dense factor reaches (no
    linear solve; numpy's @ works in long double).  r[k] < 0: no observation at point k."""
    t, delta, r = (np.asarray(a, dtype=dtype) for a in (t, delta, r))
    lam, N, Pinf = model(family, variance, inv_lengthscale, dtype)
    D = N.shape[0]
    eye, two_pi, half = np.eye(D, dtype=dtype), dtype(8.0) * np.arctan(dtype(1.0)), dtype(0.5)
    m, P, lml = np.zeros(D, dtype=dtype), Pinf.copy(), dtype(0.0)
    for k in range(t.shape[0]):
        if k > 0:
            dt = t[k] - t[k - 1]
            A, term = eye, eye
            for p in range(1, D):
                term = term @ N * (dt / p)
                A = A + term
            A = np.exp(-lam * dt) * A
            m, P = A @ m, A @ P @ A.T + (Pinf - A @ Pinf @ A.T)
        if r[k] >= 0:
            S, e = P[0, 0] + r[k], delta[k] - m[0]
            K = P[:, 0] / S
            m, P = m + K * e, P - np.outer(K, P[0, :])
            lml -= half * (np.log(two_pi * S) + e * e / S)
    return lml


def kernel_matrix(family, variance, inv_lengthscale, a, b, dtype=np.float64):
    variance, inv_lengthscale = dtype(variance), dtype(inv_lengthscale)
    rr = np.abs(np.asarray(a, dtype=dtype)[:, None] - np.asarray(b, dtype=dtype)[None, :]) * inv_lengthscale
    if family == 1:
        s = np.sqrt(dtype(3.0)) * rr
        return variance * (dtype(1.0) + s) * np.exp(-s)
    s = np.sqrt(dtype(5.0)) * rr
    return variance * (dtype(1.0) + s + s * s / dtype(3.0)) * np.exp(-s)


def _cholesky(K):
    """numpy.linalg stops at float64: the lower Cholesky factor of K in K's dtype, column by column"""
    L = np.zeros_like(K)
    for j in range(K.shape[0]):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _solve_lower(L, B):
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


DENSE_CHUNK = 1 << 15


def dense(family, variance, inv_lengthscale, t, delta, sig2, ts=None, dtype=np.float64):
    """The exact GP by a dense Cholesky factor.  sig2: the noise variances, a scalar or (N,).  dtype: np.longdouble where float64 is
    not enough for a reference (a noise variance far below the kernel's: K + sig2 I has a condition number of 1e8 and more).
    -> (lml, latent mean at ts (without the prior mean), latent variance at ts); ts None: the data times."""
    f64 = dtype == np.float64
    chol, solve = (np.linalg.cholesky, np.linalg.solve) if f64 else (_cholesky, _solve_lower)
    t, delta = np.asarray(t, dtype=dtype), np.asarray(delta, dtype=dtype)
    ts = t if ts is None else np.asarray(ts, dtype=dtype)
    K = kernel_matrix(family, variance, inv_lengthscale, t, t, dtype) + np.diag(np.broadcast_to(np.asarray(sig2, dtype=dtype), t.shape))
    L = chol(K)
    w = solve(L, delta)
    two_pi = 2.0 * np.pi if f64 else dtype(8.0) * np.arctan(dtype(1.0))
    lml = -dtype(0.5) * (w @ w) - np.log(np.diag(L)).sum() - dtype(0.5) * t.shape[0] * np.log(two_pi)
    mean, var = np.zeros(ts.shape[0], dtype=dtype), np.zeros(ts.shape[0], dtype=dtype)
    for c in range(0, ts.shape[0], DENSE_CHUNK):   # K(t, ts) in column chunks: few data and very many test times fit in memory
        V = solve(L, kernel_matrix(family, variance, inv_lengthscale, t, ts[c:c + DENSE_CHUNK], dtype))
        mean[c:c + DENSE_CHUNK], var[c:c + DENSE_CHUNK] = V.T @ w, dtype(variance) - (V * V).sum(0)
    return lml, mean, var


def merged(t, delta, sig2, ts):
    """The union the device runs over: the sorted test times ts merged behind equal data times as unobserved points.
    -> (t, delta, r, index of every test point in the union)"""
    t, ts = np.asarray(t, dtype=np.float64), np.asarray(ts, dtype=np.float64)
    pos_t = np.arange(t.shape[0]) + np.searchsorted(ts, t, side="left")
    pos_s = np.arange(ts.shape[0]) + np.searchsorted(t, ts, side="right")
    n = t.shape[0] + ts.shape[0]
    tm, dm, rm = np.zeros(n), np.zeros(n), np.full(n, -1.0)
    tm[pos_t], dm[pos_t], rm[pos_t] = t, delta, np.broadcast_to(np.asarray(sig2, dtype=np.float64), t.shape)
    tm[pos_s] = ts
    return tm, dm, rm, pos_s


TILE = 64                                                   # the device scans' tile: elements per workgroup at every level
SIZES = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
RECURSIVE_N = TILE * TILE + TILE + 1                        # 66 tile aggregates: more than one workgroup of them
DEEP_U = TILE ** 3                                          # the last scan of 3 levels; one more element: the aggregates' scan recurses
DEEP_N = TILE ** 3 + TILE + 1                               # a 4-level fit with a partial tile at levels 1 and 2
KINDS = ("plain", "repeat", "noise", "short", "long", "quiet", "loud")
NOISE = {"quiet": 2.0 ** -20, "loud": 2.0 ** 10}            # the scalar noise variance of a kind; every other kind: 0.125
DENSE_DTYPE = {"quiet": np.longdouble, "loud": np.longdouble}   # quiet: cond(K + sig2 I) ~ 1e8, the float64 factor loses 1e-8 itself


def scan_levels(n):
    """The depth of the device's scan over n elements: 1 for a single tile, one more per scan of aggregates (the library's
    ss_scan_levels; svgp_ss_info.levels reports it for the fit only)."""
    levels, m = 1, -(-n // TILE)
    while m > 1:
        levels += 1
        if m <= TILE:
            break
        m = -(-m // TILE)
    return levels


def problem(N, kind="plain", seed=0, span=10.0):
    """One regression problem whose every number is exact in float32, so that one float64 reference serves both data dtypes.
    kind: repeat - repeated time stamps; noise - per-point noise variances; short / long - a lengthscale far below the spacing
    (A ~ 0) / far above the span (Q ~ 0, ill-conditioned); quiet / loud - a noise variance of 2^-20 / 2^10 (J = 1 / r large / ~ 0).
    The test times lie before the first and after the last datum, on data and strictly between data.  span: the data lie on
    [0, span] (a float32-exact number; one that grows with N keeps a large problem out of the `long` regime).  diag: the scalar part
    of sig2."""
    rng = np.random.default_rng([seed, N])
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    t = np.sort(f32(rng.uniform(0.0, span, N)))
    if kind == "repeat" and N > 4:
        t[1], t[N // 2], t[N - 1] = t[2], t[N // 2 - 1], t[N - 2]
    y = f32(np.sin(t) + 0.3 * rng.standard_normal(N) + 0.5)
    step = max(1, N // 48)
    between = f32(0.5 * (t[:-1] + t[1:]))[::step]
    ts = np.sort(np.concatenate([f32([-1.5, -0.25]), t[::step], between, f32([span + 0.5, span + 3.0])]))
    diag = NOISE.get(kind, 0.125)
    sig2 = diag + (np.floor(rng.uniform(0.0, 256.0, N)) / 1024.0 if kind == "noise" else 0.0)
    ell = {"short": 2.0 ** -14, "long": 2.0 ** 12}.get(kind, 1.0)
    return dict(t=t, y=y, ts=ts, sig2=sig2, diag=diag, variance=1.25, inv_lengthscale=1.0 / ell, mean_const=0.5)


def grid_times(n):
    """n float32-exact, increasing test times spread over [-2, 12): -2 + 7 k / 2^17 at n evenly chosen k < 2^18"""
    assert 0 <= n <= 1 << 18
    return -2.0 + np.floor(np.arange(n) * float(1 << 18) / max(n, 1)) * (7.0 / 131072.0)


def union_problem(U):
    """problem(40) (U <= 2 TILE) or problem(129) with test times - every data time that fits and grid_times - chosen so that the union
    the device scans has exactly U points."""
    p = problem(40 if U <= 2 * TILE else 129)
    N = p["t"].shape[0]
    k = min(N, (U - N) // 2)
    return dict(p, ts=np.sort(np.concatenate([p["t"][:k], grid_times(U - N - k)])))


LAYOUTS = ("one_before", "one_on", "one_after", "all_before", "all_after", "run", "single")


def layout_problem(name):
    """problem(129) under the test-time layouts the default problems leave out: one test time (before, on, after the data), every
    test time on one side of the data, 70 copies of one data time (a run of dt = 0 longer than a tile, across a tile boundary of the
    union in both scan directions); single: one datum and 200 test times."""
    if name == "single":
        return dict(problem(1), ts=grid_times(200))
    p = problem(129)
    ts = {"one_before": np.array([-1.5]), "one_on": p["t"][64:65], "one_after": np.array([13.0]),
          "all_before": -2.0 + np.arange(37) / 32.0, "all_after": 10.5 + np.arange(37) / 32.0, "run": np.repeat(p["t"][64], 70)}[name]
    return dict(p, ts=ts)


def deep_problem():
    """The 4-level fit: DEEP_N points, 64 per lengthscale (span N / 64: the regular regime, not `long`)"""
    return problem(DEEP_N, span=DEEP_N / 64.0)


def sequential_errors(family, p, dtype=np.float64):
    """The distance of the sequential float64 filter / smoother over the union to the dense GP (factored in dtype) -> (lml relative,
    mean, var of the prior variance): what anchors the tolerances (profiles/statespace/accuracy.md)"""
    v, il, dl = p["variance"], p["inv_lengthscale"], p["y"] - p["mean_const"]
    lml_d, mean_d, var_d = (np.asarray(a, dtype=np.float64) for a in dense(family, v, il, p["t"], dl, p["sig2"], p["ts"], dtype))
    tm, dm, rm, pos = merged(p["t"], dl, p["sig2"], p["ts"])
    lml_s, mean_s, var_s = kalman(family, v, il, tm, dm, rm)
    return abs(lml_s - lml_d) / abs(lml_d), np.abs(mean_s[pos] - mean_d).max() / v, np.abs(var_s[pos] - var_d).max() / v


RUN_SPREAD = 3.9e-16   # run_spread(): measured 3.83e-16 (family 1, variances; 0 for the means and for family 2)


def run_spread(family):
    """The sequential float64 smoother over layout_problem("run"): how far the marginals at its 70 equal test times are from one value
    (largest minus smallest, of the prior variance) -> (means, variances).  The dense GP's 70 columns are one column; the smoother's
    gain P A' (A P A' + Q)^-1 at dt = 0 is the identity only up to the rounding of its solve."""
    p = layout_problem("run")
    tm, dm, rm, pos = merged(p["t"], p["y"] - p["mean_const"], p["sig2"], p["ts"])
    _, mean, var = kalman(family, p["variance"], p["inv_lengthscale"], tm, dm, rm)
    return np.ptp(mean[pos]) / p["variance"], np.ptp(var[pos]) / p["variance"]


if __name__ == "__main__":   # the reference columns of the new groups in profiles/statespace/accuracy.md
    import time
    for family in (1, 2):
        print("run of 70 equal test times, family %d: sequential spread mean %.2e var %.2e" % ((family,) + run_spread(family)))
    cases = [(f"U={U}", union_problem(U)) for U in (64, 65, 128, 4096, 4097)] + [(n, layout_problem(n)) for n in LAYOUTS]
    cases += [(f"N={N}", problem(N)) for N in (256, 257)]
    cases += [(f"{k} ({d.__name__} factor)", problem(129, k)) for k in ("quiet", "loud") for d in (np.float64, np.longdouble)]
    cases += [(f"U={U} deep", union_problem(U)) for U in (DEEP_U, DEEP_U + 1)]
    for name, p in cases:
        for family in (1, 2):
            t0 = time.time()
            e = sequential_errors(family, p, np.longdouble if "longdouble" in name else np.float64)
            print(f"| {family} | {name} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e} |   ({time.time() - t0:.1f} s)", flush=True)
    p = deep_problem()
    for family in (1, 2):
        t0 = time.time()
        a = (p["variance"], p["inv_lengthscale"], p["t"], p["y"] - p["mean_const"], np.broadcast_to(p["sig2"], p["t"].shape))
        l64 = filter_lml(family, *a)
        t1 = time.time()
        l80 = filter_lml(family, *a, dtype=np.longdouble)
        print(f"| {family} | N={DEEP_N} fit | {float(abs(l64 - l80) / abs(l80)):.2e} | | |   ({t1 - t0:.1f} s float64, {time.time() - t1:.1f} s long double)", flush=True)
