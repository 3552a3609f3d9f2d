"""Float64 numpy references for the state-space (Kalman) form of a one-dimensional Matern GP: a plain sequential Kalman filter and
Rauch-Tung-Striebel smoother over the conventions of include/svgp_mi355x.h (svgp_ss_*), and the dense Cholesky exact GP they must
equal.  Families: 1 = Matern-3/2, 2 = Matern-5/2 (the C-ABI's codes)."""
import numpy as np


def model(family, variance, inv_lengthscale):
    """-> (lam, N = F + lam I (nilpotent), Pinf)"""
    if family == 1:
        lam = np.sqrt(3.0) * inv_lengthscale
        F = np.array([[0.0, 1.0], [-lam**2, -2.0 * lam]])
        Pinf = np.diag([variance, lam**2 * variance])
    elif family == 2:
        lam = np.sqrt(5.0) * inv_lengthscale
        F = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-lam**3, -3.0 * lam**2, -3.0 * lam]])
        kap = variance * lam**2 / 3.0
        Pinf = np.array([[variance, 0.0, -kap], [0.0, kap, 0.0], [-kap, 0.0, lam**4 * variance]])
    else:
        raise ValueError("the state-space form needs a Matern-3/2 or Matern-5/2 kernel")
    return lam, F + lam * np.eye(F.shape[0]), Pinf


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


def kernel_matrix(family, variance, inv_lengthscale, a, b):
    rr = np.abs(np.asarray(a, dtype=np.float64)[:, None] - np.asarray(b, dtype=np.float64)[None, :]) * inv_lengthscale
    if family == 1:
        s = np.sqrt(3.0) * rr
        return variance * (1.0 + s) * np.exp(-s)
    s = np.sqrt(5.0) * rr
    return variance * (1.0 + s + s * s / 3.0) * np.exp(-s)


def dense(family, variance, inv_lengthscale, t, delta, sig2, ts=None):
    """The exact GP by a dense Cholesky factor.  sig2: the noise variances, a scalar or (N,).
    -> (lml, latent mean at ts (without the prior mean), latent variance at ts); ts None: the data times."""
    t, delta = np.asarray(t, dtype=np.float64), np.asarray(delta, dtype=np.float64)
    ts = t if ts is None else np.asarray(ts, dtype=np.float64)
    K = kernel_matrix(family, variance, inv_lengthscale, t, t) + np.diag(np.broadcast_to(np.asarray(sig2, dtype=np.float64), t.shape))
    L = np.linalg.cholesky(K)
    w = np.linalg.solve(L, delta)
    lml = -0.5 * (w @ w) - np.log(np.diag(L)).sum() - 0.5 * t.shape[0] * np.log(2.0 * np.pi)
    V = np.linalg.solve(L, kernel_matrix(family, variance, inv_lengthscale, t, ts))
    return lml, V.T @ w, variance - (V * V).sum(0)


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
KINDS = ("plain", "repeat", "noise", "short", "long")


def problem(N, kind="plain", seed=0):
    """One regression problem whose every number is exact in float32, so that one float64 reference serves both data dtypes.
    kind: repeat - repeated time stamps; noise - per-point noise variances; short / long - a lengthscale far below the spacing
    (A ~ 0) / far above the span (Q ~ 0, ill-conditioned).  The test times lie before the first and after the last datum, on data and
    strictly between data."""
    rng = np.random.default_rng([seed, N])
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    span = 10.0
    t = np.sort(f32(rng.uniform(0.0, span, N)))
    if kind == "repeat" and N > 4:
        t[1], t[N // 2], t[N - 1] = t[2], t[N // 2 - 1], t[N - 2]
    y = f32(np.sin(t) + 0.3 * rng.standard_normal(N) + 0.5)
    step = max(1, N // 48)
    between = f32(0.5 * (t[:-1] + t[1:]))[::step]
    ts = np.sort(np.concatenate([f32([-1.5, -0.25]), t[::step], between, f32([span + 0.5, span + 3.0])]))
    sig2 = 0.125 + (np.floor(rng.uniform(0.0, 256.0, N)) / 1024.0 if kind == "noise" else 0.0)
    ell = {"short": 2.0 ** -14, "long": 2.0 ** 12}.get(kind, 1.0)
    return dict(t=t, y=y, ts=ts, sig2=sig2, variance=1.25, inv_lengthscale=1.0 / ell, mean_const=0.5)
