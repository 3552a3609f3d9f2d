"""CPU-side check (no GPU): a sequential NumPy reference of svgp_ss_sample (Matheron's rule in state-space form; include/svgp_mi355x.h)
draws exactly the dense posterior: the sample is affine in its draws, path = mu + G xi, so xi = 0 gives mu, the unit vectors give G, and
G G' must be the full posterior covariance.  The GPU tests import the reference, the cases and the bounds: each is the float64 reference's
measured distance to its long double twin or to the long double dense GP (profiles/statespace/accuracy.md); the device gets 10 x."""
import functools

import numpy as np
import pytest

import statespace_ref as R

LD = np.longdouble
DIST_KINDS = ("plain", "repeat", "noise", "short")          # noise: per-point variances (set_noise on the device)
# in units of the prior variance (profiles/statespace/accuracy.md, "Sample paths")
MU_TOL, COV_TOL = 1.5e-15, 5.0e-16                          # mu / G G' of the float64 reference against the long double dense GP: 1.13e-15, 3.68e-16
PATH_TOL = {1: 2.0e-14, 2: 4.0e-12}                         # float64 paths against the long double ones, per family: 1.75e-14, 3.50e-12
PATH_U = (R.TILE, R.TILE + 1, R.RECURSIVE_N)                # one tile; one point into the second; 66 aggregates: their scan recurses


def _inv(S):
    """S^-1 in S's dtype by Gauss-Jordan without pivoting (numpy.linalg stops at float64; S symmetric positive definite)"""
    n = S.shape[0]
    M = np.concatenate([S, np.eye(n, dtype=S.dtype)], axis=1)
    for j in range(n):
        M[j] = M[j] / M[j, j]
        M[np.arange(n) != j] -= np.outer(M[np.arange(n) != j, j], M[j])
    return M[:, n:]


def _factor(S):
    """The lower factor of a positive semi-definite S by an unpivoted L D L'; a pivot that is not > 0 is dropped with its column"""
    D = S.shape[0]
    L, d = np.eye(D, dtype=S.dtype), np.zeros(D, dtype=S.dtype)
    for j in range(D):
        s = S[j, j] - (L[j, :j] ** 2) @ d[:j]
        d[j] = s if s > 0 else 0
        L[j + 1:, j] = (S[j + 1:, j] - (L[j + 1:, :j] * L[j, :j]) @ d[:j]) / s if s > 0 else 0
    return L * np.sqrt(d)


def sample_ref(family, p, z, eps, dtype=np.float64):
    """Sequential reference of svgp_ss_sample over the problem p (sorted t and ts), every operation in dtype.  z: (S, N + n, D) by point
    identity - rows < N the data, N + j the test time j -, eps: (S, N).  -> (S, n), the paths at the test times"""
    N, n = p["t"].shape[0], p["ts"].shape[0]
    tm, dm, rm, pos = R.merged(p["t"], p["y"] - p["mean_const"], p["sig2"], p["ts"])
    U = N + n
    ident = np.zeros(U, dtype=int)
    ident[pos], ident[np.setdiff1d(np.arange(U), pos)] = N + np.arange(n), np.arange(N)
    tm, dm, rm, z, eps = (np.asarray(a, dtype=dtype) for a in (tm, dm, rm, z, eps))
    lam, Nil, Pinf = R.model(family, p["variance"], p["inv_lengthscale"], dtype)
    D, S = Nil.shape[0], z.shape[0]
    eye = np.eye(D, dtype=dtype)
    ft, ms = np.zeros((U, S), dtype=dtype), np.zeros((U, D, S), dtype=dtype)
    As, Ps, Pms = np.zeros((U, D, D), dtype=dtype), np.zeros((U, D, D), dtype=dtype), np.zeros((U, D, D), dtype=dtype)
    x, m, P = np.zeros((D, S), dtype=dtype), np.zeros((D, S), dtype=dtype), Pinf
    for k in range(U):   # the prior path, and the filter over the residual rho = delta - ft - sqrt(r) eps
        Q = Pinf
        if k > 0:
            dt, A, term = tm[k] - tm[k - 1], eye, eye
            for q in range(1, D):
                term = term @ Nil * (dt / q)
                A = A + term
            As[k] = np.exp(-lam * dt) * A
            Q = Pinf - As[k] @ Pinf @ As[k].T
            P = As[k] @ P @ As[k].T + Q
        x = As[k] @ x + _factor(Q) @ z[:, ident[k]].T
        ft[k], m, Pms[k] = x[0], As[k] @ m, P
        if rm[k] >= 0:
            K = P[:, 0] / (P[0, 0] + rm[k])
            rho = dm[k] - ft[k] - np.sqrt(rm[k]) * eps[:, ident[k]]
            m, P = m + np.outer(K, rho - m[0]), P - np.outer(K, P[0])
        ms[k], Ps[k] = m, P
    sm, out = ms[-1], np.zeros((S, n), dtype=dtype)
    slot = {int(u): j for j, u in enumerate(pos)}
    for k in range(U - 1, -1, -1):   # the smoothed mean of the residual: mhat_k = m_k + E_k (mhat_{k+1} - A_{k+1} m_k)
        if k < U - 1:
            sm = ms[k] + Ps[k] @ As[k + 1].T @ _inv(Pms[k + 1]) @ (sm - As[k + 1] @ ms[k])
        if k in slot:
            out[:, slot[k]] = ft[k] + sm[0] + dtype(p["mean_const"])
    return out


def dist_problem(kind):
    """N = 40 data points and n = 25 of problem()'s test times (before, on, between and after the data): U = 65 crosses one tile edge"""
    p = R.problem(40, kind)
    return dict(p, ts=p["ts"][np.linspace(0, p["ts"].shape[0] - 1, 25).astype(int)])


def unit_draws(N, n, D):
    """xi = 0 and every unit vector: -> z (1 + U D + N, U, D), eps (1 + U D + N, N)"""
    U = N + n
    xi = np.concatenate([np.zeros((1, U * D + N)), np.eye(U * D + N)])
    return xi[:, :U * D].reshape(-1, U, D), xi[:, U * D:]


@functools.lru_cache(maxsize=None)
def dense_posterior(family, kind):
    """-> (problem, mean, covariance) of the dense posterior at the test times, in long double"""
    p = dist_problem(kind)
    k = lambda a, b: R.kernel_matrix(family, p["variance"], p["inv_lengthscale"], a, b, LD)
    Kxs = k(p["t"], p["ts"])
    W = _inv(k(p["t"], p["t"]) + np.diag(np.broadcast_to(np.asarray(p["sig2"], dtype=LD), p["t"].shape))) @ Kxs
    return p, W.T @ np.asarray(p["y"] - p["mean_const"], dtype=LD), k(p["ts"], p["ts"]) - Kxs.T @ W


def distribution_errors(p, mean, cov, paths):
    """paths (n, 1 + U D + N) from unit_draws -> the distances of mu and G G' to the dense posterior, of the prior variance"""
    paths = np.asarray(paths, dtype=LD)
    mu, G = paths[:, 0], paths[:, 1:] - paths[:, :1]
    return float(np.abs(mu - p["mean_const"] - mean).max() / p["variance"]), float(np.abs(G @ G.T - cov).max() / p["variance"])


def path_problem(U):
    """A union of exactly U points, plain parameters, every time step 0 (a test time on a datum) or >= 1 / 16 of the lengthscale: data on
    a jittered grid, test times before, on, half-way between and after them.  Q(dt) = Pinf - A Pinf A' has an absolute rounding error of
    ~1e-16; where Q_11 ~ dt^3 / dt^5 comes near it, Q's factor - the map from draws to paths, not their distribution - is no stable
    function of its input (R.union_problem(4161), steps down to 1e-5: float64 against long double 1.7e-5 / 2.2e-2), as for `short`."""
    n = U // 3
    N, rng = U - n, np.random.default_rng([7, U])
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    t = f32((np.arange(N) + 0.5 * rng.uniform(size=N)) / 4.0)
    y = f32(np.sin(t) + 0.3 * rng.standard_normal(N) + 0.5)
    between = f32(0.5 * (t[:-1] + t[1:]))[-(n - n // 2 - 2):]
    ts = np.sort(np.concatenate([f32([-1.5]), t[:n // 2], between, f32([t[-1] + 0.5])]))
    return dict(R.problem(1), t=t, y=y, ts=ts)


@functools.lru_cache(maxsize=None)
def path_case(family, U):
    """-> (problem of U union points, z (5, U, D), eps (5, N), the float64 reference's paths (5, n))"""
    p = path_problem(U)
    N, rng = p["t"].shape[0], np.random.default_rng([family, U])
    z, eps = rng.standard_normal((5, U, family + 1)), rng.standard_normal((5, N))
    return p, z, eps, sample_ref(family, p, z, eps)


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("kind", DIST_KINDS)
def test_the_reference_draws_the_dense_posterior(family, kind):
    p, mean, cov = dense_posterior(family, kind)
    z, eps = unit_draws(40, 25, family + 1)
    e_mu, e_cov = distribution_errors(p, mean, cov, sample_ref(family, p, z, eps).T)
    print(f"ss sample reference family={family} {kind}: mu {e_mu:.2e} G G' {e_cov:.2e}")
    assert e_mu <= MU_TOL and e_cov <= COV_TOL


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("U", PATH_U)
def test_float64_paths_against_long_double(family, U):
    p, z, eps, ref = path_case(family, U)
    assert p["t"].shape[0] + p["ts"].shape[0] == U and ref.dtype == np.float64
    err = float(np.abs(ref - sample_ref(family, p, z, eps, LD)).max() / p["variance"])
    print(f"ss sample reference family={family} U={U}: float64 against long double {err:.2e}")
    assert err <= PATH_TOL[family]
