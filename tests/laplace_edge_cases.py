"""The enumerated Laplace edge cases: one table shared by tests/test_gpu_laplace_edges.py (device against reference) and
tests/test_laplace_edges_cpu.py (the reference alone is well inside the tolerances at exactly these inputs).  Every shape is there
because a particular kernel of csrc/laplace.hip can go wrong at it; nothing here is random beyond the seeded inputs."""
import numpy as np

import laplace_ref as lr
import svgp_oracle as o

VARIANCE = 1.1
JITTER = 1e-6
SE, M32, M52 = o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52


def lik_param(lik):
    """the likelihood parameter (Gaussian sigma^2, Gamma alpha) of tests/test_gpu_laplace.py's _s2"""
    return 0.3 if lik == 0 else (2.0 if lik == 4 else 1.0)


def inv_lengthscales(d, seed):
    """distinct per feature (two swapped gradient slots differ), scaled with d so that K does not collapse to the identity"""
    u = np.random.default_rng(1000 + seed).uniform(size=d)
    return (0.6 + 0.8 * u) / np.sqrt(max(d, 2) / 2.0)


# A. the gradient across feature chunks (kLpFc = 8 features per blockIdx.z) and tile edges: (lik, family, d, N), why
GRAD_ROWS = [
    (1, SE, 1, 150),     # VEC layout, one slot in chunk 0
    (2, M32, 8, 150),    # exactly one full chunk
    (5, M52, 9, 150),    # the second chunk holds one feature (the f < d guard)
    (4, SE, 17, 130),    # three chunks; N = 2 * 64 + 2 crosses a 128 panel by two rows
    (3, M52, 64, 130),   # SVGP_MAX_D: eight full chunks, xi_s full
    (1, M32, 64, 65),    # one row in the second 64-tile, a single 128 panel
    (0, M52, 16, 64),    # exactly one 64-tile, Gaussian (d3 = 0, so u = 0)
    (2, SE, 3, 1),       # N = 1: d lml / d inv_lengthscale is exactly 0, the variance slot is not
]
GRAD_ROWVECS_ROW = (4, SE, 17, 130)   # run a second time through a ROWVECS upload
GRAD_MAXITER = 200


def grad_id(row):
    return "lik%d-fam%d-d%d-n%d" % row


def grad_problem(row):
    """-> x (d, n), y, inv_lengthscale (d,), likelihood parameter"""
    lik, fam, d, n = row
    seed = 40 + 7 * lik + d + n
    x, y = lr.synth(lik, n, d, seed=seed)
    return x, y, inv_lengthscales(d, seed), lik_param(lik)


def fd_slots(d):
    """the gradient slots (0: variance, 1 + f: feature f) the CPU companion differentiates numerically"""
    return list(range(1 + d)) if d < 16 else sorted({0, 7, 8, d - 1})


# B. one Newton step from a given start, d = 3: (lik, family, N); N = 300 / 600 / 129 are 3 / 5 / 2 panels of 128
STEP_ROWS = [(0, SE, 300), (1, M32, 600), (2, M52, 129), (3, SE, 600), (4, M32, 129), (5, M52, 300)]
STEP_D = 3


def step_id(row):
    return "lik%d-fam%d-n%d" % row


def step_problem(row, dtype=np.float64):
    """-> x, y, inv_lengthscale, likelihood parameter, f_init; x, y and f_init rounded to `dtype` (what the device is given).
    f_init = 0.8 sin(3 x_0) + 0.3 z; the probit row also starts some points at sign * f_init < -3 (the hazard's tail branch)."""
    lik, fam, n = row
    seed = 300 + 11 * lik + n
    x, y = lr.synth(lik, n, STEP_D, seed=seed)
    rng = np.random.default_rng(2000 + seed)
    f_init = 0.8 * np.sin(3.0 * x[0]) + 0.3 * rng.standard_normal(n)
    if lik == o.LIK_BERNOULLI_NORMCDF:
        sg = np.where(y > 0.5, 1.0, -1.0)
        tail = np.arange(3, n, 13)
        f_init[tail] = -sg[tail] * (3.1 + 1.4 * rng.uniform(size=tail.size))
    rnd = lambda a: a.astype(dtype).astype(np.float64)
    return rnd(x), rnd(y), inv_lengthscales(STEP_D, seed), lik_param(lik), rnd(f_init)


def step_tolerances(dtype):
    """(lml relative, vectors relative to their own maximum): those of test_maxiter_one_keeps_fnew"""
    return (1e-10, 1e-9) if np.dtype(dtype) == np.float64 else (1e-4, 1e-4)


# C. predictions: Bernoulli-normcdf, Matern-3/2 ARD, N = 300; d = 2 (COLVECS / ROWVECS) and d = 1 from a plain vector (VEC)
PRED_LIK, PRED_FAMILY, PRED_N = 5, M32, 300
PRED_NSTAR = [1, 63, 64, 65, 130]
PRED_CROSS = [(65, 1), (1, 65), (64, 130)]


def pred_problem(d, dtype=np.float64):
    """-> x, y, inv_lengthscale; x and y rounded to `dtype`"""
    x, y = lr.synth(PRED_LIK, PRED_N, d, seed=70 + d)
    rnd = lambda a: a.astype(dtype).astype(np.float64)
    return rnd(x), rnd(y), inv_lengthscales(d, 70 + d)


def pred_points(d, n, seed, dtype=np.float64):
    return np.random.default_rng(500 + seed).uniform(-2.0, 2.0, size=(d, n)).astype(dtype).astype(np.float64)


# D. warm start: N = 200, Bernoulli-logistic, d = 2, SE
WARM_N, WARM_LIK, WARM_FAMILY = 200, 1, SE
WARM_THETA1 = (1.1, np.array([0.8, 1.2]))
WARM_THETA2 = (1.6, np.array([1.0, 0.9]))


def warm_problem(dtype=np.float64):
    x, y = lr.synth(WARM_LIK, WARM_N, 2, seed=17)
    return x.astype(dtype).astype(np.float64), y.astype(dtype).astype(np.float64)
