#!/usr/bin/env python
"""VFE, Vecchia and the exact GP on one synthetic regression problem (N = 20 000, d = 2), with the held-out negative log predictive
density of each.  The exact GP is solved by matrix-free conjugate gradients (ConjugateGradients, svgp_cg_*): K(x, x) is never stored,
so it is the ground truth the two approximations are judged against at a size where the dense exact GP no longer fits the dense
entry points.  Hyperparameters are the generating ones for all three (the Wang et al. 2019 workflow would train them with a sparse
method first).

    python examples/n_exact_gp_cg.py          # needs an MI355X
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
import approxgp as ag  # noqa: E402


def main(N=20_000, n_test=2_000, M=256, k=30, seed=7):
    rng = np.random.default_rng(seed)
    d, noise = 2, 0.05
    x = rng.uniform(-3, 3, size=(d, N + n_test))
    w = rng.standard_normal((64, d)) / 0.7                      # a draw from an SE prior with lengthscale 0.7, by random features
    f_true = np.sqrt(2 * 1.3 / 64) * np.cos(w @ x + rng.uniform(0, 2 * np.pi, 64)[:, None]).T @ rng.standard_normal(64)
    y = f_true + np.sqrt(noise) * rng.standard_normal(N + n_test)
    xtr, ytr, xte, yte = x[:, :N], y[:N], x[:, N:], y[N:]
    kernel = 1.3 * ag.with_lengthscale(ag.SqExponentialKernel(), 0.7)
    f = ag.GP(kernel)
    fx = f(xtr, noise)
    nlpd = {}
    gauss_nlpd = lambda m, v: float(np.mean(0.5 * (np.log(2 * np.pi * (v + noise)) + (yte - m) ** 2 / (v + noise))))

    post = ag.posterior(ag.VFE(f(xtr[:, rng.choice(N, M, replace=False)], 1e-6)), fx, ytr)
    nlpd[f"VFE (M = {M})"] = gauss_nlpd(*post.mean_and_var(xte))

    order = np.lexsort((xtr[1], np.floor(xtr[0] * 4)))          # a coarse space-filling order for the Vecchia conditioning sets
    nn = ag.posterior(ag.NearestNeighbors(k, include_noise=True, neighbors="nearest"), f(xtr[:, order], noise), ytr[order])
    m, v = nn.local_mean_and_var(xte)
    nlpd[f"Vecchia (k = {k})"] = gauss_nlpd(m, v)

    cg = ag.posterior(ag.ConjugateGradients(tol=1e-6, maxiter=1000, n_probes=16), fx, ytr)
    nlpd["exact GP by CG"] = float(-np.mean(cg.log_predictive_density(xte, yte)))
    print(f"exact GP: lml {cg.lml:.1f} (16 probes), {cg.info.iterations} iterations, largest residual {cg.info.max_rel_residual:.1e}, "
          f"kmv products {cg.info.ms_matvec:.0f} ms, vector stage {cg.info.ms_vector:.0f} ms")
    pcg = ag.posterior(ag.ConjugateGradients(tol=1e-6, maxiter=1000, n_probes=16, precond_size=256), fx, ytr)   # the same fit, preconditioned
    nlpd["exact GP by CG, 256-point Nystrom preconditioner"] = float(-np.mean(pcg.log_predictive_density(xte, yte)))
    print(f"preconditioned: lml {pcg.lml:.1f} (16 probes), {pcg.info.iterations} iterations, largest residual {pcg.info.max_rel_residual:.1e}, "
          f"kmv products {pcg.info.ms_matvec:.0f} ms, vector stage and preconditioner {pcg.info.ms_vector:.0f} ms")
    for name, val in nlpd.items():
        print(f"held-out NLPD  {name:50s} {val:8.4f}")
    return nlpd


if __name__ == "__main__":
    main()
