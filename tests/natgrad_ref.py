"""Float64 numpy restatement of one natural-gradient step on q(u) (svgp_natgrad_step), built on the oracle's posterior, A_and_Kuf,
marginals (which returns sigma: squared here), expected_loglik_grads and whiten.  In whitened coordinates - q(v) = N(m_w, S_w),
Lambda = inv(S_w) - with A = Lk \\ Kuf over the batch, g_mu = dE/dmu, g_v = dE/dv at the marginals of the current q and
scale = num_data / batch_len:
    W = A diag(-2 scale g_v) A',  a = scale A g_mu
    Lambda'      = (1 - gamma) Lambda     + gamma (I + W)
    Lambda' m_w' = (1 - gamma) Lambda m_w + gamma (a + W m_w)
    S_w'         = inv(Lambda')
i.e. theta' = theta + gamma dL/d eta for theta = (Lambda m_w, -Lambda / 2), eta = (m_w, S_w + m_w m_w') (tests/test_natgrad_cpu.py pins
this to central differences of the oracle's ELBO).  The new q goes back to the SVA's own parametrisation: NonCentered m = m_w',
Lq = chol(S_w'); Centered m = mean_const + Lk m_w', Lq = Lk chol(S_w')."""
import numpy as np
import scipy.linalg as sla

import svgp_oracle as o


def whitened(sva: o.SVA, post: o.Posterior = None):
    """-> (m_w, S_w, Lk) of the SVA's q."""
    post = post or o.posterior(sva)
    if not sva.centered:
        return np.asarray(sva.m, dtype=np.float64), sva.Lq @ sva.Lq.T, post.Lk
    m_w, S_w = o.whiten(sva.kernel, sva.z, sva.jitter, np.asarray(sva.m, dtype=np.float64), sva.Lq @ sva.Lq.T, sva.mean_const)
    return m_w, S_w, post.Lk


def point_grads(sva: o.SVA, x, y, lik, sigma2=1.0, quadrature_n=0):
    """-> (A, g_mu, g_v) at the marginals of the SVA's q (unscaled)."""
    post = o.posterior(sva)
    A, _ = o.A_and_Kuf(post, x)
    mu, sd = o.marginals(post, x)
    gmu, gv, _ = o.expected_loglik_grads(lik, mu, sd * sd, np.asarray(y, dtype=np.float64), sigma2, quadrature_n)
    return A, gmu, gv


def step_whitened(m_w, S_w, A, gmu, gv, scale, gamma):
    """-> (m_w', S_w') from the whitened q and the point gradients."""
    M = m_w.shape[0]
    W = (A * (-2.0 * scale * gv)) @ A.T
    W = 0.5 * (W + W.T)
    a = scale * (A @ gmu)
    if gamma == 1.0:
        Lam_new = np.eye(M) + W
        rhs = a + W @ m_w
    else:
        Ls = np.linalg.cholesky(S_w)
        Linv = sla.solve_triangular(Ls, np.eye(M), lower=True)
        Lam = Linv.T @ Linv
        Lam_new = (1.0 - gamma) * Lam + gamma * (np.eye(M) + W)
        rhs = (1.0 - gamma) * (Lam @ m_w) + gamma * (a + W @ m_w)
    Ln = np.linalg.cholesky(0.5 * (Lam_new + Lam_new.T))
    m_new = sla.cho_solve((Ln, True), rhs)
    Lninv = sla.solve_triangular(Ln, np.eye(M), lower=True)
    S_new = Lninv.T @ Lninv
    return m_new, 0.5 * (S_new + S_new.T)


def step(sva: o.SVA, x, y, lik=o.LIK_GAUSSIAN, sigma2=1.0, num_data=None, gamma=1.0, quadrature_n=0, point_grads_ext=None):
    """One step -> the new oracle SVA (same kernel, z, parametrisation).  point_grads_ext = (g_mu, g_v): the caller's point gradients."""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    n = x.shape[1]
    scale = (float(num_data) if num_data is not None else float(n)) / n
    post = o.posterior(sva)
    m_w, S_w, Lk = whitened(sva, post)
    if point_grads_ext is None:
        A, gmu, gv = point_grads(sva, x, y, lik, sigma2, quadrature_n)
    else:
        A, _ = o.A_and_Kuf(post, x)
        gmu, gv = (np.asarray(g, dtype=np.float64) for g in point_grads_ext)
    m_new, S_new = step_whitened(m_w, S_w, A, gmu, gv, scale, gamma)
    Lq_w = np.linalg.cholesky(S_new)
    if sva.centered:
        m, Lq = sva.mean_const + Lk @ m_new, Lk @ Lq_w
    else:
        m, Lq = m_new, Lq_w
    return o.SVA(sva.kernel, sva.z, m, Lq, jitter=sva.jitter, mean_const=sva.mean_const, centered=sva.centered)


def problem(n, M, d, lik=o.LIK_GAUSSIAN, seed=0, family=o.KERNEL_SE, ard=False, dtype=np.float64, mean_const=0.0):
    """A seeded problem for any likelihood: collapsed_ref.problem's (kernel, z, x, y, sigma2) with y turned into labels (Bernoulli) or
    counts (Poisson) of the same latent function, and a starting q that is neither the prior nor diagonal: -> (kernel, z, x, y, sigma2,
    m0, Lq0), float64 values rounded through `dtype`."""
    import collapsed_ref as cr

    kernel, z, x, y, s2 = cr.problem(n, M, d, seed=seed, family=family, ard=ard, dtype=dtype, mean_const=mean_const)
    rng = np.random.default_rng(977 * seed + 5 * n + M + 11 * d)
    if lik in (o.LIK_BERNOULLI_LOGISTIC, o.LIK_BERNOULLI_NORMCDF):
        y = (y - mean_const + 0.3 * rng.standard_normal(n) > 0).astype(np.float64)
    elif lik == o.LIK_POISSON_EXP:
        y = rng.poisson(np.exp(np.clip(y - mean_const, -3.0, 3.0))).astype(np.float64)
    rd = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
    m0 = rd(0.3 * rng.standard_normal(M))
    Lq0 = np.tril(0.1 * rng.standard_normal((M, M)) / np.sqrt(M), -1) + np.diag(0.6 + 0.5 * rng.random(M))
    return kernel, z, x, rd(y), s2, m0, rd(Lq0)


def start_sva(kernel, z, jitter, m0, Lq0, mean_const=0.0, centered=False):
    """The oracle SVA whose WHITENED q is (m0, Lq0 Lq0'), in the asked parametrisation."""
    if not centered:
        return o.SVA(kernel, z, m0, Lq0, jitter=jitter, mean_const=mean_const, centered=False)
    zz = o._as_dn(np.asarray(z, dtype=np.float64))
    Lk = np.linalg.cholesky(o.kernelmatrix(kernel, zz) + jitter * np.eye(zz.shape[1]))
    return o.SVA(kernel, z, mean_const + Lk @ m0, Lk @ Lq0, jitter=jitter, mean_const=mean_const, centered=True)
