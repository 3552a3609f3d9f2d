"""CPU checks of tests/nn_xgrad_ref.py, the torch restatement the GPU tests of svgp_nn_lml_grad_inputs compare against: its lml is
nn_noise_ref's, its x_bar matches central differences of nn_noise_ref's lml, and the translation and scaling identities hold.
N = 12, k = 4, d = 2, the three families, the window and a random table, both vectors set.  Central differences with h = 1e-5 on
x ~ U(-2, 2) carry a truncation error h^2 and a rounding error eps |lml| / h ~ 2e-10: 1e-7 of the largest entry is allowed."""
import numpy as np
import pytest

import nn_noise_ref as nn
import nn_ref as nr
import nn_sets_ref as ns
import nn_xgrad_ref as nx
import svgp_oracle as o

N, K, D, VAR, DIAG, MC = 12, 4, 2, 1.2, 1e-2, 0.1


@pytest.mark.parametrize("form", ["window", "random"])
@pytest.mark.parametrize("fam", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
def test_restatement_matches_nn_noise_ref_and_the_identities(fam, form):
    x, y = nr.synth(N, D, seed=77)
    s, mu = nn.noise_vector(N, 5), nn.mean_vector(x)
    kern = nr.kernel_of(fam, VAR, nr.invl_for(D, True))
    tab = ns.window_table(N, K) if form == "window" else nn.random_table(N, K, 3)
    lml, xbar = nx.lml_and_xbar(kern, x, y, tab, DIAG, s, mu, MC)
    ref = nn.lml(kern, x, y, tab, DIAG, s, mu, MC)
    assert abs(lml - ref) <= 1e-12 * abs(ref)
    fd, h = np.zeros_like(x), 1e-5
    for f in range(D):
        for j in range(N):
            xp, xm = x.copy(), x.copy()
            xp[f, j] += h
            xm[f, j] -= h
            fd[f, j] = (nn.lml(kern, xp, y, tab, DIAG, s, mu, MC) - nn.lml(kern, xm, y, tab, DIAG, s, mu, MC)) / (2 * h)
    assert np.max(np.abs(xbar - fd)) <= 1e-7 * np.max(np.abs(fd))
    gil = nn.lml_grad(kern, x, y, tab, DIAG, s, mu, MC)[2]
    assert np.max(np.abs(xbar.sum(axis=1))) <= 1e-12 * np.sum(np.abs(xbar))                       # translation
    assert np.max(np.abs((x * xbar).sum(axis=1) - kern.inv_lengthscale * gil)) <= 1e-10 * np.sum(np.abs(x * xbar))   # scaling
