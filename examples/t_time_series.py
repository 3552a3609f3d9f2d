"""An irregularly sampled time series of N = 1e6 points, fitted EXACTLY: a Matern-3/2 GP in state-space form (approxgp.StateSpace),
whose log marginal likelihood costs O(N) on the device.  The three hyperparameters (variance, lengthscale, noise) are fitted by a
derivative-free optimiser (Nelder-Mead over their logarithms: the gradient of the lml is a follow-up), then the posterior is read at
times between, on, before and after the data.

    python examples/t_time_series.py [--n 1000000]"""
import argparse
import os
import sys

import numpy as np
from scipy.optimize import minimize

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "approximategps.jl_amd"))
import approxgp
from approxgp import _ffi
from approxgp.statespace import DeviceStateSpace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--maxiter", type=int, default=60)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    N = a.n
    t = np.cumsum(rng.exponential(0.01, N))                       # irregular sampling, mean gap 0.01
    f = np.sin(0.7 * t) + 0.5 * np.sin(2.9 * t + 1.0)
    y = f + 0.3 * rng.standard_normal(N)
    ctx = _ffi.Context(0)
    dev = DeviceStateSpace(ctx, t, y, np.float64)

    def kernel(p):
        return float(np.exp(p[0])) * approxgp.with_lengthscale(approxgp.Matern32Kernel(), float(np.exp(p[1])))

    def objective(p):
        return -dev.fit(dev.desc(kernel(p), float(np.exp(p[2]))))[0] / N

    res = minimize(objective, np.log([1.0, 0.2, 0.5]), method="Nelder-Mead", options={"maxiter": a.maxiter, "xatol": 1e-3, "fatol": 1e-7})
    var, ell, noise = np.exp(res.x)
    print(f"N = {N}: variance {var:.3f} lengthscale {ell:.3f} noise {noise:.4f} (true 0.09), lml / N {-res.fun:.5f} after {res.nfev} exact evaluations")
    lml, info = dev.fit(dev.desc(kernel(res.x), noise))
    ts = np.concatenate([[t[0] - 1.0], rng.uniform(t[0], t[-1], 1000), t[:3], [t[-1] + 1.0]])
    m, v = dev.predict(ts)
    truth = np.sin(0.7 * ts) + 0.5 * np.sin(2.9 * ts + 1.0)
    inside = slice(1, -1)
    print(f"posterior at {ts.shape[0]} times: RMSE to the noise-free signal {np.sqrt(np.mean((m[inside] - truth[inside]) ** 2)):.4f}, "
          f"mean sd {np.sqrt(v[inside]).mean():.4f}; one fit {info.ms_total:.1f} ms over {info.n_tiles} tiles, {info.levels} scan levels")
    dev.free()
    ctx.close()


if __name__ == "__main__":
    main()
