"""CPU companion of tests/test_gpu_laplace_edges.py: the committed proof that the inputs of tests/laplace_edge_cases.py are fit for
the tolerances the GPU tests assert.  At every row the reference's closed-form gradient agrees with central differences of its
own lml to a tenth of the GPU tolerance, and its one-step Newton result moves by less than a quarter of the fp64 tolerance when
x moves by one ulp - so a device result outside the tolerance is the device's error, not the problem's conditioning."""
import numpy as np
import pytest

import laplace_edge_cases as ec
import laplace_ref as lr
import svgp_oracle as o


@pytest.mark.parametrize("row", ec.GRAD_ROWS, ids=ec.grad_id)
def test_gradient_rows_agree_with_central_differences(row):
    lik, fam, d, n = row
    x, y, il, s2 = ec.grad_problem(row)
    _, dv, dil = lr.lml_grad(lr.kernel_of(fam, ec.VARIANCE, il), x, y, lik, s2, jitter=ec.JITTER, maxiter=ec.GRAD_MAXITER)
    g = np.concatenate([[dv], dil])
    scale = np.max(np.abs(g))
    assert scale > 0.0 and np.all(np.isfinite(g))

    def lml(slot, h):
        v, l = ec.VARIANCE, il.copy()
        if slot == 0:
            v += h
        else:
            l[slot - 1] += h
        return lr.fit(lr.kernel_of(fam, v, l), x, y, lik, s2, jitter=ec.JITTER, maxiter=ec.GRAD_MAXITER)[0]

    h = 1e-5
    for slot in ec.fd_slots(d):
        fd = (lml(slot, h) - lml(slot, -h)) / (2 * h)
        assert abs(g[slot] - fd) <= 1e-7 * scale, (slot, g[slot], fd, abs(g[slot] - fd) / scale)
    if n == 1:   # one point: K = variance + jitter whatever the lengthscales are
        assert np.all(dil == 0.0) and dv != 0.0
    else:        # K is neither the identity nor constant: the off-diagonal pairs carry the gradient
        K = o.kernelmatrix(lr.kernel_of(fam, ec.VARIANCE, il), x)
        off = np.max(K - np.diag(np.diag(K)))
        assert 0.2 <= off <= ec.VARIANCE, off


def test_gradient_table_reaches_every_chunk_count():
    """the table is what the issue enumerates: 1, 2, 3 and 8 feature chunks of 8, a partly filled last chunk, N on both sides of
    the 64-tile and the 128-panel, and the ROWVECS rerun is one of its rows"""
    chunks = {(d + 7) // 8 for _, _, d, _ in ec.GRAD_ROWS}
    assert {1, 2, 3, 8} <= chunks
    assert any(d % 8 == 1 for _, _, d, _ in ec.GRAD_ROWS)
    assert {1, 64, 65, 130, 150} <= {n for _, _, _, n in ec.GRAD_ROWS}
    assert ec.GRAD_ROWVECS_ROW in ec.GRAD_ROWS and ec.GRAD_ROWVECS_ROW[2] in (9, 17)
    assert sorted(r[0] for r in ec.STEP_ROWS) == [0, 1, 2, 3, 4, 5]
    assert {-(-r[2] // 128) for r in ec.STEP_ROWS} == {2, 3, 5}


@pytest.mark.parametrize("row", ec.STEP_ROWS, ids=ec.step_id)
def test_one_step_result_is_insensitive_to_one_ulp_of_x(row):
    lik, fam, n = row
    x, y, il, s2, f_init = ec.step_problem(row)
    k = lr.kernel_of(fam, ec.VARIANCE, il)
    ref, c, it, conv = lr.fit(k, x, y, lik, s2, jitter=ec.JITTER, f_init=f_init, maxiter=1)
    per, cp, _, _ = lr.fit(k, x * (1.0 + np.finfo(np.float64).eps), y, lik, s2, jitter=ec.JITTER, f_init=f_init, maxiter=1)
    assert it == 1 and not conv
    tol_lml, tol_vec = ec.step_tolerances(np.float64)
    assert abs(per - ref) <= 0.25 * tol_lml * abs(ref), (per, ref)
    for name in ("f", "g", "W"):
        top = np.max(np.abs(c[name]))
        assert top > 0.0
        assert np.max(np.abs(cp[name] - c[name])) <= 0.25 * tol_vec * top, name
    if lik == o.LIK_BERNOULLI_NORMCDF:   # the start reaches the hazard ratio's tail branch
        sg = np.where(y > 0.5, 1.0, -1.0)
        assert np.sum(sg * f_init < -3.0) >= 10


def test_step_inputs_survive_float32_rounding():
    """the fp32 device is given float32 x, y and f_init: the reference on those rounded inputs is what it is compared with, and
    rounding them moves the one-step lml by far less than the fp32 tolerance"""
    for row in ec.STEP_ROWS:
        lik, fam, n = row
        vals = []
        for dt in (np.float64, np.float32):
            x, y, il, s2, f_init = ec.step_problem(row, dt)
            vals.append(lr.fit(lr.kernel_of(fam, ec.VARIANCE, il), x, y, lik, s2, jitter=ec.JITTER, f_init=f_init, maxiter=1)[0])
        assert abs(vals[1] - vals[0]) <= 0.25 * ec.step_tolerances(np.float32)[0] * abs(vals[0]), (row, vals)


def test_one_rounding_models_are_small_perturbations():
    """the fp32 forward-error models of laplace_ref (every stored operand rounded once to float32) stay within a few float32 ulps
    times the problem's condition of the unrounded closed forms - and are not identical to them"""
    row = ec.GRAD_ROWS[1]
    lik, fam, d, n = row
    x, y, il, s2 = ec.grad_problem(row)
    k = lr.kernel_of(fam, ec.VARIANCE, il)
    _, dv, dil = lr.lml_grad(k, x, y, lik, s2, jitter=ec.JITTER, maxiter=ec.GRAD_MAXITER)
    _, mv, mil = lr.lml_grad(k, x, y, lik, s2, jitter=ec.JITTER, maxiter=ec.GRAD_MAXITER, one_rounding=True)
    g, m = np.concatenate([[dv], dil]), np.concatenate([[mv], mil])
    err = np.max(np.abs(g - m)) / np.max(np.abs(g))
    assert 0.0 < err <= 1e-4, err
    x, y, il = ec.pred_problem(2)
    k = lr.kernel_of(ec.PRED_FAMILY, ec.VARIANCE, il)
    _, cache, _, _ = lr.fit(k, x, y, ec.PRED_LIK, jitter=ec.JITTER)
    xs = ec.pred_points(2, 65, 0)
    exact, model = lr.predict(cache, k, x, xs), lr.predict(cache, k, x, xs, one_rounding=True)
    for e, m in zip(exact, model):
        assert 0.0 < np.max(np.abs(e - m)) <= 1e-5


def test_whole_pipeline_one_rounding_model_of_the_mean():
    """lr.fit_one_rounding follows fit()'s float32-stop path, and its predictive mean differs from the exact one by the few
    1e-6 that a cancelling sum of a float32 mode's g has to: the yardstick of the fp32 d = 1, n* = 1 case on the device"""
    x, y, il = ec.pred_problem(1, np.float32)
    k = lr.kernel_of(ec.PRED_FAMILY, ec.VARIANCE, il)
    _, cache, it, _ = lr.fit(k, x, y, ec.PRED_LIK, jitter=ec.JITTER, eps=np.finfo(np.float32).eps)
    model, it_model = lr.fit_one_rounding(k, x, y, ec.PRED_LIK, jitter=ec.JITTER)
    assert it_model == it
    assert 0.0 < np.max(np.abs(model["f"] - cache["f"])) <= 1e-6 * np.max(np.abs(cache["f"]))
    xs = ec.pred_points(1, 1, 1, np.float32)
    exact = lr.predict(cache, k, x, xs)[0]
    err = np.max(np.abs(lr.predict(model, k, x, xs, one_rounding=True)[0] - exact)) / np.max(np.abs(exact))
    assert 1e-6 <= err <= 1e-4 / 8.0, err
