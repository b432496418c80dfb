"""Host-only float64 L-BFGS (NumPy alone): the outer loop of ``inference.LinearProbe``, whose value and gradient come from the device.

``minimize(fun, x0)``: ``fun(theta) -> (f, g)`` is injected (float, float64 array of theta's shape).  Two-loop recursion over the
last ``history`` pairs, Armijo backtracking from the unit step.  The iterate the solver HOLDS is the float32-representable point it
hands to ``fun``: ``x_new = fl32(x + t d)`` -- an evaluator that rounds theta to float32 (a device kernel) is then evaluated exactly
where the solver believes it is, and every ``(s, y)`` pair is an exact difference of evaluated points.  A pair is skipped when
``s^T y`` is not safely positive (backtracking alone does not enforce the curvature condition).

It stops with ``status``
  "converged"  max|g| <= tol;
  "precision"  the line search found no decrease within its bounded number of halvings, or the step no longer moves the float32
               point: the evaluator's noise is above what ``tol`` asks for;
  "max_iter"   ``max_iter`` iterations done.
Every loop has a bound: at most ``max_iter`` iterations of at most ``max_ls`` evaluations each.
"""
import numpy as np


class Result:
    """x (float64 array of float32-representable values), f, g, n_iter, n_eval, status, log ([iterations, 4]: f, max|g|, step, evals)"""

    def __init__(self, x, f, g, n_iter, n_eval, status, log):
        self.x, self.f, self.g, self.n_iter, self.n_eval, self.status = x, f, g, n_iter, n_eval, status
        self.log = np.asarray(log, dtype=np.float64).reshape(-1, 4)


def fl32(x):
    """x rounded to float32, held as float64"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def direction(g, pairs):
    """-H g by the two-loop recursion; pairs: [(s, y, 1 / s^T y)], oldest first.  H0 = (s^T y / y^T y) I of the newest pair."""
    q = g.copy()
    alphas = []
    for s, y, rho in reversed(pairs):
        a = rho * s.dot(q)
        alphas.append(a)
        q -= a * y
    if pairs:
        s, y, _ = pairs[-1]
        q *= s.dot(y) / y.dot(y)
    for (s, y, rho), a in zip(pairs, reversed(alphas)):
        q += (a - rho * y.dot(q)) * s
    return -q


def minimize(fun, x0, *, tol=1e-4, max_iter=1000, history=10, c1=1e-4, max_ls=40, curvature_eps=1e-10):
    x = fl32(np.asarray(x0, dtype=np.float64).ravel())
    f, g = fun(x)
    g = np.asarray(g, dtype=np.float64).ravel()
    n_eval, pairs, log = 1, [], []
    status = "max_iter"
    it = 0
    while True:
        gmax = float(np.abs(g).max()) if g.size else 0.0
        if not np.isfinite(f) or not np.isfinite(gmax):
            status = "precision"                    # nothing to descend on
            break
        if gmax <= tol:
            status = "converged"
            break
        if it >= max_iter:
            break
        d = direction(g, pairs)
        slope = g.dot(d)
        if not slope < 0.0:                         # not a descent direction: forget the history, steepest descent
            pairs, d = [], -g
            slope = g.dot(d)
        t = 1.0 if pairs else min(1.0, 1.0 / float(np.sqrt(g.dot(g))))
        found = False
        for _ in range(max_ls):                     # bound: max_ls halvings
            x_new = fl32(x + t * d)
            if np.array_equal(x_new, x):
                break                               # the step is below the float32 spacing of the point
            f_new, g_new = fun(x_new)
            n_eval += 1
            if np.isfinite(f_new) and f_new <= f + c1 * t * slope:
                found = True
                break
            t *= 0.5
        if not found:
            status = "precision"
            break
        g_new = np.asarray(g_new, dtype=np.float64).ravel()
        s, y = x_new - x, g_new - g
        sy = s.dot(y)
        if sy > curvature_eps * np.sqrt(s.dot(s) * y.dot(y)):
            pairs.append((s, y, 1.0 / sy))
            if len(pairs) > history:
                pairs.pop(0)
        x, f, g = x_new, f_new, g_new
        it += 1
        log.append((f, float(np.abs(g).max()), t, n_eval))
    return Result(x, float(f), g, it, n_eval, status, log)
