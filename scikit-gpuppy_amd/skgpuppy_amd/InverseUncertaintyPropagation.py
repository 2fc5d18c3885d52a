"""Inverse uncertainty propagation -- host-side mirror of skgpuppy/InverseUncertaintyPropagation.py ("next" row f2).

Pure callers of the propagation classes: which input variances v_i give a target output variance at minimal
sampling cost  sum_i c_i / (v_i I_ii).  The analytic solver needs d values of `_get_variance_dv_h` and one
`_getFactor` at the same u -- on this backend all of them come out of ONE pass over K^-1 kept in HBM (the u-cache
of libgpx); the numerical solver drives COBYLA with repeated `propagate_GA` calls, each O(d^2) host work plus one
tiny device launch once u is cached.
"""
import numpy as np

from .UncertaintyPropagation import UncertaintyPropagationApprox, UncertaintyPropagationExact


class InverseUncertaintyPropagation(object):
    """Base class (InverseUncertaintyPropagation.py:13-52): stores the problem."""

    def __init__(self, output_variance, gp, u, c, I, input_variances=None, upga_class=UncertaintyPropagationExact,
                 coestimated=[]):
        self.coestimated = coestimated
        self.gp = gp
        self.upga_class = upga_class
        self.u = u
        self.output_variance = output_variance
        self.c = c
        self.I = I

    def get_best_solution(self):
        pass


def _followers(coestimated):
    """indices tied to the first member of their co-estimation group (v_i = v_lead I_lead / I_i)."""
    return [(group[0], i) for group in coestimated for i in group if i != group[0]]


def _reduced(c, I, coestimated):
    """(c, I, free) of the free variances: the followers of every co-estimation group removed (the successive np.delete of
    InverseUncertaintyPropagationNumerical.get_best_solution, which is the reference's)"""
    c, I = np.asarray(c, dtype=float), np.asarray(I, dtype=float)
    free = np.array(list(range(len(c))))
    for _lead, i in _followers(coestimated):
        I = np.delete(I, i)
        c = np.delete(c, i)
        free = np.delete(free, i)
    return c, I, free


def slsqp_inverse(value_and_grad, output_variance, c, I, coestimated=[], start=None, acc=1e-8, maxiter=200):
    """The gradient-based form of InverseUncertaintyPropagationNumerical.get_best_solution: minimise the cost sum_k c_k / (v_k I_k) over the
    free LOG-variances x_k = log v_k under output_variance - var(v) >= 0, by SLSQP with analytic Jacobians.

    value_and_grad(v_full [d]) -> (var, dvar_dv [d]): the output variance at the input variances v_full and its derivative in each of them
    (UncertaintyPropagationExact.propagate_GA_gradient gives both; any model of them serves, so the driver runs without a device).
    The chain rule runs through exp (dv_k / dx_k = v_k) and through the co-estimated followers: v_i = v_lead I_lead / I_i moves with its
    lead, so dvar_dv_i v_i adds to the lead's derivative.  Cost Jacobian: -c_k / (v_k I_k).  start: the free log-variances (default -10
    each, the COBYLA path's).  Returns (v_full [d], info) with info = {"x": the free log-variances, "free": their indices, "calls": the
    number of value_and_grad evaluations, "result": scipy's OptimizeResult}."""
    from scipy.optimize import minimize
    c_full, I_full = np.asarray(c, dtype=float), np.asarray(I, dtype=float)
    followers = _followers(coestimated)
    cr, Ir, free = _reduced(c_full, I_full, coestimated)
    pos = dict((int(m), k) for k, m in enumerate(free))

    def expand(x):
        v = np.zeros(len(c_full))
        v[free] = np.exp(x)
        for lead, i in followers:
            v[i] = v[lead] * I_full[lead] / I_full[i]
        return v

    memo = {"key": None, "calls": 0}

    def evaluate(x):          # SLSQP asks for the constraint and for its Jacobian at the same x: one propagation serves both
        key = np.asarray(x, dtype=float).tobytes()
        if memo["key"] != key:
            v = expand(x)
            var, dv = value_and_grad(v)
            dv = np.asarray(dv, dtype=float)
            g = np.array([dv[m] * v[m] for m in free])
            for lead, i in followers:
                g[pos[lead]] += dv[i] * v[i]
            memo.update(key=key, var=float(var), g=g, calls=memo["calls"] + 1)
        return memo["var"], memo["g"]

    cost = lambda x: np.sum(cr / np.exp(x) / Ir)          # noqa: E731
    cost_jac = lambda x: -cr / np.exp(x) / Ir             # noqa: E731
    cons = {"type": "ineq", "fun": lambda x: output_variance - evaluate(x)[0], "jac": lambda x: -evaluate(x)[1]}
    x0 = np.ones(len(cr)) * -10 if start is None else np.asarray(start, dtype=float)
    res = minimize(cost, x0, jac=cost_jac, constraints=[cons], method="SLSQP", options={"ftol": acc, "maxiter": maxiter})
    return expand(res.x), {"x": res.x, "free": free, "calls": memo["calls"], "result": res}


class InverseUncertaintyPropagationNumerical(InverseUncertaintyPropagation):
    """COBYLA on log-variances with the constraint output_variance - propagate_GA(u, diag(v))[1] >= 0
    (InverseUncertaintyPropagation.py:55-117); method="slsqp": the same cost under the same constraint by SLSQP on the closed-form
    gradient of the propagated variance (slsqp_inverse), for a upga_class that has propagate_GA_gradient."""

    def _best_solution_slsqp(self, startvalue):
        if not hasattr(self.upga_class, "propagate_GA_gradient"):
            raise TypeError("method='slsqp' needs a upga_class with propagate_GA_gradient; %s has none" % self.upga_class.__name__)
        upga = self.upga_class(self.gp)

        def value_and_grad(v):
            out = upga.propagate_GA_gradient(self.u, np.diag(v))
            return out[1], out[5]

        v, info = slsqp_inverse(value_and_grad, self.output_variance, self.c, self.I, self.coestimated, startvalue)
        assert (v > 0).all()
        self.slsqp_info = info
        return v

    def get_best_solution(self, startvalue=None, method="cobyla"):
        if method == "slsqp":
            return self._best_solution_slsqp(startvalue)
        if method != "cobyla":
            raise ValueError("method must be 'cobyla' or 'slsqp', got %r" % (method,))
        from scipy.optimize import fmin_cobyla
        c_full = np.asarray(self.c, dtype=float)
        I_full = np.asarray(self.I, dtype=float)
        c, I = c_full, I_full
        free = np.array(list(range(len(c_full))))
        for _lead, i in _followers(self.coestimated):      # same successive np.delete semantics as the reference
            I = np.delete(I, i)
            c = np.delete(c, i)
            free = np.delete(free, i)
        upga = self.upga_class(self.gp)

        def expand_log(vx):
            full = np.zeros(len(c_full))
            for k, m in enumerate(free):
                full[m] = vx[k]
            for lead, i in _followers(self.coestimated):
                full[i] = np.log(np.exp(full[lead]) * I_full[lead] / I_full[i])
            return full

        def constraint(vx):
            return self.output_variance - upga.propagate_GA(self.u, np.diag(np.exp(expand_log(vx))))[1]

        cost = lambda vx: np.sum(c / np.exp(vx) / I)      # noqa: E731
        start = np.ones(len(c)) * -10 if startvalue is None else startvalue
        vx_min = np.exp(fmin_cobyla(cost, start, [constraint]))
        assert (vx_min > 0).all()
        out = np.zeros(len(c_full))
        for k, m in enumerate(free):
            out[m] = vx_min[k]
        for lead, i in _followers(self.coestimated):
            out[i] = out[lead] * I_full[lead] / I_full[i]
        return out


class InverseUncertaintyPropagationApprox(InverseUncertaintyPropagation):
    """Closed form under the approximate propagation (InverseUncertaintyPropagation.py:121-173): weights
    sqrt(c_i / (dv/dv_i I_ii)), scaled by `_getFactor` to hit the target variance."""

    def __init__(self, output_variance, gp, u, c, I, input_variances=None, coestimated=[]):
        InverseUncertaintyPropagation.__init__(self, output_variance, gp, u, c, I, input_variances=input_variances,
                                               coestimated=coestimated, upga_class=UncertaintyPropagationApprox)

    def get_best_solution(self):
        d = len(self.u)
        I = np.asarray(self.I, dtype=float)
        upga = self.upga_class(self.gp)
        dvdv = np.array([upga._get_variance_dv_h(self.u, h) for h in range(d)])
        for lead, i in _followers(self.coestimated):
            dvdv[lead] += dvdv[i] * I[lead] / I[i]
        weights = np.sqrt(np.asarray(self.c, dtype=float) / dvdv / I)
        for lead, i in _followers(self.coestimated):
            weights[i] = weights[lead] * I[lead] / I[i]
        assert (weights > 0).all()
        factor = upga._getFactor(self.u, np.diag(weights), self.output_variance)
        optimum = factor * weights
        assert (optimum > 0).all()
        return optimum

    # ---- many operating points in one call (no reference counterpart: what a caller's loop over get_best_solution computes) ----
    @staticmethod
    def _closed_form(dvh, sigma2, c, I, coestimated, output_variance):
        """The steps of get_best_solution (InverseUncertaintyPropagation.py:139-173) for B operating points at once: dvh [B, d] (the d
        values of _get_variance_dv_h per point), sigma2 and output_variance [B] or scalar; returns the optimal input variances [B, d].
        `_getFactor` needs no propagation of its own: with Sigma = diag(w) the variance rest is sum_k w_k dvh_k (unfolded dvh).

        Unlike get_best_solution, which asserts, an infeasible point does not stop the batch: a row with a folded derivative <= 0, a
        weight that is not finite and positive, or a factor that is not positive (target variance at or below sigma2) comes back as a
        row of NaN, silently; the other rows are unaffected."""
        dvh = np.asarray(dvh, dtype=float)
        if dvh.ndim != 2:
            raise ValueError("dvh must be (B, d), got %s" % (dvh.shape,))
        B, d = dvh.shape
        c = np.asarray(c, dtype=float)
        I = np.asarray(I, dtype=float)
        if c.shape != (d,) or I.shape != (d,):
            raise ValueError("c and I must be (%d,), got %s and %s" % (d, c.shape, I.shape))
        sigma2 = np.broadcast_to(np.asarray(sigma2, dtype=float), (B,))
        target = np.broadcast_to(np.asarray(output_variance, dtype=float), (B,))
        followers = _followers(coestimated)
        dd = dvh.copy()
        with np.errstate(all="ignore"):
            for lead, i in followers:
                dd[:, lead] += dd[:, i] * I[lead] / I[i]
            weights = np.sqrt(c / dd / I)
            for lead, i in followers:
                weights[:, i] = weights[:, lead] * I[lead] / I[i]
            rest = np.zeros(B)
            for k in range(d):                               # fixed order: a row's result does not depend on the batch
                rest += weights[:, k] * dvh[:, k]
            factor = (target - sigma2) / rest
            optimum = factor[:, None] * weights
            good = (np.isfinite(weights) & (weights > 0)).all(axis=1) & np.isfinite(factor) & (factor > 0)
        optimum[~good] = np.nan
        return optimum

    def get_best_solution_many(self, U, output_variance=None):
        """get_best_solution for the rows of U (B, d) in one call: optimal input variances [B, d], NaN rows where the problem has no
        solution (_closed_form).  output_variance: [B] or scalar, default self.output_variance.  self.u is not used.
        On a PseudoInputGP (GaussianProcess.pseudo_gp()) the derivatives come from a loop over the single-input device call, one point
        after the other: the batched inverse propagation has no K^-1 form yet."""
        upga = self.upga_class(self.gp)
        dvh, sigma2 = upga._get_variance_dv_many(U)
        target = self.output_variance if output_variance is None else output_variance
        return self._closed_form(dvh, sigma2, self.c, self.I, self.coestimated, target)
