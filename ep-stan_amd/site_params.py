"""Named parameters of the built-in site models, computed from the sampled coordinates.

The reference saves the draws of arbitrary Stan parameters by name
(`fit.extract(pars=par)[par]`, /root/reference/epstan/method.py:387-392, asked for by
`Worker.tilted(save_samples=...)` / `Master.run(save_last_param=...)`; experiment/fit.py:366 passes
the models' `('alpha', 'beta')`).  The device sampler keeps the unconstrained coordinates
`theta = [phi | eta (groups) | etb (groups x D)]`; this module restates the `parameters` and
`transformed parameters` blocks of experiment/models/m{1..5}{a,b}[_sg].stan on top of them.

Draws come back chain-major (all post-warm-up draws of chain 0, then chain 1, ...), not in
PyStan's random permutation.
"""

import numpy as np

# enum epx_named (include/epx.h)
NAME_IDS = {'phi': 0, 'eta': 1, 'alpha': 2, 'beta': 3, 'sigma_a': 4, 'etb': 5, 'sigma_b': 6, 'mu_a': 7, 'mu_b': 8,
            'sigma': 9}

# sampled blocks behind phi, per b-model id: does the program have the `etb` block?
_HAS_ETB = {0: False, 1: True, 2: True, 3: True, 4: True}


def layout(model_id, D, ng, gauss):
    """Index slices of theta for a site with `ng` groups."""
    o = 1 if gauss else 0
    d = o + {0: D + 1, 1: 2, 2: D + 1, 3: 2 * D + 2, 4: 2 * D + 2}[model_id]
    eta = slice(d, d + ng)
    etb = slice(d + ng, d + ng + ng * D) if _HAS_ETB[model_id] else None
    return o, d, eta, etb


def names(model_id, gauss):
    base = ['phi', 'eta', 'alpha', 'beta', 'sigma_a']
    if _HAS_ETB[model_id]:
        base += ['etb', 'sigma_b']
    if model_id >= 3:
        base += ['mu_a', 'mu_b']
    if gauss:
        base += ['sigma']
    return base


def named_draws(model_id, D, ng, gauss, single_group, theta, wanted):
    """theta: (S, P) draws of all sampled coordinates of one site -> {name: draws}.

    Scalars of a single-group program (`real alpha`) come back as (S,), vectors as (S, D); the
    multi-group programs declare `vector[J] alpha`, `vector[D] beta[J]`: (S, J) and (S, J, D)."""
    theta = np.asarray(theta, dtype=np.float64)
    S = theta.shape[0]
    o, d, sl_eta, sl_etb = layout(model_id, D, ng, gauss)
    phi = theta[:, :d]
    b = phi[:, o:]                                       # the b-model's phi
    eta = theta[:, sl_eta]                               # (S, ng)
    etb = theta[:, sl_etb].reshape(S, ng, D) if sl_etb is not None else None
    val = {'phi': phi, 'eta': eta}
    if gauss:
        val['sigma'] = np.exp(phi[:, 0])
    if model_id == 0:                                    # phi = [log sigma_a, beta]
        sig_a = np.exp(b[:, 0])
        val['alpha'] = eta * sig_a[:, None]
        val['beta'] = b[:, 1:1 + D]                      # `vector[D] beta` is shared by the groups (m1b.stan:27-31)
    elif model_id == 1:                                  # phi = [log sigma_a, log sigma_b]
        sig_a = np.exp(b[:, 0])
        val['sigma_b'] = np.exp(b[:, 1])
        val['alpha'] = eta * sig_a[:, None]
        val['beta'] = etb * val['sigma_b'][:, None, None]
    elif model_id == 2:                                  # phi = [log sigma_a, log sigma_b (D)]
        sig_a = np.exp(b[:, 0])
        val['sigma_b'] = np.exp(b[:, 1:1 + D])
        val['alpha'] = eta * sig_a[:, None]
        val['beta'] = etb * val['sigma_b'][:, None, :]
    else:                                                # phi = [mu_a, log sigma_a, mu_b (D), log sigma_b (D)]
        sig_a = np.exp(b[:, 1])
        val['mu_a'] = b[:, 0]
        val['mu_b'] = b[:, 2:2 + D]
        val['sigma_b'] = np.exp(b[:, 2 + D:2 + 2 * D])
        val['alpha'] = val['mu_a'][:, None] + eta * sig_a[:, None]
        val['beta'] = val['mu_b'][:, None, :] + etb * val['sigma_b'][:, None, :]
    val['sigma_a'] = sig_a
    if etb is not None:
        val['etb'] = etb
    out = {}
    for name in wanted:
        if name not in val:
            raise ValueError("parameter {!r} is not defined by this site model (known: {})"
                             .format(name, sorted(val)))
        v = np.array(val[name])
        if single_group and name in ('eta', 'alpha'):
            v = v[:, 0]
        elif single_group and name in ('etb', 'beta') and v.ndim == 3:
            v = v[:, 0, :]
        out[name] = v
    return out


def named_shape(model_id, D, ng, gauss, single_group, name):
    """Per-site shape of `name` -- the shape `named_draws` returns behind the draw axis."""
    o, d, _, _ = layout(model_id, D, ng, gauss)
    if name not in names(model_id, gauss):
        raise ValueError("parameter {!r} is not defined by this site model (known: {})"
                         .format(name, sorted(names(model_id, gauss))))
    per_group = {'eta': (), 'alpha': (), 'etb': (D,), 'beta': (D,)}
    if name == 'beta' and model_id == 0:
        return (D,)
    if name in per_group:
        return per_group[name] if single_group else (ng,) + per_group[name]
    if name == 'phi':
        return (d,)
    if name == 'mu_b' or (name == 'sigma_b' and model_id != 1):
        return (D,)
    return ()


def named_moments_host(model_id, D, ng, gauss, single_group, theta, wanted):
    """(n, mean, m2) of the named parameters of ONE site from its draws theta (S, P) with NumPy:
    mean[name] and the centred sum of squares m2[name] = sum_s (x_s - mean)^2 in the per-site shapes of
    `named_draws`.  What the device kernel k_named_moments (csrc/named_moments.hip) computes; the
    expectation of its tests, and `Master.mix_pred`'s route on an engine without `named_moments`."""
    draws = named_draws(model_id, D, ng, gauss, single_group, theta, wanted)
    mean, m2 = {}, {}
    for name, x in draws.items():
        mean[name] = x.mean(axis=0)
        m2[name] = np.square(x - mean[name]).sum(axis=0)
    return np.asarray(theta).shape[0], mean, m2


# enum epx_pred (include/epx.h): the columns of a prediction record
PR_MEAN, PR_F_MEAN, PR_F_M2, PR_LPD, PR_COUNT = 0, 1, 2, 3, 4


def linear_predictor(model_id, D, ng, gauss, theta, Xn, group):
    """f (S, n): f_si = alpha_g(s) + x_i . beta_g(s) of the rows Xn (n, D) of ONE site under its draws theta (S, P),
    alpha and beta as `named_draws` forms them.  group (n): 0-based group of every row within the site (None: 0)."""
    theta = np.asarray(theta, dtype=np.float64)
    Xn = np.asarray(Xn, dtype=np.float64).reshape(-1, D)
    n, S = Xn.shape[0], theta.shape[0]
    group = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    if group.shape != (n,) or (n and (group.min() < 0 or group.max() >= ng)):
        raise ValueError("group: one 0-based index below {} per new row".format(ng))
    dr = named_draws(model_id, D, ng, gauss, False, theta, ['alpha', 'beta'])
    alpha, beta = dr['alpha'], dr['beta']                # (S, ng); (S, ng, D), m1: (S, D) shared by the groups
    f = np.empty((S, n))
    for g in np.unique(group):
        rows = np.nonzero(group == g)[0]
        bg = beta if beta.ndim == 2 else beta[:, g, :]
        f[:, rows] = alpha[:, g][:, None] + bg.dot(Xn[rows].T)
    return f


def loglik_of(gauss, theta, f, y):
    """ll (S, n) of the responses y (n) at the linear predictors f (S, n): y f - log(1 + e^f) (Bernoulli-logit models) or
    the log density of normal(f, exp(phi[0])) at y (Gaussian models, theta (S, P) the draws)."""
    y = np.asarray(y, dtype=np.float64)
    if gauss:
        ls = np.asarray(theta, dtype=np.float64)[:, 0][:, None]
        return -0.5 * np.log(2 * np.pi) - ls - 0.5 * np.square((y - f) / np.exp(ls))
    return y * f - (np.maximum(f, 0.0) + np.log1p(np.exp(-np.abs(f))))


def predict_host(model_id, D, ng, gauss, theta, Xn, group, y=None):
    """Posterior predictive of the new rows Xn (n, D) of ONE site from its draws theta (S, P) with NumPy: (n, 4),
    columns PR_MEAN, PR_F_MEAN, PR_F_M2, PR_LPD.  group (n): 0-based group of every row within the site (None: 0).
    With f_si = alpha_g(s) + x_i . beta_g(s), alpha and beta as `named_draws` forms them:
      MEAN  the mean over the draws of sigmoid(f) (Bernoulli-logit models) or of f (Gaussian models);
      F_MEAN, F_M2  the mean of f and the centred sum of squares sum_s (f_si - F_MEAN)^2;
      LPD  log mean_s exp(ll_si), ll = y f - log(1 + e^f) or the log density of normal(f, exp(phi[0])) at y, taken
           about the row's largest ll; NaN without y.
    What the device kernel k_predict (csrc/predict.hip) computes; the expectation of its tests, and `Master.predict`'s
    route on an engine without `predict`."""
    f = linear_predictor(model_id, D, ng, gauss, theta, Xn, group)
    n = f.shape[1]
    out = np.full((n, PR_COUNT), np.nan)
    if n == 0:
        return out
    fm = f.mean(axis=0)
    out[:, PR_F_MEAN] = fm
    out[:, PR_F_M2] = np.square(f - fm).sum(axis=0)
    if gauss:
        out[:, PR_MEAN] = fm
    else:
        e = np.exp(-np.abs(f))
        out[:, PR_MEAN] = np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).mean(axis=0)
    if y is not None:
        ll = loglik_of(gauss, theta, f, y)
        top = ll.max(axis=0)
        out[:, PR_LPD] = top + np.log(np.exp(ll - top).mean(axis=0))
    return out
