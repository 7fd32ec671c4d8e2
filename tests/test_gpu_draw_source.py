"""A refused call of an entry over draws leaves the context as it was.  Needs a real MI355X.

Every refusal of these entries now stands in front of the first queued copy (csrc/epx_draws.h states the order), so no
argument reaches the exits behind it, which synchronise the stream: those are left to failures of the runtime.  What can be
pinned from outside: calls refused as late as an entry refuses -- the draw source resolved, the row laid out -- change
nothing for the good calls that follow on the same context, which return the bits of a fresh context."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib                                                    # noqa: E402
from epstan_amd.engine import HipEngine                                        # noqa: E402
from test_gpu_parity import _site_problem                                      # noqa: E402
from test_quantiles_host import bits                                           # noqa: E402


def _good_calls(eng, theta, Xn):
    K = theta.shape[0]
    n, mean, m2 = eng.named_moments(['phi', 'alpha', 'beta'], theta=theta)
    stats = eng.named_order_stats(['phi', 'beta'], [0, 7, 39], theta=theta)
    hist, n_nan, _ = eng.pooled_count_pass(['phi'], 56, None, 2, theta=theta)
    arrays = [rec[name] for recs in (mean, m2, stats) for rec in recs for name in sorted(rec)]
    arrays += [hist, n_nan, eng.predict(Xn, np.arange(K + 1) * (Xn.shape[0] // K), theta=theta), eng.loo(theta=theta),
               eng.draw_diagnostics(theta=theta, chains=4)]
    arrays += [a for a in eng.pooled_moments(theta=theta)[1:]]
    return [bits(np.asarray(a, dtype=np.float64)).tolist() if np.asarray(a).dtype.kind == 'f' else np.asarray(a).tolist()
            for a in arrays]


def test_refused_calls_leave_the_context_as_it_was():
    D, K, S = 3, 2, 40
    X, y, k_lim, _, _, d, P = _site_problem('m4b_sg', D, 7, 31, K=K)
    rng = np.random.RandomState(3)
    theta, Xn = 0.5 * rng.randn(K, S, P) + 0.2, rng.randn(6, D)
    fresh = HipEngine('m4b_sg', X, y, k_lim)
    want = _good_calls(fresh, theta, Xn)
    fresh.close()
    eng = HipEngine('m4b_sg', X, y, k_lim)
    with pytest.raises(_lib.EpxError, match=r'rank 40 outside \[0, 40\)'):
        eng.named_order_stats(['phi'], [3, 40], theta=theta)
    with pytest.raises(_lib.EpxError, match='not defined'):
        eng.named_moments(['phi', 'sigma'], theta=theta)
    with pytest.raises(_lib.EpxError, match='no multiple of chains'):
        eng.draw_diagnostics(theta=theta, chains=3)
    with pytest.raises(_lib.EpxError, match='group 1 outside the 1 group'):
        eng.predict(Xn, [0, 3, 6], row_group=np.array([0, 0, 1, 0, 0, 0]), theta=theta)
    with pytest.raises(_lib.EpxError, match='no draws yet'):
        eng.loo()
    with pytest.raises(_lib.EpxError, match='no draws yet'):
        eng.pooled_count_pass(['phi'], 56, None, 2)
    with pytest.raises(_lib.EpxError, match='S = 0 draws'):
        eng.pooled_moments(theta=np.zeros((K, 0, P)))
    assert _good_calls(eng, theta, Xn) == want
    eng.close()
