"""The resident samplers (csrc/nuts.hip k_nuts and k_nuts_spec, csrc/nuts_duo.hip; csrc/nuts_gradient.inc,
csrc/nuts_gradient_groups.inc) at the edges of their LDS homes, columns and rows (resident_edge_cases.py: the table,
checked without a device by test_resident_edge_cases.py, which holds every case's kernel against the library's planning).

  H  a site one row below and one at every row count where the planner moves the cavity precision, the tree stack or the
     bookkeeping records out of LDS or serves another layout: the gradient on all of them, transitions across the row
     counts where the stack's home changes;
  I  one gradient case per reachable instantiation no earlier test compares with a reference, one transition case per
     kernel family;
  C  both sides of every DP switch, one padding column, P in 63 .. 66 and d in 62 .. 66;
  R  1, 63, 64, 65 rows (layout 1), 1, 255, 256, 257 (layouts 2, 6), a one-row site beside the largest a layout holds, and
     78 factors of exactly 2 in a lane's product;
  N  a site's bits unchanged when its neighbour's rows are multiplied by 1e300, and when they are NaN.

The bounds are the ones the existing tests of the same hooks use:
  * epx_logdensity_grad_layout: test_logdensity_gradient_at_saturated_logits's, per served layout -- log density
    lp_tol max(1, |lp|), gradient rtol = g_tol, atol = g_tol max(1, max |g|);
  * epx_nuts_transitions: test_layout_ends_trees_as_the_oracle_does's -- leapfrogs, gradients, divergences and mean depth
    equal, every draw 1e-6 relative to max(1, |ref|), the accept statistic 1e-9 + 1e-9 |ref|, for nt = 1, 2, 3;
  * every call made twice: the same bits; a layout other than the one the table claims: an error."""

import numpy as np
import pytest

import resident_edge_cases as rc
from test_gpu_parity import _engine_with_cavity, _group_engine

pytestmark = pytest.mark.gpu

# test_logdensity_gradient_at_saturated_logits: (lp_tol, g_tol) by served layout
TOL = {1: (1e-11, 1e-10), 2: (1e-11, 1e-10), 5: (1e-11, 1e-10), 6: (1e-11, 1e-10), 7: (1e-9, 1e-9), 3: (1e-10, 1e-9), 4: (1e-10, 1e-9)}

_engines = {}


def _engine(case):
    """(problem, engine, the cavities the device holds); the last few are kept for the tests that share a shape."""
    if case.shape not in _engines:
        while len(_engines) >= 4:
            _engines.pop(next(iter(_engines)))
        p = rc.problem(case)
        if case.multi:
            eng, Om, mu = _group_engine(case.model, p['X'], p['y'], p['k_lim'], p['g_cnt'], p['g_lim'], p['Oms'], p['mus'])
        else:
            eng, Om, mu = _engine_with_cavity(case.model, p['X'], p['y'], p['k_lim'], p['Oms'], p['mus'])
        assert eng.P == case.P and eng.d == case.d
        _engines[case.shape] = (p, eng, Om, mu)
    return _engines[case.shape]


def _check_gradient(case, p, eng, Om, mu):
    lp_tol, g_tol = TOL[case.served]
    worst = [0.0, 0.0]
    for k in range(case.K):
        for th in rc.thetas(case, p, k):
            lp, g = eng.logdensity_grad(k, th, layout=case.req)
            assert eng.last_layout() == case.served, (case.id, case.req, eng.last_layout())
            lp2, g2 = eng.logdensity_grad(k, th, layout=case.req)
            assert lp2 == lp and np.array_equal(g2, g), (case.id, k)                  # (the same call again: the same bits)
            lp_o, g_o = rc.oracle_gradient(case, p, k, th, Om, mu)
            assert np.isfinite(lp_o) and np.all(np.isfinite(g_o))
            gmax = max(1.0, np.abs(g_o).max())
            m_lp = abs(lp - lp_o) / (lp_tol * max(1.0, abs(lp_o)))
            m_g = (np.abs(g - g_o) / (g_tol * gmax + g_tol * np.abs(g_o))).max()
            print('%s site %d theta %s: lp %.17g oracle %.17g, %.3e of its bound; gradient %.3e of its bound'
                  % (case.id, k, 'zero' if not th.any() else 'random', lp, lp_o, m_lp, m_g))
            assert np.isfinite(lp) and np.all(np.isfinite(g)), (case.id, k, lp)
            assert abs(lp - lp_o) <= lp_tol * max(1.0, abs(lp_o)), (case.id, k, lp, lp_o)
            np.testing.assert_allclose(g, g_o, rtol=g_tol, atol=g_tol * gmax)
            worst = [max(worst[0], m_lp), max(worst[1], m_g)]
    print('MARGIN %s %s (%s, layout %d): gradient hook, lp %.3e grad %.3e of the bounds'
          % (case.part, case.id, case.claim[0], case.served, worst[0], worst[1]))


@pytest.mark.parametrize('case', rc.cases(check='grad'), ids=repr)
def test_gradient_matches_oracle(case):
    p, eng, Om, mu = _engine(case)
    _check_gradient(case, p, eng, Om, mu)


@pytest.mark.parametrize('case', rc.cases(check='trans'), ids=repr)
def test_transitions_follow_the_oracle(case):
    p, eng, Om, mu = _engine(case)
    runs = rc.oracle_transitions(case, p, Om, mu)
    dev = {}
    for nt in (1, 2, 3, 3):
        o, st = eng.nuts_transitions(p['seeds'], p['q0'], p['eps'], p['inv_e'], nt=nt, t_offset=rc.T_OFFSET, layout=case.req)
        assert eng.last_layout() == case.served, (case.id, case.req, eng.last_layout())
        if nt in dev:
            np.testing.assert_array_equal(o, dev[nt][0])                              # (the same launch again: the same bits)
            np.testing.assert_array_equal(st, dev[nt][1])
        dev[nt] = (o, st)
    worst_draw = worst_acc = 0.0
    for nt in (1, 2, 3):
        (o, st), (ref, st_o) = dev[nt], runs[nt]
        assert np.all(st[:, :, 7] == 0) and np.all(np.isfinite(o))
        for idx, name in ((2, 'leapfrogs'), (3, 'gradients'), (4, 'divergences'), (6, 'mean depth')):
            assert np.array_equal(st[:, :, idx], st_o[:, :, idx]), (case.id, nt, name, st[:, :, idx], st_o[:, :, idx])
        err = np.abs(o - ref).max(axis=(2, 3)) / np.maximum(1.0, np.abs(ref).max(axis=(2, 3)))
        acc = np.abs(st[:, :, 5] - st_o[:, :, 5]) / (1e-9 + 1e-9 * np.abs(st_o[:, :, 5]))
        worst_draw, worst_acc = max(worst_draw, err.max()), max(worst_acc, acc.max())
        assert np.all(err < 1e-6), (case.id, nt, err)
        assert np.all(acc <= 1.0), (case.id, nt, st[:, :, 5], st_o[:, :, 5])
    dep = rc.depths(runs)
    if case.part == 'H' and not case.claim[2]:
        assert dep.max() > case.claim[3]                      # (the oracle at the device's cavities still leaves the levels kept in LDS)
    print('MARGIN %s %s (%s, layout %d): transitions, tree depths up to %d, draws %.3e of 1e-6, accept %.3e of its bound'
          % (case.part, case.id, case.claim[0], case.served, dep.max(), worst_draw / 1e-6, worst_acc))


@pytest.mark.parametrize('case', rc.cases(check='neighbour'), ids=repr)
def test_a_site_does_not_depend_on_its_neighbours_rows(case):
    """Site 0 with site 1's rows as they are, multiplied by 1e300, and NaN: the same bits.  The padding columns of a
    resident row and the rows a tile holds behind the site's own are the neighbour's in memory."""
    p, eng, Om, mu = _engine(case)
    lo1 = int(p['k_lim'][1])
    ths = rc.thetas(case, p, 0)
    want = []
    for th in ths:
        lp, g = eng.logdensity_grad(0, th, layout=case.req)
        assert eng.last_layout() == case.served, (case.id, eng.last_layout())
        assert np.isfinite(lp) and np.all(np.isfinite(g))
        want.append((lp, g))
    for what in ('x 1e300', 'NaN'):
        X2 = p['X'].copy()
        if what == 'NaN':
            X2[lo1:] = np.nan
        else:
            X2[lo1:] *= rc.NEIGHBOUR_SCALE
            assert np.all(np.isfinite(X2)) and np.abs(X2[lo1:]).min() > 1e290
        eng2, Om2, mu2 = _engine_with_cavity(case.model, X2, p['y'], p['k_lim'], p['Oms'], p['mus'])
        assert np.array_equal(Om2[0], Om[0]) and np.array_equal(mu2[0], mu[0])
        for th, (lp, g) in zip(ths, want):
            for rep in range(2):
                lp2, g2 = eng2.logdensity_grad(0, th, layout=case.req)
                assert eng2.last_layout() == case.served
                assert np.array([lp2]).tobytes() == np.array([lp]).tobytes() and g2.tobytes() == g.tobytes(), (case.id, what, lp, lp2)
    print('MARGIN %s %s (%s, layout %d): site 0 bit-identical with its neighbour\'s rows x 1e300 and NaN'
          % (case.part, case.id, case.claim[0], case.served))
