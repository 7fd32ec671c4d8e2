"""The streaming sampler (layout 3: csrc/nuts_stream.hip, csrc/epx_stream_tile.h) at the edges of its row ring and at
every vector width (stream_edge_cases.py: the table, checked without a device by test_stream_edge_cases.py).

  A  the gradient hook against the C oracle -- 1, 2, 3 tiles (fewer than the ring keeps in flight), 6 and 7 (the ring's
     length and one more), both likelihood families; the fold of the logistic wave's running product at 255, 256, 257,
     513 and 1025 tiles, at theta = 0 (every factor exactly 2: 1025 of them overflow without the fold), at a random
     point and with saturated logits; the column edges D = 63 64 65 127 and 1 2; and a site's bits unchanged when its
     neighbour's rows, which its padding columns read, are multiplied by 1e300;
  B  one case per (DPB, NV) instantiation no other test compares with a reference: gradient, teacher-forced
     transitions, a whole short run, the pieced launch in both its forms;
  C  one to three tiles through the hundreds of passes of transitions and runs, also beside the resident layout 1;
  D  the tile table at the LDS limit: served one tile below it, refused at it, the context usable afterwards;
  E  the lock-step resident layout 4 at NV = 4.

The bounds are the ones the existing tests of the same hooks use:
  * epx_logdensity_grad_layout: test_streaming_gradient_matches_oracle's -- log density 1e-10 max(1, |lp|), gradient
    rtol = 1e-9, atol = 1e-9 max(1, max |g|);
  * epx_nuts_transitions: the same trees (leapfrogs, gradients, divergences equal) and every draw 1e-6 relative to
    max(1, |ref|), no chain excepted (test_stream_edge_cases.py holds the oracle's two builds together at every case);
  * whole runs: the first three kept draws of every chain 1e-3, at least three quarters of the chains equal to the end
    (1e-4) with equal leapfrog and gradient counts (test_streaming_sampler_equals_resident_and_oracle's);
  * the pieced launch: bit equality with the uncut launch;
  * every call made twice: the same bits; a request served by another layout: an error."""

import numpy as np
import pytest

import stream_edge_cases as sc
from conftest import record_slack
from epstan_amd import _lib
from epstan_amd.engine import HipEngine
from oracle import nuts_oracle as no
from test_gpu_parity import _engine_with_cavity, _group_engine

pytestmark = pytest.mark.gpu

_engines = {}


def _engine(case, row_scale=1.0):
    """(problem, engine, the cavities the device holds); shared by the tests of a case."""
    key = (case.id, row_scale)
    if key not in _engines:
        p = sc.problem(case, row_scale)
        if case.multi:
            eng, Om, mu = _group_engine(case.model, p['X'], p['y'], p['k_lim'], p['g_cnt'], p['g_lim'], p['Oms'], p['mus'])
        else:
            eng, Om, mu = _engine_with_cavity(case.model, p['X'], p['y'], p['k_lim'], p['Oms'], p['mus'])
        assert eng.P == case.P and eng.d == case.d
        _engines[key] = (p, eng, Om, mu)
    return _engines[key]


def _gradient_margins(lp, g, lp_o, g_o):
    """The differences as fractions of test_streaming_gradient_matches_oracle's bounds."""
    m_lp = abs(lp - lp_o) / (1e-10 * max(1.0, abs(lp_o)))
    m_g = (np.abs(g - g_o) / (1e-9 * max(1.0, np.abs(g_o).max()) + 1e-9 * np.abs(g_o))).max()
    return m_lp, m_g


def _check_gradient(case, p, eng, Om, mu, tag=''):
    req, served = case.layout
    worst = [0.0, 0.0]
    for k in range(case.K):
        for th in sc.thetas(case, p, k):
            lp, g = eng.logdensity_grad(k, th, layout=req)
            assert eng.last_layout() == served, (case.id, req, eng.last_layout())
            lp2, g2 = eng.logdensity_grad(k, th, layout=req)
            assert lp2 == lp and np.array_equal(g2, g), (case.id, k)                  # (the same call again: the same bits)
            lp_o, g_o = sc.oracle_gradient(case, p, k, th, Om, mu)
            m_lp, m_g = _gradient_margins(lp, g, lp_o, g_o)
            print('%s%s site %d theta %s: lp %.17g oracle %.17g, %.3e of its bound; gradient %.3e of its bound'
                  % (case.id, tag, k, 'zero' if not th.any() else 'random', lp, lp_o, m_lp, m_g))
            assert np.isfinite(lp) and np.all(np.isfinite(g)), (case.id, k, lp)
            assert abs(lp - lp_o) <= 1e-10 * max(1.0, abs(lp_o)), (case.id, k, lp, lp_o)
            np.testing.assert_allclose(g, g_o, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(g_o).max()))
            worst = [max(worst[0], m_lp), max(worst[1], m_g)]
    print('MARGIN %s %s%s: gradient hook, lp %.3e grad %.3e of the bounds' % (case.part, case.id, tag, worst[0], worst[1]))


def _transitions(case, p, eng, layout):
    """NT teacher-forced transitions on the requested layout, made twice."""
    req, served = layout
    out = None
    for rep in range(2):
        o, st = eng.nuts_transitions(p['seeds'], p['q0'], p['eps'], p['inv_e'], nt=sc.NT, t_offset=sc.T_OFFSET, layout=req)
        assert eng.last_layout() == served, (case.id, req, eng.last_layout())
        if out is not None:
            np.testing.assert_array_equal(o, out[0])                                  # (the same launch again: the same bits)
            np.testing.assert_array_equal(st, out[1])
        out = (o, st)
    return out


def _check_transitions(case, name, dev, ref):
    (o, st), (r, st_r) = dev, ref
    assert np.all(st[:, :, 7] == 0) and np.all(np.isfinite(o))
    for idx, what in ((2, 'leapfrogs'), (3, 'gradients'), (4, 'divergences')):
        assert np.array_equal(st[:, :, idx], st_r[:, :, idx]), (case.id, name, what, st[:, :, idx], st_r[:, :, idx])
    assert st_r[:, :, 3].min() >= sc.NT                       # every chain took part in a second and a third pass
    err = np.abs(o - r).max(axis=(2, 3)) / np.maximum(1.0, np.abs(r).max(axis=(2, 3)))
    print('MARGIN %s %s: transitions against %s, leapfrogs %s, largest draw difference %.3e (bound 1e-6: %.3e of it)'
          % (case.part, case.id, name, st_r[:, :, 2].ravel().astype(int).tolist(), err.max(), err.max() / 1e-6))
    assert np.all(err < 1e-6), (case.id, name, err)


def _draws(case, eng, chains):
    return np.stack([eng.get_draws(k, True).reshape(chains, sc.ITER // 2, case.P) for k in range(case.K)])


def _run(case, eng, p, layout, chains=None):
    """The whole short run on the requested layout, made twice: (draws (K, chains, ITER / 2, P), chain statistics)."""
    req, served = layout
    chains = case.chains if chains is None else chains
    opts = HipEngine.sampler_opts(chains=chains, iter=sc.ITER, init='random', layout=req)
    out = None
    for rep in range(2):
        eng.sample_batch(p['seeds'] + 10, opts)
        assert eng.last_layout() == served and eng.last_segments() >= 0, (case.id, req, eng.last_layout(), eng.last_segments())
        dr, cs = _draws(case, eng, chains), eng.get_chain_stats(chains).copy()
        if out is not None:
            np.testing.assert_array_equal(dr, out[0])
            np.testing.assert_array_equal(cs, out[1])
        out = (dr, cs)
    return out


def _check_run(case, name, dev, ref):
    """test_streaming_sampler_equals_resident_and_oracle's criterion; returns the chains equal to the end."""
    (dr, cs), (dr_r, st_r) = dev, ref
    K, C = case.K, case.chains
    assert np.all(cs[:, :, 7] == 0) and np.all(np.isfinite(dr))
    n_full, worst3, worst_full = 0, 0.0, 0.0
    for k in range(K):
        err = np.abs(dr[k] - dr_r[k]).max(axis=2) / max(1.0, np.abs(dr_r[k]).max())
        for c in range(C):
            worst3 = max(worst3, err[c, :3].max())
            assert np.all(err[c, :3] < 1e-3), (case.id, name, k, c, err[c, :3])
            if np.all(err[c] < 1e-4):
                n_full += 1
                worst_full = max(worst_full, err[c].max())
                assert cs[k, c, 2] == st_r[k, c, 2] and cs[k, c, 3] == st_r[k, c, 3], (case.id, name, k, c)
    need = (3 * K * C) // 4
    print('MARGIN %s %s: run against %s, %d of %d chains equal to the end (need %d); first three draws %.3e of 1e-3, the equal '
          'chains %.3e of 1e-4' % (case.part, case.id, name, n_full, K * C, need, worst3 / 1e-3, worst_full / 1e-4))
    record_slack('stream edges %s run vs %s: chains equal to the end' % (case.id, name), n_full, '>= %d' % need, K * C)
    assert n_full >= need, (case.id, name, n_full)
    return n_full


# ---------------------------------------------------------------- A: the gradient hook
@pytest.mark.parametrize('case', sc.cases('A-tiles') + sc.cases('A-cols'), ids=repr)
def test_gradient_at_tile_counts_and_column_edges(case):
    p, eng, Om, mu = _engine(case)
    _check_gradient(case, p, eng, Om, mu)


@pytest.mark.parametrize('case', sc.cases('A-folds'), ids=repr)
def test_gradient_across_the_folds_of_the_logistic_product(case):
    for scale in (1.0, sc.FOLD_ROW_SCALE):
        p, eng, Om, mu = _engine(case, scale)
        _check_gradient(case, p, eng, Om, mu, tag=' rows x %g' % scale)
        _engines.pop((case.id, scale))                        # (the largest inputs of the file: not kept)


@pytest.mark.parametrize('case', sc.cases('A-neighbour'), ids=repr)
def test_a_site_does_not_depend_on_its_neighbours_rows(case):
    p, eng, Om, mu = _engine(case)
    _check_gradient(case, p, eng, Om, mu)                     # (every site, the last one with the zeroed padding behind X included)
    X2 = p['X'].copy()
    X2[int(p['k_lim'][1]):] *= sc.NEIGHBOUR_SCALE
    assert np.all(np.isfinite(X2)) and np.abs(X2[int(p['k_lim'][1]):]).min() > 1e290
    eng2, Om2, mu2 = _engine_with_cavity(case.model, X2, p['y'], p['k_lim'], p['Oms'], p['mus'])
    assert np.array_equal(Om2, Om) and np.array_equal(mu2, mu)
    req, served = case.layout
    for th in sc.thetas(case, p, 0) + [np.zeros(case.P)]:
        lp, g = eng.logdensity_grad(0, th, layout=req)
        assert eng.last_layout() == served
        for rep in range(2):
            lp2, g2 = eng2.logdensity_grad(0, th, layout=req)
            assert eng2.last_layout() == served
            assert lp2 == lp and np.array_equal(g2, g), (case.id, lp, lp2, np.abs(g2 - g).max())
    print('MARGIN %s %s: site 0 bit-identical with its neighbour\'s rows x %g' % (case.part, case.id, sc.NEIGHBOUR_SCALE))


# ---------------------------------------------------------------- B, C, E: the sampler
SAMPLER_CASES = sc.cases('B') + sc.cases('C') + sc.cases('E')


@pytest.mark.parametrize('case', SAMPLER_CASES, ids=repr)
def test_sampler_case_gradient(case):
    p, eng, Om, mu = _engine(case)
    _check_gradient(case, p, eng, Om, mu)


@pytest.mark.parametrize('case', [c for c in SAMPLER_CASES if 'trans' in c.checks], ids=repr)
def test_teacher_forced_transitions_follow_the_oracle(case):
    p, eng, Om, mu = _engine(case)
    dev = _transitions(case, p, eng, case.layout)
    _check_transitions(case, 'the oracle', dev, sc.oracle_transitions(case, p, Om, mu))
    if 'resident' in case.checks:
        _check_transitions(case, 'layout 1', dev, _transitions(case, p, eng, (1, 1)))


_uncut = {}


@pytest.mark.parametrize('case', [c for c in SAMPLER_CASES if 'run' in c.checks], ids=repr)
def test_short_runs_follow_the_oracle(case):
    p, eng, Om, mu = _engine(case)
    dev = _run(case, eng, p, case.layout)
    _uncut[case.id] = dev
    _check_run(case, 'the oracle', dev, sc.oracle_run(case, p, Om, mu))
    if 'resident' in case.checks:
        dr1, cs1 = _run(case, eng, p, (1, 1))
        _check_run(case, 'layout 1', dev, (dr1, cs1))


@pytest.mark.parametrize('case', [c for c in SAMPLER_CASES if 'pieces' in c.checks], ids=repr)
def test_pieced_launch_gives_the_uncut_draws(case, monkeypatch):
    """Pieces of 3 transitions, looping workgroups and (EPX_PIECE_GRID=1) one workgroup per piece: draws and chain
    statistics of the uncut launch, bit for bit."""
    p, eng, Om, mu = _engine(case)
    chains = min(case.chains, 4)              # (the piece queue takes sites of one workgroup: a six-chain case is cut with four)
    if case.id not in _uncut or chains != case.chains:
        _uncut[case.id] = _run(case, eng, p, case.layout, chains)
    dr0, cs0 = _uncut[case.id]
    req, served = case.layout
    opts = HipEngine.sampler_opts(chains=chains, iter=sc.ITER, init='random', layout=req)
    try:
        for grid in (False, True):
            if grid:
                monkeypatch.setenv('EPX_PIECE_GRID', '1')
            eng.set_piece_queue(3, np.linspace(1.0, 2.0, case.K))
            for rep in range(2):
                eng.sample_batch(p['seeds'] + 10, opts)
                assert eng.last_layout() == served and eng.last_segments() == -(sc.ITER // 3), (case.id, eng.last_layout(), eng.last_segments())
                np.testing.assert_array_equal(_draws(case, eng, chains), dr0)
                np.testing.assert_array_equal(eng.get_chain_stats(chains), cs0)
    finally:
        eng.set_piece_queue(0)
    print('MARGIN %s %s: pieced launch (looping workgroups, one workgroup per piece) bit-identical to the uncut launch' % (case.part, case.id))


# ---------------------------------------------------------------- D: the LDS limit
def test_tile_table_at_the_lds_limit():
    """One tile below the first tile count the planner refuses (stream_edge_cases.LIMIT, read from the library by
    test_stream_edge_cases.py) the streamed site gives the oracle's gradient -- so does the small site beside it, whose
    launch carries the same tile table; at that count the call is refused by the planner, before any launch, and the
    context goes on answering as before."""
    L = sc.LIMIT
    first = L['first_refused_tiles']
    rng = np.random.RandomState(8)
    th = 0.3 * rng.randn(L['P'])
    X, y, k_lim, Oms, mus = sc.limit_problem(first - 1)
    eng, Om, mu = _engine_with_cavity(L['model'], X, y, k_lim, Oms, mus)
    good = {}
    for k in range(2):
        lp, g = eng.logdensity_grad(k, th, layout=3)
        assert eng.last_layout() == 3
        lp2, g2 = eng.logdensity_grad(k, th, layout=3)
        assert lp2 == lp and np.array_equal(g2, g)
        lo, hi = int(k_lim[k]), int(k_lim[k + 1])
        lp_o, g_o = no.logdensity_grad(L['model'], X[lo:hi], y[lo:hi], mu[k], Om[k], th)
        m_lp, m_g = _gradient_margins(lp, g, lp_o, g_o)
        print('MARGIN D %d tiles, site %d (%d rows): lp %.3e grad %.3e of the bounds' % (first - 1, k, hi - lo, m_lp, m_g))
        assert abs(lp - lp_o) <= 1e-10 * max(1.0, abs(lp_o)), (k, lp, lp_o)
        np.testing.assert_allclose(g, g_o, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(g_o).max()))
        good[k] = (lp, g)
    X2, y2, k_lim2, Oms2, mus2 = sc.limit_problem(first)
    eng2, Om2, mu2 = _engine_with_cavity(L['model'], X2, y2, k_lim2, Oms2, mus2)
    cav = [eng2.get_cavity(k) for k in range(2)]
    for k in range(2):
        with pytest.raises(_lib.EpxError, match=r'streaming sampler needs \d+ B of LDS'):
            eng2.logdensity_grad(k, th, layout=3)
    with pytest.raises(_lib.EpxError, match=r'streaming sampler needs \d+ B of LDS'):
        eng2.sample_batch(np.array([1, 2], dtype=np.int64), HipEngine.sampler_opts(chains=4, iter=4, init='random', layout=3))
    # the refused context still answers, with the bytes it returned before ...
    d = L['d']
    for k in range(2):
        assert eng2.cavity_site(k, Oms2[k] + np.eye(d), Oms2[k].dot(mus2[k]), np.eye(d), np.zeros(d))
        Om_k, mu_k = eng2.get_cavity(k)
        assert np.array_equal(Om_k, cav[k][0]) and np.array_equal(mu_k, cav[k][1])
    # ... and so does the one that was served
    for k in range(2):
        lp, g = eng.logdensity_grad(k, th, layout=3)
        assert eng.last_layout() == 3 and lp == good[k][0] and np.array_equal(g, good[k][1])
