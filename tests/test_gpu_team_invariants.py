"""Layout 7 (row team, csrc/nuts_duo.hip): what a row wave forms once per piece and uses in every lock-step pass.

A row wave keeps, for the whole piece, its group of the cavity precision (wave 3 also the rows beyond the 16-row groups,
whose products run between the group's as a third chain), the responses of its lanes' rows as bits, and the LDS addresses
of its first tile pair; only `(alpha, beta, V)` of the four chains change from pass to pass.  That is right only while
the staged rows stay what they are: per piece, never from one site to the next.  The cases are the shapes at which that
state can go wrong; layout 1 (one wave per chain, rows resident, no team) and the C restatement are the references, with
the bounds the existing tests of the same hooks use:

  * epx_logdensity_grad_layout: smoke()'s bound for layout 7 (1e-9 relative on the log density, rtol = atol = 1e-9 on the
    gradient; the cavity term's rows 64 and 65 at D = 32 are in both);
  * epx_nuts_transitions: test_gpu_parity's teacher-forced bound (the same tree, the draw to 1e-6 relative, no
    transition excepted for layout 7), here over nt = 3 consecutive transitions -- hundreds of passes of one launch;
  * the pieced launch: bit equality with the uncut launch."""

import numpy as np
import pytest

from epstan_amd.engine import HipEngine
from oracle import nuts_oracle as no
from test_gpu_parity import _engine_with_cavity, _site_problem

gpu = pytest.mark.gpu


def _tiles_per_wave(n):
    """csrc/nuts_duo.hip team_tiles_per_wave: the same EVEN number of 16-row tiles for each of the four row waves."""
    t = ((n + 15) // 16 + 3) // 4
    return (t + 1) & ~1


# (D, n): what the shape does to the four row waves
CASES = [
    (32, 500),      # the headline site: four rounds per wave, the site's last tile partial (wave 3, last round)
    (32, 512),      # no partial tile
    (32, 33),       # one round per wave; waves 1 .. 3 hold padding tiles only
    (32, 129),      # two rounds per wave; the partial tile (one row) is the FIRST tile of wave 2: the edge mask in a pass's first round
    (32, 65),       # the same with one round per wave
    (16, 200),      # two rows per bank line (RPL = 2 swizzle), two rounds per wave
]


def test_case_table_has_the_geometry_it_claims():
    """(no device) The shapes above against the kernel's tiling rule."""
    geo = {}
    for D, n in CASES:
        tpw = _tiles_per_wave(n)
        tiles = (n + 15) // 16
        part = tiles - 1 if n % 16 else None                    # index of the partial tile
        geo[(D, n)] = (tpw // 2, part, None if part is None else (part // tpw, part % tpw))
        assert tpw % 2 == 0 and 4 * tpw >= tiles
    assert geo[(32, 500)] == (4, 31, (3, 7))                    # rounds per wave, partial tile, (its wave, its place in the wave)
    assert geo[(32, 512)] == (4, None, None)
    assert geo[(32, 33)] == (1, 2, (1, 0))
    assert geo[(32, 129)] == (2, 8, (2, 0))
    assert geo[(32, 65)] == (1, 4, (2, 0))
    assert geo[(16, 200)] == (2, 12, (3, 0))


_problems = {}


def _problem(D, n):
    """Two sites with a dominant cavity (short, non-chaotic trajectories: sequences of transitions are compared), the
    engine, and adapted step sizes / typical-set points from ONE layout-1 run; shared by the tests of a shape."""
    if (D, n) not in _problems:
        K = 2
        X, y, k_lim, Oms, mus, d, P = _site_problem('m4b_sg', D, n, 400 + D + n, K=K, tight=1000.)
        eng, Om_dev, mu_dev = _engine_with_cavity('m4b_sg', X, y, k_lim, Oms, mus)
        seeds = np.array([21, 22], dtype=np.int64)
        eng.sample_batch(seeds, HipEngine.sampler_opts(chains=4, iter=40, init='random', layout=1))
        assert eng.last_layout() == 1
        cs = eng.get_chain_stats(4)
        draws = np.stack([eng.get_draws(k, True).reshape(4, 20, P) for k in range(K)])
        inv_e = np.repeat(draws.reshape(K, -1, P).var(axis=1)[:, None, :], 4, axis=1) + 1e-6
        _problems[(D, n)] = dict(X=X, y=y, k_lim=k_lim, Om=Om_dev, mu=mu_dev, P=P, eng=eng, seeds=seeds,
                                 q0=draws[:, :, -1, :].copy(), eps=cs[:, :, 1].copy(), inv_e=inv_e)
    return _problems[(D, n)]


@gpu
@pytest.mark.parametrize('D,n', CASES)
def test_team_gradient_matches_one_wave_per_chain_and_the_oracle(D, n):
    p = _problem(D, n)
    eng = p['eng']
    rng = np.random.RandomState(9)
    for k in range(2):
        lo, hi = p['k_lim'][k], p['k_lim'][k + 1]
        for trial in range(2):
            theta = rng.randn(p['P']) * (0.2 + 0.5 * trial)
            lp_o, g_o = no.logdensity_grad('m4b_sg', p['X'][lo:hi], p['y'][lo:hi], p['mu'][k], p['Om'][k], theta)
            lp1, g1 = eng.logdensity_grad(k, theta, layout=1)
            assert eng.last_layout() == 1
            lp7, g7 = eng.logdensity_grad(k, theta, layout=7)
            assert eng.last_layout() == 7
            lp7b, g7b = eng.logdensity_grad(k, theta, layout=7)
            assert lp7b == lp7 and np.array_equal(g7b, g7)
            for lp_r, g_r in ((lp1, g1), (lp_o, g_o)):
                print('D=%d n=%d site %d: lp diff %.3e (rel), gradient diff %.3e' % (D, n, k, abs(lp7 - lp_r) / max(1.0, abs(lp_r)), np.abs(g7 - g_r).max()))
                assert abs(lp7 - lp_r) <= 1e-9 * max(1.0, abs(lp_r))
                assert np.allclose(g7, g_r, rtol=1e-9, atol=1e-9)


@gpu
@pytest.mark.parametrize('D,n', CASES)
def test_team_transitions_match_one_wave_per_chain(D, n):
    p = _problem(D, n)
    eng = p['eng']
    nt = 3
    out = {}
    for layout in (1, 7, 7):
        o, st = eng.nuts_transitions(p['seeds'], p['q0'], p['eps'], p['inv_e'], nt=nt, t_offset=4, layout=layout)
        assert eng.last_layout() == layout
        if layout in out:
            np.testing.assert_array_equal(o, out[layout][0])        # (the same launch again: the same bits)
            np.testing.assert_array_equal(st, out[layout][1])
        out[layout] = (o, st)
    (o1, st1), (o7, st7) = out[1], out[7]
    assert st1[:, :, 3].min() >= 3                                  # every chain took part in a second and a third pass
    err = np.abs(o7 - o1).max(axis=(2, 3)) / np.maximum(1.0, np.abs(o1).max(axis=(2, 3)))
    print('D=%d n=%d: leapfrogs %s, largest relative difference %.3e' % (D, n, st1[:, :, 2].ravel(), err.max()))
    np.testing.assert_array_equal(st7[:, :, 2], st1[:, :, 2])       # the same trees
    assert np.all(err < 1e-6), err


@gpu
def test_pieces_of_two_sites_on_looping_workgroups_give_the_uncut_draws():
    """Two sites in pieces of 2 transitions: a looping workgroup runs consecutive pieces of one site and then pieces of
    the other (only one workgroup can hold a site at a time, so two work and the claims alternate between them).  The
    rows, the responses' bits and the cavity operands are formed again at every piece start: the draws, last states and
    statistics are the uncut launch's, repeatedly."""
    p = _problem(32, 500)
    eng = p['eng']
    it = 24
    opts = HipEngine.sampler_opts(chains=4, iter=it, init='random', layout=7)

    def run():
        eng.sample_batch(p['seeds'] + 5, opts)
        assert eng.last_layout() == 7
        return np.stack([eng.get_draws(k, all_params=True) for k in range(2)]), eng.get_chain_stats(4).copy()

    eng.set_piece_queue(0)
    dr0, cs0 = run()
    assert eng.last_segments() == 0
    try:
        eng.set_piece_queue(2, None)
        for rep in range(3):
            dr, cs = run()
            assert eng.last_segments() == -(it // 2)
            np.testing.assert_array_equal(dr, dr0)
            np.testing.assert_array_equal(cs, cs0)
    finally:
        eng.set_piece_queue(0)
