"""(no device) The front matter that the entries over draws share, csrc/epx_draws.h, through tests/draw_source_probe.hip: a
small host program that fills the plain fields of a context by hand and prints what the pure functions decide.

 * draw_source: where a call's draws come from, how many they are, and every refusal with the entry's name in it.
 * named_layout: the offsets of a row of named parameters against site_params.named_shape, for the context's largest
   site (the per-site entries) and for every site's own group count (the pooled counting pass)."""

import subprocess

import numpy as np
import pytest

from epstan_amd import site_params as sp
from epstan_amd.engine import MODEL_IDS, is_gauss
from test_tree_endings_cases import _build_probe

K, P, CHAINS, NKEEP = 3, 12, 2, 5


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    return _build_probe(tmp_path_factory.mktemp('draw_source'), 'draw_source_probe')


def _source(probe, who, drawn, k0, count, inject=False, S=0, chains=-1):
    """drawn: (k0, count) of the last sampling call, or None: nothing sampled yet."""
    dk0, dcount = drawn if drawn else (0, 0)
    args = [who, K, P, CHAINS, NKEEP, dk0, dcount, int(drawn is not None), k0, count, int(inject), S, chains]
    return subprocess.check_output([probe, 'source'] + [str(a) for a in args]).decode().strip()


def test_draw_source(probe):
    assert _source(probe, 'epx_loo', None, 0, 2) == 'refused no draws yet'
    assert _source(probe, 'epx_predict', (1, 2), 0, 2) == \
        'refused epx_predict: sites [0,2) asked, the last sampling call left draws of sites [1,3) only'
    assert _source(probe, 'epx_named_moments', (1, 2), 2, 2).startswith('refused epx_named_moments: sites [2,4) asked')
    assert _source(probe, 'epx_loo', None, 0, 2, inject=True, S=0) == 'refused epx_loo: S = 0 draws'
    # injected draws: S as given, nothing asked of the sampler's state; (S, chains, offset in c->draws, doubles to copy)
    assert _source(probe, 'epx_loo', None, 0, 2, inject=True, S=7) == 'ok 7 0 0 %d' % (2 * 7 * P)
    # retained draws: chains x nkeep per site, site k0's block at k0 * S * P
    S = CHAINS * NKEEP
    assert _source(probe, 'epx_loo', (0, 3), 1, 2) == 'ok %d %d %d %d' % (S, CHAINS, 1 * S * P, 2 * S * P)
    assert _source(probe, 'epx_pooled_moments', (1, 2), 2, 1) == 'ok %d %d %d %d' % (S, CHAINS, 2 * S * P, S * P)
    # the chains of injected draws (epx_draw_diagnostics)
    who = 'epx_draw_diagnostics'
    assert _source(probe, who, None, 0, 1, inject=True, S=10, chains=3) == \
        'refused %s: S = 10 draws are no multiple of chains = 3' % who
    assert _source(probe, who, None, 0, 1, inject=True, S=10, chains=0) == 'refused %s: chains must be in 1..16 (got 0)' % who
    assert _source(probe, who, None, 0, 1, inject=True, S=10, chains=17).startswith('refused %s: chains must be' % who)
    assert _source(probe, who, None, 0, 1, inject=True, S=0, chains=0) == 'refused %s: S = 0 draws' % who
    assert _source(probe, who, None, 0, 1, inject=True, S=10, chains=5) == 'ok 10 5 0 %d' % (10 * P)
    assert _source(probe, who, (0, 3), 0, 3, chains=7) == 'ok %d %d 0 %d' % (S, CHAINS, 3 * S * P)     # (the sampler's chains)


@pytest.mark.parametrize('model,groups', [('m1a_sg', None), ('m4b_sg', None), ('m4b', [1, 3, 2])])
def test_named_layout(probe, model, groups):
    D = 3
    mid, gauss, sg = MODEL_IDS[model] % 5, is_gauss(model), model.endswith('_sg')
    d = sp.layout(mid, D, 1, gauss)[1]
    head = [probe, 'layout', str(mid), str(int(gauss)), str(D), str(d), ','.join(map(str, groups)) if groups else '-']
    names = [name for name in sp.NAME_IDS if name in sp.names(mid, gauss)]
    lines = subprocess.check_output(head + [str(sp.NAME_IDS[name]) for name in names]).decode().splitlines()
    ngs = groups or [1]
    assert len(lines) == 1 + len(ngs)
    for line, k, ng in zip(lines, [-1] + list(range(len(ngs))), [max(ngs)] + ngs):
        sizes = [int(np.prod(sp.named_shape(mid, D, ng, gauss, sg, name), dtype=np.int64)) for name in names]
        off = np.concatenate(([0], np.cumsum(sizes)))
        assert line.split() == ['ok', str(k), str(off[-1])] + [str(o) for o in off], (model, k, ng, line)
    missing = [name for name in sp.NAME_IDS if name not in names]
    assert missing
    for name in missing:
        out = subprocess.check_output(head + [str(sp.NAME_IDS['phi']), str(sp.NAME_IDS[name])]).decode().strip()
        assert out == 'refused named parameter %d is not defined by this site model' % sp.NAME_IDS[name]
