"""(no device) The front matter that the entries over draws share, csrc/epx_draws.h, through tests/draw_source_probe.hip: a
small host program that fills the plain fields of a context by hand and prints what the pure functions decide.

 * draw_source: where a call's draws come from, how many they are, and every refusal with the entry's name in it.
 * named_layout: the offsets of a row of named parameters against site_params.named_shape, for the context's largest
   site (the per-site entries) and for every site's own group count (the pooled counting pass).
 * cut_ctx_rows: the context's own rows cut into work items (epx_loo: items of 16 x tiles rows; epx_ppc and
   epx_site_evidence: whole groups) and site_first, against the records written down here from the rows per group.
 * check_rank_count, fill_ranks, pow2_pad: the rank list of the order-statistic entries and the padding of their keys.
 * lds_budget: the one reader of EPX_PO_LDS_BYTES and EPX_LOO_LDS_BYTES."""

import os
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


SINGLE = [[3], [0], [16], [17], [65]]                  # rows per group, site by site: one group everywhere (no g_cnt)
MULTI = [[9], [8, 7, 9], [10, 6]]
MULTI_EMPTY = [[9], [8, 0, 9], [10, 6]]                # (ctx_create refuses an empty group; the cutting does not depend on that)


@pytest.mark.parametrize('item', [16, 64, 0])
@pytest.mark.parametrize('sites', [SINGLE, MULTI, MULTI_EMPTY])
def test_context_rows_cut_into_items(probe, sites, item):
    K = len(sites)
    g_cnt = [len(s) for s in sites]
    g_lim = np.concatenate(([0], np.cumsum([n for s in sites for n in s])))
    k_lim = np.concatenate(([0], np.cumsum([sum(s) for s in sites])))
    for k0, count in ((0, K), (1, 2), (K - 1, 1)):
        gi = sum(g_cnt[:k0])
        want, first = [], [0]
        for j in range(count):
            for g in range(g_cnt[k0 + j]):
                lo, hi = int(g_lim[gi]), int(g_lim[gi + 1])
                gi += 1
                if item == 0:                           # whole groups: one record each, an empty one too
                    want.append((j, g, lo, hi - lo))
                else:                                   # at most `item` rows: an empty group gives none
                    want += [(j, g, r, min(item, hi - r)) for r in range(lo, hi, item)]
            first.append(len(want))
        rows = '/'.join(','.join(str(n) for n in s) for s in sites)
        out = subprocess.check_output([probe, 'items', rows, str(k0), str(count), str(item)]).decode().splitlines()
        got = [tuple(int(w) for w in line.split()[1:]) for line in out[:-1]]
        assert all(line.startswith('wg ') for line in out[:-1]) and got == want, (sites, k0, count, item, got, want)
        assert out[-1].split() == ['first'] + [str(f) for f in first], (sites, k0, count, item, out[-1])
        # the records lie in the rows of their site, in order, and cover them
        for j in range(count):
            lo, hi = int(k_lim[k0 + j]), int(k_lim[k0 + j + 1])
            mine = got[first[j]:first[j + 1]]
            assert all(lo <= f and f + n <= hi and (item == 0 or 1 <= n <= item) for _, _, f, n in mine)
            assert sum(n for _, _, _, n in mine) == hi - lo
            assert [f for _, _, f, _ in mine] == sorted(f for _, _, f, _ in mine)
        if item == 0:
            assert len(got) == sum(g_cnt[k0:k0 + count])


def _ranks(probe, who, S, ranks):
    arg = 'null' if ranks is None else ','.join(str(r) for r in ranks) or 'none'
    return subprocess.check_output([probe, 'ranks', who, str(S), arg]).decode().strip()


@pytest.mark.parametrize('who', ['epx_named_order_stats', 'epx_predict_order_stats'])
def test_rank_list(probe, who):
    for S, ranks in ((5, [0]), (5, [0, 4]), (32, list(range(32)))):
        assert _ranks(probe, who, S, ranks).split() == ['ok'] + [str(r) for r in ranks] + ['0'] * (32 - len(ranks))
    for ranks in (None, [], list(range(33))):
        n = 0 if ranks is None else len(ranks)
        assert _ranks(probe, who, 64, ranks) == 'refused %s: between 1 and 32 ranks (got %d)' % (who, n)
    assert _ranks(probe, who, 5, [5]) == 'refused %s: rank 5 outside [0, 5), the draws per site' % who
    assert _ranks(probe, who, 5, [-1]) == 'refused %s: rank -1 outside [0, 5), the draws per site' % who
    for ranks in ([2, 2], [3, 1]):
        assert _ranks(probe, who, 5, ranks) == 'refused %s: the ranks have to be ascending and distinct' % who


def test_power_of_two_padding(probe):
    for S, want in ((1, '2 1'), (2, '2 1'), (3, '4 2'), (64, '64 6'), (65, '128 7')):
        assert subprocess.check_output([probe, 'pad', str(S)]).decode().strip() == want


@pytest.mark.parametrize('var', ['EPX_PO_LDS_BYTES', 'EPX_LOO_LDS_BYTES'])
def test_lds_budget_knob(probe, var):
    def budget(value):
        env = {k: v for k, v in os.environ.items() if k != var}
        if value is not None:
            env[var] = value
        return subprocess.check_output([probe, 'budget', var, '1000'], env=env).decode().rstrip('\n')

    assert budget(None) == '1000|'
    for value in ('0', '999'):                          # lowered: the note is what epx_predict_order_stats appends to a refusal
        assert budget(value) == "%s|; %s = %s lowers the keys' budget" % (value, var, value)
    for value in ('1000', '5000'):                      # nothing lowered, nothing said
        assert budget(value) == '1000|'
    for junk in ('', 'lots', '12k', '-1'):              # no whole non-negative number: ignored
        assert budget(junk) == '1000|'
