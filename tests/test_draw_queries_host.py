"""draw_queries.py on the CPU: the host route keeps `HipEngine`'s signatures, the resolver chooses per method, the padded
gather returns every site's own record and nothing of the padding, and predict's row planning is a pure function."""

import inspect

import numpy as np
import pytest

from epstan_amd import diagnostics, dist, draw_queries as dq, fit, loo, models, site_params
from epstan_amd.engine import HipEngine, site_spec
from epstan_amd.method import Master
from epstan_amd.util import distribute_groups
from oracle.engine_oracle import OracleEngine


# ------------------------------------------------------------------ signature parity
class Recorder(object):
    """Stands in for `Master._queries`: notes (name, args, kwargs) of every call and passes it on."""

    def __init__(self, target):
        self.target, self.calls = target, []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name, args, kw))
            return getattr(self.target, name)(*args, **kw)
        return call


@pytest.fixture(scope='module')
def master_passes():
    """What `Master` really passes each of the eight methods: the seven public queries on a small host fit (m4b, 7 groups
    on 3 sites), recorded."""
    mod = models.m4b(7, 2, 25)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    Nk, Nj_k, j_ind_k = distribute_groups(7, 3, data.Nj)
    M = Master('m4b', data.X, data.y, site_sizes=Nk, A_k={'J': Nj_k}, A_n={'j_ind': j_ind_k + 1},
               prior={'Q': Q0, 'r': r0}, chains=4, iter=40, df0=0.4,
               _engine_factory=lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, **g))
    M.run(1, verbose=False, seed=3)
    rec = M._queries = Recorder(M._queries)
    pnames, pshapes, phiers = mod.get_param_definitions()
    pmaps = fit._create_pmaps(phiers, 7, 3, Nj_k)
    M.mix_pred(pnames, pmaps, pshapes)
    M.mix_quantiles(pnames, smap=pmaps, param_shapes=pshapes)
    M.mix_quantiles('phi')
    M.predict(data.X, site_sizes=Nk, j_ind=j_ind_k + 1, y_new=data.y)
    M.predict_new_group(data.X[:9], np.arange(9) % 2, y_new=data.y[:9], R=2, seed=5)
    M.loo()
    M.diagnostics(rank=True)
    return rec.calls


def test_master_reaches_the_engine_through_the_eight_names_only(master_passes):
    assert sorted(set(name for name, _, _ in master_passes)) == sorted(dq.QUERIES) and len(dq.QUERIES) == 8


@pytest.mark.parametrize('name', dq.QUERIES)
def test_the_host_route_keeps_the_engines_signature(name, master_passes):
    host, device = inspect.signature(getattr(dq.HostDraws, name)), inspect.signature(getattr(HipEngine, name))
    for par in host.parameters.values():
        assert par.name in device.parameters, '%s: HipEngine.%s takes no `%s`' % (name, name, par.name)
        assert par.default == device.parameters[par.name].default, (name, par.name)
    calls = [(args, kw) for called, args, kw in master_passes if called == name]
    assert calls
    for args, kw in calls:                                 # every argument lands on the same name on both routes
        to_host, to_device = host.bind('self', *args, **kw).arguments, device.bind('self', *args, **kw).arguments
        assert list(to_host) == list(to_device) and all(to_host[k] is to_device[k] for k in to_host), name


# ------------------------------------------------------------------ resolution
MODEL, D, S, CHAINS = 'm4b_sg', 2, 40, 4
ROWS = np.array([0, 5, 9])


class StubEngine(object):
    """A sampling engine with `get_draws`, `num_draws` and ONE of the eight methods."""

    def __init__(self):
        self.d = site_params.layout(3, D, 1, False)[1]
        self.P = self.d + 1 + D
        self.draws = np.asfortranarray(0.3 * np.random.RandomState(0).randn(2, S, self.P))
        self.calls = []

    def num_draws(self):
        return S

    def get_draws(self, k, all_params=False):
        return np.asfortranarray(self.draws[k][:, :self.P if all_params else self.d])

    def predict(self, Xn, row_lim, row_group=None, y=None):
        self.calls.append('predict')
        return np.zeros((Xn.shape[0], site_params.PR_COUNT))


class SpiedHost(dq.HostDraws):
    """HostDraws that notes which of its eight methods were called."""


def _spied(name):
    def method(self, *args, **kw):
        self.calls.append(name)
        return getattr(dq.HostDraws, name)(self, *args, **kw)
    return method


for _name in dq.QUERIES:
    setattr(SpiedHost, _name, _spied(_name))


def test_every_method_is_resolved_on_its_own():
    rng = np.random.RandomState(1)
    eng = StubEngine()
    X, y = rng.randn(9, D), (rng.rand(9) < 0.5).astype(np.float64)
    host = SpiedHost(lambda: eng, site_spec(MODEL), D, np.ones(2, dtype=np.int64), X, y, None, ROWS, CHAINS)
    host.calls = []
    q = dq.Queries(host)
    comm = dist.LocalComm()
    n, means, m2s = q.named_moments(['alpha', 'beta'])
    assert n == S and len(means) == len(m2s) == 2 and means[1]['beta'].shape == (D,)
    stats = dq.pooled_order_stats(q, comm, ['phi'], [(eng.d,)], np.array([0, 2 * S - 1]))
    pool = np.concatenate([eng.draws[k][:, :eng.d] for k in range(2)])
    np.testing.assert_array_equal(stats['phi'], [pool.min(axis=0), pool.max(axis=0)])
    stats = q.named_order_stats(['alpha'], np.array([0, S - 1]))
    assert len(stats) == 2 and stats[0]['alpha'].shape == (2,)
    assert q.predict(X, ROWS, None, y).shape == (9, site_params.PR_COUNT)
    rows, glpd, N = q.predict_new_group(X[:4], np.zeros(4, dtype=np.int32), np.array([7]), y[:4], seed=1, t0=0, R=2)
    assert rows.shape == (4, site_params.PR_COUNT) and glpd.shape == (1,) and N == 2 * S * 2
    rec, n = q.loo(with_n=True)
    assert rec.shape == (9, loo.LO_COUNT) and n == S and q.loo().shape == rec.shape
    rec, n = q.draw_diagnostics(with_n=True)
    assert rec.shape == (2, eng.P, diagnostics.DG_COUNT) and n == S
    assert q.draw_rank_diagnostics().shape == (2, eng.P, diagnostics.RD_COUNT)
    assert eng.calls == ['predict']
    assert sorted(set(host.calls)) == sorted(set(dq.QUERIES) - {'predict'})
    with pytest.raises(AttributeError):
        q.get_draws


# ------------------------------------------------------------------ the padded gather
class TwoRanks(object):
    """World 2: `allgather_sites` puts this rank's columns and the peer's side by side, in rank order."""
    world = 2

    def __init__(self, rank, peer=None):
        self.rank, self.peer, self.sent = rank, peer, None

    def allgather_sites(self, local, K):
        self.sent = local
        peer = np.full((local.shape[0], K - local.shape[1]), 777.0) if self.peer is None else self.peer
        return np.concatenate((local, peer) if self.rank == 0 else (peer, local), axis=1)


WIDTHS = [3, 5, 2]


def _gather_on_both_ranks(records, fill, heads):
    """gather_site_records of three sites sharded 2 + 1; returns rank 0's and rank 1's result and what rank 0 sent."""
    (lo0, hi0), (lo1, hi1) = dist.site_range(3, 0, 2), dist.site_range(3, 1, 2)
    first = TwoRanks(1)
    dq.gather_site_records(first, 3, records[lo1:hi1], WIDTHS, fill, None if heads is None else heads[1])
    r0 = TwoRanks(0, first.sent)
    out0 = dq.gather_site_records(r0, 3, records[lo0:hi0], WIDTHS, fill, None if heads is None else heads[0])
    out1 = dq.gather_site_records(TwoRanks(1, r0.sent), 3, records[lo1:hi1], WIDTHS, fill,
                                  None if heads is None else heads[1])
    return out0, out1, r0.sent, (lo0, hi0, lo1, hi1)


@pytest.mark.parametrize('fill', [np.nan, 0.0], ids=['nan', 'zero'])
@pytest.mark.parametrize('heads', [None, (80.0, 76.0)], ids=['bare', 'head'])
def test_padded_gather_round_trips(fill, heads):
    rng = np.random.RandomState(3)
    records = [1.0 + rng.rand(w) for w in WIDTHS]                   # (no element equals a fill value)
    records[1][2] = np.nan                                           # a NaN of the record's own arrives as NaN
    out0, out1, sent, (lo0, hi0, lo1, hi1) = _gather_on_both_ranks(records, fill, heads)
    h = 0 if heads is None else 1
    assert sent.shape == (h + max(WIDTHS), hi0 - lo0) and sent.flags['F_CONTIGUOUS']
    for j, k in enumerate(range(lo0, hi0)):                          # the padding is the fill, behind the record
        np.testing.assert_array_equal(sent[h + WIDTHS[k]:, j], np.full(max(WIDTHS) - WIDTHS[k], fill))
    for sites, got_heads in (out0, out1):
        assert sites.shape == (3, max(WIDTHS))
        for rec, w, want in zip(sites, WIDTHS, records):
            np.testing.assert_array_equal(rec[:w], want)
            np.testing.assert_array_equal(rec[w:], np.full(max(WIDTHS) - w, fill))     # the fill and nothing else
        if heads is None:
            assert got_heads is None
        else:
            want = np.empty(3)
            want[lo0:hi0], want[lo1:hi1] = heads
            np.testing.assert_array_equal(got_heads, want)


def test_named_records_travel_through_the_padded_gather():
    """m4b on three sites of 2, 1 and 3 groups, two rows per record: every rank gets every site's own shapes back."""
    spec, ng, names, R = site_spec('m4b'), [2, 1, 3], ['alpha', 'beta', 'sigma_a'], 2
    shapes = dq.named_shapes(spec, D, ng, names)
    assert shapes[2] == [(3,), (3, D), ()]
    rng = np.random.RandomState(4)
    local = [dict((name, rng.randn(R, *sh)) for name, sh in zip(names, row)) for row in shapes]
    (lo0, hi0), (lo1, hi1) = dist.site_range(3, 0, 2), dist.site_range(3, 1, 2)
    first = TwoRanks(1)
    dq.gather_named_records(first, names, shapes, local[lo1:hi1], R, head=5)
    sites, heads = dq.gather_named_records(TwoRanks(0, first.sent), names, shapes, local[lo0:hi0], R, head=9)
    assert heads.tolist() == [9.0] * (hi0 - lo0) + [5.0] * (hi1 - lo1)
    for got, want in zip(sites, local):
        assert sorted(got) == sorted(names)
        for name in names:
            np.testing.assert_array_equal(got[name], want[name])


# ------------------------------------------------------------------ predict's row planning
NG = np.array([2, 1, 3])


def test_row_plan_by_site_index_equals_the_plan_by_site_sizes():
    n, K = 11, 3
    sizes = np.array([4, 0, 7])                                      # site 1 has no new row
    ind_sorted = np.repeat(np.arange(K), sizes)
    j_sorted = np.array([1, 2, 2, 1, 3, 1, 1, 2, 3, 3, 2])
    rows, lim, group = dq.plan_rows(n, K, sizes, None, j_sorted, NG, False, 'm4b')
    assert rows.tolist() == list(range(n)) and lim.tolist() == [0, 4, 4, 11]
    assert group.dtype == np.int32 and group.tolist() == (j_sorted - 1).tolist()
    perm = np.random.RandomState(5).permutation(n)
    rows2, lim2, group2 = dq.plan_rows(n, K, None, ind_sorted[perm], j_sorted[perm], NG, False, 'm4b')
    assert rows2.tolist() == np.argsort(ind_sorted[perm], kind='stable').tolist()
    by_sizes = dq.plan_rows(n, K, sizes, None, j_sorted[perm][rows2], NG, False, 'm4b')       # the same rows, sorted
    assert lim2.tolist() == by_sizes[1].tolist() == lim.tolist() and group2.tolist() == by_sizes[2].tolist()
    assert ind_sorted[perm][rows2].tolist() == ind_sorted.tolist()
    for k in range(K):                                               # stable: the caller's order inside a site
        assert np.all(np.diff(rows2[lim2[k]:lim2[k + 1]]) > 0)
    rows3, lim3, group3 = dq.plan_rows(n, K, sizes, None, None, np.ones(K, dtype=np.int64), True, 'm4b_sg')
    assert group3 is None and lim3.tolist() == lim.tolist() and rows3.tolist() == list(range(n))
    assert dq.plan_rows(0, K, np.zeros(K, dtype=int), None, None, NG, True, 'm4b_sg')[1].tolist() == [0, 0, 0, 0]


def test_row_plan_refusals_keep_their_texts():
    n, K = 6, 3
    sizes, ind, j_ind = np.array([2, 0, 4]), np.array([0, 0, 2, 2, 2, 2]), np.array([1, 2, 1, 2, 3, 3])

    def plan(site_sizes=None, site_ind=None, j=j_ind, single=False):
        return dq.plan_rows(n, K, site_sizes, site_ind, j, NG, single, 'm4b_sg' if single else 'm4b')
    with pytest.raises(ValueError, match=r"`site_sizes`: 3 non-negative counts that add up to the rows of `X_new`"):
        plan(site_sizes=np.array([2, 1, 4]))
    with pytest.raises(ValueError, match=r"`site_sizes`: 3 non-negative counts"):
        plan(site_sizes=np.array([7, -1, 0]))
    with pytest.raises(ValueError, match=r"`site_ind`: one site index in \[0, 3\) per row of `X_new`"):
        plan(site_ind=np.array([0, 0, 2, 2, 2, 3]))
    with pytest.raises(ValueError, match=r"`site_ind`: one site index"):
        plan(site_ind=ind.astype(np.float64))
    with pytest.raises(ValueError, match=r"site model 'm4b_sg' holds one group per site: it takes no `j_ind`"):
        plan(site_sizes=sizes, single=True)
    with pytest.raises(ValueError, match=r"site model 'm4b' holds several groups per site: give the 1-based group of every "
                                         r"new row within its site as `j_ind`"):
        plan(site_sizes=sizes, j=None)
    with pytest.raises(ValueError, match=r"`j_ind`: one integer per row of `X_new`"):
        plan(site_sizes=sizes, j=j_ind[:-1])
    with pytest.raises(ValueError, match=r"`j_ind` of row 3: group 4 outside 1..3 of site 2"):
        plan(site_ind=ind[::-1].copy(), j=np.array([3, 3, 2, 4, 2, 1]))
    assert plan(site_sizes=sizes)[2].tolist() == [0, 1, 0, 1, 2, 2]
