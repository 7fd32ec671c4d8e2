"""`Master.run` as its callers and the engine see it, on CPU with the oracle standing in for the device engine: the
sequence of engine calls that dispatch and update (tests/golden/master_run_calls.json), everything `verbose` prints
(tests/golden/master_run_verbose_<tag>.txt), and the draw-reuse state of one `run` call.

Both kinds of golden file were recorded with the spy and the scenarios of THIS file from the `method.py` of the commit
before `run` was cut into stages (tests/golden/make_golden_master_run.py rewrites them from whatever `method.py` is
checked out).  The comparison is exact, floats included: they come from the same CPU oracle and the same
arithmetic, so a difference is a changed order of operations."""

import ctypes
import inspect
import json
import os

import numpy as np
import pytest

from epstan_amd import models, reweight
from epstan_amd.method import Master
from oracle.engine_oracle import OracleEngine
import test_host_logic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

RECORDED = ('set_site_order', 'set_site_split', 'set_piece_queue', 'set_draw_reuse', 'tilted_batch', 'moments_batch',
            'force_pd', 'accept', 'set_global')


def _plain(x):
    """JSON form of an argument: arrays as lists -- but the injected draws handed to `moments_batch` (thousands of
    numbers per call, the injector's output and not `run`'s) as their shape."""
    if isinstance(x, np.ndarray):
        return {'shape': list(x.shape)} if x.size > 64 else x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, dict):
        return dict((k, _plain(x[k])) for k in sorted(x))
    if isinstance(x, ctypes.Structure):                       # (the sampler options)
        return dict((name, getattr(x, name)) for name, _ in x._fields_)
    return x


class SpyEngine(OracleEngine):
    """OracleEngine that appends [name, {argument: value}] of every RECORDED call to `calls`.  It adds what the oracle lacks:
    a piece queue and the draw-reuse switch (both only recorded), and `n_cu` / `layout` to stand for a device with
    fewer CUs than sites running the row-team kernel."""
    calls = None
    n_cu = None
    layout = None

    def set_piece_queue(self, piece_len=0, rate=None):        # (the signature of HipEngine.set_piece_queue)
        pass

    def set_draw_reuse(self, on):
        pass

    def cu_count(self):
        return OracleEngine.cu_count(self) if self.n_cu is None else self.n_cu

    def last_layout(self):
        return OracleEngine.last_layout(self) if self.layout is None else self.layout

    def team_passes(self, k0=0, count=None):
        return np.zeros(self.K - k0 if count is None else count)


def _recording(name):
    inner = getattr(SpyEngine, name)
    signature = inspect.signature(inner)

    def method(self, *args, **kwargs):
        bound = signature.bind(self, *args, **kwargs)
        bound.apply_defaults()                                # (the call as the engine receives it)
        self.calls.append([name, _plain(dict(list(bound.arguments.items())[1:]))])
        return inner(self, *args, **kwargs)
    return method


for _name in RECORDED:
    setattr(SpyEngine, _name, _recording(_name))


def spy_factory(calls, n_cu=None, layout=None, cls=SpyEngine):
    def factory(model, X, y, k_lim, **groups):
        eng = cls(model, X, y, k_lim, **groups)
        eng.calls, eng.n_cu, eng.layout = calls, n_cu, layout
        return eng
    return factory


def _sampling_master(factory, **kw):
    """The model of test_master_hands_the_schedule_of_the_next_launch_to_the_engine: the oracle's own sampler."""
    mod = models.MODELS['m1b'](4, 2, 12)
    data = mod.simulate_data(Sigma_x='rand', rng=3)
    _, _, Q0, r0 = mod.get_prior()
    return Master(mod.site_model, data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=2, iter=30,
                  _engine_factory=factory, **kw)


def _injected_master(monkeypatch, runs, factory, *args, **kw):
    monkeypatch.setattr(test_host_logic, 'factory', factory)
    return test_host_logic._master(runs, *args, **kw)


def call_traces(monkeypatch, runs):
    """Scenario -> the calls recorded while `run` ran."""
    out = {}
    for tag, kw in (('balanced', {}), ('unbalanced', {'balance_sites': False})):
        calls = []
        assert _sampling_master(spy_factory(calls), **kw).run(2, verbose=False, seed=5)[0] == 0
        out[tag] = calls
    # more sites than CUs, the row-team kernel, a site that fills the LDS: the piece queue before launch 1 and after each
    calls = []
    monkeypatch.setattr(Master, '_one_workgroup_per_cu', lambda self: True)
    assert _sampling_master(spy_factory(calls, n_cu=2, layout=7)).run(2, verbose=False, seed=5)[0] == 0
    monkeypatch.undo()
    out['piece_queue'] = calls
    calls = []
    M = _injected_master(monkeypatch, runs, spy_factory(calls), 'wide_first', 1.0, 3)
    assert M.run(4, verbose=False, return_analytics=True, seed=1)[0] == 0
    out['decay'] = calls
    calls = []                          # test_force_pd_branch
    M = _injected_master(monkeypatch, runs, spy_factory(calls), 'wide_first', 1.0, 3, df_treshold=0.9)
    assert M.run(2, verbose=False, calc_moments=False, seed=1) == 0
    out['force_pd'] = calls
    return out


# tag: scenario, iterations, df0, sites, factor, Master's further arguments, run's further arguments
VERBOSE = {
    'smooth': ('smooth', 12, 0.5, 4, 60.0, {}, {'return_analytics': True}),
    'decay': ('wide_first', 4, 1.0, 3, 60.0, {}, {'return_analytics': True}),
    'allfail': ('degenerate', 3, 0.5, 4, 60.0, {}, {'return_analytics': True}),
    'badprior': ('wide_all', 3, 1.0, 4, 400.0, {}, {'return_analytics': True}),
    'force_pd': ('wide_first', 2, 1.0, 3, 60.0, {'df_treshold': 0.9}, {'calc_moments': False}),     # test_force_pd_branch
}


def verbose_run(runs, tag):
    scenario, niter, df0, nsites, factor, master_kw, run_kw = VERBOSE[tag]
    M = test_host_logic._master(runs, scenario, df0, nsites, factor=factor, **master_kw)
    M.run(niter, verbose=True, seed=1, **run_kw)


@pytest.fixture(scope='module')
def runs(golden_dir):
    return np.load(os.path.join(golden_dir, 'master_run.npz'))


def test_engine_calls_are_those_of_the_undivided_run(monkeypatch, runs):
    with open(os.path.join(GOLDEN, 'master_run_calls.json')) as f:
        want = json.load(f)
    got = json.loads(json.dumps(call_traces(monkeypatch, runs)))       # (tuples -> lists, as the file holds them)
    assert sorted(got) == sorted(want)
    for tag in want:
        assert [c[0] for c in got[tag]] == [c[0] for c in want[tag]], tag
        for i, (g, w) in enumerate(zip(got[tag], want[tag])):
            assert g == w, (tag, i)
    # what the scenarios are there for
    names = dict((tag, [c[0] for c in got[tag]]) for tag in got)
    assert 'set_site_order' not in names['unbalanced'] and names['balanced'].count('set_site_order') == 2
    assert names['balanced'].count('set_piece_queue') == 2 and names['piece_queue'].count('set_piece_queue') == 3
    assert names['decay'].count('moments_batch') == 4 and 'tilted_batch' not in names['decay']
    assert names['force_pd'].count('force_pd') == 1


@pytest.mark.parametrize('tag', sorted(VERBOSE))
def test_verbose_prints_what_the_undivided_run_printed(capsys, runs, tag):
    # (with injected draws the times and step sizes printed are the injector's constants: no line is masked)
    verbose_run(runs, tag)
    with open(os.path.join(GOLDEN, 'master_run_verbose_%s.txt' % tag), newline='') as f:
        assert capsys.readouterr().out == f.read()


class ReweightingSpy(SpyEngine):
    """Every site passes `reuse_ok`; the tilted moments stay those of the last launch."""
    RW_MS = 3.5

    def num_draws(self):
        return 60

    def reweight_batch(self, prec_estim, k0=0, count=None):
        self.calls.append(['reweight_batch', {'prec_estim': prec_estim}])
        rec = np.zeros((self.K, 2))
        rec[:, reweight.RW_KHAT], rec[:, reweight.RW_WESS] = 0.1, self.num_draws()
        return np.ones(self.K, dtype=bool), rec, self.RW_MS


def test_reuse_state_lives_for_one_run_call():
    calls = []
    M = _sampling_master(spy_factory(calls, cls=ReweightingSpy))
    count = lambda name: sum(c[0] == name for c in calls)
    for n in (1, 2):                    # every call samples in its first iteration: no draws are carried over
        assert M.run(1, verbose=False, seed=5, reuse=True)[0] == 0
        assert (count('tilted_batch'), count('reweight_batch')) == (n, 0)
        assert [e['reused'] for e in M.reuse_log] == [False]
    info, _, (stimes, msteps, mrhats, _) = M.run(2, verbose=False, seed=6, reuse=True, return_analytics=True)
    assert info == 0 and (count('tilted_batch'), count('reweight_batch')) == (3, 1)
    assert [c[0] for c in calls if c[0] in ('tilted_batch', 'reweight_batch')][-2:] == ['tilted_batch', 'reweight_batch']
    assert [e['reused'] for e in M.reuse_log] == [False, True] and M.reuse_log[1]['n_ok'] == M.K
    assert msteps[1] == msteps[0] and mrhats[1] == mrhats[0] and stimes[1] == ReweightingSpy.RW_MS * 1e-3
    assert count('set_draw_reuse') == 3

