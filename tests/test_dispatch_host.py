"""dispatch.py: how the next sampling launch is dispatched.  Draws do not depend on it, so nothing else in the suite
fails when the policy is wrong -- only the benchmark gets slower.  Pure functions: no engine, no GPU."""

import numpy as np
import pytest

from epstan_amd import dispatch

# a rank on which the piece queue pays: more sites than CUs, one workgroup per CU
RANK = dispatch.Rank(balance=True, has_queue=True, K_local=300, n_cu=256, one_wg=True, iter=200, pieces_per_site=16,
                     lead_fraction=dispatch.LEAD_FRACTION)


def _even_work(K=300, chains=4, leapfrogs=1e5):
    """Every site about equally slow: site_schedule singles none out (n_lead == 0)."""
    lf = np.full((K, chains), leapfrogs)
    return lf.sum(axis=1), lf


@pytest.mark.parametrize('D,n_max,want', [(32, 320, False), (32, 321, True), (17, 321, True), (16, 640, False),
                                          (16, 641, True), (33, 1, True)])
def test_one_workgroup_per_cu_at_its_edges(D, n_max, want):
    # 320 rows x 32 padded columns x 8 bytes = 81920 = 80 KB: not MORE than half of the LDS
    assert dispatch.one_workgroup_per_cu(D, n_max) is want


def test_piece_len():
    assert [dispatch.piece_len(it, 16) for it in (1, 15, 16, 17, 200)] == [1, 1, 1, 1, 12]


def test_first_launch_needs_every_condition():
    assert dispatch.first_launch(RANK, launched=False) == (12, None)
    assert dispatch.first_launch(RANK._replace(balance=False), launched=False) is None
    assert dispatch.first_launch(RANK, launched=True) is None
    assert dispatch.first_launch(RANK._replace(has_queue=False), launched=False) is None
    assert dispatch.first_launch(RANK._replace(K_local=256), launched=False) is None
    assert dispatch.first_launch(RANK._replace(one_wg=False), launched=False) is None


def test_next_launch_hands_nothing_over_without_balancing_or_with_one_site():
    passes, lf = _even_work()
    assert not dispatch.schedules(RANK._replace(balance=False)) and not dispatch.schedules(RANK._replace(K_local=1))
    assert dispatch.next_launch(RANK._replace(balance=False), 7, passes, lf) is None
    assert dispatch.next_launch(RANK._replace(K_local=1), 7, passes[:1], lf[:1]) is None


def test_next_launch_clears_the_queue_where_it_does_not_pay():
    passes, lf = _even_work()
    for rank, layout in ((RANK, 1), (RANK._replace(K_local=256), 7), (RANK._replace(one_wg=False), 7)):
        K = rank.K_local
        launch = dispatch.next_launch(rank, layout, passes[:K], lf[:K])
        assert launch.piece == (0, None) and launch.n_lead == 0 and sorted(launch.order) == list(range(K))
    # lead sites: the split launch takes the queue's place
    lf = lf.copy()
    lf[7] = [900, 5e6, 800, 700]
    launch = dispatch.next_launch(RANK, 7, lf.sum(axis=1), lf)
    assert launch.n_lead == 1 and launch.order[0] == 7 and launch.piece == (0, None)
    assert sorted(launch.order) == list(range(300))


@pytest.mark.parametrize('layout', [5, 7, 3])
def test_next_launch_queues_pieces_with_the_measured_rates(layout):
    passes, lf = _even_work()
    lf = lf.copy()
    lf[:, 1] += np.arange(300)              # the slowest chain differs by site
    lf[11] = 0.0                            # a site that took no leapfrog step: its rate is that of one step
    launch = dispatch.next_launch(RANK, layout, passes, lf)
    assert launch.n_lead == 0 and sorted(launch.order) == list(range(300))
    plen, rate = launch.piece
    assert plen == max(1, 200 // 16) == 12
    want = (1e5 + np.arange(300)) / 200
    want[11] = 1.0 / 200
    np.testing.assert_array_equal(rate, want)
    np.testing.assert_array_equal(rate, np.maximum(lf.max(axis=1), 1.0) / 200)
    assert dispatch.next_launch(RANK._replace(iter=10), layout, passes, lf).piece[0] == 1


def test_next_launch_for_an_engine_without_a_piece_queue():
    passes, lf = _even_work()
    launch = dispatch.next_launch(RANK._replace(has_queue=False), 7, passes, lf)
    assert launch.piece is None and launch.n_lead == 0 and sorted(launch.order) == list(range(300))


def test_site_schedule_puts_the_slow_sites_first():
    """The two cases of test_host_logic.py's test of `Master._site_schedule`, on the function itself."""
    lf = np.full((40, 4), 1000.0)
    lf[7] = [900, 50000, 800, 700]          # one slow chain
    lf[3] = [30000, 30000, 30000, 30000]    # all slow
    lf[20] = [5000, 5000, 5000, 5000]       # heavy, but not near the slowest
    order, n_lead = dispatch.site_schedule(lf.sum(axis=1), lf)
    assert n_lead == 2 and list(order[:3]) == [7, 3, 20]
    assert sorted(order) == list(range(40))
    # every site about equally slow (first iteration): nothing to single out
    order, n_lead = dispatch.site_schedule(np.full(40, 4e5), np.full((40, 4), 1e5))
    assert n_lead == 0 and sorted(order) == list(range(40))
    # the lead fraction is the caller's (Master.LEAD_FRACTION): above 1 no site leads
    assert dispatch.site_schedule(lf.sum(axis=1), lf, lead_fraction=2.0)[1] == 0
