"""How the next sampling launch is dispatched, decided from the work of the last one: the site order, the lead sites of
a split launch and the piece queue.  Pure functions of numbers and arrays -- `Master._apply_dispatch` hands what they
return to the engine.  Draws are the same under any dispatch (include/epx.h: epx_set_site_order, epx_set_site_split,
epx_set_piece_queue), so a mistake here costs time and changes no result: tests/test_dispatch_host.py pins the policy."""

from collections import namedtuple

import numpy as np

# a site whose slowest chain took more than this fraction of the iteration's slowest chain is
# scheduled one workgroup per chain next time (measured leapfrog: 5.6 vs 10.3 us at D=32, n=500)
LEAD_FRACTION = 0.4

# What no launch changes: `balance` (Master's `balance_sites`), `has_queue` (the engine has a piece queue), the rank's
# sites and the device's CUs, `one_wg` (one_workgroup_per_cu of the rank's largest site), the sampler's iterations per
# site, the pieces a site's run is cut into and the lead fraction (Master's PIECES_PER_SITE and LEAD_FRACTION).
Rank = namedtuple('Rank', 'balance has_queue K_local n_cu one_wg iter pieces_per_site lead_fraction')

# The dispatch of one launch.  `piece`: (piece_len, rate) of the piece queue, (0, None) to clear it, None where the
# engine has none.
Launch = namedtuple('Launch', 'order n_lead piece')


def site_schedule(passes, chain_leapfrogs, n_cu=256, lead_fraction=LEAD_FRACTION):
    """Dispatch order and number of lead sites for the next sampling launch from the work of
    this one.  A launch ends with its slowest chain, and which sites hold the slow chains is
    stable from one EP iteration to the next (a property of the site's posterior geometry:
    measured rank correlation 0.96-0.98 at C3), so the sites within `lead_fraction` of the
    slowest come first, ordered by their slowest chain, and run at the shorter leapfrog of
    one workgroup per chain (engine.set_site_split); the others follow longest-first."""
    chain_leapfrogs = np.asarray(chain_leapfrogs)
    site_max = chain_leapfrogs.max(axis=1)
    lead = np.where(site_max > lead_fraction * site_max.max())[0]
    # no tail to speak of: many sites near the slowest, or enough work to keep every CU (one
    # site, i.e. up to 4 chains, each) busy for most of the slowest chain's run anyway
    busy = site_max.sum() / n_cu
    if lead.size * 4 > site_max.size or busy > 0.7 * site_max.max():
        lead = lead[:0]
    lead = lead[np.argsort(-site_max[lead], kind='stable')]
    rest = np.setdiff1d(np.arange(site_max.size), lead)
    rest = rest[np.argsort(-np.asarray(passes)[rest], kind='stable')]
    return np.concatenate((lead, rest)).astype(np.int32), int(lead.size)


def one_workgroup_per_cu(D, n_max):
    """The resident sampler keeps a site's rows (padded to 16 / 32 columns) in LDS: above half of the 160 KB
    only one workgroup fits a CU; the streaming sampler (D > 32, or rows beyond the LDS) always fills it.  Then
    a pieced launch (one resident workgroup per CU, looping over pieces) loses nothing to occupancy."""
    if D > 32:
        return True
    return n_max * (16 if D <= 16 else 32) * 8 > 80 * 1024


def piece_len(iter, pieces_per_site):
    return max(1, iter // pieces_per_site)


def _queue_pays(rank):
    """When a site fills the LDS (one workgroup per CU) and there are more sites than CUs: run the sampler from a piece
    queue -- looping workgroups claim pieces of a site's transitions, the site with the largest predicted remaining
    work first (same draws; only the dispatch changes)."""
    return rank.K_local > rank.n_cu and rank.one_wg


def first_launch(rank, launched):
    """The piece queue of a launch without history (`launched`: this Master has sampled before): equal predicted work
    per transition (the library ignores it when the launch does not run the row-wave / state-wave kernel).  Returns
    (piece_len, None), or None: leave the engine as it is."""
    if rank.balance and not launched and rank.has_queue and _queue_pays(rank):
        return piece_len(rank.iter, rank.pieces_per_site), None
    return None


def schedules(rank):
    """Whether `next_launch` has anything to say (its caller need not read the launch's statistics otherwise)."""
    return rank.balance and rank.K_local > 1


def next_launch(rank, layout, passes, leapfrogs):
    """After a launch of `layout` that took `passes` (K_local) row passes and `leapfrogs` (K_local, chains) leapfrog
    steps: the `Launch` of the next one (longest-first; results unaffected), or None: leave the engine as it is."""
    if not schedules(rank):
        return None
    order, n_lead = site_schedule(passes, leapfrogs, rank.n_cu, rank.lead_fraction)
    piece = None
    if rank.has_queue:
        piece = (0, None)
        if layout in (5, 7, 3) and n_lead == 0 and _queue_pays(rank):
            piece = (piece_len(rank.iter, rank.pieces_per_site), np.maximum(leapfrogs.max(axis=1), 1.0) / rank.iter)
    return Launch(order, n_lead, piece)
