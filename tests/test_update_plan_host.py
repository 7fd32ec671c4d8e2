"""(no device) What the update stage decides without a HIP call, csrc/epx_update.h, through tests/update_plan_probe.hip: a
small host program that prints what the pure functions decide.

 * DensePlan: where the dense kernels keep their work matrices, against the closed forms -- ld = d | 1, a block slot of
   2 d ld + 4 ld doubles, in dynamic LDS while slot * 8 + 1024 bytes fit the CU's 160 KB (d <= 99), else one slot per block
   of a global workspace.
 * TrialStats: the statistics block behind the packed sums of epx_update_trial -- both refusals, where a rank's values
   go, and what comes back from the reduced block.

CASES lists every call of the probe with the line it has to print, so that the same calls can be repeated with a build of
the probe under a host sanitizer."""

import subprocess

import pytest

from test_tree_endings_cases import _build_probe

LDS_BYTES = 160 * 1024
STAT_CAP, PACKED_EXTRA = 8, 1024


def _plan_line(d, nblocks):
    ld = d | 1
    slot = 2 * d * ld + 4 * ld
    in_lds = slot * 8 + 1024 <= LDS_BYTES
    return '%d %d %d %d %d' % (ld, slot, in_lds, slot * 8 if in_lds else 0, 0 if in_lds else slot * nblocks)


def _hex(values):
    return ' '.join(float(v).hex() for v in values)


def _cases():
    cases = [(['plan', d, nb], _plan_line(d, nb)) for d in (1, 2, 34, 98, 99, 100, 258) for nb in (1, 7)]
    few = 'refused at most %d statistics of a kind' % STAT_CAP
    cases += [(['stats', 9, 0, 1, 0], few), (['stats', 0, 9, 1, 0], few), (['stats', -1, 0, 1, 0], few),
              (['stats', 8, 8, 1, 0], 'ok 16 8 %d' % (PACKED_EXTRA - 3)),
              (['stats', 0, 0, 1, 0], 'ok 0 0 %d' % (PACKED_EXTRA - 3)),
              # n_sum + n_max * ranks + 3 against the block of 1024: 5 + 8 * 127 + 3 fills it, 6 + 8 * 127 + 3 does not fit
              (['stats', 5, 8, 127, 126], 'ok 1021 1013 %d' % (PACKED_EXTRA - 3)),
              (['stats', 6, 8, 127, 0], 'refused too many ranks (127) for the statistics block'),
              (['stats', 8, 8, 126, 3], 'ok 1016 32 %d' % (PACKED_EXTRA - 3)),
              (['stats', 8, 8, 128, 0], 'refused too many ranks (128) for the statistics block')]
    # rank 2 of 3 with two sums and three maxima: [sums | rank 0 | rank 1 | rank 2], the other ranks' slots zero
    cases.append((['pack', 2, 3, 3, 2, 1.5, -2.25, 7.0, -0.0, -3.0], _hex([1.5, -2.25] + [0.0] * 6 + [7.0, -0.0, -3.0])))
    cases.append((['pack', 2, 3, 3, 0, 1.5, -2.25, 7.0, -0.0, -3.0], _hex([1.5, -2.25, 7.0, -0.0, -3.0] + [0.0] * 6)))
    cases.append((['pack', 0, 0, 1, 0], ''))
    # the reduced block: sums as they are; per statistic the largest of the rank slots -- in the middle rank, in the last,
    # a -0.0 above negative ones, and an all-negative column
    block = [4.0, -0.5,
             1.0, -1.0, -7.0, -3.0,
             9.0, -0.0, -2.0, -4.0,
             2.0, -5.0, -2.5, -1.5]
    cases.append((['unpack', 2, 4, 3] + block, _hex([4.0, -0.5, 9.0, -0.0, -2.0, -1.5])))
    cases.append((['unpack', 1, 2, 1, 3.0, -6.0, 0.25], _hex([3.0, -6.0, 0.25])))
    cases += [(['first_bad', 1e17], '-1'), (['first_bad', 5.0], '5'), (['first_bad', 0.0], '0'), (['first_bad', 3e17], '-1'),
              (['first_bad', 99999999999999984.0], '99999999999999984')]          # (the double just below 1e17)
    return [([repr(a) if isinstance(a, float) else str(a) for a in args], want) for args, want in cases]


CASES = _cases()


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    return _build_probe(tmp_path_factory.mktemp('update_plan'), 'update_plan_probe')


def test_closed_forms_of_the_dense_plan():
    """The figures the cases rest on: the last dimension in LDS is 99 with 159 984 B, the first in the workspace 100."""
    assert _plan_line(99, 7) == '99 19998 1 159984 0'
    assert _plan_line(100, 7) == '101 20604 0 0 %d' % (20604 * 7)
    assert 20604 * 8 + 1024 == 165856 > LDS_BYTES >= 159984 + 1024


def _line(out):
    """The probe's line, its %a doubles in float.hex's spelling (every bit, the sign of a zero included)."""
    return ' '.join(float.fromhex(w).hex() if w.lstrip('-').startswith('0x') else w for w in out.decode().rstrip('\n').split(' '))


def test_update_plan_cases(probe):
    for args, want in CASES:
        assert _line(subprocess.check_output([probe] + args)) == want, args
