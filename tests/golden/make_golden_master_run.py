"""Records tests/golden/master_run_calls.json and master_run_verbose_<tag>.txt with the spy engine and the scenarios of
tests/test_master_run_stages_host.py from the `ep-stan_amd/method.py` that is checked out.  The committed files were
recorded at the commit before `Master.run` was cut into stages; the test holds every later `run` to them.

    python tests/golden/make_golden_master_run.py
"""

import contextlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    sys.path.insert(0, p)

import numpy as np
import pytest

import test_master_run_stages_host as stages

mp = pytest.MonkeyPatch()
runs = np.load(os.path.join(HERE, 'master_run.npz'))
with open(os.path.join(HERE, 'master_run_calls.json'), 'w') as f:
    traces = stages.call_traces(mp, runs)                   # one call per line
    f.write('{\n%s\n}\n' % ',\n'.join('"%s": [\n%s\n]' % (tag, ',\n'.join(json.dumps(c) for c in traces[tag]))
                                     for tag in sorted(traces)))
mp.undo()
for tag in stages.VERBOSE:
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        stages.verbose_run(runs, tag)
    with open(os.path.join(HERE, 'master_run_verbose_%s.txt' % tag), 'w', newline='') as f:
        f.write(out.getvalue())
