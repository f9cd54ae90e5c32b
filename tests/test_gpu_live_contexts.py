"""The one-context rule of the gated stages (plan_stages: a staged job gates only while its context is the only one alive on its device, unless
WGBSSEG_STAGE_GATE_SHARED is set) and the count behind it, kept across create and destroy.

The count is process-wide, so the scenario must begin in a process with no context alive at all: this module holds no module-scoped context,
and its test runs `scenario()` in a fresh Python process (this file run as a program) — inside the suite's own process a context that any earlier
module still holds would decide the form.  Borders, windows and back-pointers are the oracle's in every form (tests/intermediates.py), bit for bit.
"""
import os
import os.path as op
import subprocess
import sys

import numpy as np
import pytest

HERE = op.dirname(op.abspath(__file__))
if __name__ == '__main__':                                     # (under pytest conftest.py has put both on the path)
    sys.path[:0] = [op.dirname(HERE), HERE]

import cases
import intermediates as im
import staging
from wgbs_tools_amd import _lib

pytestmark = pytest.mark.gpu

CHUNKS = [(37, 577), (4131, 1025), (123, 65), (9001, 257)]      # 1 (mod 64) sites, the longest not first; bounds of three gated stages: 256, 512
PARAMS = (15.0, 60, 2000)                                      # no window beyond the narrow tiles' 60 sites


SWITCHES = ('WGBSSEG_STAGE_GATE', 'WGBSSEG_STAGE_GATE_SHARED', 'WGBSSEG_LAST_STAGE_PCT', 'WGBSSEG_DP_MODE')


def test_a_staged_job_gates_only_while_its_context_is_alone():
    """scenario() in a process of its own, with three forced stages and every other staging switch at its default"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env['WGBSSEG_FORCE_STAGES'] = '3'
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [op.abspath(__file__)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and 'live contexts: 6 runs as claimed' in r.stdout, r.stdout[-4000:]


def scenario():
    """One context, three forced stages, an all-narrow job: gated (three scored-block buffers, a last stage of 300 percent).  A second context
    on the device: the same job on the first is no longer gated (two buffers, equal stages) — and gated again once the second is closed.  The
    results are the same all three times."""
    slices, loci = cases.lean_step_world()
    exp = im.expected(slices, loci, CHUNKS, *PARAMS)
    pct = 300 if float(sum(e.cost.size for e in exp)) * len(slices) / 1025.0 <= 52500.0 else 100
    assert pct == 300
    seen = []

    def run(sg, label, live, gated):
        got = sg.segment_chunks([c[0] for c in CHUNKS], [c[1] for c in CHUNKS], *PARAMS)
        plan = staging.assert_form(sg.last_plan(), 1025, stages=3, gated=gated, last_pct=pct if gated else 100, dp_mode=0, live=live,
                                   default_gate=True, label=label)
        assert plan['all_narrow'] == 1 and plan['nbuf'] == (3 if gated else 2) and plan['n_stages'] == 3, (label, plan)
        whats = ('window', 'cum', 'back', 'cost') if gated else ('window', 'cum', 'back')      # (three ungated stages share two buffers)
        im.check_call(sg, exp, got, whats, label)
        seen.append(([np.asarray(b).tolist() for b in got], im.fetch(sg, 'back', exp).tolist()))

    with _lib.Segmenter(0) as first:
        first.set_betas(slices)
        first.set_loci(loci)
        run(first, 'alone', 1, 1)
        with _lib.Segmenter(0) as second:
            run(first, 'a second context alive', 2, 0)
            second.set_betas(slices)                           # (and the second one, used, counts the same)
            second.set_loci(loci)
            run(second, 'the second context itself', 2, 0)
            run(first, 'a second context alive and used', 2, 0)
        run(first, 'alone again', 1, 1)
    assert all(s == seen[0] for s in seen[1:])
    with _lib.Segmenter(0) as third:                           # both closed: a new context is alone
        third.set_betas(slices)
        third.set_loci(loci)
        run(third, 'a new context after both were closed', 1, 1)
    assert seen[-1] == seen[0]
    print('live contexts: %d runs as claimed' % len(seen))


if __name__ == '__main__':
    scenario()
