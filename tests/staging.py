"""The staging form of a segment call, as Segmenter.last_plan() reports it, against what the switches of the test ask for.

`expected_bounds` restates plan_stages' rule for the stage bounds (wgbsseg.hip): `forced` stages, cut to one per 64 sites of the longest
chunk; equal stages of S sites, S a multiple of 64, but the last, which is last_pct percent of the others'; no empty stage.  `assert_form`
checks a reported plan against it and against the rules that hang on the form: the number of scored-block buffers (3 only for a gated job of
more than two stages), the last stage's length (100 percent unless gated), k_dp16 in every stage but the last of a staged job in recurrence
mode 0, no medium or wide tile in an all-narrow job.  A test that forces a form calls it with the form it claims.
"""
import math


def expected_bounds(max_len, forced, last_pct=100):
    """-> the n_stages + 1 stage bounds of a job whose longest chunk has max_len sites under WGBSSEG_FORCE_STAGES=forced"""
    n = min(int(forced), max(1, (max_len + 63) // 64))
    parts = (n - 1) + last_pct / 100.0 if n > 1 else 1.0
    S = (int(math.ceil(max_len / parts)) + 63) // 64 * 64
    n = min(n, (max_len + S - 1) // S)
    return [min(q * S, max_len) for q in range(n)] + [max_len]


def auto_dp_mode(max_window):
    """the recurrence build the launcher picks by the job's widest window (WGBSSEG_DP_MODE can only raise it)"""
    return 2 if max_window > 512 else (1 if max_window > 64 else 0)


def assert_form(plan, max_len, stages=None, gated=None, last_pct=None, dp_mode=None, live=None, default_gate=False, label=''):
    """plan: Segmenter.last_plan().  stages: WGBSSEG_FORCE_STAGES (None: the launcher's own choice, where only a one-stage plan's bounds are
    known here).  gated / last_pct / dp_mode / live (contexts alive): what the test claims; None: not claimed, only the rules between the
    fields are checked.  default_gate: the context has the default gate switches, where an all-narrow staged job gates exactly when its context
    is alone on the device.  -> plan"""
    say = '%s%s' % (label and label + ': ', plan)
    n = plan['n_stages']
    assert n >= 1 and len(plan['bounds']) == n + 1 and len(plan['dp16']) == n and len(plan['stage_tiles']) == n, say
    assert plan['gated'] in (0, 1) and plan['all_narrow'] in (0, 1) and plan['live_contexts'] >= 1, say
    if gated is not None:
        assert plan['gated'] == int(gated), say
    if live is not None:
        assert plan['live_contexts'] == live, say
    if not plan['gated']:
        assert plan['last_pct'] == 100, say
    if last_pct is not None:
        assert plan['last_pct'] == last_pct, say
    else:
        assert plan['last_pct'] in (100, 300), say               # the launcher's own two choices
    if stages is not None:
        assert plan['bounds'] == expected_bounds(max_len, stages, plan['last_pct']), say
    elif n == 1:
        assert plan['bounds'] == [0, max_len], say
    b = plan['bounds']
    assert b[0] == 0 and b[-1] == max_len and all(x < y for x, y in zip(b, b[1:])) and all(x % 64 == 0 for x in b[:-1]), say
    assert plan['nbuf'] == (1 if n == 1 else (3 if plan['gated'] and n > 2 else 2)), say
    if dp_mode is not None:
        assert plan['dp_mode'] == dp_mode, say
    assert plan['dp16'] == [int(plan['dp_mode'] == 0 and s + 1 < n) for s in range(n)], say
    if default_gate and n > 1:
        if plan['all_narrow']:
            assert plan['gated'] == int(plan['live_contexts'] == 1), say
        elif plan['gated']:
            assert plan['live_contexts'] == 1, say
    tiles = plan['stage_tiles']
    assert all(t >= 0 for row in tiles for t in row) and all(sum(row) > 0 for row in tiles), say     # (the longest chunk has sites in every stage)
    if plan['all_narrow']:
        assert all(row[1] == 0 and row[2] == 0 for row in tiles), say
    return plan
