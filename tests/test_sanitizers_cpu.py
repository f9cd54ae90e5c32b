"""Sanitizer builds of the host-side native code (the reference has none; its `segmentor` has a real UB at max_bp == 0):
csrc/block_plan.h (the plan of a block reduction), csrc/share_plan.h (the plan of a share group, its router, its take rule), csrc/bimodal_plan.h + csrc/homog_plan.h + csrc/stats_plan.h (the plans of test_bimodal, homog and sample_stats), csrc/stitch.h + csrc/add_loci.h (chunk grid, junction stitching on the thread pool, BED rows)
and the oracle's C restatement of the
chunk DP, each compiled plain, with AddressSanitizer + UndefinedBehaviorSanitizer, and with ThreadSanitizer, and run on
deterministic toy inputs: every build must finish clean and print the same lines."""
import os.path as op
import platform
import re
import shutil
import subprocess

import pytest

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
NATIVE = op.join(ROOT, 'tests', 'native')
FLAVOURS = {'plain': [], 'asan_ubsan': ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'tsan': ['-fsanitize=thread']}


def _have(flags):
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null'] + flags, input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


def _no_aslr():
    """ThreadSanitizer of older toolchains stops at start ("unexpected memory mapping") under the larger mmap randomisation of newer
    kernels: its runs go without address-space randomisation, for that process alone, where setarch can arrange it."""
    sa = shutil.which('setarch')
    if sa and subprocess.run([sa, platform.machine(), '-R', 'true'], capture_output=True).returncode == 0:
        return [sa, platform.machine(), '-R']
    return []


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, '%s\n%s\n%s' % (' '.join(cmd), r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


@pytest.mark.skipif(not _have(FLAVOURS['asan_ubsan']) or not _have(FLAVOURS['tsan']), reason='no g++ with sanitizer runtimes')
def test_stitching_and_bed_rows_under_sanitizers(tmp_path):
    outs = {}
    for name, flags in FLAVOURS.items():
        exe = str(tmp_path / ('san_host_' + name))
        _run(['g++', '-std=c++17', '-O1', '-g', '-pthread', '-I', op.join(ROOT, 'wgbs_tools_amd', 'csrc'), op.join(NATIVE, 'san_host.cpp'), '-o', exe] + flags)
        for threads in ('1', '4'):
            bed = str(tmp_path / ('%s_%s.bed' % (name, threads)))
            text = _run((_no_aslr() if name == 'tsan' else []) + [exe, threads, bed], env={'TSAN_OPTIONS': 'halt_on_error=1', 'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'})
            outs[(name, threads)] = (text, open(bed, 'rb').read())
    ref = outs[('plain', '1')]
    assert 'checksum' in ref[0] and ref[0].count('world') == 15 and 'rc 0' in ref[0] and len(ref[1]) > 5000
    plan_line = [l for l in ref[0].splitlines() if l.startswith('block_plan: ')]
    assert len(plan_line) == 1 and ', 14 plans, 10 refusals, checksum ' in plan_line[0]          # (identical across the builds: the loop below compares whole outputs)
    share_line = [l for l in ref[0].splitlines() if l.startswith('share_plan: ')]
    assert len(share_line) == 1
    m = re.match(r'share_plan: (\d+) plans, (\d+) idle shares, (\d+) chunks routed to their owners, (\d+) junction ranges routed, (\d+) unroutable, (\d+) routes by hand, '
                 r'(\d+) refusals, take rule: (\d+) items in (\d+) sub-batches of 3 walks, (\d+) mismatches, checksum ', share_line[0])
    plans, idle, chunks, routed, unroutable, by_hand, refusals, items, subs, mismatches = (int(x) for x in m.groups())
    # the program's worlds: (regions, sites of the first region - region r has 37 r more -, chunk); each planned for 6 share counts, even | weighted, 2 halos
    worlds, counts = [(7, 40000, 5000), (5, 30000, 3000), (1, 9000, 700), (3, 500, 60000)], (1, 2, 3, 5, 8, 64)
    n_chunks = sum(-(-(n + 37 * r) // c) for k, n, c in worlds for r in range(k))
    assert plans == len(worlds) * len(counts) * 4 and refusals == 6 and by_hand == 18 and mismatches == 0
    assert chunks == n_chunks * len(counts) * 4                    # every chunk of every plan, each routed to the share that owns it
    # two ranges (+-50, +-5000 sites) at every boundary between two shares that own chunks
    assert routed + unroutable == 2 * (len(worlds) * 4 * sum(counts) - idle - plans)
    # 64 shares over at most 62 chunks and the zero weights leave shares idle; the +-50 ranges outgrow the halo of 10; the middle share of three takes
    # two items per chunk and four junction ranges, in more than one sub-batch per walk and (min_take 1: one per distinct last site) fewer than items per walk
    assert idle >= len(worlds) * 4 * 2 and routed > 0 and unroutable > 0 and items > 4 and items % 2 == 0 and 3 < subs < 3 * items
    # the plans of the pat engines and of sample_stats: 5 fixed and 200 seeded block tables (test_bimodal: every block of every table retired once, by
    # the feed's walk or at the end), 6 + 424 + 200 range lists for both row widths; every refusal refused
    pat = {l.split(':')[0]: l for l in ref[0].splitlines() if l.split(':')[0] in ('bimodal_plan', 'homog_plan', 'stats_plan')}
    m = re.match(r'bimodal_plan: 205 plans, (\d+) blocks retired, 5 refusals, 0 mismatches, checksum ', pat['bimodal_plan'])
    assert m and int(m.group(1)) > 205 * 5
    assert pat['homog_plan'].startswith('homog_plan: 205 plans, 8 refusals, 0 mismatches, checksum ')
    assert pat['stats_plan'].startswith('stats_plan: %d plans, 6 refusals, 0 mismatches, checksum ' % (2 * (6 + sum(34 - a for a in range(16)) + 200)))
    assert 'sitetable: ' in ref[0] and 'mismatches 0, concurrent misses 0' in ref[0]
    assert 'parse_blocks: rc 0 rows 40000 na 413' in ref[0] and 'parse_blocks on a float field: rc 1' in ref[0]
    assert ref[0].count('write_table pass') == 2 and 'DIFFERS' not in ref[0] and 'write_bedgraph: rc 0' in ref[0]
    assert 'parse_bed: rc 0 rows 50000 width 6 unknown 237' in ref[0] and 'parse_bed on a float column: rc 1' in ref[0] and 'write_annotated_bed: rc 0' in ref[0]
    for key, val in outs.items():
        assert val == ref, key
    # with and without speculation the same world gives the same borders
    lines = [l for l in ref[0].splitlines() if 'fuzzy=40' in l]
    assert len({l.split('checksum')[1] for l in lines}) == 1


@pytest.mark.skipif(not _have(FLAVOURS['asan_ubsan']) or not _have(FLAVOURS['tsan']), reason='no gcc with sanitizer runtimes')
def test_oracle_restatement_under_sanitizers(tmp_path):
    outs = {}
    for name, flags in FLAVOURS.items():
        exe = str(tmp_path / ('san_oracle_' + name))
        _run(['gcc', '-std=c99', '-O1', '-g', '-ffp-contract=off', '-pthread', op.join(NATIVE, 'san_oracle.c'), op.join(ROOT, 'oracle', 'segment_oracle.c'),
              op.join(ROOT, 'oracle', 'libm_probe.c'), '-o', exe, '-lm'] + flags)
        outs[name] = _run((_no_aslr() if name == 'tsan' else []) + [exe], env={'TSAN_OPTIONS': 'halt_on_error=1', 'PATH': '/usr/bin:/bin'})
    assert 'DIFFERENT' not in outs['plain'] and outs['plain'].count('identical') == 7 and 'bad data: rc' in outs['plain']
    assert outs['asan_ubsan'] == outs['plain'] and outs['tsan'] == outs['plain']
