#!/usr/bin/env python3
"""Golden text of `wgbstools beta_to_450k` from the REFERENCE ITSELF: runs only in the build container.  Imports
/root/reference/src/python/beta_to_450k.py from where it lies and runs its main() — process pool, pandas merge and to_csv as they
are — on every case of tests/array_cases.py.  Its GenomeRefPaths is replaced by a stand-in over the synthetic worlds that answers
what the command asks: the genome's name (hg38, so that the map's rows without a cpg are dropped as for that genome), the path of
ilmn2CpG.tsv.gz and the number of sites.

Recorded per case: the text (above FULL_TEXT bytes its sha1, byte and line counts and first and last three lines), what the
reference said on stderr with the map file's path replaced by {MAP}, or the refusal's message.  Every recorded text and warning
is also held against tests/array_ref.py's restatement here, so a disagreement shows when the fixture is made.

Usage:  python tests/golden/make_golden_450k.py
"""
import contextlib
import hashlib
import io
import json
import os.path as op
import shutil
import sys
import tempfile

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(op.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))
sys.path.insert(0, '/root/reference/src/python')

import array_cases as AC                        # noqa: E402
import array_ref as AR                          # noqa: E402

FULL_TEXT = 24 << 10


def record(text):
    lines = text.split(b'\n')[:-1]
    if len(text) <= FULL_TEXT:
        return {'text': text.decode()}
    return {'sha1': hashlib.sha1(text).hexdigest(), 'bytes': len(text), 'lines': len(lines),
            'first': [ln.decode() for ln in lines[:3]], 'last': [ln.decode() for ln in lines[-3:]]}


def main():
    import beta_to_450k as rb
    from utils_wgbs import IllegalArgumentError
    td = tempfile.mkdtemp()
    worlds = AC.worlds()
    where = {name: AC.write_world(td, name, w) for name, w in worlds.items()}

    class FakeGenome:
        def __init__(self, name=None):
            self.world = op.basename(op.dirname(op.dirname(name)))     # .../<world>/references/hg38
            self.genome = 'hg38'
            self.ilmn2cpg_dict = where[self.world]['map']

        def get_nr_sites(self):
            return int(sum(worlds[self.world]['sizes']))

    rb.GenomeRefPaths = FakeGenome
    fixture = {'seed': AC.SEED, 'full_text_up_to': FULL_TEXT, 'map_placeholder': AR.MAP, 'cases': {}}
    try:
        for name, case in AC.cases().items():
            w, d = worlds[case['world']], where[case['world']]
            out = op.join(td, 'out.csv')
            entry = {}
            err = io.StringIO()
            sys.argv = ['beta_to_450k'] + AC.argv_of(case, where, out) + ['-@', '2']
            try:
                with contextlib.redirect_stderr(err):
                    rb.main()
            except IllegalArgumentError as e:
                entry['error'] = ' '.join(str(a) for a in e.args)
            said = err.getvalue().replace(d['map'], AR.MAP)
            entry['stderr'] = said
            if 'error' not in entry:
                with open(out, 'rb') as f:
                    text = f.read()
                ours, warnings = AR.case_text(w, case, d['map'], op.join(d['dir'], case['ref']) if case['ref'] else None, AC.case_paths(case, where),
                                              AC.case_rows(case, w))
                assert ours == text, (name, 'tests/array_ref.py disagrees with the reference', ours[:300], text[:300])
                assert ''.join(x + '\n' for x in warnings) == said, (name, warnings, said)
                entry.update(record(text))
            fixture['cases'][name] = entry
            print('==', name, entry.get('error') or '%d bytes' % len(text), '| stderr: %d bytes' % len(said))
    finally:
        shutil.rmtree(td, ignore_errors=True)
    path = op.join(HERE, 'array_cases.json')
    with open(path, 'w') as f:
        json.dump(fixture, f, indent=0)
    print('wrote array_cases.json (%.0f KB)' % (op.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
