#!/usr/bin/env python3
"""An hg19-shaped FASTA file laid out from the benchmark's synthetic loci (synth.genome_shape / synth_loci): CG at every locus, a CG-free
filler elsewhere, every chromosome 10,000 bases longer than its last locus, lines of --width bases.  With the defaults: 25 chromosomes,
28,217,448 CpGs, about 3.1 GB of text.  `wgbstools init_genome` must give back exactly these loci (tools/bench_init_genome.py checks it).

    python tools/make_fasta.py out.fa [--sites N] [--width 60] [--seed S] [--bgzf out.fa.gz]

--bgzf: the same text as BGZF as well, the members deflated on the GPU (_lib.bgzf_deflate), 255 members' worth of text at a time."""
import argparse
import json
import os.path as op
import sys
import time

import numpy as np

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261021
FILLER = b'ATTA'                                                    # no C: a filler byte never makes a site with its neighbour
MEMBER = 65280
BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def chromosome_text(name, sub, width):
    """the record of one chromosome: CG at the loci `sub` (1-based, ascending, no two adjacent)"""
    sub = np.asarray(sub, dtype=np.int64)
    assert sub.size == 0 or (np.diff(sub) >= 2).all(), 'adjacent loci cannot both be CpGs'
    n = int(sub[-1]) + 10000 if sub.size else 10000
    seq = np.resize(np.frombuffer(FILLER, dtype=np.uint8), n)
    seq[sub - 1] = ord('C')
    seq[sub] = ord('G')
    rows = (n + width - 1) // width
    lines = np.full((rows, width + 1), ord('\n'), dtype=np.uint8)
    lines[:, :width] = np.resize(seq, rows * width).reshape(rows, width)      # (what pads the last line is cut off below)
    body = lines.reshape(-1)
    if n % width:                                                   # the last line is short: its bytes, then one newline
        body = np.concatenate([body[:(rows - 1) * (width + 1) + n % width], np.array([ord('\n')], dtype=np.uint8)])
    return b'>' + name.encode() + b'\n' + body.tobytes(), n


def make_fasta(path, sites=28217448, width=60, seed=SEED, bgzf=None):
    from wgbs_tools_amd import synth
    names, sizes = synth.genome_shape(int(sites))[:2]
    loci = synth.synth_loci(seed, sizes)
    at = np.concatenate([[0], np.cumsum(sizes)])
    bases = []
    with open(path, 'wb') as f:
        for k, name in enumerate(names):
            text, n = chromosome_text(name, loci[at[k]:at[k + 1]], width)
            f.write(text)
            bases.append(n)
    if bgzf:
        from wgbs_tools_amd import _lib
        piece = 255 * MEMBER
        with open(path, 'rb') as f, open(bgzf, 'wb') as g:
            while True:
                buf = f.read(piece)
                if not buf:
                    break
                g.write(_lib.bgzf_deflate(buf, eof=False))
            g.write(BGZF_EOF)
    return dict(names=list(names), sizes=[int(s) for s in sizes], bases=bases, loci=loci, text_bytes=op.getsize(path), bgzf_bytes=op.getsize(bgzf) if bgzf else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('fasta')
    ap.add_argument('--sites', type=int, default=28217448)
    ap.add_argument('--width', type=int, default=60)
    ap.add_argument('--seed', type=int, default=SEED)
    ap.add_argument('--bgzf')
    a = ap.parse_args()
    t0 = time.time()
    r = make_fasta(a.fasta, a.sites, a.width, a.seed, a.bgzf)
    print(json.dumps(dict(fasta=a.fasta, chromosomes=len(r['names']), sites=int(r['loci'].size), text_bytes=r['text_bytes'], bgzf_bytes=r['bgzf_bytes'],
                          seconds=round(time.time() - t0, 1))))


if __name__ == '__main__':
    main()
