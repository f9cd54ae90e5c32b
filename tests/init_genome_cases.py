"""FASTA texts for `wgbstools init_genome` (tests/golden/init_genome_cases.json holds what the reference's own functions make of them;
tests/init_genome_ref.py restates those).  No sequence line carries a blank: there the engine's rule and the reference's agree."""
import numpy as np

TILE = 4096                            # csrc/fasta_plan.h WG_FA_TILE
THREAD_BYTES = 16                      # ... WG_FA_THREAD_BYTES
MAX_NAME = 255                         # csrc/fasta_core.h WG_FA_MAX_NAME

NAMES = ['chrM', 'chr10', 'chr2', 'chrX', 'chr1', 'chrUn_x', 'chr1_random', 'MT', '7', 'chr01']


def _names_text():
    seqs = ['ACGCG', 'TTCGA', 'CGCGCGA', 'GGC', 'ACGT', 'CGCG', 'TCG', 'CCGG', 'ACGACG', 'GCGC']
    return ''.join('>%s\n%s\n' % (n, s) for n, s in zip(NAMES, seqs)).encode()


# name -> (text, no_sort)
CASES = {
    'issue_example': (b'>chr1\nacgtC\nGNNc\r\ng', False),
    'soft_masked': (b'>chr1 soft masked\nacgtCGcGnnCg\nACgTcg\n', False),
    'split_lf': (b'>chr1\nAAC\nGTT\nC\nG\nC\n', False),
    'split_crlf': (b'>chr1\r\nAAC\r\nGTT\r\nc\r\ng\r\nC\r\n', False),
    'blank_lines': (b'>chr1\nAC\n\n\nGT\n\nCG\nC\n\n', False),
    'across_sequences': (b'>chr1\nAAC\n>chr2\nGTT\nTC\n>chr3\ngCG\n', False),
    'cg_in_header': (b'>chr1 CG CGCG\nAT\n>chr2\tCG\nCG\n>chr3 >CG\nAC\nG\n', False),
    'empty_sequence': (b'>chr1\n>chr2\nCG\n>chr3\n\n>chr4\n', False),
    'no_final_newline': (b'>chr1\nACG\nTTCG', False),
    'ends_in_c': (b'>chr1\nACG\nTTC', False),
    'no_cpg': (b'>chr1\nAAAA\n>chr2\nACGT\n>chr3\nGGCC\n', False),
    'names_sorted': (_names_text(), False),
    'names_fasta_order': (_names_text(), True),
    'none_before_dropped': (b'>scaffold_1\nCGCG\n>chr2\nACG\n>chrUn\nCG\n>chr1\nCCG\n', False),
}


def every_case_text():
    """one FASTA of about 300 bytes with all of the above in it (names made distinct), for the cut tests"""
    parts = []
    for k, (name, (text, _)) in enumerate(sorted(CASES.items())):
        if name.startswith('names_') or name in ('none_before_dropped', 'every_case'):
            continue
        t = text.replace(b'>chr', b'>chr%d' % (k + 1))
        parts.append(t if t.endswith(b'\n') else t + b'\n')
    return b''.join(parts) + b'>chrX tail\r\nAC\r\n\r\nG\nCG'


CASES['every_case'] = (every_case_text(), False)


def random_world(rng, n_seqs=None, max_len=3000):
    """a FASTA text: distinct names (some kept, some not), random line widths, LF or CRLF per line, blank lines, mixed case, headers
    with descriptions that hold CG and '>', empty sequences, with or without a last newline"""
    n_seqs = int(rng.integers(1, 9)) if n_seqs is None else n_seqs
    pool = ['chr%d' % k for k in range(1, 23)] + ['chrX', 'chrY', 'chrM', 'MT', '3', '11', 'chrUn_gl1', 'chr4_random', 'scaffold7', 'chr007']
    names = [pool[i] for i in rng.permutation(len(pool))[:n_seqs]]
    out = []
    if rng.random() < 0.3:
        out.append(b'\n\r\n' if rng.random() < 0.5 else b'\n')
    for name in names:
        head = b'>' + name.encode()
        if rng.random() < 0.5:
            head += (b' ' if rng.random() < 0.5 else b'\t') + bytes(rng.choice(list(b'CG >acgt01'), size=int(rng.integers(0, 30))).astype(np.uint8))
        out.append(head + (b'\r\n' if rng.random() < 0.3 else b'\n'))
        n = 0 if rng.random() < 0.1 else int(rng.integers(1, max_len))
        seq = bytes(rng.choice(list(b'ACGTacgtNCG'), size=n).astype(np.uint8))
        width = int(rng.choice([1, 2, 7, 60, 70, 100000]))
        for at in range(0, n, width):
            out.append(seq[at:at + width] + (b'\r\n' if rng.random() < 0.2 else b'\n'))
            if rng.random() < 0.05:
                out.append(b'\n')
    text = b''.join(out)
    if rng.random() < 0.3 and text.endswith(b'\n') and not text.endswith(b'>\n'):
        text = text[:-1]
    return text


def layout_fasta(names, sizes, loci, width=60):
    """the FASTA of a synthetic genome: CG at every locus, CG-free filler elsewhere, every chromosome 10,000 bases longer than its last
    locus (what synth.write_genome writes into chrome.size), lines of `width` bases.  No two loci of a chromosome may be adjacent."""
    out, pos = [], 0
    for name, size in zip(names, sizes):
        sub = np.asarray(loci[pos:pos + size], dtype=np.int64)
        pos += size
        assert sub.size == 0 or (np.diff(sub) >= 2).all(), 'adjacent loci cannot both be CpGs'
        n = int(sub[-1]) + 10000 if sub.size else 10000
        seq = np.frombuffer((b'ATTA' * (n // 4 + 1))[:n], dtype=np.uint8).copy()
        seq[sub - 1] = ord('C')
        seq[sub] = ord('G')
        lines = seq.tobytes()
        out.append(b'>' + name.encode() + b'\n' + b'\n'.join(lines[at:at + width] for at in range(0, n, width)) + b'\n')
    return b''.join(out)
