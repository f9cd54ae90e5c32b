"""`wgbstools set_default_ref`: which genome directory the other commands use when --genome is not given (src/python/set_default_ref.py).
`references/default` is a relative symbolic link to the genome's directory; genome.references_root() says where references/ is
($WGBSTOOLS_REFERENCES is honoured).  Unlike the reference this changes no working directory to make the link."""
import argparse
import os
import os.path as op

from .genome import IllegalArgumentError, eprint, references_root


def get_genomes():
    """set_default_ref.py:28-33"""
    root = references_root()
    if not op.isdir(root):
        return []
    return [d for d in os.listdir(root) if op.isdir(op.join(root, d))]


def print_genomes():
    """set_default_ref.py:13-25"""
    genomes = get_genomes()
    if not genomes:
        print('No references found.')
        return
    dgenome = op.basename(op.realpath(op.join(references_root(), 'default')))
    print('Existing references:\n=====')
    for genome in genomes:
        if genome == 'default':
            continue
        if genome == dgenome:
            genome += ' (default)'
        print(genome)


def set_def_ref(name):
    """set_default_ref.py:35-49"""
    if name not in get_genomes() or name == 'default':
        print_genomes()
        raise IllegalArgumentError(f'Invalid reference: {name}')
    dst = op.join(references_root(), 'default')
    if op.islink(dst):
        os.unlink(dst)
    os.symlink(name, dst)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('--name', help='name of the genome (e.g. hg19, mm9...).')
    parser.add_argument('-ls', action='store_true', help='print a list of existing genomes')
    return parser.parse_args(argv)


def main(argv=None):
    """
    Change the default genome reference.
    """
    args = parse_args(argv)
    if args.name:
        set_def_ref(args.name)
        eprint(f'[wt def] changed default genome to {args.name}')
    if args.ls:
        print_genomes()
    elif not args.name:
        eprint('[wt def] you must specify either --name or -ls')


if __name__ == '__main__':
    main()
