"""Device assembly of one csrc file, compiled the way csrc/Makefile compiles it -- the one copy of that command line for the
static checks (check_w44_isa.py, check_w44_gaps.py, check_w44b_isa.py, check_fused_isa.py).

    python tools/hip_listing.py dncnn_wino44.hip [-DNAME ...] [-o out.s]     the listing of the working tree's file
    python tools/hip_listing.py dncnn_wino44.hip --against REV               ... compared with the file as of git revision REV

--against is the check of a kernel refactor: REV's pnp_svrg_amd/csrc and include trees are taken from `git archive` into a
temporary directory, both files are compiled, and the listings must be equal (exit code 0) -- apart from the one symbol hipcc
derives from a hash of the source text, `__hip_cuid_<hash>`, which is masked."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the per-file flags of csrc/Makefile that bear on device code
W44_FLAGS = ['-mllvm', '-pragma-unroll-threshold=200000', '-fno-slp-vectorize']
FILE_FLAGS = {'dncnn_wino44.hip': W44_FLAGS, 'dncnn_wino44b.hip': W44_FLAGS, 'prox.hip': ['-ffp-contract=off'],
              'prox_wavelet2d.hip': ['-ffp-contract=off'], 'nlm.hip': ['-ffp-contract=off']}


def listing(name, defines=(), root=ROOT):
    """listing text of pnp_svrg_amd/csrc/<name> under `root`, with extra -D defines"""
    csrc = os.path.join(root, 'pnp_svrg_amd', 'csrc')
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, 'listing.s')
        subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-unused-function', *FILE_FLAGS.get(name, []),
                        *defines, '-x', 'hip', '--cuda-device-only', '-S', name, '-o', out], check=True, cwd=csrc, stderr=subprocess.DEVNULL)
        return open(out).read()


def listing_at(rev, name, defines=()):
    """the same for the file as of git revision `rev`"""
    with tempfile.TemporaryDirectory() as td:
        tar = os.path.join(td, 'rev.tar')
        subprocess.run(['git', 'archive', '-o', tar, rev, 'pnp_svrg_amd/csrc', 'include'], check=True, cwd=ROOT)
        subprocess.run(['tar', '-xf', tar, '-C', td], check=True)
        return listing(name, defines, root=td)


def masked(text):
    return re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_', text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('name', help='file name under pnp_svrg_amd/csrc')
    ap.add_argument('-D', dest='defines', action='append', default=[], help='extra define (NAME or NAME=VALUE)')
    ap.add_argument('-o', dest='out', help='write the listing here (default: standard output)')
    ap.add_argument('--against', metavar='REV', help='compare with the listing of the file as of this git revision')
    a = ap.parse_args()
    defines = ['-D' + d for d in a.defines]
    text = listing(a.name, defines)
    if a.against:
        old = masked(listing_at(a.against, a.name, defines)).split('\n')
        new = masked(text).split('\n')
        differ = len(old) != len(new) or any(x != y for x, y in zip(old, new))
        first = next((i + 1 for i, (x, y) in enumerate(zip(old, new)) if x != y), min(len(old), len(new)) + 1)
        print(f'{a.name}: {len(new)} lines, ' + (f'DIFFERS from {a.against} ({len(old)} lines; first at line {first})' if differ
                                                 else f'equal to {a.against}'))
        return 1 if differ else 0
    if a.out:
        open(a.out, 'w').write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
