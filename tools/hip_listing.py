"""Device assembly of one csrc file, compiled the way csrc/Makefile compiles it -- the one copy of that command line for the
static checks (check_w44_isa.py, check_w44_gaps.py, check_w44b_isa.py, check_fused_isa.py).

    python tools/hip_listing.py dncnn_wino44.hip [-DNAME ...] [-o out.s]     the listing of the working tree's file
    python tools/hip_listing.py dncnn_wino44.hip --against REV               ... compared with the file as of git revision REV

--against is the check of a kernel refactor: REV's pnp_svrg_amd/csrc and include trees are taken from `git archive` into a
temporary directory, both files are compiled, and the listings must be equal (exit code 0) -- apart from the one symbol hipcc
derives from a hash of the source text, `__hip_cuid_<hash>`, which is masked.
    python tools/hip_listing.py csmri_fused.hip --against REV --per-kernel   ... kernel by kernel: for a change that ADDS kernels to a
                                                                              file and must leave the existing ones as they are"""
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
              'prox_wavelet2d.hip': ['-ffp-contract=off'], 'nlm.hip': ['-ffp-contract=off'], 'axpbypcz_pp.hip': ['-ffp-contract=off']}


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


def kernels(text):
    """{kernel symbol: its code and its .amdhsa_kernel descriptor block} of a listing, with the per-file numbering of local labels
    (.LBB<function>_<block>, .Lfunc_end<function>) masked: adding a kernel to a file renumbers the others without changing them."""
    text = re.sub(r'BB\d+_', 'BB_', re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', masked(text)))
    text = re.sub(r'[ \t]*;.*$', '', text, flags=re.M)          # comments (their column depends on the width of a label number)
    out = {}
    for m in re.finditer(r'^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel', text, re.M | re.S):
        name = m.group(1)
        body = re.search(r'^' + re.escape(name) + r':.*?^\.Lfunc_end:', text, re.M | re.S)
        out[name] = (body.group(0) if body else '') + '\n' + m.group(2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('name', help='file name under pnp_svrg_amd/csrc')
    ap.add_argument('-D', dest='defines', action='append', default=[], help='extra define (NAME or NAME=VALUE)')
    ap.add_argument('-o', dest='out', help='write the listing here (default: standard output)')
    ap.add_argument('--against', metavar='REV', help='compare with the listing of the file as of this git revision')
    ap.add_argument('--per-kernel', action='store_true', help='with --against: compare kernel by kernel -- every kernel REV has must '
                    'exist and be equal (code and descriptor); kernels REV does not have are listed as new')
    a = ap.parse_args()
    defines = ['-D' + d for d in a.defines]
    text = listing(a.name, defines)
    if a.against and a.per_kernel:
        old, new = kernels(listing_at(a.against, a.name, defines)), kernels(text)
        bad = [k for k in old if old[k] != new.get(k)]
        added = [k for k in new if k not in old]
        print(f'{a.name}: {len(old)} kernels of {a.against}: ' + (f'{len(bad)} DIFFER or are missing: {bad}' if bad else 'all equal')
              + f'; {len(added)} new')
        return 1 if bad or not old else 0
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
