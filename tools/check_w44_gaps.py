"""Static check of the MFMA gaps of k_mid_wino44's tile loop (csrc/dncnn_wino44.hip).

Beside an f32 MFMA one memory instruction is free and a second one in the same gap costs about an MFMA, so the
two-block-row form gives every memory instruction of the main loop a gap of its own.  This script compiles the file to
assembly and, for every production instantiation (STAMP = false, VAR = 0), walks the MFMAs of the tile loop up to
W44_EPILOGUE_BEGIN and classifies what stands between an MFMA and the next one (the last gap ends at the marker):
LDS instructions (ds_*), vector-memory instructions (global_* / buffer_*) and vector-ALU instructions (other v_*).
Prints the histogram per instantiation.  Exit code 0 = every NG = 2 instantiation has 1152 MFMAs, no gap with more than
one memory instruction and no gap that mixes vector-ALU work with a memory instruction."""
import collections, re, sys

from hip_listing import listing

MFMAS = {1: 576, 2: 1152}                                   # per region and wave: 36 points x NG block rows x 16 k-steps


def gaps(lines):
    """[(lds, vmem, valu)] for every gap behind an MFMA, up to the first epilogue marker"""
    out, cur = [], None
    for l in lines:
        l = l.strip()
        if 'W44_EPILOGUE_BEGIN' in l:
            break
        op = l.split(';')[0].split()
        if not op or op[0].startswith('.') or op[0].endswith(':'):
            continue
        op = op[0]
        if op.startswith('v_mfma'):
            if cur is not None:
                out.append(tuple(cur))
            cur = [0, 0, 0]
        elif cur is not None:
            if op.startswith('ds_'):
                cur[0] += 1
            elif op.startswith('global_') or op.startswith('buffer_'):
                cur[1] += 1
            elif op.startswith('v_'):
                cur[2] += 1
    if cur is not None:
        out.append(tuple(cur))
    return out


def analyse(asm_text):
    """{kernel name: {'ng', 'mfmas', 'hist' {(lds, vmem, valu): gaps}, 'multi' (gaps with > 1 memory instruction),
    'mixed' (gaps with vector-ALU work and a memory instruction)}} for the production instantiations"""
    res = {}
    blocks = re.split(r'\n(?=_ZN3pnp3w4412k_mid_wino44[^\n]*:\s)', asm_text)
    for blk in blocks[1:]:
        name = blk.split(':', 1)[0]
        m = re.search(r'ILb[01]ELi([12])ELb0ELi0ELb[01]EEEv', name)         # <LEAKY, NG, STAMP = false, VAR = 0, FL>
        if not m:
            continue
        lines = blk.split('\n')
        end = next((i for i, l in enumerate(lines) if l.startswith('.Lfunc_end')), len(lines))
        g = gaps(lines[:end])
        res[name] = dict(ng=int(m.group(1)), mfmas=len(g), hist=dict(collections.Counter(g)),
                         multi=sum(1 for a in g if a[0] + a[1] > 1), mixed=sum(1 for a in g if a[2] and a[0] + a[1]))
    return res


def compile_asm():
    return listing('dncnn_wino44.hip')


def main():
    res = analyse(open(sys.argv[1]).read() if len(sys.argv) > 1 else compile_asm())
    problems = 0
    for name, r in res.items():
        print(f'{name}: NG = {r["ng"]}, {r["mfmas"]} MFMAs before the epilogue, {r["multi"]} gap(s) with more than one memory '
              f'instruction, {r["mixed"]} gap(s) mixing vector-ALU and memory instructions')
        print('    LDS  VMEM  VALU  gaps')
        for (lds, vmem, valu), n in sorted(r['hist'].items()):
            print(f'    {lds:3d}  {vmem:4d}  {valu:4d}  {n:4d}')
        if r['mfmas'] != MFMAS[r['ng']] or (r['ng'] == 2 and (r['multi'] or r['mixed'])):
            problems += 1
    print(f'{len(res)} kernel instantiation(s) checked, {problems} problem(s)')
    return 1 if problems or not res else 0


if __name__ == '__main__':
    sys.exit(main())
