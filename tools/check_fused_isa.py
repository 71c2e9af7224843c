"""Static check of the hand-issued global loads of the one-kernel iteration (csrc/csmri_fused.hip) on the generated code.

hipcc does not know that the inline-asm `global_load_dwordx4 ... ; PNP_GLD` results arrive later: it may read, overwrite or
spill a destination register right behind the load.  The kernel guards every batch with a hand-counted `s_waitcnt vmcnt(N)`;
this script verifies on the ISA of every k_svrg_iter instantiation that

  * no instruction names a destination register of a tagged load before a wait that covers it has been passed, on ANY path:
    a wait `vmcnt(K)` covers a load when at least K vector-memory operations were issued after it on every path (operations
    leave the queue in issue order);
  * branches are forward, or loops without a hand-issued load in flight (the analysis is one pass over the listing, states merged
    at labels).

    python tools/check_fused_isa.py [listing.s]        (without argument: compiles csmri_fused.hip with hipcc -S first)
    python tools/check_fused_isa.py --pp [listing.s]   ... and the per-problem loops k_svrg_outer_pp and k_svrg_span_pp as well
    python tools/check_fused_isa.py --sarah [listing.s]   the SARAH instantiations instead (k_sarah_iter, k_sarah_iter_pp: plain and _pp,
                                                          denoise on and off, with and without out2), the same rule -- and for every
                                                          hand-issued store (`s_nop 4` in front of a global_store_dwordx4) the wait
                                                          state behind it: its data registers may be rewritten by the next instruction
    python tools/check_fused_isa.py --steps [listing.s]   the minibatch forms instead (k_grad_step, k_saga_iter: denoise on and off --
                                                          one kernel serves the plain and the _pp entry point), both rules
    python tools/check_fused_isa.py --spans [listing.s]   the one-launch forms instead (k_sarah_outer, k_grad_span: GD and SGD,
                                                          k_saga_span -- each serves its plain and its _pp entry point), both rules
    python tools/check_fused_isa.py --sarah-span [listing.s]   the per-problem-T2 SARAH span instead (k_sarah_span_pp: the outer body and
                                                          the inner body inside one loop), both rules
    python tools/check_fused_isa.py --hist [listing.s]    the SAGA forms with a per-problem divisor instead (k_saga_iter_hist: denoise on
                                                          and off, k_saga_span_hist), both rules
    python tools/check_fused_isa.py --w2d [listing.s]     the instantiations that hold the 2-D wavelet prox instead (MODE = 3 of
                                                          k_svrg_iter_pp, k_sarah_iter_pp, k_grad_step, k_saga_iter -- each serves its
                                                          plain and its _pp entry point -- and k_svrg_outer_prox), both rules

Also prints, per kernel, the spill traffic between workgroup barriers (where the register pressure bites)."""
import re
import sys

import hip_listing

VMEM = ('global_', 'buffer_', 'scratch_', 'flat_')


def listing(path=None, defines=()):
    return open(path).read() if path else hip_listing.listing('csmri_fused.hip', defines)


def regs_of(text):
    """VGPR numbers named in an operand string."""
    out = set()
    for m in re.finditer(r'\bv\[(\d+):(\d+)\]|\bv(\d+)\b', text):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def kernels(txt, pp=False, sarah=False, steps=False, spans=False, hist=False, w2d=False, sarah_span=False):
    """(name, body) of every k_svrg_iter instantiation and of k_svrg_outer; pp: also k_svrg_outer_pp and k_svrg_span_pp;
    sarah: the k_sarah_iter and k_sarah_iter_pp instantiations instead; steps: the k_grad_step and k_saga_iter instantiations instead;
    spans: k_sarah_outer, the k_grad_span instantiations and k_saga_span instead; hist: the k_saga_iter_hist instantiations and
    k_saga_span_hist instead; sarah_span: k_sarah_span_pp instead"""
    names = ('_ZN3pnp11k_svrg_iter', '_ZN3pnp12k_svrg_outer') + (('_ZN3pnp15k_svrg_outer_pp', '_ZN3pnp14k_svrg_span_pp') if pp else ())
    if sarah:
        names = ('_ZN3pnp12k_sarah_iter', '_ZN3pnp15k_sarah_iter_pp')
    if steps:
        names = ('_ZN3pnp11k_grad_step', '_ZN3pnp11k_saga_iter')
    if spans:
        names = ('_ZN3pnp13k_sarah_outer', '_ZN3pnp11k_grad_span', '_ZN3pnp11k_saga_span')
    if hist:
        names = ('_ZN3pnp16k_saga_iter_hist', '_ZN3pnp16k_saga_span_hist')
    if sarah_span:
        names = ('_ZN3pnp15k_sarah_span_pp',)
    if w2d:
        names = ('_ZN3pnp14k_svrg_iter_ppILi3E', '_ZN3pnp15k_sarah_iter_ppILi3E', '_ZN3pnp11k_grad_stepILi3E', '_ZN3pnp11k_saga_iterILi3E',
                 '_ZN3pnp17k_svrg_outer_prox')
    lines = txt.split('\n')
    i = 0
    while i < len(lines):
        l = lines[i]
        # (MODE = 3, the 2-D wavelet prox, is --w2d's: the other selections keep the kernels they had)
        if l.startswith(names) and l.split(';')[0].rstrip().endswith(':') and (w2d or not re.match(r'_ZN3pnp\d+k_(svrg_iter|svrg_iter_pp|sarah_iter|sarah_iter_pp|grad_step|saga_iter)ILi3E', l)):
            name = l.split(':')[0]
            body = []
            i += 1
            while i < len(lines) and not lines[i].strip().startswith('s_endpgm'):
                body.append(lines[i])
                i += 1
            yield name, body
        i += 1


def check(name, body):
    # state: {load id: (dst regs, min younger ops)}; per-label merged states
    pending = {}
    state = {}
    alive = True                                       # fallthrough reachable
    seen_labels = set()
    errors, n_loads, n_waits = [], 0, 0
    last_code = ''
    seg, segs = {'sst': 0, 'sld': 0}, []

    def merge(a, b):
        out = dict(a)
        for k, (regs, y) in b.items():
            out[k] = (regs, min(y, out[k][1])) if k in out else (regs, y)
        return out

    for ln, raw in enumerate(body):
        t = raw.strip()
        if not t or t.startswith(';'):
            continue
        if re.match(r'^\.LBB\d+_\d+:', t):
            lab = t.split(':')[0]
            seen_labels.add(lab)
            inc = pending.pop(lab, None)
            if inc is not None:
                state = merge(state, inc) if alive else inc
                alive = True
            continue
        if t.startswith('.'):
            continue
        prev_code = last_code
        code = t.split(';')[0].strip()
        last_code = code
        op = code.split()[0]
        operands = code[len(op):]
        if not alive:
            continue
        if op == 's_barrier':
            segs.append(seg)
            seg = {'sst': 0, 'sld': 0}
        if op.startswith('scratch_store'):
            seg['sst'] += 1
        if op.startswith('scratch_load'):
            seg['sld'] += 1
        # hazard: any in-flight destination named here
        used = regs_of(operands)
        for k, (regs, y) in list(state.items()):
            if used & regs and not (op.startswith('global_load') and 'PNP_GLD' in t and k == ln):
                errors.append(f'{name}: line {ln}: `{code}` names v{sorted(used & regs)} of the load issued at line {k} (in flight, {y} younger operations)')
                del state[k]
        if op == 's_waitcnt':
            m = re.search(r'vmcnt\((\d+)\)', code)
            if m:
                n_waits += 1
                K = int(m.group(1))
                state = {k: v for k, v in state.items() if v[1] < K}
        if (op.startswith('global_load') and 'PNP_GLD' in t) or (op == 'global_store_dwordx4' and prev_code != 's_nop 4' and False):
            pass
        if op.startswith('global_') and ('PNP_GLD' in t) and prev_code != 's_nop 4':
            errors.append(f'{name}: line {ln}: hand-issued load without its s_nop 4 (VALU-written scalar base)')
        if op.startswith(VMEM):
            state = {k: (r, y + 1) for k, (r, y) in state.items()}
            if 'PNP_GLD' in t:
                n_loads += 1
                dst = regs_of(operands.split(',')[0])
                state[ln] = (dst, 0)
        if op.startswith('s_cbranch') or op == 's_branch':
            lab = operands.strip()
            if lab in seen_labels:
                # a loop (the start-up delay) is fine as long as no hand-issued load is in flight around it
                if state:
                    errors.append(f'{name}: backward branch to {lab} with {len(state)} hand-issued loads in flight')
                continue
            pending[lab] = merge(pending[lab], state) if lab in pending else dict(state)
            if op == 's_branch':
                alive = False
                state = {}
    segs.append(seg)
    if state:
        errors.append(f'{name}: {len(state)} tagged loads never waited for')
    return errors, n_loads, n_waits, segs


def check_stores(name, body):
    """Every hand-issued store (gst: `s_nop 4`, global_store_dwordx4, `s_nop 1`) keeps the wait state behind it: the hazard
    recognizer does not pad inside inline asm, and the next instruction may rewrite the store's data registers."""
    code = [c for c in (raw.split(';')[0].strip() for raw in body) if c and not c.startswith('.')]
    errors, n = [], 0
    for i, c in enumerate(code):
        if c.startswith('global_store_dwordx4') and i > 0 and code[i - 1] == 's_nop 4':
            n += 1
            nxt = code[i + 1] if i + 1 < len(code) else ''
            m = re.match(r's_nop (\d+)$', nxt)
            if not (m and int(m.group(1)) >= 1):
                errors.append(f'{name}: hand-issued store `{c}` is followed by `{nxt}`, not by its wait state (s_nop 1)')
    return errors, n


def main():
    args = sys.argv[1:]
    defines = [a for a in args if a.startswith('-D')]          # e.g. -DPNP_FUSED_CLOCK: the diagnostic build
    pp = '--pp' in args                                         # also the per-problem loops: k_svrg_outer_pp, k_svrg_span_pp
    sarah = '--sarah' in args                                   # the SARAH instantiations instead, with the store rule
    steps = '--steps' in args                                   # the minibatch forms instead, with the store rule
    spans = '--spans' in args                                   # the one-launch forms instead, with the store rule
    hist = '--hist' in args                                     # the per-problem-divisor SAGA forms instead, with the store rule
    sarah_span = '--sarah-span' in args                         # the per-problem-T2 SARAH span instead, with the store rule
    w2d = '--w2d' in args                                       # the instantiations with the 2-D wavelet prox instead, with the store rule
    paths = [a for a in args if not a.startswith('-')]
    txt = listing(paths[0] if paths else None, defines)
    bad = []
    nk = 0
    for name, body in kernels(txt, pp, sarah, steps, spans, hist, w2d, sarah_span):
        nk += 1
        errors, n_loads, n_waits, segs = check(name, body)
        spill = ' '.join(f'{i}:{s["sst"]}/{s["sld"]}' for i, s in enumerate(segs) if s['sst'] or s['sld'])
        stores = ''
        if sarah or steps or spans or hist or w2d or sarah_span:
            st_errors, n_st = check_stores(name, body)
            errors = errors + st_errors
            stores = f'{n_st} hand-issued stores, '
        print(f'{name[:40]}...: {n_loads} hand-issued loads, {stores}{n_waits} vmcnt waits, {len(errors)} violations; scratch stores/loads per barrier segment: {spill}')
        bad += errors
    for e in bad[:40]:
        print('VIOLATION', e)
    if nk == 0:
        print('no k_svrg_iter kernel found')
        return 2
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
