"""Record what the one-kernel CSMRI entry points of csrc/csmri.hip answer to bad arguments -> tests/golden/csmri_refusals.json,
the table tests/test_cpu_csmri_refusals.py replays against the built library.

    python tools/record_csmri_refusals.py [--lib PATH] [-o OUT.json]

Run it on the library of the commit whose answers are to be kept (for a refactor: its parent), on a machine WITHOUT a GPU: the
argument checks answer before any HIP call, on a plan filled on the host and on fabricated, never dereferenced pointers.  The file:
    {"base":  {entry point: a valid argument list, positional as the C prototype has it -- null, a number, or (first argument) the
                            plan as {"H", "batch", "dtype"}},
     "cases": [{"entry", "case": its name, "set": {position: value} over the base, "rc": code, "error": pnp_last_error() or null}]}
A refused case (PNP_ERR_ARG) keeps code and text.  A case the checks let through (`through` below: the accepted side of a bound)
ends at the first HIP call, which fails where no device is visible: code PNP_ERR_HIP, text not kept (it quotes the failing HIP
expression).  Such a case carries a plan of batch 0, so that even with a device there would be nothing to launch."""
import argparse
import ctypes
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'csmri_refusals.json')
ERR_ARG, ERR_HIP = 1, 2
IMAX = 2 ** 31 - 1


def load_native():
    """pnp_svrg_amd/_native.py on its own (importing the package pulls in torch, which none of this needs)"""
    spec = importlib.util.spec_from_file_location('_pnp_native', os.path.join(ROOT, 'pnp_svrg_amd', '_native.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Plan(ctypes.Structure):
    """the fields of csrc/csmri_plan.h"""
    _fields_ = [('H', ctypes.c_int), ('W', ctypes.c_int), ('batch', ctypes.c_int), ('dtype', ctypes.c_int), ('NL', ctypes.c_int),
                ('work', ctypes.c_void_p), ('twtab', ctypes.c_void_p), ('mbd', ctypes.c_void_p), ('fused_min_batch', ctypes.c_int)]


def plan(H=256, dtype=0, batch=2):
    return dict(H=H, batch=batch, dtype=dtype)


def call(lib, signatures, entry, args):
    """(code, pnp_last_error() text) of one call; `args` as the file holds them"""
    fn = getattr(lib, entry, None)
    if fn is None:
        return None, 'the library has no such entry point'
    fn.restype, fn.argtypes = signatures[entry]
    lib.pnp_last_error.restype = ctypes.c_char_p
    first = None
    if args[0] is not None:
        H = args[0]['H']
        keep = Plan(H, H, args[0]['batch'], args[0]['dtype'], {256: 16, 128: 12, 64: 8}[H], None, None, None, 192)
        first = ctypes.cast(ctypes.pointer(keep), ctypes.c_void_p)
    rc = fn(first, *args[1:])
    return rc, lib.pnp_last_error().decode(errors='replace')


# ---- the cases.  The images of a batch-2 plan take 512 KiB: fabricated buffers lie 1 MiB apart, the SAGA table far from them.
IMG = 2 * 256 * 256 * 4
A = lambda k: 0x10000000 + k * 0x100000
TABLE = 0x40000000

PROTOS = {
    'pnp_csmri_svrg_step': 'p a b bitsT alpha alpha_vec beta c1 gamma c2 out denoise sigma_modifier fallback_sigma xrec sse_out sigma_out stream',
    'pnp_csmri_svrg_step_pp': 'p a b bitsT alpha alpha_pp alpha_vec beta c1 gamma gamma_pp c2 out denoise sigma_modifier sigma_modifier_pp '
                              'fallback_sigma xrec sse_out sigma_out stream',
    'pnp_csmri_sarah_step': 'p a b bitsT alpha alpha_vec beta c1 gamma c2 v_out out out2 denoise sigma_modifier fallback_sigma xrec sse_out '
                            'sigma_out stream',
    'pnp_csmri_sarah_step_pp': 'p a b bitsT alpha alpha_pp alpha_vec beta c1 gamma gamma_pp c2 v_out out out2 denoise sigma_modifier '
                               'sigma_modifier_pp fallback_sigma xrec sse_out sigma_out stream',
    'pnp_csmri_grad_step': 'p a bitsT yh YT alpha alpha_vec beta c1 out denoise sigma_modifier fallback_sigma xrec sse_out sigma_out stream',
    'pnp_csmri_grad_step_pp': 'p a bitsT yh YT alpha alpha_pp alpha_vec beta c1 out denoise sigma_modifier sigma_modifier_pp fallback_sigma '
                              'xrec sse_out sigma_out stream',
    'pnp_csmri_saga_step': 'p z bitsT YT alpha alpha_vec table row prev_row sum lr inv_hist hist out denoise sigma_modifier fallback_sigma '
                           'xrec sse_out sigma_out stream',
    'pnp_csmri_saga_step_pp': 'p z bitsT YT alpha alpha_pp alpha_vec table row prev_row sum lr lr_pp inv_hist hist out denoise sigma_modifier '
                              'sigma_modifier_pp fallback_sigma xrec sse_out sigma_out stream',
    'pnp_csmri_saga_step_hist_pp': 'p z bitsT YT alpha alpha_pp alpha_vec table row prev_row sum lr lr_pp inv_hist inv_hist_pp hist out '
                                   'denoise sigma_modifier sigma_modifier_pp fallback_sigma xrec sse_out sigma_out stream',
    'pnp_csmri_svrg_outer_step': 'p z mask_bitsT yh alpha_vec lr w_out mu_out out denoise sigma_modifier fallback_sigma xrec sse_out '
                                 'sigma_out stream',
    'pnp_csmri_svrg_outer_step_pp': 'p z mask_bitsT yh alpha_vec lr lr_pp w_out mu_out out denoise sigma_modifier sigma_modifier_pp '
                                    'fallback_sigma xrec sse_out sigma_out stream',
    'pnp_csmri_svrg_outer_iteration': 'p z w mu mask_bitsT yh alpha_vec selbits T2 lr mini_batch_size sigma_modifier fallback_sigma xrec '
                                      'sse_log log_row0 n_log sigma_out stream',
    'pnp_csmri_svrg_outer_iteration_pp': 'p z w mu mask_bitsT yh alpha_vec selbits T2 lr lr_pp mini_batch_size mb_vec sigma_modifier '
                                         'sigma_modifier_pp fallback_sigma xrec sse_log log_row0 n_log sigma_out stream',
    'pnp_csmri_svrg_outer_iteration_prox': 'p z w mu mask_bitsT yh alpha_vec selbits T2 lr lr_pp mini_batch_size mb_vec sigma_modifier '
                                           'sigma_modifier_pp fallback_sigma xrec sse_log log_row0 n_log sigma_out denoise stream',
    'pnp_csmri_svrg_span_pp': 'p z w mu mask_bitsT yh alpha_vec selbits step0 n_steps T2 t2_vec lr lr_pp mini_batch_size mb_vec '
                              'sigma_modifier sigma_modifier_pp fallback_sigma xrec sse_log log_row0 n_log sigma_out stream',
    'pnp_csmri_sarah_outer_iteration': 'p z w_prev w_next v_prev mask_bitsT yh alpha_vec selbits T2 eta lr mini_batch_size sigma_modifier '
                                       'fallback_sigma xrec sse_log log_row0 n_log sigma_out stream',
    'pnp_csmri_sarah_outer_iteration_pp': 'p z w_prev w_next v_prev mask_bitsT yh alpha_vec selbits T2 eta eta_pp lr lr_pp mini_batch_size '
                                          'mb_vec sigma_modifier sigma_modifier_pp fallback_sigma xrec sse_log log_row0 n_log sigma_out stream',
    'pnp_csmri_sarah_span_pp': 'p z w_prev w_next v_prev mask_bitsT yh alpha_vec selbits step0 n_steps T2 t2_vec eta eta_pp lr lr_pp '
                               'mini_batch_size mb_vec sigma_modifier sigma_modifier_pp fallback_sigma xrec sse_log outer_log log_row0 n_log '
                               'sigma_out stream',
    'pnp_csmri_grad_span': 'p z bitsT yh YT alpha alpha_pp alpha_vec beta denoise sigma_modifier sigma_modifier_pp fallback_sigma xrec '
                           'n_steps sse_log log_row0 n_log sigma_out stream',
    'pnp_csmri_saga_span': 'p z bitsT YT alpha alpha_pp alpha_vec table rows prev_row0 sum lr lr_pp inv_hist hist denoise sigma_modifier '
                           'sigma_modifier_pp fallback_sigma xrec n_steps sse_log log_row0 n_log sigma_out stream',
    'pnp_csmri_saga_span_hist': 'p z bitsT YT alpha alpha_pp alpha_vec table rows prev_row0 sum lr lr_pp inv_hist inv_hist_pp hist denoise '
                                'sigma_modifier sigma_modifier_pp fallback_sigma xrec n_steps sse_log log_row0 n_log sigma_out stream',
}
INTS = dict(denoise=1, hist=2, T2=3, mini_batch_size=100, log_row0=0, n_log=8, step0=0, n_steps=4)
# pointers a valid call may leave NULL ...
NULLABLE = {'stream', 'alpha_vec', 'alpha_pp', 'gamma_pp', 'lr_pp', 'eta_pp', 'sigma_modifier_pp', 'inv_hist_pp', 'mb_vec', 't2_vec', 'b',
            'c1', 'c2', 'out2', 'yh', 'YT'}
# ... and which of them a form needs all the same (of yh / YT exactly one where a form takes both)
NEEDS = {'pnp_csmri_sarah_step': 'b c1 c2', 'pnp_csmri_grad_step': 'c1 yh', 'pnp_csmri_grad_span': 'yh'}


def base(entry, signatures):
    """a valid argument set by parameter name: every required pointer an address of its own, every nullable one NULL"""
    names = PROTOS[entry].split()
    types = signatures[entry][1]
    assert len(names) == len(types), (entry, len(names), len(types))
    needs = next((v.split() for k, v in NEEDS.items() if entry.startswith(k)), [n for n in ('yh', 'YT') if n in names] + ['alpha_vec'] * ('selbits' in names))
    out = {}
    for k, (n, t) in enumerate(zip(names, types)):
        if n == 'p':
            out[n] = plan()
        elif t is ctypes.c_void_p:
            out[n] = None if n in NULLABLE and n not in needs else (TABLE if n == 'table' else A(k))
        elif t is ctypes.c_int:
            out[n] = INTS[n]
        else:
            assert t is ctypes.c_double, (entry, n, t)
            out[n] = 1.0
    return out


class ref:
    """the value of another parameter (+ a byte offset), resolved against the case's argument set"""
    def __init__(self, name, off=0):
        self.name, self.off = name, off


def wrong(names):
    """every scalar out of its range and every aliasing rule broken, for the cases where an earlier check must answer first"""
    w = {}
    for n, v in (('hist', 0), ('T2', 0), ('mini_batch_size', 0), ('n_log', 0), ('log_row0', -1), ('n_steps', 0), ('step0', -1)):
        if n in names:
            w[n] = v
    for x, y in (('w', 'z'), ('w_prev', 'z'), ('w_out', 'z'), ('table', 'z'), ('v_out', 'a'), ('outer_log', 'sse_log')):
        if x in names and y in names:
            w[x] = ref(y)
    if 'sse_out' in names:
        w['xrec'] = None
    return w


def cases_of(entry, valid):
    """[(case name, {parameter: value}, through)]: every check of the entry point violated alone, the accepted side of its bounds,
    then several violated at once -- which one answers"""
    names = list(valid)
    has = lambda *ns: all(n in names for n in ns)
    c = []
    add = lambda name, through=False, **kw: c.append((name, kw, through))
    b0 = plan(batch=0)
    # the pointers of the form's "null argument" check: the step forms take xrec, sse_out and sigma_out or leave them
    optional = {'p', 'yh', 'YT'} if has('yh', 'YT') else {'p'}
    if has('sse_out'):
        optional |= {'xrec', 'sse_out', 'sigma_out'}
    required = [n for n in names if isinstance(valid[n], int) and valid[n] >= A(0) and n not in optional]
    add('valid', through=True, p=b0)
    add('null plan', p=None)
    add(f'null {required[-1]}', **{required[-1]: None})
    add('plan 64 x 64', p=plan(H=64))
    add('plan f64', p=plan(dtype=1))
    if has('sse_out'):
        add('sse_out without xrec', xrec=None)
        add('neither sse_out nor xrec', through=True, p=b0, xrec=None, sse_out=None)
    # --- the single steps
    if entry == 'pnp_csmri_svrg_step_pp':
        add('gamma_pp with a lone c2', gamma_pp=A(50), c2=A(51))
        add('gamma_pp with c1 and c2', through=True, p=b0, gamma_pp=A(50), c1=A(52), c2=A(51))
    if has('v_out'):
        add('out2 without denoise', denoise=0, out2=A(53))
        add('out2 with denoise', through=True, p=b0, out2=A(53))
        for other in ('a', 'b', 'c2', 'out'):
            add(f'v_out is {other}', v_out=ref(other))
        add('v_out is out2', out2=ref('v_out'))
        add('v_out is c1', through=True, p=b0, v_out=ref('c1'))
    if has('yh', 'YT'):
        add('yh and YT', YT=A(44))
        add('neither yh nor YT', yh=None)
    if has('hist'):
        add('hist 0', hist=0)
        add('hist 1', through=True, p=b0, hist=1)
    if has('table'):
        tb = 2 * IMG                                              # hist = 2
        for v in ['z', 'xrec'] + (['out'] if has('out') else []):
            add(f'table ends one byte into {v}', table=ref(v, -tb + 1))
            add(f'sum starts one byte before the end of {v}', sum=ref(v, IMG - 1))
        add('table starts one byte before the end of sum', table=ref('sum', IMG - 1))
        add('sum ends one byte into table', sum=ref('table', -IMG + 1))
    if has('w_out'):
        for x, y in (('w_out', 'z'), ('mu_out', 'z'), ('w_out', 'mu_out'), ('w_out', 'out'), ('mu_out', 'out')):
            add(f'{x} is {y}', **{x: ref(y)})
        add('out is z', through=True, p=b0, out=ref('z'))
    # --- the multi-step forms
    own = [n for n in ('z', 'w', 'mu', 'w_prev', 'w_next', 'v_prev') if n in names]
    if len(own) >= 3:
        for i, x in enumerate(own):
            for y in own[i + 1:]:
                add(f'{y} is {x}', **{y: ref(x)})
    if has('outer_log'):
        add('outer_log is sse_log', outer_log=ref('sse_log'))
    if has('mini_batch_size'):
        add('mini_batch_size 0', mini_batch_size=0)
        add('mini_batch_size 1', through=True, p=b0, mini_batch_size=1)
        if has('mb_vec'):
            add('mini_batch_size 0 with mb_vec', through=True, p=b0, mini_batch_size=0, mb_vec=A(54))
    if has('n_log'):
        add('n_log 0', n_log=0)
        add('log_row0 -1', log_row0=-1)
    if has('n_steps'):
        add('n_steps 0', n_steps=0)
        add('log_row0 past its edge', log_row0=IMAX - 4 + 1)
        add('log_row0 at its edge', through=True, p=b0, log_row0=IMAX - 4)
    if has('step0'):
        add('step0 -1', step0=-1)
        add('step0 past its edge', step0=IMAX - 4 + 1)
        add('step0 at its edge', through=True, p=b0, step0=IMAX - 4)
    if has('T2'):
        add('T2 0', T2=0)
        if has('t2_vec'):
            add('T2 0 with t2_vec', through=True, p=b0, T2=0, t2_vec=A(55))
        else:
            add('T2 1', through=True, p=b0, T2=1)
    if entry.startswith('pnp_csmri_svrg_outer_iteration'):
        add('T2 2 without selbits', T2=2, selbits=None)
        add('T2 1 without selbits', through=True, p=b0, T2=1, selbits=None)
    if entry.startswith('pnp_csmri_sarah_outer_iteration'):
        add('T2 INT32_MAX', T2=IMAX)
        add('T2 INT32_MAX - 1', through=True, p=b0, T2=IMAX - 1)
        add('log_row0 past its edge', log_row0=IMAX - 1 - 3 + 1)
        add('log_row0 at its edge', through=True, p=b0, log_row0=IMAX - 1 - 3)
    if has('n_steps', 'denoise'):
        add('denoise 0', denoise=0)
    if has('n_steps', 'denoise') or has('inv_hist_pp'):
        add('denoise 2', denoise=2)
    # --- several at once
    add('null plan, everything else wrong', p=None, **wrong(names))
    add('plan 64 x 64, everything else wrong', p=plan(H=64), **wrong(names))
    add(f'null {required[0]} on an f64 plan', p=plan(dtype=1), **{required[0]: None})
    if has('w_out'):
        add('sse_out without xrec and w_out is z', xrec=None, w_out=ref('z'))
    if has('n_log') and len(own) >= 3:
        add(f'n_log 0 and {own[1]} is z', n_log=0, **{own[1]: ref('z')})
        add(f'f64 plan and {own[1]} is z', p=plan(dtype=1), **{own[1]: ref('z')})
    if has('n_steps', 'T2'):
        add('n_steps 0 and T2 0', n_steps=0, T2=0)
        add('T2 0 and n_log 0', T2=0, n_log=0)
    if has('hist', 'out'):
        add('hist 0 and table over z', hist=0, table=ref('z'))
    if has('hist', 'n_steps'):
        add('hist 0 and n_steps 0', hist=0, n_steps=0)
        add('denoise 0 and table over z', denoise=0, table=ref('z'))
    if has('n_steps', 'denoise'):
        add('denoise 2 on a 64 x 64 plan', denoise=2, p=plan(H=64))
    if has('yh', 'YT'):
        add('yh and YT on a 64 x 64 plan', YT=A(44), p=plan(H=64))
    if has('yh', 'YT', 'n_steps'):
        add('yh and YT and n_steps 0', YT=A(44), n_steps=0)
    if has('v_out'):
        add('out2 without denoise and v_out is a', denoise=0, out2=A(53), v_out=ref('a'))
        add('v_out is a on an f64 plan', v_out=ref('a'), p=plan(dtype=1))
    if entry.startswith('pnp_csmri_sarah_outer_iteration'):
        add('mini_batch_size 0 and a null plan', mini_batch_size=0, p=None)
        add('T2 0 on an f64 plan', T2=0, p=plan(dtype=1))
    if entry == 'pnp_csmri_svrg_outer_iteration_prox':
        # denoise = 1 is the _pp call (its name in the messages) and all of the above ran with it: the same with the 2-D prox, then
        # the values that are neither
        for name, kw, through in list(c):
            c.append((name + ', denoise 2', dict(kw, denoise=2), through))
        add('denoise 0', denoise=0)
        add('denoise 3', denoise=3)
        add('denoise 0 and a null plan', denoise=0, p=None)
    return c


def build_cases(signatures):
    """({entry: base argument list}, [(entry, case name, {position: value}, through)])"""
    bases, out = {}, []
    for entry in PROTOS:
        valid = base(entry, signatures)
        names = list(valid)
        bases[entry] = [valid[n] for n in names]
        seen = set()
        for name, kw, through in cases_of(entry, valid):
            assert name not in seen, (entry, name)
            seen.add(name)
            args = dict(valid)
            for k, v in kw.items():
                assert k in args, (entry, name, k)
                if not isinstance(v, ref):
                    args[k] = v
            for k, v in kw.items():                                # references see the other values of the case
                if isinstance(v, ref):
                    args[k] = args[v.name] + v.off
            if through:
                assert args['p'] is not None and args['p']['batch'] == 0, (entry, name)
            out.append((entry, name, {str(names.index(k)): args[k] for k in kw}, through))
    return bases, out


def arguments(table, case):
    """the positional arguments of one case of the file"""
    args = list(table['base'][case['entry']])
    for k, v in case['set'].items():
        args[int(k)] = v
    return args


def replay(lib, native, path):
    """--replay: [[code, text], ...] of the file's cases on standard output, for the test to compare.  It runs in a process of its own
    with the devices hidden (HIDE), and makes sure of that first: pnp_csmri_plan_create has to fail for want of a device, or no case is
    run -- a case that a broken check lets through must end at the first HIP call, never in a launch on the fabricated pointers."""
    lib.pnp_csmri_plan_create.restype, lib.pnp_csmri_plan_create.argtypes = native.SIGNATURES['pnp_csmri_plan_create']
    h = ctypes.c_void_p()
    if lib.pnp_csmri_plan_create(ctypes.byref(h), 64, 64, 1, native.F32) != ERR_HIP:
        lib.pnp_csmri_plan_destroy.argtypes = [ctypes.c_void_p]
        lib.pnp_csmri_plan_destroy(h)
        sys.exit('a device is visible to the replay: no case run')
    table = json.load(open(path))
    json.dump([call(lib, native.SIGNATURES, c['entry'], arguments(table, c)) for c in table['cases']], sys.stdout)


HIDE = dict(HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lib', help='the library to record from (default: the built one of this tree)')
    ap.add_argument('-o', dest='out', default=OUT)
    ap.add_argument('--replay', action='store_true', help='run the cases of the file (-o) and print [[code, text], ...] instead')
    a = ap.parse_args()
    native = load_native()
    lib = ctypes.CDLL(a.lib or native.LIB_PATH)
    if a.replay:
        return replay(lib, native, a.out)
    if os.path.exists('/dev/kfd'):
        sys.exit('record on a machine without a GPU: a case the checks let through has to end at the first HIP call')
    bases, cases = build_cases(native.SIGNATURES)
    table = dict(base=bases, cases=[])
    for entry, name, sets, through in cases:
        case = dict(entry=entry, case=name, set=sets)
        rc, text = call(lib, native.SIGNATURES, entry, arguments(table, case))
        want = ERR_HIP if through else ERR_ARG
        assert rc == want, f'{entry} / {name}: code {rc} ({text}), the case was written for {want}'
        table['cases'].append(dict(case, rc=rc, error=text if rc == ERR_ARG else None))
    with open(a.out, 'w') as f:
        f.write('{"base": {\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in bases.items()) + '\n},\n"cases": [\n'
                + ',\n'.join(json.dumps(t) for t in table['cases']) + '\n]}\n')
    n_arg = sum(t['rc'] == ERR_ARG for t in table['cases'])
    print(f'{len(table["cases"])} cases over {len(bases)} entry points: {n_arg} refused, {len(table["cases"]) - n_arg} let through -> {a.out}')


if __name__ == '__main__':
    main()
