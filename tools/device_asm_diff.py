#!/usr/bin/env python3
"""Is the device code of two trees the same?  No GPU needed.

    python tools/device_asm_diff.py <base-tree> <this-tree> [--jobs N] [--only inst_lean,fast_lean]

Every ray-optics_amd/csrc/*.hip present in either tree is compiled to gfx950 assembly with the
build's own flags (<this-tree>/ray-optics_amd/build.py FLAGS) plus `--cuda-device-only -S`;
hipcc's output for one input is deterministic.  Lines that name the per-compilation
`__hip_cuid_<hash>` symbol and the `.file` / `.ident` directives are dropped and the rest is
compared as text.  One line per translation unit; where a unit differs, the kernels whose
bodies differ with old -> new code size and register / scratch figures from their kernel
descriptors.  Exit status 0 only when every unit is identical.

This is the criterion of a refactor of the kernels' headers: identical text is identical code,
so nothing has to be timed."""
import argparse
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile


def load_build(tree):
    spec = importlib.util.spec_from_file_location('rox_build', os.path.join(tree, 'ray-optics_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def units(tree):
    d = os.path.join(tree, 'ray-optics_amd', 'csrc')
    return {f[:-4] for f in os.listdir(d) if f.endswith('.hip')} if os.path.isdir(d) else set()


def device_asm(cc, flags, tree, unit, out):
    src = os.path.join(tree, 'ray-optics_amd', 'csrc', unit + '.hip')
    if not os.path.exists(src):
        return None
    p = subprocess.run([cc, *flags, '--cuda-device-only', '-S', src, '-o', out], stderr=subprocess.PIPE, text=True)
    if p.returncode:
        raise RuntimeError(f'{src} does not compile:\n{p.stderr}')
    with open(out) as f:
        return [ln.rstrip('\n') for ln in f
                if '__hip_cuid_' not in ln and not re.match(r'\s*\.(file|ident)\b', ln)]


FIGURES = (('vgpr', r'\.amdhsa_next_free_vgpr\s+(\d+)'), ('sgpr', r'\.amdhsa_next_free_sgpr\s+(\d+)'),
           ('scratch', r'; ScratchSize:\s*(\d+)'), ('code', r'; codeLenInByte = (\d+)'))


def kernels(asm):
    """{symbol: (body lines, figures)} of the kernels of one unit's assembly: a kernel's code runs
    from its label to its `.amdhsa_kernel` descriptor, the figures follow up to the next function.
    (Block labels carry the function's index in the unit: taken out, so that a kernel added or
    removed in front does not make every later body differ.)"""
    label = {ln.split(':')[0]: i for i, ln in enumerate(asm) if re.match(r'[\w.$]+:', ln)}
    out = {}
    for i, ln in enumerate(asm):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln)
        if not m:
            continue
        stop = next((j for j in range(i, len(asm)) if '-- Begin function' in asm[j]), len(asm))
        text = '\n'.join(asm[i:stop])
        fig = {k: (lambda f: int(f.group(1)) if f else None)(re.search(p, text)) for k, p in FIGURES}
        body = [re.sub(r'\.L(BB|func_begin|func_end|tmp)\d+', r'.L\1', s) for s in asm[label[m.group(1)]:i]]
        out[m.group(1)] = (body, fig)
    return out


def report(unit, a, b):
    if a is None or b is None:
        print(f'{unit}: only in the {"new" if a is None else "base"} tree')
        return False
    if a == b:
        print(f'{unit}: identical ({len(a)} lines)')
        return True
    ka, kb = kernels(a), kernels(b)
    differ = [k for k in sorted(set(ka) | set(kb)) if k not in ka or k not in kb or ka[k][0] != kb[k][0]]
    print(f'{unit}: DIFFERENT ({len(a)} -> {len(b)} lines, {len(differ)} of {len(set(ka) | set(kb))} kernel bodies)')
    for k in differ:
        fa, fb = (ka[k][1] if k in ka else None), (kb[k][1] if k in kb else None)
        fmt = lambda f: 'absent' if f is None else ' '.join(f'{n}={f[n]}' for n, _ in FIGURES)
        print(f'    {k}\n        {fmt(fa)}  ->  {fmt(fb)}')
    return False


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('base')
    ap.add_argument('tree')
    ap.add_argument('--jobs', type=int, default=None)
    ap.add_argument('--only', default=None, help='comma-separated translation units (inst_lean,fast_lean)')
    args = ap.parse_args()
    build = load_build(args.tree)
    cc = build.hipcc()
    jobs = min(16, args.jobs or build.jobs())
    todo = sorted(units(args.base) | units(args.tree))
    if args.only:
        todo = [u for u in todo if u in set(args.only.split(','))]
    with tempfile.TemporaryDirectory() as td, concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        fut = {(u, side): ex.submit(device_asm, cc, build.FLAGS, tree, u, os.path.join(td, f'{side}_{u}.s'))
               for u in todo for side, tree in (('a', args.base), ('b', args.tree))}
        same = [report(u, fut[u, 'a'].result(), fut[u, 'b'].result()) for u in todo]
    print(f'{sum(same)} of {len(same)} translation units identical')
    return 0 if same and all(same) else 1


if __name__ == '__main__':
    sys.exit(main())
