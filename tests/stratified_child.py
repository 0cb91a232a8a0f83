"""The device side of tests/test_gpu_stratified.py, and its child process: ROX_SMALL_BLOCKS is read
once per process, so each forced workgroup form gets a process of its own.

    python tests/stratified_child.py <dir with the oracle's <case>.npz>

Traces the pupil grid of every stratified system (tests/stratified_systems.py) -- alone and as a
rox_trace_pupil_grids batch over the three wavelengths, modes FULL / LAST / HITS, apertures checked
and unchecked -- compares with the oracle bit for bit and prints one JSON line:
{"failures": [...], "launches": [32 counts of rox_diag_trace_launches]}.  With ROX_SMALL_BLOCKS
set, a launch in the other workgroup form is a failure."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_FORMS = 32


def form(inst, fast, small):
    """index of a launch form in rox_diag_trace_launches"""
    return (inst * 2 + fast) * 2 + small


def form_name(i):
    import stratified_systems as S
    inst = S.INSTANCES[i >> 2] if (i >> 2) < len(S.INSTANCES) else 'general_gtab'
    return inst + ('/fast' if i & 2 else '') + ('/small' if i & 1 else '/regular')


def trace_counts(lib):
    c = (C.c_uint64 * N_FORMS)()
    assert lib.rox_diag_trace_launches(c, N_FORMS) == 0
    return np.array(c[:], dtype=np.int64)


class Launches:
    """what the counter saw between two looks: `took(...)` checks the launches since the last one"""

    def __init__(self, lib, failures):
        self.lib, self.failures = lib, failures
        self.last = trace_counts(lib)
        self.total = np.zeros(N_FORMS, dtype=np.int64)

    def by_form(self):
        return {form_name(i): int(self.total[i]) for i in np.flatnonzero(self.total)}

    def took(self, what, n, inst, small=None):
        """n launches since the last look, all of instance `inst`, exact (fast = 0), and -- where
        `small` is given -- all in that workgroup form"""
        now = trace_counts(self.lib)
        d, self.last = now - self.last, now
        self.total += d
        ok = [form(inst, 0, s) for s in ((0, 1) if small is None else (int(small),))]
        if d.sum() != n or d[ok].sum() != n:
            self.failures.append(f'{what}: expected {n} launch(es) of form(s) {ok}, the counter '
                                 f'shows {dict((form_name(i), int(d[i])) for i in np.flatnonzero(d))}')


def trace_grids(eng, c, ref, launches, failures, small, modes=None, checks=(1, 0)):
    """the grid and batch part of the matrix for one system"""
    import stratified_systems as S
    from rayoptics_amd.engine import make_grid, make_opts
    inst = S.expected_instance(c.table)
    grid = c.grid(make_grid)
    W = len(S.WVLS)
    for check in checks:
        for mode in (modes or S.MODES):
            what = f'{c.name} mode {mode} check {check}'
            opts = c.grid_opts(make_opts, mode, check)
            one = eng.trace_pupil_grid(c.field, grid, c.wvl, opts, nan_fill=True).to_host()
            launches.took(what + ' grid', 1, inst, small)
            S.compare(one, ref[f'grid/{c.wvl}/{mode}/{check}'], what + ' grid', failures)
            res = eng.trace_pupil_grids([c.field] * W, list(range(W)), grid, [opts] * W, nan_fill=True)
            launches.took(what + ' batch', 1, inst, small)
            for w, r in enumerate(res):
                S.compare(r.to_host(), ref[f'grid/{w}/{mode}/{check}'], what + f' batch item {w}', failures)


def load_refs(refdir, name):
    """{key: {field: array}} of one case, as the parent stored it (save_refs)"""
    out = {}
    with np.load(os.path.join(refdir, name + '.npz')) as z:
        for k in z.files:
            key, f = k.rsplit('|', 1)
            out.setdefault(key, {})[f] = z[k]
    return out


def save_refs(refdir, name, ref):
    np.savez(os.path.join(refdir, name + '.npz'),
             **{f'{key}|{f}': a for key, arrs in ref.items() if key.startswith('grid/') for f, a in arrs.items()})


def main():
    refdir = sys.argv[1]
    import rayoptics_amd  # noqa: F401
    import stratified_systems as S
    from rayoptics_amd.engine import TraceEngine, load_library
    forced = os.environ.get('ROX_SMALL_BLOCKS')
    small = None if forced is None else forced == '1'
    failures = []
    launches = Launches(load_library(), failures)
    for c in S.cases():
        eng = TraceEngine(c.table, device='cuda:0')
        trace_grids(eng, c, load_refs(refdir, c.name), launches, failures, small)
        eng.close()
    if small is not None:       # every launch of the process, not only those looked at one by one
        total = trace_counts(launches.lib)
        other = [i for i in range(N_FORMS) if (i & 1) != int(small) and total[i]]
        if other:
            failures.append(f'ROX_SMALL_BLOCKS={forced}: launches in the other form, counters {other}')
    print(json.dumps({'failures': failures[:40], 'n_failures': len(failures),
                      'launches': [int(v) for v in launches.total]}))


if __name__ == '__main__':
    main()
