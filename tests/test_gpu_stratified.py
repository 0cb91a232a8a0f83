"""-m gpu: every bit-exact trace instance, in both workgroup forms, on rays that get through.

tests/stratified_systems.py builds three tame systems per compiled feature instance (lean, even,
radial, poly, aplist, evenap, general), each with tilts and decentres in both rt_orders, conics, a
DUMMY or PHANTOM row and, in half of them, a mirror; tests/test_stratified_systems_host.py proves
on the CPU that rays traverse them and are lost in the rear half too.  Here every system goes
through the pupil-grid entry (45 x 46 rays: the last tile is ragged at 1024, 512 and 256
threads), the batched entry, a ray list with per-ray wavelengths (the regular kernels), a 65-ray
list (the small-workgroup kernels) and packed hits in both forms -- modes FULL, LAST and HITS,
apertures checked and unchecked -- and must equal the oracle bit for bit, zero signs included.
rox_diag_trace_launches says which kernel each call took: the instance the Python restatement of
the launch policy predicts, never the tolerance-mode twin, in the workgroup form the launch rule
gives these sizes.  ROX_FILTER_PHANTOMS must move the systems with a PHANTOM row to `general`;
two child processes force each workgroup form on every grid launch (ROX_SMALL_BLOCKS)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from rayoptics_amd import abi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

GENERAL = 6


@pytest.fixture()
def pack_form():
    """sets ROX_PACK_TWO_PASS for the library (read per call) and restores it"""
    saved = os.environ.get('ROX_PACK_TWO_PASS')

    def set_(v):
        os.environ['ROX_PACK_TWO_PASS'] = v
    yield set_
    if saved is None:
        os.environ.pop('ROX_PACK_TWO_PASS', None)
    else:
        os.environ['ROX_PACK_TWO_PASS'] = saved


def pack_counts(lib):
    import ctypes as C
    c = (C.c_uint64 * 2)()
    assert lib.rox_diag_pack_launches(c) == 0
    return np.array([int(c[0]), int(c[1])])


def trace_lists(eng, c, ref, launches, failures, inst, keys=None, extra=0, modes=None, checks=(1, 0)):
    """the two ray lists of the matrix: per-ray wavelengths -> the regular kernels, 65 rays at one
    wavelength -> the small-workgroup kernels"""
    import stratified_systems as S
    from rayoptics_amd.engine import make_opts
    ps, ds = c.pt0[:, :S.R_SMALL], c.dir0[:, :S.R_SMALL]
    for check in checks:
        for mode in (modes or S.MODES):
            what = f'{c.name} mode {mode} check {check}'
            opts = c.list_opts(make_opts, mode, check, extra)
            k_list, k_small = keys or (f'list/{mode}/{check}', f'small/{mode}/{check}')
            got = eng.trace_rays(c.pt0, c.dir0, c.wi, opts, nan_fill=True).to_host()
            launches.took(what + ' list', 1, inst, small=False)
            S.compare(got, ref[k_list], what + ' list', failures)
            got = eng.trace_rays(ps, ds, c.wvl, opts, nan_fill=True).to_host()
            launches.took(what + ' 65-ray list', 1, inst, small=True)
            S.compare(got, ref[k_small], what + ' 65-ray list', failures)


def trace_packed(eng, c, ref, launches, failures, inst, pack_form):
    """packed hits in both forms: the pairs and their count are the oracle's"""
    import stratified_systems as S
    from full_placement_child import same_bits
    from rayoptics_amd.engine import make_grid, make_opts
    grid = c.grid(make_grid)
    W = len(S.WVLS)

    def same(got, key, what):     # (an OK ray can carry a NaN pair: equal, or both NaN)
        want = ref[key]['hits']
        if not same_bits(got, want):
            failures.append(f'{what}: {got.shape[0]} packed pairs, the oracle {want.shape[0]}'
                            + ('' if got.shape != want.shape else ', pairs differ'))
    for two_pass in (0, 1):
        pack_form(str(two_pass))
        for check in (1, 0):
            what = f'{c.name} packed two_pass {two_pass} check {check}'
            before = pack_counts(eng.lib)
            xy = eng.trace_pupil_grid_hits(c.field, grid, c.wvl, c.grid_opts(make_opts, abi.OUT_HITS_COMPACT, check))
            launches.took(what + ' grid', 1, inst)
            same(xy, f'pack_grid/{c.wvl}/{check}', what + ' grid')
            xy = eng.trace_rays_hits(c.pt0, c.dir0, c.wi, c.list_opts(make_opts, abi.OUT_HITS_COMPACT, check))
            launches.took(what + ' list', 1, inst)
            same(xy, f'pack_list/{check}', what + ' list')
            took = pack_counts(eng.lib) - before
            if took.tolist() != [2 * (1 - two_pass), 2 * two_pass]:
                failures.append(f'{what}: pack launches (fused, two-pass) = {took.tolist()}')
            if two_pass == 0:       # the batched entry packs in the fused form only
                opts = c.grid_opts(make_opts, abi.OUT_HITS_COMPACT, check)
                res = eng.trace_pupil_grids_hits([c.field] * W, list(range(W)), grid, [opts] * W)
                launches.took(what + ' batch', 1, inst)
                for w, xy in enumerate(res):
                    same(xy, f'pack_grid/{w}/{check}', what + f' batch item {w}')


def totals(cs):
    """per-instance figures for the record, from the oracle's FULL traces with apertures checked
    (rays through, late failures) and unchecked (TIR, MISSED)"""
    import stratified_systems as S
    t = dict(rays=0, through=0, late=0, tir=0, missed=0)
    for c in cs:
        ref, N = S.oracle_results(c), c.table.n_ifcs
        for key in (f'grid/{c.wvl}/%d/%d', 'list/%d/%d'):
            chk, unc = ref[key % (abi.OUT_FULL, 1)], ref[key % (abi.OUT_FULL, 0)]
            t['rays'] += len(chk['status'])
            t['through'] += int((chk['status'] == abi.OK).sum())
            t['late'] += int(((chk['status'] != abi.OK) & (chk['fail_surf'] >= N / 2)).sum())
            t['tir'] += int((unc['status'] == abi.TIR).sum())
            t['missed'] += int((unc['status'] == abi.MISSED_SURFACE).sum())
    return t


@pytest.mark.parametrize('instance', ['lean', 'even', 'radial', 'poly', 'aplist', 'evenap', 'general'])
def test_instance_equals_the_oracle_in_the_form_the_launch_rule_picks(instance, pack_form):
    import stratified_systems as S
    import stratified_child as child
    from helpers import record
    from rayoptics_amd.engine import TraceEngine
    failures = []
    launches = None
    for c in S.cases(instance):
        ref = S.oracle_results(c)
        inst = S.expected_instance(c.table)
        assert S.INSTANCES[inst] == instance
        eng = TraceEngine(c.table)
        launches = launches or child.Launches(eng.lib, failures)
        # at these sizes the launch rule gives grids, batches and scalar-wavelength lists the
        # small-workgroup kernels; lists with per-ray wavelengths keep the regular ones
        child.trace_grids(eng, c, ref, launches, failures, small=True)
        trace_lists(eng, c, ref, launches, failures, inst)
        trace_packed(eng, c, ref, launches, failures, inst, pack_form)
        eng.close()
    record('stratified', instance=instance, launches=launches.by_form(), **totals(S.cases(instance)))
    assert not failures, (len(failures), failures[:12])
    assert launches.total[child.form(S.INSTANCES.index(instance), 0, 0)] > 0
    assert launches.total[child.form(S.INSTANCES.index(instance), 0, 1)] > 0


def test_phantom_filtering_moves_every_instance_to_general():
    """FULL packets under ROX_FILTER_PHANTOMS of the systems that hold a PHANTOM row, at least
    one per instance: `general` takes the launch, and the packets are the oracle's"""
    import stratified_systems as S
    import stratified_child as child
    from helpers import record
    from rayoptics_amd.engine import TraceEngine, make_grid, make_opts
    failures = []
    launches = None
    seen = set()
    for c in S.cases():
        if not c.has_phantom:
            continue
        seen.add(c.instance)
        ref = S.oracle_results(c)
        assert S.expected_instance(c.table, abi.FILTER_PHANTOMS) == GENERAL
        eng = TraceEngine(c.table)
        assert eng.num_segments(abi.FILTER_PHANTOMS) == c.table.n_ifcs - 1
        launches = launches or child.Launches(eng.lib, failures)
        opts = c.grid_opts(make_opts, abi.OUT_FULL, 1, abi.FILTER_PHANTOMS)
        got = eng.trace_pupil_grid(c.field, c.grid(make_grid), c.wvl, opts, nan_fill=True).to_host()
        launches.took(c.name + ' filtered grid', 1, GENERAL, small=True)
        S.compare(got, ref['filt_grid'], c.name + ' filtered grid', failures)
        trace_lists(eng, c, ref, launches, failures, GENERAL, keys=('filt_list', 'filt_small'),
                    extra=abi.FILTER_PHANTOMS, modes=(abi.OUT_FULL,), checks=(1,))
        eng.close()
    assert seen == set(S.INSTANCES)
    record('stratified_phantom_filter', systems=len([c for c in S.cases() if c.has_phantom]),
           launches=launches.by_form())
    assert not failures, (len(failures), failures[:12])


@pytest.fixture(scope='module')
def oracle_refs(tmp_path_factory):
    """the oracle's grids of every system, computed once, as <case>.npz (removed afterwards:
    the FULL packets of 21 systems are ~300 MB)"""
    import shutil
    import stratified_systems as S
    import stratified_child as child
    d = str(tmp_path_factory.mktemp('stratified'))
    for c in S.cases():
        child.save_refs(d, c.name, S.oracle_results(c))
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize('small', [0, 1])
def test_forced_workgroup_form(oracle_refs, small):
    """ROX_SMALL_BLOCKS=0 / 1 (read once: a child process each): the grid and batch part of the
    matrix for all seven instances, every launch in the forced form"""
    import stratified_systems as S
    import stratified_child as child
    from helpers import record
    env = {k: v for k, v in os.environ.items() if k not in ('ROX_SMALL_BLOCKS', 'ROX_FORCE_INSTANCE')}
    env['ROX_SMALL_BLOCKS'] = str(small)
    p = subprocess.run([sys.executable, os.path.join(HERE, 'stratified_child.py'), oracle_refs],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    by_form = {child.form_name(i): n for i, n in enumerate(out['launches']) if n}
    record('stratified_forced_form', small=small, launches=by_form)
    assert not out['failures'], (out['n_failures'], out['failures'][:12])
    # 21 systems x 2 aperture settings x 3 modes x (grid + batch), each instance's share in its form
    for i in range(len(S.INSTANCES)):
        assert out['launches'][child.form(i, 0, small)] == 3 * 2 * 3 * 2, by_form
