"""-m gpu, round 3: packed hits appended over several launches (ROX_HITS_APPEND) into HBM
and into pinned / shared host memory, the sharded spot diagram through both exchanges on
one rank, tables beyond 64 KiB of LDS, BASELINE configs[2] from the .zmx import at full
size, and bench.py launching its own ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from rayoptics_amd import abi, SurfaceTable, field_struct
import helpers as H

pytestmark = pytest.mark.gpu

SPOT = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_hits(wl, fi, wi, grid_kw, flags=SPOT):
    from oracle import oracle
    N = wl.n_ifcs
    o = oracle.make_opts(flags=flags, out_mode=abi.OUT_HITS_COMPACT, first_surf=1, last_surf=N - 2,
                         foc=wl.foc, image_pt=wl.image_pts[fi])
    return oracle.trace_pupil_grid(wl.table, wl.fields[fi], oracle.make_grid((-1., -1.), (1., 1.), **grid_kw),
                                   wi, o).hits


def test_hits_append_packs_several_grids_without_a_host_round_trip():
    """three (field, wavelength) grids and two row blocks appended into one buffer: the
    buffer equals the concatenation of the oracle's packed hits, the per-launch counts come
    back in one read; the same into a pinned host destination"""
    import torch
    from rayoptics_amd import workloads
    from rayoptics_amd.engine import TraceEngine, make_opts, make_grid, _pool
    wl = workloads.load('dblgauss_c2')
    N = wl.n_ifcs
    eng = TraceEngine(wl.table)
    jobs = [(0, 0, dict(num=96)), (2, 1, dict(num=96)), (1, 2, dict(num=96, row_begin=10, row_count=37)),
            (2, 0, dict(num=96, row_begin=47, row_count=49)), (1, 1, dict(num=5))]
    want = [oracle_hits(wl, fi, wi, kw) for fi, wi, kw in jobs]
    cap = sum((kw.get('row_count') or kw['num']) * kw['num'] for _f, _w, kw in jobs)
    for where in ('hbm', 'pinned'):
        lease = None
        dest = None
        if where == 'pinned':
            lease = _pool.take(torch, 16 * cap)
            dest = (lease.ptr, cap)
        pack = eng.hits_pack(cap, len(jobs), dest=dest)
        for fi, wi, kw in jobs:
            o = make_opts(flags=SPOT | abi.HITS_APPEND, out_mode=abi.OUT_HITS_COMPACT, first_surf=1,
                          last_surf=N - 2, foc=wl.foc, image_pt=wl.image_pts[fi])
            eng.trace_pupil_grid_hits_append(wl.fields[fi], make_grid((-1., -1.), (1., 1.), **kw), wi, o, pack)
        counts = pack.counts()
        np.testing.assert_array_equal(counts, [len(w) for w in want])
        total = int(counts.sum())
        got = pack.xy[:total].cpu().numpy() if where == 'hbm' else lease.array((total, 2), np.float64)
        assert np.array_equal(got, np.concatenate(want)), where
        assert int(pack.count.item()) == total
        with pytest.raises(Exception, match='full'):
            o = make_opts(flags=SPOT | abi.HITS_APPEND, out_mode=abi.OUT_HITS_COMPACT, first_surf=1,
                          last_surf=N - 2, foc=wl.foc, image_pt=wl.image_pts[0])
            eng.trace_pupil_grid_hits_append(wl.fields[0], make_grid((-1., -1.), (1., 1.), 96), 0, o, pack)
    # appending is refused in the other output modes
    from rayoptics_amd.engine import EngineError
    with pytest.raises(EngineError, match='HITS_APPEND'):
        eng.trace_pupil_grid(wl.fields[0], make_grid((-1., -1.), (1., 1.), 8), 0,
                             make_opts(flags=SPOT | abi.HITS_APPEND, out_mode=abi.OUT_HITS, first_surf=1,
                                       last_surf=N - 2))
    eng.close()


def test_hits_append_over_chunked_launches():
    """ROX_RAYS_PER_LAUNCH=4096: every appended grid is several launches whose running
    total ping-pongs between two device slots (subprocess: the limit is read once)"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import rayoptics_amd
from rayoptics_amd import abi, workloads
from rayoptics_amd.engine import TraceEngine, make_opts, make_grid
from oracle import oracle
wl = workloads.load('rc_telescope_c4'); N = wl.n_ifcs
eng = TraceEngine(wl.table)
SPOT = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
pack = eng.hits_pack(5 * 150 * 150, 5)
want = []
for fi in range(5):
    o = make_opts(flags=SPOT | abi.HITS_APPEND, out_mode=abi.OUT_HITS_COMPACT, first_surf=1, last_surf=N - 2,
                  foc=wl.foc, image_pt=wl.image_pts[fi])
    eng.trace_pupil_grid_hits_append(wl.fields[fi], make_grid((-1., -1.), (1., 1.), 150), 0, o, pack)
    oo = oracle.make_opts(flags=SPOT, out_mode=abi.OUT_HITS_COMPACT, first_surf=1, last_surf=N - 2,
                          foc=wl.foc, image_pt=wl.image_pts[fi])
    want.append(oracle.trace_pupil_grid(wl.table, wl.fields[fi], oracle.make_grid((-1., -1.), (1., 1.), 150), 0, oo).hits)
c = pack.counts()
assert list(c) == [len(w) for w in want], (c, [len(w) for w in want])
assert np.array_equal(pack.xy[:int(c.sum())].cpu().numpy(), np.concatenate(want))
print('chunked append ok', int(c.sum()))
''' % (ROOT, os.path.join(ROOT, 'tests'))
    env = dict(os.environ, ROX_RAYS_PER_LAUNCH='4096')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'chunked append ok' in r.stdout


@pytest.mark.parametrize('pipeline', [True, False])
@pytest.mark.parametrize('exchange', ['rccl', 'host'])
def test_sharded_spot_one_rank_both_exchanges(exchange, pipeline):
    """dist.trace_spot_sharded without a process group: the packed pairs reach host memory
    through the D2H copy ('rccl') or are written by the kernels straight into a registered
    MAP_SHARED segment ('host'); both equal the oracle's survivors per grid"""
    from rayoptics_amd import workloads, dist as rdist
    from rayoptics_amd.engine import TraceEngine
    wl = workloads.load('dblgauss_c2')
    eng = TraceEngine(wl.table)
    num, nw = 160, len(wl.table.wvls)
    seg = None
    if exchange == 'host':
        plan = rdist.partition(len(wl.fields), nw, num, 1)
        if pipeline:        # one region per (field, wavelength) grid
            seg = rdist.HostSegment.for_grids(eng, f'rox_test_seg_{os.getpid()}', len(wl.fields) * nw, num, 0,
                                              create=True)
        else:               # round 3's form: one slice per rank, written by the kernels themselves
            seg = rdist.HostSegment(eng, f'rox_test_seg_{os.getpid()}', [rdist.rays_of(plan[0], num)], 0,
                                    create=True)
    try:
        tm = {}
        # (pipelined: pieces of 7 000 rays, so that every grid is several launches and copies)
        out = rdist.trace_spot_sharded(eng, wl.fields, wl.image_pts, nw, num, wl.foc, exchange=exchange,
                                       segment=seg, timings=tm, pipeline=pipeline, max_piece_rays=7000)
        assert len(out) == len(wl.fields) * nw
        for (fi, wi), xy in out.items():
            want = oracle_hits(wl, fi, wi, dict(num=num))
            assert np.array_equal(xy, want), (exchange, fi, wi)
        assert tm['pairs_total'] == sum(len(v) for v in out.values())
        if pipeline:
            assert tm['stages'] == tm['pieces'][0] > len(out)
            if exchange == 'rccl':      # the gather alone: the arrays stay in this GPU's memory
                dev = rdist.trace_spot_sharded(eng, wl.fields, wl.image_pts, nw, num, wl.foc, exchange='rccl',
                                               result_on='device', max_piece_rays=7000)
                for key, xy in out.items():
                    assert dev[key].is_cuda and np.array_equal(dev[key].cpu().numpy(), xy), key
    finally:
        if seg is not None:
            seg.close(unlink=True)
    eng.close()


def lens_chain(n_lenses):
    surfs = [dict(cv=0.0, thi=1.0e10, n=1.0, max_aperture=1e12)]
    for _ in range(n_lenses):
        surfs.append(dict(cv=1 / 103.0, thi=4.0, n=[1.5168, 1.5200, 1.5140], max_aperture=14.0))
        surfs.append(dict(cv=-1 / 103.0, thi=46.0, n=1.0, max_aperture=14.0))
    surfs.append(dict(cv=0.0, thi=0.0, n=1.0, max_aperture=50.0))
    return SurfaceTable.from_prescription(surfs, wvls=(587.6, 486.1, 656.3), stop_idx=1)


def test_tables_beyond_64_kib_of_lds():
    """122 and 202 interfaces: 90 and 150 KB of dynamic LDS per workgroup (the default
    limit is 64 KiB; the instance's limit is raised on first use), FULL packets and hits
    bit-exact vs the oracle; explicit rays with per-ray wavelengths stage all three index
    rows; the aiming kernel stages the same table"""
    from oracle import oracle
    from rayoptics_amd.engine import TraceEngine, make_opts, make_grid
    for n_lenses in (60, 100):
        tbl = lens_chain(n_lenses)
        N = tbl.n_ifcs
        assert N == 2 * n_lenses + 2
        eng = TraceEngine(tbl)
        theta = np.deg2rad(0.4)
        fld = field_struct([0.0, -1.0e10 * np.tan(theta), 0.0], (0., 0.), 9.0, 1.0e10)
        grid = make_grid((-1., -1.), (1., 1.), 48)
        for mode in (abi.OUT_FULL, abi.OUT_HITS):
            opts = make_opts(flags=SPOT, out_mode=mode, first_surf=1, last_surf=N - 2)
            dev = eng.trace_pupil_grid(fld, grid, 1, opts, nan_fill=True).to_host()
            orc = oracle.trace_pupil_grid(tbl, fld, oracle.make_grid((-1., -1.), (1., 1.), 48), 1, opts)
            np.testing.assert_array_equal(dev.status, orc.status)
            assert np.array_equal(dev.seg, orc.seg, equal_nan=True), (N, mode)
            assert np.array_equal(dev.op, orc.op, equal_nan=True)
            assert (dev.status == 0).sum() > 500
        rng = np.random.default_rng(N)
        R = 700
        pt0 = np.stack([rng.uniform(-8, 8, R), rng.uniform(-8, 8, R), np.full(R, -50.0)])
        d = np.stack([rng.uniform(-.01, .01, R), rng.uniform(-.01, .01, R), np.ones(R)])
        d /= np.linalg.norm(d, axis=0)
        wi = rng.integers(0, 3, R).astype(np.int32)
        opts = make_opts(flags=abi.CHECK_APERTURES, out_mode=abi.OUT_LAST, first_surf=1, last_surf=N - 2)
        dev = eng.trace_rays(pt0, d, wi, opts, nan_fill=True).to_host()
        orc = oracle.trace_rays(tbl, pt0, d, wi, opts)
        np.testing.assert_array_equal(dev.status, orc.status)
        assert np.array_equal(dev.seg, orc.seg, equal_nan=True)
        if n_lenses > 60:       # (the aiming kernel stages every wavelength's rows: 175 KB at 202)
            eng.close()
            continue
        a = abi.Aim()
        a.pt0[1] = -1.0e10 * np.tan(theta)
        a.z_enp, a.y_target, a.z_dir0, a.wvl_idx, a.surf, a.flip = 1.0e10, 0.0, 1.0, 1, 1, 1
        y_dev, r_dev = eng.aim_chief_rays([a])
        y_orc, r_orc = oracle.aim_chief_rays(tbl, [a], 1e-12)
        assert r_dev[0] == r_orc[0] and np.array_equal(y_dev, y_orc)
        eng.close()


def test_c3_zmx_import_3fields_3wvls_512():
    """BASELINE configs[2] from the .zmx import (US08427765-1.ZMX: 13 interfaces, one
    EVENASPH, wide-angle 'real height' fields): 3 fields x 3 wavelengths x 512x512 hits
    bit-exact vs the oracle, FULL packets on a 192x192 grid"""
    from oracle import oracle
    from rayoptics_amd import workloads
    from rayoptics_amd.engine import TraceEngine, make_opts, make_grid
    wl = workloads.load('zmx_evenasph_c3')
    N = wl.n_ifcs
    assert N == 13 and len(wl.fields) == 3 and len(wl.table.wvls) == 3
    assert all(f.kind == abi.FLD_EPD_WIDE for f in wl.fields)
    flags = abi.CHECK_APERTURES | abi.APPLY_VIGNETTING       # wide angle: the object is not intersected
    eng = TraceEngine(wl.table)
    grid = make_grid((-1., -1.), (1., 1.), 512)
    through = 0
    for fi in range(3):
        for wi in range(3):
            opts = make_opts(flags=flags, out_mode=abi.OUT_HITS, first_surf=1, last_surf=N - 2,
                             foc=wl.foc, image_pt=wl.image_pts[fi])
            dev = eng.trace_pupil_grid(wl.fields[fi], grid, wi, opts, nan_fill=True).to_host()
            orc = oracle.trace_pupil_grid(wl.table, wl.fields[fi], oracle.make_grid((-1., -1.), (1., 1.), 512),
                                          wi, opts)
            np.testing.assert_array_equal(dev.status, orc.status)
            np.testing.assert_array_equal(dev.fail_surf, orc.fail_surf)
            assert np.array_equal(dev.seg, orc.seg, equal_nan=True), (fi, wi)
            through += int((dev.status == 0).sum())
    assert 0.3 * 9 * 512 * 512 < through < 0.9 * 9 * 512 * 512
    opts = make_opts(flags=flags, out_mode=abi.OUT_FULL, first_surf=1, last_surf=N - 2)
    g = make_grid((-1., -1.), (1., 1.), 192)
    dev = eng.trace_pupil_grid(wl.fields[2], g, 0, opts, nan_fill=True).to_host()
    orc = oracle.trace_pupil_grid(wl.table, wl.fields[2], oracle.make_grid((-1., -1.), (1., 1.), 192), 0, opts)
    np.testing.assert_array_equal(dev.status, orc.status)
    assert np.array_equal(dev.seg, orc.seg, equal_nan=True) and np.array_equal(dev.op, orc.op, equal_nan=True)
    eng.close()


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it: the script re-executes itself
    under torch.distributed.run (here two ranks sharing device 0, gloo carrying the
    collectives) and rank 0 prints exactly one JSON line.  At N > 1 the headline is the
    strong-scaled spot problem with the exchange INSIDE the timed region (verdict r3 #2): the
    line says so, its time per step covers at least this rank's kernels plus the delivery of
    every grid, and the collective-free figure has moved to `weak_full`"""
    env = dict(os.environ, ROX_BENCH_BACKEND='gloo', ROX_BENCH_SHARE_GPU='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3',
                        '--warmup', '1', '--strong-num', '192', '--full', '--no-cpu-baseline', '--no-configs'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    b = json.loads(lines[0])
    assert b['ok'] is True
    assert b['n_gpus'] == 2 and b['ranks_seen_by_backend'] == 2
    # the headline: fixed total work, exchange inside the timed region
    assert b['scaling'] == 'strong' and 'exchange inside the timed region' in b['headline']
    assert 'configs[4]' in b['config']['workload']
    # both exchanges are timed with the exchange inside the timed region; the headline is the faster
    h = b['strong_headline']
    # (+ the gather alone -- the pairs left in rank 0's HBM: north_star's "RCCL gather over xGMI" --
    # beside them, never the headline)
    assert set(h['ms_per_step_by_exchange']) == {'rccl', 'host', 'rccl_device'} and not h['errors']
    to_host = {k: v for k, v in h['ms_per_step_by_exchange'].items() if k != 'rccl_device'}
    assert h['exchange'] == min(to_host, key=to_host.get)
    assert b['rccl_gather_only_ms'] == h['ms_per_step_by_exchange']['rccl_device']
    assert b['preflight']['ok'] and list(b['preflight']['steps_ms']) == [
        'all_gather_on_side_stream', 'grouped_isend_irecv_to_rank0', 'all_reduce_fence']
    assert b['config']['exchange'].startswith(h['exchange'])
    assert b['ms_per_step'] == pytest.approx(h['ms_per_step_by_exchange'][h['exchange']])
    assert b['config']['rays_per_step'] == 45 * 192 * 192
    assert 0 < b['config']['pairs_to_host'] < b['config']['rays_per_step']
    assert b['strong_headline']['grids_delivered'] == 45
    assert b['value'] == pytest.approx(b['config']['intersections_per_step'] / (b['ms_per_step'] * 1e-3))
    assert set(b['predicted_ms']['rccl_to_host']) == {'1', '2', '4', '8'}
    # a pass cannot be shorter than the kernels of the busiest rank
    s = b['strong_scaling']
    assert b['ms_per_step'] >= 0.5 * s['c5']['kernel_ms_max_over_ranks']
    # the weak figure is still there, under its own key
    w = b['weak_full']
    assert w['scaling'] == 'weak' and w['value'] > 1e9 and 'FULL' in w['config']['workload']
    assert s['ranks'] == 2 and s['ranks_seen_by_backend'] == 2
    # (rccl_tolerance_mode: the same problem behind the opt-in ROX_FAST_FP64 kernels -- the same
    # rays get through on this lens, so the same number of pairs arrives)
    assert b['bench_wall_s'] > 0
    for prob, variants in (('c5', ('rccl', 'host', 'rccl_device', 'rccl_unpipelined', 'rccl_tolerance_mode')),
                           ('c4', ('rccl', 'host')), ('c2_sharded', ('rccl', 'rccl_device'))):
        for ex in variants:
            rec = s[prob][ex]
            assert 'error' not in rec, (prob, ex, rec)
            assert rec['end_to_end_ms'] > 0 and 0 < rec['pairs'] < s[prob]['rays'], (prob, ex)
        assert len({s[prob][ex]['pairs'] for ex in variants}) == 1
    assert s['c5']['rccl']['grids_delivered'] == 45 and s['c4']['rccl']['grids_delivered'] == 5
    assert s['c2_sharded']['rccl']['grids_delivered'] == 1


def test_bench_reports_a_hung_exchange_and_keeps_its_line():
    """the watchdog around the legs that contain collectives: with a timeout they cannot meet,
    rank 0 still prints exactly one JSON line -- the weak figure measured before, "ok": false,
    the leg that hung named -- and the run ends with exit status 3 (a deadlock must
    not look like success)"""
    env = dict(os.environ, ROX_BENCH_BACKEND='gloo', ROX_BENCH_SHARE_GPU='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '5',
                        '--warmup', '2', '--full', '--no-cpu-baseline', '--no-configs', '--strong-timeout', '0.02'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode != 0
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    b = json.loads(lines[0])
    assert b['ok'] is False and b['hung_in'] in ('strong_headline', 'strong_scaling')
    assert b['n_gpus'] == 2 and b['value'] > 1e9 and b['roofline']['frac'] > 0.1
    assert 'timed out' in b['strong_scaling']['error']


def test_bench_force_dist_rehearses_the_strong_headline_on_one_rank():
    """--force-dist: the N > 1 code path (process group, fences, the pipelined exchange as the
    headline) with a single rank"""
    env = dict(os.environ, ROX_BENCH_BACKEND='gloo')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env['MASTER_PORT'] = str(29000 + os.getpid() % 900)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--force-dist',
                        '--steps', '3', '--warmup', '1', '--strong-num', '256', '--no-cpu-baseline',
                        '--no-configs', '--no-strong'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    b = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    # --no-strong also skips the headline leg: the weak line, unchanged
    assert b['scaling'] == 'weak' and 'weak_full' not in b


def aim2d_problem(m, wvl_idx=None):
    a = abi.Aim()
    for i in range(3):
        a.pt0[i] = m['pt0'][i]
    a.z_enp, a.x_target, a.y_target, a.z_dir0 = m['z_enp'], 0.0, 0.0, m['z_dir0']
    a.wvl_idx, a.surf, a.flip = (m['wvl_idx'] if wvl_idx is None else wvl_idx), m['surf'], 1
    a.two_d, a.epsfcn = 1, m['epsfcn']
    return a


def test_two_dimensional_chief_ray_aiming():
    """iterate_ray's fsolve branch (fields off the y axis) in the batched aiming launch:
    MINPACK's hybrd per lane == the CPU restatement (itself bit-identical to SciPy's fsolve)
    bit for bit, == the aim points the reference itself found (stored with the workloads);
    mixed with 1-D problems in one launch; perturbed problems incl. ones whose trial rays fail"""
    from oracle import oracle
    from rayoptics_amd import workloads
    from rayoptics_amd.engine import TraceEngine
    rng = np.random.default_rng(4)
    n_err = n_conv = 0
    for name in ('dblgauss_c2', 'nikkor_c3', 'cell_phone', 'singlet_c1', 'rc_telescope_c4', 'litho_c5'):
        wl = workloads.load(name)
        assert wl.aim2d, name
        eng = TraceEngine(wl.table)
        probs = [aim2d_problem(m) for m in wl.aim2d]
        aim, res = eng.aim_chief_rays(probs)
        for m, xy, r in zip(wl.aim2d, aim, res):
            assert r != abi.AIM_TRACE_ERROR     # (ier is not consulted by iterate_ray)
            assert np.array_equal(xy, m['aim']), (name, xy, m['aim'])
        # every wavelength, the 1-D problems of the workload in between, perturbed copies
        allp = []
        for w in range(len(wl.table.wvls)):
            for m in wl.aim2d:
                allp.append(aim2d_problem(m, w))
                p = aim2d_problem(m, w)
                p.pt0[0] *= rng.uniform(0.2, 3.0)
                p.pt0[1] *= rng.uniform(0.2, 3.0)
                p.z_enp *= rng.uniform(0.7, 1.3)
                p.epsfcn *= 10.0 ** rng.uniform(-3, 1)
                p.x_target, p.y_target = rng.normal(size=2) * 0.05
                allp.append(p)
            for m in wl.aim or []:
                a = abi.Aim()
                for i in range(3):
                    a.pt0[i] = m['pt0'][i]
                a.z_enp, a.y_target, a.z_dir0 = m['z_enp'], 0.0, m['z_dir0']
                a.wvl_idx, a.surf, a.flip = w, m['surf'], 1
                allp.append(a)
        a_dev, r_dev = eng.aim_chief_rays(allp)
        a_orc, r_orc = oracle.aim_chief_rays(wl.table, allp)
        np.testing.assert_array_equal(r_dev, r_orc)
        assert np.array_equal(a_dev, a_orc, equal_nan=True), name
        n_err += int((r_dev == abi.AIM_TRACE_ERROR).sum())
        n_conv += int((r_dev == abi.AIM_CONVERGED).sum())
        eng.close()
    assert n_conv > 100


# ---------------------------------------------------------------- wide-angle pupil search
@pytest.mark.parametrize('name', ['dblgauss', 'nikkor'])
def test_wide_angle_pupil_search_on_the_device(name):
    """rox_find_real_enp (wideangle.find_real_enp: sampled walk, find_edge, newton, brentq;
    one lane per problem): z_enp, the last trial ray's z and the result code identical to the
    oracle's, z_enp identical to what the reference itself returned (tests/golden/
    wideangle.npz), ROX_ENP_REFERENCE_RAISES exactly where the reference raised"""
    from oracle import oracle
    from rayoptics_amd.engine import TraceEngine
    from test_oracle_wideangle import golden_model
    tbl, probs, z_ref, raised = golden_model(name)
    eng = TraceEngine(tbl)
    z_d, res_d = eng.find_real_enp(probs)
    z_o, res_o = oracle.find_real_enp(tbl, probs)
    np.testing.assert_array_equal(res_d, res_o)
    np.testing.assert_array_equal(z_d, z_o)
    np.testing.assert_array_equal(res_d == abi.ENP_REFERENCE_RAISES, raised)
    ok = ~raised
    np.testing.assert_array_equal(z_d[ok, 0], z_ref[ok])
    # one problem at a time gives the same answers (no cross-lane state)
    for k in (0, 7, len(probs) - 1):
        z1, r1 = eng.find_real_enp(probs[k:k + 1])
        assert r1[0] == res_d[k] and np.array_equal(z1[0], z_d[k])
    eng.close()
