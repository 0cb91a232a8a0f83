"""-m gpu: the argument checks of the search entries, the trace entries (with ROX_HOST_POINTERS and
without), rox_trace_pupil_grids and rox_time_pupil_grid answer what tests/golden/
host_entry_errors.json records: every return code and rox_last_error() text, in order, and the
bytes of a few valid calls behind them (singlet table, n = 1 problems, 4-ray batches).

The fixture was recorded from the library as it was before its host side was split into one
translation unit per concern, with this file's collect():

    ROX_LIB=<library> python tests/test_gpu_host_entry_errors.py <fixture.json>

Every call without ROX_HOST_POINTERS fails its checks before anything is launched (its buffers
are host memory)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'host_entry_errors.json')


def collect():
    """{'calls': [[name, rc, text or None when rc == 0], ...], 'valid': {name: hex bytes}}"""
    from rayoptics_amd import abi, workloads
    from rayoptics_amd.engine import TraceEngine, load_library, make_grid, make_opts
    lib = load_library()
    wl = workloads.load('singlet_c1')
    eng = TraceEngine(wl.table)
    h, N, fld, null = eng._handle, wl.n_ifcs, wl.fields[1], None
    calls = []

    def call(name, rc):
        calls.append([name, int(rc), lib.rox_last_error().decode() if rc != 0 else None])

    def ptr(a):
        return a.ctypes.data

    # ---- the five search entries
    m = wl.aim[1]
    aim = abi.Aim()
    aim.pt0[0], aim.pt0[1], aim.pt0[2] = m['pt0']
    aim.z_enp, aim.y_target, aim.z_dir0 = m['z_enp'], 0.0, m['z_dir0']
    aim.wvl_idx, aim.surf, aim.flip = m['wvl_idx'], m['surf'], 1
    xy, res, lxy, lst = np.zeros(2), np.zeros(1, np.int32), np.zeros(2), np.zeros(1, np.int32)

    def raw(name, sys_=h, n=1, probs=aim, xy_=xy, res_=res, lxy_=lxy, lst_=lst):
        call('iterate_ray_raw: ' + name, lib.rox_iterate_ray_raw(
            sys_, n, C.byref(probs) if probs is not None else null, 1e-12,
            ptr(xy_) if xy_ is not None else null, ptr(res_) if res_ is not None else null,
            ptr(lxy_) if lxy_ is not None else null, ptr(lst_) if lst_ is not None else null, null))

    def with_fields(proto, **kw):
        p = type(proto).from_buffer_copy(proto)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    raw('null system', sys_=null)
    raw('n < 0', n=-1)
    raw('null probs', probs=None)
    raw('null aim_xy', xy_=None)
    raw('null result', res_=None)
    raw('last_xy without last_status', lst_=None)
    raw('last_status without last_xy', lxy_=None)
    raw('n = 0', n=0)
    raw('n = 0, null arrays', n=0, probs=None, xy_=None, res_=None, lxy_=None, lst_=None)
    raw('wvl_idx 7', probs=with_fields(aim, wvl_idx=7))
    raw('wvl_idx -1', probs=with_fields(aim, wvl_idx=-1))
    raw('surf N', probs=with_fields(aim, surf=N))
    raw('surf -1', probs=with_fields(aim, surf=-1))
    raw('two_d, epsfcn < 0', probs=with_fields(aim, two_d=1, epsfcn=-1.0))
    raw('two_d, epsfcn nan', probs=with_fields(aim, two_d=1, epsfcn=float('nan')))
    call('aim_chief_rays: null probs', lib.rox_aim_chief_rays(h, 1, null, 1e-12, ptr(xy), ptr(res), null))
    call('aim_chief_rays: null system', lib.rox_aim_chief_rays(null, 1, C.byref(aim), 1e-12, ptr(xy), ptr(res), null))
    call('aim_chief_rays: wvl_idx 7', lib.rox_aim_chief_rays(h, 1, C.byref(with_fields(aim, wvl_idx=7)), 1e-12,
                                                             ptr(xy), ptr(res), null))
    call('aim_chief_rays: n = 0', lib.rox_aim_chief_rays(h, 0, null, 1e-12, null, null, null))

    enp = abi.Enp()
    enp.dir0[2] = 1.0
    enp.rot[0] = enp.rot[4] = enp.rot[8] = 1.0
    enp.obj_dist, enp.z_enp_0, enp.surf = 100.0, 1.0, 1

    def find_enp(name, sys_=h, n=1, probs=enp, z=xy, res_=res):
        call('find_real_enp: ' + name, lib.rox_find_real_enp(
            sys_, n, C.byref(probs) if probs is not None else null, 1e-12,
            ptr(z) if z is not None else null, ptr(res_) if res_ is not None else null, null))

    find_enp('null system', sys_=null)
    find_enp('n < 0', n=-1)
    find_enp('null probs', probs=None)
    find_enp('null z_out', z=None)
    find_enp('null result', res_=None)
    find_enp('n = 0', n=0)
    find_enp('wvl_idx 1', probs=with_fields(enp, wvl_idx=1))
    find_enp('surf N', probs=with_fields(enp, surf=N))
    find_enp('surf -1', probs=with_fields(enp, surf=-1))

    it = abi.PupilIter()
    it.fld = fld
    it.start_r0, it.r_target, it.xy, it.indx = 1.0, 1.0, 1, 1
    sr = np.zeros(1)

    def pupil_iter(name, sys_=h, n=1, probs=it, out=sr):
        call('iterate_pupil_rays: ' + name, lib.rox_iterate_pupil_rays(
            sys_, n, C.byref(probs) if probs is not None else null, 1e-12,
            ptr(out) if out is not None else null, null))

    def bad_kind(proto):
        p = with_fields(proto)
        p.fld.kind = 99
        return p

    pupil_iter('null system', sys_=null)
    pupil_iter('n < 0', n=-1)
    pupil_iter('null probs', probs=None)
    pupil_iter('null start_r', out=None)
    pupil_iter('n = 0', n=0)
    pupil_iter('wvl_idx 1', probs=with_fields(it, wvl_idx=1))
    pupil_iter('indx N', probs=with_fields(it, indx=N))
    pupil_iter('indx -1', probs=with_fields(it, indx=-1))
    pupil_iter('xy 2', probs=with_fields(it, xy=2))
    pupil_iter('fld.kind 99', probs=bad_kind(it))

    vg = abi.Vig()
    vg.fld = fld
    vg.unit_dir[1], vg.xy, vg.stop_surf, vg.max_iter = 1.0, 1, 1, 10
    clip = np.zeros(1, np.int32)

    def vig(name, sys_=h, n=1, probs=vg, v=sr, c=clip):
        call('calc_vignetting: ' + name, lib.rox_calc_vignetting(
            sys_, n, C.byref(probs) if probs is not None else null, 1e-12,
            ptr(v) if v is not None else null, ptr(c) if c is not None else null, null))

    vig('null system', sys_=null)
    vig('n < 0', n=-1)
    vig('null probs', probs=None)
    vig('null vig', v=None)
    vig('null clip_surf', c=None)
    vig('n = 0', n=0)
    vig('wvl_idx -1', probs=with_fields(vg, wvl_idx=-1))
    vig('stop_surf N', probs=with_fields(vg, stop_surf=N))
    vig('xy -1', probs=with_fields(vg, xy=-1))
    vig('max_iter < 0', probs=with_fields(vg, max_iter=-1))
    vig('fld.kind 99', probs=bad_kind(vg))

    # ---- the three trace entries, with ROX_HOST_POINTERS and without
    grid = make_grid((-1., -1.), (1., 1.), 2)                  # 4 rays
    nseg = C.c_int32()
    assert lib.rox_system_num_segments(h, 0, C.byref(nseg)) == 0
    seg = np.zeros((nseg.value, abi.SEG_DOUBLES, 4))
    op, st, fs = np.zeros(4), np.zeros(4, np.uint8), np.zeros(4, np.int16)
    hits = np.zeros(1, np.int64)
    pt0 = np.zeros((3, 4))
    dir0 = np.zeros((3, 4))
    py = np.array([-2.0, 0.0, 1.0, 3.0])
    pt0[1] = 5.0
    d = np.stack([np.zeros(4), py - 5.0, np.full(4, 100.0)])
    dir0[:] = d / np.sqrt((d * d).sum(axis=0))
    px = np.zeros(4)
    wv = np.zeros(4, np.int32)

    def out_of(ld=4, seg_=seg, n_hits=None):
        o = abi.Out()
        o.seg, o.op, o.status, o.fail_surf, o.ld = (ptr(seg_) if seg_ is not None else None), ptr(op), ptr(st), ptr(fs), ld
        o.n_hits = ptr(n_hits) if n_hits is not None else None
        return o

    def opts_of(flags, out_mode=abi.OUT_FULL, **kw):
        return make_opts(flags=abi.INTERSECT_OBJ | abi.CHECK_APERTURES | flags, out_mode=out_mode,
                         first_surf=1, last_surf=N - 2, **kw)

    def ref(x):
        return C.byref(x) if x is not None else null

    for hp in (abi.HOST_POINTERS, 0):
        tag = ' [host pointers]' if hp else ' [device pointers]'
        o, out = opts_of(hp), out_of()

        def rays(name, sys_=h, n=4, p=pt0, d_=dir0, w=None, wall=0, o_=o, out_=out):
            call('trace_rays: ' + name + tag, lib.rox_trace_rays(
                sys_, n, ptr(p) if p is not None else null, ptr(d_) if d_ is not None else null,
                ptr(w) if w is not None else null, wall, ref(o_), ref(out_), null))

        rays('null system', sys_=null)
        rays('null opts', o_=None)
        rays('null out', out_=None)
        rays('out_mode 9', o_=opts_of(hp, out_mode=9))
        rays('out_mode -1', o_=opts_of(hp, out_mode=-1))
        rays('OPD without wf', o_=opts_of(hp, out_mode=abi.OUT_OPD))
        rays('HITS_COMPACT without n_hits', o_=opts_of(hp, out_mode=abi.OUT_HITS_COMPACT))
        rays('HITS_COMPACT', o_=opts_of(hp, out_mode=abi.OUT_HITS_COMPACT), out_=out_of(ld=2, n_hits=hits))
        rays('HITS_APPEND with OUT_HITS', o_=opts_of(hp | abi.HITS_APPEND, out_mode=abi.OUT_HITS))
        rays('out.ld < n_rays', out_=out_of(ld=3))
        rays('null out.seg', out_=out_of(seg_=None))
        rays('null pt0', p=None)
        rays('null dir0', d_=None)
        rays('n < 0', n=-4)
        rays('wvl_idx_all 1', wall=1)
        rays('wvl_idx_all -1', wall=-1)
        rays('n = 0', n=0, p=None, d_=None)
        if hp:
            rays('wvl_idx[2] = 3 in a host list', w=np.array([0, 0, 3, 0], np.int32))
            rays('wvl_idx[0] = -1 in a host list', w=np.array([-1, 0, 0, 0], np.int32))

        def pgrid(name, sys_=h, f=fld, g=grid, w=0, o_=o, out_=out):
            call('trace_pupil_grid: ' + name + tag, lib.rox_trace_pupil_grid(
                sys_, ref(f), ref(g), w, ref(o_), ref(out_), null))

        pgrid('null system', sys_=null)
        pgrid('null fld', f=None)
        pgrid('null grid', g=None)
        pgrid('null opts', o_=None)
        pgrid('null out', out_=None)
        pgrid('fld.kind 99', f=bad_kind(it).fld)
        pgrid('grid.num 0', g=make_grid((-1., -1.), (1., 1.), 0))
        pgrid('wvl_idx 1', w=1)
        pgrid('row block outside', g=make_grid((-1., -1.), (1., 1.), 2, row_begin=1, row_count=2))
        pgrid('out.ld < rays', out_=out_of(ld=3))
        pgrid('out_mode 9', o_=opts_of(hp, out_mode=9))
        pgrid('null out.seg', out_=out_of(seg_=None))

        def plist(name, sys_=h, f=fld, n=4, x=px, y=py, w=0, o_=o, out_=out):
            call('trace_pupil_list: ' + name + tag, lib.rox_trace_pupil_list(
                sys_, ref(f), n, ptr(x) if x is not None else null, ptr(y) if y is not None else null,
                w, ref(o_), ref(out_), null))

        plist('null system', sys_=null)
        plist('null opts', o_=None)
        plist('null fld', f=None)
        plist('fld.kind -1', f=with_fields(fld, kind=-1))
        plist('null px', x=None)
        plist('null py', y=None)
        plist('n < 0', n=-1)
        plist('wvl_idx 1', w=1)
        plist('out.ld < n_rays', out_=out_of(ld=1))
        plist('n = 0', n=0, x=None, y=None)

    # ---- rox_trace_pupil_grids and rox_time_pupil_grid
    o, out = opts_of(0), out_of()

    def grids(name, sys_=h, n=2, flds=(fld, fld), wvls=(0, 0), g=grid, os_=(o, o), outs=(out, out)):
        call('trace_pupil_grids: ' + name, lib.rox_trace_pupil_grids(
            sys_, n, (abi.Field * 2)(*flds) if flds else null, (C.c_int32 * 2)(*wvls) if wvls else null,
            ref(g), (abi.Opts * 2)(*os_) if os_ else null, (abi.Out * 2)(*outs) if outs else null, null))

    grids('null system', sys_=null)
    grids('n < 0', n=-1)
    grids('null flds', flds=None)
    grids('null wvl_idx', wvls=None)
    grids('null opts', os_=None)
    grids('null outs', outs=None)
    grids('n = 0', n=0)
    grids('ROX_HOST_POINTERS in item 1', os_=(o, opts_of(abi.HOST_POINTERS)))
    grids('ROX_HITS_APPEND in item 0', os_=(opts_of(abi.HITS_APPEND), o))
    grids('out_mode differs in item 1', os_=(o, opts_of(0, out_mode=abi.OUT_HITS)))
    grids('ROX_FILTER_PHANTOMS differs in item 1', os_=(o, opts_of(abi.FILTER_PHANTOMS)))
    grids('null grid', g=None)
    grids('wvl_idx 1 in item 0', wvls=(1, 0))
    grids('fld.kind 99 in item 0', flds=(bad_kind(it).fld, fld))
    grids('out.ld < rays in item 0', outs=(out_of(ld=3), out))

    ms = C.c_double()

    def timed(name, sys_=h, f=fld, g=grid, w=0, o_=o, out_=out, launches=1, ms_=ms):
        call('time_pupil_grid: ' + name, lib.rox_time_pupil_grid(
            sys_, ref(f), ref(g), w, ref(o_), ref(out_), null, launches, ref(ms_)))

    timed('null system', sys_=null)
    timed('null mean_ms', ms_=None)
    timed('launches 0', launches=0)
    timed('ROX_HOST_POINTERS', o_=opts_of(abi.HOST_POINTERS))
    timed('null fld', f=None)
    timed('null grid', g=None)
    timed('null opts', o_=None)
    timed('null out', out_=None)
    timed('wvl_idx -1', w=-1)
    timed('grid.num 0', g=make_grid((-1., -1.), (1., 1.), 0))
    timed('out.ld < rays', out_=out_of(ld=3))

    # ---- valid calls: the bytes of their results
    # (a chief ray aimed off the axis of the stop, so that no answer is zero; every output buffer
    # starts as 0x55 bytes, and those the call is not given must stay so)
    valid = {}
    off_axis = with_fields(aim, y_target=0.75)
    for a in (xy, res, lxy, lst):
        a.view(np.uint8)[...] = 0x55
    raw('valid, with last_xy', probs=off_axis)
    valid['iterate_ray_raw with last_xy'] = b''.join(a.tobytes() for a in (xy, res, lxy, lst)).hex()
    for a in (xy, res, lxy, lst):
        a.view(np.uint8)[...] = 0x55
    raw('valid, without last_xy', probs=off_axis, lxy_=None, lst_=None)
    valid['iterate_ray_raw without last_xy'] = b''.join(a.tobytes() for a in (xy, res, lxy, lst)).hex()
    call('trace_rays: valid, staged, per-ray wavelengths', lib.rox_trace_rays(
        h, 4, ptr(pt0), ptr(dir0), ptr(wv), 0, C.byref(opts_of(abi.HOST_POINTERS)), C.byref(out_of()), null))
    valid['staged trace_rays'] = b''.join(a.tobytes() for a in (seg, op, st, fs)).hex()
    eng.close()
    return {'calls': calls, 'valid': valid}


@pytest.mark.gpu
def test_host_entries_answer_bad_and_valid_calls_as_recorded():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = collect()
    assert len(want['calls']) > 150 and sum(rc != 0 for _n, rc, _t in want['calls']) > 140
    assert [c[0] for c in got['calls']] == [c[0] for c in want['calls']]
    differ = [(g, w) for g, w in zip(got['calls'], want['calls']) if g != w]
    assert not differ, differ
    assert all(rc == 0 for name, rc, _t in got['calls'] if 'valid' in name or 'n = 0' in name)
    assert got['valid'] == want['valid']
    # what was recorded: aim_xy[2], result, last_xy[2], last_status = 16 + 4 + 16 + 4 bytes.  With
    # last_xy nothing is left of the 0x55 fill and the y coordinates are not zero; without, the
    # first two are the same and the last two are still the fill
    with_last, without = (np.frombuffer(bytes.fromhex(want['valid']['iterate_ray_raw ' + k]), np.uint8)
                          for k in ('with last_xy', 'without last_xy'))
    assert len(with_last) == len(without) == 40
    for lo, hi in ((0, 8), (8, 16), (16, 20), (20, 28), (28, 36), (36, 40)):
        assert not (with_last[lo:hi] == 0x55).all(), (lo, hi)
    assert with_last[8:16].any() and with_last[28:36].any()
    assert np.array_equal(without[:20], with_last[:20]) and (without[20:] == 0x55).all()


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    with open(sys.argv[1], 'w') as f:
        json.dump(collect(), f, indent=1)
        f.write('\n')
