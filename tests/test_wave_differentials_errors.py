"""Every ROX_E_ARG case of rox_wave_differentials names its parameter (and item) before anything is
enqueued and leaves the outputs untouched; reached through ctypes as tests/test_gpu_ghost.py
reaches rox_segment_foci."""
import ctypes as C

import numpy as np
import pytest

from packets_fixture import torch, upload  # noqa: F401 (torch: the fixture)
from rayoptics_amd import SurfaceTable, abi

pytestmark = pytest.mark.gpu

FILL = -7.25


def test_argument_errors(torch):
    from rayoptics_amd.engine import TraceEngine
    surfs = [dict(cv=0, thi=10.0)] + [dict(cv=0.01 * k, thi=3.0, n=1.5 if k % 2 else 1.0) for k in (1, 2)]
    eng = TraceEngine(SurfaceTable.from_prescription(surfs + [dict(cv=0, thi=0)]))
    lib, sys = eng.lib, eng._handle
    n_seg, R, n_aux = 4, 65, 2
    rng = np.random.default_rng(1)
    seg = rng.normal(size=(n_seg, 10, R))
    res = [upload(eng, seg, np.zeros(R, np.uint8), np.zeros(R, np.int16)) for _ in range(2)]
    aux = torch.zeros((2, n_aux, R), dtype=torch.float64, device=eng.device)
    n_cols = n_aux + 11 * n_seg
    cols = torch.full((2, n_cols, R), FILL, dtype=torch.float64, device=eng.device)
    item = np.full((2, 3), -7, np.int64)
    pivot, sums = np.full((2, n_cols), FILL), np.full((2, n_cols), FILL)
    gram = np.full((2, n_cols, n_cols), FILL)

    def call(**kw):
        a = dict(sys=sys, n_items=2, outs=True, n_rays=R, wvl=[0, 0], n_sel=n_seg, sel=None, n_aux=n_aux,
                 aux=aux.data_ptr(), aux_stride=n_aux * R, ld_aux=R, cols=cols.data_ptr(), ld_cols=R,
                 item=item.ctypes.data, pivot=pivot.ctypes.data, sums=sums.ctypes.data, gram=gram.ctypes.data,
                 ld=None, null_seg=False)
        a.update(kw)
        outs = (abi.Out * 2)(*[r.out_struct() for r in res])
        if a['ld'] is not None:
            outs[1].ld = a['ld']
        if a['null_seg']:
            outs[1].seg = None
        wvl = np.asarray(a['wvl'], np.int32) if a['wvl'] is not None else None
        sel = np.asarray(a['sel'], np.int32) if a['sel'] is not None else None
        rc = lib.rox_wave_differentials(a['sys'], abi.INTERSECT_OBJ, a['n_items'], outs if a['outs'] else None,
                                        a['n_rays'], wvl.ctypes.data if wvl is not None else None, a['n_sel'],
                                        sel.ctypes.data if sel is not None else None, a['n_aux'], a['aux'],
                                        a['aux_stride'], a['ld_aux'], a['cols'], a['ld_cols'], a['item'], a['pivot'],
                                        a['sums'], a['gram'], None)
        return rc, lib.rox_last_error().decode()

    cases = [(dict(sys=None), 'sys'), (dict(outs=False), 'outs'), (dict(wvl=None), 'wvl_idx'),
             (dict(n_items=0), 'n_items'), (dict(n_items=abi.MAX_FOCUS_ITEMS + 1), 'n_items'),
             (dict(n_rays=0), 'n_rays'), (dict(n_rays=(1 << 28) + 1), 'n_rays'),
             (dict(ld=R - 1), 'item 1: ld'), (dict(null_seg=True), 'item 1: null seg'),
             (dict(sel=[0, 4], n_sel=2), 'sel_slot[1]'), (dict(sel=[-1, 2], n_sel=2), 'sel_slot[0]'),
             (dict(sel=[2, 2], n_sel=2), 'sel_slot[1]'), (dict(sel=[2, 1], n_sel=2), 'sel_slot[1]'),
             (dict(n_sel=n_seg - 1), 'n_sel'), (dict(sel=[0], n_sel=n_seg + 1), 'n_sel'),
             (dict(n_aux=-1), 'n_aux'), (dict(n_aux=abi.MAX_WD_AUX + 1), 'n_aux'),
             (dict(aux=None), 'aux'), (dict(ld_aux=R - 1), 'ld_aux'), (dict(ld_cols=R - 1), 'ld_cols'),
             (dict(wvl=[0, 1]), 'item 1: wvl_idx'), (dict(wvl=[-1, 0]), 'item 0: wvl_idx'),
             (dict(cols=None, item=None, pivot=None, sums=None, gram=None), 'null cols, item and gram'),
             (dict(item=None), 'gram'), (dict(pivot=None), 'gram'), (dict(sums=None), 'gram'),
             (dict(gram=None, item=None), 'item'), (dict(gram=None, pivot=None), 'pivot'),
             (dict(sel=[], n_sel=0, n_aux=0, aux=None), 'n_cols')]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and 'rox_wave_differentials' in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (cols == FILL).all().item() and (item == -7).all()
    for a in (pivot, sums, gram):
        assert (a == FILL).all()
    # and the same arguments untouched by a case above are a valid call
    rc, msg = call()
    assert rc == 0, msg
    assert (item[:, 0] == R).all() and not (gram == FILL).any()
    eng.close()


def test_more_than_512_columns(torch):
    """the library's own check of n_cols = n_aux + 11*n_sel (TraceEngine.wave_differentials refuses
    the same before it calls): the 44 slots of the lithography lens with 29 and with 32 aux rows"""
    from rayoptics_amd import workloads
    from rayoptics_amd.engine import TraceEngine
    eng = TraceEngine(workloads.load('litho_c5').table)
    n_seg, R = eng.num_segments(abi.INTERSECT_OBJ), 65
    assert n_seg == 44
    res = upload(eng, np.random.default_rng(2).normal(size=(n_seg, 10, R)), np.zeros(R, np.uint8), np.zeros(R, np.int16))
    outs = (abi.Out * 1)(res.out_struct())
    wvl = np.zeros(1, np.int32)
    for n_aux in (29, 32):
        n_cols = n_aux + 11 * n_seg
        aux = torch.zeros((1, n_aux, R), dtype=torch.float64, device=eng.device)
        cols = torch.full((1, n_cols, R), FILL, dtype=torch.float64, device=eng.device)
        item = np.full((1, 3), -7, np.int64)
        pivot, sums = np.full((1, n_cols), FILL), np.full((1, n_cols), FILL)
        gram = np.full((1, n_cols, n_cols), FILL)
        rc = eng.lib.rox_wave_differentials(eng._handle, abi.INTERSECT_OBJ, 1, outs, R, wvl.ctypes.data, n_seg, None,
                                            n_aux, aux.data_ptr(), n_aux * R, R, cols.data_ptr(), R,
                                            item.ctypes.data, pivot.ctypes.data, sums.ctypes.data, gram.ctypes.data,
                                            None)
        msg = eng.lib.rox_last_error().decode()
        assert rc == -1 and 'rox_wave_differentials' in msg and 'n_cols' in msg and str(n_cols) in msg, (rc, msg)
        torch.cuda.synchronize()
        assert (cols == FILL).all().item() and (item == -7).all()
        for a in (pivot, sums, gram):
            assert (a == FILL).all()
    eng.close()
