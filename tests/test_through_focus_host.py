"""CPU-side checks of the through-focus entry (rox_trace_through_focus,
analyses.through_focus): struct layouts against the header, argument errors without a device,
the best-focus rule on synthetic curves, and -- with the reference installed -- the drop-in's
planes and rows against the reference's own focus_wavefront / focus_fan (an engine double serves
the new entry as K oracle FAN launches)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rayoptics_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


def test_focus_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of rox_focus_plane and rox_focus_stats under gcc == the ctypes mirror"""
    structs = {'rox_focus_plane': abi.FocusPlane, 'rox_focus_stats': abi.FocusStats}
    lines = ['#include <stdio.h>', '#include <stddef.h>',
             f'#include "{ROOT}/include/roxtrace.h"', 'int main(void) {',
             'printf("max %d\\n", ROX_MAX_FOCUS_PLANES);']
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _t in st._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-o', str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got['max']) == abi.MAX_FOCUS_PLANES >= 256
    for cname, st in structs.items():
        assert int(got[cname]) == C.sizeof(st), cname
        for fname, _t in st._fields_:
            assert int(got[f'{cname}.{fname}']) == getattr(st, fname).offset, f'{cname}.{fname}'


def _args(n_planes=2, ld=64, rows=True, stats=True, out_mode=abi.OUT_FAN, planes=True, flags=0):
    from rayoptics_amd.engine import make_grid, make_opts
    from rayoptics_amd.table import field_struct
    fld = field_struct([0.0, 0.0, 0.0], (0., 0.), 1.0, 10.0)
    grid = make_grid((-1., -1.), (1., 1.), 8)             # 64 rays
    opts = make_opts(flags=flags, out_mode=out_mode, first_surf=1, last_surf=2)
    p = (abi.FocusPlane * max(n_planes, 1))()
    for q in p:
        q.wf.ref_radius = 100.0
    buf = np.zeros(3 * 64 * max(n_planes, 1))
    st = (abi.FocusStats * max(n_planes, 1))()
    return (None, C.byref(fld), C.byref(grid), 0, C.byref(opts), n_planes, p if planes else None,
            buf.ctypes.data if rows else None, ld, None, st if stats else None, None), buf


@pytest.mark.parametrize('kw,msg', [
    (dict(n_planes=0), b'n_planes'),
    (dict(n_planes=abi.MAX_FOCUS_PLANES + 1), b'n_planes'),
    (dict(planes=False), b'planes is null'),
    (dict(ld=63), b'ld (63) < rays (64)'),
    (dict(rows=False, stats=False), b'both null'),
    (dict(out_mode=abi.OUT_OPD), b'ROX_OUT_FAN'),
    (dict(flags=abi.HOST_POINTERS), b'device pointers only'),
])
def test_argument_errors_without_a_device(lib, kw, msg):
    """every argument error returns ROX_E_ARG with its message before a device is touched (no
    system exists here: the checks come before the handle is looked at)"""
    args, _buf = _args(**kw)
    assert lib.rox_trace_through_focus(*args) == -1
    assert msg in lib.rox_last_error(), lib.rox_last_error()


def test_a_bad_plane_wavefront_is_an_argument_error(lib):
    args, _buf = _args()
    args[6][1].wf.ref_radius = 0.0
    assert lib.rox_trace_through_focus(*args) == -1
    assert b'plane 1' in lib.rox_last_error()
    args, _buf = _args()
    args[6][0].wf.kind = 7
    assert lib.rox_trace_through_focus(*args) == -1
    assert b'plane 0' in lib.rox_last_error()
    args, _buf = _args()                     # valid arguments, no system: still no device
    assert lib.rox_trace_through_focus(*args) == -1
    assert b'null system' in lib.rox_last_error()


def test_best_focus_rule():
    from rayoptics_amd.analyses import best_focus
    x = np.linspace(-0.2, 0.3, 11)
    f, kind = best_focus(x, 3.0 * (x - 0.071) ** 2 + 0.5)      # interior minimum: exact vertex
    assert kind == 'vertex' and abs(f - 0.071) < 1e-12
    f, kind = best_focus(x, np.abs(x - 0.071))                  # not a parabola: between neighbours
    i = int(np.argmin(np.abs(x - 0.071)))
    assert kind == 'vertex' and x[i - 1] <= f <= x[i + 1]
    assert best_focus(x, x) == (x[0], 'end')                     # minimum at an end
    assert best_focus(x, -x) == (x[-1], 'end')
    assert best_focus(x, np.ones_like(x)) == (x[0], 'end')       # a flat curve: the first sample
    v = np.ones_like(x)
    v[4:7] = 0.5                          # flat bottom: the first minimum and its neighbours
    f, kind = best_focus(x, v)
    assert kind == 'vertex' and x[3] <= f <= x[5]
    v = (x - 0.05) ** 2
    v[0] = np.nan                                                # planes no ray reached are skipped
    assert best_focus(x, v)[1] == 'vertex'
    f, kind = best_focus(x, np.full_like(x, np.nan))
    assert kind == 'none' and np.isnan(f)
