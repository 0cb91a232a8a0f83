"""The argument checks of the two packet entries, rox_surface_footprints and
rox_surface_transmission, answer what tests/golden/packet_entry_errors.json records: every return
code and the whole rox_last_error() text, in order, compared for equality.

The cases: the 19 of test_transmission_host.c_error_cases() (through its call_tx: addresses the
entry never reads), the 15 of test_gpu_beam_footprints.test_argument_errors, three of
rox_surface_transmission that need the system (wvl_idx >= the number of wavelengths, n_coat != the
number of interfaces, a valid call) and a valid call of rox_surface_footprints -- these on the
dblgauss grid_f0 golden packet as 2 items, R as stored, n_bins = 4.  A case that fails before the
system is read runs without a device too, with addresses in place of the system and the packets.

The fixture was recorded from the library as it was before the two entries shared
csrc/rox_packets.hpp, on a GPU, with this file's collect():

    ROX_LIB=<library> python tests/test_packet_entry_errors.py <fixture.json>"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'packet_entry_errors.json')
N_BINS = 4


class Packets:
    """the arguments of both entries over the golden packet as 2 items: with an engine the system and
    the packets in HBM, without one addresses no case that fails its checks first ever reads"""

    def __init__(self, eng=None):
        from helpers import fixture
        from rayoptics_amd import abi
        from rayoptics_amd.engine import FOOTPRINT_DTYPE, TX_ITEM_DTYPE, TX_SURFACE_DTYPE
        fx = fixture('dblgauss')
        c = fx['grid_f0']
        n_seg, _ten, self.R = c['seg'].shape
        self.N, self.n_wvls, self.flags = fx.table.n_ifcs, len(fx.table.wvls), int(c['flags'])
        self.sys, self.out = 8, abi.Out(seg=8, status=8, fail_surf=8, ld=self.R)
        if eng is not None:
            from packets_fixture import upload
            assert eng.num_segments(self.flags) == n_seg
            self.res = upload(eng, c['seg'], c['status'], c['fail_surf'])
            self.sys, self.out = eng._handle, self.res.out_struct()
        self.fp = np.zeros((2, n_seg), FOOTPRINT_DTYPE)
        self.maps = np.zeros((2, n_seg, N_BINS, N_BINS), np.uint32)
        self.hw = np.full(n_seg, 20.0)
        self.rows = np.zeros((2, 4, self.R))
        self.surf = np.zeros((2, n_seg), TX_SURFACE_DTYPE)
        self.item = np.zeros(2, TX_ITEM_DTYPE)

    def outs(self, item1):
        """(abi.Out * 2): the packet twice, ``item1`` replacing fields of the second"""
        from rayoptics_amd import abi
        o = abi.Out.from_buffer_copy(bytes(self.out))
        for field, value in item1.items():
            setattr(o, field, value)
        return (abi.Out * 2)(self.out, o)

    def footprints(self, lib, n_items=1, n_rays=None, flags=1, item1={}, fp=True, hw='good', n_bins=N_BINS, maps=True):
        hw = self.hw if isinstance(hw, str) else hw
        return lib.rox_surface_footprints(self.sys, self.flags, flags, n_items, self.outs(item1),
                                          self.R if n_rays is None else n_rays, self.fp.ctypes.data if fp else None,
                                          hw.ctypes.data if hw is not None else None, n_bins,
                                          self.maps.ctypes.data if maps else None, None)

    def transmission(self, lib, wvl=(0, 1), n_coat=0):
        w = np.array(wvl, np.int32)
        kind, value = np.zeros(self.N, np.int32), np.ones((self.N, 2))
        return lib.rox_surface_transmission(self.sys, self.flags, 0, 2, self.outs({}), self.R, w.ctypes.data, n_coat,
                                            kind.ctypes.data if n_coat else None,
                                            value.ctypes.data if n_coat else None, self.rows.ctypes.data, self.R,
                                            self.surf.ctypes.data, self.item.ctypes.data, None)


def cases(p):
    """[(name, call(lib) -> rc, whether it reads the system)] in the fixture's order"""
    from rayoptics_amd import abi
    from test_transmission_host import c_error_cases, call_tx
    out = [('transmission: ' + name, lambda lib, over=over: call_tx(lib, dict(over)), False)
           for name, over, _word in c_error_cases()]
    out += [('transmission: ' + name, lambda lib, kw=kw: p.transmission(lib, **kw), True) for name, kw in (
        ('wvl_idx = the number of wavelengths', dict(wvl=(0, p.n_wvls))),
        ('n_coat one short of the interfaces', dict(n_coat=p.N - 1)),
        ('valid', dict()))]
    R = p.R
    nan_hw, neg_hw = p.hw.copy(), p.hw.copy()
    nan_hw[3], neg_hw[2] = np.nan, -1.0
    out += [('footprints: ' + name, lambda lib, kw=kw: p.footprints(lib, **kw), needs) for name, kw, needs in (
        ('n_items 0', dict(n_items=0), False),
        ('n_items over', dict(n_items=abi.MAX_FOCUS_ITEMS + 1), False),
        ('null seg', dict(item1=dict(seg=None), n_items=2), False),
        ('null status', dict(item1=dict(status=None), n_items=2), False),
        ('null fail_surf', dict(item1=dict(fail_surf=None), n_items=2), False),
        ('ld < n_rays', dict(item1=dict(ld=R - 1), n_items=2), False),
        ('n_rays 0', dict(n_rays=0), False),
        ('n_rays over', dict(n_rays=(1 << 28) + 1), False),
        ('maps without half_width', dict(hw=None), True),
        ('n_bins 0', dict(n_bins=0), True),
        ('n_bins 513', dict(n_bins=513), True),
        ('half_width nan', dict(hw=nan_hw), True),
        ('half_width negative', dict(hw=neg_hw), True),
        ('unknown flag', dict(flags=4), False),
        ('null fp and maps', dict(fp=False, maps=False), False),
        ('valid', dict(n_items=2), True))]
    return out


def replay(lib, p, with_system):
    """[[name, rc, text or None when rc == 0], ...] of every case, or of those that do not read the system"""
    calls = []
    for name, call, needs_system in cases(p):
        if with_system or not needs_system:
            rc = int(call(lib))
            calls.append([name, rc, lib.rox_last_error().decode() if rc != 0 else None])
    return calls


def collect():
    from rayoptics_amd.engine import TraceEngine, load_library
    from helpers import fixture
    eng = TraceEngine(fixture('dblgauss').table)
    calls = replay(load_library(), Packets(eng), True)
    eng.close()
    return {'calls': calls}


def recorded():
    with open(FIXTURE) as f:
        want = json.load(f)['calls']
    assert len(want) == 38 and sum(rc == -1 for _n, rc, _t in want) == 36 and sum(rc == 0 for _n, rc, _t in want) == 2
    assert all((text is None) == (rc == 0) for _n, rc, text in want)
    return want


def test_checks_before_the_system_answer_as_recorded_without_a_device():
    import ctypes as C
    import importlib.util
    from rayoptics_amd import abi
    spec = importlib.util.spec_from_file_location('rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    got = replay(abi.declare(C.CDLL(b.build())), Packets(), False)
    names = {c[0] for c in got}
    assert len(got) == 29 and all(rc == -1 for _n, rc, _t in got)
    assert got == [c for c in recorded() if c[0] in names]


@pytest.mark.gpu
def test_every_check_answers_as_recorded():
    got = collect()['calls']
    want = recorded()
    differ = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not differ, differ


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    with open(sys.argv[1], 'w') as f:
        json.dump(collect(), f, indent=1)
        f.write('\n')
