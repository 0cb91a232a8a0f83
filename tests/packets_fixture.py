"""TEST INFRASTRUCTURE for the -m gpu tests of the entries that walk the ROX_OUT_FULL packets of
finished launches (rox_surface_footprints, rox_surface_transmission, rox_surface_thinfilm,
rox_projected_solid_angle, rox_segment_foci, rox_weighted_maps): the ``torch`` fixture, host
packets put into HBM, packets traced there and packets copied back."""
import numpy as np
import pytest

from rayoptics_amd import abi


@pytest.fixture(scope='module')
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch


def upload(eng, seg, status, fail_surf):
    """host packets -> a DeviceResult-shaped FULL buffer (NaN where no record was written)"""
    from rayoptics_amd.engine import DeviceResult
    t = eng.torch
    n_seg, _ten, R = seg.shape
    res = DeviceResult(t, eng.device, n_seg, R, abi.OUT_FULL, False, True)
    res.seg.copy_(t.from_numpy(np.ascontiguousarray(seg)))
    res.status.copy_(t.from_numpy(np.ascontiguousarray(status, dtype=np.uint8)))
    res.fail_surf.copy_(t.from_numpy(np.ascontiguousarray(fail_surf, dtype=np.int16)))
    return res


def trace_packets(eng, flags, flds, wis, num, span=1.0):
    """one FULL launch of num x num rays over [-span, span]^2 of the pupil for every (flds[i], wis[i]),
    all traced with ``flags``; the packets stay in HBM"""
    from rayoptics_amd.engine import make_grid, make_opts
    opts = [make_opts(flags=flags, out_mode=abi.OUT_FULL) for _ in flds]
    return eng.trace_pupil_grids(flds, wis, make_grid((-span, -span), (span, span), num), opts, want_pupil=False)


def host_of(results, want):
    """[the arrays named in ``want`` of every result, copied to the host]"""
    out = []
    for r in results:
        h = r.to_host(want=want)
        out.append(tuple(np.array(getattr(h, name)) for name in want))
    return out
