"""TEST INFRASTRUCTURE for the through-focus tests: a workloads.TableModel over one model of
tests/golden/through_focus.npz (tests/golden/make_through_focus.py), whose setup_pupil_coords
hands out, per focus shift, the reference's own reference sphere at that focus -- as the
reference's trace.setup_pupil_coords (trace.py:608-624) does for a live model."""
import json
import os

import numpy as np

from rayoptics_amd import SurfaceTable, abi, workloads
from rayoptics_amd.table import wavefront_from_array

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'through_focus.npz')
MODELS = ('dblgauss', 'zmx_evenasph_c3')


def load():
    return np.load(PATH)


class FocusFixtureModel(workloads.TableModel):
    def __init__(self, z, name):
        self.name = name
        self.z = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        d = self.z
        tbl = SurfaceTable.from_dict(json.loads(str(d['table_json'])))
        wi = int(d['wvl_idx'])
        fld = abi.Field.from_buffer_copy(d['field'].tobytes())
        super().__init__(workloads.SimpleWorkload(tbl, [fld], [tuple(d['image_pt'][0])], ref_wvl_idx=wi))
        self.wvl = float(d['wvl'])
        self._units_per_nm = 1.0 / (float(d['convert_to_opd']) * self.wvl)
        self.fields[0]._vig_bbox = (d['bbox'][0], d['bbox'][1])
        self.focs = [float(f) for f in d['focs']]

    def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
        k = self.focs.index(float(foc))
        fld.rox_wavefront = wavefront_from_array(self.z['wavefront'][k])
        ip = self.z['image_pt'][k]
        return (np.array([ip[0], ip[1], 0.0]), None, None, None), None


def focus_wavefront_rows(z_grid):
    """the reference's focus_wavefront grid [num][num][3] -> OPD per ray in ray order (waves)"""
    return np.asarray(z_grid)[:, :, 2].reshape(-1)


def focus_fan_rows(z_fan):
    """the reference's focus_fan rows [num][5] (px, py, dx, dy, opd) -> [3][num]"""
    return np.asarray(z_fan)[:, 2:5].T
