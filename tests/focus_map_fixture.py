"""TEST INFRASTRUCTURE for the through-focus map tests: a workloads.TableModel over one model of
tests/golden/through_focus_map.npz (tests/golden/make_through_focus_map.py) -- every field at
every wavelength -- whose setup_pupil_coords hands out, per (field, wavelength, focus shift), the
reference's own reference sphere there, as the reference's trace.setup_pupil_coords
(trace.py:608-624) does for a live model."""
import json
import os

import numpy as np

from rayoptics_amd import SurfaceTable, abi, workloads
from rayoptics_amd.table import wavefront_from_array

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'through_focus_map.npz')
MODELS = ('dblgauss', 'zmx_evenasph_c3')


def load():
    return np.load(PATH)


class FocusMapFixtureModel(workloads.TableModel):
    def __init__(self, z, name):
        self.name = name
        self.z = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        d = self.z
        tbl = SurfaceTable.from_dict(json.loads(str(d['table_json'])))
        self.wvls = [float(w) for w in d['wvls']]
        self.central_wvl = float(d['central_wvl'])
        ref = self.wvls.index(self.central_wvl)
        flds = [abi.Field.from_buffer_copy(b.tobytes()) for b in d['fields']]
        ipts = [tuple(d['image_pt'][f, ref, 0]) for f in range(len(flds))]
        super().__init__(workloads.SimpleWorkload(tbl, flds, ipts, ref_wvl_idx=ref),
                         sys_units_per_nm=float(d['units_per_nm']))
        for f, tf in enumerate(self.fields):
            tf._vig_bbox = (d['bbox'][f, 0], d['bbox'][f, 1])
        self.field_wts = [float(w) for w in d['field_wts']]
        self.spectral_wts = [float(w) for w in d['spectral_wts']]
        self.focs = [float(f) for f in d['focs']]
        self.ref_focs = [int(k) for k in d['ref_focs']]

    def map_kwargs(self):
        """what through_focus_map takes from osp on a live model"""
        return dict(flds=self.fields, wvls=self.wvls, field_wts=self.field_wts,
                    spectral_wts=self.spectral_wts, ref_wvl=self.central_wvl)

    def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
        f = self.fields.index(fld)
        w = self.wvls.index(float(wvl))
        k = self.focs.index(float(foc))
        fld.rox_wavefront = wavefront_from_array(self.z['wavefront'][f, w, k])
        ip = self.z['image_pt'][f, w, k]
        return (np.array([ip[0], ip[1], 0.0]), None, None, None), None
