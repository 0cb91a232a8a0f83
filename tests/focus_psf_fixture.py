"""TEST INFRASTRUCTURE for the diffraction through-focus tests: a model over one field of
tests/golden/through_focus_psf.npz (tests/golden/make_through_focus_psf.py).  As
focus_fixture.FocusFixtureModel it hands out the reference's own reference sphere per focus
shift; it also carries the reference's paraxial enp_radius / exp_radius and each focus's
reference-sphere radius, so calc_psf_scaling can be formed as the reference forms it."""
import os
from types import SimpleNamespace

import numpy as np

from focus_fixture import FocusFixtureModel

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'through_focus_psf.npz')
FIELDS = ('f0', 'f1')           # on axis, full field


def load():
    return np.load(PATH)


class FocusPsfFixtureModel(FocusFixtureModel):
    def __getitem__(self, key):
        if key == 'analysis_results':
            fod = SimpleNamespace(enp_radius=float(self.z['enp_radius']), exp_radius=float(self.z['exp_radius']))
            return {'parax_data': SimpleNamespace(fod=fod)}
        return super().__getitem__(key)

    def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
        (ip, _a, _b, _c), cr = super().setup_pupil_coords(fld, wvl, foc, image_pt, image_delta)
        k = self.focs.index(float(foc))
        return (ip, None, float(self.z['ref_radius'][k]), None), cr
