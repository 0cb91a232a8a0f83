"""Every .zmx and .seq prescription in the reference tree, through rayoptics_amd.ingest and
through the reference's own importer (build container only): the surface tables are equal field
by field, or the file is on a short list with the reason.

Refractive indices are compared exactly except behind *model glasses* (Zemax ___BLANK records,
CODE V fictitious codes 'nnn.vvv'): their dispersion comes from opticalglass.modelglass, absent
here (oracle/refshim.py carries a synthetic stand-in) -- catalogue parity is unpinned
(DESIGN.md section 5); at the d line both sides hold nd."""
import glob
import os
import pathlib

import numpy as np
import pytest

from test_ingest_reference import REF, rows_equal

pytestmark = pytest.mark.needs_reference


def tree_files(*exts):
    """the files of the reference tree with these extensions, relative to REF"""
    return sorted(os.path.relpath(p, REF) for ext in exts
                  for p in glob.glob(os.path.join(REF, '**', f'*.{ext}'), recursive=True))


# the reference tree's prescription files, listed here rather than globbed at collection so that
# the test ids are the same whether or not the tree is present; test_file_lists_are_the_reference_tree
# keeps the lists complete
FILES = [
    'codev/tests/CODV_32327.seq',
    'codev/tests/CODV_35571.seq',
    'codev/tests/CODV_49664.seq',
    'codev/tests/CODV_65564.seq',
    'codev/tests/CODV_65988.seq',
    'codev/tests/CODV_65988_noDOE.seq',
    'codev/tests/achroMangin.seq',
    'codev/tests/achroMangin_ok.seq',
    'codev/tests/ag_dblgauss.seq',
    'codev/tests/asp46.seq',
    'codev/tests/dar_test.seq',
    'codev/tests/dec_rev_tilt_test.seq',
    'codev/tests/dec_test.seq',
    'codev/tests/dec_tilt_test.seq',
    'codev/tests/folded_lenses.seq',
    'codev/tests/landscape_lens.seq',
    'codev/tests/lens_reflection_test.seq',
    'codev/tests/mangin.seq',
    'codev/tests/paraboloid.seq',
    'codev/tests/paraboloid_f8.seq',
    'codev/tests/questar35.seq',
    'codev/tests/rc_f16.seq',
    'codev/tests/schmidt.seq',
    'codev/tests/schmidt_sph.seq',
    'codev/tests/singlet.seq',
    'codev/tests/test.seq',
    'codev/tests/threemir.seq',
    'codev/tests/tilt_test.seq',
    'codev/tests/unfolded_lenses_w_ape.seq',
    'elem/tests/ACL3026U-Zemax(ZMX).zmx',
    'zemax/models/PhotoPrime/US05331467-1.zmx',
    'zemax/tests/354710-C-Zemax(ZMX).zmx',
    'zemax/tests/ASL5040-UV-Zemax(ZMX).zmx',
    'zemax/tests/HoO-V2C18Ex03.zmx',
    'zemax/tests/HoO-V2C18Ex27.zmx',
    'zemax/tests/HoO-V2C18Ex46.zmx',
    'zemax/tests/HoO-V2C18Ex66.zmx',
    'zemax/tests/HoO-V2C18Ex66NEW.zmx',
    'zemax/tests/US00583336-2-scaled.zmx',
    'zemax/tests/US05831776-1.zmx',
    'zemax/tests/US08011793-1.zmx',
    'zemax/tests/zmax_37992.zmx',
    'zemax/tests/zmax_55278.zmx',
]
# a Q-type asphere: the reference's importer keeps the base conic and drops the Q terms
# (zmxread.py:295-333); the default ingest does the same, with a warning and a record
UNMODELLED = {'zemax/tests/ASL5040-UV-Zemax(ZMX).zmx': 'QED_TYPE'}
REFERENCE_FAILS = set()


def reference_table(path, kind):
    from oracle import refshim
    refshim.install()
    from rayoptics_amd import SurfaceTable
    from rayoptics.seq.sequential import SequentialModel
    from rayoptics.optical.opticalmodel import OpticalModel
    if kind == 'zmx':
        from rayoptics.zemax import zmxread
        for enc in ('utf-16', 'utf-8', 'iso-8859-1'):
            try:
                inpt = pathlib.Path(path).open(encoding=enc).read()
                break
            except UnicodeError:
                pass
        opm, _info = zmxread.read_lens(None, inpt, do_update=False)
    else:
        from rayoptics.codev import cmdproc
        # (files with aperture data make read_lens size the other surfaces by tracing rays,
        # cmdproc.py:89-95: control plane; max_aperture is neutralised in the comparison)
        saved = SequentialModel.set_clear_apertures, OpticalModel.update_model
        SequentialModel.set_clear_apertures = lambda self, **kw: None
        OpticalModel.update_model = lambda self, **kw: None
        try:
            opm, _info = cmdproc.read_lens(pathlib.Path(path), do_update=False)
        finally:
            SequentialModel.set_clear_apertures, OpticalModel.update_model = saved
    opm['seq_model'].update_model()
    return SurfaceTable.from_seq_model(opm['seq_model'])


@pytest.mark.parametrize('rel', FILES)
def test_every_prescription_file_of_the_reference_tree(rel):
    import logging
    from rayoptics_amd import ingest, UnsupportedModelError
    logging.disable(logging.CRITICAL)
    try:
        path = os.path.join(REF, rel)
        kind = rel.rsplit('.', 1)[1]
        if rel in UNMODELLED:
            with pytest.raises(UnsupportedModelError, match=UNMODELLED[rel]):
                ingest.read(path, unknown_types='raise')
            with pytest.warns(UserWarning, match=UNMODELLED[rel]):
                pres = ingest.read(path)
            assert [t for _i, t in pres.unmodelled_types] == [UNMODELLED[rel]]
        else:
            pres = ingest.read(path)
            assert pres.unmodelled_types == []
        ours = pres.to_table(index_of=ingest.reference_fallback_index)
        if rel in REFERENCE_FAILS:
            assert ours.n_ifcs >= 3
            return
        theirs = reference_table(path, kind)
        if kind == 'seq':                       # CODE V listings give max_aperture no value
            for t in (ours, theirs):
                for r in t.rows:
                    r.max_aperture = 1.0
        # (glasses the file defines itself -- CODE V PRV ... END -- are interpolated by
        # opticalglass in the reference: treated like model glasses)
        model_cols = [i for i, m in enumerate(pres.media)
                      if m[0] == 'model' or (m[0] == 'glass' and m[1] in pres.private_glasses)]
        if model_cols:
            d = min(range(len(ours.wvls)), key=lambda w: abs(ours.wvls[w] - 587.5618))
            for t in (ours, theirs):
                t.n_table = t.n_table.copy()
            for i in model_cols:
                if abs(ours.wvls[d] - 587.5618) < 0.05:     # the d line itself: both sides hold nd
                    assert abs(ours.n_table[d, i] - theirs.n_table[d, i]) < 1e-5, (rel, i)
                theirs.n_table[:, i] = ours.n_table[:, i]
                # a mirror-like gap repeats the previous index: propagate the neutralisation
            for i, m in enumerate(pres.media):
                if m[0] == 'mirror' and i > 0:
                    theirs.n_table[:, i] = ours.n_table[:, i] = ours.n_table[:, i - 1]
        rows_equal(ours, theirs, rel)
    finally:
        logging.disable(logging.NOTSET)


ROA_FILES = [
    'gui/tests/Sasian Triplet old.roa',
    'gui/tests/cell_phone_camera_old.roa',
    'models/Cassegrain.roa',
    'models/Dall_Kirkham.roa',
    'models/HybridAchromat.roa',
    'models/Ritchey_Chretien.roa',
    'models/Sasian Triplet.roa',
    'models/TwoMirror.roa',
    'models/TwoSphericalMirror.roa',
    'models/collimator.roa',
    'models/double2frelay.roa',
    'models/f2 focuser.roa',
    'models/galilean.roa',
    'models/petzval.roa',
    'models/singlet_f5.roa',
    'models/telephoto.roa',
    'models/thin_triplet.roa',
    'models/thin_triplet_floating_stop.roa',
    'models/thinlens.roa',
    'models/thinlens_floating_stop.roa',
    'optical/tests/Nikon Nikkor Z 14-30mm f-4 S.roa',
    'optical/tests/US007277232_Example04P.roa',
    'optical/tests/US007277232_Example04P_hikari_glasses.roa',
    'optical/tests/cell_phone_camera.roa',
    'optical/tests/singlet_f3.roa',
    'zemax/models/PhotoPrime/US05331467-1_asm.roa',
]


def test_file_lists_are_the_reference_tree():
    assert FILES == tree_files('zmx', 'seq')
    assert ROA_FILES == tree_files('roa')


@pytest.mark.parametrize('rel', ROA_FILES)
def test_every_roa_file_of_the_reference_tree(rel):
    """.roa models: the reference's own loader needs json_tricks (absent); the stand-in that
    rebuilds the reference's objects from the JSON (tests/golden/refmodels.load_roa) covers the
    files without catalogue glasses or thin lenses -- for those the tables are compared; every
    file must at least parse into a table (or be refused loudly)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'golden'))
    import refmodels as rm
    from rayoptics_amd import SurfaceTable, ingest, UnsupportedModelError
    path = os.path.join(REF, rel)
    pres = ingest.read_roa(path)
    try:
        opm = rm.load_roa(path)
    except (ValueError, KeyError):
        try:
            assert pres.to_table(index_of=ingest.reference_fallback_index).n_ifcs == len(pres.ifcs) >= 3
        except UnsupportedModelError:
            pass
        return
    sm = opm['seq_model']
    try:
        theirs = SurfaceTable.from_seq_model(sm)
    except UnsupportedModelError:
        with pytest.raises(UnsupportedModelError):
            pres.to_table(index_of=ingest.reference_fallback_index)
        return
    wvls = theirs.wvls
    ours = pres.to_table(wvls=wvls, index_of=ingest.reference_fallback_index)
    ours.n_table[:, :len(sm.gaps)] = np.array([[g.medium.rindex(w) for w in wvls] for g in sm.gaps]).T
    ours.n_table[:, len(sm.gaps):] = theirs.n_table[:, len(sm.gaps):]
    for t in (ours, theirs):
        t.rows[0].max_aperture = t.rows[-1].max_aperture = 1.0
    rows_equal(ours, theirs, rel)
