"""Two-reflection ghosts without a GPU: ghost.unfold's row counts, source maps and transforms,
ghost.ghost_pairs' skip reasons, the orientation of ghost.coating_tables, the merging and ranking of
analyses.Ghosts from synthetic records, the NumPy restatement of rox_segment_foci on a closed
form, and the reference fixture tests/golden/ghost.npz (tests/golden/make_ghost.py: the reference's
hand-unfolded models): unfold's rows against the reference's path tuples exactly, the oracle's
packets of the unfolded tables against the reference's within 1e-10 * max(1, |ref|)."""
import json
import os

import numpy as np
import pytest

import segfoci_ref as SR
from helpers import ATOL, GOLDEN, fixture, phase_table
from rayoptics_amd import SurfaceTable, abi, analyses, ghost, workloads
from rayoptics_amd.coatings import Coating
from test_gpu_ghost import catadioptric_model

U = 2.0 ** -53
CASES = (('dblgauss', 2, 1), ('dblgauss', 7, 3), ('dblgauss', 11, 10), ('singlet', 2, 1))


def dblgauss():
    return workloads.load('dblgauss_c2').table


def test_the_export_and_the_record():
    from rayoptics_amd.engine import SEG_FOCUS_DTYPE, load_library
    lib = load_library()
    assert hasattr(lib, 'rox_segment_foci') and 'rox_segment_foci' in abi.EXPORTS
    assert SEG_FOCUS_DTYPE.itemsize == 136 == SR.DTYPE.itemsize and SEG_FOCUS_DTYPE == SR.DTYPE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'roxtrace.h')).read()
    assert 'int rox_segment_foci(rox_system *sys, uint32_t trace_flags, int32_t n_items, const rox_out *outs,' in src
    assert '} rox_seg_focus;             /* 136 bytes' in src


@pytest.mark.parametrize('j,i', [(2, 1), (8, 7), (7, 3), (11, 1)])
def test_unfold_rows_and_source_maps(j, i):
    t = dblgauss()
    N = t.n_ifcs
    u = ghost.unfold(t, j, i)
    Nu = N + 2 * (j - i)
    assert u.table.n_ifcs == Nu and u.table.n_table.shape == (len(t.wvls), Nu) and u.pair == (j, i)
    assert u.source.tolist() == list(range(j + 1)) + list(range(j - 1, i, -1)) + list(range(i, N))
    assert u.pass_.tolist() == [0] * (j + 1) + [1] * (j - i) + [2] * (N - 1 - i)
    assert np.flatnonzero(u.reflects).tolist() == [j, 2 * j - i]
    rows = u.table.rows
    for k in range(Nu):
        s, src = int(u.source[k]), t.rows[int(u.source[k])]
        assert rows[k].mode == (abi.REFLECT if u.reflects[k] else src.mode)
        for name in ('profile', 'ncoef', 'n_ap', 'flags', 'cv', 'cc', 'ec', 'cR', 'max_aperture'):
            assert getattr(rows[k], name) == getattr(src, name), (k, name)
        assert bytes(rows[k].ap) == bytes(src.ap) and bytes(rows[k].ph) == bytes(src.ph)
        back = j <= k < 2 * j - i
        g = s - 1 if back else s
        assert u.segment_gap[k] == g
        assert np.array_equal(u.table.n_table[:, k], t.n_table[:, g])
        assert rows[k].z_dir == (-t.rows[g].z_dir if back else t.rows[g].z_dir)
        if back:                                    # centred: exactly the identity and (0, 0, -thi)
            assert list(rows[k].rt) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and rows[k].rt_order == abi.RT_C_ORDER
            assert list(rows[k].t) == [0.0, 0.0, -t.rows[g].t[2]] and str(rows[k].t[0]) == '0.0'
        else:
            assert bytes(rows[k])[:0] == b'' and list(rows[k].rt) == list(src.rt) and list(rows[k].t) == list(src.t)
    for k in range(j):                              # the object side up to j is untouched
        assert bytes(rows[k]) == bytes(t.rows[k])
    for k in range(i + 1, N):
        assert bytes(rows[k + 2 * (j - i)]) == bytes(t.rows[k])
    assert u.segment_pass.tolist() == [0] * j + [1] * (j - i) + [2] * (N - i)
    with pytest.raises(ValueError, match='is not a pair'):
        ghost.unfold(t, i, j)


def test_inverse_transform_of_a_decentered_gap():
    """Forward is p' = rt (p - t); the row back carries rt' = rt^T exactly and t' = -(rt t),
    component a formed as -((rt[a][0] t0 + rt[a][1] t1) + rt[a][2] t2): three products and two sums,
    so |t' + rt t| <= 3 u sum_k |rt[a][k] t[k]| (the standard bound gamma_3 of a 3-term dot product,
    first order) -- the rounding of one 3 x 3 product.  Forward followed by the inverse then
    returns p up to that and the orthogonality defect D = max |rt^T rt - I| of the STORED rt (a
    property of the table, measured in longdouble): |back(forward(p)) - p| <= 3 D |p - t|_1 +
    3 u sum|rt t| summed over the three components."""
    t = fixture('tilted_singlet').table
    ld = np.longdouble
    tilted = [g for g in range(1, t.n_ifcs - 2)
              if not np.array_equal(np.array(list(t.rows[g].rt)).reshape(3, 3), np.identity(3))]
    assert tilted, 'the fixture has no decentered gap'
    j, i = t.n_ifcs - 2, 1
    pairs, skipped = ghost.ghost_pairs(t)
    assert (j, i) in pairs and not skipped
    u = ghost.unfold(t, j, i)
    rng = np.random.default_rng(2)
    checked = 0
    for k in range(j, 2 * j - i):
        g = int(u.segment_gap[k])
        rt = np.array(list(t.rows[g].rt)).reshape(3, 3)
        tt = np.array(list(t.rows[g].t))
        rb = np.array(list(u.table.rows[k].rt)).reshape(3, 3)
        tb = np.array(list(u.table.rows[k].t))
        assert np.array_equal(rb, rt.T) and u.table.rows[k].rt_order == abi.RT_C_ORDER
        exact = -(rt.astype(ld) @ tt.astype(ld))
        bound_t = 3 * U * (np.abs(rt) @ np.abs(tt))
        assert (np.abs(tb.astype(ld) - exact) <= bound_t).all(), (g, tb, exact)
        D = float(np.abs(rt.T.astype(ld) @ rt.astype(ld) - np.identity(3)).max())
        p = rng.uniform(-10, 10, (3, 64))
        fwd = rt.astype(ld) @ (p.astype(ld) - tt.astype(ld)[:, None])
        back = rb.astype(ld) @ (fwd - tb.astype(ld)[:, None])
        bound = 3 * D * np.abs(p - tt[:, None]).sum(axis=0) + bound_t.sum() + 4 * 2.0 ** -64 * 64
        assert (np.abs(back - p).max(axis=0) <= bound).all(), (g, np.abs(back - p).max(), bound.min())
        checked += g in tilted
    assert checked, 'no decentered gap in the doubled section'


def test_pairs_and_skip_reasons():
    t = dblgauss()
    pairs, skipped = ghost.ghost_pairs(t)
    assert len(pairs) == 45 and not skipped and all(0 < i < j < t.n_ifcs - 1 for j, i in pairs)
    assert 6 not in {s for p in pairs for s in p}           # the stop: no index step
    assert ghost.ghost_pairs(t, surfaces=[7, 3, 6])[0] == [(7, 3)]
    with pytest.raises(ValueError, match='surfaces'):
        ghost.ghost_pairs(t, surfaces=[0])
    # the RC telescope: mirrors in air, nothing refracts -- no pair and nothing to skip
    assert ghost.ghost_pairs(workloads.load('rc_telescope_c4').table) == ([], [])
    pairs, skipped = ghost.ghost_pairs(catadioptric_model().workload.table)
    assert pairs == [(2, 1), (6, 5)]
    assert skipped == [((j, i), 'interface 3 between them is a mirror') for j, i in ((5, 1), (5, 2), (6, 1), (6, 2))]
    # a DOE on a refracting surface between two others
    rng = np.random.default_rng(3)
    while True:
        tbl, k = phase_table(rng, 'doe')
        lo = [s for s in range(1, k) if ghost.can_reflect(tbl, s)]
        hi = [s for s in range(k + 1, tbl.n_ifcs - 1) if ghost.can_reflect(tbl, s)]
        if lo and hi:
            break
    pairs, skipped = ghost.ghost_pairs(tbl)
    assert not ghost.can_reflect(tbl, k) and all(k not in p for p in pairs)
    want = {(j, i) for j in hi for i in lo}
    assert {p for p, _w in skipped} == want
    assert all(why == f'interface {k} between them carries a phase element' for _p, why in skipped)
    with pytest.raises(ValueError, match='phase element'):
        ghost.unfold(tbl, hi[0], lo[0])


def test_coating_tables_orientation():
    t = dblgauss()
    nt = t.n_table
    W = len(t.wvls)
    c = Coating([(1.38, 100.0), (2.1, 50.0)])
    u = ghost.unfold(t, 7, 3)
    ct = ghost.coating_tables(t, u, c)
    first, idx, thick = ct['stack_first'], ct['layer_index'], ct['layer_thickness']

    def layers(k):
        return [(idx[0, m, 0], thick[m]) for m in range(first[k], first[k + 1])]

    as_written, flipped = [(1.38, 100.0), (2.1, 50.0)], [(2.1, 50.0), (1.38, 100.0)]
    assert idx.shape == (W, first[-1], 2) and (idx[..., 1] == 0).all()
    for k in range(u.table.n_ifcs):
        s = int(u.source[k])
        air_b4, air_after = (u.table.n_table[:, k - 1] == 1).all(), (u.table.n_table[:, k] == 1).all()
        if u.reflects[k]:
            assert ct['coat_kind'][k] == abi.COAT_STACK
            behind = nt[:, 7] if s == 7 else nt[:, 2]
            assert np.array_equal(ct['sub_index'][:, k, 0], behind) and (ct['sub_index'][:, k, 1] == 0).all()
            # 7: met from the air, as written; 3: met from the glass, reversed
            assert layers(k) == (as_written if s == 7 else flipped), (k, layers(k))
        elif 0 < s < t.n_ifcs - 1 and air_b4 != air_after:
            assert ct['coat_kind'][k] == abi.COAT_STACK
            assert layers(k) == (as_written if air_b4 else flipped), (k, layers(k))
        else:
            assert ct['coat_kind'][k] == abi.COAT_BARE and layers(k) == []
    # rows 8 .. 10 run back through 6, 5, 4: surface 5 (glass -> air nominally) is entered from the air
    assert [int(s) for s in u.source[8:11]] == [6, 5, 4] and layers(9) == as_written and layers(5) == flipped
    # no coating: bare transmissions, reflecting rows a stack without layers
    ct = ghost.coating_tables(t, u, None)
    assert ct['stack_first'][-1] == 0 and [int(k) for k in np.flatnonzero(ct['coat_kind'] == abi.COAT_STACK)] == [7, 11]
    assert (ct['coat_kind'][~u.reflects] == abi.COAT_BARE).all()
    # a fixed transmission reflects the rest; 'ideal' reflects nothing
    ct = ghost.coating_tables(t, u, (0.99, 0.98))
    for k in (7, 11):
        assert ct['coat_kind'][k] == abi.COAT_FIXED and np.allclose(ct['coat_value'][k], (0.01, 0.02), rtol=0, atol=2 * U)
    assert ct['coat_kind'][5] == abi.COAT_FIXED and ct['coat_value'][5].tolist() == [0.99, 0.98]
    ct = ghost.coating_tables(t, u, 'ideal')
    for k in (7, 11):
        assert ct['coat_kind'][k] == abi.COAT_FIXED and ct['coat_value'][k].tolist() == [0.0, 0.0]
    assert (ct['coat_kind'][~u.reflects] == abi.COAT_IDEAL).all()
    # a dict entry on the cemented surface 4 (glass both sides): as written on the way in, reversed back
    ct = ghost.coating_tables(t, u, {4: c})
    first, idx, thick = ct['stack_first'], ct['layer_index'], ct['layer_thickness']
    assert layers(4) == as_written and layers(10) == flipped and layers(12) == as_written


def synthetic_records(P, F, W, n_seg, seed=0):
    from rayoptics_amd.engine import SEG_FOCUS_DTYPE
    rng = np.random.default_rng(seed)
    recs = []
    for _p in range(P):
        r = np.zeros((F, W, n_seg), SEG_FOCUS_DTYPE)
        r['n'] = 100
        r['w_sum'] = rng.uniform(1e-4, 1e-3, (F, W, n_seg))
        r['w_in'] = r['w_sum'] * 0.5
        r['n_in'] = 50
        r['a_mean'] = rng.normal(size=(F, W, n_seg, 2))
        r['m_bb'] = r['w_sum'] * 0.01
        r['m_ab'] = -r['m_bb'] * 5.0                        # zeta* = 5
        r['m_aa'] = r['m_bb'] * 25.0 + r['w_sum'] * 0.04    # smallest RMS 0.2
        r['z_in_min'], r['z_in_max'], r['z_out_min'], r['z_out_max'] = -1.0, 1.0, 9.0, 10.0
        recs.append(r)
    return recs


def test_ghosts_merging_and_ranking():
    P, F, W, n_seg = 3, 2, 3, 7
    recs = synthetic_records(P, F, W, n_seg)
    recs[1]['w_sum'][:, :, -1] *= 100.0                     # the brightest ghost
    for name in ('w_in', 'm_aa', 'm_ab', 'm_bb'):
        recs[1][name][:, :, -1] *= 100.0
    recs[2]['n'][0, 1, -1] = 0                              # an item without a ray
    for name in ('w_sum', 'w_in'):
        recs[2][name][0, 1, -1] = 0.0
    for name in ('a_mean', 'm_aa', 'm_ab', 'm_bb'):
        recs[2][name][0, 1, -1] = np.nan
    slots = [dict(source=np.arange(n_seg), pass_=np.array([0, 0, 1, 1, 2, 2, 2]), gap=np.arange(n_seg))] * P
    for r in recs:                                          # only slot 3's focus lies in its segment
        r['z_out_min'][:, :, [0, 1, 2, 4, 5]] = 1.5
        r['z_out_max'][:, :, [0, 1, 2, 4, 5]] = 2.0
    signal = np.full((F, W), 0.9)
    s = np.array([1.0, 2.0, 1.0])
    g = analyses.Ghosts([(2, 1), (3, 1), (3, 2)], [((5, 1), 'why')], recs, slots, signal, s)
    assert g.flux.shape == (P, F, W) and np.array_equal(g.flux[0], recs[0]['w_sum'][:, :, -1])
    assert np.allclose(g.ratio, g.flux / 0.9) and np.allclose(g.in_detector[0], 0.5)
    assert np.allclose(g.focus_distance[:2], 5.0) and np.isnan(g.focus_distance[2, 0, 1])
    assert np.allclose(g.rms_patch[0], np.sqrt(25.0 * 0.01 + 0.04))
    assert np.allclose(g.poly_flux[0], (g.flux[0] * s).sum(axis=1) / s.sum())
    assert np.allclose(g.poly_ratio[0], g.poly_flux[0] / 0.9)
    # the item without a ray: no flux (it counts as 0 in the merge), and no patch (it takes no part)
    keep = [0, 2]
    assert g.flux[2, 0, 1] == 0.0 and np.isclose(g.poly_flux[2, 0], (g.flux[2, 0] * s).sum() / s.sum())
    assert np.isnan(g.rms_patch[2, 0, 1]) and np.isnan(g.in_detector[2, 0, 1])
    assert np.isclose(g.poly_rms_patch[2, 0], (g.rms_patch[2, 0, keep] * s[keep]).sum() / s[keep].sum())
    assert [p for p, _f in g.ranking()][0] == 1 and len(g.ranking()) == P
    foci = g.internal_foci
    assert {f['source'] for f in foci} == {3} and {f['pass_'] for f in foci} == {1}
    assert len(foci) == P * F * W and all(abs(f['zeta'] - 5.0) < 1e-12 and abs(f['rms_min'] - 0.2) < 1e-12 for f in foci)
    text = g.table(2)
    assert text.count('\n') == 3 and '(  3,   1)' in text.splitlines()[1] and 'skipped: why' in text
    empty = analyses.Ghosts([], [], [], [], signal, s)
    assert empty.flux.shape == (0, F, W) and empty.ranking() == [] and empty.internal_foci == []


def test_restatement_on_a_closed_form():
    """two rays through (0, 0, 10) with slopes +-0.1 and weights 1 and 3: every moment by hand"""
    seg = np.zeros((1, 10, 4))
    for r, (m, z0) in enumerate(((0.1, 0.0), (-0.1, 1.0))):
        n = 1.0 / np.sqrt(1.0 + m * m)
        seg[0, :, r] = [m * (z0 - 10.0), 0.0, z0, m * n, 0.0, n, 20.0, 0, 0, 1]
    seg[0, :, 2:] = np.nan
    status = np.array([0, 0, 1, 4], np.uint8)
    rec, ab, ex = SR.segment_foci(seg, status, np.array([1.0, 3.0, np.nan, np.nan]))
    r = rec[0]
    assert r['n'] == 2 and r['n_in'] == 2 and r['n_bad'] == 0 and r['w_sum'] == 4.0 == r['w_in']
    # a = -10 b: a = (-1, +1), b = (+0.1, -0.1); mean b = (0.1 - 0.3)/4 = -0.05; m_bb = 1*0.15^2 + 3*0.05^2 = 0.03
    assert np.allclose(r['b_mean'], (-0.05, 0.0), atol=4 * U) and np.allclose(r['a_mean'], (0.5, 0.0), atol=8 * U)
    assert np.isclose(r['m_bb'], 0.03, rtol=16 * U) and np.isclose(r['m_ab'], -0.3, rtol=16 * U)
    assert np.isclose(r['m_aa'], 3.0, rtol=16 * U)
    zeta, ms_min, ms0 = SR.derive(rec)
    assert abs(float(zeta[0]) - 10.0) < 1e-13 and abs(float(ms_min[0])) < 1e-14 and np.isclose(float(ms0[0]), 0.75)
    assert r['z_in_min'] == 0.0 and r['z_in_max'] == 1.0 and r['z_out_min'] > 19.0
    from rayoptics_amd.engine import seg_focus_derive
    z2, m2, m0, inside = seg_focus_derive(rec)
    assert abs(z2[0] - 10.0) < 1e-13 and m2[0] < 1e-14 and inside[0] and np.isclose(m0[0], 0.75)
    # a negative and an infinite weight are counted in n_bad and nowhere else; N == 0 in n_flat
    seg[0, 5, 1] = 0.0
    rec, _ab, _ex = SR.segment_foci(seg, np.zeros(4, np.uint8), np.array([1.0, 3.0, -1.0, np.inf]))
    assert rec['n'][0] == 1 and rec['n_flat'][0] == 1 and rec['n_bad'][0] == 2 and rec['m_aa'][0] == 0.0


def ghost_fixture():
    return np.load(os.path.join(GOLDEN, 'ghost.npz'))


@pytest.mark.parametrize('name,j,i', CASES)
def test_unfold_against_the_reference_tuples(name, j, i):
    z = ghost_fixture()
    key = f'{name}_{j}_{i}'
    nominal = SurfaceTable.from_dict(json.loads(str(z[f'{key}/nominal_json'])))
    theirs = SurfaceTable.from_dict(json.loads(str(z[f'{key}/unfolded_json'])))
    ours = ghost.unfold(nominal, j, i).table
    assert ours.n_ifcs == theirs.n_ifcs and ours.wvls == theirs.wvls
    assert np.array_equal(ours.n_table, theirs.n_table)
    assert [r.z_dir for r in ours.rows][:-1] == z[f'{key}/z_dir'].tolist()
    # rt_order is not part of a tuple: it records which memory layout the reference's rt array has
    # (which dgemv NumPy reaches, table.rt_order_of).  unfold states ROX_RT_C_ORDER for the rows it
    # inverts; the reference builds its reversed gaps' (identity) matrices as transposed views.  On
    # an identity matrix both orders give the same bits, so the tag is set aside and everything
    # else -- mode, profile, apertures, rt, t, z_dir, flags -- is compared byte for byte.
    back = range(j, 2 * j - i)
    for k in back:
        assert list(theirs.rows[k].rt) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and ours.rows[k].rt_order == abi.RT_C_ORDER
        theirs.rows[k].rt_order = abi.RT_C_ORDER
    do, dt = ours.to_dict(), theirs.to_dict()
    for k, (a, b) in enumerate(zip(do['rows'], dt['rows'])):
        assert a == b, (k, {n: (a[n], b[n]) for n in a if a[n] != b[n]})
    for a, b in zip(ours.rows, theirs.rows):
        assert bytes(a) == bytes(b)


@pytest.mark.parametrize('name,j,i', CASES)
def test_oracle_packets_against_the_reference(name, j, i):
    from oracle import oracle
    z = ghost_fixture()
    key = f'{name}_{j}_{i}'
    nominal = SurfaceTable.from_dict(json.loads(str(z[f'{key}/nominal_json'])))
    tbl = ghost.unfold(nominal, j, i).table
    wi = int(z[f'{key}/wvl_idx'])
    opts = oracle.make_opts(flags=abi.INTERSECT_OBJ | abi.APPLY_VIGNETTING, out_mode=abi.OUT_FULL, first_surf=1,
                            last_surf=tbl.n_ifcs - 2)
    for f, (fb, pupil, ref) in enumerate(zip(z[f'{key}/fields'], z[f'{key}/pupil'], z[f'{key}/seg'])):
        fld = abi.Field.from_buffer_copy(fb.tobytes())
        res = oracle.trace_pupil_list(tbl, fld, np.ascontiguousarray(pupil[:, 0]), np.ascontiguousarray(pupil[:, 1]),
                                      wi, opts)
        assert (res.status == abi.OK).all(), (key, f, res.status)        # no ray is left out
        seg = np.asarray(res.seg)
        assert seg.shape == ref.shape == (tbl.n_ifcs, 10, 25)
        err = np.abs(seg - ref) / np.maximum(1.0, np.abs(ref))
        print(f'{key} field {f}: largest scaled deviation {err.max():.3g}')
        assert err.max() <= ATOL, (key, f, err.max())
