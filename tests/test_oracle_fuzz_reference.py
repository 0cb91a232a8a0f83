"""Randomized differential test, oracle vs the reference: random hand-built paths -- every
profile kind, mirrors, dummies, phantoms, clear-aperture lists, tilted/decentered transforms
held either as the F-ordered transpose view or as a C-ordered array -- traced by the
reference's own trace_raw and by oracle/rox_oracle.c, compared bit for bit (segments, op,
status, failing surface, partial packets).

Where the reference is not importable the oracle is checked against the reference's side as
stored in tests/golden/fuzz_paths.npz (tests/golden/make_golden.py --only-fuzz): each path's
surface table, the generator state its rays are drawn from, and per ray the status, failing
surface and a 64-bit digest of the packet (tests/helpers.py packet_digest).  Where it is
importable, the live comparison also regenerates the stored case and requires it unchanged."""
import json
import os

import numpy as np
import pytest

SEEDS = range(30)
R = 160
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fuzz_paths.npz')


def rot(rng, max_deg):
    a, b, c = np.deg2rad(rng.uniform(-max_deg, max_deg, 3))
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return rx @ ry @ rz


def random_path(rng):
    from rayoptics.elem import profiles, surface
    n_surf = int(rng.integers(1, 8))
    N = n_surf + 2
    path = []
    zdir = 1
    for i in range(N):
        interior = 0 < i < N - 1
        s = surface.Surface(interact_mode='dummy')
        thi = float(rng.uniform(1.0, 15.0)) if i > 0 else float(rng.choice([20.0, 300.0]))
        n = 1.0
        if interior:
            s.interact_mode = str(rng.choice(['transmit'] * 6 + ['reflect', 'dummy', 'phantom']))
            kind = int(rng.integers(0, 8))
            cv = float(rng.uniform(-0.07, 0.07)) if rng.random() > 0.15 else 0.0
            cc = float(rng.uniform(-2.0, 1.0))
            co = [float(rng.normal() * 10.0 ** (-(3 + 2 * k))) for k in range(int(rng.integers(0, 5)))]
            co += [0.0] * (10 - len(co))
            if kind <= 2:
                s.profile = profiles.Spherical(c=cv)
            elif kind == 3:
                s.profile = profiles.Conic(c=cv, cc=cc)
            elif kind == 4:
                s.profile = profiles.EvenPolynomial(c=cv, cc=cc, coefs=co)
            elif kind == 5:
                s.profile = profiles.RadialPolynomial(c=cv, ec=cc + 1.0, coefs=co)
            elif kind == 6:
                s.profile = profiles.YToroid(c=cv, cR=float(rng.uniform(-0.05, 0.05)), cc=cc, coefs=co)
            else:
                s.profile = profiles.XToroid(c=cv, cR=float(rng.uniform(-0.05, 0.05)), cc=cc, coefs=co)
            s.profile.update()
            s.max_aperture = float(rng.uniform(4.0, 12.0))
            if rng.random() < 0.3:
                cas = []
                for _ in range(int(rng.integers(1, 3))):
                    kw = dict(x_offset=float(rng.uniform(-1, 1)), y_offset=float(rng.uniform(-1, 1)),
                              is_obscuration=bool(rng.random() < 0.2))
                    if rng.random() < 0.6:
                        cas.append(surface.Circular(radius=float(rng.uniform(2, 9)), **kw))
                    else:
                        cas.append(surface.Rectangular(x_half_width=float(rng.uniform(2, 9)),
                                                       y_half_width=float(rng.uniform(2, 9)), **kw))
                s.clear_apertures = cas
            if s.interact_mode == 'reflect':
                zdir = -zdir
            if zdir < 0:
                thi = -thi
            n = 1.0 if rng.random() < 0.4 else float(rng.uniform(1.3, 1.9))
        else:
            s.max_aperture = 1e12
        t = np.array([0., 0., thi if i < N - 1 else 0.0])
        if interior and rng.random() < 0.3:
            m = rot(rng, 6.0)
            t[:2] = rng.uniform(-0.5, 0.5, 2)
            # the reference holds r.transpose() (an F-ordered view); C-ordered
            # arrays arise from 'dec and return' decenters
            rt = m.transpose() if rng.random() < 0.5 else np.ascontiguousarray(m.transpose())
        else:
            rt = np.identity(3)
        path.append([s, None, (rt, t), n, zdir])
    return path


def options(seed, N):
    """trace_raw keywords and the matching oracle flags of case `seed` on an N-interface path"""
    from rayoptics_amd import abi
    check = bool(seed % 3)
    filt = (seed % 4 == 0)
    kw = dict(first_surf=int(seed % 2), last_surf=(N - 2) if seed % 5 else None,
              check_apertures=check, filter_out_phantoms=filt)
    flags = abi.INTERSECT_OBJ | (abi.CHECK_APERTURES if check else 0) | (abi.FILTER_PHANTOMS if filt else 0)
    return kw, flags


def random_rays(rng, thi0):
    """the R rays of a case, drawn after its path"""
    pt0 = np.stack([rng.uniform(-6, 6, R), rng.uniform(-6, 6, R), np.zeros(R)])
    tgt = np.stack([rng.uniform(-10, 10, R), rng.uniform(-10, 10, R), np.full(R, thi0)])
    d = tgt - pt0
    d /= np.linalg.norm(d, axis=0)
    d[:, 0] = [0., 0., 1.]
    pt0[:, 0] = 0.0
    return pt0, d


def reference_case(seed):
    """case `seed` traced by the reference: the path's surface table (JSON), the generator state
    the rays are drawn from (JSON) with the object distance thi0, the rays, and per ray the
    packet (seg [N, 10, R], NaN past its last segment), op, status and failing surface;
    valid[r] is False where trace_raw raised a non-Trace exception (degenerate geometry: no
    contract)"""
    from oracle import refshim
    refshim.install()
    from rayoptics.raytr.raytrace import trace_raw
    from rayoptics.raytr import traceerror as terr
    from rayoptics_amd import SurfaceTable, abi
    rng = np.random.default_rng(7000 + seed)
    path = random_path(rng)
    N = len(path)
    tbl = SurfaceTable.from_paths([path], [550.0])
    thi0 = path[0][2][1][2]
    state = json.dumps(rng.bit_generator.state)
    pt0, d = random_rays(rng, thi0)
    kw, _flags = options(seed, N)
    kinds = {terr.TraceMissedSurfaceError: abi.MISSED_SURFACE, terr.TraceTIRError: abi.TIR,
             terr.TraceRayBlockedError: abi.BLOCKED}
    seg = np.full((N, 10, R), np.nan)
    op = np.full(R, np.nan)
    status = np.zeros(R, np.int64)
    fail_surf = np.full(R, -1, np.int64)
    valid = np.ones(R, bool)
    for r in range(R):
        try:
            with np.errstate(all='ignore'):
                ray, op_r, _ = trace_raw(iter(path), pt0[:, r].copy(), d[:, r].copy(), 550.0, **kw)
            st, surf = abi.OK, -1
        except terr.TraceError as e:
            st, surf = kinds[type(e)], e.surf
            ray, op_r, _ = e.ray_pkg
        except (ValueError, ZeroDivisionError, FloatingPointError):
            valid[r] = False
            continue
        status[r], fail_surf[r], op[r] = st, surf, op_r
        seg[:len(ray), :, r] = np.array([np.concatenate([s[0], s[1], [s[2]], s[3]])
                                         for s in ray]).reshape(-1, 10)
    return {'table': np.array(json.dumps(tbl.to_dict())), 'rng': np.array(state), 'thi0': np.array(thi0),
            'pt0': pt0, 'd': d, 'seg': seg, 'op': op, 'status': status, 'fail_surf': fail_surf,
            'valid': valid}


def stored_form(case):
    """what tests/golden/fuzz_paths.npz keeps of a reference_case(): the rays as the generator
    state they are drawn from, the packets as one packet_digest per ray"""
    import helpers as H
    out = {k: case[k] for k in ('table', 'rng', 'thi0', 'status', 'fail_surf', 'valid')}
    out['status'] = out['status'].astype(np.int8)
    out['fail_surf'] = out['fail_surf'].astype(np.int8)
    out['digest'] = H.packet_digests(case['seg'], case['op'], case['valid'])
    return out


def stored_case(seed):
    with np.load(GOLDEN) as z:
        return {k.split('_', 1)[1]: z[k] for k in z.files if k.split('_', 1)[0] == f's{seed}'}


def trace_oracle(seed, table_json, pt0, d):
    from oracle import oracle
    from rayoptics_amd import SurfaceTable
    tbl = SurfaceTable.from_dict(json.loads(str(table_json)))
    kw, flags = options(seed, tbl.n_ifcs)
    opts = oracle.make_opts(flags=flags, first_surf=kw['first_surf'],
                            last_surf=-1 if kw['last_surf'] is None else kw['last_surf'])
    with np.errstate(all='ignore'):
        return tbl.n_ifcs, oracle.trace_rays(tbl, pt0, d, 0, opts)


def assert_oracle_equals(seed, ref):
    """the oracle on case `seed` against the reference's packets (a reference_case())"""
    N, res = trace_oracle(seed, ref['table'], ref['pt0'], ref['d'])
    rays = np.flatnonzero(ref['valid'])
    for r in rays:
        st, surf = ref['status'][r], ref['fail_surf'][r]
        assert res.status[r] == st and res.fail_surf[r] == surf, (seed, r, st, surf)
        want, got = ref['seg'][:, :, r], res.seg[:N, :, r]
        assert np.array_equal(want, got, equal_nan=True), (seed, r, np.argwhere(want != got)[:3].tolist())
        assert np.isnan(res.seg[N:, :, r]).all()
        assert np.array_equal(ref['op'][r], res.op[r], equal_nan=True)
    assert len(rays) > R // 2


@pytest.mark.needs_reference
@pytest.mark.parametrize('seed', SEEDS)
def test_oracle_equals_reference_on_random_paths(seed):
    live = reference_case(seed)
    assert_oracle_equals(seed, live)
    # ... and the stored case is this one
    stored, ref = stored_form(live), stored_case(seed)
    assert sorted(stored) == sorted(ref)
    for k in stored:
        assert stored[k].shape == ref[k].shape and np.array_equal(stored[k], ref[k]), (seed, k)


@pytest.mark.parametrize('seed', SEEDS)
def test_oracle_equals_stored_reference_on_random_paths(seed):
    """the same comparison against the stored case: every ray's status and failing surface,
    and its packet (segments, op) bit for bit by digest"""
    import helpers as H
    ref = stored_case(seed)
    pt0, d = random_rays(H.rng_from_state(ref['rng']), float(ref['thi0']))
    N, res = trace_oracle(seed, ref['table'], pt0, d)
    rays = np.flatnonzero(ref['valid'])
    for r in rays:
        st, surf = ref['status'][r], ref['fail_surf'][r]
        assert res.status[r] == st and res.fail_surf[r] == surf, (seed, r, st, surf)
        assert H.packet_digest(res.seg[:N, :, r], res.op[r]) == ref['digest'][r], (seed, r, res.seg[:N, :, r])
        assert np.isnan(res.seg[N:, :, r]).all()
    assert len(rays) > R // 2
