"""Random systems stratified by trace-kernel instance, on rays that mostly get through.

tests/test_gpu_fuzz.py draws hostile systems: most of its rays die at the first interfaces, and
which compiled feature instance (csrc/rox_config.hpp ROX_TRACE_INSTANCES) a seed reaches is an
accident.  Here the instance is an argument: make_system(rng, instance) builds a tame design of
10 to 14 interfaces whose feature set is that instance's, and every system, whatever its
instance, carries what the bundled workloads never combine with it -- two tilted and decentred
rows (one per rt_order), conics, a DUMMY or PHANTOM row, and in about half of them a mirror.
The clear apertures follow a paraxial marginal + chief ray, a little tighter or wider than the
beam, so that rays are lost all the way down the system and not at the front only.

tests/test_stratified_systems_host.py proves with the oracle alone that the committed seed list
(SEEDS) meets the conditions the GPU tests rely on; tests/test_gpu_stratified.py runs them."""
import os
import sys

import numpy as np

from rayoptics_amd import SurfaceTable, abi
from rayoptics_amd.table import field_struct

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# kInstances order (csrc/rox_config.hpp); the feature bits of rox_system_create's scan
INSTANCES = ('lean', 'even', 'radial', 'poly', 'aplist', 'evenap', 'general')
F_EVEN, F_RADIAL, F_TOROID, F_APLIST, F_PHFILT, F_PHASE = 1, 2, 4, 8, 16, 32
F_POLY = F_EVEN | F_RADIAL | F_TOROID
F_ALL = F_POLY | F_APLIST | F_PHFILT | F_PHASE
INSTANCE_FEAT = (0, F_EVEN, F_RADIAL, F_POLY, F_APLIST, F_EVEN | F_APLIST, F_ALL)
# what make_system puts into a system of each instance: exactly the instance's features, except
# `general`, which is reached by a toroid beside an aperture list (no narrower instance has both)
SYSTEM_FEAT = dict(lean=0, even=F_EVEN, radial=F_RADIAL, poly=F_POLY, aplist=F_APLIST,
                   evenap=F_EVEN | F_APLIST, general=F_TOROID | F_APLIST)

WVLS = (486.1, 587.6, 656.3)
R_LIST = 2070           # = 45 x 46, the pupil grid of the GPU tests
GRID_NUM, GRID_ROWS = 46, 45
R_SMALL = 65

# The systems of the suite: three per instance, (instance, k) -> seed.  Chosen once, on the CPU,
# so that the oracle alone meets the conditions of tests/test_stratified_systems_host.py; the
# k-th system of an instance holds a PHANTOM row (k = 0), a DUMMY row (k = 1) or either (k = 2).
SEEDS = {
    'lean': (6, 14, 36),
    'even': (20, 29, 34),
    'radial': (4, 12, 29),
    'poly': (1, 15, 17),
    'aplist': (21, 23, 81),
    'evenap': (18, 70, 77),
    'general': (10, 11, 29),
}


def features(table):
    """the feature scan of rox_system_create (csrc/roxtrace.hip)"""
    f = 0
    for r in table.rows:
        if r.profile == abi.EVENPOLY:
            f |= F_EVEN
        elif r.profile == abi.RADIALPOLY:
            f |= F_RADIAL
        elif r.profile in (abi.YTOROID, abi.XTOROID):
            f |= F_TOROID
        elif r.profile == abi.THINLENS:
            f |= F_PHASE
        if r.n_ap > 0:
            f |= F_APLIST
        if r.ph.kind != abi.PH_NONE:
            f |= F_PHASE
    return f


def expected_instance(table, flags=0):
    """index into INSTANCES of the instance the host launches for (table, rox_opts.flags):
    launch_setup's need -- the system's features, plus F_PHFILT when ROX_FILTER_PHANTOMS drops a
    segment (an interior PHANTOM row: system_slot_map) -- and pick_instance's first cover"""
    need = features(table)
    N = table.n_ifcs
    if (flags & abi.FILTER_PHANTOMS) and any(table.rows[i].mode == abi.PHANTOM for i in range(1, N - 1)):
        need |= F_PHFILT
    for i, feat in enumerate(INSTANCE_FEAT):
        if (need & ~feat) == 0:
            return i
    return len(INSTANCE_FEAT) - 1


def _rot(rng, max_deg):
    a, b, c = np.deg2rad(rng.uniform(-max_deg, max_deg, 3))
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return rx @ ry @ rz


def _pick(rng, pool, k):
    """k distinct members of pool, taken out of it"""
    got = [int(v) for v in rng.choice(pool, size=k, replace=False)]
    for v in got:
        pool.remove(v)
    return got


def make_system(rng, instance, odd_row=None, mirror=None):
    """a SurfaceTable of 10 to 14 interfaces whose features are SYSTEM_FEAT[instance].
    odd_row: 'phantom' / 'dummy' (None: drawn); mirror: True / False (None: drawn)."""
    feat = SYSTEM_FEAT[instance]
    N = int(rng.integers(10, 15))
    interior = list(range(1, N - 1))
    odd_row = odd_row or ('phantom', 'dummy')[int(rng.integers(0, 2))]
    mirror = bool(rng.random() < 0.5) if mirror is None else mirror
    # -- which row is what
    pool = list(interior)
    i_odd = _pick(rng, [i for i in pool if 3 <= i <= N - 3], 1)[0]
    pool.remove(i_odd)
    i_mirror = -1
    if mirror:
        i_mirror = _pick(rng, [i for i in pool if N // 3 <= i <= N - 4], 1)[0]
        pool.remove(i_mirror)
    profile = {}
    if feat & F_EVEN:
        for i in _pick(rng, pool, 2 if instance != 'poly' else 1):
            profile[i] = abi.EVENPOLY
    if feat & F_RADIAL:
        for i in _pick(rng, pool, 2 if instance != 'poly' else 1):
            profile[i] = abi.RADIALPOLY
    if feat & F_TOROID:
        for i in _pick(rng, pool, 1):
            profile[i] = int(rng.choice([abi.YTOROID, abi.XTOROID]))
    for i in _pick(rng, pool, 2):
        profile[i] = abi.CONIC
    if i_mirror > 0 and rng.random() < 0.5:     # a mirror with an asphere / conic profile
        donors = [i for i in profile if i != i_odd]
        profile[i_mirror] = profile.pop(int(rng.choice(donors)))
    tilted = _pick(rng, [i for i in interior if i != i_odd and 2 <= i <= N - 3], 2)
    ap_rows = []
    if feat & F_APLIST:
        ap_rows = [int(v) for v in rng.choice([i for i in interior if i >= 2], size=3, replace=False)]
    # one stronger glass-to-air row in the rear half: steep rays are totally reflected there
    i_strong = -1

    rows = (abi.Surface * N)()
    W = len(WVLS)
    n_table = np.ones((W, N))
    thi0 = float(rng.uniform(60.0, 200.0))
    A = float(rng.uniform(7.0, 10.0))           # semi-aperture of the first interface
    h = float(rng.uniform(0.5, 2.5))            # field height the apertures are sized for
    # paraxial marginal (y, u) and chief (yb, ub) ray of the unfolded system
    y, u = 0.0, A / thi0
    yb, ub = -h, h / thi0
    n_in = 1.0
    glass = False
    zdir = 1.0
    for i in range(N):
        r = rows[i]
        inside = 0 < i < N - 1
        r.mode = abi.DUMMY
        r.profile = abi.SPHERICAL
        r.ec = 1.0
        for k in range(3):
            r.rt[4 * k] = 1.0
        r.rt_order = int(rng.integers(0, 2))
        r.max_aperture = 1e12
        thi = thi0 if i == 0 else float(rng.uniform(2.0, 7.0))
        if i == N - 2:
            thi = float(rng.uniform(6.0, 14.0))
        if i == 0:
            y, yb = y + u * thi, yb + ub * thi
        n_out = n_in
        if inside:
            zdir_in = zdir
            if i == i_odd:
                r.mode = abi.PHANTOM if odd_row == 'phantom' else abi.DUMMY
            elif i == i_mirror:
                r.mode = abi.REFLECT
            else:
                r.mode = abi.TRANSMIT
                glass = not glass
                n_out = float(rng.uniform(1.45, 1.85)) if glass else 1.0
            r.profile = profile.get(i, abi.SPHERICAL)
            # -- curvature: a few hundredths, its sign mostly steering the marginal ray back
            cv = float(rng.uniform(0.005, 0.04))
            if i_strong < 0 and r.mode == abi.TRANSMIT and not glass and i >= N // 2 and i not in profile:
                i_strong = i
                cv = float(rng.uniform(0.055, 0.075))
            if r.mode == abi.REFLECT:
                k_pow = -2.0 * n_in
                cv *= 0.4
            else:
                k_pow = n_out - n_in
            want_pos = (u * y > 0) == (rng.random() < 0.8)      # positive power on a diverging beam
            if k_pow != 0.0:
                c_unf = abs(cv) if (k_pow > 0) == want_pos else -abs(cv)
            else:
                c_unf = cv if rng.random() < 0.5 else -cv
            if i == i_strong:       # concave towards the glass: the normals lean against the beam
                c_unf = abs(cv)
            r.cv = c_unf * zdir_in
            if r.profile != abi.SPHERICAL:
                r.cc = float(rng.uniform(-2.0, 1.0))
                r.ec = r.cc + 1.0
            if r.profile >= abi.EVENPOLY:
                r.ncoef = int(rng.integers(1, 5))
                for k in range(r.ncoef):
                    r.coefs[k] = float(rng.normal() * 0.3 * 10.0 ** (-(3 + 2 * k)))
            if r.profile >= abi.YTOROID:
                r.cR = float(rng.uniform(-0.03, 0.03))
            if r.mode in (abi.TRANSMIT, abi.REFLECT):
                phi = k_pow * c_unf
                if r.mode == abi.REFLECT:
                    u, ub = u - y * phi / n_in, ub - yb * phi / n_in
                else:
                    u, ub = (n_in * u - y * phi) / n_out, (n_in * ub - yb * phi) / n_out
            beam = abs(y) + abs(yb)
            if i == 1:
                r.max_aperture = A
            else:
                r.max_aperture = max(1.5, float(rng.uniform(0.85, 1.12)) * beam + 0.3)
            if i in ap_rows:
                r.n_ap = int(rng.integers(1, 3))
                for k in range(r.n_ap):
                    a = r.ap[k]
                    a.kind = int(rng.choice([abi.AP_CIRCULAR, abi.AP_RECTANGULAR]))
                    a.is_obscuration = 0
                    a.x_offset, a.y_offset = (float(v) for v in rng.uniform(-0.3, 0.3, 2))
                    a.a = max(1.5, float(rng.uniform(0.9, 1.2)) * beam + 0.3)
                    a.b = max(1.5, float(rng.uniform(0.9, 1.2)) * beam + 0.3)
                if i == ap_rows[0]:             # a small central obscuration
                    a = r.ap[r.n_ap - 1]
                    a.kind, a.is_obscuration = abi.AP_CIRCULAR, 1
                    a.a = a.b = float(rng.uniform(0.3, 0.8))
            if r.mode == abi.REFLECT:
                zdir = -zdir
            if i in tilted:
                r.rt_order = abi.RT_F_ORDER if i == tilted[0] else abi.RT_C_ORDER
                m = _rot(rng, 1.5)
                for a_ in range(3):
                    for b_ in range(3):
                        r.rt[3 * a_ + b_] = float(m[a_, b_])
                r.t[0], r.t[1] = (float(v) for v in rng.uniform(-0.3, 0.3, 2))
            y, yb = y + u * thi, yb + ub * thi
        r.z_dir = zdir
        r.t[2] = (thi * zdir) if i < N - 1 else 0.0
        for w in range(W):
            n_table[w, i] = 1.0 if n_out == 1.0 else n_out + 0.006 * (1 - w)
        n_in = n_out
    tbl = SurfaceTable(rows, n_table, WVLS)
    tbl.design = dict(thi0=thi0, A=A, h=h, odd_row=i_odd, mirror=i_mirror, tilted=tilted, strong=i_strong)
    return tbl


def make_rays(rng, tbl, R=R_LIST):
    """pt0, dir0 [3, R]: ~90 % gentle rays aimed inside the first aperture, ~10 % as
    test_gpu_fuzz.random_rays draws them (its hand-laid rays included), a few steep ones"""
    from test_gpu_fuzz import random_rays
    thi0, A, h = tbl.design['thi0'], tbl.design['A'], tbl.design['h']
    n_wild = max(4, R // 10)
    n_steep = min(32, R // 16)
    n_gentle = R - n_wild - n_steep

    def disc(n, rad):
        rr, az = rad * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
        return np.stack([rr * np.cos(az), rr * np.sin(az)])
    tgt = np.concatenate([disc(n_gentle, 0.98 * A), np.full((1, n_gentle), thi0)])
    pt0 = np.concatenate([disc(n_gentle, h), np.zeros((1, n_gentle))])
    # steep: 15 to 50 degrees off the axis, still meeting the first interface well inside it
    th, az = np.deg2rad(rng.uniform(15., 50., n_steep)), rng.uniform(0, 2 * np.pi, n_steep)
    tgt_s = np.concatenate([disc(n_steep, 0.6 * A), np.full((1, n_steep), thi0)])
    pt0_s = tgt_s - thi0 * np.stack([np.tan(th) * np.cos(az), np.tan(th) * np.sin(az), np.ones(n_steep)])
    pt0_w, d_w = random_rays(rng, tbl, n_wild)
    pt0 = np.concatenate([pt0, pt0_s], axis=1)
    d = np.concatenate([tgt, tgt_s], axis=1) - pt0
    d /= np.linalg.norm(d, axis=0)
    pt0, d = np.concatenate([pt0, pt0_w], axis=1), np.concatenate([d, d_w], axis=1)
    perm = rng.permutation(R)           # no wave is all of one kind
    return np.ascontiguousarray(pt0[:, perm]), np.ascontiguousarray(d[:, perm])


def make_field(rng, tbl):
    """a rox_field (ROX_FLD_EPD) for the pupil-grid entries: an object point off the axis, the
    pupil on the first interface and a little larger than its aperture, small vignetting factors"""
    thi0, A, h = tbl.design['thi0'], tbl.design['A'], tbl.design['h']
    pt0 = (float(rng.uniform(-h, h)), float(rng.uniform(-h, h)), 0.0)
    aim = tuple(float(v) for v in rng.uniform(-0.2, 0.2, 2))
    vig = tuple(float(v) for v in rng.uniform(0.0, 0.08, 4))
    return field_struct(pt0, aim, 1.05 * A, thi0, vig=vig, z_dir0=1.0, kind=abi.FLD_EPD)


class Case:
    """one system of the suite with everything the tests trace through it"""

    def __init__(self, instance, k):
        self.instance, self.k = instance, k
        self.seed = SEEDS[instance][k]
        rng = np.random.default_rng([INSTANCES.index(instance), self.seed])
        self.table = make_system(rng, instance, odd_row=(None, 'phantom', 'dummy')[(k + 1) % 3])
        self.pt0, self.dir0 = make_rays(rng, self.table)
        self.wi = rng.integers(0, len(WVLS), R_LIST).astype(np.int32)
        self.field = make_field(rng, self.table)
        self.wvl = int(rng.integers(0, len(WVLS)))
        self.has_phantom = any(r.mode == abi.PHANTOM for r in self.table.rows)

    @property
    def name(self):
        return f'{self.instance}{self.k}'

    def list_opts(self, make_opts, mode, check, extra=0):
        """rox_opts of the ray lists: the options vary from system to system as in test_gpu_fuzz"""
        N = self.table.n_ifcs
        flags = (abi.INTERSECT_OBJ if self.k != 1 else 0) | (abi.CHECK_APERTURES if check else 0) | extra
        return make_opts(flags=flags, out_mode=mode, first_surf=int(self.k % 2),
                         last_surf=(N - 2) if self.k else -1, foc=0.01 * self.seed, image_pt=(0.1, -0.2))

    def grid_opts(self, make_opts, mode, check, extra=0):
        N = self.table.n_ifcs
        flags = abi.INTERSECT_OBJ | abi.APPLY_VIGNETTING | (abi.CHECK_APERTURES if check else 0) | extra
        return make_opts(flags=flags, out_mode=mode, first_surf=1, last_surf=N - 2, foc=-0.02 * self.k,
                         image_pt=(-0.05, 0.15))

    def grid(self, make_grid):
        return make_grid((-1., -1.), (1., 1.), GRID_NUM, row_begin=0, row_count=GRID_ROWS)


_cases = {}


def case(instance, k):
    if (instance, k) not in _cases:
        _cases[instance, k] = Case(instance, k)
    return _cases[instance, k]


def cases(instance=None):
    return [case(i, k) for i in (INSTANCES if instance is None else (instance,)) for k in range(3)]


# ---- the matrix the GPU tests trace, as the oracle computes it ---------------------------------
MODES = (abi.OUT_FULL, abi.OUT_LAST, abi.OUT_HITS)
FIELDS = ('seg', 'op', 'status', 'fail_surf', 'pupil')


def _arrays(res):
    return {f: getattr(res, f) for f in FIELDS if getattr(res, f, None) is not None}


def oracle_results(c):
    """every trace of the matrix through the oracle, computed once per case:
    grid/<wvl>/<mode>/<check>   the 45 x 46 pupil grid at each wavelength (the items of the batch)
    list/<mode>/<check>         the 2070-ray list with per-ray wavelengths
    small/<mode>/<check>        its first 65 rays at one wavelength
    pack_grid/<wvl>/<check>, pack_list/<check>      packed hits: {'hits': [n, 2]}
    filt_grid, filt_list, filt_small                FULL under ROX_FILTER_PHANTOMS (PHANTOM row only)"""
    if getattr(c, '_oracle', None) is not None:
        return c._oracle
    from oracle import oracle
    mk, t = oracle.make_opts, c.table
    grid = c.grid(oracle.make_grid)
    ps, ds = np.ascontiguousarray(c.pt0[:, :R_SMALL]), np.ascontiguousarray(c.dir0[:, :R_SMALL])
    out = {}
    with np.errstate(all='ignore'):
        for check in (1, 0):
            for mode in MODES:
                for w in range(len(WVLS)):
                    out[f'grid/{w}/{mode}/{check}'] = _arrays(
                        oracle.trace_pupil_grid(t, c.field, grid, w, c.grid_opts(mk, mode, check)))
                out[f'list/{mode}/{check}'] = _arrays(
                    oracle.trace_rays(t, c.pt0, c.dir0, c.wi, c.list_opts(mk, mode, check)))
                out[f'small/{mode}/{check}'] = _arrays(
                    oracle.trace_rays(t, ps, ds, c.wvl, c.list_opts(mk, mode, check)))
            for w in range(len(WVLS)):
                out[f'pack_grid/{w}/{check}'] = dict(hits=oracle.trace_pupil_grid(
                    t, c.field, grid, w, c.grid_opts(mk, abi.OUT_HITS_COMPACT, check)).hits)
            out[f'pack_list/{check}'] = dict(hits=oracle.trace_rays(
                t, c.pt0, c.dir0, c.wi, c.list_opts(mk, abi.OUT_HITS_COMPACT, check)).hits)
        if c.has_phantom:
            F = abi.FILTER_PHANTOMS
            out['filt_grid'] = _arrays(oracle.trace_pupil_grid(
                t, c.field, grid, c.wvl, c.grid_opts(mk, abi.OUT_FULL, 1, F)))
            out['filt_list'] = _arrays(oracle.trace_rays(
                t, c.pt0, c.dir0, c.wi, c.list_opts(mk, abi.OUT_FULL, 1, F)))
            out['filt_small'] = _arrays(oracle.trace_rays(t, ps, ds, c.wvl, c.list_opts(mk, abi.OUT_FULL, 1, F)))
    c._oracle = out
    return out


def compare(got, ref, what, failures):
    """got (a host result object) against ref (a dict of the oracle's arrays): equal or both NaN,
    zero signs included (full_placement_child.same_bits); differences are appended to failures"""
    from full_placement_child import same_bits
    for f, r in ref.items():
        g = np.asarray(getattr(got, f))
        if f == 'seg' and g.ndim == 3:
            r = r[:g.shape[0]]          # (the oracle's FULL buffer has a row per interface)
        if same_bits(g, r):
            continue
        if g.shape != r.shape:
            failures.append(f'{what}: {f} has shape {g.shape}, the oracle {r.shape}')
            continue
        if g.dtype.kind == 'f':
            diff = ~((g == r) | (np.isnan(g) & np.isnan(r)))
            kind = 'values'
            if not diff.any():
                diff, kind = np.signbit(g) != np.signbit(r), 'zero signs only'
        else:
            diff, kind = g != r, 'values'
        failures.append(f'{what}: {f} differs from the oracle ({kind}) in {int(diff.sum())} entries, '
                        f'first {np.argwhere(diff)[:3].tolist()}')
