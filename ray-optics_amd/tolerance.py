"""Tolerancing from one trace: the host side of rox_wave_differentials (include/roxtrace.h).

The device leaves, per (field, wavelength) item, the covariance sums of per-ray columns: aux rows
(column 0 the nominal OPD W0 in waves, then the pupil coordinates) and eleven first-order changes
of optical path per selected slot (COLUMN_KINDS).  Everything here is NumPy on n_cols-sized
objects.

A perturbation is a coefficient vector over the slot columns -- [n_cols], or [n_items, n_cols]
where it depends on the wavelength -- in path length (system units) per unit of its amplitude;
:class:`Perturbations` builds them.  The columns are INCREASES of optical path and ROX_OUT_OPD
falls as a ray's path grows, so in waves

    W(e, c) = W0 - (1/lambda_i) * sum_q e_q coef_q . cols - (1/lambda_i) * sum_m c_m comp_m . cols

per ray of item i.  The mean-square wavefront of a field -- each wavelength's own piston removed,
wavelengths merged with the spectral weights -- is a quadratic form z^T H_f z in z = (1, e, c)
(:class:`Quadratic`); the compensators c, one value shared by every field and wavelength, follow in
closed form from the weighted sum of the H_f.  First order leaves out a term of order (transverse
aberration x change of ray angle); the object-space rays are kept and the stop is not re-aimed."""
import numpy as np

from . import abi

COLUMN_KINDS = ('dx', 'dy', 'dz', 'rx', 'ry', 'rz', 'cv', 'pw', 'a0', 'a45', 'dn')
_AXIS = {'x': 0, 'y': 1, 'z': 2, 0: 0, 1: 1, 2: 2}


def slot_interfaces(table, trace_flags=0):
    """the interface of every FULL-packet slot (engine.TraceEngine.slot_interfaces)"""
    N = table.n_ifcs
    filt = bool(int(trace_flags) & abi.FILTER_PHANTOMS)
    return [i for i, row in enumerate(table.rows) if not (filt and row.mode == abi.PHANTOM and 0 < i < N - 1)]


def column_names(table, slots=None, n_aux=0, trace_flags=0):
    """the name of every column: ('aux', a) for the aux rows, then (slot, kind) for the eleven
    columns of every selected slot, kind one of COLUMN_KINDS"""
    n_seg = len(slot_interfaces(table, trace_flags))
    slots = list(range(n_seg)) if slots is None else [int(k) for k in slots]
    return [('aux', a) for a in range(int(n_aux))] + [(k, kind) for k in slots for kind in COLUMN_KINDS]


class Tolerance:
    """a named perturbation: ``coef`` [n_cols] or [n_items, n_cols] and the magnitude of its range"""

    def __init__(self, name, coef, magnitude, unit=''):
        self.name, self.coef, self.magnitude, self.unit = str(name), np.asarray(coef, dtype=np.float64), \
            float(magnitude), unit

    def __repr__(self):
        return f'Tolerance({self.name!r}, +-{self.magnitude:g} {self.unit})'


class Perturbations:
    """the coefficient vectors of a table's perturbations over the columns of one
    wave_differentials call: ``slots`` (None: all) and ``n_aux`` as given to it, ``wvl_idxs`` the
    items' rows of the index table (for the builders that depend on wavelength)"""

    def __init__(self, table, slots=None, n_aux=0, wvl_idxs=(0,), trace_flags=0):
        self.table = table
        self.slot_ifc = slot_interfaces(table, trace_flags)
        n_seg = len(self.slot_ifc)
        self.slots = list(range(n_seg)) if slots is None else [int(k) for k in slots]
        self.n_aux = int(n_aux)
        self.n_cols = self.n_aux + len(COLUMN_KINDS) * len(self.slots)
        self.wvl_idxs = [int(w) for w in wvl_idxs]
        self.image = table.n_ifcs - 1

    # -- columns
    def col(self, s, kind):
        """the column of interface ``s`` (negative: from the image back) and ``kind``"""
        s = int(s) + (self.table.n_ifcs if int(s) < 0 else 0)
        if s not in self.slot_ifc or self.slot_ifc.index(s) not in self.slots:
            raise ValueError(f'interface {s} has no selected slot')
        return self.n_aux + len(COLUMN_KINDS) * self.slots.index(self.slot_ifc.index(s)) + COLUMN_KINDS.index(kind)

    def _vec(self):
        return np.zeros(self.n_cols)

    def _check_surface(self, s, what):
        if not 0 < int(s) < self.table.n_ifcs:
            raise ValueError(f'{what}: interface {s} outside [1, {self.table.n_ifcs - 1}]')

    def _parallel(self, s1, s2, what):
        """the frames of interfaces s1 .. s2 are parallel: rt of rows s1 .. s2 - 1 the identity"""
        for i in range(int(s1), int(s2)):
            rt = np.array(list(self.table.rows[i].rt)).reshape(3, 3)
            if not np.array_equal(rt, np.identity(3)):
                raise ValueError(f'{what}: the frames of interfaces {i} and {i + 1} are not parallel')

    def _vertex(self, s1, s):
        """the vertex of interface s in the frame of s1 (parallel frames)"""
        v = np.zeros(3)
        for i in range(int(s1), int(s)):
            v = v + np.array(list(self.table.rows[i].t))
        return v

    # -- rigid bodies
    def surface_decenter(self, s, axis):
        self._check_surface(s, 'surface_decenter')
        v = self._vec()
        v[self.col(s, ('dx', 'dy', 'dz')[_AXIS[axis]])] = 1.0
        return v

    def surface_tilt(self, s, axis):
        self._check_surface(s, 'surface_tilt')
        v = self._vec()
        v[self.col(s, ('rx', 'ry', 'rz')[_AXIS[axis]])] = 1.0
        return v

    def element_decenter(self, s1, s2, axis):
        if not 0 < int(s1) <= int(s2) < self.table.n_ifcs:
            raise ValueError(f'element_decenter: interfaces {s1} .. {s2} are not a group')
        self._parallel(s1, s2, 'element_decenter')
        return sum(self.surface_decenter(s, axis) for s in range(int(s1), int(s2) + 1))

    def element_tilt(self, s1, s2, axis, pivot_z=None):
        """the group s1 .. s2 rotated by a unit angle about ``axis`` through the point
        (0, 0, pivot_z) of s1's frame (None: s1's vertex): per surface the rotation about its own
        vertex plus the shift axis x (vertex - pivot)"""
        if not 0 < int(s1) <= int(s2) < self.table.n_ifcs:
            raise ValueError(f'element_tilt: interfaces {s1} .. {s2} are not a group')
        self._parallel(s1, s2, 'element_tilt')
        a = np.identity(3)[_AXIS[axis]]
        P = np.array([0.0, 0.0, 0.0 if pivot_z is None else float(pivot_z)])
        v = self._vec()
        for s in range(int(s1), int(s2) + 1):
            v = v + self.surface_tilt(s, axis)
            shift = np.cross(a, self._vertex(s1, s) - P)
            for c in range(3):
                v[self.col(s, ('dx', 'dy', 'dz')[c])] += shift[c]
        return v

    def thickness(self, g):
        """gap g (after interface g) grows by one unit: every later interface, the image
        included, shifts by +z"""
        if not 0 <= int(g) < self.table.n_ifcs - 1:
            raise ValueError(f'thickness: gap {g} outside [0, {self.table.n_ifcs - 2}]')
        self._parallel(int(g) + 1, self.table.n_ifcs - 1, 'thickness')
        v = self._vec()
        for s in range(int(g) + 1, self.table.n_ifcs):
            if s in self.slot_ifc:
                v[self.col(s, 'dz')] = 1.0
        return v

    # -- figure
    def curvature(self, s):
        self._check_surface(s, 'curvature')
        v = self._vec()
        v[self.col(s, 'cv')] = 1.0
        return v

    def radius(self, s):
        """per unit of radius: dcv = -dR / R^2"""
        cv = float(self.table.rows[int(s)].cv)
        if cv == 0.0:
            raise ValueError(f'radius: interface {s} is flat')
        return self.curvature(s) * (-cv * cv)

    def power_fringes(self, s, wvl_nm, semi_diameter, units_per_nm=1e-6):
        """per fringe of power against a test plate at ``wvl_nm``: half a wave of sag at the rim"""
        self._check_surface(s, 'power_fringes')
        v = self._vec()
        v[self.col(s, 'pw')] = 0.5 * wvl_nm * units_per_nm / float(semi_diameter) ** 2
        return v

    def irregularity_fringes(self, s, wvl_nm, semi_diameter, angle=0.0, units_per_nm=1e-6):
        """per fringe of astigmatic irregularity at ``angle`` (radians)"""
        self._check_surface(s, 'irregularity_fringes')
        k = 0.5 * wvl_nm * units_per_nm / float(semi_diameter) ** 2
        v = self._vec()
        v[self.col(s, 'a0')] = k * np.cos(2 * angle)
        v[self.col(s, 'a45')] = k * np.sin(2 * angle)
        return v

    # -- media
    def index(self, g):
        if not 0 < int(g) < self.table.n_ifcs - 1:
            raise ValueError(f'index: gap {g} outside [1, {self.table.n_ifcs - 2}]')
        v = self._vec()
        v[self.col(g, 'dn')] = 1.0
        return v

    def abbe(self, g, ref_wvl_idx=0):
        """per unit of dV/V at a fixed index at the reference wavelength: dn_w = -(n_w - n_ref)
        -> [n_items, n_cols]"""
        base = self.index(g)
        nt = np.abs(np.asarray(self.table.n_table))
        return np.stack([-(nt[w, int(g)] - nt[int(ref_wvl_idx), int(g)]) * base for w in self.wvl_idxs])

    def elements(self):
        """[(s1, s2)]: consecutive interfaces with a medium other than air between them.  Every glass
        gap is an element of its own: the two halves of a cemented doublet come as (s, s + 1) and
        (s + 1, s + 2), not as one group (element_decenter(s, s + 2, ..) is that group)"""
        nt = np.abs(np.asarray(self.table.n_table))[0]
        return [(s, s + 1) for s in range(1, self.table.n_ifcs - 2) if nt[s] != 1.0]


GRADES = {'commercial': dict(decenter=0.05, tilt=np.radians(3 / 60), thickness=0.1, power=3.0, irregularity=1.0,
                             index=1e-3, abbe=0.008),
          'precision': dict(decenter=0.02, tilt=np.radians(1 / 60), thickness=0.025, power=1.0, irregularity=0.25,
                            index=3e-4, abbe=0.003)}


def default_tolerances(pert, grade='commercial', test_wvl_nm=632.8, units_per_nm=1e-6, ref_wvl_idx=0):
    """a standard set over ``pert`` (a :class:`Perturbations`): per glass element decentres and
    tilts in x and y, its thickness, index and Abbe number; per glass surface power and
    irregularity fringes over its max_aperture.  What to know about the set: an element is one
    glass gap (Perturbations.elements), so the halves of a cemented group are decentred and tilted
    separately, which overstates what a cemented group can do -- pass element_decenter /
    element_tilt over the whole group for a build-like set; an element whose frames are not
    parallel, or that is followed by frames that are not, gets no decentre, tilt or thickness
    tolerance (the builders' ValueError is taken as "not applicable", silently); ``ref_wvl_idx`` is
    the row of the index table that the Abbe tolerance holds fixed (analyses.tolerance_sensitivity
    passes the first wavelength of its call, not the central one)."""
    g = GRADES[grade]
    out = []
    seen = set()
    for s1, s2 in pert.elements():
        try:
            for ax in 'xy':
                out.append(Tolerance(f'E{s1}-{s2} decentre {ax}', pert.element_decenter(s1, s2, ax), g['decenter'], 'mm'))
                out.append(Tolerance(f'E{s1}-{s2} tilt {ax}', pert.element_tilt(s1, s2, ax), g['tilt'], 'rad'))
            out.append(Tolerance(f'T{s1} thickness', pert.thickness(s1), g['thickness'], 'mm'))
        except ValueError:
            pass
        out.append(Tolerance(f'N{s1} index', pert.index(s1), g['index']))
        out.append(Tolerance(f'V{s1} Abbe', pert.abbe(s1, ref_wvl_idx), g['abbe'], 'dV/V'))
        for s in (s1, s2):
            if s in seen:
                continue
            seen.add(s)
            sd = float(pert.table.rows[s].max_aperture)
            if not (np.isfinite(sd) and sd > 0):
                continue
            out.append(Tolerance(f'S{s} power', pert.power_fringes(s, test_wvl_nm, sd, units_per_nm), g['power'], 'fr'))
            out.append(Tolerance(f'S{s} irregularity', pert.irregularity_fringes(s, test_wvl_nm, sd, 0.0, units_per_nm),
                                 g['irregularity'], 'fr'))
    return out


def covariances(item, sums, gram):
    """per item the covariance of the columns over the counted rays (each item's own means
    removed): cov = gram/n - (sums/n)(sums/n)^T -> [n_items, n_cols, n_cols]; an item without a
    counted ray gives NaN"""
    n = np.asarray(item['n'], dtype=np.float64)[:, None, None]
    with np.errstate(invalid='ignore', divide='ignore'):
        m = np.asarray(sums)[:, :, None] / n
        return np.asarray(gram) / n - m * np.swapaxes(m, 1, 2)


class Quadratic:
    """the mean-square wavefront as a quadratic form.  ``cov`` [F, W, n_cols, n_cols] (waves are
    made here: ``wave_scale`` [F, W] = 1/lambda in system units), ``coefs`` Q perturbations and
    ``comps`` M compensators (each [n_cols] or [F*W, n_cols]), ``w0_col`` the column of W0 in
    waves.  H[f] is the (1 + Q + M)^2 form of field f over z = (1, e, c), polychromatic."""

    def __init__(self, cov, wave_scale, coefs, comps, spectral_wts, field_wts=None, w0_col=0):
        cov = np.asarray(cov, dtype=np.float64)
        F, W, n_cols, _ = cov.shape
        self.F, self.W, self.Q, self.M = F, W, len(coefs), len(comps)
        sw = np.asarray(spectral_wts, dtype=np.float64)
        self.sw = sw / sw.sum()
        fw = np.ones(F) if field_wts is None else np.asarray(field_wts, dtype=np.float64)
        self.fw = fw / fw.sum()
        self.cov = cov
        self.ws = ws = np.asarray(wave_scale, dtype=np.float64).reshape(F, W)
        K = 1 + self.Q + self.M
        self.A = np.zeros((F, W, n_cols, K))            # the columns' vectors of z's entries, in waves
        for q, c in enumerate(list(coefs) + list(comps)):
            c = np.asarray(c, dtype=np.float64)
            c = np.broadcast_to(c, (F * W, n_cols)).reshape(F, W, n_cols)
            self.A[:, :, :, 1 + q] = -ws[:, :, None] * c
        self.A[:, :, w0_col, 0] = 1.0
        Hi = np.einsum('fwak,fwab,fwbl->fwkl', self.A, cov, self.A)
        self.H = np.einsum('w,fwkl->fkl', self.sw, Hi)  # [F, K, K]
        self.Hall = np.einsum('f,fkl->kl', self.fw, self.H)

    def compensate(self, e):
        """the compensator values that minimise the field-weighted mean square for the amplitudes
        ``e`` [.., Q] -> [.., M]"""
        e = np.asarray(e, dtype=np.float64)
        if self.M == 0:
            return np.zeros(e.shape[:-1] + (0,))
        n = 1 + self.Q
        Hcc, Hcx = self.Hall[n:, n:], self.Hall[n:, :n]
        x = np.concatenate([np.ones(e.shape[:-1] + (1,)), e], axis=-1)
        return -np.linalg.solve(Hcc, Hcx @ x[..., None])[..., 0] if e.ndim > 1 else -np.linalg.solve(Hcc, Hcx @ x)

    def mean_square(self, e, c=None):
        """[.., F]: the mean-square wavefront (waves^2) of every field for amplitudes ``e`` [.., Q]
        and compensators ``c`` [.., M] (None: the best ones)"""
        e = np.asarray(e, dtype=np.float64)
        c = self.compensate(e) if c is None else np.asarray(c, dtype=np.float64)
        z = np.concatenate([np.ones(e.shape[:-1] + (1,)), e, c], axis=-1)
        return np.maximum(np.einsum('...k,fkl,...l->...f', z, self.H, z), 0.0)

    def rms(self, e, c=None):
        return np.sqrt(self.mean_square(e, c))


class ToleranceSensitivity:
    """what analyses.tolerance_sensitivity returns.

    ``names`` / ``magnitudes`` [Q]; ``nominal_rms`` [F] and ``nominal_poly`` (the field-weighted
    RMS) in waves, uncompensated; ``rms_plus`` / ``rms_minus`` [Q, F] the RMS with one tolerance at
    +- its magnitude after compensation, ``comp_plus`` / ``comp_minus`` [Q, M] the compensators'
    motions (system units), ``delta_rms`` [Q, F] the larger increase over the compensated nominal;
    ``pupil_tilt`` [Q, F, 2] the tilt of each tolerance's wavefront change at its magnitude, from
    its fit against the pupil columns (waves per unit pupil coordinate), and ``image_shift``
    [Q, F, 2] the (x, y) position of the image relative to the image slot that this tilt amounts to
    (:meth:`_pupil_fit`); ``quadratic`` the
    :class:`Quadratic`; ``item`` / ``pivot`` / ``sums`` / ``gram`` what the device returned and,
    with ``keep_cols``, ``cols`` the per-ray columns in HBM [F*W, n_cols, R]."""

    def __init__(self, tolerances, comp_names, quadratic, item, pivot, sums, gram, flds=None, wvls=None,
                 image_cols=None, cols=None, num_rays=None, pupil_cols=(1, 2)):
        self.tolerances = list(tolerances)
        self.names = [t.name for t in self.tolerances]
        self.magnitudes = np.array([t.magnitude for t in self.tolerances])
        self.comp_names = list(comp_names)
        self.quadratic = q = quadratic
        self.item, self.pivot, self.sums, self.gram, self.cols = item, pivot, sums, gram, cols
        self.flds, self.wvls, self.num_rays = flds, wvls, num_rays
        Q = q.Q
        zero = np.zeros(Q)
        self.nominal_rms = q.rms(zero, np.zeros(q.M))
        self.nominal_poly = float(np.sqrt((q.fw * self.nominal_rms ** 2).sum()))
        self.nominal_compensated = q.rms(zero)
        self.nominal_comp = q.compensate(zero)
        E = np.diag(self.magnitudes)
        self.comp_plus, self.comp_minus = q.compensate(E), q.compensate(-E)
        self.rms_plus, self.rms_minus = q.rms(E), q.rms(-E)
        self.delta_rms = np.maximum(self.rms_plus, self.rms_minus) - self.nominal_compensated[None, :]
        self.pupil_tilt = self.image_shift = None
        if image_cols is not None and pupil_cols is not None:
            self.pupil_tilt, self.image_shift = self._pupil_fit(pupil_cols, image_cols)

    def _pupil_fit(self, pupil_cols, image_cols):
        """-> (pupil_tilt [Q, F, 2], image_shift [Q, F, 2]).  Per field, polychromatic, the
        least-squares fit of a wavefront change against the pupil columns (px, py) is its tilt, in
        waves per unit of the pupil coordinate.  The same fit of the image slot's dx and dy columns
        gives the 2 x 2 matrix K of tilt per unit shift of the image slot -- of the reference
        sphere's centre; the shift that cancels tolerance q's tilt, -K^-1 tilt_q, is where the
        image lies relative to the image slot with q at its magnitude."""
        q = self.quadratic
        n_cols = q.A.shape[2]
        p = list(pupil_cols)
        tilt, shift = np.zeros((q.Q, q.F, 2)), np.zeros((q.Q, q.F, 2))
        for f in range(q.F):
            Cpp, cq, ck = np.zeros((2, 2)), np.zeros((2, q.Q)), np.zeros((2, 2))
            for w in range(q.W):
                B = np.zeros((n_cols, 2))
                for c in range(2):
                    B[image_cols[c], c] = -q.ws[f, w]
                Cp = q.cov[f, w][p, :]
                Cpp += q.sw[w] * Cp[:, p]
                cq += q.sw[w] * (Cp @ q.A[f, w, :, 1:1 + q.Q])
                ck += q.sw[w] * (Cp @ B)
            t = np.linalg.solve(Cpp, cq) * self.magnitudes[None, :]      # [2, Q]
            K = np.linalg.solve(Cpp, ck)
            tilt[:, f, :] = t.T
            shift[:, f, :] = (-np.linalg.solve(K, t)).T
        return tilt, shift

    def rss(self):
        """[F] the root-sum-square estimate of the RMS wavefront: sqrt(nominal^2 + sum_q
        delta_q^2), delta_q the larger compensated change of tolerance q at +- its magnitude"""
        d = np.maximum(self.delta_rms, 0.0)
        return np.sqrt(self.nominal_compensated ** 2 + (d * d).sum(axis=0))

    def worst(self, n=10):
        """the n tolerances with the largest field-weighted change -> [(name, magnitude, change)]"""
        w = (self.quadratic.fw[None, :] * self.delta_rms).sum(axis=1)
        order = np.argsort(-w)[:n]
        return [(self.names[i], float(self.magnitudes[i]), float(w[i])) for i in order]

    def table(self, n=10):
        lines = [f'{"tolerance":<28s} {"+-":>10s} {"d rms (waves)":>14s}']
        for name, mag, ch in self.worst(n):
            lines.append(f'{name:<28s} {mag:>10.3g} {ch:>14.5f}')
        lines.append(f'nominal {self.nominal_poly:.5f} waves; RSS per field ' +
                     ' '.join(f'{v:.5f}' for v in self.rss()))
        return '\n'.join(lines)

    def monte_carlo(self, n_trials, dist='uniform', seed=0, percentiles=(50, 90, 98)):
        """``n_trials`` draws of every tolerance -- uniform over +- its magnitude, or normal with
        sigma = magnitude / 2 -- each a quadratic form with its own best compensators; no device
        work -> (rms [n_trials, F], percentiles [len(percentiles), F])"""
        rng = np.random.default_rng(seed)
        Q = self.quadratic.Q
        if dist == 'uniform':
            e = rng.uniform(-1.0, 1.0, (int(n_trials), Q))
        elif dist == 'normal':
            e = rng.normal(0.0, 0.5, (int(n_trials), Q))
        else:
            raise ValueError(f"monte_carlo: dist {dist!r} is not 'uniform' or 'normal'")
        rms = self.quadratic.rms(e * self.magnitudes[None, :])
        return rms, np.percentile(rms, percentiles, axis=0)

    def delta_map(self, q, item):
        """the pupil map [num_rays, num_rays] of tolerance q's wavefront change (waves per unit
        amplitude) of item ``item``, NaN where a ray is not counted: a device product of the kept
        columns (``keep_cols``)"""
        if self.cols is None:
            raise ValueError('delta_map: needs keep_cols=True')
        t = self.cols
        import torch
        f, w = divmod(int(item), self.quadratic.W)
        a = torch.from_numpy(np.ascontiguousarray(self.quadratic.A[f, w, :, 1 + int(q)])).to(t.device)
        # (NaN columns of rays that are not counted stay NaN: 0 * NaN)
        m = (a[:, None] * t[int(item)]).sum(dim=0)
        return m.reshape(self.num_rays, self.num_rays).cpu().numpy()
