"""Thin-film coatings and metal mirrors for the transmission analysis.

A :class:`Coating` is a stack of homogeneous layers, each ``(material, thickness_nm)``, listed from
the outside (air) towards the glass -- the way coating prescriptions are written -- and, for a
mirror, the metal behind them (``substrate``).  A material is a real or complex number, a callable
``n(wvl_nm)``, a ``(wvls_nm, n)`` table interpolated linearly, or any object with
``rindex(wvl_nm)``.  The convention is N = n + ik with exp(-iwt): k > 0 absorbs.

``Coating.coefficients`` evaluates a stack on the host (NumPy) for plots of R against wavelength
and angle; ``stack_tables`` builds the arrays rox_surface_thinfilm takes
(include/roxtrace.h states the arithmetic of the device)."""
import collections
import numbers

import numpy as np

from . import abi

Coefficients = collections.namedtuple('Coefficients', 'rs rp ts tp Rs Rp Ts Tp')


def index_of(material, wvl_nm):
    """the complex index of ``material`` at ``wvl_nm`` (a scalar)"""
    w = float(wvl_nm)
    if isinstance(material, str):
        raise ValueError(f'Coating: material {material!r}: names are not looked up (no catalogue): pass an index')
    if hasattr(material, 'rindex'):
        v = material.rindex(w)
    elif callable(material):
        v = material(w)
    elif isinstance(material, numbers.Number):
        v = material
    else:
        try:
            ws, ns = material
            ws, ns = np.asarray(ws, dtype=np.float64).reshape(-1), np.asarray(ns, dtype=np.complex128).reshape(-1)
            if ws.size != ns.size or ws.size < 1 or not (np.diff(ws) > 0).all():
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f'Coating: material {material!r} is not a number, a callable n(wvl_nm), a table '
                             f'(wvls_nm, n) with increasing wavelengths or an object with rindex(wvl_nm)') from None
        v = complex(np.interp(w, ws, ns.real), np.interp(w, ws, ns.imag))
    v = complex(v)
    if not (np.isfinite(v.real) and np.isfinite(v.imag) and v.real >= 0.0 and v.imag >= 0.0 and abs(v) > 0.0):
        raise ValueError(f'Coating: index {v!r} of {material!r} at {w} nm: re and im must be finite and >= 0 '
                         f'(N = n + ik, k > 0 absorbs)')
    return v


def _sqrt_up(z):
    """sqrt on the branch Im >= 0 (Re >= 0 when Im == 0)"""
    g = np.sqrt(np.asarray(z, dtype=np.complex128))
    return np.where(g.imag < 0.0, -g, g)


class Coating:
    """``layers``: a sequence of (material, thickness_nm) from the outside (air) towards the glass;
    ``substrate``: the metal behind the layers of a mirror coating (None: an ideal conductor is not
    assumed -- a Coating on a mirror needs one); ``name``: for messages."""

    def __init__(self, layers, substrate=None, name=None):
        self.layers = []
        for layer in layers:
            try:
                material, d = layer
                d = float(d)
            except (TypeError, ValueError):
                raise ValueError(f'Coating: layer {layer!r} is not (material, thickness_nm)') from None
            if not (np.isfinite(d) and d >= 0.0):
                raise ValueError(f'Coating: thickness {d!r} nm must be finite and >= 0')
            self.layers.append((material, d))
        if len(self.layers) > abi.MAX_COAT_LAYERS:
            raise ValueError(f'Coating: {len(self.layers)} layers, more than {abi.MAX_COAT_LAYERS}')
        self.substrate = substrate
        self.name = name

    def __repr__(self):
        return f'Coating({self.name or ""}: {len(self.layers)} layers' + \
            (', on a substrate)' if self.substrate is not None else ')')

    @classmethod
    def quarter_wave(cls, n, wvl0_nm, name=None):
        """one layer of index ``n`` (evaluated at ``wvl0_nm``), a quarter of ``wvl0_nm`` thick optically"""
        n0 = index_of(n, wvl0_nm).real
        if not n0 > 0.0:
            raise ValueError(f'Coating.quarter_wave: index {n0!r} must be > 0')
        return cls([(n, float(wvl0_nm) / (4.0 * n0))], name=name or f'quarter wave n={n0:g} at {float(wvl0_nm):g} nm')

    def reversed(self):
        """the same layers crossed the other way"""
        return Coating(self.layers[::-1], self.substrate, self.name)

    @property
    def thicknesses(self):
        return np.array([d for _m, d in self.layers], dtype=np.float64)

    def indices(self, wvl_nm):
        """complex [n_layers] at ``wvl_nm``; a layer's re must be > 0"""
        out = np.array([index_of(m, wvl_nm) for m, _d in self.layers], dtype=np.complex128)
        if out.size and not (out.real > 0.0).all():
            raise ValueError(f'Coating: a layer index with re <= 0 at {float(wvl_nm)} nm: {out}')
        return out

    def coefficients(self, n_in, n_out, wvl_nm, cos_inc=1.0):
        """Amplitude and power coefficients of the stack between ``n_in`` (real) and ``n_out`` (real,
        or complex: a metal), the layers crossed in the order they are listed, at vacuum wavelength
        ``wvl_nm`` and cosine of incidence ``cos_inc`` (in ``n_in``); the two broadcast.  The
        characteristic matrix of every layer (Macleod, Thin-Film Optical Filters), with e^(Im delta)
        divided out of each layer so that absorbing layers do not overflow.
        -> Coefficients(rs, rp, ts, tp, Rs, Rp, Ts, Tp): rs, rp are the ratios of the tangential
        fields (rs == rp at normal incidence), ts, tp those of the electric field amplitudes;
        Ts, Tp include the ratio of the admittances: R + T = 1 for a lossless stack."""
        wvl, ci = np.broadcast_arrays(np.asarray(wvl_nm, dtype=np.float64), np.asarray(cos_inc, dtype=np.float64))
        shape = wvl.shape
        wvl, ci = wvl.reshape(-1), ci.reshape(-1)
        uniq, inv = np.unique(wvl, return_inverse=True)
        n0 = np.array([index_of(n_in, w) for w in uniq])[inv]
        ns = np.array([index_of(n_out, w) for w in uniq])[inv]
        if (n0.imag != 0.0).any() or not (n0.real > 0.0).all():
            raise ValueError('Coating.coefficients: the medium of incidence must be real')
        n0 = n0.real
        lay = np.array([self.indices(w) for w in uniq]).reshape(uniq.size, len(self.layers))[inv]    # [M, L]
        a2 = n0 * n0 * (1.0 - ci * ci)
        with np.errstate(all='ignore'):
            g0, gs = n0 * ci + 0j, _sqrt_up(ns * ns - a2)
            y0 = {'s': g0, 'p': n0 * n0 / g0}
            ye = {'s': gs, 'p': ns * ns / gs}
            B = {k: np.ones_like(gs) for k in 'sp'}
            C = {k: ye[k].copy() for k in 'sp'}
            att = np.zeros(wvl.shape)
            for j in range(len(self.layers) - 1, -1, -1):
                N = lay[:, j]
                g = _sqrt_up(N * N - a2)
                delta = 2.0 * np.pi * self.layers[j][1] * g / wvl
                e2 = np.exp(-2.0 * delta.imag)
                ch, sh = (1.0 + e2) / 2.0, (1.0 - e2) / 2.0
                cs = np.cos(delta.real) * ch - 1j * np.sin(delta.real) * sh
                sn = np.sin(delta.real) * ch + 1j * np.cos(delta.real) * sh
                att = att + delta.imag
                for k, y in (('s', g), ('p', N * N / g)):
                    B[k], C[k] = cs * B[k] - 1j * sn * C[k] / y, -1j * y * sn * B[k] + cs * C[k]
            out = {}
            for k in 'sp':
                den = y0[k] * B[k] + C[k]
                out['r' + k] = (y0[k] * B[k] - C[k]) / den
                tau = np.exp(-att) * 2.0 * y0[k] / den
                out['T' + k] = ye[k].real / y0[k].real * np.abs(tau) ** 2
                out['t' + k] = tau if k == 's' else tau * ci / (gs / ns)
                out['R' + k] = np.abs(out['r' + k]) ** 2
        return Coefficients(*(out[k].reshape(shape) for k in ('rs', 'rp', 'ts', 'tp', 'Rs', 'Rp', 'Ts', 'Tp')))


def stack_tables(table, stacks, what='stack_tables'):
    """the arrays rox_surface_thinfilm takes for ``stacks`` = {interface index: Coating}, each
    Coating's layers already in the order the light crosses them (from the medium before the
    interface to the medium after it) -> (stack_first int32 [n_ifcs + 1], layer_thickness [L],
    layer_index [n_wvls, L, 2], sub_index [n_wvls, n_ifcs, 2] or None without a mirror among
    them), the indices evaluated at every wavelength of ``table`` (nm)."""
    N, wvls = table.n_ifcs, list(table.wvls)
    first = np.zeros(N + 1, np.int32)
    thick, index = [], [[] for _w in wvls]
    sub = None
    for i in range(N):
        c = stacks.get(i)
        if c is not None:
            row = table.rows[i]
            mirror = row.mode == abi.REFLECT
            glass = row.mode == abi.TRANSMIT and row.profile != abi.THINLENS and row.ph.kind == abi.PH_NONE
            if not 0 < i < N - 1 or not (mirror or glass):
                raise ValueError(f'{what}: coatings: interface {i} takes no Coating: it is not a refracting surface '
                                 f'(thin lenses and phase elements excluded) or a mirror between object and image')
            if mirror and c.substrate is None:
                raise ValueError(f'{what}: coatings: the Coating on mirror {i} has no substrate (the metal)')
            thick += [d for _m, d in c.layers]
            for w, wvl in enumerate(wvls):
                index[w] += list(c.indices(wvl))
            if mirror:
                if sub is None:
                    sub = np.zeros((len(wvls), N, 2))
                    sub[:, :, 0] = 1.0
                for w, wvl in enumerate(wvls):
                    v = index_of(c.substrate, wvl)
                    sub[w, i] = v.real, v.imag
        first[i + 1] = len(thick)
    if len(thick) > abi.MAX_COAT_LAYERS_TOTAL:
        raise ValueError(f'{what}: coatings: {len(thick)} layers in all, more than {abi.MAX_COAT_LAYERS_TOTAL}')
    idx = np.array(index, dtype=np.complex128).reshape(len(wvls), len(thick))
    return first, np.array(thick, dtype=np.float64), np.ascontiguousarray(np.stack([idx.real, idx.imag], axis=-1)), sub
