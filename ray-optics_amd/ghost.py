"""Two-reflection ghost paths as surface tables.

Light reflected at a refracting surface j and again at an earlier one i (0 < i < j < N - 1)
travels on to the image: the ghost (j, i).  Its path is an ordinary sequential path -- the
reference models one as a hand-unfolded SequentialModel of transmit, reflect, reflect, transmit
whose reversed gaps carry t = (0, 0, -thi), the index unsigned and z_dir = -1 between the
reflections -- which is the row convention of ``rox_surface``: ``unfold`` builds that table from
the nominal one, and the trace kernels, the oracle and ``rox_surface_thinfilm`` take it as it is.

``ghost_pairs``     which pairs there are, and which are skipped and why
``unfold``          the table of one pair, with each row's source interface, pass and role
``coating_tables``  the user's ``coatings`` (read against the nominal table) as the coating
                    tables of an unfolded table: ROX_REFLECT rows with a stack and a real
                    ``sub_index`` give the Fresnel reflection of a bare or coated dielectric
"""
import ctypes as C

import numpy as np

from . import abi
from .coatings import index_of
from .table import SurfaceTable


def can_reflect(table, s):
    """whether interface s is a refracting surface a ghost can reflect at: ROX_TRANSMIT, no thin
    lens, no phase element, and an index step at some wavelength"""
    if not 0 < s < table.n_ifcs - 1:
        return False
    row = table.rows[s]
    nt = np.asarray(table.n_table)
    return bool(row.mode == abi.TRANSMIT and row.profile != abi.THINLENS and row.ph.kind == abi.PH_NONE and
                (nt[:, s - 1] != nt[:, s]).any())


def _blocker(table, s):
    """why a ghost cannot cross interface s twice more, or None"""
    row = table.rows[s]
    if row.mode == abi.REFLECT:
        return f'interface {s} between them is a mirror'
    if row.ph.kind != abi.PH_NONE:
        return f'interface {s} between them carries a phase element'
    if row.profile == abi.THINLENS:
        return f'interface {s} between them is a thin lens'
    return None


def ghost_pairs(table, surfaces=None):
    """-> (pairs, skipped): ``pairs`` the (j, i), 0 < i < j < N - 1, whose two rows can both
    reflect (``can_reflect``), j ascending then i ascending; ``surfaces`` restricts the
    candidates to those interface indices.  A pair with a mirror, a phase element or a thin lens
    among the rows i + 1 .. j - 1 is not unfolded: it goes to ``skipped`` as ((j, i), reason)."""
    N = table.n_ifcs
    cand = [s for s in range(1, N - 1) if can_reflect(table, s)]
    if surfaces is not None:
        want = {int(s) for s in surfaces}
        bad = sorted(s for s in want if not 0 < s < N - 1)
        if bad:
            raise ValueError(f'ghost_pairs: surfaces {bad} are not interface indices in [1, {N - 2}]')
        cand = [s for s in cand if s in want]
    pairs, skipped = [], []
    for j in cand:
        for i in cand:
            if i >= j:
                break
            why = next((w for w in (_blocker(table, s) for s in range(i + 1, j)) if w), None)
            if why:
                skipped.append(((j, i), why))
            else:
                pairs.append((j, i))
    return pairs, skipped


class Unfolded:
    """what :func:`unfold` returns: ``table`` (N + 2(j - i) rows) and per row ``source`` (the
    nominal interface), ``pass_`` (reflections before the row: 0, 1 or 2) and ``reflects``;
    ``pair`` = (j, i).  ``segment_pass[u]`` is the pass the ray is on after row u, and
    ``segment_gap[u]`` the nominal gap it crosses there (the medium it is in)."""

    def __init__(self, table, pair, source, pass_, reflects, segment_gap):
        self.table, self.pair = table, pair
        self.source = np.asarray(source, np.int32)
        self.pass_ = np.asarray(pass_, np.int32)
        self.reflects = np.asarray(reflects, bool)
        self.segment_gap = np.asarray(segment_gap, np.int32)
        self.segment_pass = self.pass_ + self.reflects


def _copy_row(dst, src):
    C.memmove(C.byref(dst), C.byref(src), C.sizeof(abi.Surface))


def _rt_of(row):
    return np.array(list(row.rt), dtype=np.float64).reshape(3, 3)


def _set_inverse(dst, fwd):
    """dst's transform <- the inverse of row ``fwd``'s: forward is p' = rt (p - t), so the way
    back is p = rt^T p' + t = rt^T (p' - t'), t' = -(rt t).  An undecentered gap (rt the identity,
    t = (0, 0, thi)) gives exactly the identity and (0, 0, -thi)."""
    rt = _rt_of(fwd)
    t = np.array(list(fwd.t), dtype=np.float64)
    ti = np.array([-((rt[a, 0] * t[0] + rt[a, 1] * t[1]) + rt[a, 2] * t[2]) + 0.0 for a in range(3)])
    for a in range(3):
        for b in range(3):
            dst.rt[3 * a + b] = rt[b, a]
        dst.t[a] = ti[a]
    dst.rt_order = abi.RT_C_ORDER


def unfold(table, j, i):
    """the table of ghost (j, i): rows 0 .. j - 1 as they are, the row from j ROX_REFLECT, the rows
    from j - 1 .. i + 1 with their modes, the row from i ROX_REFLECT with row i's own transform,
    index column and z_dir, then rows i + 1 .. N - 1 as they are.  A row that sends the ray back
    over gap g (from interface g + 1 to g) carries the inverse of row g's transform
    (``_set_inverse``), n_table[:, g] unchanged and z_dir = -z_dir[g]; profile, apertures,
    max_aperture and flags are copied.  The object side up to j is untouched, so the nominal
    system's rox_field, vignetting box and aim serve every ghost.  -> :class:`Unfolded`"""
    N = table.n_ifcs
    j, i = int(j), int(i)
    if not 0 < i < j < N - 1:
        raise ValueError(f'unfold: ({j}, {i}) is not a pair with 0 < i < j < {N - 1}')
    for s in range(i + 1, j):
        why = _blocker(table, s)
        if why:
            raise ValueError(f'unfold: ({j}, {i}): {why}')
    Nu = N + 2 * (j - i)
    rows = (abi.Surface * Nu)()
    nt = np.asarray(table.n_table)
    n_table = np.ones((nt.shape[0], Nu))
    source, pass_, reflects, gaps = [], [], [], []

    def put(s, p, back, reflect):
        u = len(source)
        _copy_row(rows[u], table.rows[s])
        g = s - 1 if back else s                 # the gap the ray crosses next
        if back:
            _set_inverse(rows[u], table.rows[g])
            rows[u].z_dir = -table.rows[g].z_dir
        if reflect:
            rows[u].mode = abi.REFLECT
        n_table[:, u] = nt[:, g]
        source.append(s); pass_.append(p); reflects.append(reflect); gaps.append(g)

    for s in range(j):
        put(s, 0, False, False)
    put(j, 0, True, True)
    for s in range(j - 1, i, -1):
        put(s, 1, True, False)
    put(i, 1, False, True)
    for s in range(i + 1, N):
        put(s, 2, False, False)
    assert len(source) == Nu
    stop = table.stop_idx if table.stop_idx is None or table.stop_idx < j else None
    return Unfolded(SurfaceTable(rows, n_table, table.wvls, stop), (j, i), source, pass_, reflects, gaps)


def coating_tables(table, unf, coatings):
    """``coatings`` -- anything analyses.transmission takes, read against the nominal ``table`` --
    as the coating tables of the unfolded table ``unf``: a dict of the keyword arguments
    TraceEngine.surface_thinfilm takes (coat_kind, coat_value, stack_first, layer_thickness,
    layer_index, sub_index).

    A Coating is written outside-first: the outside of a surface is its air side when exactly one
    side is air, else the side the nominal light comes from.  A row crosses (or meets) the layers
    as written when its light arrives from the outside, reversed otherwise -- the flip rule of
    the transmission analysis applied to the unfolded table's own media, so a coating is crossed
    in reverse on the way back.  Transmitting rows take their source's kind and value.  Reflecting
    rows are ROX_COAT_STACK with the source's layers (none without a Coating) and ``sub_index``
    the real index of the medium behind the surface; a fixed (Ts, Tp) becomes ROX_COAT_FIXED
    (1 - Ts, 1 - Tp), 'ideal' reflectance 0."""
    from .analyses import _coating_tables
    N, Nu = table.n_ifcs, unf.table.n_ifcs
    W = len(table.wvls)
    kind0, value0, stacks0 = _coating_tables(table, coatings)
    if kind0 is None:
        kind0, value0 = np.zeros(N, np.int32), np.ones((N, 2))
    nt = np.asarray(table.n_table)

    def air(g):
        return bool((nt[:, g] == 1.0).all())

    kind = np.zeros(Nu, np.int32)
    value = np.ones((Nu, 2))
    first = np.zeros(Nu + 1, np.int32)
    thick, index = [], [[] for _w in range(W)]
    sub = np.zeros((W, Nu, 2))
    sub[:, :, 0] = 1.0
    for u in range(Nu):
        s = int(unf.source[u])
        first[u] = len(thick)
        if not 0 < s < N - 1:
            kind[u], value[u] = kind0[s], value0[s]
            continue
        # the nominal side the light arrives from: gap s - 1 going forward, gap s going back
        came = int(unf.segment_gap[u - 1])
        outside = s - 1 if (air(s - 1) or not air(s)) or table.rows[s].mode == abi.REFLECT else s
        c = stacks0.get(s)
        if c is not None:
            # stacks0 holds the layers in the order the nominal light crosses them
            written = c if outside == s - 1 else c.reversed()
            c = written if came == outside else written.reversed()
        if table.rows[s].mode == abi.REFLECT and c is not None and c.substrate is not None:
            for w, wvl in enumerate(table.wvls):          # a nominal mirror's metal
                v = index_of(c.substrate, wvl)
                sub[w, u] = v.real, v.imag
        if unf.reflects[u]:
            behind = s if came == s - 1 else s - 1
            sub[:, u, 0] = nt[:, behind]
            if kind0[s] == abi.COAT_FIXED:
                kind[u], value[u] = abi.COAT_FIXED, 1.0 - value0[s]
            elif kind0[s] == abi.COAT_IDEAL:
                kind[u], value[u] = abi.COAT_FIXED, 0.0
            else:
                kind[u] = abi.COAT_STACK
        else:
            kind[u], value[u] = kind0[s], value0[s]
        if kind[u] == abi.COAT_STACK and c is not None:
            thick += [d for _m, d in c.layers]
            for w, wvl in enumerate(table.wvls):
                index[w] += list(c.indices(wvl))
    first[Nu] = len(thick)
    if len(thick) > abi.MAX_COAT_LAYERS_TOTAL:
        raise ValueError(f'ghost: coatings: {len(thick)} layers in all, more than {abi.MAX_COAT_LAYERS_TOTAL}')
    idx = np.array(index, dtype=np.complex128).reshape(W, len(thick))
    return dict(coat_kind=kind, coat_value=value, stack_first=first,
                layer_thickness=np.array(thick, dtype=np.float64),
                layer_index=np.ascontiguousarray(np.stack([idx.real, idx.imag], axis=-1)), sub_index=sub)
