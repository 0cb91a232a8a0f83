"""Drop-ins for the list / grid / fan drivers of ``rayoptics.raytr.analyses``.

  trace_list_of_rays <- rayoptics/raytr/analyses.py:458-510   (+ trace_rays_soa, its array form)
  trace_ray_list     <- rayoptics/raytr/analyses.py:437-455
  trace_ray_grid     <- rayoptics/raytr/analyses.py:666-696
  trace_ray_fan      <- rayoptics/raytr/analyses.py:212-230
  eval_fan / trace_fan / focus_fan <- rayoptics/raytr/analyses.py:233-345 (RayFan: dx, dy
                        and OPD of every fan ray in one launch, ROX_OUT_FAN)
  eval_wavefront     <- rayoptics/raytr/analyses.py:699-732 (OPD fused on device)
  trace_wavefront / focus_wavefront <- rayoptics/raytr/analyses.py:735-791 (RayGrid, PSF)
  trace_pupil_coords / focus_pupil_coords <- rayoptics/raytr/analyses.py:545-580 (RayList, RayGeoPSF)
  through_focus      (new) the refocus functions over a range of focus shifts: one trace,
                        K focus planes, per-plane statistics (rox_trace_through_focus)
  through_focus_map  (new) through_focus for every field and wavelength in one launch, with
                        polychromatic statistics, field curvature and the white-light best
                        focus (rox_trace_through_focus_grids)
  through_focus_psf  (new) diffraction through focus: the PSF and Strehl ratio of every plane
                        of a through_focus scan, from the rows in HBM (rox_focus_psf)
  through_focus_mtf  (new) the MTF through focus along image x and y, per field and
                        polychromatic, from the PSFs in HBM (rox_focus_mtf)
  through_focus_gmtf (new) the geometric MTF and line spread through focus along any
                        direction, from the rays in HBM (rox_focus_gmtf)
  relative_illumination (new) radiometric relative illumination from the image-space solid
                        angle of each field's pupil grid (rox_projected_solid_angle)
  image_simulation   (new) a scene through the lens: geometric polychromatic PSFs of a grid of
                        field nodes (rox_weighted_maps), a field-varying blur and the distortion
                        warp (rox_varying_blur, rox_image_warp)
"""
import numpy as np

from . import abi, session
from .coatings import Coating, stack_tables
from .engine import make_grid
from .raypkg import HostPackets
from .trace import opts_from_kwargs, emit, _trace_pupil, _launch_setup


def _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt=None, image_delta=None):
    """trace.setup_pupil_coords (rayoptics/raytr/trace.py:608-624): the reference's
    own for a live model (chief ray cached on the field, reference sphere host
    math); table-backed models bring theirs"""
    own = getattr(opt_model, 'setup_pupil_coords', None)
    if own is not None:
        return own(fld, wvl, foc, image_pt=image_pt, image_delta=image_delta)
    from rayoptics.raytr import trace as ref_trace
    return ref_trace.setup_pupil_coords(opt_model, fld, wvl, foc, image_pt=image_pt,
                                        image_delta=image_delta)


def trace_list_of_rays(opt_model, rays, output_filter=None, rayerr_filter=None,
                       **kwargs):
    """explicit (pt0, dir0, wvl) rays; per-ray wavelengths allowed"""
    rays = list(rays)
    eng = session.engine_for(opt_model)
    tbl = eng.table
    R = len(rays)
    pt0 = np.empty((3, R))
    dir0 = np.empty((3, R))
    wvls = np.empty(R)
    wi = np.empty(R, dtype=np.int32)
    for r, (p, d, w) in enumerate(rays):
        pt0[:, r], dir0[:, r], wvls[r] = p, d, w
        wi[r] = tbl.wvl_index(w)
    # partial packets (rayerr_filter='full') need the FULL layout
    out_mode = (abi.OUT_LAST if output_filter == 'last' and rayerr_filter != 'full'
                else abi.OUT_FULL)
    opts = opts_from_kwargs(tbl.n_ifcs, kwargs, out_mode)
    from .engine import HOST_DIRECT_BYTES
    per_ray = 8 * (abi.SEG_DOUBLES * (tbl.n_ifcs if out_mode == abi.OUT_FULL else 1) + 8)
    if R * per_ray <= HOST_DIRECT_BYTES and hasattr(eng, 'trace_rays_np'):
        host = eng.trace_rays_np(pt0, dir0, wi, opts)       # (small lists: no device-to-host copies)
    else:
        host = eng.trace_rays(pt0, dir0, wi, opts).to_host()
    pk = HostPackets(host, tbl, opts.flags, out_mode, wvls)
    ifcs = opt_model['seq_model'].ifcs
    named = True        # trace.trace() wraps in RayPkg (trace.py:250)
    ray_list = []
    for r, ray in enumerate(rays):
        if pk.status[r] != abi.OK:
            if rayerr_filter == 'full':
                ray_list.append((ray, pk.error(r, ifcs, with_pkg=True, named=False)))
            elif rayerr_filter == 'summary':
                ray_list.append((ray, pk.error(r, ifcs, with_pkg=False)))
            continue
        pkg = pk.pkg(r, named)
        if output_filter is None:
            ray_list.append(pkg)
        elif output_filter == 'last':
            seg, op_delta, wvl = pkg
            ray_list.append((seg[-1], op_delta, wvl))
        else:
            ray_list.append(output_filter(pkg))
    return ray_list


def trace_rays_soa(opt_model, pt0, dir0, wvl, out_mode=abi.OUT_FULL, on_device=False, **kwargs):
    """array form of :func:`trace_list_of_rays` for large batches: ``pt0``,
    ``dir0`` are ``[3, R]`` arrays (numpy or torch), ``wvl`` one wavelength or
    ``R`` of them (nm, members of the spectral region).  No per-ray Python
    objects are created: returns the engine's ``DeviceResult`` (``on_device``)
    or a :class:`~.raypkg.HostPackets`, whose ``pkg(r)`` / ``error(r)`` give the
    reference-shaped view of any single ray on demand."""
    eng = session.engine_for(opt_model)
    tbl = eng.table
    if np.ndim(wvl) == 0:
        wi = tbl.wvl_index(wvl)
    else:
        lut = {w: i for i, w in enumerate(tbl.wvls)}
        wi = np.fromiter((lut[float(w)] for w in wvl), dtype=np.int32, count=len(wvl))
    opts = opts_from_kwargs(tbl.n_ifcs, kwargs, out_mode)
    res = eng.trace_rays(pt0, dir0, wi, opts)
    if on_device:
        return res
    return HostPackets(res.to_host(), tbl, opts.flags, out_mode, wvl)


def trace_ray_list(opt_model, pupil_coords, fld, wvl, foc, append_if_none=False,
                   output_filter=None, rayerr_filter=None, **kwargs):
    kwargs['apply_vignetting'] = kwargs.get('apply_vignetting', True)
    named = kwargs.get('use_named_tuples', False)
    items = pupil_coords if isinstance(pupil_coords, (list, np.ndarray)) else list(pupil_coords)
    if isinstance(items, np.ndarray) and items.ndim == 2 and items.shape[1] >= 2 and items.dtype.kind == 'f':
        pc = items[:, :2].astype(float)
    else:
        pc = np.array([[p[0], p[1]] for p in items], dtype=float).reshape(-1, 2)
    pk = _trace_pupil(opt_model, fld, wvl, kwargs, output_filter, rayerr_filter,
                      pupil_list=(pc[:, 0].copy(), pc[:, 1].copy()))
    ifcs = opt_model['seq_model'].ifcs
    ray_list = []
    # Field.apply_vignetting scales `pupil[:]`: a view for an ndarray (the caller's
    # coordinates change in place), a copy for a list or tuple
    whole = isinstance(items, np.ndarray) and items.ndim == 2 and items.shape[1] >= 2
    if whole:                                   # every row at once
        items[:, 0], items[:, 1] = pk.pupil[0], pk.pupil[1]
    for r, p in enumerate(items):
        if not whole and isinstance(p, np.ndarray):
            p[0], p[1] = pk.pupil[0, r], pk.pupil[1, r]
        pkg, _err = emit(pk, r, output_filter, rayerr_filter, named, ifcs)
        if pkg is not None:
            ray_list.append([p[0], p[1], pkg])
        elif append_if_none:
            ray_list.append([p[0], p[1], None])
    return ray_list


def trace_ray_grid(opt_model, grid_rng, fld, wvl, foc, append_if_none=True,
                   output_filter=None, rayerr_filter=None, **kwargs):
    kwargs['apply_vignetting'] = kwargs.get('apply_vignetting', False)   # :674
    named = kwargs.get('use_named_tuples', False)
    num = grid_rng[2]
    pk = _trace_pupil(opt_model, fld, wvl, kwargs, output_filter, rayerr_filter,
                      grid=make_grid(grid_rng[0], grid_rng[1], num))
    ifcs = opt_model['seq_model'].ifcs
    grid = []
    for i in range(num):
        row = []
        for j in range(num):
            r = i * num + j
            pkg, _err = emit(pk, r, output_filter, rayerr_filter, named, ifcs)
            if pkg is not None:
                row.append([pk.pupil[0, r], pk.pupil[1, r], pkg])
            elif append_if_none:
                row.append([pk.pupil[0, r], pk.pupil[1, r], None])
        grid.append(row)
    return grid


def trace_ray_fan(opt_model, fan_rng, fld, wvl, foc, output_filter=None,
                  rayerr_filter=None, **kwargs):
    kwargs['apply_vignetting'] = kwargs.get('apply_vignetting', True)
    pk = _trace_pupil(opt_model, fld, wvl, kwargs, output_filter, rayerr_filter,
                      grid=make_grid(fan_rng[0], fan_rng[1], fan_rng[2], abi.GRID_FAN))
    ifcs = opt_model['seq_model'].ifcs
    fan = []
    for r in range(fan_rng[2]):
        pkg, _err = emit(pk, r, output_filter, rayerr_filter, True, ifcs)   # :222
        if pkg is not None:
            fan.append([pk.pupil[0, r], pk.pupil[1, r], pkg])
    return fan


def eval_wavefront(opt_model, fld, wvl, foc, image_pt_2d=None, image_delta=None,
                   num_rays=21, value_if_none=np.nan, **kwargs):
    """rayoptics/raytr/analyses.py:699-732: OPD (in waves) over the vignetted
    pupil bounding box.  Chief ray and reference sphere come from the
    reference's own ``setup_pupil_coords``; the num_rays**2 traces *and* their
    ``wave_abr_full_calc`` (rayoptics/raytr/waveabr.py:256-307) run in one
    launch (ROX_OUT_OPD).  Packet filters or an infinite reference sphere take
    the generic route: device trace, reference ``waveabr`` on the lazy views."""
    from .table import wavefront_from_model, UnsupportedModelError
    ref_sphere, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt_2d, image_delta)
    fld.chief_ray = cr_pkg
    fld.ref_sphere = ref_sphere
    oversize = kwargs.get('oversize', 1.)
    vig_bbox = fld.vignetting_bbox(opt_model['osp']['pupil'], oversize=oversize)
    grid_def = [vig_bbox[0], vig_bbox[1], num_rays]
    kwargs['check_apertures'] = kwargs.get('check_apertures', True)
    convert_to_opd = 1 / opt_model.nm_to_sys_units(wvl)
    fused = kwargs.get('output_filter') is None and kwargs.get('rayerr_filter') is None \
        and not kwargs.get('filter_out_phantoms', False)
    wf = None
    if fused:
        try:
            wf = wavefront_from_model(opt_model, fld)
        except UnsupportedModelError:
            fused = False
    if not fused:
        from rayoptics.raytr import waveabr
        fod = opt_model['analysis_results']['parax_data'].fod
        grid = trace_ray_grid(opt_model, grid_def, fld, wvl, foc, **kwargs)
        return np.array([[(px, py, convert_to_opd * waveabr.wave_abr_full_calc(
            fod, fld, wvl, foc, pkg, cr_pkg, ref_sphere)) if pkg is not None
            else (px, py, value_if_none) for px, py, pkg in row] for row in grid])
    kwargs.pop('output_filter', None)
    kwargs.pop('rayerr_filter', None)
    kwargs['apply_vignetting'] = kwargs.get('apply_vignetting', False)     # trace_ray_grid :674
    pk = _trace_pupil(opt_model, fld, wvl, kwargs, None, None,
                      grid=make_grid(grid_def[0], grid_def[1], num_rays),
                      out_mode=abi.OUT_OPD, wf=wf)
    ok = pk.status == abi.OK
    opd = np.where(ok, convert_to_opd * pk.seg[0, 0], value_if_none)
    out = np.stack([pk.pupil[0], pk.pupil[1], opd], axis=1)
    return out.reshape(num_rays, num_rays, 3)


def seq_trace_wavefront(self, fld, wvl, foc, num_rays=32):
    with session.hold(self.opt_model):      # one validation of the model for the whole call
        return _seq_trace_wavefront(self, fld, wvl, foc, num_rays)


def _seq_trace_wavefront(self, fld, wvl, foc, num_rays=32):
    """rayoptics/seq/sequential.py:1087-1114 as a replacement *method* of
    SequentialModel: [x, y, opd] over the unit pupil square, opd in waves
    (``opd / nm_to_sys_units(wvl)``), 0.0 where the ray failed.  The reference
    reaches this through trace.trace_grid with a per-ray ``wave_abr_full_calc``
    callback; here trace and OPD are one ROX_OUT_OPD launch."""
    from .table import wavefront_from_model
    opt_model = self.opt_model
    rs_pkg, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc)
    fld.chief_ray = cr_pkg
    fld.ref_sphere = rs_pkg
    wf = wavefront_from_model(opt_model, fld)
    # trace.trace_grid forces check_apertures (trace.py:583); trace_base's default vignetting
    pk = _trace_pupil(opt_model, fld, wvl, dict(check_apertures=True, apply_vignetting=True),
                      None, None, grid=make_grid((-1., -1.), (1., 1.), num_rays),
                      out_mode=abi.OUT_OPD, wf=wf)
    ok = pk.status == abi.OK
    with np.errstate(invalid='ignore'):
        opd = np.where(ok, pk.seg[0, 0] / opt_model.nm_to_sys_units(wvl), 0.0)
    return np.stack([pk.pupil[0], pk.pupil[1], opd], axis=1).reshape(num_rays, num_rays, 3)


class _DeferredWavefront:
    """what the fused :func:`trace_wavefront` hands to :func:`focus_wavefront`
    in place of a grid of ray packets: the grid definition and trace options.
    The trace does not depend on the focus, so re-evaluating trace + OPD on the
    device for every refocus gives what the reference's pre-calc / refocus split
    gives (same formulas, same operation order, waveabr.py:309-353)."""

    def __init__(self, grid_def, kwargs, ctx=None):
        self.grid_def = grid_def
        self.kwargs = kwargs
        self._ctx = ctx             # (opt_model, fld, wvl, foc) for consumers of the grid itself
        self._grid = None

    # any other consumer of RayGrid.grid_pkg[0] sees the reference's grid of
    # [px, py, ray_pkg] rows, traced on first use (FULL packets)
    def _materialise(self):
        if self._grid is None:
            opt_model, fld, wvl, foc = self._ctx
            self._grid = trace_ray_grid(opt_model, self.grid_def, fld, wvl, foc,
                                        **dict(self.kwargs))
        return self._grid

    def __iter__(self):
        return iter(self._materialise())

    def __len__(self):
        return len(self._materialise())

    def __getitem__(self, i):
        return self._materialise()[i]


class _DeferredPreCalc:
    """the second half of the reference's trace_wavefront result (the
    wave_abr_pre_calc grid, rayoptics/raytr/analyses.py:755-764), computed from the
    materialised packets only if a consumer other than focus_wavefront asks"""

    def __init__(self, deferred, cr_pkg, ref_sphere):
        self._d, self._cr, self._rs, self._upd = deferred, cr_pkg, ref_sphere, None

    def _materialise(self):
        if self._upd is None:
            from rayoptics.raytr import waveabr
            opt_model, fld, wvl, foc = self._d._ctx
            fod = opt_model['analysis_results']['parax_data'].fod
            self._upd = [[waveabr.wave_abr_pre_calc(fod, fld, wvl, foc, pkg, self._cr, self._rs)
                          if pkg is not None else None for _px, _py, pkg in row]
                         for row in self._d._materialise()]
        return self._upd

    def __iter__(self):
        return iter(self._materialise())

    def __len__(self):
        return len(self._materialise())

    def __getitem__(self, i):
        return self._materialise()[i]


def _opd_fusable(kwargs):
    return (kwargs.get('output_filter') is None and kwargs.get('rayerr_filter') is None
            and not kwargs.get('filter_out_phantoms', False))


def _opd_grid(opt_model, fld, wvl, grid_def, kwargs, wf, value_if_none):
    kw = dict(kwargs)
    for k in ('output_filter', 'rayerr_filter', 'oversize'):
        kw.pop(k, None)
    kw['apply_vignetting'] = kw.get('apply_vignetting', False)      # trace_ray_grid :674
    num = grid_def[2]
    pk = _trace_pupil(opt_model, fld, wvl, kw, None, None,
                      grid=make_grid(grid_def[0], grid_def[1], num),
                      out_mode=abi.OUT_OPD, wf=wf)
    convert_to_opd = 1 / opt_model.nm_to_sys_units(wvl)
    ok = pk.status == abi.OK
    opd = np.where(ok, convert_to_opd * pk.seg[0, 0], value_if_none)
    return np.stack([pk.pupil[0], pk.pupil[1], opd], axis=1).reshape(num, num, 3)


def trace_wavefront(opt_model, fld, wvl, foc, image_pt_2d=None, image_delta=None,
                    num_rays=21, **kwargs):
    """rayoptics/raytr/analyses.py:735-766"""
    from .table import wavefront_from_model, UnsupportedModelError
    ref_sphere, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt_2d, image_delta)
    fld.chief_ray = cr_pkg
    fld.ref_sphere = ref_sphere
    oversize = kwargs.get('oversize', 1.)
    vig_bbox = fld.vignetting_bbox(opt_model['osp']['pupil'], oversize=oversize)
    grid_def = [vig_bbox[0], vig_bbox[1], num_rays]
    kwargs['check_apertures'] = kwargs.get('check_apertures', True)
    if _opd_fusable(kwargs):
        try:
            wavefront_from_model(opt_model, fld)         # finite reference sphere?
            d = _DeferredWavefront(grid_def, dict(kwargs), (opt_model, fld, wvl, foc))
            return d, _DeferredPreCalc(d, cr_pkg, ref_sphere)
        except UnsupportedModelError:
            pass
    from rayoptics.raytr import waveabr
    fod = opt_model['analysis_results']['parax_data'].fod
    grid = trace_ray_grid(opt_model, grid_def, fld, wvl, foc, **kwargs)
    upd_grid = [[waveabr.wave_abr_pre_calc(fod, fld, wvl, foc, pkg, cr_pkg, ref_sphere)
                 if pkg is not None else None for _px, _py, pkg in row] for row in grid]
    return grid, upd_grid


def focus_wavefront(opt_model, grid_pkg, fld, wvl, foc, image_pt_2d=None,
                    image_delta=None, value_if_none=np.nan, **kwargs):
    """rayoptics/raytr/analyses.py:769-791"""
    from .table import wavefront_from_model, UnsupportedModelError
    grid, upd_grid = grid_pkg
    ref_sphere, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt_2d, image_delta)
    if isinstance(grid, _DeferredWavefront):
        try:
            own = getattr(fld, 'rox_wavefront', None)   # table-backed models: prebuilt
            wf = own if own is not None else wavefront_from_model(opt_model, fld, cr_pkg, ref_sphere)
            if wf.kind == abi.WF_INF_FULL:
                # RayGrid's route is wave_abr_pre_calc + wave_abr_calc (waveabr.py:427-488):
                # on an infinite reference sphere the final sum is associated differently
                # from wave_abr_full_calc_inf_ref's
                wf = abi.Wavefront.from_buffer_copy(bytes(wf))
                wf.kind = abi.WF_INF_SPLIT
            return _opd_grid(opt_model, fld, wvl, grid.grid_def, grid.kwargs, wf, value_if_none)
        except UnsupportedModelError:       # the sphere went infinite at this focus
            from rayoptics.raytr import waveabr
            fod = opt_model['analysis_results']['parax_data'].fod
            g = trace_ray_grid(opt_model, grid.grid_def, fld, wvl, foc, **dict(grid.kwargs))
            return np.array([[(px, py, waveabr.wave_abr_full_calc(fod, fld, wvl, foc, pkg, cr_pkg,
                                                                  ref_sphere)
                               / opt_model.nm_to_sys_units(wvl)) if pkg is not None
                              else (px, py, value_if_none) for px, py, pkg in row] for row in g])
    from rayoptics.raytr import waveabr
    fod = opt_model['analysis_results']['parax_data'].fod
    convert_to_opd = 1 / opt_model.nm_to_sys_units(wvl)
    return np.array([[(g[0], g[1], convert_to_opd * waveabr.wave_abr_calc(
        fod, fld, wvl, foc, g[2], cr_pkg, u, ref_sphere)) if g[2] is not None
        else (g[0], g[1], value_if_none) for g, u in zip(ig, iu)] for ig, iu in zip(grid, upd_grid)])


class _DeferredRayList:
    """what the fused :func:`trace_pupil_coords` hands to
    :func:`focus_pupil_coords`: the pupil coordinates and trace options.  It
    still behaves as the reference's list of ``[px, py, ray_pkg]`` entries for
    any other consumer (materialised by a FULL device trace on first use)."""

    def __init__(self, opt_model, pupil_coords, fld, wvl, foc, kwargs):
        self.opt_model, self.fld, self.wvl, self.foc = opt_model, fld, wvl, foc
        self.pupil = np.array([[p[0], p[1]] for p in pupil_coords], dtype=float).reshape(-1, 2)
        self.kwargs = kwargs
        self._list = None

    def _materialise(self):
        if self._list is None:
            self._list = trace_ray_list(self.opt_model, [p.copy() for p in self.pupil],
                                        self.fld, self.wvl, self.foc, **dict(self.kwargs))
        return self._list

    def __iter__(self):
        return iter(self._materialise())

    def __len__(self):
        return len(self._materialise())

    def __getitem__(self, i):
        return self._materialise()[i]


def trace_pupil_coords(opt_model, pupil_coords, fld, wvl, foc,
                       image_pt_2d=None, image_delta=None, **kwargs):
    """rayoptics/raytr/analyses.py:545-558"""
    ref_sphere, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt_2d, image_delta)
    fld.chief_ray = cr_pkg
    fld.ref_sphere = ref_sphere
    kwargs['check_apertures'] = kwargs.get('check_apertures', True)
    if _opd_fusable(kwargs) and not kwargs.get('append_if_none', False):
        return _DeferredRayList(opt_model, pupil_coords, fld, wvl, foc, dict(kwargs))
    return trace_ray_list(opt_model, pupil_coords, fld, wvl, foc, **kwargs)


def focus_pupil_coords(opt_model, ray_list, fld, wvl, foc,
                       image_pt_2d=None, image_delta=None, **kwargs):
    """rayoptics/raytr/analyses.py:561-580: transverse aberrations of
    pre-traced rays at a (new) focus.  For the deferred list this is one HITS
    launch over the pupil coordinates (the trace does not depend on focus)."""
    ref_sphere, _cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt_2d, image_delta)
    image_pt = ref_sphere[0]
    if isinstance(ray_list, _DeferredRayList):
        kw = dict(ray_list.kwargs)
        for k in ('output_filter', 'rayerr_filter', 'append_if_none'):
            kw.pop(k, None)
        kw['apply_vignetting'] = kw.get('apply_vignetting', True)
        eng, f, wi, opts = _launch_setup(opt_model, fld, wvl, kw, abi.OUT_HITS_COMPACT,
                                         foc, image_pt[:2])
        return eng.trace_pupil_list_hits(f, ray_list.pupil[:, 0].copy(),
                                         ray_list.pupil[:, 1].copy(), wi, opts)
    data = []
    for _px, _py, pkg in ray_list:
        if pkg is not None:
            seg = pkg[0][-1]
            dist = foc / seg[1][2]
            t_abr = (seg[0] + dist * seg[1]) - image_pt
            data.append((t_abr[0], t_abr[1]))
        else:
            data.append(np.nan)
    return np.array(data)


# ---- RayFan ------------------------------------------------------------------
def _fan_def(xy, num_rays):
    fan_start = np.array([0., 0.])
    fan_stop = np.array([0., 0.])
    fan_start[xy] = -1.0
    fan_stop[xy] = 1.0
    return [fan_start, fan_stop, num_rays]


def _fan_data(opt_model, fld, wvl, foc, fan_def, kwargs, wf, image_pt):
    """one ROX_OUT_FAN launch -> the reference's fan_data list: ((px, py), (dx, dy, opd))
    for every ray that gets through (trace_ray_fan drops the others, analyses.py:212-230)"""
    kw = dict(kwargs)
    for k in ('output_filter', 'rayerr_filter'):
        kw.pop(k, None)
    kw['apply_vignetting'] = kw.get('apply_vignetting', True)
    pk = _trace_pupil(opt_model, fld, wvl, kw, None, None,
                      grid=make_grid(fan_def[0], fan_def[1], fan_def[2], abi.GRID_FAN),
                      out_mode=abi.OUT_FAN, foc=foc, image_pt=image_pt[:2], wf=wf)
    convert_to_opd = 1 / opt_model.nm_to_sys_units(wvl)
    seg = pk.seg[0]
    return [((pk.pupil[0, r], pk.pupil[1, r]), (seg[0, r], seg[1, r], convert_to_opd * seg[2, r]))
            for r in range(fan_def[2]) if pk.status[r] == abi.OK]


def eval_fan(opt_model, fld, wvl, foc, xy, image_pt_2d=None, image_delta=None, num_rays=21,
             output_filter=None, rayerr_filter=None, **kwargs):
    """rayoptics/raytr/analyses.py:233-274: dx, dy and OPD across a fan"""
    from .table import wavefront_from_model
    ref_sphere, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt_2d, image_delta)
    fld.chief_ray = cr_pkg
    fld.ref_sphere = ref_sphere
    fan_def = _fan_def(xy, num_rays)
    if output_filter is None and rayerr_filter is None and not kwargs.get('filter_out_phantoms', False):
        wf = wavefront_from_model(opt_model, fld)
        return _fan_data(opt_model, fld, wvl, foc, fan_def, kwargs, wf, ref_sphere[0])
    from rayoptics.raytr import waveabr
    fod = opt_model['analysis_results']['parax_data'].fod
    fan = trace_ray_fan(opt_model, fan_def, fld, wvl, foc, output_filter=output_filter,
                        rayerr_filter=rayerr_filter, **kwargs)
    convert_to_opd = 1 / opt_model.nm_to_sys_units(wvl)
    out = []
    for px, py, pkg in fan:
        if pkg is not None:
            seg = pkg[0][-1]
            t_abr = (seg[0] + (foc / seg[1][2]) * seg[1]) - ref_sphere[0]
            opd = convert_to_opd * waveabr.wave_abr_full_calc(fod, fld, wvl, foc, pkg, cr_pkg, ref_sphere)
            out.append(((px, py), (t_abr[0], t_abr[1], opd)))
        else:
            out.append((px, py, np.nan))
    return out


class _DeferredFan(_DeferredWavefront):
    """what the fused :func:`trace_fan` hands to :func:`focus_fan`: the fan
    definition and trace options (a fan of [px, py, ray_pkg] for anyone else)"""

    def _materialise(self):
        if self._grid is None:
            opt_model, fld, wvl, foc = self._ctx
            kw = dict(self.kwargs)
            self._grid = trace_ray_fan(opt_model, self.grid_def, fld, wvl, foc, **kw)
        return self._grid


class _DeferredFanPreCalc(_DeferredPreCalc):
    def _materialise(self):
        if self._upd is None:
            from rayoptics.raytr import waveabr
            opt_model, fld, wvl, foc = self._d._ctx
            fod = opt_model['analysis_results']['parax_data'].fod
            self._upd = [waveabr.wave_abr_pre_calc(fod, fld, wvl, foc, pkg, self._cr, self._rs)
                         if pkg is not None else None for _px, _py, pkg in self._d._materialise()]
        return self._upd


def trace_fan(opt_model, fld, wvl, foc, xy, image_pt_2d=None, image_delta=None, num_rays=21,
              output_filter=None, rayerr_filter=None, **kwargs):
    """rayoptics/raytr/analyses.py:277-314"""
    ref_sphere, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt_2d, image_delta)
    fld.chief_ray = cr_pkg
    fld.ref_sphere = ref_sphere
    fan_def = _fan_def(xy, num_rays)
    if output_filter is None and rayerr_filter is None and not kwargs.get('filter_out_phantoms', False):
        d = _DeferredFan(fan_def, dict(kwargs), (opt_model, fld, wvl, foc))
        return d, _DeferredFanPreCalc(d, cr_pkg, ref_sphere)
    from rayoptics.raytr import waveabr
    from rayoptics.raytr import traceerror as terr
    fod = opt_model['analysis_results']['parax_data'].fod
    fan = trace_ray_fan(opt_model, fan_def, fld, wvl, foc, output_filter=output_filter,
                        rayerr_filter=rayerr_filter, **kwargs)
    upd_fan = [waveabr.wave_abr_pre_calc(fod, fld, wvl, foc, pkg, cr_pkg, ref_sphere)
               if pkg is not None and not isinstance(pkg, terr.TraceError) else None
               for _px, _py, pkg in fan]
    return fan, upd_fan


def focus_fan(opt_model, fan_pkg, fld, wvl, foc, image_pt_2d=None, image_delta=None, **kwargs):
    """rayoptics/raytr/analyses.py:317-345"""
    from .table import wavefront_from_model
    fan, upd_fan = fan_pkg
    ref_sphere, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt_2d, image_delta)
    if isinstance(fan, _DeferredFan):
        own = getattr(fld, 'rox_wavefront', None)
        wf = own if own is not None else wavefront_from_model(opt_model, fld, cr_pkg, ref_sphere)
        if wf.kind == abi.WF_INF_FULL:          # the pre-calc / calc split, as in focus_wavefront
            wf = abi.Wavefront.from_buffer_copy(bytes(wf))
            wf.kind = abi.WF_INF_SPLIT
        return _fan_data(opt_model, fld, wvl, foc, fan.grid_def, fan.kwargs, wf, ref_sphere[0])
    from rayoptics.raytr import waveabr
    from rayoptics.raytr import traceerror as terr
    fod = opt_model['analysis_results']['parax_data'].fod
    convert_to_opd = 1 / opt_model.nm_to_sys_units(wvl)
    out = []
    for (px, py, pkg), fiu in zip(fan, upd_fan):
        if pkg is not None and not isinstance(pkg, terr.TraceError):
            seg = pkg[0][-1]
            t_abr = (seg[0] + (foc / seg[1][2]) * seg[1]) - ref_sphere[0]
            opd = convert_to_opd * waveabr.wave_abr_calc(fod, fld, wvl, foc, pkg, cr_pkg, fiu, ref_sphere)
            out.append(((px, py), (t_abr[0], t_abr[1], opd)))
        else:
            out.append((px, py, np.nan))
    return out


# ---- through focus -----------------------------------------------------------------
def best_focus(focs, values):
    """the focus at which a sampled curve is least: the vertex of the parabola through the
    sampled minimum and its two neighbours -> (focus, 'vertex'); the end sample when the
    minimum is the first or last sample -> (focus, 'end').  (The first minimum's parabola always
    opens upwards; 'sample' -- the sample itself -- guards the degenerate arithmetic.)  NaN
    samples (planes no ray reached) are skipped; none left -> (nan, 'none')."""
    f = np.asarray(focs, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64)
    ok = ~np.isnan(v)
    if not ok.any():
        return float('nan'), 'none'
    f, v = f[ok], v[ok]
    i = int(np.argmin(v))
    if i == 0 or i == len(v) - 1:
        return float(f[i]), 'end'
    (x0, x1, x2), (y0, y1, y2) = f[i - 1:i + 2], v[i - 1:i + 2]
    # divided differences: y = y1 + b (x - x1) + c (x - x1)(x - x0)
    d01, d12 = (y1 - y0) / (x1 - x0), (y2 - y1) / (x2 - x1)
    c = (d12 - d01) / (x2 - x0)
    if not c > 0:
        return float(f[i]), 'sample'
    return float(0.5 * (x0 + x1) - 0.5 * d01 / c), 'vertex'


class ThroughFocus:
    """what :func:`through_focus` returns.

    focs       the focus shifts, as given
    stats      NumPy structured array [K] (engine.FOCUS_STATS_DTYPE): n, centroid (cx, cy),
               rms_spot (about the centroid), rms_spot_image_pt, and the OPD's mean, rms about
               the mean, min and max -- OPD in waves, converted as focus_fan converts
    rows       [K, 3, R] (x abr, y abr, OPD in waves) per ray and plane, NaN where a ray
               failed; ``status`` [R] -- with ``rows=True`` only, else None
    best_focus_spot / best_focus_wavefront (+ ``_kind``): :func:`best_focus` of the RMS
               spot radius / of the RMS wavefront error"""

    def __init__(self, focs, stats, rows, status):
        self.focs = np.asarray(focs, dtype=np.float64)
        self.stats = stats
        self.rows = rows
        self.status = status
        self.best_focus_spot, self.best_focus_spot_kind = best_focus(self.focs, stats['rms_spot'])
        self.best_focus_wavefront, self.best_focus_wavefront_kind = best_focus(self.focs,
                                                                               stats['opd_rms'])

    @property
    def rms_spot(self):
        return self.stats['rms_spot']

    @property
    def rms_wavefront(self):
        return self.stats['opd_rms']


def _check_focs(focs, what):
    focs = [float(f) for f in np.atleast_1d(focs)]
    if not 1 <= len(focs) <= abi.MAX_FOCUS_PLANES:
        raise ValueError(f'{what}: 1 to {abi.MAX_FOCUS_PLANES} focus values, got {len(focs)}')
    return focs


def _focus_planes(opt_model, fld, wvl, focs, image_pt_2d=None, image_delta=None, radii=None):
    """the rox_focus_plane of every focus shift, each built as focus_wavefront / focus_fan build
    their one focus (rayoptics/raytr/analyses.py:313-342, 769-791): setup_pupil_coords at that
    foc, its reference sphere as rox_wavefront (the pre-calc / calc split on an infinite sphere,
    :352-357).  The field keeps the last focus's chief ray and reference sphere.  ``radii``, a
    list, receives each focus's reference-sphere radius ref_sphere[2]."""
    from .table import wavefront_from_model
    planes = []
    for foc in focs:
        ref_sphere, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, foc, image_pt_2d, image_delta)
        if radii is not None:
            radii.append(ref_sphere[2])
        own = getattr(fld, 'rox_wavefront', None)       # table-backed models: prebuilt
        wf = own if own is not None else wavefront_from_model(opt_model, fld, cr_pkg, ref_sphere)
        wf = abi.Wavefront.from_buffer_copy(bytes(wf))
        if wf.kind == abi.WF_INF_FULL:                  # as focus_wavefront / focus_fan
            wf.kind = abi.WF_INF_SPLIT
        p = abi.FocusPlane()
        p.foc = foc
        p.image_pt[0], p.image_pt[1] = float(ref_sphere[0][0]), float(ref_sphere[0][1])
        p.wf = wf
        planes.append(p)
    fld.chief_ray, fld.ref_sphere = cr_pkg, ref_sphere
    return planes


def _focus_grid(opt_model, fld, xy, num_rays, kw):
    """the pupil grid of a scan (and its trace options into ``kw``): ``xy=None`` the square grid
    trace_wavefront traces (:735-766), ``xy=0`` / ``1`` trace_fan's fan (:277-314)"""
    for k in ('output_filter', 'rayerr_filter'):
        kw.pop(k, None)
    if xy is None:
        oversize = kw.pop('oversize', 1.)
        vig_bbox = fld.vignetting_bbox(opt_model['osp']['pupil'], oversize=oversize)
        kw['check_apertures'] = kw.get('check_apertures', True)
        kw['apply_vignetting'] = kw.get('apply_vignetting', False)
        return make_grid(vig_bbox[0], vig_bbox[1], num_rays)
    fan_def = _fan_def(xy, num_rays)
    kw['apply_vignetting'] = kw.get('apply_vignetting', True)
    return make_grid(fan_def[0], fan_def[1], fan_def[2], abi.GRID_FAN)


def _stats_in_waves(stats, opt_model, wvl):
    """the device statistics with the OPD in waves, converted as focus_fan converts"""
    convert_to_opd = 1 / opt_model.nm_to_sys_units(wvl)
    stats = stats.copy()
    for k in ('opd_mean', 'opd_rms', 'opd_min', 'opd_max'):
        stats[k] = convert_to_opd * stats[k]
    return stats


def through_focus(opt_model, fld, wvl, focs, num_rays=21, xy=None, image_pt_2d=None,
                  image_delta=None, rows=False, **kwargs):
    """A through-focus scan on the device: the pupil grid is traced once and evaluated at
    every focus shift in ``focs`` (rox_trace_through_focus).  Each plane is built exactly as
    focus_wavefront / focus_fan build their one focus (rayoptics/raytr/analyses.py:313-342,
    769-791): setup_pupil_coords at that foc, its reference sphere as rox_wavefront (the
    pre-calc / calc split on an infinite sphere, :352-357).  ``xy=None`` traces the square
    pupil grid trace_wavefront does (the field's vignetting box, apertures checked), ``xy=0``
    / ``1`` the fan trace_fan does.  A focus whose reference sphere the device cannot express
    raises UnsupportedModelError for the whole call."""
    from .engine import grid_rays
    focs = _check_focs(focs, 'through_focus')
    planes = _focus_planes(opt_model, fld, wvl, focs, image_pt_2d, image_delta)
    kw = dict(kwargs)
    grid = _focus_grid(opt_model, fld, xy, num_rays, kw)
    eng, f, wi, opts = _launch_setup(opt_model, fld, wvl, kw, abi.OUT_FAN)
    out = eng.trace_pupil_grid_focus(f, grid, wi, opts, planes, want_rows=rows)
    stats, dev_rows = out if rows else (out, None)
    stats = _stats_in_waves(stats, opt_model, wvl)
    host_rows = status = None
    if dev_rows is not None:
        convert_to_opd = 1 / opt_model.nm_to_sys_units(wvl)
        host_rows, status = dev_rows.to_host()
        host_rows = np.array(host_rows[:, :, :grid_rays(grid)])
        host_rows[:, 2] = convert_to_opd * host_rows[:, 2]
    return ThroughFocus(focs, stats, host_rows, status)


class ThroughFocusPSF:
    """what :func:`through_focus_psf` returns.

    focs       the focus shifts, as given
    stats      [K] engine.FOCUS_STATS_DTYPE: the geometric statistics, as :func:`through_focus`
               returns them
    n          [K] rays with status OK on each plane's grid
    strehl     [K] |sum_ok exp(i 2 pi W)|^2 / n^2 of each plane's OPD W in waves (NaN: no ray)
    psf_peak   [K] the maximum of |FFT|^2 each PSF was normalised by (calc_psf's AP_max)
    psf        [K, maxdim, maxdim] each plane's calc_psf -- NumPy, a torch tensor in HBM with
               ``on_device=True``, or None with ``psf=False``
    best_focus_strehl (+ ``_kind``): :func:`best_focus` of -strehl -- the diffraction focus
    delta_x / delta_xp [K]: calc_psf_scaling (rayoptics/raytr/analyses.py:818-845) at each focus,
               with that focus's reference-sphere radius; None without paraxial data"""

    def __init__(self, focs, stats, psf_stats, psf, delta_x=None, delta_xp=None):
        self.focs = np.asarray(focs, dtype=np.float64)
        self.stats = stats
        self.n = psf_stats['n'].copy()
        self.strehl = psf_stats['strehl'].copy()
        self.psf_peak = psf_stats['psf_peak'].copy()
        self.psf = psf
        self.delta_x = delta_x
        self.delta_xp = delta_xp
        self.best_focus_strehl, self.best_focus_strehl_kind = best_focus(self.focs, -self.strehl)


def _psf_block_fits(ndim, maxdim):
    """calc_psf's slice assignment (analyses.py:861-863) has a matching shape only for an even
    ndim whose block fits inside maxdim (the rox_calc_psf / rox_focus_psf rules)"""
    o = maxdim // 2 - (ndim // 2 - 1)
    return ndim >= 2 and ndim % 2 == 0 and maxdim >= 2 and o >= 0 and o + ndim <= maxdim and maxdim <= 32768


def psf_scaling(opt_model, wvl, ndim, maxdim, ref_sphere_radius):
    """calc_psf_scaling (rayoptics/raytr/analyses.py:818-845), the same arithmetic, with the
    reference-sphere radius given -> (delta_x, delta_xp); None for a model without paraxial data
    (a workloads.TableModel has no 'analysis_results')"""
    try:
        results = opt_model['analysis_results']
    except KeyError:
        return None
    fod = results['parax_data'].fod
    wl = opt_model.nm_to_sys_units(wvl)
    fill_factor = ndim/maxdim
    max_D = 2 * fod.enp_radius / fill_factor
    delta_x = max_D / maxdim
    C = wl/fod.exp_radius
    delta_theta = (fill_factor * C) / 2
    delta_xp = delta_theta * ref_sphere_radius
    return delta_x, delta_xp


def through_focus_psf(opt_model, fld, wvl, focs, num_rays=32, maxdim=128, image_pt_2d=None,
                      image_delta=None, psf=True, on_device=False, **kwargs):
    """Diffraction through focus on the device: the square pupil grid trace_wavefront traces is
    traced once and evaluated at every focus shift (as :func:`through_focus` with ``xy=None``),
    and each plane's OPD grid -- what focus_wavefront returns at that focus
    (rayoptics/raytr/analyses.py:769-791) -- goes through calc_psf (:848-875) and a Strehl ratio
    without leaving HBM (rox_focus_psf).  Returns a :class:`ThroughFocusPSF`; the diffraction
    best focus is the peak of the Strehl curve."""
    from .engine import grid_rays
    focs = _check_focs(focs, 'through_focus_psf')
    num_rays, maxdim = int(num_rays), int(maxdim)
    if num_rays < 2 or num_rays % 2:
        raise ValueError(f'through_focus_psf: num_rays must be even and >= 2, got {num_rays}')
    if not _psf_block_fits(num_rays, maxdim):
        raise ValueError(f'through_focus_psf: the {num_rays} x {num_rays} grid does not fit in maxdim {maxdim}')
    radii = []
    planes = _focus_planes(opt_model, fld, wvl, focs, image_pt_2d, image_delta, radii=radii)
    kw = dict(kwargs)
    grid = _focus_grid(opt_model, fld, None, num_rays, kw)
    assert grid_rays(grid) == num_rays * num_rays
    eng, f, wi, opts = _launch_setup(opt_model, fld, wvl, kw, abi.OUT_FAN)
    stats, dev_rows = eng.trace_pupil_grid_focus(f, grid, wi, opts, planes, want_rows=True, want_stats=True)
    convert_to_opd = 1 / opt_model.nm_to_sys_units(wvl)
    dev_psf, psf_stats = eng.focus_psf(dev_rows, num_rays, maxdim, convert_to_opd, want_psf=psf)
    out_psf = None
    if dev_psf is not None:
        out_psf = dev_psf[0] if on_device else dev_psf[0].cpu().numpy()
    delta_x = delta_xp = None
    scal = [psf_scaling(opt_model, wvl, num_rays, maxdim, r) for r in radii]
    if all(s is not None for s in scal):
        delta_x = np.array([s[0] for s in scal])
        delta_xp = np.array([s[1] for s in scal])
    return ThroughFocusPSF(focs, _stats_in_waves(stats, opt_model, wvl), psf_stats[0], out_psf,
                           delta_x, delta_xp)


# polychromatic statistics per field and plane (through_focus_map): the weighted ray count,
# the weighted centroid in image coordinates, the RMS spot radius about it and about the
# reference wavelength's image point, and the RMS wavefront error (each wavelength about its own
# mean, in its own waves)
POLY_STATS_DTYPE = np.dtype([('n', np.float64), ('cx', np.float64), ('cy', np.float64),
                             ('rms_spot', np.float64), ('rms_spot_ref_pt', np.float64),
                             ('rms_wavefront', np.float64)])


def poly_merge(stats, image_pts, spectral_wts, ref_index):
    """the polychromatic statistics [K] of one field from its per-wavelength records.

    stats       [W, K] FOCUS_STATS_DTYPE, OPD in waves of each wavelength
    image_pts   [W, K, 2] each plane's image point (ref_sphere[0][:2] at that wavelength)
    spectral_wts  [W] weights s_w
    ref_index   the wavelength whose image point rms_spot_ref_pt is measured about

    With c_w = image_pt_w + (cx, cy) and M2_w = n_w rms_spot_w^2 (positions in absolute image
    coordinates, so lateral colour counts -- as the reference's spot diagram measures every
    wavelength against the central wavelength's image point, rayoptics/seq/sequential.py:1058-1085):
    N = sum s_w n_w, C = sum s_w n_w c_w / N, rms_spot = sqrt(sum s_w (M2_w + n_w |c_w - C|^2) / N),
    rms_spot_ref_pt the same about the reference image point, rms_wavefront =
    sqrt(sum s_w n_w opd_rms_w^2 / N).  Records with n = 0 are skipped; none left -> NaN."""
    stats = np.asarray(stats)
    W, K = stats.shape
    ip = np.asarray(image_pts, dtype=np.float64).reshape(W, K, 2)
    s = np.asarray(spectral_wts, dtype=np.float64).reshape(W, 1)
    n = stats['n'].astype(np.float64)
    use = n > 0
    sn = np.where(use, s * n, 0.0)
    c = ip + np.stack([stats['cx'], stats['cy']], axis=-1)
    c = np.where(use[..., None], c, 0.0)
    m2 = np.where(use, n * np.where(use, stats['rms_spot'], 0.0) ** 2, 0.0)
    w2 = np.where(use, np.where(use, stats['opd_rms'], 0.0) ** 2, 0.0)
    N = sn.sum(axis=0)
    out = np.full(K, np.nan, dtype=POLY_STATS_DTYPE)
    out['n'] = N
    ok = N > 0
    with np.errstate(invalid='ignore', divide='ignore'):
        C = (sn[..., None] * c).sum(axis=0) / N[:, None]
        d2 = ((c - C[None]) ** 2).sum(axis=-1)
        d2r = ((c - ip[ref_index][None]) ** 2).sum(axis=-1)
        sm2 = np.where(use, s * m2, 0.0)
        out['cx'] = np.where(ok, C[:, 0], np.nan)
        out['cy'] = np.where(ok, C[:, 1], np.nan)
        out['rms_spot'] = np.where(ok, np.sqrt((sm2 + sn * d2).sum(axis=0) / N), np.nan)
        out['rms_spot_ref_pt'] = np.where(ok, np.sqrt((sm2 + sn * d2r).sum(axis=0) / N), np.nan)
        out['rms_wavefront'] = np.where(ok, np.sqrt((sn * w2).sum(axis=0) / N), np.nan)
    return out


class ThroughFocusMap:
    """what :func:`through_focus_map` returns.

    focs, wvls, field_wts, spectral_wts, ref_wvl   as used
    stats       [F, W, K] FOCUS_STATS_DTYPE, each [f, w] what through_focus(flds[f], wvls[w])
                returns (OPD in waves of that wavelength)
    image_pts   [F, W, K, 2] each plane's image point
    rows        [F, W, K, 3, R] and ``status`` [F, W, R] with ``rows=True``, else None
    best_focus_spot / best_focus_wavefront [F, W] (+ ``_kind``): :func:`best_focus` per curve
    poly        [F, K] POLY_STATS_DTYPE: :func:`poly_merge` of each field's wavelengths
    best_focus_field [F] (+ ``_kind``): the best focus of each field's polychromatic RMS spot --
                the through-focus field curvature
    best_focus (+ ``_kind``): the best focus of the field-weighted mean polychromatic RMS spot"""

    def __init__(self, focs, wvls, field_wts, spectral_wts, ref_wvl, stats, image_pts, rows, status):
        self.focs = np.asarray(focs, dtype=np.float64)
        self.wvls = list(wvls)
        self.field_wts = np.asarray(field_wts, dtype=np.float64)
        self.spectral_wts = np.asarray(spectral_wts, dtype=np.float64)
        self.ref_wvl = ref_wvl
        self.stats = stats
        self.image_pts = image_pts
        self.rows = rows
        self.status = status
        F, W, _K = stats.shape
        self.best_focus_spot = np.empty((F, W))
        self.best_focus_wavefront = np.empty((F, W))
        self.best_focus_spot_kind = np.empty((F, W), dtype=object)
        self.best_focus_wavefront_kind = np.empty((F, W), dtype=object)
        for f in range(F):
            for w in range(W):
                self.best_focus_spot[f, w], self.best_focus_spot_kind[f, w] = best_focus(
                    self.focs, stats[f, w]['rms_spot'])
                self.best_focus_wavefront[f, w], self.best_focus_wavefront_kind[f, w] = best_focus(
                    self.focs, stats[f, w]['opd_rms'])
        ref = self.wvls.index(ref_wvl)
        self.poly = np.stack([poly_merge(stats[f], image_pts[f], self.spectral_wts, ref) for f in range(F)])
        self.best_focus_field, self.best_focus_field_kind = field_best_focus(self.focs, self.poly['rms_spot'])
        self.best_focus, self.best_focus_kind = overall_best_focus(self.focs, self.poly['rms_spot'],
                                                                   self.field_wts)


def field_best_focus(focs, curves):
    """:func:`best_focus` of each field's curve [F, K] -> (focus [F], kind [F])"""
    res = [best_focus(focs, c) for c in np.asarray(curves, dtype=np.float64)]
    return np.array([r[0] for r in res]), np.array([r[1] for r in res], dtype=object)


def overall_best_focus(focs, curves, field_wts):
    """:func:`best_focus` of sum_f wt_f curves[f] / sum_f wt_f"""
    wt = np.asarray(field_wts, dtype=np.float64)
    return best_focus(focs, (wt[:, None] * np.asarray(curves, dtype=np.float64)).sum(axis=0) / wt.sum())


def _map_spec(opt_model, flds, wvls, field_wts, spectral_wts, ref_wvl, what):
    """the fields, wavelengths and weights of a map: defaults from osp (the fields of osp['fov']
    with their ``wt``, the wavelengths of osp['wvls'] with its spectral_wts, ref_wvl = its
    central_wvl), checked -> (flds, wvls, field_wts, spectral_wts, ref_wvl)"""
    osp = opt_model['osp'] if flds is None or wvls is None or ref_wvl is None else None
    if flds is None:
        flds = list(osp['fov'].fields)
        if field_wts is None:
            field_wts = [f.wt for f in flds]
    if wvls is None:
        wvls = list(osp['wvls'].wavelengths)
        if spectral_wts is None:
            spectral_wts = list(osp['wvls'].spectral_wts)
    flds, wvls = list(flds), [float(w) for w in wvls]
    if field_wts is None:
        field_wts = [getattr(f, 'wt', 1.0) for f in flds]
    if spectral_wts is None:
        spectral_wts = [1.0] * len(wvls)
    if ref_wvl is None:
        ref_wvl = osp['wvls'].central_wvl
    ref_wvl = float(ref_wvl)
    if ref_wvl not in wvls:
        raise ValueError(f'{what}: ref_wvl {ref_wvl} is not one of the wavelengths {wvls}')
    F, W = len(flds), len(wvls)
    if not 1 <= F * W <= abi.MAX_FOCUS_ITEMS:
        raise ValueError(f'{what}: 1 to {abi.MAX_FOCUS_ITEMS} (field, wavelength) items, got {F * W}')
    if len(field_wts) != F or len(spectral_wts) != W:
        raise ValueError(f'{what}: one weight per field and per wavelength')
    return flds, wvls, field_wts, spectral_wts, ref_wvl


def _map_items(opt_model, flds, wvls, focs, xy, num_rays, kwargs, radii=None):
    """every (field, wavelength) item of a map, field-major, each built as through_focus builds
    its one scan -> (engine, fields, wavelength indices, grids, options, planes); ``radii``, a
    list, receives each item's list of reference-sphere radii"""
    planes, grids, fs, wis, opts_list = [], [], [], [], []
    eng = None
    for fld in flds:
        for wvl in wvls:                                # each item as through_focus builds it
            r = [] if radii is not None else None
            planes.append(_focus_planes(opt_model, fld, wvl, focs, radii=r))
            if radii is not None:
                radii.append(r)
            kw = dict(kwargs)
            grids.append(_focus_grid(opt_model, fld, xy, num_rays, kw))
            eng, f, wi, opts = _launch_setup(opt_model, fld, wvl, kw, abi.OUT_FAN)
            fs.append(f)
            wis.append(wi)
            opts_list.append(opts)
    return eng, fs, wis, grids, opts_list, planes


def _wave_scales(opt_model, wvls, n_items):
    """[n_items] 1 / wavelength in system units of each (field, wavelength) item: OPD -> waves"""
    W = len(wvls)
    return np.array([1 / opt_model.nm_to_sys_units(wvls[i % W]) for i in range(n_items)])


def _image_pts(planes):
    """[items, K, 2] the image point of every plane of every item"""
    return np.array([[(p.image_pt[0], p.image_pt[1]) for p in ps] for ps in planes])


def through_focus_map(opt_model, focs, flds=None, wvls=None, num_rays=21, xy=None, field_wts=None,
                      spectral_wts=None, ref_wvl=None, rows=False, **kwargs):
    """Through-focus scans of every field at every wavelength in ONE device call
    (rox_trace_through_focus_grids): item (f, w) is through_focus(opt_model, flds[f], wvls[w],
    focs, num_rays, xy, ...) -- the same planes, grid and statistics, bit for bit -- and the
    per-field polychromatic statistics, field curvature and white-light best focus follow on the
    host (:class:`ThroughFocusMap`).  Defaults: the fields of osp['fov'] with their ``wt``, the
    wavelengths of osp['wvls'] with its spectral_wts, ref_wvl = its central_wvl (a
    workloads.TableModel has no osp: pass them).  A focus whose reference sphere the device
    cannot express raises UnsupportedModelError for the whole call."""
    from .engine import grid_rays
    focs = _check_focs(focs, 'through_focus_map')
    flds, wvls, field_wts, spectral_wts, ref_wvl = _map_spec(opt_model, flds, wvls, field_wts, spectral_wts,
                                                             ref_wvl, 'through_focus_map')
    F, W, K = len(flds), len(wvls), len(focs)
    eng, fs, wis, grids, opts_list, planes = _map_items(opt_model, flds, wvls, focs, xy, num_rays, kwargs)
    out = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=rows)
    stats, dev_rows = out if rows else (out, None)
    stats = np.stack([_stats_in_waves(stats[i], opt_model, wvls[i % W]) for i in range(F * W)])
    image_pts = _image_pts(planes)
    host_rows = status = None
    if dev_rows is not None:
        R = grid_rays(grids[0])
        host_rows, status = dev_rows.to_host()
        host_rows = np.array(host_rows[:, :, :, :R])
        scale = _wave_scales(opt_model, wvls, F * W)
        for i in range(F * W):
            host_rows[i, :, 2] = scale[i] * host_rows[i, :, 2]
        host_rows = host_rows.reshape(F, W, K, 3, R)
        status = np.asarray(status)[:, :R].reshape(F, W, R)
    return ThroughFocusMap(focs, wvls, field_wts, spectral_wts, ref_wvl, stats.reshape(F, W, K),
                           image_pts.reshape(F, W, K, 2), host_rows, status)


# ---- beam footprints on every surface ---------------------------------------------
# the half width of a surface's map: its semi-diameter times this margin, so that the record that
# set the semi-diameter lies strictly inside the last bin
FOOTPRINT_MAP_MARGIN = 1.0 + 2.0 ** -20


class BeamFootprints:
    """what :func:`beam_footprints` returns.

    ``records``       [F, W, n_seg] rox_footprint records (engine.FOOTPRINT_DTYPE)
    ``slot_ifc``      [n_seg] the interface index of each slot
    ``semi_diameter`` [n_seg] sqrt(max r2_max) over the items; 0 where no record was counted
    ``bbox``          [n_seg, 2, 2] the union bounding box (min, max) x (x, y)
    ``max_aoi``       [n_seg] the largest angle of incidence in degrees (NaN: none), produced by
                      item ``max_aoi_item`` [n_seg, 2] = (field, wavelength) (-1: none)
    ``lost_by_field`` [F, n_seg, 5] rays lost at each slot by status, summed over wavelengths;
                      ``lost`` [n_seg, 5] their sum
    ``maps``          [F, W, n_seg, B, B] or None; ``field_maps`` [F, n_seg, B, B] summed over
                      wavelengths, ``union_map`` [n_seg, B, B] and ``overlap`` [n_seg, B, B] the
                      number of fields that light each bin; ``half_width`` [n_seg] of the maps
    ``results``       the device packets, with ``keep_packets``"""

    def __init__(self, records, slot_ifc, n_ifcs, trace_flags, maps=None, half_width=None, results=None):
        self.records = records
        self.slot_ifc = np.asarray(slot_ifc)
        self.n_ifcs = int(n_ifcs)
        self.trace_flags = int(trace_flags)
        self.results = results
        F, W, n_seg = records.shape
        flat = records.reshape(F * W, n_seg)
        r2 = flat['r2_max'].max(axis=0)
        self.semi_diameter = np.sqrt(np.where(r2 >= 0.0, r2, 0.0))
        self.bbox = np.stack([flat['min'].min(axis=0), flat['max'].max(axis=0)], axis=1)
        cmin = np.where(np.isnan(flat['cos_inc_min']), np.inf, flat['cos_inc_min'])
        item = cmin.argmin(axis=0)
        best = cmin.min(axis=0)
        some = np.isfinite(best)
        self.max_aoi = np.where(some, np.degrees(np.arccos(np.clip(np.where(some, best, 1.0), -1.0, 1.0))), np.nan)
        self.max_aoi_item = np.where(some[:, None], np.stack([item // W, item % W], axis=1), -1)
        self.lost_by_field = records['n_fail'].sum(axis=1)
        self.lost = self.lost_by_field.sum(axis=0)
        self.maps = maps
        self.half_width = half_width
        self.field_maps = self.union_map = self.overlap = None
        if maps is not None:
            self.field_maps = maps.astype(np.int64).sum(axis=1)
            self.union_map = self.field_maps.sum(axis=0)
            self.overlap = (self.field_maps > 0).sum(axis=0)

    def clear_apertures(self, margin=0.0):
        """the semi-diameter per interface index times (1 + margin), ready for
        ``ifc.set_max_aperture`` (0 for an interface without a slot or a record); the model is
        not touched"""
        margin = float(margin)
        if not (np.isfinite(margin) and margin >= 0.0):
            raise ValueError(f'clear_apertures: margin {margin} is not finite and >= 0')
        out = np.zeros(self.n_ifcs)
        out[self.slot_ifc] = self.semi_diameter * (1.0 + margin)
        return out


def _packet_items(opt_model, flds, wvls, num_rays, check_apertures, what, out_mode=abi.OUT_FULL):
    """every (field, wavelength) item of a packet analysis, field-major, each set up for a FULL
    (or ``out_mode``) launch over the field's vignetted pupil; defaults as _map_spec, ref_wvl the
    first wavelength given -> (engine, flds, wvls, spectral_wts, fields, wavelength indices,
    options, trace flags)"""
    if num_rays < 1 or num_rays * num_rays > abi.MAX_FOOTPRINT_RAYS:
        raise ValueError(f'{what}: num_rays {num_rays} outside [1, 16384]')
    flds, wvls, _fw, spectral_wts, _ref = _map_spec(opt_model, flds, wvls, None, None,
                                                    wvls[0] if wvls is not None and len(wvls) else None, what)
    fs, wis, opts_list = [], [], []
    eng = None
    for fld in flds:
        for wvl in wvls:
            kw = dict(check_apertures=bool(check_apertures), apply_vignetting=True)
            eng, f, wi, opts = _launch_setup(opt_model, fld, wvl, kw, out_mode)
            fs.append(f)
            wis.append(wi)
            opts_list.append(opts)
    flags = int(opts_list[0].flags)
    if any(int(o.flags) != flags for o in opts_list):
        raise ValueError(f'{what}: the fields do not share their trace flags')
    return eng, flds, wvls, spectral_wts, fs, wis, opts_list, flags


def _trace_packets(eng, fs, wis, opts_list, num_rays):
    """the items' num_rays x num_rays grids over the unit pupil box in one FULL launch; the packets
    stay in HBM"""
    return eng.trace_pupil_grids(fs, wis, make_grid((-1., -1.), (1., 1.), num_rays), opts_list, want_pupil=False)


def beam_footprints(opt_model, flds=None, wvls=None, num_rays=64, maps=0, check_apertures=False, partial=True,
                    ok_only=False, keep_packets=False):
    """The beam on every surface from a dense pupil grid, on the device: one FULL launch
    (rox_trace_pupil_grids) over every (field, wavelength) -- ``num_rays`` x ``num_rays`` rays
    over each field's vignetted pupil (the unit pupil box with apply_vignetting, as the spot
    diagram figures trace it) -- whose packets stay in HBM, then one rox_surface_footprints call
    over them: what vigcalc.set_clear_apertures asks of four rim rays per field
    (rayoptics/raytr/vigcalc.py:31-63), asked of every ray.  ``maps`` > 0 adds a second call for
    ``maps`` x ``maps`` histograms of the landing points per (field, wavelength, surface) over
    [-h, h]^2, h = the surface's semi-diameter just found times FOOTPRINT_MAP_MARGIN (1 + 2^-20:
    the farthest record falls inside the last bin, not on its closed edge); a surface without a
    record gets h = 1.  ``partial`` / ``ok_only`` select the records as the entry documents.
    Defaults as the through-focus maps: the fields of osp['fov'], the wavelengths of osp['wvls']
    (a workloads.TableModel has no osp: pass them).  Returns :class:`BeamFootprints`."""
    num_rays, maps = int(num_rays), int(maps)
    if not 0 <= maps <= abi.MAX_FOOTPRINT_BINS:
        raise ValueError(f'beam_footprints: maps {maps} outside [0, {abi.MAX_FOOTPRINT_BINS}]')
    eng, flds, wvls, _sw, fs, wis, opts_list, flags = _packet_items(opt_model, flds, wvls, num_rays, check_apertures,
                                                                    'beam_footprints')
    F, W = len(flds), len(wvls)
    results = _trace_packets(eng, fs, wis, opts_list, num_rays)
    rec, _none = eng.surface_footprints(results, flags, partial=partial, ok_only=ok_only)
    n_seg = rec.shape[1]
    tbl = eng.table
    slot_ifc = eng.slot_interfaces(flags)
    hmaps = hw = None
    if maps:
        r2 = rec['r2_max'].max(axis=0)
        hw = np.where(r2 > 0.0, np.sqrt(np.where(r2 > 0.0, r2, 1.0)) * FOOTPRINT_MAP_MARGIN, 1.0)
        _rec, hmaps = eng.surface_footprints(results, flags, partial=partial, ok_only=ok_only, half_width=hw,
                                             n_bins=maps, want_records=False)
        hmaps = hmaps.reshape(F, W, n_seg, maps, maps)
    return BeamFootprints(rec.reshape(F, W, n_seg), slot_ifc, tbl.n_ifcs, flags, hmaps, hw,
                          results if keep_packets else None)


# ---- Fresnel transmission and polarization over full packets ------------------------
def _weighted_mean(v, s):
    """[F, W] values merged over wavelengths with the weights s [W]; a NaN value (no ray counted)
    takes no part, and a field without any value is NaN"""
    v = np.asarray(v, dtype=np.float64)
    ok = np.isfinite(v)
    w = np.where(ok, np.asarray(s, dtype=np.float64)[None, :], 0.0)
    tot = w.sum(axis=1)
    num = (w * np.where(ok, v, 0.0)).sum(axis=1)
    return np.where(tot > 0.0, num / np.where(tot > 0.0, tot, 1.0), np.nan)


class Transmission:
    """what :func:`transmission` returns.

    ``items``         [F, W] rox_tx_item records (engine.TX_ITEM_DTYPE); ``surfaces`` [F, W, n_seg]
                      rox_tx_surface records (engine.TX_SURFACE_DTYPE)
    ``T``             [F, W] the mean transmission of unpolarized light over the rays that arrived
                      (NaN: none did)
    ``throughput``    [F, W] sum of T over the rays launched: vignetting counted
    ``poly_T``, ``poly_throughput``  [F] merged over the wavelengths with the spectral weights
    ``pupil_fraction``  [F] the share of the unit pupil box each field's grid spans: with
                      apply_vignetting a field's rays are launched over its own vignetted box
                      [-(1 - vlx), 1 - vux] x [-(1 - vly), 1 - vuy], so a ray of a vignetted field
                      stands for less of the entrance pupil -- (2 - vlx - vux)(2 - vly - vuy)/4
    ``relative``      [F] poly_throughput * pupil_fraction over that of field ``ref_field``:
                      RELATIVE TRANSMISSION INCLUDING VIGNETTING, by the vignetting factors and
                      by the rays the apertures block alike.  (Where a field's factors differ
                      between the two sides of an axis, its two halves are sampled at different
                      densities; the box's area then weights their mean.)  It is not radiometric
                      relative illumination: no projected pupil area, no cos^4 and no distortion
                      term is applied -- that is :func:`relative_illumination`.
    ``surface_T``     [F, W, n_seg] the mean (Ts + Tp)/2 of each slot (1 at the object, the image
                      and every interface counted as ideal)
    ``surface_loss``  the slots ranked by their loss 1 - mean (Ts + Tp)/2 over every item's
                      rays, largest first: a list of (slot, interface, loss)
    ``slot_ifc``      [n_seg] the interface index of each slot
    ``diattenuation_max``, ``diattenuation_mean``  [F, W]
    ``T_map``, ``D_map``  [F, W, num_rays, num_rays] views of the rows, NaN where a ray failed
                      (x the first axis), or None
    ``E1``, ``E2``    [F, W, 3, num_rays, num_rays] the exit field vectors of the x-like and the
                      y-like input state in the image frame (complex where a Coating was
                      evaluated: a stack's ts and tp differ in phase), or None
    ``results``       the device packets, with ``keep_packets``"""

    def __init__(self, items, surfaces, slot_ifc, spectral_wts, ref_field=0, rows=None, num_rays=None, results=None,
                 pupil_fraction=None):
        self.items, self.surfaces = items, surfaces
        self.slot_ifc = np.asarray(slot_ifc)
        self.spectral_wts = np.asarray(spectral_wts, dtype=np.float64)
        self.ref_field = int(ref_field)
        self.results = results
        F, W = items.shape
        if not 0 <= self.ref_field < F:
            raise ValueError(f'Transmission: ref_field {ref_field} outside [0, {F})')
        n = items['n_ok'].astype(np.float64)
        some = n > 0
        den = np.where(some, n, 1.0)
        self.T = np.where(some, items['t_sum'] / den, np.nan)
        self.throughput = items['t_sum'] / items['n_rays']
        self.diattenuation_mean = np.where(some, items['d_sum'] / den, np.nan)
        self.diattenuation_max = items['d_max'].copy()
        self.poly_T = _weighted_mean(self.T, self.spectral_wts)
        self.poly_throughput = _weighted_mean(self.throughput, self.spectral_wts)
        self.pupil_fraction = np.ones(F) if pupil_fraction is None else np.asarray(pupil_fraction, dtype=np.float64)
        if self.pupil_fraction.shape != (F,):
            raise ValueError(f'Transmission: one pupil_fraction per field, got {self.pupil_fraction.shape}')
        weighted = self.poly_throughput * self.pupil_fraction
        self.relative = weighted / weighted[self.ref_field]
        ns = surfaces['n'].astype(np.float64)
        self.surface_T = np.where(ns > 0, surfaces['t_sum'] / np.where(ns > 0, ns, 1.0), np.nan)
        tot_n = ns.sum(axis=(0, 1))
        mean = np.where(tot_n > 0, surfaces['t_sum'].sum(axis=(0, 1)) / np.where(tot_n > 0, tot_n, 1.0), 1.0)
        loss = 1.0 - mean
        order = sorted(range(loss.shape[0]), key=lambda k: (-loss[k], k))
        self.surface_loss = [(k, int(self.slot_ifc[k]), float(loss[k])) for k in order]
        self.T_map = self.D_map = self.E1 = self.E2 = None
        if rows is not None:
            num = int(num_rays)
            grid = rows.reshape(F, W, rows.shape[1], num, num)
            self.T_map, self.D_map = grid[:, :, 0], grid[:, :, 3]
            if rows.shape[1] == 10:
                self.E1, self.E2 = grid[:, :, 4:7], grid[:, :, 7:10]
            elif rows.shape[1] == 16:           # thin films: complex amplitudes
                self.E1 = grid[:, :, 4:7] + 1j * grid[:, :, 10:13]
                self.E2 = grid[:, :, 7:10] + 1j * grid[:, :, 13:16]


def _coating_tables(table, coatings):
    """``coatings`` of :func:`transmission` -> (coat_kind [n_ifcs], coat_value [n_ifcs, 2],
    {interface: Coating in the order the light crosses its layers}) or (None, None, {})"""
    if coatings is None:
        return None, None, {}
    N = table.n_ifcs
    kind = np.zeros(N, np.int32)
    value = np.ones((N, 2), np.float64)
    stacks = {}
    nt = np.asarray(table.n_table)

    def air(i):
        return bool((nt[:, i] == 1.0).all())

    def stack(i, c):
        """a Coating is written outside-first: as written where the light comes from the air (or
        onto a mirror), flipped where the glass is the preceding medium"""
        flip = 0 < i < N - 1 and table.rows[i].mode != abi.REFLECT and air(i) and not air(i - 1)
        kind[i], stacks[i] = abi.COAT_STACK, c.reversed() if flip else c

    def fixed(v):
        try:
            v = None if isinstance(v, str) else np.asarray(v, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            v = None
        if v is None or v.shape[0] not in (1, 2) or not (np.isfinite(v).all() and (v >= 0).all() and (v <= 1).all()):
            raise ValueError(f'transmission: coatings: {coatings!r} is not \'bare\', \'ideal\', a power '
                             f'transmission in [0, 1] or a pair (Ts, Tp) of them')
        return (v[0], v[-1])

    if isinstance(coatings, str):
        if coatings != 'ideal':
            raise ValueError(f'transmission: coatings: {coatings!r} is not None, \'ideal\', a value or a dict')
        kind[:] = abi.COAT_IDEAL
    elif isinstance(coatings, dict):
        for i, c in coatings.items():
            if not (isinstance(i, (int, np.integer)) and 0 < i < N - 1):
                raise ValueError(f'transmission: coatings: key {i!r} is not an interface index in [1, {N - 2}]')
            if isinstance(c, str) and c in ('bare', 'ideal'):
                kind[i] = abi.COAT_IDEAL if c == 'ideal' else abi.COAT_BARE
            elif isinstance(c, Coating):
                stack(i, c)
            else:
                kind[i], value[i] = abi.COAT_FIXED, fixed(c)
    else:
        v = None if isinstance(coatings, Coating) else fixed(coatings)
        for i in range(1, N - 1):
            if table.rows[i].mode == abi.TRANSMIT and air(i - 1) != air(i):     # glass on exactly one side
                if v is None:
                    stack(i, coatings)
                else:
                    kind[i], value[i] = abi.COAT_FIXED, v
    return kind, value, stacks


def transmission(opt_model, flds=None, wvls=None, num_rays=64, coatings=None, check_apertures=True, pupil_maps=True,
                 fields=False, keep_packets=False, packets=None, ref_field=0):
    """How much of the light arrives, on the device: one FULL launch (rox_trace_pupil_grids) over
    every (field, wavelength), set up exactly as :func:`beam_footprints` does, whose packets stay
    in HBM, then one rox_surface_transmission call over them -- the Fresnel equations at every
    interface with two orthogonal field vectors carried along each ray (include/roxtrace.h states
    the arithmetic).  ``packets``: the result of ``beam_footprints(..., keep_packets=True)`` (or
    its ``results``) over the same fields, wavelengths and ``num_rays`` -- no ray is traced again,
    one trace serves both analyses.  ``coatings``: None (bare surfaces), 'ideal' (every interface
    lossless), a power transmission or a pair (Ts, Tp) for every glass-air surface, or a dict
    {interface index: 'bare' | 'ideal' | value | (Ts, Tp)}.  A :class:`coatings.Coating` -- a
    thin-film stack, absorbing layers and a metal substrate included -- is accepted wherever a
    value is: given bare it goes on every glass-air surface, flipped where the glass is the
    preceding medium; as a dict value it is applied as written, outside-first on the air side
    (on a mirror its ``substrate`` is the metal).  With a Coating present the one call is
    rox_surface_thinfilm (the other interfaces' kinds alongside) and ``E1``, ``E2`` are complex.
    ``pupil_maps`` keeps the per-ray rows (T_map, D_map), ``fields`` adds the exit field vectors.
    Spectral weights as the through-focus maps take them (osp['wvls'], or 1 per wavelength when
    ``wvls`` is given).

    ``relative`` of the result is relative transmission including vignetting -- poly_throughput
    times the share of the unit pupil box the field's vignetting factors leave its grid, over that
    of field ``ref_field``.  It is NOT radiometric relative illumination: no projected
    pupil area, cos^4 or distortion term is applied; :func:`relative_illumination` answers that,
    from the image-space solid angle of the same grids.  Out of scope here are
    absorbing glasses (bulk absorption) and diffraction efficiencies: thin lenses and phase
    elements are counted as ideal, and so is a mirror without a Coating.
    Returns :class:`Transmission`."""
    num_rays = int(num_rays)
    eng, flds, wvls, spectral_wts, fs, wis, opts_list, flags = _packet_items(opt_model, flds, wvls, num_rays,
                                                                             check_apertures, 'transmission')
    F, W = len(flds), len(wvls)
    if not 0 <= int(ref_field) < F:
        raise ValueError(f'transmission: ref_field {ref_field} outside [0, {F})')
    box = [(2.0 - f.vlx - f.vux) * (2.0 - f.vly - f.vuy) / 4.0 for f in fs[W - 1::W]]     # one per field
    kind, value, stacks = _coating_tables(eng.table, coatings)
    film = stack_tables(eng.table, stacks, 'transmission') if stacks else None
    if packets is not None:
        flags = int(getattr(packets, 'trace_flags', flags))
        results = list(getattr(packets, 'results', packets) or [])
        if len(results) != F * W or any(int(r.R) != num_rays * num_rays for r in results):
            raise ValueError(f'transmission: packets are not {F * W} items of {num_rays}^2 rays (were they kept '
                             f'with keep_packets=True?)')
    else:
        results = _trace_packets(eng, fs, wis, opts_list, num_rays)
    if film is None:
        rows, surf, item = eng.surface_transmission(results, flags, wis, coat_kind=kind, coat_value=value,
                                                    want_rows=bool(pupil_maps or fields), fields=bool(fields))
    else:
        first, thick, index, sub = film
        rows, surf, item = eng.surface_thinfilm(results, flags, wis, [float(eng.table.wvls[w]) for w in wis],
                                                coat_kind=kind, coat_value=value, stack_first=first,
                                                layer_thickness=thick, layer_index=index, sub_index=sub,
                                                want_rows=bool(pupil_maps or fields), fields=bool(fields))
    n_seg = surf.shape[1]
    return Transmission(item.reshape(F, W), surf.reshape(F, W, n_seg), eng.slot_interfaces(flags), spectral_wts,
                        ref_field, rows, num_rays, results if keep_packets else None, box)


# ---- radiometric relative illumination from the image-space solid angle -------------
def _coating_stack_tables(table, coatings, what):
    """``coatings`` of :func:`transmission` -> (coat_kind, coat_value, the stack tables of
    coatings.stack_tables or None without a Coating), checked"""
    kind, value, stacks = _coating_tables(table, coatings)
    return kind, value, stack_tables(table, stacks, what) if stacks else None


def _transmission_rows(eng, results, flags, wis, tables):
    """the transmission (or, with a Coating, thin-film) call of :func:`transmission` over packets
    in HBM with the per-ray rows left there; ``tables`` from _coating_stack_tables -> (rows: a
    device tensor [n_items, 4, R], row 0 = T; the raw rox_tx_item records [n_items, 72], also in HBM)"""
    kind, value, film = tables
    if film is None:
        rows, _surf, item = eng.surface_transmission(results, flags, wis, coat_kind=kind, coat_value=value,
                                                     on_device=True)
    else:
        first, thick, index, sub = film
        rows, _surf, item = eng.surface_thinfilm(results, flags, wis, [float(eng.table.wvls[w]) for w in wis],
                                                 coat_kind=kind, coat_value=value, stack_first=first,
                                                 layer_thickness=thick, layer_index=index, sub_index=sub,
                                                 on_device=True)
    return rows, item


class RelativeIllumination:
    """what :func:`relative_illumination` returns.

    ``items``         [F, W] rox_sa_item records (engine.SA_ITEM_DTYPE)
    ``omega_raw``     [F, W] |A|, A = a_full + a_tri: the projected solid angle of the image-space
                      bundle as the cells with three or four rays that arrived add up to
    ``omega``         [F, W] |A + c|, the boundary-corrected projected solid angle: a cell with k of
                      its corners inside the beam is on average k/4 inside it, and A counted such
                      cells as 0, 0, 1/2 or 1, so c = cell * (n1/4 + n2/2 + n3/4) with cell =
                      a_full / n4 the mean full cell and nk = n_cells[k]
    ``boundary_share``  [F, W] c / (A + c): what the correction contributes -- the handle on
                      convergence, which is first-order in 1 / num_rays
    ``ri``            [F, W] omega / omega[ref_field], per wavelength
    ``poly_omega``, ``poly_ri``  [F] omega merged over the wavelengths with the spectral weights,
                      and its ratio to that of field ``ref_field``
    ``omega_t``, ``ri_t``, ``poly_omega_t``, ``poly_ri_t``  the same of the integral of T dL dM
                      (aw_full + aw_tri, the correction scaled by its ratio to A); None without
                      ``coatings``
    ``fno_eff``       [F, W] 1 / (2 sqrt(omega / pi)), the effective image-space F-number
    ``chief_dir``     [F, W, 2] (l_sum, m_sum) / n_ok, the mean direction of arrival
    ``na_max``        [F, W] sqrt(r2_max), the largest sine of arrival
    ``folded``        [F, W] a_abs exceeds |A| by more than (n3 + n4) * 2^-52 * a_abs: the pupil
                      map folds over and the signed area under-counts
    ``cell_maps``     [F, W, num_rays - 1, num_rays - 1] the cells' signed areas (x the first
                      axis), or None
    ``flds``          the fields, those a ``sweep`` made included
    An item without a ray is NaN throughout; so is a ratio to an ``omega`` of 0 (an afocal image
    space)."""

    def __init__(self, items, spectral_wts, ref_field=0, weighted=False, cell_maps=None, flds=None):
        self.items = items
        self.spectral_wts = np.asarray(spectral_wts, dtype=np.float64)
        self.ref_field = int(ref_field)
        self.cell_maps = cell_maps
        self.flds = flds
        F, _W = items.shape
        if not 0 <= self.ref_field < F:
            raise ValueError(f'RelativeIllumination: ref_field {ref_field} outside [0, {F})')
        nc = items['n_cells'].astype(np.float64)
        some = items['n_ok'] > 0
        with np.errstate(divide='ignore', invalid='ignore'):
            A = items['a_full'] + items['a_tri']
            cell = np.where(nc[..., 4] > 0, items['a_full'] / np.where(nc[..., 4] > 0, nc[..., 4], 1.0), 0.0)
            corr = cell * (nc[..., 1] * 0.25 + nc[..., 2] * 0.5 + nc[..., 3] * 0.25)
            self.omega_raw = np.where(some, np.abs(A), np.nan)
            self.omega = np.where(some, np.abs(A + corr), np.nan)
            self.boundary_share = np.where(some, corr / (A + corr), np.nan)
            self.ri, self.poly_omega, self.poly_ri = self._ratios(self.omega)
            self.omega_t = self.ri_t = self.poly_omega_t = self.poly_ri_t = None
            if weighted:
                Aw = items['aw_full'] + items['aw_tri']
                self.omega_t = np.where(some, np.abs(Aw + corr * (Aw / A)), np.nan)
                self.ri_t, self.poly_omega_t, self.poly_ri_t = self._ratios(self.omega_t)
            self.fno_eff = 1.0 / (2.0 * np.sqrt(self.omega / np.pi))
            n = np.where(some, items['n_ok'], 1).astype(np.float64)
            self.chief_dir = np.where(some[..., None], np.stack([items['l_sum'] / n, items['m_sum'] / n], axis=-1),
                                      np.nan)
            self.na_max = np.sqrt(items['r2_max'])
            self.folded = items['a_abs'] - np.abs(A) > (nc[..., 3] + nc[..., 4]) * 2.0 ** -52 * items['a_abs']

    def _ratios(self, omega):
        """(omega / omega[ref_field] per wavelength, omega merged over the wavelengths, its ratio)"""
        poly = _weighted_mean(omega, self.spectral_wts)
        return omega / omega[self.ref_field][None, :], poly, poly / poly[self.ref_field]


def _field_sweep(opt_model, n):
    """``n`` fields evenly spaced from the axis to the model's outermost field along that field's
    (x, y) direction: copies of it without vignetting factors, aimed in one batch"""
    import copy
    from .trace import aim_chief_rays
    from .workloads import TableModel
    n = int(n)
    if n < 2:
        raise ValueError(f'relative_illumination: sweep {n} < 2')
    if isinstance(opt_model, TableModel):
        raise ValueError('relative_illumination: sweep needs a live model: a TableModel carries prebuilt fields only')
    fov = opt_model['osp']['fov']
    _value, k = fov.max_field()
    outer = fov.fields[k]
    flds = []
    for t in np.linspace(0.0, 1.0, n):
        f = copy.copy(outer)
        f.x, f.y = float(outer.x * t), float(outer.y * t)
        f.vux = f.vuy = f.vlx = f.vly = 0.0
        f.chief_ray = f.ref_sphere = None
        flds.append(f)
    for f, aim in zip(flds, aim_chief_rays(opt_model, flds)):
        f.aim_info = aim
    return flds


def relative_illumination(opt_model, flds=None, wvls=None, num_rays=128, coatings=None, check_apertures=True,
                          ref_field=0, sweep=None, cell_maps=False):
    """Radiometric relative illumination, on the device: how bright each field's image point is
    compared with field ``ref_field``'s.  For a Lambertian object of uniform radiance the
    irradiance at an image point is proportional to the integral of T dL dM over the direction
    cosines (L, M) with which the bundle arrives (conservation of basic radiance; Rimmer, "Relative
    illumination calculations", 1986): cos^4, pupil aberration, distortion and vignetting are all
    in that one area, which rox_projected_solid_angle takes from the ``num_rays`` x ``num_rays``
    pupil grid of every (field, wavelength) where its rows are (include/roxtrace.h states the
    arithmetic).  Items and defaults as :func:`transmission`: field-major, the unit pupil box with
    apply_vignetting.  Without ``coatings`` one OUT_LAST launch and one call (T = 1: the geometric
    answer).  With ``coatings`` -- anything :func:`transmission` accepts, a Coating included, or
    'bare' for the Fresnel losses of uncoated surfaces -- the FULL launch, the transmission (or
    thin-film) call with its rows left on the device, and the call with row 0 (T) as the weight.

    ``sweep`` = n replaces ``flds`` by n fields evenly spaced from the axis to the outermost field
    along its (x, y) direction, without vignetting factors (the clear apertures do the
    vignetting) and aimed in one batch: the RI-against-field curve.  A live model only.

    Limits.  The object is taken as Lambertian.  (L, M) are direction cosines in the image
    interface's own frame: for a curved or tilted image this is the irradiance on that frame's
    z-plane.  An afocal image space has omega = 0 and its ratios are NaN.  The estimate converges
    first-order in 1 / num_rays (``boundary_share``).  Returns :class:`RelativeIllumination`."""
    num_rays = int(num_rays)
    if not 2 <= num_rays <= abi.MAX_SA_NUM:
        raise ValueError(f'relative_illumination: num_rays {num_rays} outside [2, {abi.MAX_SA_NUM}]')
    if sweep is not None:
        flds = _field_sweep(opt_model, sweep)
    weighted = coatings is not None
    eng, flds, wvls, spectral_wts, fs, wis, opts_list, flags = _packet_items(
        opt_model, flds, wvls, num_rays, check_apertures, 'relative_illumination',
        abi.OUT_FULL if weighted else abi.OUT_LAST)
    F, W = len(flds), len(wvls)
    if not 0 <= int(ref_field) < F:
        raise ValueError(f'relative_illumination: ref_field {ref_field} outside [0, {F})')
    rows = None
    if weighted:
        bare = isinstance(coatings, str) and coatings == 'bare'
        tables = _coating_stack_tables(eng.table, None if bare else coatings, 'relative_illumination')
    results = _trace_packets(eng, fs, wis, opts_list, num_rays)
    if weighted:
        rows, _item = _transmission_rows(eng, results, flags, wis, tables)
    items, cells = eng.projected_solid_angle(results, num_rays, weight=rows, weight_row=0, want_cells=bool(cell_maps))
    if cells is not None:
        cells = cells.reshape(F, W, num_rays - 1, num_rays - 1)
    return RelativeIllumination(items.reshape(F, W), spectral_wts, ref_field, weighted, cells, flds)


# ---- two-reflection ghosts ---------------------------------------------------------
class Ghosts:
    """what :func:`ghost_analysis` returns.  P pairs, F fields, W wavelengths; a pair is (j, i):
    reflected at interface j, then at the earlier interface i.

    ``pairs``         the P pairs analysed; ``skipped`` the pairs left out, as ((j, i), reason)
    ``records``       P arrays [F, W, n_seg_p] of rox_seg_focus records (engine.SEG_FOCUS_DTYPE),
                      the rays weighted by the ghost path's transmission; ``slots`` P dicts with
                      the ``source`` interface, the ``pass_`` (reflections so far) and the nominal
                      ``gap`` (medium) of the segment after each slot
    ``rays``          [P, F, W] rays that arrive at the image
    ``flux``          [P, F, W] the sum of their weights; ``signal`` [F, W] that of the nominal path
    ``ratio``         [P, F, W] flux / signal
    ``in_detector``   [P, F, W] the share of the flux that lands inside ``detector`` (1 without one)
    ``centroid``      [P, F, W, 2] the weighted centroid of the ghost patch on the image plane
    ``rms_patch``     [P, F, W] its weighted RMS radius
    ``focus_distance``  [P, F, W] where the ghost focuses, from the image plane along z (NaN: a
                      collimated bundle)
    ``poly_flux``, ``poly_ratio``, ``poly_rms_patch``  [P, F] merged over the wavelengths with the
                      spectral weights of :class:`Transmission` (poly_ratio = poly_flux over the
                      signal merged the same way)
    ``internal_foci`` the ghost light's foci between two interfaces, after the first reflection: a
                      list of dicts (pair, field, wvl, source, pass_, gap, zeta, rms_min)
    ``results``       the device packets of every pair, with ``keep_packets``; ``trace_flags`` the
                      rox_opts.flags they were traced with
    Items without a ray, or whose weights sum to 0, are NaN in the derived figures.

    With ``maps`` (rox_weighted_maps over the detector, a field's wavelengths summed into one map
    with the normalised spectral weights; None of these without):
    ``map_edges``     (x edges [nbx + 1], y edges [nby + 1]) of the detector's bins
    ``irradiance``    [P, F, nbx, nby] the ghost's flux per bin over the bin's area and over the
                      field's polychromatic signal flux (1 / length^2): its sum times the bin area
                      is poly_ratio times the share of the flux inside the detector
    ``irradiance_total``  [F, nbx, nby] the sum over the pairs, in pair order
    ``signal_irradiance`` [F, nbx, nby] the same of the nominal path
    ``peak``          [P, F] the ghost's brightest bin; ``peak_over_signal`` [P, F] that over the
                      signal's brightest bin on the same grid (NaN for a field whose image point
                      lies off the detector: there is no signal to compare with)
    ``ray_counts``    [P, F, nbx, nby] the rays behind each bin"""

    def __init__(self, pairs, skipped, records, slots, signal, spectral_wts, results=None, maps=None):
        from .engine import seg_focus_derive
        self.pairs = [tuple(p) for p in pairs]
        self.skipped = list(skipped)
        self.records, self.slots = list(records), list(slots)
        self.signal = np.asarray(signal, dtype=np.float64)
        self.spectral_wts = np.asarray(spectral_wts, dtype=np.float64)
        self.results, self.trace_flags = results, None
        F, W = self.signal.shape
        P = len(self.pairs)
        img = np.zeros((P, F, W), dtype=self.records[0].dtype) if P else np.zeros((0, F, W))
        for p, rec in enumerate(self.records):
            img[p] = rec[:, :, -1]
        self.internal_foci = []
        self.map_edges = self.irradiance = self.irradiance_total = self.signal_irradiance = None
        self.peak = self.peak_over_signal = self.ray_counts = None
        if maps is not None:
            self._set_maps(**maps)
        if P == 0:
            z = np.zeros((0, F, W))
            self.rays = z.astype(np.int64)
            self.flux = self.ratio = self.in_detector = self.rms_patch = self.focus_distance = z
            self.centroid = np.zeros((0, F, W, 2))
            self.poly_flux = self.poly_ratio = self.poly_rms_patch = np.zeros((0, F))
            return
        with np.errstate(divide='ignore', invalid='ignore'):
            zeta, _ms_min, ms_0, _inside = seg_focus_derive(img)
            self.rays = img['n'].copy()
            self.flux = img['w_sum'].copy()
            self.ratio = self.flux / self.signal[None]
            some = self.flux > 0.0
            self.in_detector = np.where(some, img['w_in'] / np.where(some, self.flux, 1.0), np.nan)
            self.centroid = img['a_mean'].copy()
            self.rms_patch = np.sqrt(ms_0)
            self.focus_distance = zeta
            self.poly_flux = np.stack([_weighted_mean(f, self.spectral_wts) for f in self.flux])
            poly_signal = _weighted_mean(self.signal, self.spectral_wts)
            self.poly_ratio = self.poly_flux / poly_signal[None]
            self.poly_rms_patch = np.stack([_weighted_mean(r, self.spectral_wts) for r in self.rms_patch])
        for p, (rec, sl) in enumerate(zip(self.records, self.slots)):
            zeta, ms_min, _ms_0, inside = seg_focus_derive(rec[:, :, :-1])
            for f, w, k in zip(*np.nonzero(inside & (np.asarray(sl['pass_'])[None, None, :-1] >= 1))):
                self.internal_foci.append(dict(pair=self.pairs[p], field=int(f), wvl=int(w),
                                               source=int(sl['source'][k]), pass_=int(sl['pass_'][k]),
                                               gap=int(sl['gap'][k]), zeta=float(zeta[f, w, k]),
                                               rms_min=float(np.sqrt(ms_min[f, w, k]))))

    def _set_maps(self, window, wmaps, scale_exp, counts, signal_wmaps, signal_scale_exp):
        """the map attributes from the integer sums of rox_weighted_maps: ``window`` = the
        detector's (hx, hy); ``wmaps`` int64 [P, F, nbx, nby] with ``scale_exp`` [P, F] and
        ``counts`` [P, F, nbx, nby] of the pairs, ``signal_wmaps`` [F, nbx, nby] with
        ``signal_scale_exp`` [F] of the nominal path -- each map the sum over the field's
        wavelengths of the normalised spectral weight times the rays' weights"""
        hx, hy = (float(v) for v in window)
        sig = np.asarray(signal_wmaps, dtype=np.int64)
        F, nbx, nby = sig.shape
        P = len(self.pairs)
        wm = np.asarray(wmaps, dtype=np.int64).reshape(P, F, nbx, nby)
        self.map_edges = (np.linspace(-hx, hx, nbx + 1), np.linspace(-hy, hy, nby + 1))
        area = (2.0 * hx / nbx) * (2.0 * hy / nby)
        poly_signal = _weighted_mean(self.signal, self.spectral_wts)
        with np.errstate(divide='ignore', invalid='ignore'):
            flux = np.ldexp(wm.astype(np.float64), -np.asarray(scale_exp, dtype=np.int32).reshape(P, F, 1, 1))
            self.irradiance = flux / area / poly_signal[None, :, None, None]
            sflux = np.ldexp(sig.astype(np.float64), -np.asarray(signal_scale_exp, dtype=np.int32).reshape(F, 1, 1))
            self.signal_irradiance = sflux / area / poly_signal[:, None, None]
            self.irradiance_total = np.zeros((F, nbx, nby))
            for p in range(P):
                self.irradiance_total = self.irradiance_total + self.irradiance[p]
            self.peak = self.irradiance.max(axis=(2, 3)) if P else np.zeros((0, F))
            top = self.signal_irradiance.max(axis=(1, 2))
            self.peak_over_signal = self.peak / np.where(top > 0.0, top, np.nan)[None]
        self.ray_counts = np.asarray(counts).reshape(P, F, nbx, nby).astype(np.int64)

    def _figure(self):
        """[P, F] poly_ratio / (pi * poly_rms_patch^2), -inf where a field has no flux or no patch"""
        with np.errstate(divide='ignore', invalid='ignore'):
            fig = self.poly_ratio / (np.pi * self.poly_rms_patch ** 2)
        return np.where(np.isnan(fig), -np.inf, fig)

    def ranking(self, by='area'):
        """the pairs by their largest poly_ratio / (pi * poly_rms_patch^2) over the fields -- flux
        over patch area, the brightest ghost first: a list of (pair index, figure); a pair without
        flux ranks last.  ``by='peak'`` (with maps): by their largest peak_over_signal instead."""
        if by not in ('area', 'peak'):
            raise ValueError(f"Ghosts.ranking: by {by!r} is not 'area' or 'peak'")
        if by == 'peak':
            if self.peak_over_signal is None:
                raise ValueError("Ghosts.ranking: by='peak' needs ghost_analysis(..., maps=...)")
            fig = np.where(np.isnan(self.peak_over_signal), -np.inf, self.peak_over_signal)
        else:
            fig = self._figure()
        best = fig.max(axis=1) if fig.size else np.zeros(0)
        order = sorted(range(len(self.pairs)), key=lambda p: (-best[p], p))
        return [(p, float(best[p])) for p in order]

    def table(self, n=10):
        """the ``n`` worst ghosts as text, one line per pair (its worst field)"""
        with_maps = self.peak_over_signal is not None
        lines = [' pair (j, i)   flux/signal   RMS patch   focus from image   in detector   flux/signal/area' +
                 ('   peak/signal peak' if with_maps else '')]
        figure = self._figure()
        for p, fig in self.ranking()[:n]:
            f = int(np.argmax(figure[p]))
            j, i = self.pairs[p]
            lines.append(f' ({j:3d}, {i:3d})   {self.poly_ratio[p, f]:11.3e}   {self.poly_rms_patch[p, f]:9.4g}   '
                         f'{_weighted_mean(self.focus_distance[p], self.spectral_wts)[f]:16.4g}   '
                         f'{_weighted_mean(self.in_detector[p], self.spectral_wts)[f]:11.3f}   {fig:16.3e}' +
                         (f'   {self.peak_over_signal[p, f]:18.3e}' if with_maps else ''))
        for (j, i), why in self.skipped:
            lines.append(f' ({j:3d}, {i:3d})   skipped: {why}')
        return '\n'.join(lines)


def ghost_analysis(opt_model, flds=None, wvls=None, num_rays=64, coatings=None, surfaces=None, pairs=None,
                   check_apertures=True, detector=None, keep_packets=False, maps=None):
    """Two-reflection ghosts, on the device: for every pair of refracting surfaces (j, i) the light
    reflected at j and again at the earlier i, followed to the image.  Items and defaults as
    :func:`transmission`.  Per pair: the unfolded table (ghost.unfold) on its own engine, one FULL
    launch over every (field, wavelength) with the nominal fields -- the object side up to j is
    untouched, so aim and vignetting box serve --, one rox_surface_thinfilm call whose rows stay
    in HBM (ghost.coating_tables: the reflecting rows are the Fresnel reflection of the bare or
    coated surface, total internal reflection included) and one rox_segment_foci call weighted
    by its row 0.  One nominal :func:`transmission` call gives the signal flux per item.
    ``coatings`` as :func:`transmission` takes them; ``surfaces`` restricts the reflecting
    interfaces; ``pairs`` names the (j, i) to analyse (each must be one ghost.ghost_pairs finds
    or skips); ``detector``: (hx, hy), the half-widths of a detector centred on the image axis.
    ``maps``: an int or (nbx, nby) -- irradiance maps over the ``detector`` (required then): per
    pair one rox_weighted_maps call on the packets and rows already in HBM, the field's wavelengths
    summed into one map with the normalised spectral weights; the nominal path, whose packets and
    rows then stay in HBM too, gets the same call (``signal_irradiance``).
    Not followed: the sensor as a reflector, more than two reflections, pairs with a mirror, a
    phase element or a thin lens between them (reported in ``skipped``).  Returns :class:`Ghosts`."""
    from . import ghost
    num_rays = int(num_rays)
    what = 'ghost_analysis'
    bins = None
    if maps is not None:
        if detector is None:
            raise ValueError(f'{what}: maps needs a detector (hx, hy): the maps cover it')
        bins = (int(maps), int(maps)) if np.ndim(maps) == 0 else tuple(int(b) for b in maps)
        if len(bins) != 2 or not all(1 <= b <= abi.MAX_WMAP_BINS for b in bins):
            raise ValueError(f'{what}: maps {maps!r} is not an int or (nbx, nby) in [1, {abi.MAX_WMAP_BINS}]')
    eng, flds, wvls, spectral_wts, fs, wis, opts_list, flags = _packet_items(opt_model, flds, wvls, num_rays,
                                                                             check_apertures, what)
    F, W = len(flds), len(wvls)
    table = eng.table
    found, skipped = ghost.ghost_pairs(table, surfaces)
    if pairs is not None:
        want = [(int(j), int(i)) for j, i in pairs]
        known = set(found) | {p for p, _why in skipped}
        for p in want:
            if p not in known:
                raise ValueError(f'{what}: pairs: {p} is not a pair of reflecting refracting surfaces (j, i), i < j')
        found = [p for p in found if p in want]
        skipped = [(p, why) for p, why in skipped if p in want]
    window = None
    if detector is not None:
        window = np.asarray(detector, dtype=np.float64).reshape(-1)
        if window.shape[0] != 2 or not (window > 0).all():
            raise ValueError(f'{what}: detector {detector!r} is not a pair (hx, hy) > 0')
    wvls_nm = [float(table.wvls[w]) for w in wis]
    map_kw, gmaps = None, None
    if bins is None:
        signal = transmission(opt_model, flds, wvls, num_rays, coatings, check_apertures,
                              pupil_maps=False).items['t_sum']
    else:
        # a field's W items add into that field's map, each times its normalised spectral weight
        s_norm = np.asarray(spectral_wts, dtype=np.float64)
        map_kw = dict(slot=-1, weight_row=0, item_factor=np.tile(s_norm / s_norm.sum(), F),
                      item_map=np.repeat(np.arange(F), W), n_maps=F, window=(0.0, 0.0, window[0], window[1]),
                      bins=bins, raw=True)
        results = _trace_packets(eng, fs, wis, opts_list, num_rays)
        rows, item = _transmission_rows(eng, results, flags, wis, _coating_stack_tables(table, coatings, what))
        from .engine import TX_ITEM_DTYPE, records_view
        signal = records_view(item, TX_ITEM_DTYPE)['t_sum'].reshape(F, W)
        swm, _cnt, sexp, _it = eng.weighted_maps(results, flags, weight=rows, **map_kw)
        gmaps = dict(window=window, wmaps=[], scale_exp=[], counts=[], signal_wmaps=swm, signal_scale_exp=sexp)
        del results, rows
    records, slots, kept = [], [], []
    for j, i in found:
        unf = ghost.unfold(table, j, i)
        geng = session.engine_for_table(unf.table)
        gopts = []
        for o in opts_list:
            g = abi.Opts.from_buffer_copy(bytes(o))
            g.last_surf = unf.table.n_ifcs - 2
            gopts.append(g)
        results = _trace_packets(geng, fs, wis, gopts, num_rays)
        rows, _surf, _item = geng.surface_thinfilm(results, flags, wis, wvls_nm, on_device=True,
                                                   **ghost.coating_tables(table, unf, coatings))
        rec = geng.segment_foci(results, flags, weight=rows, weight_row=0, window=window)
        if gmaps is not None:
            wm, cnt, exp, _it = geng.weighted_maps(results, flags, weight=rows, want_counts=True, **map_kw)
            gmaps['wmaps'].append(wm)
            gmaps['scale_exp'].append(exp)
            gmaps['counts'].append(cnt)
        sl = geng.slot_interfaces(flags)
        records.append(rec.reshape(F, W, len(sl)))
        slots.append(dict(source=unf.source[sl], pass_=unf.segment_pass[sl], gap=unf.segment_gap[sl]))
        if keep_packets:
            kept.append(results)
    out = Ghosts(found, skipped, records, slots, signal, spectral_wts, kept if keep_packets else None, gmaps)
    out.trace_flags = flags
    return out


# ---- image simulation: field-varying blur and distortion of a scene ------------------------------
def hat_cells(coord, node):
    """the cell k and fraction t of every coordinate among the strictly increasing ``node``, as
    rox_varying_blur places a pixel (include/roxtrace.h): k = 0, t = 0 before the first node or
    with one node; k = len - 1, t = 0 from the last node on; else node[k] <= coord < node[k + 1]
    and t = (coord - node[k]) / (node[k + 1] - node[k])"""
    coord = np.asarray(coord, dtype=np.float64)
    node = np.asarray(node, dtype=np.float64)
    k = np.zeros(coord.shape, dtype=np.int64)
    t = np.zeros(coord.shape, dtype=np.float64)
    if len(node) > 1:
        last = coord >= node[-1]
        k[last] = len(node) - 1
        mid = ~(coord < node[0]) & ~last
        km = np.searchsorted(node, coord[mid], 'right') - 1
        k[mid] = km
        t[mid] = (coord[mid] - node[km]) / (node[km + 1] - node[km])
    return k, t


def hat_interp(v, node_y, node_x, y, x):
    """node values ``v`` [GY, GX, ...] blended by the hat functions at the points (y, x) (arrays of
    one shape): constant beyond the outermost nodes"""
    v = np.asarray(v, dtype=np.float64)
    k, ty = hat_cells(y, node_y)
    l, tx = hat_cells(x, node_x)
    k1, l1 = np.minimum(k + 1, v.shape[0] - 1), np.minimum(l + 1, v.shape[1] - 1)
    ty = ty.reshape(ty.shape + (1,) * (v.ndim - 2))
    tx = tx.reshape(tx.shape + (1,) * (v.ndim - 2))
    return (1.0 - ty) * ((1.0 - tx) * v[k, l] + tx * v[k, l1]) + ty * ((1.0 - tx) * v[k1, l] + tx * v[k1, l1])


def distortion_displacement(node_y, node_x, err, steps=8):
    """The displacement field rox_image_warp takes, on the node grid, from the distortion ``err``
    [GY, GX, 2] = (real - ideal) chief-ray point at the nodes in pixels (row, column): the light of
    the ideal point q lands at q + e(q), so the output pixel p shows q = p + D with D = -e(p + D),
    solved by ``steps`` fixed-point steps from D = 0, e blended between the nodes by the hat
    functions.  A step shrinks the error by the steepest slope of the blended e (a few per cent
    for a camera lens: under 5 %, eight steps reach 1e-9 px)."""
    err = np.asarray(err, dtype=np.float64)
    py, px = np.meshgrid(np.asarray(node_y, dtype=np.float64), np.asarray(node_x, dtype=np.float64), indexing='ij')
    d = np.zeros_like(err)
    for _ in range(int(steps)):
        d = -hat_interp(err, node_y, node_x, py + d[..., 0], px + d[..., 1])
    return d


def _chief_ray_image_pts(opt_model, flds, wvls, what, prepared=None):
    """[F, W, 2] the image point (x, y) of the chief ray of every (field, wavelength), field-major:
    one small launch (pupil (0, 0) is the first ray of a 2 x 2 grid, and the fixed point of the
    vignetting map) written straight to the host.  ``prepared``: the (engine, fields, wavelength
    indices, options) of _packet_items, else each item is set up as _packet_items does"""
    if prepared is None:
        fs, wis, opts_list = [], [], []
        for fld in flds:
            for wvl in wvls:
                eng, f, wi, opts = _launch_setup(opt_model, fld, wvl, dict(check_apertures=False,
                                                                           apply_vignetting=True), abi.OUT_FULL)
                fs.append(f), wis.append(wi), opts_list.append(opts)
    else:
        eng, fs, wis, opts_list = prepared
    host = eng.trace_pupil_grids_host(fs, wis, make_grid((0., 0.), (1., 1.), 2), opts_list)
    pts = np.empty((len(fs), 2))
    for i, h in enumerate(host):
        if int(h.status[0]) != abi.OK:
            raise ValueError(f'{what}: the chief ray of field {i // len(wvls)} at {wvls[i % len(wvls)]} nm '
                             f'does not reach the image (status {int(h.status[0])})')
        pts[i] = h.seg[-1, 0:2, 0]
    return pts.reshape(len(flds), len(wvls), 2)


class SimulatedImage:
    """What :func:`image_simulation` returns.

    ``image``          [C, H, W] (or [H, W] as the scene came) the simulated picture
    ``blurred``        the picture before the distortion warp (``image`` itself without one)
    ``psfs``           [C, GY, GX, S, S] the PSF stack, tap [a][b] = rows, columns; in HBM
    ``node_px``        (node_y [GY], node_x [GX]) the nodes in pixel coordinates
    ``image_pts``      [node, wvl, 2] the chief-ray image point (x, y) of every node and wavelength
    ``distortion_px``  [GY, GX, 2] (real - ideal) chief-ray point in pixels (row, column), or None
    ``displacement``   [GY, GX, 2] what the warp took (distortion_displacement), or None
    ``gain``           [C, node] the PSF sums: the node's relative transmission, vignetting
                       included, times ``window_share``
    ``window_share``   [C, node] the share of the node's light inside its PSF window (NaN: none)"""

    def __init__(self, image, blurred, psfs, node_px, image_pts, distortion_px, displacement, gain, window_share):
        self.image, self.blurred, self.psfs, self.node_px = image, blurred, psfs, node_px
        self.image_pts, self.distortion_px, self.displacement = image_pts, distortion_px, displacement
        self.gain, self.window_share = gain, window_share


def _field_measure(fov, xy):
    """the quantity the ideal image point is linear in, of field coordinates (x, y) in the units of
    ``fov``: the tangents of the chief ray's direction for an angular field, else the height"""
    x, y = float(xy[0]), float(xy[1])
    if fov.key[1] != 'angle':
        return np.array([x, y])
    ax, ay = np.deg2rad(x), np.deg2rad(y)
    return np.array([np.tan(ax), np.tan(ay) / np.cos(ax)])


def _field_of_measure(fov, u):
    if fov.key[1] != 'angle':
        return float(u[0]), float(u[1])
    ax = np.arctan(u[0])
    return float(np.rad2deg(ax)), float(np.rad2deg(np.arctan(u[1] * np.cos(ax))))


def _simulation_nodes(opt_model, nodes, H, W, pitch, what):
    """a live model's node fields on a regular gy x gx grid of ideal image points spanning the
    picture, edge pixels included -> (fields row-major, node_y, node_x, ideal points [n, 2]).
    The ideal map is linear in the field measure, its slope the real chief-ray image point (at the
    central wavelength) of 1/1024 of the outermost field per unit measure."""
    import copy
    from .trace import aim_chief_rays
    from .workloads import TableModel
    if isinstance(opt_model, TableModel):
        raise ValueError(f'{what}: a TableModel carries prebuilt fields only: pass flds and node_px')
    gy, gx = int(nodes[0]), int(nodes[1])
    if gy < 1 or gx < 1 or gy * gx + 1 > abi.MAX_FOCUS_ITEMS:
        raise ValueError(f'{what}: nodes {nodes!r} outside 1 to {abi.MAX_FOCUS_ITEMS - 1} in all')
    fov = opt_model['osp']['fov']
    scale = float(fov.value) if fov.is_relative else 1.0
    _value, k = fov.max_field()
    outer = fov.fields[k]
    u_outer = _field_measure(fov, (outer.x * scale, outer.y * scale))
    if not np.any(u_outer):
        raise ValueError(f'{what}: the outermost field is on the axis: the ideal map has no slope')

    def field_at(u):
        f = copy.copy(outer)
        x, y = _field_of_measure(fov, u)
        f.x, f.y = x / scale, y / scale
        f.vux = f.vuy = f.vlx = f.vly = 0.0
        f.chief_ray = f.ref_sphere = None
        return f

    def aim(flds):
        for f, a in zip(flds, aim_chief_rays(opt_model, flds)):
            f.aim_info = a

    u_small = u_outer / 1024.0
    probe = [field_at(u_small)]
    aim(probe)
    r_small = _chief_ray_image_pts(opt_model, probe, [opt_model['osp']['wvls'].central_wvl], what)[0, 0]
    slope = float(np.dot(r_small, u_small) / np.dot(u_small, u_small))
    if not (np.isfinite(slope) and slope != 0.0):
        raise ValueError(f'{what}: the chief ray of a small field gives no image scale')
    node_y = np.linspace(0.0, H - 1.0, gy) if gy > 1 else np.array([(H - 1) / 2.0])
    node_x = np.linspace(0.0, W - 1.0, gx) if gx > 1 else np.array([(W - 1) / 2.0])
    ideal = np.array([[(x - (W - 1) / 2.0) * pitch, (y - (H - 1) / 2.0) * pitch] for y in node_y for x in node_x])
    flds = [field_at(r / slope) for r in ideal]
    aim(flds)
    return flds, node_y, node_x, ideal


def image_simulation(opt_model, scene, pixel_pitch, nodes=(5, 5), flds=None, node_px=None, ideal_pts=None, wvls=None,
                     channels=None, num_rays=128, psf_size=33, check_apertures=True, distortion=True, edge='zero',
                     on_device=False, psf='geometric', psf_oversample=3, psf_ref_foc=0.0):
    """What a scene looks like through the lens, on the device: sharp where the lens is sharp,
    soft and darker where it is not, with the colour fringes of lateral colour and the lens's
    distortion.  ``scene`` is [H, W] or [C, H, W]; the image frame's origin is the centre of the
    picture, columns along +x and rows along +y, ``pixel_pitch`` in system units.

    1. Nodes.  On a live model ``nodes`` = (gy, gx) puts node fields on a regular grid of ideal
       image points spanning the picture, edge pixels included: copies of the outermost field
       without vignetting factors, aimed in one batch; the ideal map is linear in the field (in its
       tangents for an angular field), its slope taken from the real chief ray of 1/1024 of the
       outermost field, and assumes a rotationally symmetric lens.  With ``flds`` (gy*gx prebuilt
       fields, row-major) and ``node_px`` = (node_y, node_x) the nodes are taken as given -- a
       workloads.TableModel works this way; ``ideal_pts`` [gy*gx, 2] = (x, y), needed for the
       distortion, is then optional.
    2. One FULL launch of every node x wavelength item, ``num_rays`` x ``num_rays`` rays over the
       node's pupil, and one small launch for their chief rays.
    3. PSFs: per channel one rox_weighted_maps call, one map per node, the node's wavelengths
       its items with the channel's spectral factors -- ``channels`` None: one channel weighted by
       the spectral weights; else a [C, n_wvl] matrix, RGB responses for instance (a [H, W] scene
       is then seen by every channel).  The window of ``psf_size`` bins of one pixel is centred on
       the node's chief-ray image point at the reference (first given, else central) wavelength, so
       lateral colour stays in the PSF.  A ray's weight is the item's spectral factor times the
       share of the unit pupil box the field's vignetting factors leave (a prebuilt field's grid
       covers the shrunken box; a live node has none and the clear apertures vignette).  The stack
       is scaled by the reciprocal of the usable flux (inside the window or not) of the channel's
       brightest node and stays in HBM.
    4. rox_varying_blur and, with ``distortion`` where the ideal points are known,
       rox_image_warp by :func:`distortion_displacement`.

    ``psf='huygens'`` takes step 3 from :func:`trace_huygens_rows` and rox_huygens_psf instead:
    the nodes' diffraction PSFs on the same windows, sampled at ``psf_oversample`` x
    ``psf_oversample`` points per pixel and summed per pixel, each wavelength's PSF scaled to its
    share of the node's usable flux (its spectral factor times the pupil share times the rays that
    arrive), so that a node's PSF sums to its relative transmission as the geometric one does.
    What a diffraction PSF throws outside the window is not known from inside it:
    ``window_share`` is then 1 minus twice the share of the window's outermost ring of samples.
    ``num_rays`` is the pupil sampling (64 is plenty; the default of 128 suits the ray histogram);
    ``psf_ref_foc`` is the focus at which the reference spheres are set up (the picture is still
    taken in the image plane).

    Limits.  With the default ``psf='geometric'`` the PSFs are geometric: right where the spot,
    not the aperture, sets the contrast.  A
    PSF's shape is not stretched by the local distortion.  Vignetting is counted; cos^4 and the
    area change of distortion are not (:func:`relative_illumination` has those).  No coatings.
    A node more than 1 % of whose light misses its window raises a warning: enlarge ``psf_size``.
    Returns :class:`SimulatedImage`; with ``on_device`` its pictures are torch tensors."""
    import warnings
    from .engine import WMAP_ITEM_DTYPE, records_view
    what = 'image_simulation'
    S, pitch = int(psf_size), float(pixel_pitch)
    if not (1 <= S <= abi.MAX_BLUR_TAPS and S % 2 == 1):
        raise ValueError(f'{what}: psf_size {psf_size} is not odd in [1, {abi.MAX_BLUR_TAPS}]')
    if not (np.isfinite(pitch) and pitch > 0.0):
        raise ValueError(f'{what}: pixel_pitch {pixel_pitch!r} is not finite and > 0')
    if edge not in ('zero', 'replicate'):
        raise ValueError(f"{what}: edge is 'zero' or 'replicate', not {edge!r}")
    if psf not in ('geometric', 'huygens'):
        raise ValueError(f"{what}: psf is 'geometric' or 'huygens', not {psf!r}")
    if psf == 'huygens' and not 1 <= int(psf_oversample) <= 16:
        raise ValueError(f'{what}: psf_oversample {psf_oversample} outside [1, 16]')
    if not hasattr(scene, 'shape'):
        scene = np.asarray(scene, dtype=np.float64)
    shape = tuple(int(n) for n in scene.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f'{what}: scene is [H, W] or [C, H, W], not {shape}')
    H, W = shape[-2:]
    if flds is None:
        flds, node_y, node_x, ideal_pts = _simulation_nodes(opt_model, nodes, H, W, pitch, what)
    else:
        if node_px is None:
            raise ValueError(f'{what}: flds needs node_px = (node_y, node_x)')
        node_y = np.asarray(node_px[0], dtype=np.float64).reshape(-1)
        node_x = np.asarray(node_px[1], dtype=np.float64).reshape(-1)
        flds = list(flds)
        if len(flds) != len(node_y) * len(node_x):
            raise ValueError(f'{what}: {len(flds)} flds for {len(node_y)} x {len(node_x)} nodes')
    GY, GX = len(node_y), len(node_x)
    N = GY * GX
    ref_first = wvls is not None and len(wvls) > 0
    eng, flds, wvls, spectral_wts, fs, wis, opts_list, flags = _packet_items(opt_model, flds, wvls, int(num_rays),
                                                                             check_apertures, what)
    Wn = len(wvls)
    factors = np.asarray(spectral_wts if channels is None else channels, dtype=np.float64).reshape(-1, Wn)
    C = factors.shape[0]
    if not (1 <= C <= abi.MAX_BLUR_CHANNELS and np.isfinite(factors).all() and (factors >= 0).all()):
        raise ValueError(f'{what}: channels is [C, {Wn}], finite and >= 0, C in [1, {abi.MAX_BLUR_CHANNELS}]')
    if len(shape) == 3 and shape[0] != C:
        raise ValueError(f'{what}: the scene has {shape[0]} channels, channels {C}')
    t = eng.torch
    scene_t = scene if isinstance(scene, t.Tensor) else t.from_numpy(np.ascontiguousarray(scene, dtype=np.float64))
    scene_t = scene_t.to(device=eng.device, dtype=t.float64).reshape(-1, H, W)
    if len(shape) == 2 and C > 1:
        scene_t = scene_t.expand(C, H, W)
    scene_t = scene_t.contiguous()

    # the chief rays: the window centres, and the distortion
    image_pts = _chief_ray_image_pts(opt_model, flds, wvls, what, (eng, fs, wis, opts_list)).reshape(N, Wn, 2)
    # the reference wavelength of _packet_items: the first one given, else the central one
    ref = 0 if ref_first else wvls.index(float(opt_model['osp']['wvls'].central_wvl))
    centre = image_pts[:, ref]
    window = np.concatenate([centre, np.full((N, 2), S * pitch / 2.0)], axis=1)

    # a field's vignetting factors shrink the pupil box its grid covers: a ray stands for less pupil
    area = np.array([(2.0 - getattr(f, 'vlx', 0.0) - getattr(f, 'vux', 0.0)) / 2.0 *
                     ((2.0 - getattr(f, 'vly', 0.0) - getattr(f, 'vuy', 0.0)) / 2.0) for f in flds])
    if psf == 'huygens':
        psfs, gain, share = _huygens_stack(opt_model, flds, wvls, int(num_rays), check_apertures, centre, S, pitch,
                                           int(psf_oversample), area, factors, (GY, GX), psf_ref_foc, what)
    else:
        results = _trace_packets(eng, fs, wis, opts_list, int(num_rays))
        psfs = t.empty((C, GY, GX, S, S), dtype=t.float64, device=eng.device)
        gain, share = np.zeros((C, N)), np.full((C, N), np.nan)
        for c in range(C):
            maps, _cnt, exp, item = eng.weighted_maps(results, flags,
                                                      item_factor=(area[:, None] * factors[c]).reshape(-1),
                                                      item_map=np.repeat(np.arange(N), Wn), n_maps=N, window=window,
                                                      bins=S, on_device=True)
            flux_in, flux = simulation_flux(records_view(item, WMAP_ITEM_DTYPE), exp.cpu().numpy(), N)
            top = flux.max()
            if top > 0.0:
                # x is the maps' first axis; the product with the reciprocal is one IEEE rounding wherever it runs
                psfs[c] = (maps.transpose(1, 2) * (1.0 / float(top))).reshape(GY, GX, S, S)
                gain[c] = flux_in / top
                share[c] = np.where(flux > 0.0, flux_in / np.where(flux > 0.0, flux, 1.0), np.nan)
            else:
                psfs[c] = 0.0
        del results
    low = np.argwhere(share < 0.99)
    if len(low):
        c, n = low[np.argmin(share[low[:, 0], low[:, 1]])]
        warnings.warn(f'{what}: {len(low)} (channel, node) PSF windows miss more than 1 % of their light '
                      f'(channel {c}, node {n}: {1 - share[c, n]:.1%}): enlarge psf_size', stacklevel=2)

    blurred = eng.varying_blur(scene_t, psfs, node_y, node_x, edge=edge, on_device=True)
    image, err, disp = blurred, None, None
    if ideal_pts is not None:
        ideal = np.asarray(ideal_pts, dtype=np.float64).reshape(N, 2)
        err = ((centre - ideal) / pitch)[:, ::-1].reshape(GY, GX, 2)        # (x, y) -> (row, column)
        if distortion:
            disp = distortion_displacement(node_y, node_x, err)
            image = eng.image_warp(blurred, node_y, node_x, disp, on_device=True)
    if len(shape) == 2 and C == 1:
        image, blurred = image[0], blurred[0]
    if not on_device:
        blurred = blurred.cpu().numpy()
        image = blurred if disp is None else image.cpu().numpy()
    elif disp is None:
        image = blurred
    return SimulatedImage(image, blurred, psfs, (node_y, node_x), image_pts, err, disp, gain, share)


def _huygens_stack(opt_model, flds, wvls, num_rays, check_apertures, centre, S, pitch, over, area, factors, nodes,
                   ref_foc, what):
    """the PSF stack [C, GY, GX, S, S] of image_simulation(psf='huygens'), its gains and window
    shares [C, N]: every (node, wavelength) item's Huygens PSF at ``over`` x ``over`` points per
    pixel of the node's window (bin a of the window spans centre - S pitch / 2 + [a, a + 1] pitch,
    as the geometric maps' bins do), summed per pixel and divided by its sum over the window, then
    weighted by the item's share of the usable flux of the channel's brightest node"""
    hr = trace_huygens_rows(opt_model, flds, wvls, num_rays, check_apertures, ref_foc, what)
    eng, t = hr.eng, hr.eng.torch
    GY, GX = nodes
    N, Wn, C = len(flds), len(wvls), factors.shape[0]
    n_s, p_s = S * over, pitch / over
    origins = np.asarray(centre, dtype=np.float64) - S * pitch / 2.0 + p_s / 2.0
    planes = huygens_planes(hr.centres, origins, [0.0], Wn)
    fine, _field, stats = eng.huygens_psf(hr.rows, hr.status, planes, n_s, n_s, p_s, p_s, n_rays=hr.n_rays)
    fine = fine.reshape(N, Wn, n_s, n_s)
    ring = fine[:, :, 0, :].sum(-1) + fine[:, :, -1, :].sum(-1) + fine[:, :, 1:-1, 0].sum(-1) + fine[:, :, 1:-1, -1].sum(-1)
    pix = fine.reshape(N, Wn, S, over, S, over).sum(dim=(3, 5))
    total = pix.sum(dim=(2, 3))
    unit = t.where(total > 0.0, 1.0 / t.where(total > 0.0, total, t.ones_like(total)), t.zeros_like(total))
    pix = (pix * unit[:, :, None, None]).transpose(2, 3)             # rows along y, columns along x
    n_ok = stats['n'].reshape(N, Wn).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        ring_share = np.where(stats['sum'].reshape(N, Wn) > 0.0,
                              ring.cpu().numpy() / stats['sum'].reshape(N, Wn), 0.0)
    psfs = t.zeros((C, GY, GX, S, S), dtype=t.float64, device=eng.device)
    gain, share = np.zeros((C, N)), np.full((C, N), np.nan)
    for c in range(C):
        flux_w = area[:, None] * factors[c][None, :] * n_ok                      # [N, Wn]
        flux = flux_w.sum(axis=1)
        top = flux.max()
        if not top > 0.0:
            continue
        w = t.from_numpy(flux_w / top).to(eng.device)
        psfs[c] = (pix * w[:, :, None, None]).sum(dim=1).reshape(GY, GX, S, S)
        gain[c] = flux / top
        with np.errstate(invalid='ignore', divide='ignore'):
            share[c] = np.where(flux > 0.0, 1.0 - 2.0 * (flux_w * ring_share).sum(axis=1) / flux, np.nan)
    return psfs, gain, share


def simulation_flux(item, scale_exp, n_nodes):
    """(the flux inside the window, the usable flux) [n_nodes] of the nodes' maps from the item
    records and scale exponents of image_simulation's rox_weighted_maps call (items node-major):
    the integer sums of a node's items, converted as the maps are"""
    q_in = item['q_in'].reshape(n_nodes, -1).sum(axis=1)
    q_all = q_in + item['q_out'].reshape(n_nodes, -1).sum(axis=1)
    e = -np.asarray(scale_exp, dtype=np.int64)
    return np.ldexp(q_in.astype(np.float64), e), np.ldexp(q_all.astype(np.float64), e)


# ---- tolerancing from one trace: wavefront differentials ----------------------------------------
def _compensator(pert, c):
    """a compensator -> (name, coefficient vector): 'focus' (the image slot's dz), 'image_x' /
    'image_y', ('thickness', g), or a tolerance.Tolerance"""
    if c == 'focus':
        return 'focus', pert.surface_decenter(pert.image, 'z')
    if c in ('image_x', 'image_y'):
        return c, pert.surface_decenter(pert.image, c[-1])
    if isinstance(c, tuple) and len(c) == 2 and c[0] == 'thickness':
        return f'thickness {int(c[1])}', pert.thickness(int(c[1]))
    if hasattr(c, 'coef') and hasattr(c, 'name'):
        return c.name, c.coef
    raise ValueError(f"tolerance_sensitivity: compensator {c!r} is not 'focus', 'image_x', 'image_y', "
                     "('thickness', g) or a Tolerance")


def tolerance_sensitivity(opt_model, tolerances=None, flds=None, wvls=None, num_rays=64, compensators=('focus',),
                          check_apertures=True, keep_cols=False, foc=0.0, grade='commercial', field_wts=None):
    """As-built performance from ONE nominal trace (rox_wave_differentials): one FULL launch over
    every (field, wavelength) -- ``num_rays`` x ``num_rays`` rays over each field's vignetted
    pupil, as beam_footprints traces them -- one through-focus launch of the same grid with the
    one plane ``foc`` for the nominal OPD, and one wave_differentials call with the OPD in waves
    and the pupil coordinates as aux rows.  The rest is host algebra on the covariance of the
    per-ray columns (tolerance.Quadratic): the RMS wavefront per field with every tolerance at
    +- its magnitude after the ``compensators`` ('focus', 'image_x', 'image_y', ('thickness', g)
    or a Tolerance; one value for all fields and wavelengths) have been set, RSS, Monte Carlo.
    ``tolerances``: tolerance.Tolerance objects, or a callable taking the tolerance.Perturbations
    of this call and returning them; None: tolerance.default_tolerances(``grade``).  First order:
    the object-space rays are kept, the stop is not re-aimed, and a term of order (transverse
    aberration x change of ray angle) is left out.  Returns
    :class:`tolerance.ToleranceSensitivity`."""
    from . import tolerance as T
    from .trace import _launch_setup
    what = 'tolerance_sensitivity'
    num_rays = int(num_rays)
    eng, flds, wvls, spectral_wts, fs, wis, opts_list, flags = _packet_items(opt_model, flds, wvls, num_rays,
                                                                             check_apertures, what)
    F, W = len(flds), len(wvls)
    results = _trace_packets(eng, fs, wis, opts_list, num_rays)
    grid = make_grid((-1., -1.), (1., 1.), num_rays)
    planes, f2, w2, o2 = [], [], [], []
    for fld in flds:
        for wvl in wvls:
            planes.append(_focus_planes(opt_model, fld, wvl, [float(foc)]))
            kw = dict(check_apertures=bool(check_apertures), apply_vignetting=True)
            _eng, f, wi, opts = _launch_setup(opt_model, fld, wvl, kw, abi.OUT_FAN)
            f2.append(f)
            w2.append(wi)
            o2.append(opts)
    _stats, rows = eng.trace_pupil_grids_focus(f2, w2, [grid] * (F * W), o2, planes, want_rows=True)
    t = eng.torch
    R = num_rays * num_rays
    scale = t.from_numpy(_wave_scales(opt_model, wvls, F * W)).to(rows.rows.device)
    ax = t.linspace(-1.0, 1.0, num_rays, dtype=t.float64, device=rows.rows.device)
    aux = t.empty((F * W, 3, R), dtype=t.float64, device=rows.rows.device)
    aux[:, 0] = rows.rows[:, 0, 2, :R] * scale[:, None]
    aux[:, 1] = ax.repeat_interleave(num_rays)[None, :]
    aux[:, 2] = ax.repeat(num_rays)[None, :]
    item, pivot, sums, gram, cols = eng.wave_differentials(results, flags, wis, aux=aux, want_cols=keep_cols)
    if (item['n'] < 2).any():
        raise ValueError(f'{what}: an item has fewer than two rays through (n = {item["n"].tolist()})')
    pert = T.Perturbations(eng.table, None, 3, wis, flags)
    if tolerances is None:
        tolerances = T.default_tolerances(pert, grade, units_per_nm=opt_model.nm_to_sys_units(1.0),
                                          ref_wvl_idx=wis[0])
    elif callable(tolerances):
        tolerances = tolerances(pert)
    tolerances = list(tolerances)
    comps = [_compensator(pert, c) for c in compensators]
    n_cols = pert.n_cols
    cov = T.covariances(item, sums, gram).reshape(F, W, n_cols, n_cols)
    if field_wts is None:
        field_wts = [getattr(f, 'wt', 1.0) for f in flds]
    quad = T.Quadratic(cov, _wave_scales(opt_model, wvls, F * W), [tol.coef for tol in tolerances],
                       [c for _n, c in comps], spectral_wts, field_wts)
    return T.ToleranceSensitivity(tolerances, [n for n, _c in comps], quad, item, pivot, sums, gram, flds, wvls,
                                  image_cols=(pert.col(-1, 'dx'), pert.col(-1, 'dy')), cols=cols, num_rays=num_rays)


# ---- MTF through focus ----------------------------------------------------------
# the PSF stack through_focus_mtf holds at once: larger maps run rox_focus_psf / rox_focus_mtf
# over consecutive groups of items (the results do not depend on the grouping)
MTF_PSF_CHUNK_BYTES = 512 << 20


def _check_freqs(freqs, what):
    nu = np.asarray(freqs, dtype=np.float64).reshape(-1)
    if not 1 <= nu.size <= abi.MAX_MTF_FREQS:
        raise ValueError(f'{what}: 1 to {abi.MAX_MTF_FREQS} frequencies, got {nu.size}')
    if not (np.isfinite(nu).all() and (nu >= 0).all()):
        raise ValueError(f'{what}: frequencies must be finite and >= 0, got {nu}')
    return nu


def _given_pitch(pitch, shape, what):
    """a given pixel pitch as float64 broadcast to shape, checked (None stays None)"""
    if pitch is None:
        return None
    pitch = np.array(np.broadcast_to(np.asarray(pitch, dtype=np.float64), shape))
    if not (np.isfinite(pitch).all() and (pitch > 0).all()):
        raise ValueError(f'{what}: pitch must be finite and > 0')
    return pitch


def _default_pitch(opt_model, wvls, num_rays, maxdim, radii, shape, what):
    """[F, W, K] calc_psf_scaling's delta_xp of every plane, radii[i] being item i's reference
    sphere radii"""
    W = len(wvls)
    scal = [[psf_scaling(opt_model, wvls[i % W], num_rays, maxdim, r) for r in rs] for i, rs in enumerate(radii)]
    if any(x is None for xs in scal for x in xs):
        raise ValueError(f'{what}: the model has no paraxial data for calc_psf_scaling: pass pitch [F, W, K]')
    return np.array([[x[1] for x in xs] for xs in scal], dtype=np.float64).reshape(shape)


def poly_otf_merge(otf, image_pts, spectral_wts, ref_index, freqs, dirs=None):
    """the polychromatic line OTFs [K, 2, Q] of one field from its per-wavelength OTFs.

    otf         [W, K, 2, Q] complex: each wavelength's line OTFs along image x and y, phase
                about that wavelength's own image point
    image_pts   [W, K, 2] each plane's image point
    spectral_wts  [W] weights s_w;  ref_index: the wavelength whose image point is the origin

    poly_otf(nu) = sum_w s_w exp(-2 pi i nu D_w) OTF_w(nu) / sum_w s_w, D_w the component of
    image_pt_w - image_pt_ref along the direction, so lateral colour counts.  Entries whose OTF is
    NaN are skipped and the remaining weights renormalised; none left -> NaN.  One wavelength
    gives its own OTF exactly (its weight is 1 and its phase factor exp(0) = 1).

    ``dirs`` [D, 2] = (ex, ey): the OTFs are [W, K, D, Q] along these directions (the geometric
    OTFs of rox_focus_gmtf) and D_w = ex * dx + ey * dy of image_pt_w - image_pt_ref.  None: x
    and y."""
    otf = np.asarray(otf, dtype=np.complex128)
    W, K, _two, Q = otf.shape
    ip = np.asarray(image_pts, dtype=np.float64).reshape(W, K, 2)
    nu = np.asarray(freqs, dtype=np.float64).reshape(Q)
    delta = ip - ip[ref_index][None]                                    # [W, K, 2]
    if dirs is not None:
        e = np.asarray(dirs, dtype=np.float64).reshape(-1, 2)
        if e.shape[0] != otf.shape[2]:
            raise ValueError(f'poly_otf_merge: {e.shape[0]} directions for OTFs along {otf.shape[2]}')
        delta = e[:, 0] * delta[..., 0:1] + e[:, 1] * delta[..., 1:2]   # [W, K, D]
    shifted = np.exp(-2j * np.pi * delta[..., None] * nu) * otf          # [W, K, 2, Q]
    ok = ~np.isnan(otf)
    s = np.where(ok, np.asarray(spectral_wts, dtype=np.float64).reshape(W, 1, 1, 1), 0.0)
    total = s.sum(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        wt = s / total
    out = np.where(ok, wt * shifted, 0.0).sum(axis=0)
    return np.where(total > 0, out, np.nan + 0j)


class ThroughFocusMTF:
    """what :func:`through_focus_mtf` returns.

    focs, freqs, wvls, field_wts, spectral_wts, ref_wvl   as used
    otf         [F, W, K, 2, Q] complex: the line OTFs of each PSF along image x (direction 0)
                and y (1) -- rox_focus_mtf: the DTFT of the PSF's projection, phase in image
                coordinates about the plane's image point; NaN above a plane's Nyquist
                frequency 1 / (2 pitch) and on planes no ray reached
    mtf         [F, W, K, 2, Q] abs(otf)
    pitch       [F, W, K] each PSF's pixel pitch (calc_psf_scaling's delta_xp at that focus)
    image_pts   [F, W, K, 2] each plane's image point
    strehl      [F, W, K] each plane's Strehl ratio (rox_focus_psf)
    poly_otf / poly_mtf [F, K, 2, Q]: :func:`poly_otf_merge` of each field's wavelengths
    best_focus  [F, 2, Q] (+ ``_kind``): :func:`best_focus` of -poly_mtf per field, direction
                and frequency
    best_focus_all [Q] (+ ``_kind``): the same of the field-weighted mean over both directions
    meridional  [F] True for a field whose image points stay in the y-z plane (x == 0 at every
                wavelength and focus): there y is tangential and x sagittal
    tangential / sagittal [F, K, Q]: poly_mtf along y / x for meridional fields, NaN rows for
                the others (their tangential direction is neither x nor y)
    psf         [F, W, K, maxdim, maxdim] with ``psf=True`` (a torch tensor in HBM with
                ``on_device=True``), else None"""

    def __init__(self, focs, freqs, wvls, field_wts, spectral_wts, ref_wvl, otf, pitch, image_pts, strehl,
                 psf=None):
        self.focs = np.asarray(focs, dtype=np.float64)
        self.freqs = np.asarray(freqs, dtype=np.float64)
        self.wvls = list(wvls)
        self.field_wts = np.asarray(field_wts, dtype=np.float64)
        self.spectral_wts = np.asarray(spectral_wts, dtype=np.float64)
        self.ref_wvl = ref_wvl
        self.otf = otf
        self.mtf = np.abs(otf)
        self.pitch = pitch
        self.image_pts = image_pts
        self.strehl = strehl
        self.psf = psf
        F, _W, K, _two, Q = otf.shape
        ref = self.wvls.index(ref_wvl)
        self.poly_otf = np.stack([poly_otf_merge(otf[f], image_pts[f], self.spectral_wts, ref, self.freqs)
                                  for f in range(F)])
        self.poly_mtf = np.abs(self.poly_otf)
        self.best_focus = np.empty((F, 2, Q))
        self.best_focus_kind = np.empty((F, 2, Q), dtype=object)
        for f in range(F):
            for d in range(2):
                for q in range(Q):
                    self.best_focus[f, d, q], self.best_focus_kind[f, d, q] = best_focus(
                        self.focs, -self.poly_mtf[f, :, d, q])
        mean = self.poly_mtf.mean(axis=2)                                   # [F, K, Q] both directions
        wt = self.field_wts[:, None, None]
        curve = (wt * mean).sum(axis=0) / self.field_wts.sum()              # [K, Q]
        res = [best_focus(self.focs, -curve[:, q]) for q in range(Q)]
        self.best_focus_all = np.array([r[0] for r in res])
        self.best_focus_all_kind = np.array([r[1] for r in res], dtype=object)
        self.meridional = np.all(np.asarray(image_pts)[..., 0] == 0.0, axis=(1, 2))

    def _view(self, d):
        out = np.full(self.poly_mtf.shape[:2] + self.poly_mtf.shape[3:], np.nan)
        out[self.meridional] = self.poly_mtf[self.meridional, :, d, :]
        return out

    @property
    def tangential(self):
        """[F, K, Q] the polychromatic MTF along y of the meridional fields (NaN rows elsewhere)"""
        return self._view(1)

    @property
    def sagittal(self):
        """[F, K, Q] the polychromatic MTF along x of the meridional fields (NaN rows elsewhere)"""
        return self._view(0)


def through_focus_mtf(opt_model, focs, freqs, flds=None, wvls=None, num_rays=32, maxdim=128, field_wts=None,
                      spectral_wts=None, ref_wvl=None, psf=False, on_device=False, pitch=None, **kwargs):
    """The MTF through focus, along image x and y, of every field at every wavelength, and its
    polychromatic merge per field, on the device: one rox_trace_through_focus_grids launch traces
    each item's square pupil grid (as :func:`through_focus_psf`) and evaluates it at every focus,
    rox_focus_psf turns the rows into PSFs (each calc_psf of that focus's focus_wavefront grid),
    and rox_focus_mtf takes the line OTFs of every PSF at ``freqs`` (cycles per system unit) --
    the PSFs stay in HBM.  The merge over wavelengths follows on the host
    (:class:`ThroughFocusMTF`).  Fields, wavelengths and weights default as in
    :func:`through_focus_map`.  Each PSF's pitch is calc_psf_scaling's delta_xp at its focus; a
    model without paraxial data (a workloads.TableModel) needs ``pitch`` [F, W, K].  ``maxdim``
    must be at least 2 ``num_rays``: below that the pupil autocorrelation wraps and the MTF is
    aliased.  ``psf=True`` keeps the PSFs (in HBM with ``on_device=True``)."""
    from .engine import grid_rays
    what = 'through_focus_mtf'
    focs = _check_focs(focs, what)
    num_rays, maxdim = int(num_rays), int(maxdim)
    if num_rays < 2 or num_rays % 2:
        raise ValueError(f'{what}: num_rays must be even and >= 2, got {num_rays}')
    if maxdim < 2 * num_rays:
        raise ValueError(f'{what}: maxdim {maxdim} < 2 num_rays = {2 * num_rays}: the pupil autocorrelation '
                         f'would wrap (an aliased MTF)')
    if not _psf_block_fits(num_rays, maxdim):
        raise ValueError(f'{what}: the {num_rays} x {num_rays} grid does not fit in maxdim {maxdim}')
    nu = _check_freqs(freqs, what)
    flds, wvls, field_wts, spectral_wts, ref_wvl = _map_spec(opt_model, flds, wvls, field_wts, spectral_wts,
                                                             ref_wvl, what)
    F, W, K = len(flds), len(wvls), len(focs)
    pitch = _given_pitch(pitch, (F, W, K), what)
    radii = []
    eng, fs, wis, grids, opts_list, planes = _map_items(opt_model, flds, wvls, focs, None, num_rays, kwargs,
                                                        radii=radii)
    assert grid_rays(grids[0]) == num_rays * num_rays
    if pitch is None:
        pitch = _default_pitch(opt_model, wvls, num_rays, maxdim, radii, (F, W, K), what)
    _none, dev_rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True,
                                                  want_stats=False)
    scale = _wave_scales(opt_model, wvls, F * W)
    flat_pitch = pitch.reshape(F * W, K)
    per_item = K * maxdim * maxdim * 8
    step = max(1, MTF_PSF_CHUNK_BYTES // per_item)
    from .engine import FocusRows
    otf, strehl, psfs = [], [], []
    for i0 in range(0, F * W, step):
        i1 = min(F * W, i0 + step)
        part = FocusRows(dev_rows.rows[i0:i1], dev_rows.status[i0:i1])
        dev_psf, psf_stats = eng.focus_psf(part, num_rays, maxdim, scale[i0:i1], want_psf=True)
        otf.append(eng.focus_mtf(dev_psf, flat_pitch[i0:i1], nu))
        strehl.append(psf_stats['strehl'])
        if psf:
            psfs.append(dev_psf if on_device else dev_psf.cpu().numpy())
        del dev_psf
    otf = np.concatenate(otf).reshape(F, W, K, 2, nu.size)
    strehl = np.concatenate(strehl).reshape(F, W, K)
    image_pts = _image_pts(planes).reshape(F, W, K, 2)
    out_psf = None
    if psf:
        if on_device:
            import torch
            out_psf = torch.cat(psfs).reshape(F, W, K, maxdim, maxdim)
        else:
            out_psf = np.concatenate(psfs).reshape(F, W, K, maxdim, maxdim)
    return ThroughFocusMTF(focs, nu, wvls, field_wts, spectral_wts, ref_wvl, otf, pitch, image_pts, strehl,
                           out_psf)


# ---- geometric MTF and line spread through focus -------------------------------------------
def gmtf_directions(directions, image_pts_ref):
    """the direction vectors [F, D, 2] of :func:`through_focus_gmtf`: each of ``directions`` is
    'x' = (1, 0), 'y' = (0, 1), 't' (tangential: the unit vector from the axis to the field's
    image point ``image_pts_ref[f]``, (0, 1) for a field on the axis), 's' (sagittal:
    (t_y, -t_x)) or an explicit (ex, ey), taken as given -- a unit vector keeps the frequencies in
    cycles per system unit.  Returns (dirs, labels)."""
    what = 'through_focus_gmtf'
    if isinstance(directions, str):
        directions = (directions,)
    directions = list(directions)
    if not 1 <= len(directions) <= abi.MAX_GMTF_DIRS:
        raise ValueError(f'{what}: 1 to {abi.MAX_GMTF_DIRS} directions, got {len(directions)}')
    ip = np.asarray(image_pts_ref, dtype=np.float64).reshape(-1, 2)
    F = ip.shape[0]
    r = np.hypot(ip[:, 0], ip[:, 1])
    on_axis = ~(r > 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        t = np.where(on_axis[:, None], np.array([0.0, 1.0]), ip / r[:, None])
    sag = np.stack([t[:, 1], -t[:, 0]], axis=-1) + 0.0                  # (+ 0.0: no -0)
    dirs = np.empty((F, len(directions), 2))
    labels = []
    for d, spec in enumerate(directions):
        if isinstance(spec, str):
            if spec not in ('x', 'y', 't', 's'):
                raise ValueError(f"{what}: a direction is 'x', 'y', 't', 's' or (ex, ey), got {spec!r}")
            dirs[:, d] = {'x': np.array([1.0, 0.0]), 'y': np.array([0.0, 1.0]), 't': t, 's': sag}[spec]
            labels.append(spec)
            continue
        try:
            v = np.asarray(spec, dtype=np.float64)
        except (TypeError, ValueError):
            v = np.empty(0)
        if v.shape != (2,) or not np.isfinite(v).all() or not v.any():
            raise ValueError(f"{what}: a direction is 'x', 'y', 't', 's' or a finite non-zero (ex, ey), got {spec!r}")
        dirs[:, d] = v
        labels.append((float(v[0]), float(v[1])))
    return dirs, labels


def lsf_edges(center, half_width, bins):
    """[..., bins + 1] edges of ``bins`` equal bins over center -+ half_width"""
    c = np.asarray(center, dtype=np.float64)[..., None]
    h = np.asarray(half_width, dtype=np.float64)[..., None]
    return c + h * np.linspace(-1.0, 1.0, int(bins) + 1)


def poly_lsf_merge(lsf, n_ok, spectral_wts):
    """[W, K, D, B] ray counts per bin and [W, K] ray totals of one field ->
    sum_w s_w lsf_w / n_w / sum_w s_w [K, D, B], the unit-energy line spread whose transform
    :func:`poly_otf_merge` gives; wavelengths with no ray are skipped and the rest renormalised,
    none left -> NaN"""
    lsf = np.asarray(lsf, dtype=np.float64)
    n = np.asarray(n_ok, dtype=np.float64)
    W = n.shape[0]
    s = np.where(n > 0, np.asarray(spectral_wts, dtype=np.float64).reshape(W, 1), 0.0)     # [W, K]
    total = s.sum(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        per = np.where(n[..., None, None] > 0, lsf / n[..., None, None], 0.0)
        out = (s[..., None, None] * per).sum(axis=0) / total[:, None, None]
    return np.where(total[:, None, None] > 0, out, np.nan)


class ThroughFocusGMTF:
    """what :func:`through_focus_gmtf` returns.

    focs, freqs, wvls, field_wts, spectral_wts, ref_wvl, directions   as used
    dirs        [F, D, 2] each field's direction vectors (ex, ey)
    otf         [F, W, K, D, Q] complex: the geometric OTF of each spot along each direction --
                rox_focus_gmtf: the mean of exp(-2 pi i nu u) over the rays, u = ex x + ey y about
                the plane's image point; NaN on planes no ray reached
    mtf         [F, W, K, D, Q] abs(otf)
    n_ok        [F, W, K] OK rays per plane
    image_pts   [F, W, K, 2] each plane's image point
    poly_otf / poly_mtf [F, K, D, Q]: :func:`poly_otf_merge` of each field's wavelengths along
                its directions
    best_focus  [F, D, Q] (+ ``_kind``): :func:`best_focus` of -poly_mtf per field, direction
                and frequency
    best_focus_all [Q] (+ ``_kind``): the same of the field-weighted mean over the directions
    tangential / sagittal [F, K, Q]: poly_mtf along 't' / 's', for every field (None when that
                direction was not asked for)
    With ``lsf_bins`` (else None):
    lsf         [F, W, K, D, B] ray counts per bin
    lsf_edges   [F, K, D, B + 1] the bin edges along each direction, in the reference
                wavelength's coordinates (about its image point)
    poly_lsf    [F, K, D, B] :func:`poly_lsf_merge` of each field's wavelengths: the fraction of
                the light in each bin
    esf         [F, K, D, B] its cumulative sum (the edge spread at each bin's right edge)
    lsf_inside  [F, K, D] the fraction of the light inside the edges"""

    def __init__(self, focs, freqs, wvls, field_wts, spectral_wts, ref_wvl, directions, dirs, otf, n_ok,
                 image_pts, lsf=None, lsf_edges=None):
        self.focs = np.asarray(focs, dtype=np.float64)
        self.freqs = np.asarray(freqs, dtype=np.float64)
        self.wvls = list(wvls)
        self.field_wts = np.asarray(field_wts, dtype=np.float64)
        self.spectral_wts = np.asarray(spectral_wts, dtype=np.float64)
        self.ref_wvl = ref_wvl
        self.directions = list(directions)
        self.dirs = np.asarray(dirs, dtype=np.float64)
        self.otf = otf
        self.mtf = np.abs(otf)
        self.n_ok = n_ok
        self.image_pts = image_pts
        F, _W, K, D, Q = otf.shape
        ref = self.wvls.index(ref_wvl)
        self.poly_otf = np.stack([poly_otf_merge(otf[f], image_pts[f], self.spectral_wts, ref, self.freqs,
                                                 dirs=self.dirs[f]) for f in range(F)])
        self.poly_mtf = np.abs(self.poly_otf)
        self.best_focus = np.empty((F, D, Q))
        self.best_focus_kind = np.empty((F, D, Q), dtype=object)
        for f in range(F):
            for d in range(D):
                for q in range(Q):
                    self.best_focus[f, d, q], self.best_focus_kind[f, d, q] = best_focus(
                        self.focs, -self.poly_mtf[f, :, d, q])
        mean = self.poly_mtf.mean(axis=2)                                   # [F, K, Q] every direction
        wt = self.field_wts[:, None, None]
        curve = (wt * mean).sum(axis=0) / self.field_wts.sum()              # [K, Q]
        res = [best_focus(self.focs, -curve[:, q]) for q in range(Q)]
        self.best_focus_all = np.array([r[0] for r in res])
        self.best_focus_all_kind = np.array([r[1] for r in res], dtype=object)
        self.lsf = lsf
        self.lsf_edges = lsf_edges
        self.poly_lsf = self.esf = self.lsf_inside = None
        if lsf is not None:
            self.poly_lsf = np.stack([poly_lsf_merge(lsf[f], n_ok[f], self.spectral_wts) for f in range(F)])
            self.esf = np.cumsum(self.poly_lsf, axis=-1)
            self.lsf_inside = self.poly_lsf.sum(axis=-1)

    def _along(self, label):
        if label not in self.directions:
            return None
        return self.poly_mtf[:, :, self.directions.index(label), :]

    @property
    def tangential(self):
        """[F, K, Q] the polychromatic MTF along each field's tangential direction"""
        return self._along('t')

    @property
    def sagittal(self):
        """[F, K, Q] the polychromatic MTF along each field's sagittal direction"""
        return self._along('s')


def through_focus_gmtf(opt_model, focs, freqs, flds=None, wvls=None, num_rays=64,
                       directions=('x', 'y', 't', 's'), lsf_bins=0, lsf_half_width=None, field_wts=None,
                       spectral_wts=None, ref_wvl=None, **kwargs):
    """The geometric MTF through focus -- the transform of the ray spot, the tool for a lens far
    from the diffraction limit -- of every field at every wavelength, and its polychromatic merge
    per field, on the device: one rox_trace_through_focus_grids launch traces each item's square
    pupil grid (``num_rays`` across) and evaluates it at every focus, and one rox_focus_gmtf call
    sums exp(-2 pi i nu u) over the rows in HBM, at any ``freqs`` (cycles per system unit; no
    Nyquist limit) and along any ``directions`` (:func:`gmtf_directions`: 'x', 'y', 't', 's' or
    (ex, ey); 't' of a field points from the axis to its image point at ``ref_wvl`` and the focus
    nearest 0).  Fields, wavelengths and weights default as in :func:`through_focus_map`.

    ``lsf_bins`` > 0 adds the line spread function: the rays of each plane binned along each
    direction into ``lsf_bins`` equal bins over -+ ``lsf_half_width`` about the field's
    polychromatic spot centroid (:func:`poly_merge`, lateral colour included); the default half
    width is 3 times the field's largest polychromatic RMS spot over the foci.
    Returns a :class:`ThroughFocusGMTF`."""
    from .engine import grid_rays
    what = 'through_focus_gmtf'
    focs = _check_focs(focs, what)
    nu = _check_freqs(freqs, what)
    num_rays = int(num_rays)
    if num_rays < 1:
        raise ValueError(f'{what}: num_rays must be >= 1, got {num_rays}')
    lsf_bins = int(lsf_bins)
    if not 0 <= lsf_bins <= abi.MAX_LSF_BINS:
        raise ValueError(f'{what}: lsf_bins {lsf_bins} outside [0, {abi.MAX_LSF_BINS}]')
    if lsf_half_width is not None:
        hw = np.asarray(lsf_half_width, dtype=np.float64)
        if hw.ndim > 1 or not (np.isfinite(hw).all() and (hw > 0).all()):
            raise ValueError(f'{what}: lsf_half_width must be finite and > 0 (one, or one per field)')
    gmtf_directions(directions, [(0.0, 0.0)])                               # checked before any device work
    flds, wvls, field_wts, spectral_wts, ref_wvl = _map_spec(opt_model, flds, wvls, field_wts, spectral_wts,
                                                             ref_wvl, what)
    F, W, K = len(flds), len(wvls), len(focs)
    if lsf_half_width is not None and hw.ndim == 1 and hw.size != F:
        raise ValueError(f'{what}: lsf_half_width must be finite and > 0 (one, or one per field)')
    s = np.asarray(spectral_wts, dtype=np.float64)
    eng, fs, wis, grids, opts_list, planes = _map_items(opt_model, flds, wvls, focs, None, num_rays, kwargs)
    R = grid_rays(grids[0])
    image_pts = _image_pts(planes).reshape(F, W, K, 2)
    ref = wvls.index(ref_wvl)
    k0 = int(np.argmin(np.abs(focs)))
    dirs, labels = gmtf_directions(directions, image_pts[:, ref, k0])
    D = len(labels)
    stats, dev_rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True)
    item_dirs = np.repeat(dirs, W, axis=0)                                  # [F W, D, 2]
    edges = ref_edges = None
    if lsf_bins:
        stats = stats.reshape(F, W, K)
        pm = [poly_merge(stats[f], image_pts[f], s, ref) for f in range(F)]
        C = np.stack([np.stack([m['cx'], m['cy']], axis=-1) for m in pm])   # [F, K, 2] absolute
        if lsf_half_width is None:
            rms = [m['rms_spot'][np.isfinite(m['rms_spot'])] for m in pm]
            hw = 3.0 * np.array([r.max() if r.size else np.nan for r in rms])
            if not (np.isfinite(hw).all() and (hw > 0).all()):
                raise ValueError(f'{what}: no default lsf_half_width for a field whose spot has no size: pass one')
        hw = np.broadcast_to(hw, (F,))
        about = np.nan_to_num(C - image_pts[:, ref])                        # [F, K, 2] in ref coordinates
        center = dirs[:, None, :, 0] * about[:, :, None, 0] + dirs[:, None, :, 1] * about[:, :, None, 1]
        ref_edges = lsf_edges(center, hw[:, None, None], lsf_bins)          # [F, K, D, B + 1]
        # each wavelength's rows are about its own image point
        delta = image_pts - image_pts[:, ref][:, None]                      # [F, W, K, 2]
        shift = dirs[:, None, None, :, 0] * delta[..., None, 0] + dirs[:, None, None, :, 1] * delta[..., None, 1]
        edges = (ref_edges[:, None] - shift[..., None]).reshape(F * W, K, D, lsf_bins + 1)
        if not (np.diff(edges, axis=-1) > 0).all():
            raise ValueError(f'{what}: lsf_half_width {hw} over {lsf_bins} bins gives no increasing edges')
    otf, lsf, n_ok = eng.focus_gmtf(dev_rows, R, item_dirs, nu, edges=edges)
    return ThroughFocusGMTF(focs, nu, wvls, field_wts, spectral_wts, ref_wvl, labels, dirs,
                            otf.reshape(F, W, K, D, nu.size), n_ok.reshape(F, W, K), image_pts,
                            lsf=None if lsf is None else lsf.reshape(F, W, K, D, lsf_bins), lsf_edges=ref_edges)


# ---- encircled energy through focus ---------------------------------------------------------
def curve_radius(radii, curve, fraction):
    """the radius at which a sampled encircled-energy curve first reaches ``fraction``: linear
    interpolation inside the first segment that crosses it (the first sample when it already
    does); NaN when the curve never reaches it or holds NaN"""
    r = np.asarray(radii, dtype=np.float64)
    e = np.asarray(curve, dtype=np.float64)
    if np.isnan(e).any():
        return float('nan')
    hit = np.nonzero(e >= fraction)[0]
    if not hit.size:
        return float('nan')
    j = int(hit[0])
    if j == 0:
        return float(r[0])
    t = (fraction - e[j - 1]) / (e[j] - e[j - 1])
    return float(r[j - 1] + t * (r[j] - r[j - 1]))


def _curve_radii(radii, curves, fractions):
    """curve_radius over [..., n] radii and curves -> [..., Nf]"""
    r = np.asarray(radii, dtype=np.float64)
    c = np.asarray(curves, dtype=np.float64)
    lead = c.shape[:-1]
    r = np.broadcast_to(r, c.shape)
    out = np.empty(lead + (len(fractions),))
    for idx in np.ndindex(*lead):
        out[idx] = [curve_radius(r[idx], c[idx], fq) for fq in fractions]
    return out


class ThroughFocusEE:
    """what :func:`through_focus_ee` returns.

    focs, fractions, radii, wvls, field_wts, spectral_wts, ref_wvl, kind   as used
                ('geometric' or 'diffraction'; ``radii`` None when not given)
    image_pts   [F, W, K, 2] each plane's image point
    n_ok        [F, W, K] OK rays per plane (geometric; None for diffraction)
    strehl      [F, W, K] each plane's Strehl ratio (diffraction; None for geometric)
    pitch       [F, W, K] each PSF's pixel pitch (diffraction; None for geometric)
    centroid    [F, W, K, 2] each item's centre about its image point: the spot centroid
                (geometric) or the PSF centroid (diffraction)
    ee_radius   [F, W, K, Nf] the radius about that centre holding each fraction: the exact
                order statistic of the rays (geometric, rox_focus_ee), or interpolated on the
                item's curve (diffraction); NaN where no ray arrived
    ee          [F, W, K, Nr] the encircled energy at ``radii`` about that centre (None without
                ``radii``)
    curve_radii [F, K, n_curve] the radii of each field's polychromatic curve
    poly_ee     [F, K, n_curve] the polychromatic encircled energy about the field's polychromatic
                centroid at curve_radii
    poly_ee_at  [F, K, Nr] the same at ``radii`` (None without ``radii``)
    poly_ee_radius [F, K, Nf] poly_ee interpolated at each fraction: its resolution is the
                curve's step, curve_radii[..., 1]
    best_focus  [F, Nf] (+ ``_kind``): :func:`best_focus` of each field's poly_ee_radius curve
    best_focus_all [Nf] (+ ``_kind``): the same of the field-weighted mean of poly_ee_radius"""

    def __init__(self, focs, fractions, radii, wvls, field_wts, spectral_wts, ref_wvl, kind, image_pts,
                 centroid, ee_radius, ee, curve_radii, poly_ee, poly_ee_at, n_ok=None, strehl=None, pitch=None):
        self.focs = np.asarray(focs, dtype=np.float64)
        self.fractions = np.asarray(fractions, dtype=np.float64)
        self.radii = None if radii is None else np.asarray(radii, dtype=np.float64)
        self.wvls = list(wvls)
        self.field_wts = np.asarray(field_wts, dtype=np.float64)
        self.spectral_wts = np.asarray(spectral_wts, dtype=np.float64)
        self.ref_wvl = ref_wvl
        self.kind = kind
        self.image_pts = image_pts
        self.centroid = centroid
        self.n_ok = n_ok
        self.strehl = strehl
        self.pitch = pitch
        self.ee_radius = ee_radius
        self.ee = ee
        self.curve_radii = curve_radii
        self.poly_ee = poly_ee
        self.poly_ee_at = poly_ee_at
        self.poly_ee_radius = _curve_radii(curve_radii, poly_ee, self.fractions)
        F, _K, Nf = self.poly_ee_radius.shape
        self.best_focus = np.empty((F, Nf))
        self.best_focus_kind = np.empty((F, Nf), dtype=object)
        for f in range(F):
            for q in range(Nf):
                self.best_focus[f, q], self.best_focus_kind[f, q] = best_focus(self.focs, self.poly_ee_radius[f, :, q])
        res = [overall_best_focus(self.focs, self.poly_ee_radius[:, :, q], self.field_wts) for q in range(Nf)]
        self.best_focus_all = np.array([r[0] for r in res])
        self.best_focus_all_kind = np.array([r[1] for r in res], dtype=object)


def _check_fractions(fractions, what):
    f = np.asarray(fractions, dtype=np.float64).reshape(-1)
    if not 1 <= f.size <= abi.MAX_EE_FRACTIONS:
        raise ValueError(f'{what}: 1 to {abi.MAX_EE_FRACTIONS} fractions, got {f.size}')
    if not ((f > 0).all() and (f <= 1).all()):
        raise ValueError(f'{what}: fractions must lie in (0, 1], got {f}')
    return f


def _check_radii(radii, what):
    if radii is None:
        return None
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if not 1 <= r.size <= abi.MAX_EE_RADII:
        raise ValueError(f'{what}: 1 to {abi.MAX_EE_RADII} radii, got {r.size}')
    if not (np.isfinite(r).all() and (r >= 0).all() and (np.diff(r) >= 0).all()):
        raise ValueError(f'{what}: radii must be finite, >= 0 and non-decreasing, got {r}')
    return r


def poly_centroid(centroid, image_pts, wts, ok):
    """C [K, 2] = sum_w wts_w (image_pt_w + centroid_w) / sum_w wts_w over the entries with ``ok``
    (centroid, image_pts [W, K, 2]; wts [W] or [W, K]); NaN where no weight is left"""
    W, K = np.asarray(ok).shape
    w = np.where(ok, np.broadcast_to(np.asarray(wts, dtype=np.float64).reshape(W, -1), (W, K)), 0.0)
    c = np.where(ok[..., None], np.asarray(image_pts) + np.asarray(centroid), 0.0)
    tot = w.sum(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(tot[:, None] > 0, (w[..., None] * c).sum(axis=0) / tot[:, None], np.nan)


def through_focus_ee(opt_model, focs, fractions=(0.5, 0.8), radii=None, kind='geometric', flds=None, wvls=None,
                     num_rays=64, maxdim=None, field_wts=None, spectral_wts=None, ref_wvl=None, pitch=None,
                     n_curve=256, **kwargs):
    """Encircled energy through focus, per field and wavelength and polychromatic per field, on the
    device: one rox_trace_through_focus_grids launch traces each item's square pupil grid (as
    :func:`through_focus_mtf`) and evaluates it at every focus.  Fields, wavelengths and weights
    default as in :func:`through_focus_map`.  Returns a :class:`ThroughFocusEE`.

    ``kind='geometric'``: the spot of the rays.  Per item, about the plane's spot centroid,
    rox_focus_ee gives the exact order-statistic radius holding each fraction and, with ``radii``
    (1-D, system units), the fraction of the rays within each.  Per field, about the polychromatic
    centroid C of :func:`poly_merge` (lateral colour included), each wavelength's ray counts are
    weighted by its spectral weight, poly_ee(r) = sum_w s_w counts_w(r) / sum_w s_w n_w, on
    ``n_curve`` radii from 0 to the farthest ray R_max (the last one ulp beyond it);
    poly_ee_radius is interpolated on that curve, to a resolution of R_max / (n_curve - 1).

    ``kind='diffraction'``: the PSFs of rox_focus_psf (``num_rays`` even, ``maxdim`` -- default
    4 ``num_rays`` -- at least 2 ``num_rays``), in groups under MTF_PSF_CHUNK_BYTES.  Per item,
    about the PSF's own centroid, rox_focus_psf_ee gives the curve on ``n_curve`` radii from 0 to
    p maxdim / 2 (p its pitch) and ee_radius is interpolated on it.  Per field, about
    C = sum_w s_w (image_pt_w + centroid_w) / sum_w s_w, poly_ee = sum_w s_w ee_w / sum_w s_w of
    the unit-energy PSFs, on radii up to the smallest window of the field's wavelengths.  The EE
    is that of the PSF window, which is periodic: light the window wraps counts where it lands.
    Each PSF's pitch is calc_psf_scaling's delta_xp; a model without paraxial data needs
    ``pitch`` [F, W, K]."""
    from .engine import grid_rays, FocusRows
    what = 'through_focus_ee'
    focs = _check_focs(focs, what)
    frac = _check_fractions(fractions, what)
    rad = _check_radii(radii, what)
    if kind not in ('geometric', 'diffraction'):
        raise ValueError(f"{what}: kind must be 'geometric' or 'diffraction', got {kind!r}")
    n_curve = int(n_curve)
    if not 2 <= n_curve <= abi.MAX_EE_RADII:
        raise ValueError(f'{what}: n_curve {n_curve} outside [2, {abi.MAX_EE_RADII}]')
    num_rays = int(num_rays)
    if kind == 'diffraction':
        maxdim = 4 * num_rays if maxdim is None else int(maxdim)
        if num_rays < 2 or num_rays % 2:
            raise ValueError(f'{what}: num_rays must be even and >= 2, got {num_rays}')
        if maxdim < 2 * num_rays:
            raise ValueError(f'{what}: maxdim {maxdim} < 2 num_rays = {2 * num_rays}')
        if not _psf_block_fits(num_rays, maxdim):
            raise ValueError(f'{what}: the {num_rays} x {num_rays} grid does not fit in maxdim {maxdim}')
    elif num_rays < 1:
        raise ValueError(f'{what}: num_rays must be >= 1, got {num_rays}')
    flds, wvls, field_wts, spectral_wts, ref_wvl = _map_spec(opt_model, flds, wvls, field_wts, spectral_wts,
                                                             ref_wvl, what)
    F, W, K = len(flds), len(wvls), len(focs)
    s = np.asarray(spectral_wts, dtype=np.float64)
    if kind == 'diffraction':
        pitch = _given_pitch(pitch, (F, W, K), what)
    ref_radii = []
    eng, fs, wis, grids, opts_list, planes = _map_items(opt_model, flds, wvls, focs, None, num_rays, kwargs,
                                                        radii=ref_radii)
    R = grid_rays(grids[0])
    image_pts = _image_pts(planes).reshape(F, W, K, 2)
    args = dict(focs=focs, fractions=frac, radii=rad, wvls=wvls, field_wts=field_wts, spectral_wts=spectral_wts,
                ref_wvl=ref_wvl, kind=kind, image_pts=image_pts)

    if kind == 'geometric':
        stats, dev_rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True)
        stats = stats.reshape(F, W, K)
        own = np.nan_to_num(np.stack([stats['cx'], stats['cy']], axis=-1))          # [F, W, K, 2]
        flat = (F * W, K)
        _c, ee_radius, n_ok = eng.focus_ee(dev_rows, R, own.reshape(flat + (2,)), None, frac)
        ee = None
        if rad is not None:
            counts, _r, _n = eng.focus_ee(dev_rows, R, own.reshape(flat + (2,)), rad, None)
            with np.errstate(invalid='ignore', divide='ignore'):
                ee = np.where(n_ok[..., None] > 0, counts / n_ok[..., None], np.nan).reshape(F, W, K, -1)
        ref = wvls.index(ref_wvl)
        pm = [poly_merge(stats[f], image_pts[f], s, ref) for f in range(F)]
        C = np.stack([np.stack([m['cx'], m['cy']], axis=-1) for m in pm])           # [F, K, 2]
        about = np.nan_to_num(C[:, None] - image_pts).reshape(flat + (2,))          # [F W, K, 2]
        _c, far, _n = eng.focus_ee(dev_rows, R, about, None, [1.0])
        far = far.reshape(F, W, K)
        with np.errstate(invalid='ignore'):
            r_max = np.where(np.isnan(far).all(axis=1), 0.0, np.nanmax(np.where(np.isnan(far), -np.inf, far), axis=1))
        curve_radii = r_max[..., None] * np.linspace(0.0, 1.0, n_curve)             # [F, K, n_curve]
        # R_max^2 may round below the farthest ray's d2: the last radius is one ulp beyond R_max
        curve_radii[..., -1] = np.nextafter(r_max, np.inf)
        counts, _r, _n = eng.focus_ee(dev_rows, R, about, np.repeat(curve_radii, W, axis=0), None)
        n_ok = n_ok.reshape(F, W, K)
        poly_ee = _poly_counts(counts.reshape(F, W, K, n_curve), n_ok, s)
        poly_ee_at = None
        if rad is not None:
            counts, _r, _n = eng.focus_ee(dev_rows, R, about, rad, None)
            poly_ee_at = _poly_counts(counts.reshape(F, W, K, -1), n_ok, s)
        return ThroughFocusEE(centroid=np.stack([stats['cx'], stats['cy']], axis=-1),
                              ee_radius=ee_radius.reshape(F, W, K, -1), ee=ee, curve_radii=curve_radii,
                              poly_ee=poly_ee, poly_ee_at=poly_ee_at, n_ok=n_ok, **args)

    # diffraction
    assert R == num_rays * num_rays
    if pitch is None:
        pitch = _default_pitch(opt_model, wvls, num_rays, maxdim, ref_radii, (F, W, K), what)
    _none, dev_rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True,
                                                  want_stats=False)
    scale = _wave_scales(opt_model, wvls, F * W)
    window = pitch * (maxdim / 2)                                                   # [F, W, K]
    item_radii = window[..., None] * np.linspace(0.0, 1.0, n_curve)                 # [F, W, K, n_curve]
    curve_radii = window.min(axis=1)[..., None] * np.linspace(0.0, 1.0, n_curve)   # [F, K, n_curve]
    per_field = W * K * maxdim * maxdim * 8
    fstep = max(1, MTF_PSF_CHUNK_BYTES // per_field)                                # whole fields per group
    strehl = np.empty((F, W, K))
    centroid = np.empty((F, W, K, 2))
    item_ee = np.empty((F, W, K, n_curve))
    per_w = np.empty((F, W, K, n_curve))
    ee = None if rad is None else np.empty((F, W, K, rad.size))
    per_w_at = None if rad is None else np.empty((F, W, K, rad.size))
    C = np.empty((F, K, 2))
    for f0 in range(0, F, fstep):
        f1 = min(F, f0 + fstep)
        part = FocusRows(dev_rows.rows[f0 * W:f1 * W], dev_rows.status[f0 * W:f1 * W])
        dev_psf, psf_stats = eng.focus_psf(part, num_rays, maxdim, scale[f0 * W:f1 * W], want_psf=True)
        p = pitch[f0:f1].reshape(-1, K)
        e, cen = eng.focus_psf_ee(dev_psf, p, None, item_radii[f0:f1].reshape(-1, K, n_curve))
        item_ee[f0:f1] = e.reshape(f1 - f0, W, K, n_curve)
        centroid[f0:f1] = cen.reshape(f1 - f0, W, K, 2)
        strehl[f0:f1] = psf_stats['strehl'].reshape(f1 - f0, W, K)
        if rad is not None:
            e, _cen = eng.focus_psf_ee(dev_psf, p, None, rad, want_centroid=False)
            ee[f0:f1] = e.reshape(f1 - f0, W, K, -1)
        for f in range(f0, f1):
            C[f] = poly_centroid(centroid[f], image_pts[f], s, np.isfinite(centroid[f]).all(axis=-1))
        about = np.nan_to_num(C[f0:f1, None] - image_pts[f0:f1]).reshape(-1, K, 2)
        e, _cen = eng.focus_psf_ee(dev_psf, p, about, np.repeat(curve_radii[f0:f1], W, axis=0),
                                   want_centroid=False)
        per_w[f0:f1] = e.reshape(f1 - f0, W, K, n_curve)
        if rad is not None:
            e, _cen = eng.focus_psf_ee(dev_psf, p, about, rad, want_centroid=False)
            per_w_at[f0:f1] = e.reshape(f1 - f0, W, K, -1)
        del dev_psf
    ee_radius = _curve_radii(item_radii, item_ee, frac)
    poly_ee = _poly_psf(per_w, s)
    poly_ee_at = None if rad is None else _poly_psf(per_w_at, s)
    return ThroughFocusEE(centroid=centroid, ee_radius=ee_radius, ee=ee, curve_radii=curve_radii, poly_ee=poly_ee,
                          poly_ee_at=poly_ee_at, strehl=strehl, pitch=pitch, **args)


def _poly_counts(counts, n_ok, s):
    """[F, W, K, N] ray counts, [F, W, K] ray totals -> sum_w s_w counts_w / sum_w s_w n_w [F, K, N]"""
    num = (s[None, :, None, None] * counts).sum(axis=1)
    den = (s[None, :, None] * n_ok).sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den[..., None] > 0, num / den[..., None], np.nan)


def _poly_psf(ee, s):
    """[F, W, K, N] unit-energy EE curves -> sum_w s_w ee_w / sum_w s_w over the wavelengths whose
    curve is not NaN [F, K, N]; NaN where none is left"""
    ok = ~np.isnan(ee)
    w = np.where(ok, s[None, :, None, None], 0.0)
    tot = w.sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(tot > 0, np.where(ok, w * ee, 0.0).sum(axis=1) / tot, np.nan)


# ---- Zernike fits through focus --------------------------------------------------------------
def zero_crossing(focs, values):
    """the focus at which a sampled curve crosses zero: a sample that is exactly 0 -> (focus,
    'sample'); else linear interpolation inside the first pair of neighbouring samples of
    opposite sign -> (focus, 'crossing').  NaN samples are skipped; no pair brackets zero ->
    (nan, 'none')."""
    f = np.asarray(focs, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64)
    ok = ~np.isnan(v)
    f, v = f[ok], v[ok]
    for i in range(len(v)):
        if v[i] == 0.0:
            return float(f[i]), 'sample'
        if i + 1 < len(v) and (v[i] < 0) != (v[i + 1] < 0) and v[i + 1] != 0.0:
            return float(f[i] + (f[i + 1] - f[i]) * v[i] / (v[i] - v[i + 1])), 'crossing'
    return float('nan'), 'none'


class ThroughFocusZernike:
    """what :func:`through_focus_zernike` returns.

    focs, wvls, field_wts, spectral_wts, ref_wvl   as used
    terms       the (n, m, scale) of each coefficient; ``names`` their classical names
    coef        [F, W, K, J] the least-squares coefficients, in waves (NaN where a plane's fit
                failed: stats['fit'] 1 too few rays, 2 singular)
    stats       [F, W, K] engine.ZERNIKE_STATS_DTYPE: n, n_outside, rms, rms_residual,
                pv_residual (waves), cond, fit
    circle      [F, W, 3] (cx, cy, radius) of the unit circle in pupil coordinates
    defocus_zero [F, W] (+ ``_kind``): :func:`zero_crossing` of each item's defocus (2, 0)
                coefficient through focus (NaN, 'none' without a defocus term)
    defocus_zero_field [F] (+ ``_kind``): the same at ref_wvl"""

    def __init__(self, focs, wvls, field_wts, spectral_wts, ref_wvl, terms, coef, stats, circle):
        from .zernike import term_names
        self.focs = np.asarray(focs, dtype=np.float64)
        self.wvls, self.field_wts, self.spectral_wts, self.ref_wvl = wvls, field_wts, spectral_wts, ref_wvl
        self.terms = list(terms)
        self.names = term_names(self.terms)
        self.coef = coef
        self.stats = stats
        self.circle = circle
        F, W, _K, _J = coef.shape
        self.defocus_zero = np.full((F, W), np.nan)
        self.defocus_zero_kind = np.full((F, W), 'none', dtype=object)
        jd = [j for j, t in enumerate(self.terms) if (t[0], t[1]) == (2, 0)]
        if jd:
            for f in range(F):
                for w in range(W):
                    self.defocus_zero[f, w], self.defocus_zero_kind[f, w] = zero_crossing(
                        self.focs, coef[f, w, :, jd[0]])
        ref = self.wvls.index(ref_wvl)
        self.defocus_zero_field = self.defocus_zero[:, ref].copy()
        self.defocus_zero_field_kind = self.defocus_zero_kind[:, ref].copy()


def zernike_terms(terms='fringe', n_terms=37):
    """'fringe' / 'noll' and a count, or explicit (n, m[, scale]) triples -> checked triples"""
    from . import zernike as Z
    if isinstance(terms, str):
        if terms == 'fringe':
            return Z.fringe_terms(n_terms)
        if terms == 'noll':
            return Z.noll_terms(n_terms)
        raise ValueError(f"Zernike terms: 'fringe', 'noll' or (n, m, scale) triples, got {terms!r}")
    return Z.check_terms(terms)


def zernike_circles(grids, circle, n_items, what):
    """[n_items, 3] (cx, cy, radius): 'pupil' the unit circle, 'bbox' each grid's vignetting box's
    centre and half its larger side, or values broadcast to [n_items, 3]"""
    if isinstance(circle, str):
        if circle == 'pupil':
            return np.tile([0.0, 0.0, 1.0], (n_items, 1))
        if circle == 'bbox':
            return np.array([[0.5 * (g.start[0] + g.stop[0]), 0.5 * (g.start[1] + g.stop[1]),
                              0.5 * max(abs(g.stop[0] - g.start[0]), abs(g.stop[1] - g.start[1]))]
                             for g in grids])
        raise ValueError(f"{what}: circle 'pupil', 'bbox' or (cx, cy, radius), got {circle!r}")
    c = np.array(np.broadcast_to(np.asarray(circle, dtype=np.float64), (n_items, 3)))
    if not (np.isfinite(c).all() and (c[:, 2] > 0).all()):
        raise ValueError(f'{what}: circle must be finite with radius > 0')
    return c


def through_focus_zernike(opt_model, focs, flds=None, wvls=None, num_rays=64, terms='fringe', n_terms=37,
                          circle='pupil', field_wts=None, spectral_wts=None, ref_wvl=None, **kwargs):
    """Zernike fits of the wavefront of every field at every wavelength through focus, on the
    device: one rox_trace_through_focus_grids launch traces each item's square pupil grid (the
    trace_wavefront grid, as :func:`through_focus_map` with ``xy=None``) and evaluates it at every
    focus, and one rox_focus_zernike fits each plane's OPD in waves -- the rows stay in HBM.
    ``terms``: 'fringe' or 'noll' (the first ``n_terms``) or (n, m, scale) triples; ``circle``:
    'pupil' the unit circle of the entrance pupil, 'bbox' the circle about each field's vignetting
    box with half its larger side, or (cx, cy, radius) broadcast to [F, W, 3].  Fields,
    wavelengths and weights default as in :func:`through_focus_map`
    (:class:`ThroughFocusZernike`)."""
    what = 'through_focus_zernike'
    focs = _check_focs(focs, what)
    num_rays = int(num_rays)
    if num_rays < 2:
        raise ValueError(f'{what}: num_rays must be >= 2, got {num_rays}')
    tl = zernike_terms(terms, n_terms)
    flds, wvls, field_wts, spectral_wts, ref_wvl = _map_spec(opt_model, flds, wvls, field_wts, spectral_wts,
                                                             ref_wvl, what)
    F, W, K = len(flds), len(wvls), len(focs)
    if not isinstance(circle, str):
        circle = np.broadcast_to(np.asarray(circle, dtype=np.float64), (F, W, 3)).reshape(F * W, 3)
    eng, fs, wis, grids, opts_list, planes = _map_items(opt_model, flds, wvls, focs, None, num_rays, kwargs)
    circ = zernike_circles(grids, circle, F * W, what)
    _none, dev_rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True,
                                                  want_stats=False)
    scale = _wave_scales(opt_model, wvls, F * W)
    coef, stats = eng.focus_zernike(dev_rows, grids, tl, scale, circ)
    J = len(tl)
    return ThroughFocusZernike(focs, wvls, field_wts, spectral_wts, ref_wvl, tl,
                               np.asarray(coef).reshape(F, W, K, J), np.asarray(stats).reshape(F, W, K),
                               circ.reshape(F, W, 3))


def wavefront_zernike(opt_model, fld, wvl, foc=0., num_rays=64, terms='fringe', n_terms=37, circle='pupil',
                      **kwargs):
    """the Zernike fit of one field's wavefront at one wavelength and focus: :func:`through_focus_zernike`
    of that single item -> (coef [J] in waves, stats record, terms)"""
    r = through_focus_zernike(opt_model, [foc], flds=[fld], wvls=[wvl], num_rays=num_rays, terms=terms,
                              n_terms=n_terms, circle=circle, field_wts=[1.0], spectral_wts=[1.0],
                              ref_wvl=wvl, **kwargs)
    return r.coef[0, 0, 0], r.stats[0, 0, 0], r.terms


# ---- Huygens point spread functions on the detector's pixel grid --------------------------------
# rayoptics/raytr/waveabr.py:305 forms an OPD as ... - ray_op ... + cr_op ...: the chief ray's
# optical path to the reference sphere minus the ray's.  The ray's own path is minus that.
HUYGENS_OPD_SIGN = -1.0


def huygens_rows(seg, opd, centre, radius, n_img, wvl_sys):
    """The rows of rox_huygens_psf from the rays at the image: ``seg`` [10, R] the ROX_OUT_LAST
    packet (p in rows 0-2, d in rows 3-5), ``opd`` [R] the ROX_OUT_OPD row (system units) about the
    reference sphere of centre ``centre`` (x, y, z in image coordinates) and radius ``radius``;
    torch tensors, float64.  Ray r is a plane wavelet that arrives along d_r.  Its optical path at
    the centre c, up to a constant common to all rays, is its path to the reference sphere plus
    n times what lies between the sphere and the plane through c normal to d_r: with TA = p - c
    and q = |TA|^2 - (d.TA)^2 the ray meets the sphere sqrt(R^2 - q) before that plane, so
        Phi_r = HUYGENS_OPD_SIGN * W_r - n q / (sqrt(R^2 - q) + |R|)
    (the second term is n (sqrt(R^2 - q) - |R|), written without cancellation).  n is |n_img|: d is
    the direction the light travels in, also where an odd number of mirrors has turned it towards
    -z and the reference's index carries a sign, and a path grows along it.  Returns [4, R] =
    (Phi / lambda, n d / lambda): cycles, and cycles per system unit about c."""
    t = __import__('torch')
    ta = [seg[i] - float(centre[i]) for i in range(3)]
    d = [seg[3 + i] for i in range(3)]
    dta = d[0] * ta[0] + d[1] * ta[1] + d[2] * ta[2]
    q = ta[0] * ta[0] + ta[1] * ta[1] + ta[2] * ta[2] - dta * dta
    R = abs(float(radius))
    n = abs(float(n_img))
    phi = HUYGENS_OPD_SIGN * opd - n * q / (t.sqrt(R * R - q) + R)
    k = n / float(wvl_sys)
    return t.stack([phi / float(wvl_sys), k * d[0], k * d[1], k * d[2]])


class HuygensRows:
    """the traced items of :func:`huygens_psf`, still on the engine's device: ``rows`` [F*W, 4, ld],
    ``status`` [F*W, ld], ``n_rays``; ``centres`` [F*W, 3] the reference spheres' centres (image
    coordinates), ``radii`` [F*W]; the fields, wavelengths, spectral weights and the index of the
    reference wavelength"""

    def __init__(self, eng, rows, status, n_rays, centres, radii, flds, wvls, spectral_wts, ref):
        self.eng, self.rows, self.status, self.n_rays = eng, rows, status, n_rays
        self.centres, self.radii, self.flds, self.wvls = centres, radii, flds, wvls
        self.spectral_wts, self.ref = spectral_wts, ref


def trace_huygens_rows(opt_model, flds=None, wvls=None, num_rays=64, check_apertures=True, ref_foc=0.0,
                       what='huygens_psf'):
    """Every (field, wavelength) item's ``num_rays`` x ``num_rays`` pupil grid in two launches of
    rox_trace_pupil_grids -- ROX_OUT_LAST for p and d at the image, ROX_OUT_OPD for W about the
    item's reference sphere at focus ``ref_foc`` -- and :func:`huygens_rows` on them where they
    lie -> :class:`HuygensRows`.  An infinite reference sphere raises ValueError."""
    from .table import wavefront_from_model
    ref_first = wvls is not None and len(wvls) > 0
    eng, flds, wvls, spectral_wts, fs, wis, opts_last, _flags = _packet_items(opt_model, flds, wvls, int(num_rays),
                                                                             check_apertures, what, abi.OUT_LAST)
    ref = 0 if ref_first else wvls.index(float(opt_model['osp']['wvls'].central_wvl))
    opts_opd, centres, radii, n_img = [], [], [], []
    for fld in flds:
        for wvl in wvls:
            ref_sphere, cr_pkg = _setup_pupil_coords(opt_model, fld, wvl, float(ref_foc))
            own = getattr(fld, 'rox_wavefront', None)
            wf = own if own is not None else wavefront_from_model(opt_model, fld, cr_pkg, ref_sphere)
            wf = abi.Wavefront.from_buffer_copy(bytes(wf))
            if wf.kind != abi.WF_FINITE or not np.isfinite(wf.ref_radius) or abs(wf.ref_radius) > 1e8 \
                    or wf.ref_radius == 0.0:
                raise ValueError(f'{what}: the reference sphere of a field at {wvl} nm is infinite (radius '
                                 f'{wf.ref_radius!r}): a Huygens PSF needs a finite exit pupil')
            kw = dict(check_apertures=bool(check_apertures), apply_vignetting=True)
            _e, _f, _wi, o = _launch_setup(opt_model, fld, wvl, kw, abi.OUT_OPD, wf=wf)
            opts_opd.append(o)
            ip = ref_sphere[0]
            centres.append((float(ip[0]), float(ip[1]), float(ref_foc)))
            radii.append(float(wf.ref_radius))
            n_img.append(float(wf.n_img))
    grid = make_grid((-1., -1.), (1., 1.), int(num_rays))
    last = eng.trace_pupil_grids(fs, wis, grid, opts_last, want_pupil=False)
    opd = eng.trace_pupil_grids(fs, wis, grid, opts_opd, want_pupil=False)
    t = getattr(eng, 'torch', None) or __import__('torch')
    from .engine import padded_ld
    R = int(num_rays) * int(num_rays)
    ld = padded_ld(R)
    n_items = len(fs)
    rows = t.zeros((n_items, 4, ld), dtype=t.float64, device=eng.device)
    status = t.full((n_items, ld), abi.BLOCKED, dtype=t.uint8, device=eng.device)
    W = len(wvls)
    for i in range(n_items):
        lam = opt_model.nm_to_sys_units(wvls[i % W])
        rows[i, :, :R] = huygens_rows(last[i].seg, opd[i].seg[0], centres[i], radii[i], n_img[i], lam)
        s_last, s_opd = last[i].status, opd[i].status
        status[i, :R] = t.where(s_last == abi.OK, s_opd, s_last)
    return HuygensRows(eng, rows, status, R, np.array(centres), np.array(radii), flds, wvls,
                       [float(w) for w in spectral_wts], ref)


class HuygensPSF:
    """What :func:`huygens_psf` returns.  F fields, W wavelengths, K focus planes, S x S pixels.

    ``psf``           [F, W, K, S, S] |U|^2 of every item and plane, first pixel axis along x; NumPy,
                      or with ``on_device`` a torch tensor in HBM
    ``poly``          [F, K, S, S] sum over w of spectral_wts[w] * psf[f, w, k] / norm[f, w, k]: all
                      wavelengths of a field lie on one window, so lateral colour is in it
    ``strehl``        [F, W, K] psf at the pixel nearest the reference sphere's centre over ``norm``
                      (the reference wavelength's centre is a pixel; the others lie up to half a
                      pixel off)
    ``norm``, ``sum`` [F, W, K] (sum of the amplitudes)^2 -- the peak of a perfect wavefront -- and
                      the sum of psf over the window
    ``border_share``  [F, W, K] the share of ``sum`` in the window's outermost ring of pixels: the
                      handle on a window that is too small
    ``peak``, ``peak_px``  [F, W, K] and [F, W, K, 2] the largest value and its pixel
    ``n``             [F, W] the rays that reached the image
    ``origins``       [F, 2] image coordinates (x, y) of pixel (0, 0); pixel (a, b) lies at origin +
                      (a, b) * pixel_pitch
    ``centres``       [F, W, 3] the reference spheres' centres
    ``poly_strehl``   [F, K] the spectrally weighted mean of ``strehl``;
    ``best_focus`` / ``best_focus_kind``  [F] :func:`best_focus` of its negative"""

    def __init__(self, focs, wvls, spectral_wts, pixel_pitch, psf, poly, stats, border_share, origins, centres):
        self.focs = np.asarray(focs, dtype=np.float64)
        self.wvls, self.spectral_wts, self.pixel_pitch = wvls, np.asarray(spectral_wts, dtype=np.float64), pixel_pitch
        self.psf, self.poly, self.stats = psf, poly, stats
        self.strehl, self.norm, self.sum, self.peak = stats['strehl'], stats['norm'], stats['sum'], stats['peak']
        self.peak_px = np.stack([stats['peak_ix'], stats['peak_iy']], axis=-1)
        self.n = stats['n'][:, :, 0]
        self.border_share, self.origins, self.centres = border_share, origins, centres
        w = self.spectral_wts / self.spectral_wts.sum()
        self.poly_strehl = np.einsum('w,fwk->fk', w, np.nan_to_num(self.strehl, nan=0.0))
        bf = [best_focus(self.focs, -s) for s in self.poly_strehl]
        self.best_focus = np.array([b[0] for b in bf])
        self.best_focus_kind = [b[1] for b in bf]


def huygens_window(centre_xy, size, pixel_pitch):
    """the origin -- image coordinates of pixel (0, 0) -- of a window of ``size`` pixels whose
    pixel size // 2 lies on ``centre_xy``"""
    return np.asarray(centre_xy, dtype=np.float64) - (int(size) // 2) * float(pixel_pitch)


def huygens_planes(centres, origins, focs, n_wvls):
    """[F*W, K, 3] the (x0, y0, dz) of rox_huygens_psf: field f's window origin and the focus
    planes about item (f, w)'s reference-sphere centre"""
    centres = np.asarray(centres, dtype=np.float64)
    focs = np.asarray(focs, dtype=np.float64)
    planes = np.empty((centres.shape[0], len(focs), 3))
    for i, c in enumerate(centres):
        planes[i, :, 0:2] = np.asarray(origins[i // n_wvls]) - c[0:2]
        planes[i, :, 2] = focs - c[2]
    return planes


def huygens_psf(opt_model, pixel_pitch, size=64, focs=(0.,), flds=None, wvls=None, num_rays=64,
                check_apertures=True, on_device=False, ref_foc=0.0):
    """Huygens point spread functions on the detector's pixel grid, through focus, on the device.
    Every traced ray is a plane wavelet with its own phase and real direction of arrival; their
    complex sum is taken at ``size`` x ``size`` pixels of ``pixel_pitch`` (system units) on every
    focus plane ``focs`` (image shifted along z) and squared -- pupil distortion, an anamorphic
    off-axis pupil and vignetting come with the rays, and pitch, window and defocus are free.

    Two launches of rox_trace_pupil_grids over every (field, wavelength) item (:func:`trace_huygens_rows`:
    ``num_rays`` x ``num_rays`` rays over the field's vignetted pupil box, the reference spheres set
    up at focus ``ref_foc``), then one rox_huygens_psf call: a complex GEMM on the fp64 matrix
    cores.  All wavelengths of a field share one window, its pixel size // 2 on the chief ray of
    the reference wavelength (the first given, else the central one).  Amplitudes are 1: no
    apodization, no coatings.  Sampling: the pupil grid aliases the PSF with a period of
    lambda * (rays across) / (2 NA); keep size * pixel_pitch well below it.
    Defaults as :func:`through_focus_map`; a workloads.TableModel passes ``flds`` and ``wvls``.
    An infinite reference sphere raises ValueError.  Returns :class:`HuygensPSF`."""
    from .engine import records_view, HUYGENS_STATS_DTYPE
    what = 'huygens_psf'
    focs = _check_focs(focs, what)
    S, pitch = int(size), float(pixel_pitch)
    if not 1 <= S <= abi.MAX_HUYGENS_PIXELS:
        raise ValueError(f'{what}: size {size} outside [1, {abi.MAX_HUYGENS_PIXELS}]')
    if not (np.isfinite(pitch) and pitch > 0.0):
        raise ValueError(f'{what}: pixel_pitch {pixel_pitch!r} is not finite and > 0')
    hr = trace_huygens_rows(opt_model, flds, wvls, num_rays, check_apertures, ref_foc, what)
    eng, t = hr.eng, hr.eng.torch
    F, W, K = len(hr.flds), len(hr.wvls), len(focs)
    centres = hr.centres.reshape(F, W, 3)
    origins = np.stack([huygens_window(centres[f, hr.ref, 0:2], S, pitch) for f in range(F)])
    planes = huygens_planes(hr.centres, origins, focs, W)
    psf, _field, raw = eng.huygens_psf(hr.rows, hr.status, planes, S, S, pitch, pitch, n_rays=hr.n_rays,
                                       stats_on_device=True)
    psf = psf.reshape(F, W, K, S, S)
    ring = psf[..., 0, :].sum(-1) + psf[..., -1, :].sum(-1) if S > 1 else psf[..., 0, :].sum(-1)
    if S > 2:
        ring = ring + psf[..., 1:-1, 0].sum(-1) + psf[..., 1:-1, -1].sum(-1)
    stats = records_view(raw, HUYGENS_STATS_DTYPE).reshape(F, W, K)
    norm = t.from_numpy(np.ascontiguousarray(stats['norm'])).to(eng.device)
    wts = t.tensor(hr.spectral_wts, dtype=t.float64, device=eng.device)
    scaled = psf * (wts.reshape(1, W, 1) / norm).reshape(F, W, K, 1, 1)
    poly = t.nan_to_num(scaled, nan=0.0).sum(dim=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        border = ring.cpu().numpy() / stats['sum']
    if not on_device:
        psf, poly = psf.cpu().numpy(), poly.cpu().numpy()
    return HuygensPSF(focs, hr.wvls, hr.spectral_wts, pitch, psf, poly, stats, border, origins, centres)


# ---- point spread function ------------------------------------------------------
PSF_BACKEND = None          # None -> engine.calc_psf (the HIP path); tests inject a double


def calc_psf(wavefront, ndim, maxdim):
    """rayoptics/raytr/analyses.py:848-875: the PSF of an OPD grid -- the zero-padded
    pupil function exp(i 2 pi W), its shifted 2-D FFT, |.|^2, normalised.  One call
    into the library (``rox_calc_psf``: a pruned DFT on the fp64 matrix cores) instead
    of a maxdim x maxdim Python loop and a host FFT; any even ``ndim`` that fits,
    any ``maxdim``."""
    fn = PSF_BACKEND
    if fn is None:
        from .engine import calc_psf as fn
    return fn(wavefront, ndim, maxdim)


def update_psf_data(pupil_grid, build='rebuild'):
    """rayoptics/raytr/analyses.py:878-883"""
    pupil_grid.update_data(build=build)
    return calc_psf(pupil_grid.grid[2], pupil_grid.num_rays, pupil_grid.maxdim)
