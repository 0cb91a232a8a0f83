"""Launch wrappers over the C ABI of libroxtrace.so (include/roxtrace.h).

PyTorch is used only as plumbing: device buffers and the current HIP stream.
There is no CPU fallback -- a missing library, or a missing GPU, raises.
"""
import collections
import ctypes as C
import functools
import os
import threading

import numpy as np

from . import abi
from .table import SurfaceTable

_HERE = os.path.dirname(os.path.abspath(__file__))
# ROX_LIB selects an experiment build of the same HIP source (tools/ab_bench.py)
LIB_PATH = os.environ.get('ROX_LIB') or os.path.join(_HERE, 'libroxtrace.so')
_lib = None


class EngineError(RuntimeError):
    pass


def load_library():
    """dlopen libroxtrace.so; never falls back to anything else."""
    global _lib
    if _lib is None:
        # torch ships its own libamdhip64; it must be the HIP runtime of the
        # process *before* libroxtrace.so (linked against the same SONAME)
        # is dlopen'ed, or the two sides would not share device pointers
        import torch  # noqa: F401
        if not os.environ.get('ROX_LIB'):
            # missing (fresh checkout) or stale (a source, header or flag changed
            # since it was built -- build.py compares a digest of its inputs):
            # compile the HIP sources in-tree now.  A stale library is never loaded.
            try:
                import importlib.util
                spec = importlib.util.spec_from_file_location(
                    'rox_build', os.path.join(_HERE, 'build.py'))
                b = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(b)
                b.build()
            except Exception as e:
                raise EngineError(
                    f'{LIB_PATH} is missing or stale and could not be built ({e!r}): run '
                    '`python ray-optics_amd/build.py` (hipcc --offload-arch=gfx950).  '
                    'There is no CPU fallback.')
        if not os.path.exists(LIB_PATH):
            raise EngineError(f'{LIB_PATH} is missing.  There is no CPU fallback.')
        lib = abi.declare(C.CDLL(LIB_PATH))
        if lib.rox_abi_version() != abi.ABI_VERSION:
            raise EngineError('libroxtrace.so ABI version mismatch')
        _lib = lib
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = load_library().rox_last_error().decode(errors='replace')
        raise EngineError(f'{what} failed ({rc}): {msg}')


def make_opts(flags=abi.INTERSECT_OBJ, out_mode=abi.OUT_FULL, first_surf=0,
              last_surf=-1, eps=1.0e-12, fuzz=1e-5, foc=0.0, image_pt=(0., 0.), wf=None):
    o = abi.Opts()
    if wf is not None:
        o.wf = wf
    o.flags, o.out_mode = int(flags), int(out_mode)
    o.first_surf, o.last_surf = int(first_surf), int(last_surf)
    o.eps, o.fuzz, o.foc = float(eps), float(fuzz), float(foc)
    o.image_pt[0], o.image_pt[1] = float(image_pt[0]), float(image_pt[1])
    return o


def make_grid(start, stop, num, kind=abi.GRID_PRODUCT, row_begin=0, row_count=0):
    g = abi.Grid()
    g.start[0], g.start[1] = float(start[0]), float(start[1])
    g.stop[0], g.stop[1] = float(stop[0]), float(stop[1])
    g.num, g.kind = int(num), int(kind)
    g.row_begin, g.row_count = int(row_begin), int(row_count)
    return g


def grid_rays(grid):
    """number of rays a rox_grid describes"""
    if grid.kind == abi.GRID_FAN:
        return grid.num
    return (grid.row_count or grid.num) * grid.num


def calc_psf(opd, ndim, maxdim):
    """analyses.calc_psf (rayoptics/raytr/analyses.py:848-875) on the device:
    ``opd`` is the [ndim, ndim] OPD grid in waves (NumPy, NaN = no data, or a
    float64 torch tensor already in HBM); returns the normalised [maxdim, maxdim]
    PSF as the same kind of array.  A pruned DFT as two complex fp64 GEMMs on
    the matrix cores (csrc/psf.hip)."""
    import torch
    if not torch.cuda.is_available():
        raise EngineError('no GPU visible: the PSF kernels have no CPU fallback')
    lib = load_library()
    ndim, maxdim = int(ndim), int(maxdim)
    if isinstance(opd, torch.Tensor):
        w = opd.to(dtype=torch.float64).contiguous()
        if tuple(w.shape) != (ndim, ndim):
            raise ValueError(f'opd is {tuple(w.shape)}, expected ({ndim}, {ndim})')
        out = torch.empty((maxdim, maxdim), dtype=torch.float64, device=w.device)
        with torch.cuda.device(w.device):
            _check(lib.rox_calc_psf(w.data_ptr(), ndim, maxdim, out.data_ptr(), 0,
                                    C.c_void_p(torch.cuda.current_stream(w.device).cuda_stream)),
                   'rox_calc_psf')
        out._keep = w
        return out
    w = np.ascontiguousarray(opd, dtype=np.float64)
    if w.shape != (ndim, ndim):
        raise ValueError(f'opd is {w.shape}, expected ({ndim}, {ndim})')
    out = np.empty((maxdim, maxdim))
    _check(lib.rox_calc_psf(w.ctypes.data, ndim, maxdim, out.ctypes.data, abi.HOST_POINTERS, None),
           'rox_calc_psf')
    return out


_NP_DTYPES = {}


def _np_dtypes(torch):
    if not _NP_DTYPES:
        _NP_DTYPES.update({torch.float64: np.float64, torch.uint8: np.uint8,
                           torch.int16: np.int16, torch.int32: np.int32,
                           torch.int64: np.int64})


# rox_focus_stats (include/roxtrace.h) as a NumPy record: what trace_pupil_grid_focus returns
FOCUS_STATS_DTYPE = np.dtype([(name, np.int64 if name == 'n' else np.float64)
                              for name, _t in abi.FocusStats._fields_])
assert FOCUS_STATS_DTYPE.itemsize == C.sizeof(abi.FocusStats)


def records_view(raw, dtype):
    """the raw uint8 records [.., dtype.itemsize] an entry returns with ``on_device`` (a tensor, or
    its NumPy copy) -> a ``dtype`` array [..] on the host"""
    a = np.ascontiguousarray(raw.cpu().numpy() if hasattr(raw, 'cpu') else raw)
    return a.view(dtype).reshape(a.shape[:-1])


# rox_focus_psf_stats: what focus_psf returns
FOCUS_PSF_STATS_DTYPE = np.dtype([(name, np.int64 if name == 'n' else np.float64)
                                  for name, _t in abi.FocusPsfStats._fields_])
assert FOCUS_PSF_STATS_DTYPE.itemsize == C.sizeof(abi.FocusPsfStats)


# rox_huygens_stats: what huygens_psf returns
HUYGENS_STATS_DTYPE = np.dtype([('n', np.int64), ('norm', np.float64), ('sum', np.float64), ('peak', np.float64),
                                ('strehl', np.float64), ('peak_ix', np.int32), ('peak_iy', np.int32)])
assert HUYGENS_STATS_DTYPE.itemsize == C.sizeof(abi.HuygensStats)


# rox_footprint: what surface_footprints returns
FOOTPRINT_DTYPE = np.dtype([('n', np.int64), ('n_fail', np.int64, (5,)), ('n_inc', np.int64),
                            ('min', np.float64, (2,)), ('max', np.float64, (2,)), ('r2_max', np.float64),
                            ('cx', np.float64), ('cy', np.float64), ('rms_r', np.float64),
                            ('cos_inc_min', np.float64), ('cos_inc_sum', np.float64),
                            ('cos_exit_min', np.float64)])
assert FOOTPRINT_DTYPE.itemsize == C.sizeof(abi.Footprint)


def footprint_view(records):
    """the uint8 tensor [n_items, n_seg, 144] surface_footprints(on_device=True) returns -> a
    FOOTPRINT_DTYPE array [n_items, n_seg] on the host"""
    return records_view(records, FOOTPRINT_DTYPE)


# rox_tx_surface / rox_tx_item: what surface_transmission returns
TX_SURFACE_DTYPE = np.dtype([('n', np.int64)] + [(name, np.float64) for name in
                                                ('ts_sum', 'tp_sum', 't_sum', 'ts_min', 'tp_min', 'ci_sum', 'ci_min')])
TX_ITEM_DTYPE = np.dtype([('n_ok', np.int64), ('n_rays', np.int64)] +
                         [(name, np.float64) for name in ('t_sum', 't_min', 't_max', 't1_sum', 't2_sum', 'd_sum', 'd_max')])
assert TX_SURFACE_DTYPE.itemsize == C.sizeof(abi.TxSurface)
assert TX_ITEM_DTYPE.itemsize == C.sizeof(abi.TxItem)


def tx_view(records, dtype):
    """the uint8 tensor surface_transmission(on_device=True) returns for ``surf`` or ``item`` -> a
    TX_SURFACE_DTYPE / TX_ITEM_DTYPE array on the host"""
    return records_view(records, dtype)


# rox_sa_item: what projected_solid_angle returns
SA_ITEM_DTYPE = np.dtype([('n_ok', np.int64), ('n_cells', np.int64, (5,))] +
                         [(name, np.float64) for name in ('a_full', 'a_tri', 'a_abs', 'aw_full', 'aw_tri', 'l_sum',
                                                          'm_sum', 'l_min', 'l_max', 'm_min', 'm_max', 'r2_max')])
assert SA_ITEM_DTYPE.itemsize == C.sizeof(abi.SaItem)


# rox_seg_focus: what segment_foci returns
SEG_FOCUS_DTYPE = np.dtype([(name, np.int64) for name in ('n', 'n_flat', 'n_bad', 'n_in')] +
                           [('w_sum', np.float64), ('w_in', np.float64), ('a_mean', np.float64, (2,)),
                            ('b_mean', np.float64, (2,))] +
                           [(name, np.float64) for name in ('m_aa', 'm_ab', 'm_bb', 'z_in_min', 'z_in_max',
                                                            'z_out_min', 'z_out_max')])
assert SEG_FOCUS_DTYPE.itemsize == C.sizeof(abi.SegFocus)

# rox_wmap_item: the item records of weighted_maps
WMAP_ITEM_DTYPE = np.dtype([(name, np.int64) for name in ('n_in', 'n_out', 'n_bad', 'q_in', 'q_out')])
# rox_wd_item: what wave_differentials returns per item
WD_ITEM_DTYPE = np.dtype([(name, np.int64) for name in ('n', 'n_bad', 'pivot_ray')])
assert WD_ITEM_DTYPE.itemsize == C.sizeof(abi.WdItem)
assert WMAP_ITEM_DTYPE.itemsize == C.sizeof(abi.WmapItem)


def seg_focus_derive(rec):
    """what the host derives from rox_seg_focus records (any shape): ``(zeta, ms_min, ms_0,
    inside)`` -- the plane z = zeta* = -m_ab/m_bb of the slot's frame at which the weighted
    mean-square radius of the bundle about its centroid is smallest, its value there
    (m_aa - m_ab^2/m_bb)/w_sum (clipped at 0), its value m_aa/w_sum at z = 0, and whether zeta*
    lies between the z_in and the z_out range (the focus is in the segment).  NaN / False where
    nothing counted; a collimated bundle (m_bb == 0) has zeta* = NaN and ms_min = ms_0."""
    with np.errstate(divide='ignore', invalid='ignore'):
        maa, mab, mbb, w = rec['m_aa'], rec['m_ab'], rec['m_bb'], rec['w_sum']
        conv = mbb > 0
        zeta = np.where(conv, -mab / np.where(conv, mbb, 1.0), np.nan)
        ms_0 = maa / w
        ms_min = np.where(conv, np.maximum(maa - mab * mab / np.where(conv, mbb, 1.0), 0.0) / w, ms_0)
        lo = np.minimum(rec['z_in_min'], rec['z_out_min'])
        hi = np.maximum(rec['z_in_max'], rec['z_out_max'])
        inside = conv & (zeta >= lo) & (zeta <= hi)
    return zeta, ms_min, ms_0, inside


# rox_zernike_stats: what focus_zernike returns
ZERNIKE_STATS_DTYPE = np.dtype([('n', np.int64), ('n_outside', np.int64), ('rms', np.float64),
                                ('rms_residual', np.float64), ('pv_residual', np.float64),
                                ('cond', np.float64), ('fit', np.int32), ('reserved', np.int32)])
assert ZERNIKE_STATS_DTYPE.itemsize == C.sizeof(abi.ZernikeStats)


def zernike_stats_view(raw):
    """the ZERNIKE_STATS_DTYPE array [..] of the raw uint8 records [.., 56] focus_zernike returns
    with ``on_device`` (copied to the host)"""
    return records_view(raw, ZERNIKE_STATS_DTYPE)


class FocusRows:
    """the per-ray rows of a through-focus launch on the device: ``rows`` [K, 3, R] (x abr,
    y abr, OPD in system units; rays that fail keep NaN) and ``status`` [R] -- of a batched
    launch [n_items, K, 3, R] and [n_items, R]"""

    def __init__(self, rows, status):
        self.rows = rows
        self.status = status

    def to_host(self):
        """(rows, status) as NumPy arrays"""
        return self.rows.cpu().numpy(), self.status.cpu().numpy()


def _f64(x, shape):
    """x as a C-contiguous float64 array broadcast to shape"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), shape))


def padded_ld(R):
    """row pitch (in doubles) of the SoA packet buffer: the native library's
    ``rox_packet_ld`` (include/roxtrace.h), which C callers use too.  Rows exactly
    2^k bytes apart put one ray's 130 packet components on the same HBM channel;
    the library's pitch spreads them."""
    return int(load_library().rox_packet_ld(int(R)))


def _default_pool_budget():
    """ROX_PINNED_POOL_MB, else an eighth of the host's RAM, at most 4 GiB: page-locked memory
    kept by the pool is taken from what HostSegment registration, RCCL and other pinned
    allocations can get"""
    env = os.environ.get('ROX_PINNED_POOL_MB')
    if env:
        return int(env) << 20
    try:
        ram = os.sysconf('SC_PAGE_SIZE') * os.sysconf('SC_PHYS_PAGES')
    except (ValueError, OSError, AttributeError):
        ram = 32 << 30
    return int(min(4 << 30, max(256 << 20, ram // 8)))


class PinnedPool:
    """page-locked host buffers that outlive one call: handing the caller a
    NumPy array that *is* the pinned buffer saves a second pass over the data
    (a 13 MB spot diagram is ~1.5 ms of memcpy, five times the trace).  A block
    goes back to the pool when the last array viewing it is garbage-collected.

    Thread safety: ``take`` and ``trim`` hold the pool's lock.  A block comes back from
    ``_Lease.__del__`` -- any thread, any time, possibly inside a garbage collection that a
    thread holding the lock triggered -- so ``give_back`` takes no lock: it appends to a deque
    (atomic under the GIL) that the next ``take`` / ``trim`` shelves under the lock."""

    def __init__(self):
        self._lock = threading.Lock()
        self._returned = collections.deque()    # (nbytes, tensor) not yet shelved
        self._free = {}         # nbytes (rounded) -> [uint8 pinned tensors]
        self._shelved = 0       # bytes sitting in _free
        # Blocks are kept up to a byte budget, not a count: a SpotDiagramFigure holds nine arrays
        # of one size at a time, and releasing / re-pinning the surplus cost 3 ms per block
        # (hipHostFree + hipHostMalloc) -- 95 ms per refresh at num_rays = 256 with a bound of
        # four blocks per size (tools/spot_figure_profile.py).
        self.budget = _default_pool_budget()

    @property
    def _held(self):
        """bytes the pool keeps pinned right now (shelved + returned and not yet shelved)"""
        with self._lock:
            self._drain()
            return self._shelved

    @staticmethod
    def _round(nbytes):
        if nbytes > (64 << 20):                 # big blocks: 16 MiB granules
            return (nbytes + (16 << 20) - 1) // (16 << 20) * (16 << 20)
        n = 4096
        while n < nbytes:
            n *= 2
        return n

    def take(self, torch, nbytes):
        n = self._round(max(int(nbytes), 1))
        with self._lock:
            self._drain()
            lst = self._free.get(n)
            t = None
            if lst:
                t = lst.pop()
                self._shelved -= n
        if t is None:
            t = torch.empty(n, dtype=torch.uint8).pin_memory()
        return _Lease(self, n, t)

    def give_back(self, n, t):
        # (from _Lease.__del__: no lock, see the class docstring)
        self._returned.append((n, t))

    def _drain(self):
        while True:
            try:
                n, t = self._returned.popleft()
            except IndexError:
                return
            self._shelve(n, t)

    def _shelve(self, n, t):
        # bounded by max(budget, one block): what does not fit is unpinned.  Room is made by
        # dropping blocks of OTHER sizes first (largest first) -- a pool that has swept many sizes
        # keeps what is in use now -- and a single block larger than the whole budget is still
        # kept while nothing else is (re-pinning gigabytes per call costs a second)
        if self._shelved + n > self.budget:
            for m in sorted((m for m, lst in self._free.items() if m != n and lst), reverse=True):
                while self._free[m] and self._shelved + n > self.budget:
                    self._free[m].pop()
                    self._shelved -= m
                if self._shelved + n <= self.budget:
                    break
        if self._shelved + n <= self.budget or self._shelved == 0:
            self._free.setdefault(n, []).append(t)
            self._shelved += n

    def trim(self):
        """un-pin everything the pool keeps (blocks on loan are not touched); returns the
        bytes released.  ``session.clear()`` calls it."""
        with self._lock:
            self._drain()
            freed = self._shelved
            self._free.clear()
            self._shelved = 0
        return freed


class _Lease:
    """one pinned block on loan; NumPy arrays made by :meth:`array` keep it
    alive (they hold it as their base object)"""

    def __init__(self, pool, n, tensor):
        self._pool, self._n, self.tensor = pool, n, tensor
        self.ptr = tensor.data_ptr()

    def array(self, shape, dtype, offset=0):
        a = np.asarray(_View(self, shape, np.dtype(dtype).str, self.ptr + offset))
        return a

    def __del__(self):
        try:
            self._pool.give_back(self._n, self.tensor)
        except Exception:
            pass


class _View:
    def __init__(self, lease, shape, typestr, ptr):
        self._lease = lease
        self.__array_interface__ = {'shape': tuple(shape), 'typestr': typestr,
                                    'data': (ptr, False), 'version': 3}


_pool = PinnedPool()

# pupil launches whose outputs are at most this many bytes go through ROX_HOST_POINTERS
# (TraceEngine.trace_pupil_np); the library bounces up to 4 MiB through its mapped block
HOST_DIRECT_BYTES = 1 << 20


class DeviceResult:
    """SoA trace results resident in HBM (torch tensors on the engine's device).

    seg: FULL [n_seg, 10, R] | LAST [10, R] | HITS [2, R];  op [R] f64;
    status [R] u8;  fail_surf [R] i16;  pupil [2, R] f64 or None.
    Slots the trace does not write (segments past a failure, LAST/HITS rows of
    failed rays) keep the buffer's prior contents: NaN when ``nan_fill``.
    """

    def __init__(self, torch, device, n_seg, R, out_mode, want_pupil, nan_fill, ld=None):
        self.ld = padded_ld(R) if ld is None else max(int(ld), 1)
        if out_mode == abi.OUT_FULL:
            shape = (n_seg, abi.SEG_DOUBLES, self.ld)
        elif out_mode == abi.OUT_LAST:
            shape = (abi.SEG_DOUBLES, self.ld)
        elif out_mode == abi.OUT_OPD:
            shape = (1, self.ld)
        elif out_mode == abi.OUT_FAN:
            shape = (3, self.ld)
        else:
            shape = (2, self.ld)
        new = (lambda s: torch.full(s, float('nan'), dtype=torch.float64, device=device)) \
            if nan_fill else (lambda s: torch.empty(s, dtype=torch.float64, device=device))
        self.R = R
        self.out_mode = out_mode
        self._torch = torch
        self._seg = new(shape)                  # pitched storage
        self.seg = self._seg[..., :R]           # [.., R] view the callers index
        self.op = new((R,))
        self.status = torch.empty((R,), dtype=torch.uint8, device=device)
        self.fail_surf = torch.empty((R,), dtype=torch.int16, device=device)
        self._pupil = new((2, self.ld)) if want_pupil else None
        self.pupil = self._pupil[:, :R] if want_pupil else None

    def out_struct(self):
        o = abi.Out()
        o.seg = self._seg.data_ptr()
        o.op = self.op.data_ptr()
        o.status = self.status.data_ptr()
        o.fail_surf = self.fail_surf.data_ptr()
        o.pupil = self._pupil.data_ptr() if self._pupil is not None else None
        o.ld = self.ld
        return o

    def to_host(self, want=('seg', 'op', 'status', 'fail_surf', 'pupil')):
        """NumPy copies of the arrays named in ``want`` (others None), through
        pooled pinned memory, one synchronisation"""
        class _H:
            pass
        h = _H()
        h.R, h.out_mode = self.R, self.out_mode
        torch = self._torch
        pend = []
        for name in ('seg', 'op', 'status', 'fail_surf', 'pupil'):
            t = getattr(self, name) if name in want else None
            if t is None:
                setattr(h, name, None)
                continue
            lease = _pool.take(torch, t.numel() * t.element_size())
            dst = lease.tensor[:t.numel() * t.element_size()].view(t.dtype).view(t.shape)
            dst.copy_(t, non_blocking=True)
            pend.append((name, lease, t))
        torch.cuda.current_stream(self.seg.device).synchronize()
        for name, lease, t in pend:
            setattr(h, name, lease.array(t.shape, _NP_DTYPES[t.dtype]))
        return h


class HitsPack:
    """A buffer that ROX_OUT_HITS_COMPACT | ROX_HITS_APPEND launches pack their
    surviving (x, y) pairs into, one launch behind the other, with the running
    count on the device: ``xy`` [cap, 2] f64 in HBM -- or ``dest`` = (pointer,
    capacity) of other device-visible memory, e.g. a slice of a pinned shared host
    segment -- ``count`` [1] i64, and the cumulative count after each launch."""

    def __init__(self, torch, device, cap, max_launches, dest=None):
        self._torch, self.device = torch, device
        if dest is None:
            self.xy = torch.empty((int(cap), 2), dtype=torch.float64, device=device)
            self.seg_ptr, self.cap = self.xy.data_ptr(), int(cap)
        else:
            self.xy = None
            self.seg_ptr, self.cap = int(dest[0]), int(dest[1])
        self.count = torch.zeros(1, dtype=torch.int64, device=device)
        self.cum = torch.zeros(max(int(max_launches), 1), dtype=torch.int64, device=device)
        self.n_launches = 0
        self.rays = 0

    def counts(self):
        """survivors per launch (synchronises the launch stream).  The kernels never store
        at or beyond the capacity handed to them (rox_out.ld); a launch that needed more
        leaves a negative running count, reported here"""
        c = self.cum[:self.n_launches].cpu().numpy()
        if (c < 0).any():
            k = int(np.argmax(c < 0))
            raise EngineError(f'HitsPack overflow: launch {k} needed {-int(c[k])} pairs of room, '
                              f'the destination holds {self.cap}')
        return np.diff(np.concatenate([[0], c])).astype(np.int64)


def _in_flight(fn):
    """a TraceEngine entry that uses the device handle (see TraceEngine.__init__)"""
    @functools.wraps(fn)
    def guarded(self, *args, **kwargs):
        self._enter()
        try:
            return fn(self, *args, **kwargs)
        finally:
            self._leave()
    return guarded


class ModelMemo:
    """What the drop-in layer remembers per MODEL STATE -- i.e. per engine: a model edit makes a
    new engine (session.engine_for), so nothing here outlives the state it was computed from.

    ``chief_rays``  {(bytes(rox_field), wavelength index): (seg [N, 10], op) | None}: the
                    one-launch chief-ray batch of trace.trace_chief_ray
    ``obj_coords``  the memo of ``osp.obj_coords(fld)`` (table._obj_coords: the reverse
                    chief-ray iteration of real-image-height fields, once per launch
                    instead of once per ray)
    ``scratch``     device-resident launch outputs that product calls reduce on the device
                    (trace.trace_grid_spot_stats)

    session.engine_for hands one engine to every thread that traces the same model: writers
    hold ``lock``."""
    __slots__ = ('lock', 'chief_rays', 'obj_coords', 'scratch')

    def __init__(self):
        self.lock = threading.Lock()
        self.chief_rays = {}
        self.obj_coords = {}
        self.scratch = {}       # device buffers the product calls reuse ({(thread, rays): DeviceResult})

    def clear(self):
        with self.lock:
            self.chief_rays.clear()
            self.obj_coords.clear()
            self.scratch.clear()


class TraceEngine:
    """one immutable surface table on one GPU.

    A model edit means a new engine, as ``path_sequence.cache_clear()`` does in
    the reference (rayoptics/seq/sequential.py:666-668)."""

    def __init__(self, table: SurfaceTable, device=None):
        import torch
        if not torch.cuda.is_available():
            raise EngineError('no GPU visible: the trace engine has no CPU fallback')
        self.torch = torch
        _np_dtypes(torch)
        self.lib = load_library()
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None
                                   else torch.device(device).index or 0)
        self.table = table
        self.memo = ModelMemo()         # cleared by close()
        self._nseg = {}
        self._handle = C.c_void_p()
        # lifetime of the device handle under threads (session.engine_for hands one engine to
        # every thread that traces the same model, and evicts by LRU): calls in flight are
        # counted; close() with calls in flight is carried out by the last of them; a call on
        # a closed engine re-creates the handle from the table it was built from.  The handle
        # is therefore never destroyed under a running rox_* call (ctypes drops the GIL).
        self._life = threading.Lock()
        self._calls = 0
        self._close_pending = False
        with self._life:
            self._open()

    def _open(self):
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_set_device(self.device.index), 'rox_set_device')
            _check(self.lib.rox_system_create(self.table.rows, self.table.n_ifcs,
                                              self.table.n_table.ctypes.data,
                                              self.table.wvls_arr.ctypes.data,
                                              len(self.table.wvls), C.byref(self._handle)),
                   'rox_system_create')

    def _destroy(self):
        if self._handle:
            self.lib.rox_system_destroy(self._handle)
            self._handle = C.c_void_p()
        self._close_pending = False

    def _enter(self):
        with self._life:
            if not self._handle:
                self._open()
            self._calls += 1

    def _leave(self):
        with self._life:
            self._calls -= 1
            if self._calls == 0 and self._close_pending:
                self._destroy()

    @property
    def is_open(self):
        return bool(self._handle)

    def close(self):
        """destroy the device handle -- at once, or, with calls in flight on other threads,
        when the last of them returns.  A later call re-creates it."""
        self.memo.clear()
        with self._life:
            if self._calls > 0:
                self._close_pending = True
            else:
                self._destroy()

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    # -- helpers ------------------------------------------------------------
    @_in_flight
    def num_segments(self, flags=0):
        n = C.c_int32()
        _check(self.lib.rox_system_num_segments(self._handle, int(flags), C.byref(n)),
               'rox_system_num_segments')
        return n.value

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, x, dtype):
        t = self.torch
        if isinstance(x, t.Tensor):
            return x.to(device=self.device, dtype=dtype).contiguous()
        return t.from_numpy(np.ascontiguousarray(x)).to(device=self.device, dtype=dtype)

    def _result(self, R, opts, want_pupil, nan_fill, out):
        if out is not None:
            return out
        return DeviceResult(self.torch, self.device, self.num_segments(opts.flags), R,
                            opts.out_mode, want_pupil, nan_fill)

    # -- entries --------------------------------------------------------------
    @_in_flight
    def trace_rays(self, pt0, dir0, wvl_idx=0, opts=None, nan_fill=False, out=None):
        """pt0, dir0: [3, R] (numpy or torch); wvl_idx: int or int32[R]"""
        t = self.torch
        opts = opts or make_opts()
        pt0 = self._dev(pt0, t.float64)
        dir0 = self._dev(dir0, t.float64)
        R = pt0.shape[1]
        if np.ndim(wvl_idx) == 0 and not isinstance(wvl_idx, t.Tensor):
            wi, wi_ptr, wi_all = None, None, int(wvl_idx)
        else:
            wi = self._dev(wvl_idx, t.int32)
            wi_ptr, wi_all = wi.data_ptr(), 0
        res = self._result(R, opts, False, nan_fill, out)
        o = res.out_struct()
        with t.cuda.device(self.device):
            _check(self.lib.rox_trace_rays(self._handle, R, pt0.data_ptr(), dir0.data_ptr(),
                                           wi_ptr, wi_all, C.byref(opts), C.byref(o),
                                           self._stream()), 'rox_trace_rays')
        res._keep = (pt0, dir0, wi)     # inputs must outlive the async launch
        return res

    @_in_flight
    def trace_pupil_grid(self, fld, grid, wvl_idx=0, opts=None, want_pupil=True,
                         nan_fill=False, out=None):
        opts = opts or make_opts()
        R = grid_rays(grid)
        res = self._result(R, opts, want_pupil, nan_fill, out)
        o = res.out_struct()
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_trace_pupil_grid(self._handle, C.byref(fld), C.byref(grid),
                                                 int(wvl_idx), C.byref(opts), C.byref(o),
                                                 self._stream()), 'rox_trace_pupil_grid')
        return res

    def _batch_args(self, flds, wvl_idxs, opts_list, outs):
        n = len(flds)
        if not (len(wvl_idxs) == len(opts_list) == len(outs) == n):
            raise EngineError('trace_pupil_grids: flds, wvl_idxs, opts and outs differ in length')
        f_arr = (abi.Field * n)(*flds)
        w_arr = (C.c_int32 * n)(*[int(w) for w in wvl_idxs])
        o_arr = (abi.Opts * n)(*opts_list)
        out_arr = (abi.Out * n)(*outs)
        return n, f_arr, w_arr, o_arr, out_arr

    @_in_flight
    def trace_pupil_grids(self, flds, wvl_idxs, grid, opts_list, want_pupil=True,
                          nan_fill=False, outs=None):
        """``grid`` traced for every (flds[i], wvl_idxs[i], opts_list[i]) in ONE launch
        (rox_trace_pupil_grids): the (field x wavelength) loops of a spot diagram, a set of
        ray fans or a wavefront map.  Returns one DeviceResult per item; each is what
        trace_pupil_grid would have returned for it."""
        R = grid_rays(grid)
        n = len(flds)
        res = [self._result(R, opts_list[i], want_pupil, nan_fill, outs[i] if outs else None)
               for i in range(n)]
        n, f_arr, w_arr, o_arr, out_arr = self._batch_args(flds, wvl_idxs, opts_list,
                                                           [r.out_struct() for r in res])
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_trace_pupil_grids(self._handle, n, f_arr, w_arr, C.byref(grid),
                                                  o_arr, out_arr, self._stream()),
                   'rox_trace_pupil_grids')
        return res

    @_in_flight
    def trace_pupil_grids_host(self, flds, wvl_idxs, grid, opts_list):
        """FULL / LAST packets (or the FAN / OPD / HITS rows) of several small pupil grids by ONE
        launch whose stores go straight into one pinned host block -- no copy-engine transfer,
        one synchronise -- for figure-sized batches (the chief rays of every field and
        wavelength of a model, trace.trace_chief_ray; the fans of a RayFanFigure).  Returns one host result per item (``seg`` [n_seg, 10, R],
        ``op``, ``status``, ``fail_surf``, ``pupil``: NumPy views of the block; segments past
        a failure are NaN)."""
        R = grid_rays(grid)
        n = len(flds)
        mode = opts_list[0].out_mode
        # every item's slice of the pinned block is sized from the first item's output mode and
        # segment count: the library takes per-item options, so a list that mixes them would
        # have the kernel write past a slice (the library checks the same for a batched launch,
        # but falls back to per-item launches for a single item)
        ph = opts_list[0].flags & abi.FILTER_PHANTOMS
        for o in opts_list:
            if o.out_mode != mode or (o.flags & abi.FILTER_PHANTOMS) != ph:
                raise EngineError('trace_pupil_grids_host: out_mode and FILTER_PHANTOMS must be the '
                                  'same for every item')
        if len(opts_list) != n or len(wvl_idxs) != n:
            raise EngineError('trace_pupil_grids_host: one wavelength index and one rox_opts per field')
        if mode == abi.OUT_FULL:
            rows = self.num_segments(opts_list[0].flags) * abi.SEG_DOUBLES
        else:
            rows = {abi.OUT_LAST: abi.SEG_DOUBLES, abi.OUT_OPD: 1, abi.OUT_FAN: 3, abi.OUT_HITS: 2}[mode]
        b_seg, b_op, b_pu = 8 * rows * R, 8 * R, 16 * R
        b_st, b_fs = (R + 15) // 16 * 16, (2 * R + 15) // 16 * 16
        per = b_seg + b_op + b_pu + b_st + b_fs
        lease = _pool.take(self.torch, per * n)
        whole = lease.array((per * n // 8,), np.float64)
        whole.fill(np.nan)
        outs, views = [], []
        for i in range(n):
            base = lease.ptr + i * per
            o = abi.Out()
            o.seg, o.op, o.pupil = base, base + b_seg, base + b_seg + b_op
            o.status = base + b_seg + b_op + b_pu
            o.fail_surf = o.status + b_st
            o.ld = R
            outs.append(o)
            off = i * per

            class _H:
                pass
            h = _H()
            h.R, h.out_mode = R, mode
            h.seg = lease.array((rows // abi.SEG_DOUBLES, abi.SEG_DOUBLES, R) if mode == abi.OUT_FULL
                                else (rows, R), np.float64, off)
            h.op = lease.array((R,), np.float64, off + b_seg)
            h.pupil = lease.array((2, R), np.float64, off + b_seg + b_op)
            h.status = lease.array((R,), np.uint8, off + b_seg + b_op + b_pu)
            h.fail_surf = lease.array((R,), np.int16, off + b_seg + b_op + b_pu + b_st)
            views.append(h)
        n, f_arr, w_arr, o_arr, out_arr = self._batch_args(flds, wvl_idxs, opts_list, outs)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_trace_pupil_grids(self._handle, n, f_arr, w_arr, C.byref(grid),
                                                  o_arr, out_arr, self._stream()),
                   'rox_trace_pupil_grids')
        self.torch.cuda.current_stream(self.device).synchronize()
        return views

    @_in_flight
    def trace_pupil_grids_hits(self, flds, wvl_idxs, grid, opts_list):
        """ROX_OUT_HITS_COMPACT for several (field, wavelength) pairs in one launch: a list of
        (R_ok, 2) arrays, each a view of the pinned block the kernel packed that item's
        survivors into (one synchronise for all of them)."""
        R = grid_rays(grid)
        leases, outs = [], []
        for _ in flds:
            lease, o, _st = self._hits_out(R)
            leases.append(lease)
            outs.append(o)
        n, f_arr, w_arr, o_arr, out_arr = self._batch_args(flds, wvl_idxs, opts_list, outs)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_trace_pupil_grids(self._handle, n, f_arr, w_arr, C.byref(grid),
                                                  o_arr, out_arr, self._stream()),
                   'rox_trace_pupil_grids')
        self.torch.cuda.current_stream(self.device).synchronize()
        return [lease.array((C.c_int64.from_address(lease.ptr + 16 * R).value, 2), np.float64)
                for lease in leases]

    @_in_flight
    def trace_pupil_list(self, fld, px, py, wvl_idx=0, opts=None, want_pupil=True,
                         nan_fill=False, out=None):
        t = self.torch
        opts = opts or make_opts()
        px = self._dev(px, t.float64)
        py = self._dev(py, t.float64)
        R = px.shape[0]
        res = self._result(R, opts, want_pupil, nan_fill, out)
        o = res.out_struct()
        with t.cuda.device(self.device):
            _check(self.lib.rox_trace_pupil_list(self._handle, C.byref(fld), R, px.data_ptr(),
                                                 py.data_ptr(), int(wvl_idx), C.byref(opts),
                                                 C.byref(o), self._stream()),
                   'rox_trace_pupil_list')
        res._keep = (px, py)
        return res

    @_in_flight
    def trace_pupil_np(self, fld, wvl_idx, opts, grid=None, px=None, py=None):
        """A SMALL pupil launch (a fan, a handful of rays, a figure-sized grid) with plain NumPy
        buffers through the library's ROX_HOST_POINTERS path: inputs and results cross in one
        device-mapped pinned block that the kernel reads and writes directly -- one launch, one
        synchronise, no torch tensors, no copy-engine transfers (a DeviceResult + to_host costs
        five device-to-host copies: ~1.2 ms of a RayFanFigure refresh went there).  Returns the
        host result (``seg`` [n_seg, 10, R] or [rows, R], ``op``, ``status``, ``fail_surf``,
        ``pupil``; slots the trace does not produce are NaN).  Callers keep it to batches of
        at most HOST_DIRECT_BYTES."""
        mode = opts.out_mode
        if grid is not None:
            R = grid_rays(grid)
        else:
            px = np.ascontiguousarray(px, dtype=np.float64)
            py = np.ascontiguousarray(py, dtype=np.float64)
            R = px.shape[0]
        if mode == abi.OUT_FULL:
            key = opts.flags & abi.FILTER_PHANTOMS
            nseg = self._nseg.get(key)
            if nseg is None:
                nseg = self._nseg[key] = self.num_segments(opts.flags)
            shape = (nseg, abi.SEG_DOUBLES, R)
        else:
            shape = ({abi.OUT_LAST: abi.SEG_DOUBLES, abi.OUT_OPD: 1, abi.OUT_FAN: 3, abi.OUT_HITS: 2}[mode], R)

        class _H:
            pass
        h = _H()
        h.R, h.out_mode = R, mode
        h.seg = np.empty(shape)
        h.op = np.empty(R)
        h.status = np.empty(R, dtype=np.uint8)
        h.fail_surf = np.empty(R, dtype=np.int16)
        h.pupil = np.empty((2, R))
        o = abi.Out()
        o.seg, o.op, o.status = h.seg.ctypes.data, h.op.ctypes.data, h.status.ctypes.data
        o.fail_surf, o.pupil, o.ld = h.fail_surf.ctypes.data, h.pupil.ctypes.data, R
        saved = opts.flags
        opts.flags = saved | abi.HOST_POINTERS
        try:
            with self.torch.cuda.device(self.device):
                if grid is not None:
                    rc = self.lib.rox_trace_pupil_grid(self._handle, C.byref(fld), C.byref(grid), int(wvl_idx),
                                                       C.byref(opts), C.byref(o), self._stream())
                else:
                    rc = self.lib.rox_trace_pupil_list(self._handle, C.byref(fld), R, px.ctypes.data,
                                                       py.ctypes.data, int(wvl_idx), C.byref(opts),
                                                       C.byref(o), self._stream())
        finally:
            opts.flags = saved
        _check(rc, 'rox_trace_pupil_grid' if grid is not None else 'rox_trace_pupil_list')
        return h

    @_in_flight
    def trace_rays_np(self, pt0, dir0, wvl_idx, opts):
        """explicit rays ([3, R] arrays, one wavelength index or R of them) with plain NumPy
        buffers through ROX_HOST_POINTERS -- the small-batch form of :meth:`trace_rays`, see
        :meth:`trace_pupil_np`"""
        pt0 = np.ascontiguousarray(pt0, dtype=np.float64)
        dir0 = np.ascontiguousarray(dir0, dtype=np.float64)
        R = pt0.shape[1]
        mode = opts.out_mode
        if mode == abi.OUT_FULL:
            shape = (self.num_segments(opts.flags), abi.SEG_DOUBLES, R)
        else:
            shape = ({abi.OUT_LAST: abi.SEG_DOUBLES, abi.OUT_HITS: 2}[mode], R)
        if np.ndim(wvl_idx) == 0:
            wi, wi_ptr, wi_all = None, None, int(wvl_idx)
        else:
            wi = np.ascontiguousarray(wvl_idx, dtype=np.int32)
            wi_ptr, wi_all = wi.ctypes.data, 0

        class _H:
            pass
        h = _H()
        h.R, h.out_mode, h.pupil = R, mode, None
        h.seg = np.empty(shape)
        h.op = np.empty(R)
        h.status = np.empty(R, dtype=np.uint8)
        h.fail_surf = np.empty(R, dtype=np.int16)
        o = abi.Out()
        o.seg, o.op, o.status = h.seg.ctypes.data, h.op.ctypes.data, h.status.ctypes.data
        o.fail_surf, o.ld = h.fail_surf.ctypes.data, R
        saved = opts.flags
        opts.flags = saved | abi.HOST_POINTERS
        try:
            with self.torch.cuda.device(self.device):
                rc = self.lib.rox_trace_rays(self._handle, R, pt0.ctypes.data, dir0.ctypes.data, wi_ptr,
                                             wi_all, C.byref(opts), C.byref(o), self._stream())
        finally:
            opts.flags = saved
        _check(rc, 'rox_trace_rays')
        return h

    # -- spot diagram: hits compacted on the device, written to pinned memory ----
    def _hits_out(self, R, want_status=False):
        """a pinned block for up to R (x, y) pairs + the count, and its rox_out"""
        lease = _pool.take(self.torch, 16 * R + 64)
        o = abi.Out()
        o.seg = lease.ptr
        o.n_hits = lease.ptr + 16 * R           # 8-byte count behind the pairs
        o.ld = R
        st = None
        if want_status:
            st = self.torch.empty((R,), dtype=self.torch.uint8, device=self.device)
            o.status = st.data_ptr()
        return lease, o, st

    def _hits_finish(self, lease, R):
        self.torch.cuda.current_stream(self.device).synchronize()
        n = C.c_int64.from_address(lease.ptr + 16 * R).value
        return lease.array((n, 2), np.float64)

    @_in_flight
    def trace_pupil_grid_hits(self, fld, grid, wvl_idx, opts):
        """ROX_OUT_HITS_COMPACT over a pupil grid: the (R_ok, 2) array of
        transverse aberrations, in ray order, as a NumPy array that views the
        pinned buffer the kernel wrote (no device->host copy, no host copy)."""
        R = grid_rays(grid)
        lease, o, _st = self._hits_out(R)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_trace_pupil_grid(self._handle, C.byref(fld), C.byref(grid),
                                                 int(wvl_idx), C.byref(opts), C.byref(o),
                                                 self._stream()), 'rox_trace_pupil_grid')
        return self._hits_finish(lease, R)

    def hits_pack(self, cap, max_launches, dest=None):
        return HitsPack(self.torch, self.device, cap, max_launches, dest)

    @_in_flight
    def spot_stats(self, res, x_edges=None, y_edges=None):
        """rox_spot_stats over the device-resident output of a ROX_OUT_HITS launch
        (``res``: a DeviceResult of that mode -- rays that did not reach the image are skipped):
        ``(summary, hist)`` with ``summary`` a dict (n, centroid, rms_radius about the centroid,
        min / max per axis, the raw sums) and ``hist`` = numpy.histogram2d(x, y, bins=[x_edges,
        y_edges])[0] as uint32 (None without edges).  Nothing but 72 bytes and the histogram
        crosses PCIe (RayGeoPSF's 2-D histogram, rayoptics/mpl/analysisfigure.py:237-290)."""
        if res.out_mode != abi.OUT_HITS:
            raise EngineError('spot_stats reads the rows of a ROX_OUT_HITS launch')
        return self._spot_stats(res.seg.data_ptr(), res.ld, res.status.data_ptr(), None, res.R,
                                abi.SPOT_ROWS, x_edges, y_edges)

    @_in_flight
    def trace_pupil_grid_focus(self, fld, grid, wvl_idx, opts, planes, want_rows=False,
                               want_stats=True):
        """rox_trace_through_focus: trace the pupil grid once and evaluate it at every focus
        plane (``planes``: a sequence of abi.FocusPlane, a FAN launch's foc / image_pt / wf
        each).  ``opts.out_mode`` must be OUT_FAN.  Returns the per-plane statistics as a
        NumPy structured array of FOCUS_STATS_DTYPE (None with ``want_stats=False``) and,
        with ``want_rows``, ``(stats, FocusRows)`` -- rows bit-identical to one
        ``trace_pupil_grid`` FAN launch per plane."""
        t = self.torch
        planes = list(planes)
        K = len(planes)
        p_arr = (abi.FocusPlane * max(K, 1))(*planes)
        R = grid_rays(grid)
        ld = padded_ld(R)
        rows = status = None
        if want_rows:
            rows = t.full((max(K, 1), 3, ld), float('nan'), dtype=t.float64, device=self.device)
            status = t.empty((R,), dtype=t.uint8, device=self.device)
        stats = np.empty(max(K, 1), dtype=FOCUS_STATS_DTYPE) if want_stats else None
        with t.cuda.device(self.device):
            _check(self.lib.rox_trace_through_focus(
                self._handle, C.byref(fld), C.byref(grid), int(wvl_idx), C.byref(opts), K, p_arr,
                rows.data_ptr() if rows is not None else None, ld,
                status.data_ptr() if status is not None else None,
                stats.ctypes.data if stats is not None else None, self._stream()),
                'rox_trace_through_focus')
        if not want_rows:
            return stats
        return stats, FocusRows(rows[:, :, :R], status)

    @_in_flight
    def trace_pupil_grids_focus(self, flds, wvl_idxs, grids, opts_list, planes, want_rows=False,
                                want_stats=True):
        """rox_trace_through_focus_grids: n_items through-focus scans in one launch -- item i is
        ``trace_pupil_grid_focus(flds[i], grids[i], wvl_idxs[i], opts_list[i], planes[i])``
        (``planes``: n_items lists of K abi.FocusPlane each; the grids may differ in start /
        stop only).  Returns the statistics as a FOCUS_STATS_DTYPE array [n_items, K] (None with
        ``want_stats=False``) and, with ``want_rows``, ``(stats, FocusRows)`` with rows
        [n_items, K, 3, R] and status [n_items, R] -- each item bit-identical to its single
        call."""
        t = self.torch
        flds, grids, opts_list = list(flds), list(grids), list(opts_list)
        planes = [list(p) for p in planes]
        n = len(flds)
        K = len(planes[0]) if planes else 0
        if not (len(wvl_idxs) == len(grids) == len(opts_list) == len(planes) == n) or \
                any(len(p) != K for p in planes):
            raise EngineError('trace_pupil_grids_focus: one field, wavelength, grid, opts and '
                              'list of K planes per item')
        f_arr = (abi.Field * max(n, 1))(*flds)
        w_arr = (C.c_int32 * max(n, 1))(*[int(w) for w in wvl_idxs])
        g_arr = (abi.Grid * max(n, 1))(*grids)
        o_arr = (abi.Opts * max(n, 1))(*opts_list)
        p_arr = (abi.FocusPlane * max(n * K, 1))(*[p for ps in planes for p in ps])
        R = grid_rays(grids[0]) if n else 0
        ld = padded_ld(R)
        rows = status = None
        if want_rows:
            rows = t.full((max(n, 1), max(K, 1), 3, ld), float('nan'), dtype=t.float64, device=self.device)
            status = t.empty((max(n, 1), ld), dtype=t.uint8, device=self.device)
        stats = np.empty((max(n, 1), max(K, 1)), dtype=FOCUS_STATS_DTYPE) if want_stats else None
        with t.cuda.device(self.device):
            _check(self.lib.rox_trace_through_focus_grids(
                self._handle, n, f_arr, w_arr, g_arr, o_arr, K, p_arr,
                rows.data_ptr() if rows is not None else None, ld,
                status.data_ptr() if status is not None else None,
                stats.ctypes.data if stats is not None else None, self._stream()),
                'rox_trace_through_focus_grids')
        if not want_rows:
            return stats
        return stats, FocusRows(rows[:, :, :, :R], status[:, :R])

    def _focus_rows(self, focus_rows, what):
        """the [n_items][K][3][ld] rows and [n_items][ld] status of a through-focus launch (a
        single scan gains the item axis) -> (rows, status, n_items, K, ld)"""
        rows, status = focus_rows.rows, focus_rows.status
        if rows.dim() == 3:
            rows, status = rows.unsqueeze(0), status.unsqueeze(0)
        n_items, K = int(rows.shape[0]), int(rows.shape[1])
        ld = int(rows.stride(2))
        if rows.dtype != self.torch.float64 or rows.stride(3) != 1 or rows.stride(1) != 3 * ld or \
                rows.stride(0) != K * 3 * ld or status.stride(-1) != 1 or \
                (n_items > 1 and status.stride(0) != ld):
            raise EngineError(f'{what} reads the [n_items][K][3][ld] rows and [n_items][ld] status '
                              'of a through-focus launch')
        return rows, status, n_items, K, ld

    def _psf_stack(self, psf, what):
        """the contiguous float64 [n_items][K][M][M] PSFs of focus_psf -> (n_items, K, M)"""
        if psf.dim() != 4 or psf.dtype != self.torch.float64 or not psf.is_contiguous() or \
                int(psf.shape[2]) != int(psf.shape[3]):
            raise EngineError(f'{what} reads the contiguous float64 [n_items][K][M][M] PSFs of focus_psf')
        return int(psf.shape[0]), int(psf.shape[1]), int(psf.shape[2])

    def _out(self, on_device, shape, dtype, tdtype, tshape=None):
        """an array a C entry writes -> (array, pointer): a torch tensor on this engine's device
        (of shape ``tshape``, default ``shape``) with ``on_device``, else a NumPy array"""
        if on_device:
            a = self.torch.empty(shape if tshape is None else tshape, dtype=tdtype, device=self.device)
            return a, a.data_ptr()
        a = np.empty(shape, dtype=dtype)
        return a, a.ctypes.data

    def _records_out(self, on_device, shape, dtype):
        """_out for the records of a C struct: a ``dtype`` array, or with ``on_device`` a uint8
        tensor of the struct's bytes per record (``records_view`` reads it on the host)"""
        return self._out(on_device, shape, dtype, self.torch.uint8, (*shape, dtype.itemsize))

    def _packets(self, results, trace_flags, what, modes=(abi.OUT_FULL,), num=None):
        """the FULL packets of finished launches (a single DeviceResult gains the item axis) ->
        (results, n_items, n_seg, R, outs), outs the abi.Out array a packet entry reads.  An entry
        that reads other packets too names their ``modes`` (every item then has the first one's, and
        n_seg is what that one holds, 1 for OUT_LAST); one that reads ``num`` x ``num`` product
        grids names ``num``"""
        results = [results] if isinstance(results, DeviceResult) else list(results)
        n_items = len(results)
        if not 1 <= n_items <= abi.MAX_FOCUS_ITEMS:
            raise EngineError(f'{what}: 1 to {abi.MAX_FOCUS_ITEMS} items, got {n_items}')
        if num is not None and not 2 <= num <= abi.MAX_SA_NUM:
            raise EngineError(f'{what}: num {num} outside [2, {abi.MAX_SA_NUM}]')
        mode = results[0].out_mode if len(modes) > 1 else modes[0]
        if mode not in modes:
            raise EngineError(f'{what}: reads OUT_LAST or OUT_FULL packets, not out_mode {mode}')
        if len(modes) > 1:
            n_seg = int(results[0].seg.shape[0]) if mode == abi.OUT_FULL else 1
        else:
            n_seg = self.num_segments(int(trace_flags))
        R = int(results[0].R) if num is None else num * num
        for i, r in enumerate(results):
            if r.out_mode != mode or (mode == abi.OUT_FULL and int(r.seg.shape[0]) != n_seg) or int(r.R) != R:
                raise EngineError(f'{what}: item {i} is not a FULL packet of {n_seg} segments and {R} rays'
                                  if num is None else f'{what}: item {i} is not a packet of out_mode {mode}, '
                                  f'{n_seg} segments and {num} x {num} rays')
        return results, n_items, n_seg, R, (abi.Out * n_items)(*[r.out_struct() for r in results])

    def _weight_rows(self, what, weight, weight_row, n_items, R):
        """the ``weight`` of a packet entry -- a contiguous float64 device tensor [n_items, n_rows,
        >= R], row ``weight_row`` of which weighs the rays; None: no weights -> (the DEVICE
        pointer of item 0's row or None, weight_stride)"""
        t = self.torch
        if weight is None:
            return None, 0
        if not hasattr(weight, 'data_ptr') or weight.dim() != 3 or weight.dtype != t.float64 or \
                not weight.is_contiguous() or not weight.is_cuda or int(weight.shape[0]) != n_items or \
                int(weight.shape[2]) < R or not 0 <= int(weight_row) < int(weight.shape[1]):
            raise EngineError(f'{what}: weight is a contiguous float64 device tensor [{n_items}, n_rows, '
                              f'R >= {R}] and weight_row one of its rows')
        return (weight.data_ptr() + 8 * int(weight_row) * int(weight.shape[2]),
                int(weight.shape[1]) * int(weight.shape[2]))

    @_in_flight
    def focus_psf(self, focus_rows, ndim, maxdim, wave_scale, want_psf=True):
        """rox_focus_psf over the rows of a through-focus launch (``focus_rows``: the FocusRows
        trace_pupil_grid_focus / trace_pupil_grids_focus return, still in HBM): the OPD grid in
        waves of each plane is ``wave_scale[i] * OPD`` of item i's first ndim*ndim rays (NaN where
        a ray failed), its PSF bit-identical to calc_psf of that grid.  Returns ``(psf, stats)``:
        the PSFs as a float64 tensor in HBM [n_items, K, maxdim, maxdim] (None without
        ``want_psf``) and a FOCUS_PSF_STATS_DTYPE array [n_items, K] (n, strehl, psf_peak)."""
        t = self.torch
        rows, status, n_items, K, ld = self._focus_rows(focus_rows, 'focus_psf')
        scale = _f64(wave_scale, (n_items,))
        ndim, maxdim = int(ndim), int(maxdim)
        if ndim * ndim > int(rows.shape[3]) or ndim * ndim > int(status.shape[-1]):
            raise EngineError(f'focus_psf: a {ndim} x {ndim} grid needs {ndim * ndim} rays, the rows hold '
                              f'{int(rows.shape[3])}')
        psf = t.empty((n_items, K, maxdim, maxdim), dtype=t.float64, device=self.device) if want_psf else None
        stats = np.empty((n_items, K), dtype=FOCUS_PSF_STATS_DTYPE)
        with t.cuda.device(self.device):
            _check(self.lib.rox_focus_psf(n_items, K, rows.data_ptr(), ld, status.data_ptr(),
                                          scale.ctypes.data, ndim, maxdim,
                                          psf.data_ptr() if psf is not None else None,
                                          stats.ctypes.data, self._stream()), 'rox_focus_psf')
        return psf, stats

    @_in_flight
    def focus_mtf(self, psf, pitch, freqs, on_device=False):
        """rox_focus_mtf over the PSFs focus_psf returns (``psf``: float64 [n_items, K, M, M] in
        HBM): the line OTF of every plane along image x and y at the frequencies ``freqs``
        (cycles per system unit), ``pitch`` (broadcast to [n_items, K]) being each plane's pixel
        pitch.  Returns a complex128 array [n_items, K, 2, Q] (direction 0 = x, 1 = y), or with
        ``on_device`` a complex128 tensor of that shape in HBM.  NaN above a plane's Nyquist
        frequency and on planes no ray reached."""
        t = self.torch
        n_items, K, M = self._psf_stack(psf, 'focus_mtf')
        p = _f64(pitch, (n_items, K))
        f = np.ascontiguousarray(np.asarray(freqs, dtype=np.float64).reshape(-1))
        Q = int(f.size)
        out, ptr = self._out(on_device, (n_items, K, 2, Q, 2), np.float64, t.float64)
        with t.cuda.device(self.device):
            _check(self.lib.rox_focus_mtf(n_items, K, psf.data_ptr(), M, p.ctypes.data, Q, f.ctypes.data,
                                          ptr, self._stream()), 'rox_focus_mtf')
        if on_device:
            return t.view_as_complex(out)
        return out.view(np.complex128)[..., 0]

    @_in_flight
    def focus_ee(self, focus_rows, n_rays, centers, radii, fractions, on_device=False):
        """rox_focus_ee over the rows of a through-focus launch (``focus_rows``: the FocusRows
        trace_pupil_grid_focus / trace_pupil_grids_focus return, still in HBM): the geometric
        encircled energy of each plane's spot over the first ``n_rays`` rays with status OK,
        about ``centers`` (broadcast to [n_items, K, 2], in the rows' coordinates; None = the
        image point).  ``radii`` (broadcast to [n_items, K, Nr], non-decreasing per plane; None
        for no counts) and ``fractions`` ([Nf] in (0, 1]; None for no radii).  Returns
        ``(counts, ee_radius, n_ok)``: int64 [n_items, K, Nr] rays with d2 <= r^2, float64
        [n_items, K, Nf] the exact order-statistic radius that holds each fraction (NaN where no
        ray arrived), int64 [n_items, K] -- NumPy, or torch tensors in HBM with ``on_device``;
        None for what was not asked."""
        t = self.torch
        rows, status, n_items, K, ld = self._focus_rows(focus_rows, 'focus_ee')
        n_rays = int(n_rays)
        if not 1 <= n_rays <= min(int(rows.shape[3]), int(status.shape[-1])):
            raise EngineError(f'focus_ee: n_rays {n_rays} outside [1, {int(rows.shape[3])}]')
        if radii is None and fractions is None:
            raise EngineError('focus_ee: radii or fractions (or both)')
        c = _f64(centers, (n_items, K, 2)) if centers is not None else None
        r = f = None
        Nr = Nf = 0
        if radii is not None:
            r = np.asarray(radii, dtype=np.float64)
            Nr = int(r.shape[-1]) if r.ndim else 1
            r = _f64(r, (n_items, K, Nr))
        if fractions is not None:
            f = np.ascontiguousarray(np.asarray(fractions, dtype=np.float64).reshape(-1))
            Nf = int(f.size)
        none = (None, None)
        counts, p_counts = self._out(on_device, (n_items, K, Nr), np.int64, t.int64) if r is not None else none
        eer, p_eer = self._out(on_device, (n_items, K, Nf), np.float64, t.float64) if f is not None else none
        n_ok, p_nok = self._out(on_device, (n_items, K), np.int64, t.int64)
        with t.cuda.device(self.device):
            _check(self.lib.rox_focus_ee(n_items, K, rows.data_ptr(), ld, status.data_ptr(), n_rays,
                                         c.ctypes.data if c is not None else None, Nr,
                                         r.ctypes.data if r is not None else None, p_counts, Nf,
                                         f.ctypes.data if f is not None else None, p_eer, p_nok,
                                         self._stream()), 'rox_focus_ee')
        return counts, eer, n_ok

    @_in_flight
    def focus_gmtf(self, focus_rows, n_rays, dirs, freqs, edges=None, on_device=False):
        """rox_focus_gmtf over the rows of a through-focus launch (``focus_rows``: the FocusRows
        trace_pupil_grid_focus / trace_pupil_grids_focus return, still in HBM): the geometric OTF
        and the line spread of each plane's spot over the first ``n_rays`` rays with status OK,
        along the directions ``dirs`` (broadcast to [n_items, D, 2] = (ex, ey); a ray projects to
        u = ex*x + ey*y).  ``freqs`` ([Q], cycles per system unit; None for no OTF) and ``edges``
        (broadcast to [n_items, K, D, B + 1], strictly increasing; None for no line spread).
        Returns ``(otf, lsf, n_ok)``: complex128 [n_items, K, D, Q] = mean exp(-2 pi i nu u) (NaN
        where no ray arrived), int64 [n_items, K, D, B] = numpy.histogram(u, edges) counts, int64
        [n_items, K] -- NumPy, or torch tensors in HBM with ``on_device``; None for what was not
        asked."""
        t = self.torch
        rows, status, n_items, K, ld = self._focus_rows(focus_rows, 'focus_gmtf')
        n_rays = int(n_rays)
        if not 1 <= n_rays <= min(int(rows.shape[3]), int(status.shape[-1])):
            raise EngineError(f'focus_gmtf: n_rays {n_rays} outside [1, {int(rows.shape[3])}]')
        if freqs is None and edges is None:
            raise EngineError('focus_gmtf: freqs or edges (or both)')
        dv = np.asarray(dirs, dtype=np.float64)
        if dv.ndim < 1 or dv.shape[-1] != 2:
            raise EngineError('focus_gmtf: dirs are (ex, ey) pairs')
        D = int(dv.shape[-2]) if dv.ndim > 1 else 1
        dv = _f64(dv, (n_items, D, 2))
        f = e = None
        Q = B = 0
        if freqs is not None:
            f = np.ascontiguousarray(np.asarray(freqs, dtype=np.float64).reshape(-1))
            Q = int(f.size)
        if edges is not None:
            e = np.asarray(edges, dtype=np.float64)
            B = int(e.shape[-1]) - 1 if e.ndim else 0
            e = _f64(e, (n_items, K, D, B + 1))
        none = (None, None)
        otf, p_otf = self._out(on_device, (n_items, K, D, Q, 2), np.float64, t.float64) if f is not None else none
        lsf, p_lsf = self._out(on_device, (n_items, K, D, B), np.int64, t.int64) if e is not None else none
        n_ok, p_nok = self._out(on_device, (n_items, K), np.int64, t.int64)
        with t.cuda.device(self.device):
            _check(self.lib.rox_focus_gmtf(n_items, K, rows.data_ptr(), ld, status.data_ptr(), n_rays, D,
                                           dv.ctypes.data, Q, f.ctypes.data if f is not None else None, p_otf,
                                           B, e.ctypes.data if e is not None else None, p_lsf, p_nok,
                                           self._stream()), 'rox_focus_gmtf')
        if otf is not None:
            otf = t.view_as_complex(otf) if on_device else otf.view(np.complex128)[..., 0]
        return otf, lsf, n_ok

    @_in_flight
    def focus_zernike(self, focus_rows, grids, terms, wave_scale, circle=None, on_device=False):
        """rox_focus_zernike over the rows of a through-focus launch (``focus_rows``: the
        FocusRows trace_pupil_grid_focus / trace_pupil_grids_focus return, still in HBM): the
        least-squares Zernike coefficients, in waves, of the OPD ``wave_scale[i] * OPD`` of every
        plane.  ``grids``: one abi.Grid (PRODUCT, whole) per item, or one for all; ``terms``:
        (n, m, scale) triples or abi.ZernikeTerm; ``wave_scale`` broadcast to [n_items];
        ``circle`` broadcast to [n_items, 3] (cx, cy, radius) in pupil coordinates, None = the
        unit circle.  Returns ``(coef, stats)``: float64 [n_items, K, J] and a
        ZERNIKE_STATS_DTYPE array [n_items, K] -- NumPy, or with ``on_device`` a torch tensor in
        HBM and a torch uint8 tensor [n_items, K, 56] of the raw records (``zernike_stats_view``
        reads it on the host)."""
        t = self.torch
        rows, status, n_items, K, ld = self._focus_rows(focus_rows, 'focus_zernike')
        if isinstance(grids, abi.Grid):
            grids = [grids] * n_items
        grids = list(grids)
        if len(grids) == 1:
            grids = grids * n_items
        if len(grids) != n_items:
            raise EngineError(f'focus_zernike: {len(grids)} grids for {n_items} items')
        tl = [tm if isinstance(tm, abi.ZernikeTerm) else
              abi.ZernikeTerm(int(tm[0]), int(tm[1]), float(tm[2]) if len(tm) > 2 else 1.0)
              for tm in terms]
        J = len(tl)
        g_arr = (abi.Grid * max(n_items, 1))(*grids)
        z_arr = (abi.ZernikeTerm * max(J, 1))(*tl)
        ws = _f64(wave_scale, (n_items,))
        c = _f64(circle, (n_items, 3)) if circle is not None else None
        coef, p_coef = self._out(on_device, (n_items, K, J), np.float64, t.float64)
        stats, p_stats = self._records_out(on_device, (n_items, K), ZERNIKE_STATS_DTYPE)
        with t.cuda.device(self.device):
            _check(self.lib.rox_focus_zernike(n_items, K, rows.data_ptr(), ld, status.data_ptr(), g_arr,
                                              c.ctypes.data if c is not None else None, ws.ctypes.data, J,
                                              z_arr, p_coef, p_stats, self._stream()), 'rox_focus_zernike')
        return coef, stats

    def slot_interfaces(self, flags=0):
        """the interface index of every FULL-packet slot: with ROX_FILTER_PHANTOMS in ``flags``
        the phantom interfaces between object and image have none (raytrace.py:185-188)"""
        N = self.table.n_ifcs
        filt = bool(int(flags) & abi.FILTER_PHANTOMS)
        return [i for i, row in enumerate(self.table.rows)
                if not (filt and row.mode == abi.PHANTOM and 0 < i < N - 1)]

    @_in_flight
    def surface_footprints(self, results, trace_flags, partial=True, ok_only=False, half_width=None, n_bins=0,
                           on_device=False, want_records=True):
        """rox_surface_footprints over the FULL packets of finished launches (``results``: the list
        of DeviceResult trace_pupil_grids(..., OUT_FULL) returns, or a single one, still in HBM;
        ``trace_flags``: the rox_opts.flags they were traced with): per (item, slot) the count,
        bounding box, largest radius squared, centroid, RMS radius, extreme cosines of incidence
        and exit and the rays lost there.  ``partial``: the partial record of a BLOCKED / TIR /
        EVANESCENT ray counts; ``ok_only``: only rays with status OK count.  With ``n_bins`` > 0,
        ``half_width`` ([n_seg]) and numpy.histogram2d maps of the landing points over
        [-half_width[k], half_width[k]]^2.  Returns ``(records, maps)``: a FOOTPRINT_DTYPE array
        [n_items, n_seg] (None without ``want_records``) and uint32 [n_items, n_seg, n_bins,
        n_bins] or None -- NumPy, or with ``on_device`` a torch uint8 tensor [n_items, n_seg, 144]
        of the raw records (``footprint_view`` reads it on the host) and an int32 tensor of the
        map's bit patterns."""
        t = self.torch
        results, n_items, n_seg, R, outs = self._packets(results, trace_flags, 'surface_footprints')
        n_bins = int(n_bins)
        if not want_records and n_bins <= 0:
            raise EngineError('surface_footprints: records or maps (or both)')
        hw = None
        if n_bins > 0:
            if n_bins > abi.MAX_FOOTPRINT_BINS:
                raise EngineError(f'surface_footprints: n_bins {n_bins} outside [1, {abi.MAX_FOOTPRINT_BINS}]')
            if half_width is None:
                raise EngineError('surface_footprints: maps need half_width')
            hw = _f64(half_width, (n_seg,))
            if not (np.isfinite(hw).all() and (hw > 0).all()):
                raise EngineError('surface_footprints: half_width must be finite and > 0')
        flags = (abi.FP_PARTIAL if partial else 0) | (abi.FP_OK_ONLY if ok_only else 0)
        none = (None, None)
        rec, p_rec = self._records_out(on_device, (n_items, n_seg), FOOTPRINT_DTYPE) if want_records else none
        maps, p_maps = self._out(on_device, (n_items, n_seg, n_bins, n_bins), np.uint32, t.int32) \
            if n_bins > 0 else none
        with t.cuda.device(self.device):
            _check(self.lib.rox_surface_footprints(self._handle, int(trace_flags), flags, n_items, outs, R,
                                                   p_rec, hw.ctypes.data if hw is not None else None, n_bins,
                                                   p_maps, self._stream()), 'rox_surface_footprints')
        return rec, maps

    def _transmission(self, what, entry, field_rows, results, trace_flags, wvl_idxs, coat_kind, coat_value,
                      want_rows, fields, on_device, tables=None):
        """the body of surface_transmission and surface_thinfilm: ``entry`` is the C entry
        rox_<what>, ``field_rows`` its n_rows with ``fields``.  ``tables(n_items, N, ck)`` checks
        what the entry takes besides and returns those arrays (None for a null pointer) as two
        tuples: the arguments that follow wvl_idx, and those that follow coat_value."""
        t = self.torch
        results, n_items, n_seg, R, outs = self._packets(results, trace_flags, what)
        wi = np.ascontiguousarray(np.asarray(wvl_idxs, dtype=np.int32).reshape(-1))
        if wi.shape[0] != n_items:
            raise EngineError(f'{what}: {wi.shape[0]} wvl_idxs for {n_items} items')
        N = self.table.n_ifcs
        if (coat_kind is None) != (coat_value is None):
            raise EngineError(f'{what}: coat_kind and coat_value go together')
        ck = cv = None
        if coat_kind is not None:
            ck = np.ascontiguousarray(np.asarray(coat_kind, dtype=np.int32).reshape(-1))
            cv = np.ascontiguousarray(np.asarray(coat_value, dtype=np.float64))
            if ck.shape[0] != N or cv.shape != (N, 2):
                raise EngineError(f'{what}: coat_kind [{ck.shape[0]}] and coat_value '
                                  f'{list(cv.shape)} are not [{N}] and [{N}, 2], one entry per interface')
        after_wvl, after_coat = tables(n_items, N, ck) if tables else ((), ())
        n_rows = field_rows if fields else 4
        rows, p_rows = self._out(on_device, (n_items, n_rows, R), np.float64, t.float64) if want_rows \
            else (None, None)
        surf, p_surf = self._records_out(on_device, (n_items, n_seg), TX_SURFACE_DTYPE)
        item, p_item = self._records_out(on_device, (n_items,), TX_ITEM_DTYPE)
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None     # noqa: E731
        with t.cuda.device(self.device):
            _check(entry(self._handle, int(trace_flags), abi.TX_FIELDS if fields else 0, n_items, outs, R,
                         wi.ctypes.data, *map(ptr, after_wvl), N if ck is not None else 0, ptr(ck), ptr(cv),
                         *map(ptr, after_coat), p_rows, R, p_surf, p_item, self._stream()), 'rox_' + what)
        return rows, surf, item

    @_in_flight
    def surface_transmission(self, results, trace_flags, wvl_idxs, coat_kind=None, coat_value=None, want_rows=True,
                             fields=False, on_device=False):
        """rox_surface_transmission over the FULL packets of finished launches (``results``,
        ``trace_flags`` as surface_footprints; ``wvl_idxs``: the wavelength index each item was
        traced at): Fresnel transmission and polarization ray tracing of every OK ray.
        ``coat_kind`` ([n_ifcs] of abi.COAT_*) and ``coat_value`` ([n_ifcs, 2] = (Ts, Tp), read
        where the kind is COAT_FIXED) go together; without them every interface is bare.
        Returns ``(rows, surf, item)``: float64 [n_items, n_rows, R] with rows T, T1, T2, D (and
        with ``fields`` the two exit field vectors, n_rows = 10), NaN where a ray failed (None
        without ``want_rows``); a TX_SURFACE_DTYPE array [n_items, n_seg]; a TX_ITEM_DTYPE array
        [n_items] -- NumPy, or with ``on_device`` torch tensors (the records as uint8 [..., 64]
        and [n_items, 72]; ``tx_view`` reads them on the host)."""
        return self._transmission('surface_transmission', self.lib.rox_surface_transmission, 10, results,
                                  trace_flags, wvl_idxs, coat_kind, coat_value, want_rows, fields, on_device)

    @_in_flight
    def surface_thinfilm(self, results, trace_flags, wvl_idxs, wvls_nm=None, coat_kind=None, coat_value=None,
                         stack_first=None, layer_thickness=None, layer_index=None, sub_index=None, want_rows=True,
                         fields=False, on_device=False):
        """rox_surface_thinfilm: surface_transmission with complex field vectors and, where
        ``coat_kind`` is abi.COAT_STACK, a thin-film stack evaluated per ray.  ``wvls_nm``: each
        item's vacuum wavelength; ``stack_first`` ([n_ifcs + 1] CSR offsets), ``layer_thickness``
        ([L], the unit of ``wvls_nm``), ``layer_index`` ([n_wvls, L, 2] = (re, im) per row of the
        index table) and ``sub_index`` ([n_wvls, n_ifcs, 2], the metal behind a mirror's stack) as
        coatings.stack_tables builds them.  Returns ``(rows, surf, item)`` as surface_transmission
        does; with ``fields`` n_rows = 16: re(E1), re(E2), im(E1), im(E2)."""
        what = 'surface_thinfilm'

        def tables(n_items, N, ck):
            W = len(self.table.wvls)
            wv = sf = lt = li = sb = None
            if wvls_nm is not None:
                wv = np.ascontiguousarray(np.asarray(wvls_nm, dtype=np.float64).reshape(-1))
                if wv.shape[0] != n_items:
                    raise EngineError(f'{what}: {wv.shape[0]} wvls_nm for {n_items} items')
            if stack_first is not None:
                sf = np.ascontiguousarray(np.asarray(stack_first, dtype=np.int32).reshape(-1))
                if ck is None or sf.shape[0] != N + 1:
                    raise EngineError(f'{what}: stack_first [{sf.shape[0]}] is not [{N + 1}] beside coat_kind')
                L = int(sf[-1])
                lt = np.ascontiguousarray(np.asarray(layer_thickness if layer_thickness is not None else [],
                                                     dtype=np.float64).reshape(-1))
                li = np.ascontiguousarray(np.asarray(layer_index if layer_index is not None
                                                     else np.zeros((W, 0, 2)), dtype=np.float64))
                if lt.shape[0] != L or li.shape != (W, L, 2):
                    raise EngineError(f'{what}: layer_thickness [{lt.shape[0]}] and layer_index {list(li.shape)} '
                                      f'are not [{L}] and [{W}, {L}, 2], the layers of stack_first and the '
                                      f'wavelengths of the table')
                if L > 0 and wv is None:
                    raise EngineError(f'{what}: layers need wvls_nm')
            elif layer_thickness is not None or layer_index is not None:
                raise EngineError(f'{what}: layer_thickness and layer_index go with stack_first')
            if sub_index is not None:
                sb = np.ascontiguousarray(np.asarray(sub_index, dtype=np.float64))
                if sb.shape != (W, N, 2):
                    raise EngineError(f'{what}: sub_index {list(sb.shape)} is not [{W}, {N}, 2]')
            return (wv,), (sf, lt, li, sb)

        return self._transmission(what, self.lib.rox_surface_thinfilm, 16, results, trace_flags, wvl_idxs, coat_kind,
                                  coat_value, want_rows, fields, on_device, tables)

    @_in_flight
    def projected_solid_angle(self, results, num, weight=None, weight_row=0, want_cells=False, on_device=False):
        """rox_projected_solid_angle over the finished ``num`` x ``num`` product grids of a
        trace_pupil_grids call (``results``: its list of DeviceResult, OUT_LAST or OUT_FULL, or a
        single one, still in HBM): the signed area each grid covers in the direction cosines
        (L, M) its rays reach the image with, over the rays with status OK.  ``weight``: a
        contiguous float64 device tensor [n_items, n_rows, R], row ``weight_row`` of which weighs
        the rays -- what surface_transmission(..., on_device=True) returns as ``rows``, row 0 its
        T.  Returns ``(items, cells)``: a SA_ITEM_DTYPE array [n_items] and, with ``want_cells``,
        float64 [n_items, num - 1, num - 1] of the cells' signed areas (else None) -- NumPy, or
        with ``on_device`` torch tensors (the records as uint8 [n_items, 144]; ``records_view``
        reads them on the host)."""
        t = self.torch
        what = 'projected_solid_angle'
        num = int(num)
        results, n_items, n_seg, R, outs = self._packets(results, None, what, (abi.OUT_LAST, abi.OUT_FULL), num)
        dir_row = (n_seg - 1) * abi.SEG_DOUBLES + 3
        p_w, stride = self._weight_rows(what, weight, weight_row, n_items, R)
        item, p_item = self._records_out(on_device, (n_items,), SA_ITEM_DTYPE)
        cells, p_cells = self._out(on_device, (n_items, num - 1, num - 1), np.float64, t.float64) \
            if want_cells else (None, None)
        with t.cuda.device(self.device):
            _check(self.lib.rox_projected_solid_angle(n_items, num, outs, dir_row, p_w, stride, p_item, p_cells,
                                                      self._stream()), 'rox_projected_solid_angle')
        return item, cells

    @_in_flight
    def segment_foci(self, results, trace_flags, weight=None, weight_row=0, window=None, on_device=False):
        """rox_segment_foci over the FULL packets of finished launches (``results``, ``trace_flags``
        as surface_footprints): per (item, slot) the weighted moments of the straight lines the OK
        rays leave the slot's interface on, from which ``seg_focus_derive`` finds where the bundle
        is smallest.  ``weight``: a contiguous float64 device tensor [n_items, n_rows, R], row
        ``weight_row`` of which weighs the rays -- what surface_thinfilm(..., on_device=True)
        returns as ``rows``, row 0 its T; None: every weight is 1.  ``window``: (hx, hy), both
        > 0: ``w_in`` and ``n_in`` count the rays that meet the plane z = 0 of the slot's frame
        within it.  Returns a SEG_FOCUS_DTYPE array [n_items, n_seg] -- NumPy, or with
        ``on_device`` a torch uint8 tensor [n_items, n_seg, 136] of the raw records
        (``records_view`` reads it on the host)."""
        t = self.torch
        what = 'segment_foci'
        results, n_items, n_seg, R, outs = self._packets(results, trace_flags, what)
        p_w, stride = self._weight_rows(what, weight, weight_row, n_items, R)
        win = None
        if window is not None:
            win = _f64(window, (2,))
            if not (win > 0).all():
                raise EngineError(f'{what}: window (hx, hy) must be > 0')
        rec, p_rec = self._records_out(on_device, (n_items, n_seg), SEG_FOCUS_DTYPE)
        with t.cuda.device(self.device):
            _check(self.lib.rox_segment_foci(self._handle, int(trace_flags), n_items, outs, R, p_w, stride,
                                             win.ctypes.data if win is not None else None, p_rec,
                                             self._stream()), 'rox_segment_foci')
        return rec

    @_in_flight
    def weighted_maps(self, results, trace_flags, slot=-1, weight=None, weight_row=0, item_factor=None,
                      item_map=None, n_maps=None, window=None, bins=64, want_counts=False, on_device=False,
                      raw=False):
        """rox_weighted_maps over the FULL packets of finished launches (``results``, ``trace_flags``
        as surface_footprints): numpy.histogram2d(weights=) of where the OK rays reach ``slot``
        (-1: the image), summed exactly in 64-bit fixed point -- the maps do not depend on the
        order of anything.  ``weight`` / ``weight_row`` as segment_foci; ``item_factor`` [n_items]
        multiplies an item's weights (finite, >= 0); ``item_map`` [n_items] names the map each item
        adds into (``n_maps`` of them; None: one map per item).  ``window``: (cx, cy, hx, hy),
        one for all maps or [n_maps, 4]; ``bins``: an int or (nbx, nby).  Returns ``(maps,
        counts, scale_exp, items)``: float64 [n_maps, nbx, nby] = ldexp(the integer sums,
        -scale_exp) (with ``raw`` the int64 sums themselves), uint32 counts of the same shape
        (None without ``want_counts``), int32 [n_maps] and a WMAP_ITEM_DTYPE array [n_items] --
        NumPy, or with ``on_device`` torch tensors (the conversion then runs on the device; the
        counts as int32 bits, the records as uint8 [n_items, 40]: ``records_view``)."""
        t = self.torch
        what = 'weighted_maps'
        results, n_items, n_seg, R, outs = self._packets(results, trace_flags, what)
        p_w, stride = self._weight_rows(what, weight, weight_row, n_items, R)
        if not -1 <= int(slot) < n_seg:
            raise EngineError(f'{what}: slot {slot} outside [-1, {n_seg})')
        fac = imap = None
        if item_factor is not None:
            fac = _f64(item_factor, (n_items,))
            if not (np.isfinite(fac) & (fac >= 0)).all():
                raise EngineError(f'{what}: item_factor must be finite and >= 0')
        if item_map is not None:
            imap = np.ascontiguousarray(np.asarray(item_map, dtype=np.int32).reshape(-1))
            n_maps = int(imap.max()) + 1 if n_maps is None and imap.size else n_maps
            if imap.shape[0] != n_items or n_maps is None or not (0 <= imap).all() or not (imap < n_maps).all():
                raise EngineError(f'{what}: item_map is [{n_items}] with values in [0, n_maps)')
        elif n_maps not in (None, n_items):
            raise EngineError(f'{what}: n_maps {n_maps} without item_map is not the {n_items} items')
        n_maps = n_items if n_maps is None else int(n_maps)
        if not 1 <= n_maps <= abi.MAX_FOCUS_ITEMS:
            raise EngineError(f'{what}: 1 to {abi.MAX_FOCUS_ITEMS} maps, got {n_maps}')
        if window is None:
            raise EngineError(f'{what}: needs window = (cx, cy, hx, hy)')
        win = _f64(window, (n_maps, 4))
        if not (np.isfinite(win).all() and (win[:, 2:] > 0).all()):
            raise EngineError(f'{what}: window (cx, cy, hx, hy) must be finite with hx, hy > 0')
        nbx, nby = (int(bins), int(bins)) if np.ndim(bins) == 0 else (int(bins[0]), int(bins[1]))
        if not (1 <= nbx <= abi.MAX_WMAP_BINS and 1 <= nby <= abi.MAX_WMAP_BINS):
            raise EngineError(f'{what}: bins ({nbx}, {nby}) outside [1, {abi.MAX_WMAP_BINS}]')
        wm, p_wm = self._out(on_device, (n_maps, nbx, nby), np.int64, t.int64)
        cnt, p_cnt = self._out(on_device, (n_maps, nbx, nby), np.uint32, t.int32) if want_counts else (None, None)
        exp, p_exp = self._out(on_device, (n_maps,), np.int32, t.int32)
        item, p_item = self._records_out(on_device, (n_items,), WMAP_ITEM_DTYPE)
        with t.cuda.device(self.device):
            _check(self.lib.rox_weighted_maps(self._handle, int(trace_flags), n_items, outs, R, int(slot), p_w, stride,
                                              fac.ctypes.data if fac is not None else None,
                                              imap.ctypes.data if imap is not None else None, n_maps,
                                              win.ctypes.data, nbx, nby, p_wm, p_cnt, p_exp, p_item,
                                              self._stream()), 'rox_weighted_maps')
        if raw:
            return wm, cnt, exp, item
        if on_device:
            # 2^-scale_exp from its bits (scale_exp in [-1000, 1000]: a normal number); the product is
            # ldexp's correctly rounded result
            two = ((1023 - exp.to(t.int64)) << 52).view(t.float64)
            return wm.to(t.float64) * two[:, None, None], cnt, exp, item
        return np.ldexp(wm.astype(np.float64), -exp[:, None, None]), cnt, exp, item

    def _picture(self, what, name, x, tail):
        """a float64 picture or stack of an image-simulation entry, ``tail`` trailing axes behind
        an optional channel axis -> (the array the call reads, kept by the caller; its pointer; its
        shape with the channel axis; whether it came without one).  A torch tensor must be
        contiguous float64 on this engine's device; anything else goes through NumPy."""
        t = self.torch
        if isinstance(x, t.Tensor):
            if x.dtype != t.float64 or not x.is_contiguous() or not x.is_cuda or x.device != self.device:
                raise EngineError(f'{what}: {name} as a tensor is contiguous float64 on {self.device}')
            ptr = x.data_ptr()
        else:
            x = np.ascontiguousarray(x, dtype=np.float64)
            ptr = x.ctypes.data
        if x.ndim not in (tail, tail + 1):
            raise EngineError(f'{what}: {name} has {tail} or {tail + 1} axes, not {x.ndim}')
        bare = x.ndim == tail
        shape = ((1,) if bare else ()) + tuple(int(n) for n in x.shape)
        return x, ptr, shape, bare

    def _node_axes(self, what, node_y, node_x):
        ny = np.ascontiguousarray(np.asarray(node_y, dtype=np.float64).reshape(-1))
        nx = np.ascontiguousarray(np.asarray(node_x, dtype=np.float64).reshape(-1))
        if not (1 <= ny.shape[0] and 1 <= nx.shape[0] and ny.shape[0] * nx.shape[0] <= abi.MAX_FOCUS_ITEMS):
            raise EngineError(f'{what}: 1 to {abi.MAX_FOCUS_ITEMS} nodes, got {ny.shape[0]} x {nx.shape[0]}')
        return ny, nx

    @_in_flight
    def varying_blur(self, scene, psf, node_y, node_x, edge='zero', on_device=False):
        """rox_varying_blur: ``scene`` [H, W] or [C, H, W] convolved with the PSFs ``psf``
        [GY, GX, S, S] or [C, GY, GX, S, S] given at the nodes ``node_y`` [GY] x ``node_x`` [GX]
        (pixel coordinates, strictly increasing) and blended between them by hat functions, every
        source pixel spreading with its own local PSF; tap [a][b] is the light displaced by
        a - (S - 1)/2 rows and b - (S - 1)/2 columns.  ``edge``: 'zero' (light from outside the
        picture is none) or 'replicate'.  Pictures and stacks are contiguous float64 torch tensors
        on this engine's device, or anything NumPy converts.  Returns the picture in the scene's
        shape -- NumPy, or with ``on_device`` a torch tensor.  include/roxtrace.h states the
        arithmetic; tests/imgsim_ref.py restates it."""
        t = self.torch
        what = 'varying_blur'
        scene, p_scene, (C, H, W), bare = self._picture(what, 'scene', scene, 2)
        psf, p_psf, pshape, _b = self._picture(what, 'psf', psf, 4)
        ny, nx = self._node_axes(what, node_y, node_x)
        S = pshape[-1]
        if pshape != (C, ny.shape[0], nx.shape[0], S, S):
            raise EngineError(f'{what}: psf {pshape} is not [{C}, {ny.shape[0]}, {nx.shape[0]}, S, S]')
        if edge not in ('zero', 'replicate'):
            raise EngineError(f"{what}: edge is 'zero' or 'replicate', not {edge!r}")
        flags = abi.BLUR_EDGE_REPLICATE if edge == 'replicate' else abi.BLUR_EDGE_ZERO
        out, p_out = self._out(on_device, (C, H, W), np.float64, t.float64)
        with t.cuda.device(self.device):
            _check(self.lib.rox_varying_blur(C, H, W, p_scene, S, ny.shape[0], nx.shape[0], p_psf, ny.ctypes.data,
                                             nx.ctypes.data, p_out, flags, self._stream()), 'rox_varying_blur')
        return out[0] if bare else out

    @_in_flight
    def image_warp(self, image, node_y, node_x, disp, on_device=False):
        """rox_image_warp: ``image`` [H, W] or [C, H, W] resampled bilinearly at (i + dy, j + dx),
        (dy, dx) the displacements ``disp`` [GY, GX, 2] (pixels, host) at the nodes blended
        bilinearly between them; a tap outside the picture reads 0.  Arrays and the return as
        varying_blur."""
        t = self.torch
        what = 'image_warp'
        image, p_in, (C, H, W), bare = self._picture(what, 'image', image, 2)
        ny, nx = self._node_axes(what, node_y, node_x)
        d = _f64(disp, (ny.shape[0], nx.shape[0], 2))
        out, p_out = self._out(on_device, (C, H, W), np.float64, t.float64)
        with t.cuda.device(self.device):
            _check(self.lib.rox_image_warp(C, H, W, p_in, ny.shape[0], nx.shape[0], ny.ctypes.data, nx.ctypes.data,
                                           d.ctypes.data, p_out, self._stream()), 'rox_image_warp')
        return out[0] if bare else out

    @_in_flight
    def huygens_psf(self, rows, status, planes, nx, ny, pitch_x, pitch_y, n_rays=None, amp=None, want_psf=True,
                    want_field=False, stats_on_device=False):
        """rox_huygens_psf: the complex sum of the OK rays' plane wavelets at the pixels of a product
        grid, squared.  ``rows`` [n_items, 4, ld] = (phi, xi, eta, zeta) -- cycles, and cycles per
        system unit -- ``status`` [n_items, ld] and the optional amplitudes ``amp`` [n_items, ld]
        are contiguous tensors on this engine's device (float64, uint8, float64); ``planes``
        [n_items, K, 3] = (x0, y0, dz) on the host: pixel (a, b) of a plane is the image point
        (x0 + a pitch_x, y0 + b pitch_y), displaced dz along z.  Only the first ``n_rays`` (default
        ld) rays count.  Returns ``(psf, field, stats)``: float64 tensors in HBM [n_items, K, nx, ny]
        and [n_items, K, nx, ny, 2] (None unless wanted) and a HUYGENS_STATS_DTYPE array
        [n_items, K] (n, norm, sum, peak, strehl, peak_ix, peak_iy) -- with ``stats_on_device`` its
        bytes as a uint8 tensor (``records_view`` reads it).  include/roxtrace.h states the
        arithmetic; tests/huygens_ref.py restates it."""
        t = self.torch
        what = 'huygens_psf'

        def dev(x, name, dtype, shape):
            if not isinstance(x, t.Tensor) or x.dtype != dtype or not x.is_contiguous() or not x.is_cuda or \
                    x.device != self.device or (shape is not None and tuple(x.shape) != shape):
                raise EngineError(f'{what}: {name} is a contiguous {dtype} tensor on {self.device}'
                                  + (f' of shape {shape}' if shape else ''))
            return x
        rows = dev(rows, 'rows', t.float64, None)
        if rows.dim() != 3 or int(rows.shape[1]) != 4:
            raise EngineError(f'{what}: rows are [n_items, 4, ld], not {tuple(rows.shape)}')
        n_items, ld = int(rows.shape[0]), int(rows.shape[2])
        status = dev(status, 'status', t.uint8, (n_items, ld))
        if amp is not None:
            amp = dev(amp, 'amp', t.float64, (n_items, ld))
        pl = np.ascontiguousarray(planes, dtype=np.float64)
        if pl.ndim != 3 or pl.shape[0] != n_items or pl.shape[2] != 3:
            raise EngineError(f'{what}: planes are [{n_items}, K, 3], not {pl.shape}')
        K = int(pl.shape[1])
        nx, ny = int(nx), int(ny)
        n_rays = ld if n_rays is None else int(n_rays)
        if not (1 <= nx <= abi.MAX_HUYGENS_PIXELS and 1 <= ny <= abi.MAX_HUYGENS_PIXELS):
            raise EngineError(f'{what}: nx, ny in [1, {abi.MAX_HUYGENS_PIXELS}], got {nx}, {ny}')
        psf = t.empty((n_items, K, nx, ny), dtype=t.float64, device=self.device) if want_psf else None
        field = t.empty((n_items, K, nx, ny, 2), dtype=t.float64, device=self.device) if want_field else None
        stats, p_stats = self._records_out(stats_on_device, (n_items, K), HUYGENS_STATS_DTYPE)
        with t.cuda.device(self.device):
            _check(self.lib.rox_huygens_psf(n_items, K, n_rays, rows.data_ptr(), ld,
                                            amp.data_ptr() if amp is not None else None, status.data_ptr(),
                                            pl.ctypes.data, nx, ny, float(pitch_x), float(pitch_y),
                                            psf.data_ptr() if psf is not None else None,
                                            field.data_ptr() if field is not None else None, p_stats,
                                            self._stream()), 'rox_huygens_psf')
        return psf, field, stats

    @_in_flight
    def wave_differentials(self, results, trace_flags, wvl_idxs, slots=None, aux=None, want_cols=False,
                           on_device=False, want_gram=True):
        """rox_wave_differentials over the FULL packets of finished launches (``results``,
        ``trace_flags`` as surface_footprints; ``wvl_idxs`` as surface_transmission): per OK ray
        the first-order change of optical path under the eleven perturbations of every selected
        slot (``slots``: strictly increasing FULL-packet slots, None = all; tolerance.COLUMN_KINDS
        names the eleven), behind the ``aux`` rows -- a contiguous float64 device tensor
        [n_items, n_aux, >= R] of per-ray functions that join the covariance, or None.  Returns
        ``(item, pivot, sums, gram, cols)``: a WD_ITEM_DTYPE array [n_items] (n, n_bad,
        pivot_ray), float64 [n_items, n_cols] twice and [n_items, n_cols, n_cols] (None without
        ``want_gram``) -- NumPy, or with ``on_device`` torch tensors (the records as uint8
        [n_items, 24]: ``records_view``) -- and, with ``want_cols``, the columns left in HBM as a
        float64 tensor [n_items, n_cols, R], NaN where a ray is not counted (else None)."""
        t = self.torch
        what = 'wave_differentials'
        results, n_items, n_seg, R, outs = self._packets(results, trace_flags, what)
        wi = np.ascontiguousarray(np.asarray(wvl_idxs, dtype=np.int32).reshape(-1))
        if wi.shape[0] != n_items:
            raise EngineError(f'{what}: {wi.shape[0]} wvl_idxs for {n_items} items')
        sel = None
        n_sel = n_seg
        if slots is not None:
            sel = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
            n_sel = int(sel.shape[0])
        n_aux, p_aux, aux_stride, ld_aux = 0, None, 0, 0
        if aux is not None:
            if not hasattr(aux, 'data_ptr') or aux.dim() != 3 or aux.dtype != t.float64 or \
                    not aux.is_contiguous() or not aux.is_cuda or int(aux.shape[0]) != n_items or \
                    int(aux.shape[2]) < R:
                raise EngineError(f'{what}: aux is a contiguous float64 device tensor [{n_items}, n_aux, R >= {R}]')
            n_aux, ld_aux = int(aux.shape[1]), int(aux.shape[2])
            p_aux, aux_stride = (aux.data_ptr() if n_aux else None), n_aux * ld_aux
        n_cols = n_aux + abi.WD_SLOT_COLS * n_sel
        if not 1 <= n_cols <= abi.MAX_WD_COLS:
            raise EngineError(f'{what}: n_cols = n_aux + {abi.WD_SLOT_COLS}*n_sel = {n_cols} outside '
                              f'[1, {abi.MAX_WD_COLS}]')
        cols = t.empty((n_items, n_cols, R), dtype=t.float64, device=self.device) if want_cols else None
        item, p_item = self._records_out(on_device, (n_items,), WD_ITEM_DTYPE)
        pivot, p_pivot = self._out(on_device, (n_items, n_cols), np.float64, t.float64)
        sums, p_sums = self._out(on_device, (n_items, n_cols), np.float64, t.float64)
        gram, p_gram = self._out(on_device, (n_items, n_cols, n_cols), np.float64, t.float64) if want_gram \
            else (None, None)
        with t.cuda.device(self.device):
            _check(self.lib.rox_wave_differentials(self._handle, int(trace_flags), n_items, outs, R, wi.ctypes.data,
                                                   n_sel, sel.ctypes.data if sel is not None else None,
                                                   n_aux, p_aux, aux_stride, ld_aux,
                                                   cols.data_ptr() if cols is not None else None, R,
                                                   p_item, p_pivot, p_sums, p_gram, self._stream()),
                   'rox_wave_differentials')
        return item, pivot, sums, gram, cols

    @_in_flight
    def focus_psf_ee(self, psf, pitch, centers, radii, want_centroid=True):
        """rox_focus_psf_ee over the PSFs focus_psf returns (``psf``: float64 [n_items, K, M, M] in
        HBM): the fraction of each PSF's sum over the pixels whose centre lies within ``radii``
        (broadcast to [n_items, K, Nr], non-decreasing per plane) of ``centers`` (broadcast to
        [n_items, K, 2] in image coordinates about the image point, None = each PSF's own
        centroid); ``pitch`` (broadcast to [n_items, K]) is each plane's pixel pitch, pixel
        (j, l) sitting at (-p (j - M/2), -p (l - M/2)) as in focus_mtf.  Returns
        ``(ee, centroid)``: float64 [n_items, K, Nr] (NaN on planes no ray reached) and
        [n_items, K, 2] (None without ``want_centroid``)."""
        t = self.torch
        n_items, K, M = self._psf_stack(psf, 'focus_psf_ee')
        p = _f64(pitch, (n_items, K))
        r = np.asarray(radii, dtype=np.float64)
        Nr = int(r.shape[-1]) if r.ndim else 1
        r = _f64(r, (n_items, K, Nr))
        c = _f64(centers, (n_items, K, 2)) if centers is not None else None
        ee = np.empty((n_items, K, Nr), dtype=np.float64)
        cen = np.empty((n_items, K, 2), dtype=np.float64) if want_centroid else None
        with t.cuda.device(self.device):
            _check(self.lib.rox_focus_psf_ee(n_items, K, psf.data_ptr(), M, p.ctypes.data,
                                             c.ctypes.data if c is not None else None, Nr, r.ctypes.data,
                                             ee.ctypes.data, cen.ctypes.data if cen is not None else None,
                                             self._stream()), 'rox_focus_psf_ee')
        return ee, cen

    def _spot_stats(self, seg_ptr, ld, status_ptr, n_hits_ptr, n, layout, x_edges, y_edges):
        summ = abi.SpotSummary()
        hist = None
        xe = ye = None
        nxe = nye = 0
        hp = None
        if x_edges is not None:
            xe = np.ascontiguousarray(x_edges, dtype=np.float64)
            ye = np.ascontiguousarray(y_edges, dtype=np.float64)
            nxe, nye = len(xe), len(ye)
            hist = np.empty((nxe - 1, nye - 1), dtype=np.uint32)
            hp = hist.ctypes.data
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_spot_stats(seg_ptr, int(ld), status_ptr, n_hits_ptr, int(n), int(layout),
                                           None if xe is None else xe.ctypes.data, nxe,
                                           None if ye is None else ye.ctypes.data, nye,
                                           C.byref(summ), hp, self._stream()), 'rox_spot_stats')
        n_ok = int(summ.n)
        out = {'n': n_ok, 'sum': (summ.sum[0], summ.sum[1]), 'sum_sq': (summ.sum_sq[0], summ.sum_sq[1]),
               'min': (summ.min[0], summ.min[1]), 'max': (summ.max[0], summ.max[1])}
        if n_ok:
            cx, cy = summ.sum[0] / n_ok, summ.sum[1] / n_ok
            var = (summ.sum_sq[0] + summ.sum_sq[1]) / n_ok - (cx * cx + cy * cy)
            out['centroid'] = (cx, cy)
            out['rms_radius'] = float(np.sqrt(max(var, 0.0)))
        else:
            out['centroid'], out['rms_radius'] = (float('nan'), float('nan')), float('nan')
        return out, hist

    @_in_flight
    def trace_pupil_grid_hits_append(self, fld, grid, wvl_idx, opts, pack):
        """enqueue one ROX_OUT_HITS_COMPACT | ROX_HITS_APPEND launch behind the pairs
        ``pack`` already holds; nothing is synchronised"""
        R = grid_rays(grid)
        if pack.rays + R > pack.cap or pack.n_launches >= pack.cum.numel():
            raise EngineError(f'HitsPack full: {pack.rays} + {R} rays into a capacity of {pack.cap}')
        if not (opts.flags & abi.HITS_APPEND) or opts.out_mode != abi.OUT_HITS_COMPACT:
            raise EngineError('trace_pupil_grid_hits_append needs OUT_HITS_COMPACT | HITS_APPEND')
        o = abi.Out()
        o.seg = pack.seg_ptr
        o.n_hits = pack.count.data_ptr()
        o.ld = pack.cap
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_trace_pupil_grid(self._handle, C.byref(fld), C.byref(grid),
                                                 int(wvl_idx), C.byref(opts), C.byref(o),
                                                 self._stream()), 'rox_trace_pupil_grid')
            k = pack.n_launches
            pack.cum[k:k + 1].copy_(pack.count, non_blocking=True)      # same stream: ordered
        pack.n_launches += 1
        pack.rays += R
        return pack

    @_in_flight
    def trace_pupil_grid_hits_at(self, fld, grid, wvl_idx, opts, seg_ptr, cap, n_hits_ptr):
        """enqueue one ROX_OUT_HITS_COMPACT launch (not appending) whose packed pairs go to
        ``seg_ptr`` (room for ``cap`` pairs, device or device-visible memory) and whose count
        goes to ``n_hits_ptr`` (int64, device-visible); nothing is synchronised.  The unit of
        the pipelined sharded spot diagram (dist.trace_spot_sharded)"""
        if opts.out_mode != abi.OUT_HITS_COMPACT or (opts.flags & abi.HITS_APPEND):
            raise EngineError('trace_pupil_grid_hits_at needs OUT_HITS_COMPACT without HITS_APPEND')
        o = abi.Out()
        o.seg, o.n_hits, o.ld = int(seg_ptr), int(n_hits_ptr), int(cap)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_trace_pupil_grid(self._handle, C.byref(fld), C.byref(grid),
                                                 int(wvl_idx), C.byref(opts), C.byref(o),
                                                 self._stream()), 'rox_trace_pupil_grid')

    def copy_async(self, dst_ptr, src_ptr, nbytes, stream=None):
        """rox_copy_async in the order of ``stream`` (a torch stream; None = the current one)"""
        st = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_copy_async(C.c_void_p(int(dst_ptr)), C.c_void_p(int(src_ptr)),
                                           C.c_size_t(int(nbytes)), st), 'rox_copy_async')

    # -- host memory other processes share (dist.HostSegment) ------------------------
    def pin_host_memory(self, ptr, nbytes):
        """register [ptr, ptr+nbytes) with the HIP runtime; returns the pointer kernels
        on this device write it through"""
        dev = C.c_void_p()
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_pin_host_memory(C.c_void_p(ptr), C.c_size_t(nbytes), C.byref(dev)),
                   'rox_pin_host_memory')
        return dev.value

    def unpin_host_memory(self, ptr):
        _check(self.lib.rox_unpin_host_memory(C.c_void_p(ptr)), 'rox_unpin_host_memory')

    @_in_flight
    def trace_pupil_list_hits(self, fld, px, py, wvl_idx, opts):
        t = self.torch
        px = self._dev(px, t.float64)
        py = self._dev(py, t.float64)
        R = px.shape[0]
        lease, o, _st = self._hits_out(R)
        with t.cuda.device(self.device):
            _check(self.lib.rox_trace_pupil_list(self._handle, C.byref(fld), R, px.data_ptr(),
                                                 py.data_ptr(), int(wvl_idx), C.byref(opts),
                                                 C.byref(o), self._stream()),
                   'rox_trace_pupil_list')
        return self._hits_finish(lease, R)

    @_in_flight
    def trace_rays_hits(self, pt0, dir0, wvl_idx, opts):
        t = self.torch
        pt0 = self._dev(pt0, t.float64)
        dir0 = self._dev(dir0, t.float64)
        R = pt0.shape[1]
        if np.ndim(wvl_idx) == 0 and not isinstance(wvl_idx, t.Tensor):
            wi, wi_ptr, wi_all = None, None, int(wvl_idx)
        else:
            wi = self._dev(wvl_idx, t.int32)
            wi_ptr, wi_all = wi.data_ptr(), 0
        lease, o, _st = self._hits_out(R)
        with t.cuda.device(self.device):
            _check(self.lib.rox_trace_rays(self._handle, R, pt0.data_ptr(), dir0.data_ptr(),
                                           wi_ptr, wi_all, C.byref(opts), C.byref(o),
                                           self._stream()), 'rox_trace_rays')
        return self._hits_finish(lease, R)

    # -- one ray (raytrace.trace) -----------------------------------------------
    @_in_flight
    def trace_one(self, pt0, dir0, wvl_idx, opts):
        """one explicit ray, FULL packets, through the library's ROX_HOST_POINTERS
        path: the ray and its packet live in one NumPy block; the library copies
        the 48 input bytes into a device-mapped pinned block, the kernel reads and
        writes that block directly, and the packet is copied back (one launch, one
        synchronise, no copy-engine transfer).  Slots past a failure are NaN."""
        key = opts.flags & abi.FILTER_PHANTOMS
        nseg = self._nseg.get(key)
        if nseg is None:
            nseg = self._nseg[key] = self.num_segments(opts.flags)
        buf = np.empty(8 + abi.SEG_DOUBLES * nseg)
        buf[0:3] = pt0
        buf[3:6] = dir0
        base = buf.ctypes.data
        o = abi.Out()
        o.seg, o.op, o.status, o.fail_surf, o.ld = base + 64, base + 48, base + 56, base + 58, 1
        saved = opts.flags
        opts.flags = saved | abi.HOST_POINTERS
        try:
            if self.torch.cuda.current_device() == self.device.index:
                rc = self.lib.rox_trace_rays(self._handle, 1, base, base + 24, None, int(wvl_idx),
                                             C.byref(opts), C.byref(o), None)
            else:
                with self.torch.cuda.device(self.device):
                    rc = self.lib.rox_trace_rays(self._handle, 1, base, base + 24, None,
                                                 int(wvl_idx), C.byref(opts), C.byref(o), None)
        finally:
            opts.flags = saved
        _check(rc, 'rox_trace_rays')

        class _H:
            pass
        h = _H()
        h.R, h.out_mode, h.pupil = 1, abi.OUT_FULL, None
        h.seg = buf[8:].reshape(nseg, abi.SEG_DOUBLES, 1)
        h.op = buf[6:7]
        h.status = buf[7:8].view(np.uint8)[0:1]
        h.fail_surf = buf[7:8].view(np.int16)[1:2]
        return h

    # -- chief-ray aiming ---------------------------------------------------------
    @_in_flight
    def aim_chief_rays(self, probs, eps=1.0e-12):
        """probs: sequence of abi.Aim -> (aim float64[n, 2] = (x1, y1), result int32[n])"""
        n = len(probs)
        arr = (abi.Aim * n)(*probs)
        aim = np.zeros((n, 2))
        result = np.zeros(n, dtype=np.int32)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_aim_chief_rays(self._handle, n, arr, float(eps),
                                               aim.ctypes.data, result.ctypes.data,
                                               self._stream()), 'rox_aim_chief_rays')
        return aim, result

    @_in_flight
    def iterate_pupil_rays(self, probs, eps=1.0e-12):
        """probs: sequence of abi.PupilIter -> start_r float64[n] (vigcalc.iterate_pupil_ray)"""
        n = len(probs)
        arr = (abi.PupilIter * n)(*probs)
        out = np.zeros(n)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_iterate_pupil_rays(self._handle, n, arr, float(eps), out.ctypes.data,
                                                   self._stream()), 'rox_iterate_pupil_rays')
        return out

    @_in_flight
    def iterate_ray_raw(self, probs, eps=1.0e-12):
        """trace.iterate_ray_raw over the path this engine's table describes: (aim [n, 2],
        result [n], last_xy [n, 2] = pupil-plane coordinates of the last trial ray the
        iteration evaluated, last_status [n] = its trace status)"""
        n = len(probs)
        arr = (abi.Aim * n)(*probs)
        aim = np.zeros((n, 2))
        result = np.zeros(n, dtype=np.int32)
        last_xy = np.zeros((n, 2))
        last_st = np.zeros(n, dtype=np.int32)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_iterate_ray_raw(self._handle, n, arr, float(eps), aim.ctypes.data,
                                                result.ctypes.data, last_xy.ctypes.data,
                                                last_st.ctypes.data, self._stream()),
                   'rox_iterate_ray_raw')
        return aim, result, last_xy, last_st

    @_in_flight
    def find_real_enp(self, probs, eps=1.0e-12):
        """probs: sequence of abi.Enp -> (z float64[n, 2] = (z_enp, z of the last trial ray),
        result int32[n] = abi.ENP_*)"""
        n = len(probs)
        arr = (abi.Enp * n)(*probs)
        z = np.zeros((n, 2))
        result = np.zeros(n, dtype=np.int32)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_find_real_enp(self._handle, n, arr, float(eps),
                                              z.ctypes.data, result.ctypes.data,
                                              self._stream()), 'rox_find_real_enp')
        return z, result

    @_in_flight
    def calc_vignetting(self, probs, eps=1.0e-12):
        """probs: sequence of abi.Vig -> (vig float64[n], clip_surf int32[n])"""
        n = len(probs)
        arr = (abi.Vig * n)(*probs)
        vig = np.zeros(n)
        clip = np.zeros(n, dtype=np.int32)
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_calc_vignetting(self._handle, n, arr, float(eps),
                                                vig.ctypes.data, clip.ctypes.data,
                                                self._stream()), 'rox_calc_vignetting')
        return vig, clip

    def time_pupil_grid_sustained(self, fld, grid, wvl_idx, opts, out, launches=20, batches=7,
                                  warm_ms=120.0):
        """median over `batches` of :meth:`time_pupil_grid` after `warm_ms` of
        back-to-back launches: the GPU's clocks take tens of milliseconds of
        continuous work to settle (a cold 20-launch batch reads 10-30 % slow,
        tools/sustained_probe.py), so steady-state kernel times are quoted"""
        import time as _time
        t0 = _time.perf_counter()
        while (_time.perf_counter() - t0) * 1e3 < warm_ms:
            self.time_pupil_grid(fld, grid, wvl_idx, opts, out, launches)
        ts = sorted(self.time_pupil_grid(fld, grid, wvl_idx, opts, out, launches)
                    for _ in range(batches))
        return ts[len(ts) // 2]

    @_in_flight
    def time_pupil_grid(self, fld, grid, wvl_idx, opts, out, launches):
        """mean duration (ms) of the trace kernel over `launches` launches,
        from HIP events recorded on the launch stream"""
        ms = C.c_double()
        o = out.out_struct()
        with self.torch.cuda.device(self.device):
            _check(self.lib.rox_time_pupil_grid(self._handle, C.byref(fld), C.byref(grid),
                                                int(wvl_idx), C.byref(opts), C.byref(o),
                                                self._stream(), int(launches), C.byref(ms)),
                   'rox_time_pupil_grid')
        return ms.value
