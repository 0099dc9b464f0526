"""The one argument, stream and flag path of every Python wrapper of the C-ABI.

Inputs are host arrays (NumPy, unyt, lists) or torch tensors on the GPU; :func:`is_device`
tells them apart.  ``host_f64`` / ``dev_f64`` / ``positions_f64`` return a contiguous float64
array or tensor or raise ``ValueError`` naming the argument, the shape found and the shape
expected.  ``cast=True`` converts any dtype, ``cast=False`` refuses all but float64; each
entry point keeps the strictness it always had:

    ======================================  ===========  ===============
    entry point                             host arrays  device tensors
    ======================================  ===========  ===============
    sightline_columns, nearest_haloes       refuse       refuse
    sightline_spectra                       refuse       refuse
    halo_profiles, aperture_sums            refuse       refuse
    project2d_f64 (create_image)            cast         refuse
    stage_particles, knn_smoothing_lengths  cast         refuse
    the periodic-box helpers                cast         refuse
    project2d_props_f64 (create_images)     cast         cast
    IonisationTable, ion_masses             cast         cast
    project_callable (the plug-in path)     cast         (host only)
    ======================================  ===========  ===============

``stream=`` is a ``torch.cuda.Stream``, a raw ``hipStream_t`` handle or None (torch's current
stream) everywhere: :func:`raw_stream`.  A wrapper that creates device temporaries (uploads,
``.contiguous()`` copies, products) does so inside :class:`stream_scope`, which makes the
call's stream torch's current one and, on exit, tells the caching allocator that the kept
tensors were used there.  The wrappers of device-resident float32 arrays (``project2d``,
``project3d``) create none and only call :func:`raw_stream`.

Kernel ids live in ``tools/projections/_kernels.py``, axis codes in ``_axes.py``.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib


def is_device(a) -> bool:
    """A torch tensor on the GPU (anything else is taken for a host array)."""
    return hasattr(a, "is_cuda") and a.is_cuda


def dptr(a):
    """``_lib.ptr`` of a float64 array or tensor (None: NULL)."""
    return _lib.ptr(a, _lib._d)


def _shape_error(name, found, expected):
    return ValueError(f"{name} must have shape {tuple(expected)}, got {tuple(found)}")


def host_f64(a, name, shape=None, *, cast, flat=False):
    """``a`` as a C-contiguous float64 NumPy array (``flat``: reshaped to 1-D first)."""
    x = np.asarray(a)
    if not cast and x.dtype != np.float64:
        raise ValueError(f"{name} must be float64, got {x.dtype}")
    if flat and x.ndim != 1:
        x = x.reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float64)
    if shape is not None and x.shape != tuple(shape):
        raise _shape_error(name, x.shape, shape)
    return x


def dev_f64(t, name, shape=None, dev=None, *, cast=False, flat=False):
    """``t`` as a contiguous float64 device tensor (on ``dev`` when given)."""
    import torch
    if not is_device(t) or (dev is not None and t.device != dev) or \
            (not cast and t.dtype != torch.float64):
        raise ValueError(f"{name} must be a float64 tensor on {dev or 'the GPU'}")
    if flat and t.dim() != 1:
        t = t.reshape(-1)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _shape_error(name, t.shape, shape)
    return t.to(torch.float64).contiguous()


def upload_f64(a, name, shape=None, dev=None, *, cast=False, flat=False):
    """``(float64 device tensor, was_host)``: a host array is cast and copied to ``dev``
    (default: the current GPU), a device tensor goes through :func:`dev_f64` and stays where
    it is.  Call it inside a :class:`stream_scope` when the call has a stream of its own."""
    if is_device(a):
        return dev_f64(a, name, shape, cast=cast, flat=flat), False
    import torch
    x = host_f64(a, name, shape, cast=True, flat=flat)
    _lib.require_gpu(0 if dev is None else dev.index or 0)
    if not x.flags.writeable:  # torch.from_numpy wants a writeable buffer
        x = x.copy()
    return torch.from_numpy(x).to("cuda" if dev is None else dev), True


def positions_f64(positions, name="positions", *, cast):
    """The (N, 3) float64 check: ``(array or tensor, N, on_device)``.  Device tensors are
    never cast."""
    if is_device(positions):
        import torch
        if positions.dtype != torch.float64 or positions.dim() != 2 or positions.shape[1] != 3:
            raise ValueError(f"{name} must be an (N, 3) float64 tensor")
        return positions.contiguous(), int(positions.shape[0]), True
    pos = np.asarray(positions)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"{name} must have shape (N, 3), got {pos.shape}")
    return host_f64(pos, name, cast=cast), pos.shape[0], False


def raw_stream(stream, dev):
    """The integer ``hipStream_t`` of ``stream``: a ``torch.cuda.Stream``, a raw handle, or
    None for torch's current stream on ``dev``."""
    if stream is None:
        import torch
        return torch.cuda.current_stream(dev).cuda_stream
    return getattr(stream, "cuda_stream", stream)


class stream_scope:
    """``with stream_scope(dev, stream) as s:`` -- torch allocates and computes on the call's
    stream inside the block, ``s.raw`` is the handle for the native call, and every tensor
    given to ``s.keep(...)`` (None skipped) is ``record_stream``-ed on exit, so the caching
    allocator reuses its memory only after the stream's work."""

    def __init__(self, dev, stream):
        import torch
        self.raw = raw_stream(stream, dev)
        self._ext = torch.cuda.ExternalStream(self.raw, device=dev)
        self._ctx = torch.cuda.stream(self._ext)
        self._kept = []

    def keep(self, *tensors):
        self._kept.extend(t for t in tensors if t is not None)

    def __enter__(self):
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self._ctx.__exit__(*exc)
        for t in self._kept:
            t.record_stream(self._ext)


def call_flags(device_ptrs=False, ratio=False, accumulate=False, deterministic=False,
               device_outputs=False) -> int:
    """The ``flags`` argument of the C-ABI (ASP_F_* of include/asp.h)."""
    return ((_lib.ASP_F_DEVICE_PTRS if device_ptrs else 0) | (_lib.ASP_F_RATIO if ratio else 0)
            | (_lib.ASP_F_ACCUMULATE if accumulate else 0)
            | (_lib.ASP_F_DETERMINISTIC if deterministic else 0)
            | (_lib.ASP_F_DEVICE_OUTPUTS if device_outputs else 0))


def sample_sums(entry, lead, positions, smoothing_lengths, particle_properties, weights, points,
                widths, columns, kid, deterministic, device, stream, *, extra=(), bins=(),
                width=None):
    """What ``sightline_columns``, ``sample_points`` and ``sightline_spectra`` share: the
    float64 checks of the particle fields and of ``points`` ((M, w) with w in ``widths``), on
    the host or on
    ``positions``' device, the ``A * w`` product for ``weights``, the float32 output(s) and the
    call of the ``_f64`` entry point ``entry``, whose arguments after N are ``lead``, then the
    point columns ``columns(w)``.  Returns the (M,) sums, or weighted means with ``weights``.

    ``sightline_spectra`` adds ``extra``, further (N,) particle fields as (array, name) that the
    entry point takes before N, ``bins``, its scalars between M and the kernel id, and
    ``width``, the values per point: the result is (M, width)."""
    fields = ((smoothing_lengths, "smoothing_lengths"), (particle_properties, "particle_properties"),
              (weights, "weights"))
    shape = (lambda m: (m,)) if width is None else (lambda m: (m, width))
    shapes = " or ".join(f"(M, {w})" for w in widths)

    def call(on_device, pos, h, a0, a1, more, n, cols, m, out0, out1, dev_index, raw):
        _lib.check(getattr(_lib.lib(), entry)(
            dptr(pos), dptr(h), dptr(a0), dptr(a1), *map(dptr, more), n, *lead, *map(dptr, cols), m,
            *bins, kid,
            call_flags(on_device, weights is not None, deterministic=deterministic),
            _lib.ptr(out0), _lib.ptr(out1), dev_index, raw))

    if is_device(positions):
        import torch
        dev = positions.device
        pts = points
        if (not is_device(pts) or pts.dtype != torch.float64 or pts.device != dev
                or pts.dim() != 2 or pts.shape[1] not in widths):
            raise ValueError(f"points must be an {shapes} float64 tensor on {dev}")
        m = pts.shape[0]
        with stream_scope(dev, stream) as scope:  # the temporaries are ordered on the call's stream
            pos, n, _ = positions_f64(positions, cast=False)
            h, a0, a1 = (None if a is None else dev_f64(a, name, (n,), dev) for a, name in fields)
            more = [dev_f64(a, name, (n,), dev) for a, name in extra]
            cols = [pts[:, c].contiguous() for c in columns(pts.shape[1])]
            if a1 is not None:
                a0 = a0 * a1
            out0 = alloc_out(shape(m), torch.float32, dev)
            out1 = None if a1 is None else alloc_out(shape(m), torch.float32, dev)
            scope.keep(pos, h, a0, a1, *more, *cols, out1)
            call(True, pos, h, a0, a1, more, n, cols, m, out0, out1, dev.index or 0, scope.raw)
        return out0
    pos, n, _ = positions_f64(positions, cast=False)
    h, a0, a1 = (None if a is None else host_f64(a, name, (n,), cast=False) for a, name in fields)
    more = [host_f64(a, name, (n,), cast=False) for a, name in extra]
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] not in widths:
        raise ValueError(f"points must have shape {shapes}, got {pts.shape}")
    pts = host_f64(pts, "points", cast=False)
    cols = [np.ascontiguousarray(pts[:, c]) for c in columns(pts.shape[1])]
    m = pts.shape[0]
    if a1 is not None:
        a0 = a0 * a1
    out0 = alloc_out(shape(m), np.float32, None, zeros=True)
    out1 = None if a1 is None else alloc_out(shape(m), np.float32, None, zeros=True)
    if m == 0:
        return out0
    _lib.require_gpu(device)
    call(False, pos, h, a0, a1, more, n, cols, m, out0, out1, device, None)
    return out0


def alloc_out(shape, dtype, dev, given=None, *, zeros=False, name="outputs"):
    """A fresh output of ``shape`` -- a tensor of torch ``dtype`` on ``dev``, or a NumPy array
    of NumPy ``dtype`` when ``dev`` is None -- or ``given`` after checking that it is one:
    contiguous, of that dtype and element count, on that device."""
    if dev is None:
        if given is None:
            return (np.zeros if zeros else np.empty)(shape, dtype=dtype)
        ok = (isinstance(given, np.ndarray) and given.dtype == dtype
              and given.flags.c_contiguous and given.size == math.prod(shape))
    else:
        if given is None:
            import torch
            return (torch.zeros if zeros else torch.empty)(shape, dtype=dtype, device=dev)
        ok = (is_device(given) and given.dtype == dtype and given.device == dev
              and given.is_contiguous() and given.numel() == math.prod(shape))
    if not ok:
        raise ValueError(f"{name} must be contiguous {dtype} {tuple(shape)} "
                         f"{'arrays' if dev is None else f'tensors on {dev}'}")
    return given
