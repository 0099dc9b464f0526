"""SPH kernels, the ``kernel_func`` plugin point of ``create_image``.

Mirrors ``quartic_spline_kernel`` (/root/reference/src/astro_sph_tools/tools/projections/
_kernels.pyx:9-20): ``W(r, h)`` over two 1-D float64 arrays, returning a new float64
array, evaluated ON THE GPU (asp_kernel_eval).  Despite its name the reference kernel is
the M4 cubic spline with support 2h and 3-D normalisation 1/(pi h^3); that is kept.
The two ``*_column_kernel`` objects are those kernels integrated along the line of sight
(2-D normalisation 1/h^2): maps made with them are column densities and conserve sum A.

The kernel objects also carry the C-ABI kernel id, which is how ``create_image``
recognises them and runs the whole projection natively.  Any other callable (the
reference's own compiled kernel included) goes through the plugin path: neighbour pairs
from the device, the callable evaluated on the host (_plugin.py).
"""
from __future__ import annotations

import numpy as np

from ... import _lib


class SPHKernel:
    """A device-evaluable SPH kernel: callable like the reference's kernel_func."""

    def __init__(self, name: str, kernel_id: int, doc: str):
        self.__name__ = name
        self.kernel_id = kernel_id
        self.__doc__ = doc

    def __repr__(self):
        return f"<asp_amd SPH kernel {self.__name__} (id {self.kernel_id})>"

    def __call__(self, r, h, *, device: int = 0):
        r = np.asarray(r)
        h = np.asarray(h)
        # The reference's typed memoryview signature (double[:] r, double[:] h) raises
        # ValueError for any other buffer dtype or dimensionality.
        for a in (r, h):
            if a.dtype != np.float64:
                raise ValueError(f"Buffer dtype mismatch, expected 'double' but got '{a.dtype}'")
            if a.ndim != 1:
                raise ValueError(f"Buffer has wrong number of dimensions (expected 1, got {a.ndim})")
        if h.shape[0] < r.shape[0]:
            raise ValueError("h is shorter than r")
        r = np.ascontiguousarray(r)
        h = np.ascontiguousarray(h[: r.shape[0]])
        w = np.zeros(r.shape[0], dtype=np.float64)
        if r.shape[0] == 0:
            return w
        _lib.require_gpu(device)
        _lib.check(_lib.lib().asp_kernel_eval(self.kernel_id, _lib.ptr(r, _lib._d),
                                              _lib.ptr(h, _lib._d), _lib.ptr(w, _lib._d),
                                              r.shape[0], 0, device, None))
        return w


quartic_spline_kernel = SPHKernel(
    "quartic_spline_kernel", _lib.ASP_KERNEL_CUBIC_SPLINE,
    "M4 cubic spline, support 2h: W = (1 - 1.5q^2 + 0.75q^3)/(pi h^3) for q < 1, "
    "0.25 (2-q)^3/(pi h^3) for 1 <= q < 2, else 0 (q = r/h).  _kernels.pyx:9-20.")

cubic_spline_kernel = quartic_spline_kernel

wendland_c2_kernel = SPHKernel(
    "wendland_c2_kernel", _lib.ASP_KERNEL_WENDLAND_C2,
    "Wendland C2, support 2h, 3-D normalisation: W = 21/(16 pi h^3) (1-q/2)^4 (1+2q), "
    "q = r/h < 2.  Build-defined (SURVEY.md §8(a)).")

indicator_kernel = SPHKernel(
    "indicator_kernel", _lib.ASP_KERNEL_INDICATOR,
    "W = 1 for every pair inside 2h: create_image with this kernel and A = 1 counts the "
    "neighbours of every pixel (neighbour-set verification).")

cubic_spline_column_kernel = SPHKernel(
    "cubic_spline_column_kernel", _lib.ASP_KERNEL_CUBIC_SPLINE_COLUMN,
    "M4 cubic spline integrated along the line of sight: W_col(r, h) = F(q) / (pi h^2), "
    "F(q) = 2 int_0^sqrt(4-q^2) w(sqrt(q^2+z^2)) dz with w the cubic spline's shape and "
    "q = r/h the projected distance; 3/(2 pi h^2) at q = 0, 0 for q >= 2, "
    "2 pi int W_col r dr = 1.  A map of A is the column density of A.")

wendland_c2_column_kernel = SPHKernel(
    "wendland_c2_column_kernel", _lib.ASP_KERNEL_WENDLAND_C2_COLUMN,
    "Wendland C2 integrated along the line of sight: W_col(r, h) = 21 F(q) / (16 pi h^2), "
    "F the same integral over (1-r/2)^4 (1+2r); 7/(4 pi h^2) at q = 0, 0 for q >= 2, "
    "2 pi int W_col r dr = 1.")

KERNELS = {k.kernel_id: k for k in (quartic_spline_kernel, wendland_c2_kernel, indicator_kernel,
                                    cubic_spline_column_kernel, wendland_c2_column_kernel)}
COLUMN_KERNEL_IDS = (_lib.ASP_KERNEL_CUBIC_SPLINE_COLUMN, _lib.ASP_KERNEL_WENDLAND_C2_COLUMN)

# The one table of kernel names: each kernel object's __name__, with and without "_kernel",
# and the short spellings of the cubic spline.
KERNEL_IDS = {"cubic": _lib.ASP_KERNEL_CUBIC_SPLINE, "cubic_spline": _lib.ASP_KERNEL_CUBIC_SPLINE,
              "cubic_column": _lib.ASP_KERNEL_CUBIC_SPLINE_COLUMN}
for _k in KERNELS.values():
    KERNEL_IDS[_k.__name__] = KERNEL_IDS[_k.__name__[:-len("_kernel")]] = _k.kernel_id
# the names the device-tensor entry points (asp_amd.device) have always taken
DEVICE_KERNEL_NAMES = ("cubic", "quartic_spline_kernel", "cubic_spline", "wendland_c2", "indicator",
                       "cubic_column", "wendland_c2_column")



def device_kernel_id(kernel) -> int:
    """One of the three lookups over KERNEL_IDS, one per family of entry points, each with the
    failure its callers (and their tests) rely on:

    * ``device_kernel_id`` (asp_amd.device): an int passes through unchecked (the C-ABI
      refuses a bad id), a str outside DEVICE_KERNEL_NAMES is a KeyError, anything else goes
      to ``native_kernel_id``;
    * ``named_kernel_id`` (sightline_columns): an SPHKernel or any name of KERNEL_IDS, else a
      ValueError listing the names;
    * ``kernel_id_of`` / ``native_kernel_id`` (create_image and the other ``kernel_func=``
      mirrors of the reference): an SPHKernel of this package; any other callable is None
      (the plug-in path) / a TypeError; a non-callable is a TypeError.
    """
    if isinstance(kernel, int):
        return kernel
    if isinstance(kernel, str):
        if kernel not in DEVICE_KERNEL_NAMES:
            raise KeyError(kernel)
        return KERNEL_IDS[kernel]
    return native_kernel_id(kernel)


def named_kernel_id(kernel) -> int:
    if isinstance(kernel, SPHKernel):
        return kernel.kernel_id
    if isinstance(kernel, str) and kernel in KERNEL_IDS:
        return KERNEL_IDS[kernel]
    raise ValueError(f"kernel {kernel!r} is not one of {sorted(KERNEL_IDS)} or an SPHKernel")


def kernel_id_of(kernel_func):
    """The C-ABI kernel id of one of this package's kernels, or None for any other
    callable (it then runs through the plugin path, _plugin.project_callable)."""
    kid = getattr(kernel_func, "kernel_id", None)
    if isinstance(kernel_func, SPHKernel) and kid in KERNELS:
        return kid
    if not callable(kernel_func):
        raise TypeError(f"kernel_func {kernel_func!r} is not callable")
    return None


def native_kernel_id(kernel_func) -> int:
    """kernel_id_of for the paths with no plugin (device arrays, cubes, periodic maps)."""
    kid = kernel_id_of(kernel_func)
    if kid is None:
        raise TypeError(f"kernel_func {kernel_func!r} cannot run on the GPU here; use "
                        "quartic_spline_kernel, wendland_c2_kernel, indicator_kernel, "
                        "cubic_spline_column_kernel or wendland_c2_column_kernel "
                        "(create_image accepts any callable)")
    return kid
