"""ctypes binding of libasp_hip.so (the C-ABI in include/asp.h).

The product path has no CPU fallback: if the HIP library is missing this module raises
at import-use time, and if no GPU is visible every projection call raises RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)  # astro-sph-tools_amd/
LIB_PATH = os.environ.get("ASP_LIB", os.path.join(ROOT, "lib", "libasp_hip.so"))

ASP_KERNEL_CUBIC_SPLINE = 0
ASP_KERNEL_WENDLAND_C2 = 1
ASP_KERNEL_INDICATOR = 2
ASP_KERNEL_CUBIC_SPLINE_COLUMN = 3
ASP_KERNEL_WENDLAND_C2_COLUMN = 4

ASP_F_DEVICE_PTRS = 0x1
ASP_F_RATIO = 0x2
ASP_F_ACCUMULATE = 0x4
ASP_F_DETERMINISTIC = 0x8
ASP_F_DEVICE_OUTPUTS = 0x10

ASP_PB_WRAP = 0x1
ASP_PB_SHIFT_ORIGIN = 0x2
ASP_PB_SHIFT_CENTRE = 0x4
ASP_PB_ORIGIN_IS_CENTRE = 0x8
ASP_PB_IMAGES = 0x10
ASP_PB_DISPLACEMENT = 0x20

ASP_OK = 0
ASP_ERR_INVALID = -1
ASP_ERR_HIP = -2
ASP_ERR_NOMEM = -3
ASP_ERR_UNSUPPORTED = -4

ASP_MATCH_MAPPING = 0
ASP_MATCH_REORDER = 1

STAGES = ("memset", "count", "colscan", "tilescan", "scatter", "scale", "deposit", "merge",
          "wide", "ratio", "cube_count", "cube_colscan", "cube_tilescan", "cube_scatter",
          "cube_deposit", "cube_merge", "gather", "knn_prep", "knn_search", "nearest_prep",
          "nearest_search")
# asp_sample2d's stages, numbered after STAGES (21, 22)
SAMPLE_STAGES = ("sample_prep", "sample_deposit")
ALL_STAGES = STAGES + SAMPLE_STAGES
# asp_spectra2d's deposit (23; its prep is sample_prep), after ALL_STAGES
SPECTRA_STAGES = ("spectra_deposit",)
PROFILE_STAGES = ALL_STAGES + SPECTRA_STAGES  # every stage profile() / profile_read() know
SPECTRA_T = 5.0  # ASP_SPECTRA_T of include/asp_spectra.h

_lib = None

_f = C.POINTER(C.c_float)
_d = C.POINTER(C.c_double)
_i32 = C.POINTER(C.c_int32)
_i64 = C.POINTER(C.c_int64)
_u8 = C.POINTER(C.c_uint8)

# The C-ABI of include/asp.h, one entry per function: its argument types.  lib() applies them;
# a new entry point adds its line here and nothing else in this module.
_I, _Q, _R, _V = C.c_int32, C.c_int64, C.c_double, C.c_void_p
_GRID2 = [_R] * 4 + [_I] * 3  # x_min, x_max, y_min, y_max, nx, ny, chunk_size
PROTOTYPES = {
    "asp_version": [],
    "asp_last_error": [],
    "asp_device_count": [],
    "asp_project2d": [_f] * 5 + [_Q] + _GRID2 + [_I, _I, _f, _f, _I, _V],
    "asp_project2d_rows": [_f] * 5 + [_Q] + _GRID2 + [_I] * 4 + [_f, _f, _I, _V],
    "asp_project2d_props": [_f, _f, _f, C.POINTER(_f), _I, _Q] + _GRID2
                           + [_I, _I, C.POINTER(_f), _I, _V],
    "asp_project2d_props_f64": [_d, _d, C.POINTER(_d), _I, _Q, _I] + _GRID2
                               + [_I, _I, C.POINTER(_f), _I, _V],
    "asp_project2d_sph": [_f] * 5 + [C.POINTER(_f), _I, _Q] + _GRID2
                         + [_I, _I, C.POINTER(_f), _I, _V],
    "asp_project2d_sph_f64": [_d] * 4 + [C.POINTER(_d), _I, _Q, _I] + _GRID2
                             + [_I, _I, C.POINTER(_f), _I, _V],
    "asp_project2d_f64": [_d] * 4 + [_Q, _I] + _GRID2 + [_I, _I, _f, _f, _I, _V],
    "asp_pairs_begin": [_d, _d, _Q, _I] + _GRID2 + [_I, _I, _V, _i64, C.POINTER(_V)],
    "asp_pairs_emit": [_V, _I, _I, _i64, _i32, _d],
    "asp_pairs_end": [_V],
    "asp_project3d": [_f] * 5 + [_Q] + [_R] * 6 + [_I] * 7 + [_f, _I, _V],
    "asp_kernel_eval": [_I, _d, _d, _d, _Q, _I, _I, _V],
    "asp_chunk_ranges": [_f, _f, _f, _Q] + _GRID2 + [_i32] * 4 + [_I, _I, _V],
    "asp_pixel_neighbours": [_f, _f, _f, _Q] + _GRID2 + [_i64, _Q, _i64, _i32, _Q, _i64, _I],
    "asp_ratio": [_f, _f, _Q, _I, _V],
    "asp_profile": [_I, _I],
    "asp_profile_stages": [_I, C.c_uint32],
    "asp_profile_read": [_I, _d, _i64, _I],
    "asp_last_stats": [_I, _i64, _I],
    "asp_release": [_I],
    "asp_stage_particles": [_d] * 4 + [_Q, _I, _d, _R, _I] + [_f] * 5 + [_Q, _i64, _I, _I, _V],
    "asp_periodic": [_I, _d, _Q, _d, _Q, _Q, _R, _I, _d, _I, _V],
    "asp_wrapped_distance": [_d, _Q, _d, _Q, _Q, _R, _I, _d, _I, _V],
    "asp_knn_smoothing_lengths": [_d, _Q, _I, _d, _I, _I, _V],
    "asp_table_interp3": [_d, _I, _I, _I, _d, _d, _d, _d, _I, _I, _R, _Q, _R, _I, _d, _d, _d,
                          _I, _V],
    "asp_table_interp": [_d, _I, _i32, C.POINTER(_V), _d, _I, _I, _R, _Q, _R, _I, _I, _d, _d,
                         _d, _I, _V],
    "asp_nearest": [_d, _Q, _d, _Q, C.POINTER(C.c_uint32), _I, _R, _i32, _d, _I, _I, _V],
    "asp_match_ids": [_i64, _u8, _Q, _i64, _u8, _Q, _I, _i32, _u8, _i64, _I, _I, _V],
    "asp_take_rows": [_V, _Q, _Q, _i32, _Q, _V, _V, _I, _I, _V],
    "asp_sample2d": [_f] * 5 + [_Q, _d, _d, _Q, _I, _I, _f, _f, _I, _V],
    "asp_sample2d_f64": [_d] * 4 + [_Q, _I, _d, _d, _Q, _I, _I, _f, _f, _I, _V],
}
RESTYPES = {"asp_last_error": C.c_char_p}  # every other function returns int
# Every symbol include/asp.h declares (tests check the library exports all of them).
EXPORTS = tuple(PROTOTYPES)
# The C-ABI of include/asp_points.h (the 3-D point sampler), kept apart from the table of asp.h.
POINT_PROTOTYPES = {
    "asp_sample3d": [_f] * 6 + [_Q, _d, _d, _d, _Q, _I, _I, _f, _f, _I, _V],
    "asp_sample3d_f64": [_d] * 4 + [_Q, _d, _d, _d, _Q, _I, _I, _f, _f, _I, _V],
}
# The C-ABI of include/asp_profiles.h (halo-centred profiles and aperture sums).
PROFILE_PROTOTYPES = {
    "asp_halo_profiles": [_d, _d, _I, _Q, _d, _d, _Q, _d, _I, _R, _i64, _d, _I, _I, _V],
}
# The C-ABI of include/asp_spectra.h (sightline spectra).
_VELBINS = [_R, _R, _I, _I]  # v0, dv, nbins, ring
SPECTRA_PROTOTYPES = {
    "asp_spectra2d": [_f] * 5 + [_d, _f, _Q, _d, _d, _Q] + _VELBINS + [_I, _I, _f, _f, _I, _V],
    "asp_spectra2d_f64": [_d] * 6 + [_Q, _I, _d, _d, _Q] + _VELBINS + [_I, _I, _f, _f, _I, _V],
}


class ASPError(RuntimeError):
    pass


def build():
    """Compile libasp_hip.so in-tree (hipcc --offload-arch=gfx950)."""
    import subprocess
    subprocess.run(["make", "-s", "-j8", "-C", ROOT], check=True)


def lib():
    """Load libasp_hip.so (torch first when present, so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"HIP extension not built: {LIB_PATH} missing "
                          f"(run `make -C {ROOT}` or __graft_entry__.build())")
    if "torch" not in sys.modules:
        try:  # torch ships its own libamdhip64; load it first so there is one runtime
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    for name, argtypes in {**PROTOTYPES, **POINT_PROTOTYPES, **PROFILE_PROTOTYPES,
                           **SPECTRA_PROTOTYPES}.items():
        fn = getattr(L, name, None)  # (absent from an older A/B build, ASP_LIB)
        if fn is not None:
            fn.argtypes, fn.restype = argtypes, RESTYPES.get(name, C.c_int)
    _lib = L
    return L


def check(rc: int):
    if rc == ASP_OK:
        return
    msg = lib().asp_last_error().decode(errors="replace")
    if rc == ASP_ERR_INVALID:
        raise ValueError(msg)
    if rc == ASP_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == ASP_ERR_NOMEM:
        raise MemoryError(msg)
    raise ASPError(f"HIP error: {msg}")


def require_gpu(device: int = 0):
    n = lib().asp_device_count()
    if n <= 0:
        raise RuntimeError("no HIP device visible: the projector runs on MI355X only "
                           "(there is no CPU fallback)")
    if not 0 <= device < n:
        raise ValueError(f"device {device} out of range (have {n})")


def ptr(a, t=_f):
    """ctypes pointer of a numpy array, or of a torch tensor's device memory, or NULL."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.cast(C.c_void_p(a.data_ptr()), t)
    return a.ctypes.data_as(t)


def last_stats(device: int = 0):
    """The words of asp_last_stats (include/asp.h) by name.  After a k-NN call with
    ASP_KNN_COUNT: ``evals`` window distances, ``evals_small`` per-lane cell-scan distances,
    ``evals_gather`` entries the shared cell pass streamed, ``evals_wide`` top-k insertions,
    ``knn_fallbacks`` (the word of ``large``) waves whose shared cell pass fell back to the
    per-lane pass."""
    s = (C.c_int64 * 16)()
    check(lib().asp_last_stats(device, s, 16))
    return {"records": s[0], "items": s[1], "wide": s[2], "tile": s[3], "tiles": s[4],
            "records_per_item": s[5], "merges": s[6], "slabs": s[7], "large": s[8],
            "knn_fallbacks": s[8],
            "evals": s[9], "evals_small": s[10], "evals_gather": s[11], "evals_wide": s[12],
            "scatter_path": s[13], "placement_runs": s[14], "layout_reuse": s[15]}


def profile(device: int = 0, enable: bool = True, stages=None):
    """Start (and reset) / stop per-stage HIP-event timing inside the library; ``stages``
    (names of PROFILE_STAGES) limits the events to those stages."""
    if stages is None or not enable:
        check(lib().asp_profile(device, 1 if enable else 0))
    else:
        mask = 0
        for s in stages:
            mask |= 1 << PROFILE_STAGES.index(s)
        check(lib().asp_profile_stages(device, mask))


def profile_read(device: int = 0):
    """{stage: (total_ms, launches)} since the last reset."""
    ms = (C.c_double * len(PROFILE_STAGES))()
    n = (C.c_int64 * len(PROFILE_STAGES))()
    check(lib().asp_profile_read(device, ms, n, len(PROFILE_STAGES)))
    return {s: (ms[i], n[i]) for i, s in enumerate(PROFILE_STAGES)}
