"""Every compute entry point rejects a device index outside [0, asp_device_count()) with
ASP_ERR_INVALID -- the one check that guards the index into the library's per-device
tables -- and leaves nothing behind: the same call on device 0 then succeeds (no lock held,
no end event missing).  Each call is the smallest valid one (one particle / row / point)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXT = (-1.0, 1.0, -1.0, 1.0)  # a 4 x 4 image, chunk size 2, Wendland C2
MAP = (*EXT, 4, 4, 2, 1)


def _f32(*v):
    return np.array(v, dtype=np.float32)


def _f64(*v):
    return np.array(v, dtype=np.float64)


def _calls():
    """name -> f(device) -> return code; keeps every array alive in the closure."""
    import torch
    from asp_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    _d, _f, _i32, _i64 = _lib._d, _lib._f, _lib._i32, _lib._i64
    u, v, h, a = _f32(0.1), _f32(-0.2), _f32(0.3), _f32(1.0)
    out = np.zeros((4, 4), dtype=np.float32)
    pos, h64, a64 = _f64(0.1, -0.2, 0.05).reshape(1, 3), _f64(0.3), _f64(1.0)
    props = (_f * 1)(p(a))
    outs = (_f * 1)(p(out))
    cube = np.zeros((4, 4, 4), dtype=np.float32)
    hk, idx, dist = np.zeros(1), np.zeros(1, dtype=np.int32), np.zeros(1)
    query, centre, first = pos + 1.0, pos + 1.5, np.zeros(1, dtype=np.int32)  # inside [0, 4)^3
    ids, counts = np.array([7], dtype=np.int64), np.zeros(3, dtype=np.int64)
    row, taken = _f64(2.5), np.zeros(1)
    n_out = C.c_int64(0)
    cr = [np.zeros(1, dtype=np.int32) for _ in range(4)]
    pix, off, nb, tot = (np.array([5], dtype=np.int64), np.zeros(2, dtype=np.int64),
                         np.zeros(4, dtype=np.int32), C.c_int64(0))
    dev = torch.device("cuda:0")
    t = lambda *x: torch.tensor(x, dtype=torch.float64, device=dev)  # noqa: E731
    da, db, dout = t(0.25, 1.5, 2.75), t(1.0), t(0.0, 0.0, 0.0)
    table, grid, pts, tout = t(*range(8)), t(0.0, 1.0), t(0.5, 0.5, 0.5), t(0.0)
    table1, pts1 = t(1.0, 3.0), t(0.5)
    axes = (C.c_void_p * 1)(grid.data_ptr())
    shape = (C.c_int32 * 1)(2)
    r0, r1 = torch.tensor([1.0, 4.0], device=dev), torch.tensor([2.0, 0.0], device=dev)
    su, sv = torch.zeros(1, device=dev), torch.zeros(1, device=dev)  # (device outputs)
    tile_pairs = np.zeros(1, dtype=np.int64)

    def pairs_begin(d):
        session = C.c_void_p()
        rc = L.asp_pairs_begin(p(pos, _d), p(h64, _d), 1, 2, *EXT, 4, 4, 2, 0, d, None,
                               p(tile_pairs, _i64), C.byref(session))
        if session:
            assert L.asp_pairs_end(session) == _lib.ASP_OK
        return rc

    return {
        "asp_project2d": lambda d: L.asp_project2d(p(u), p(v), p(h), p(a), None, 1, *MAP, 0,
                                                   p(out), None, d, None),
        "asp_project2d_rows": lambda d: L.asp_project2d_rows(p(u), p(v), p(h), p(a), None, 1, *EXT,
                                                             4, 4, 2, 0, 4, 1, 0, p(out), None, d,
                                                             None),
        "asp_project2d_f64": lambda d: L.asp_project2d_f64(p(pos, _d), p(h64, _d), p(a64, _d), None,
                                                           1, 2, *MAP, 0, p(out), None, d, None),
        "asp_project2d_props": lambda d: L.asp_project2d_props(p(u), p(v), p(h), props, 1, 1, *MAP,
                                                               0, outs, d, None),
        "asp_project2d_sph": lambda d: L.asp_project2d_sph(p(u), p(v), p(h), p(a), None, props, 1,
                                                           1, *MAP, 0, outs, d, None),
        "asp_project3d": lambda d: L.asp_project3d(p(u), p(v), p(h), p(h), p(a), 1, *EXT, -1.0, 1.0,
                                                   4, 4, 4, 0, 4, 1, 0, p(cube), d, None),
        "asp_knn_smoothing_lengths": lambda d: L.asp_knn_smoothing_lengths(p(pos, _d), 1, 1,
                                                                           p(hk, _d), 0, d, None),
        "asp_nearest": lambda d: L.asp_nearest(p(query, _d), 1, p(centre, _d), 1, None, 1, 4.0,
                                               p(idx, _i32), p(dist, _d), 0, d, None),
        "asp_match_ids": lambda d: L.asp_match_ids(p(ids, _i64), None, 1, p(ids, _i64), None, 1, 0,
                                                   p(idx, _i32), None, p(counts, _i64), 0, d, None),
        "asp_take_rows": lambda d: L.asp_take_rows(row.ctypes.data, 1, 8, p(first, _i32), 1, None,
                                                   taken.ctypes.data, 0, d, None),
        "asp_stage_particles": lambda d: L.asp_stage_particles(p(pos, _d), None, None, None, 1, 2,
                                                               None, 0.0, 0, p(su), p(sv), None,
                                                               None, None, 1, C.byref(n_out), 0, d,
                                                               None),
        "asp_periodic": lambda d: L.asp_periodic(_lib.ASP_PB_WRAP, p(da, _d), 3, None, 1, 3, 1.0, 0,
                                                 p(dout, _d), d, None),
        "asp_wrapped_distance": lambda d: L.asp_wrapped_distance(p(da, _d), 3, p(dout, _d), 3, 1,
                                                                 1.0, 0, p(db, _d), d, None),
        "asp_kernel_eval": lambda d: L.asp_kernel_eval(1, p(h64, _d), p(h64, _d), p(hk, _d), 1, 0,
                                                       d, None),
        "asp_chunk_ranges": lambda d: L.asp_chunk_ranges(p(u), p(v), p(h), 1, *EXT, 4, 4, 2,
                                                         *(p(c, _i32) for c in cr), 0, d, None),
        "asp_pixel_neighbours": lambda d: L.asp_pixel_neighbours(p(u), p(v), p(h), 1, *EXT, 4, 4, 2,
                                                                 p(pix, _i64), 1, p(off, _i64),
                                                                 p(nb, _i32), 4, C.byref(tot), d),
        "asp_table_interp3": lambda d: L.asp_table_interp3(p(table, _d), 2, 2, 2, p(grid, _d),
                                                           p(grid, _d), p(grid, _d), p(pts, _d), 3,
                                                           0, 0.0, 1, -np.inf, 0, None, None,
                                                           p(tout, _d), d, None),
        "asp_table_interp": lambda d: L.asp_table_interp(p(table1, _d), 1, shape, axes, p(pts1, _d),
                                                         1, 0, 0.0, 1, -np.inf, 0, 0, None, None,
                                                         p(tout, _d), d, None),
        "asp_ratio": lambda d: L.asp_ratio(p(r0), p(r1), 2, d, None),
        "asp_pairs_begin": pairs_begin,
    }


@pytest.fixture(scope="module")
def calls(gpu):
    return _calls()


@pytest.mark.parametrize("name", [
    "asp_project2d", "asp_project2d_rows", "asp_project2d_f64", "asp_project2d_props",
    "asp_project2d_sph", "asp_project3d", "asp_knn_smoothing_lengths", "asp_nearest",
    "asp_match_ids", "asp_take_rows", "asp_stage_particles", "asp_periodic",
    "asp_wrapped_distance", "asp_kernel_eval", "asp_chunk_ranges", "asp_pixel_neighbours",
    "asp_table_interp3", "asp_table_interp", "asp_ratio", "asp_pairs_begin"])
def test_bad_device_is_invalid_and_leaves_nothing_behind(calls, name):
    import torch
    from asp_amd import _lib
    call = calls[name]
    for device in (-1, _lib.lib().asp_device_count()):
        assert call(device) == _lib.ASP_ERR_INVALID, (name, device)
    assert call(0) == _lib.ASP_OK, (name, _lib.lib().asp_last_error())
    torch.cuda.synchronize()
