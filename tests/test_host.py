"""CPU-side tests: the C-ABI library loads and exports every declared symbol, the host
mirror of the reference interface behaves like the reference, synthetic inputs follow
their laws.  No GPU compute here."""
import os
import re

import numpy as np
import pytest

from conftest import REPO


def test_header_symbols_exported(asp):
    """Every function include/asp.h declares is exported by libasp_hip.so."""
    from asp_amd import _lib
    hdr = open(os.path.join(REPO, "include", "asp.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(asp_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert L.asp_version() // 10000 == 1


def test_no_device_is_loud(asp):
    """On a host without a GPU the product path raises; there is no CPU fallback."""
    from asp_amd import _lib
    from asp_amd.tools.projections import create_image
    if _lib.lib().asp_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError, match="no HIP device"):
        create_image([[0, 0, 0]], [0.5], [1.0], (4, 4), 4, 2, -1, 1, -1, 1)


def test_c_abi_argument_validation(asp):
    """Argument errors are reported as ASP_ERR_INVALID before any device work."""
    from asp_amd import _lib
    L = _lib.lib()
    z = np.zeros(1, np.float32)
    o = np.zeros(16, np.float32)
    P = _lib.ptr
    # x_max < x_min
    rc = L.asp_project2d(P(z), P(z), P(z), P(z), None, 1, 1.0, -1.0, -1.0, 1.0, 4, 4, 4, 0, 0,
                         P(o), None, 0, None)
    assert rc == _lib.ASP_ERR_INVALID and b"grid" in L.asp_last_error()
    rc = L.asp_project2d(P(z), P(z), P(z), P(z), None, 1, -1.0, 1.0, -1.0, 1.0, 4, 4, 4, 7, 0,
                         P(o), None, 0, None)
    assert rc == _lib.ASP_ERR_INVALID
    rc = L.asp_project2d(P(z), P(z), P(z), P(z), P(z), 1, -1.0, 1.0, -1.0, 1.0, 4, 4, 4, 0, 0,
                         P(o), None, 0, None)
    assert rc == _lib.ASP_ERR_INVALID  # a1 without out1
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_axis_resolution(asp):
    from asp_amd import CoordinateAxes
    from asp_amd._axes import axis_index
    assert [axis_index(a) for a in CoordinateAxes] == [0, 1, 2]
    assert axis_index("x") == 0 and axis_index("Y") == 1 and axis_index("z") == 2
    assert axis_index(b"x") == 0 and axis_index(7) == 2  # anything else is Z, as in the ref
    assert str(CoordinateAxes.X) == "x" and CoordinateAxes.from_string(" Z ") == CoordinateAxes.Z
    with pytest.raises(ValueError):
        CoordinateAxes.from_string("w")

    class RefAxes:  # the reference's enum: only .name matters
        name = "Y"
    assert axis_index(RefAxes()) == 1


def test_kernel_plugin_resolution(asp):
    from asp_amd.tools.projections import (indicator_kernel, quartic_spline_kernel,
                                           wendland_c2_kernel)
    from asp_amd.tools.projections._kernels import kernel_id_of
    assert kernel_id_of(quartic_spline_kernel) == 0
    assert kernel_id_of(wendland_c2_kernel) == 1
    assert kernel_id_of(indicator_kernel) == 2

    def quartic_spline_kernel_ref(r, h):
        return r
    # a callable that merely shares the reference kernel's name is NOT taken for the
    # native kernel: every non-package callable goes to the plugin path (None)
    quartic_spline_kernel_ref.__name__ = "quartic_spline_kernel"
    assert kernel_id_of(quartic_spline_kernel_ref) is None
    assert kernel_id_of(lambda r, h: r) is None
    with pytest.raises(TypeError):
        kernel_id_of(3.0)
    from asp_amd.tools.projections._kernels import native_kernel_id
    with pytest.raises(TypeError):
        native_kernel_id(lambda r, h: r)
    assert native_kernel_id(wendland_c2_kernel) == 1
    with pytest.raises(ValueError, match="dtype"):
        quartic_spline_kernel(np.zeros(3, np.float32), np.ones(3))
    assert quartic_spline_kernel(np.zeros(0), np.zeros(0)).shape == (0,)


def test_create_image_argument_errors(asp):
    from asp_amd.tools.projections import create_image
    with pytest.raises(ValueError):
        create_image(np.zeros((3, 2)), np.ones(3), np.ones(3), (4, 4), 4, 2, -1, 1, -1, 1)
    with pytest.raises(ValueError):
        create_image(np.zeros((3, 3)), np.ones(2), np.ones(3), (4, 4), 4, 2, -1, 1, -1, 1)
    with pytest.raises(ValueError, match="zero"):
        create_image(np.zeros((3, 3)), np.ones(3), np.ones(3), (4, 4), 0, 2, -1, 1, -1, 1)
    with pytest.raises(TypeError):
        create_image(np.zeros((3, 3)), np.ones(3), np.ones(3), (4, 4), 2.5, 2, -1, 1, -1, 1)
    # negative chunk size: range(0, N, -k) is empty in the reference -> zero image, no GPU
    img = create_image(np.zeros((3, 3)), np.ones(3), np.ones(3), (4, 5), -2, 2, -1, 1, -1, 1)
    assert img.shape == (4, 5) and img.dtype == np.float64 and not img.any()


def test_create_images_argument_errors(asp):
    """create_images (several maps from one binning): the property count and each array's
    length are checked before the device is touched, and the no-GPU shortcuts of
    create_image (negative chunk size -> zero maps) hold per map."""
    from asp_amd.tools.projections import create_images
    pos, h = np.zeros((3, 3)), np.ones(3)
    with pytest.raises(ValueError):
        create_images(pos, h, [], (4, 4), 4, 2, -1, 1, -1, 1)
    with pytest.raises(ValueError):
        create_images(pos, h, [np.ones(3)] * 7, (4, 4), 4, 2, -1, 1, -1, 1)
    with pytest.raises(ValueError):
        create_images(pos, h, [np.ones(3), np.ones(2)], (4, 4), 4, 2, -1, 1, -1, 1)
    maps = create_images(pos, h, [np.ones(3), np.ones(3)], (4, 5), -2, 2, -1, 1, -1, 1)
    assert len(maps) == 2 and all(m.shape == (4, 5) and not m.any() for m in maps)


def test_plummer_laws():
    from asp_amd.plummer import plummer
    p = plummer(20000, seed=0, h_law="physical")
    r = np.linalg.norm(p["pos"], axis=1)
    assert np.allclose(r, p["r"])
    # Plummer enclosed-mass fraction M(<r) = r^3 / (1 + r^2)^1.5 (u capped at 0.999)
    for rr in (0.5, 1.0, 2.0):
        frac = np.mean(r < rr)
        assert abs(frac - rr ** 3 / (1 + rr * rr) ** 1.5) < 0.015
    assert np.allclose(p["h"], 1.2 * np.cbrt(p["m"] / p["rho"]))
    q = plummer(100, seed=0, h_law="pixel", grid=4096, extent=4.0)
    assert np.all(q["h"] == 0.75 * 8.0 / 4096)
    assert np.array_equal(plummer(50, seed=3)["pos"], plummer(50, seed=3)["pos"])


def test_zslab_bounds_equal_count():
    import torch
    from asp_amd.distributed import zslab_bounds
    z = torch.randn(200_000)
    e = zslab_bounds(z, 4)
    assert len(e) == 5 and e[0] == float("-inf") and e[-1] == float("inf")
    counts = [int(((z >= e[r]) & (z < e[r + 1])).sum()) for r in range(4)]
    assert sum(counts) == z.numel()
    assert max(counts) - min(counts) < 0.02 * z.numel()


def test_plugin_argument_lengths():
    """The plug-in session reads len(h) rows of positions: mismatched arrays are a
    ValueError before any native call (as the native path's _call.host_f64 checks)."""
    from asp_amd.tools.projections._plugin import project_callable
    f = lambda r, h: r  # noqa: E731
    pos = np.zeros((10, 3))
    with pytest.raises(ValueError):
        project_callable(pos, np.ones(12), [np.ones(12)], (2, 2), (8, 8), 4, (0, 1, 0, 1), f)
    with pytest.raises(ValueError):
        project_callable(pos, np.ones(10), [np.ones(9)], (2, 2), (8, 8), 4, (0, 1, 0, 1), f)
    with pytest.raises(ValueError):
        project_callable(np.zeros((10, 2)), np.ones(10), [np.ones(10)], (2, 2), (8, 8), 4,
                         (0, 1, 0, 1), f)


def test_cpu_baseline_chunk_counts():
    """bench.py's CPU-baseline regressor: the particles the reference's chunk cull admits
    (_projector.py:38-48) into each chunk, by a 2-D difference array -- equal to the
    brute-force count of the cull's inequalities for every chunk."""
    import sys
    sys.path.insert(0, REPO)
    import bench
    rng = np.random.default_rng(5)
    n, G, cs, ext = 20_000, 256, 32, 4.0
    pos = rng.normal(0, 1.2, (n, 3))
    h = rng.uniform(0.0, 0.3, n)
    x = bench.chunk_cull_counts(pos, h, G, cs, ext)
    nc, w = G // cs, 2 * ext / (G // cs)
    u, v, r = pos[:, 0], pos[:, 1], 2 * np.abs(h)
    want = np.zeros(nc * nc)
    for cx in range(nc):
        for cy in range(nc):
            xl, yl = -ext + cx * w, -ext + cy * w
            want[cx * nc + cy] = np.sum((u >= xl - r) & (u < xl + w + r) & (v >= yl - r) &
                                        (v < yl + w + r))
    assert np.abs(x - want).max() <= 0.001 * want.max()  # float edge cases at chunk bounds


def test_bench_workload_tags():
    """bench.py's config tag: configs[3] (cfg4) is the Z-slab decomposition only; a row-slab
    line at the same size is tagged cfg4-rows (verdict r04: a row line labelled cfg4)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.workload_tag(100_000_000, 4096, 1, False) == "cfg3"
    assert b.workload_tag(100_000_000, 4096, 8, False) == "cfg4"
    assert b.workload_tag(100_000_000, 4096, 8, True) == "cfg4-rows"
    assert b.workload_tag(10_000_000, 2048, 1, False) == "cfg2"
    assert b.workload_tag(2_000_000, 1024, 2, True) == "custom"


def test_bench_n_gt_1_defaults(monkeypatch):
    """The N > 1 defaults: north_star's Z-slabs + one reduce; rows gather by all-gather."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(REPO, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8"])
    a = b.parse()
    assert a.decomp == "zslab" and a.op == "reduce" and a.rows_gather == "all"


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """bench.py --dump-outputs: small arrays whole (float64 kept, the rest as float32, None
    left out); arrays above the budget as the same sorted, duplicate-free sample of their
    elements on every call; --full and --dump-outputs are off by default."""
    import importlib.util
    import sys
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(REPO, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 2
    x = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    y = torch.arange(7, dtype=torch.float64)
    b.dump_outputs(str(tmp_path / "a"), {"x": x, "y": y, "none": None})
    assert sorted(os.listdir(tmp_path / "a")) == ["x.npy", "y.npy"]
    gx, gy = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "y.npy")
    assert gx.dtype == np.float32 and gx.shape == (10, 100) and np.array_equal(gx, x.numpy())
    assert gy.dtype == np.float64 and np.array_equal(gy, y.numpy())
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 4000)  # x (4000 B) + z (8000 B) no longer fit
    z = torch.arange(1000, dtype=torch.float64) * 0.5
    for d in ("b", "c"):
        b.dump_outputs(str(tmp_path / d), {"x": x, "z": z})
    sx, sz = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "b" / "z.npy")
    assert sx.dtype == np.float32 and sz.dtype == np.float64
    assert sx.nbytes + sz.nbytes <= 4000 and sx.size == 500 and sz.size == 250
    assert np.all(np.diff(sx) > 0) and np.all(np.diff(sz) > 0)  # elements of x / z, no repeats
    assert np.all(sx == np.round(sx)) and sx.max() < 1000 and np.all(sz * 2 == np.round(sz * 2))
    assert np.array_equal(sx, np.load(tmp_path / "c" / "x.npy"))
    assert np.array_equal(sz, np.load(tmp_path / "c" / "z.npy"))


def test_row_slabs_group_needs_u():
    """A group member passing u=None would skip the all-reduce the others join (a hang);
    it is refused instead."""
    import pytest
    from asp_amd.distributed import row_slabs
    with pytest.raises(ValueError, match="needs u on every rank"):
        row_slabs(4096, 4, None, (-1.0, 1.0), group=object())
