"""The Python call layer on the GPU: every ``stream=`` takes a torch stream or its raw handle,
and the wrappers that create device temporaries (the ``.contiguous()`` copy of a strided
input, the upload of a host array) do so on the call's stream -- the results are those of the
default stream.  (The ordering itself is by construction, asp_amd/_call.stream_scope; a test
cannot show a race that is absent, and these do not try to.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4096


def _strided_positions():
    """(strided (N, 3) float64 device view, its contiguous copy), ready on every stream."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(11)
    base = torch.rand((3, N), dtype=torch.float64, device="cuda", generator=g)
    pos = base.t()
    assert not pos.is_contiguous() and pos.shape == (N, 3)
    want = pos.contiguous()
    torch.cuda.synchronize()
    return pos, want


def test_stream_scope_is_the_calls_stream(gpu):
    import torch
    from asp_amd._call import raw_stream, stream_scope
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    assert raw_stream(side, dev) == raw_stream(side.cuda_stream, dev) == side.cuda_stream
    assert raw_stream(None, dev) == torch.cuda.current_stream(dev).cuda_stream
    for stream in (side, side.cuda_stream):
        with stream_scope(dev, stream) as scope:
            assert scope.raw == side.cuda_stream
            assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream
            t = torch.ones(8, device=dev)
            scope.keep(t, None)
        assert torch.cuda.current_stream(dev).cuda_stream != side.cuda_stream
    with torch.cuda.stream(side), stream_scope(dev, None) as scope:
        assert scope.raw == side.cuda_stream
    side.synchronize()
    assert float(t.sum()) == 8.0


def test_knn_strided_positions_on_a_side_stream(gpu):
    import torch
    from asp_amd.knn import knn_smoothing_lengths
    pos, contiguous = _strided_positions()
    want = knn_smoothing_lengths(contiguous, 32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for stream in (side, side.cuda_stream):
        got = knn_smoothing_lengths(pos, 32, stream=stream)
        side.synchronize()
        assert got.dtype == torch.float64 and torch.equal(got, want)
    assert bool(torch.isfinite(want).all()) and float(want.min()) > 0


def test_stage_strided_positions_on_a_side_stream(gpu):
    import torch
    from asp_amd.stage import stage_particles
    pos, contiguous = _strided_positions()
    g = torch.Generator(device="cuda").manual_seed(12)
    h = torch.rand(N, dtype=torch.float64, device="cuda", generator=g) * 0.05
    a = torch.rand((N, 2), dtype=torch.float64, device="cuda", generator=g)[:, 0]  # strided too
    assert not a.is_contiguous()
    want = stage_particles(contiguous, h, a.contiguous(), projection_axis=0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for stream in (side, side.cuda_stream):
        u, v, hf, (a0,) = stage_particles(pos, h, a, projection_axis=0, stream=stream)
        side.synchronize()
        for got, w in zip((u, v, hf, a0), (want[0], want[1], want[2], want[3][0])):
            assert got.dtype == torch.float32 and got.shape == (N,) and torch.equal(got, w)
    assert torch.equal(want[0], contiguous[:, 1].float())  # axis 0: (u, v) = (y, z)


def test_props_f64_host_arrays_under_a_side_stream(gpu, oracle):
    """project2d_props_f64 uploads its host arrays itself: called while a side stream is
    torch's current one, each map equals asp_project2d_f64's map of that property.  Both are
    within the value bar E of the exact sum over the same (fp64-decided) neighbour sets, E
    with value_bar.F64_INPUT_ULPS as the device rounds the raw fp64 h and a itself, so they
    differ by at most 2 E per pixel; zero pixels agree exactly."""
    import torch
    import value_bar as vb
    from asp_amd.device import project2d_f64, project2d_props_f64
    rng = np.random.default_rng(21)
    n, size, ext, kernel = 2000, (64, 64), (-1.0, 1.0, -1.0, 1.0), "wendland_c2"
    pos = rng.normal(0, 0.4, (n, 3))
    h = rng.uniform(0.02, 0.2, n)
    props = [rng.uniform(0.5, 2.0, n), rng.uniform(1e3, 1e5, n)]
    kw = dict(projection_axis=2, image_size=size, extent=ext, chunk_size=vb.CHUNK, kernel=kernel)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        maps = project2d_props_f64(pos, h, props, **kw)
    side.synchronize()
    s = dict(u=pos[:, 0], v=pos[:, 1], h=h, cls=np.zeros(n, int), names=("all",))
    for a, got in zip(props, maps):
        assert got.dtype == torch.float32 and tuple(got.shape) == size
        want, _ = project2d_f64(pos, h, a, **kw)
        E, by_class = vb.bar2d(oracle, s, a, kernel, size=size, ext=ext,
                               extra_ulps=vb.F64_INPUT_ULPS)
        assert np.count_nonzero(want) > size[0] * size[1] // 2
        worst = vb.assert_terms_close(got.cpu().numpy(), want, 2.0 * E, by_class)
        print(f"props_f64 vs project2d_f64: worst |g - r| / 2E = {worst:.3g}")


def test_project2d_and_project3d_take_stream_objects(gpu):
    import torch
    from asp_amd.device import project2d, project2d_props, project3d
    from asp_amd.plummer import plummer_torch
    d = plummer_torch(1000, seed=3, h_law="physical", extent=4.0, grid=64, device="cuda")
    ones = torch.ones_like(d["h"])
    kw2 = dict(image_size=(64, 64), extent=(-4.0, 4.0, -4.0, 4.0), kernel="indicator")
    kw3 = dict(cube_size=(32, 32, 32), extent=(-4.0, 4.0) * 3, kernel="indicator")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    maps, cubes, multi = [], [], []
    for stream in (side.cuda_stream, side):
        maps.append(project2d(d["x"], d["y"], d["h"], ones, stream=stream, **kw2)[0])
        multi.append(project2d_props(d["x"], d["y"], d["h"], [ones], stream=stream, **kw2)[0])
        cubes.append(project3d(d["x"], d["y"], d["z"], d["h"], ones, stream=stream, **kw3))
        side.synchronize()
    assert torch.equal(maps[0], maps[1]) and torch.equal(cubes[0], cubes[1])
    assert torch.equal(multi[0], maps[0]) and torch.equal(multi[1], maps[0])
    assert float(maps[0].sum()) > 0 and float(cubes[0].sum()) > 0
    assert torch.equal(maps[0], maps[0].round()) and torch.equal(cubes[0], cubes[0].round())
