"""Halo-centred radial profiles and aperture sums on the GPU (asp_halo_profiles,
asp_amd.haloes.halo_profiles / aperture_sums) against the NumPy brute force of the definition
(tests/halo_profile_ref.py; tests/test_halo_profile_ref.py pins it to scipy's periodic KDTree).

The bar of every case (halo_profile_ref.assert_bar): count equals the brute force exactly; where
count == 0 the sum is exactly 0; where count == 1 the sum is bit-equal to the member's property;
elsewhere |sum - ref| <= count * 2^-52 * S_abs, S_abs the brute force's sum of |prop| over the
bin -- two fp64 summation orders of k terms are each within (k - 1) 2^-53 S_abs of the exact
sum, so the bound is derived, not measured.
"""
import numpy as np
import pytest

from halo_profile_ref import assert_bar, brute_profiles, lattice_case, lattice_shells, mixed_case

pytestmark = pytest.mark.gpu

KNOBS = ("ASP_PROFILE_LIGHT", "ASP_PROFILE_ITEM", "ASP_PROFILE_PRUNE", "ASP_PROFILE_BATCH",
         "ASP_PROFILE_CELLS")


@pytest.fixture(scope="module")
def mixed():
    """The mixed case with its brute force (all four properties), computed once."""
    c = mixed_case()
    c["ref"] = brute_profiles(c["pos"], c["centres"], c["radii"], c["edges"], c["L"], c["props"])
    assert c["ref"].gap > 2.0 ** -40
    return c


def run(c, props=(), radii="own", edges=None, **kw):
    from asp_amd.haloes import halo_profiles
    return halo_profiles(c["pos"], c["centres"], c["radii"] if isinstance(radii, str) else radii,
                         c["edges"] if edges is None else edges, c["L"], list(props), **kw)


_REFS = {}


def ref_for(key, c, radii, edges, props):
    """The brute force of a variant of the mixed case, computed once per module."""
    if key not in _REFS:
        _REFS[key] = brute_profiles(c["pos"], c["centres"], radii, edges, c["L"], props)
    return _REFS[key]


def sub(ref, ks):
    """The brute force restricted to properties ks."""
    from halo_profile_ref import Ref
    return Ref(ref.count, ref.sums[list(ks)], ref.sabs[list(ks)], ref.gap)


def test_mixed_defaults(gpu, mixed):
    count, sums = run(mixed, mixed["props"])
    assert_bar(count, sums, mixed["ref"])
    ones = sums[3]  # the property of ones: sum = count up to the bar (exactly, in fact)
    assert np.array_equal(ones, count.astype(np.float64))
    assert count[6].sum() == len(mixed["pos"]) and count[5].sum() == 0


@pytest.mark.parametrize("env", [
    {"ASP_PROFILE_LIGHT": "0"},                                # every halo in the wave class
    {"ASP_PROFILE_LIGHT": "2147483647"},                       # every halo in the lane class
    {"ASP_PROFILE_LIGHT": "0", "ASP_PROFILE_ITEM": "64"},      # many items per halo
    {"ASP_PROFILE_LIGHT": "0", "ASP_PROFILE_ITEM": "1"},       # the item cap (1024 per halo)
    {"ASP_PROFILE_LIGHT": "0", "ASP_PROFILE_ITEM": "1073741824"},  # one item per halo
    {"ASP_PROFILE_LIGHT": "300", "ASP_PROFILE_ITEM": "301"},   # both classes, items of a few rows
    {"ASP_PROFILE_PRUNE": "0"},
    {"ASP_PROFILE_PRUNE": "0", "ASP_PROFILE_LIGHT": "0"},
    {"ASP_PROFILE_BATCH": "6001"},                             # four batches
    {"ASP_PROFILE_BATCH": "997", "ASP_PROFILE_LIGHT": "0"},    # twenty-one
    {"ASP_PROFILE_CELLS": "1"},
    {"ASP_PROFILE_CELLS": "2"},
    {"ASP_PROFILE_CELLS": "7"},
    {"ASP_PROFILE_CELLS": "2", "ASP_PROFILE_LIGHT": "0", "ASP_PROFILE_ITEM": "50"},
    {"ASP_PROFILE_CELLS": "33", "ASP_PROFILE_LIGHT": "2147483647"},
    {"ASP_PROFILE_CELLS": "64", "ASP_PROFILE_LIGHT": "0"},
], ids=lambda e: "-".join(f"{k[12:]}={v}" for k, v in e.items()))
def test_mixed_every_knob_each_way(gpu, mixed, monkeypatch, env):
    """Every class sees every halo, every item size, every grid: same counts, sums in the bar."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    count, sums = run(mixed, mixed["props"][:2])
    assert_bar(count, sums, sub(mixed["ref"], (0, 1)))


def test_prune_counts_are_identical_and_saves_pairs(gpu, mixed, monkeypatch):
    from asp_amd.device import stats
    monkeypatch.setenv("ASP_PROFILE_COUNT", "1")
    count, _ = run(mixed)
    tested = stats(0)["evals"]
    monkeypatch.setenv("ASP_PROFILE_PRUNE", "0")
    count0, _ = run(mixed)
    assert np.array_equal(count, count0) and np.array_equal(count, mixed["ref"].count)
    assert count.sum() <= tested <= stats(0)["evals"] <= len(mixed["pos"]) * len(mixed["centres"])


@pytest.mark.parametrize("ks", [(), (2,), (0, 1, 2, 3)], ids=["0", "1", "4"])
def test_mixed_nprops(gpu, mixed, ks):
    count, sums = run(mixed, [mixed["props"][k] for k in ks])
    assert sums.shape == (len(ks),) + count.shape
    assert_bar(count, sums, sub(mixed["ref"], ks))


@pytest.mark.parametrize("light", [None, "0", "2147483647"])
@pytest.mark.parametrize("nbins", [1, 64])
def test_mixed_nbins(gpu, mixed, monkeypatch, nbins, light):
    if light is not None:
        monkeypatch.setenv("ASP_PROFILE_LIGHT", light)
    edges = np.array([0.0, 1.0]) if nbins == 1 else np.linspace(0.0, 3.0, 65) ** 2 / 3.0
    props = mixed["props"][:1]
    ref = ref_for(nbins, mixed, mixed["radii"], edges, props)
    count, sums = run(mixed, props, edges=edges)
    assert count.shape == (300, nbins)
    assert_bar(count, sums, ref)


@pytest.mark.parametrize("light", [None, "0", "2147483647"])
def test_mixed_absolute_edges(gpu, mixed, monkeypatch, light):
    """radii=None: the edges are lengths, the same for every halo; 0.3 > 0: the particles
    nearest a centre are left out, and 6 > L / 2 reaches past the half box."""
    if light is not None:
        monkeypatch.setenv("ASP_PROFILE_LIGHT", light)
    edges = np.array([0.3, 0.5, 1.0, 2.5, 6.0])
    props = mixed["props"][1:3]
    ref = ref_for("absolute", mixed, None, edges, props)
    assert ref.gap > 2.0 ** -40
    count, sums = run(mixed, props, radii=None, edges=edges)
    assert_bar(count, sums, ref)


@pytest.mark.parametrize("light", [None, "0", "2147483647"])
def test_lattice_ties(gpu, monkeypatch, light):
    """d2 exactly on a threshold: T_b <= d2 < T_b+1, hand-derived shells."""
    if light is not None:
        monkeypatch.setenv("ASP_PROFILE_LIGHT", light)
    c = lattice_case()
    count, sums = run(c, c["props"])
    for j in range(len(c["centres"])):
        assert count[j].tolist() == lattice_shells() == [1, 26, 66]
    assert np.array_equal(sums[0], count.astype(np.float64))
    count, _ = run(c, edges=np.array([0.5, 1.0, 2.0, 3.0]))  # edges[0] > 0: not the centre's own
    assert count[0].tolist() == [0, 26, 66]
    for cells in ("1", "3", "8"):
        monkeypatch.setenv("ASP_PROFILE_CELLS", cells)
        count, _ = run(c)
        assert np.all(count == np.array([1, 26, 66]))


def test_odd_values(gpu, mixed):
    c = dict(mixed)
    pos = mixed["pos"].copy()
    rows = np.array([0, 63, 64, 4000, 19_999])
    pos[rows, [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    prop = mixed["props"][0].copy()
    prop[[7, 5000]] = [np.nan, np.inf]
    c["pos"] = pos
    ref = brute_profiles(pos, c["centres"], c["radii"], c["edges"], c["L"], [prop, mixed["props"][3]])
    assert 0 < (~np.isfinite(ref.sums[0])).sum() < ref.count.size // 2
    assert ref.count[6].sum() == len(pos) - len(rows)  # a non-finite row belongs to no halo
    count, sums = run(c, [prop, mixed["props"][3]])
    assert_bar(count, sums, ref)  # (the non-finite bins are exactly the brute force's)
    # a centre at exactly L, a negative radius
    bad = mixed["centres"].copy()
    bad[123, 2] = mixed["L"]
    with pytest.raises(ValueError, match="box"):
        run(dict(mixed, centres=bad))
    neg = mixed["radii"].copy()
    neg[77] = -1e-9
    with pytest.raises(ValueError, match="radius"):
        run(mixed, radii=neg)
    neg[77] = np.nan
    with pytest.raises(ValueError, match="radius"):
        run(mixed, radii=neg)


def test_accumulate_two_halves(gpu, mixed):
    """ASP_F_ACCUMULATE: the two halves of the particles added up equal one call on all."""
    from asp_amd.haloes import halo_profiles
    h = len(mixed["pos"]) // 2
    props = mixed["props"][:2]
    args = (mixed["centres"], mixed["radii"], mixed["edges"], mixed["L"])
    first = halo_profiles(mixed["pos"][:h], *args, [p[:h] for p in props])
    count, sums = halo_profiles(mixed["pos"][h:], *args, [p[h:] for p in props], accumulate=first)
    assert count is first[0] and sums is first[1]
    assert_bar(count, sums, sub(mixed["ref"], (0, 1)))


def test_device_tensors_on_a_stream(gpu, mixed):
    """Device tensors give the counts of host arrays, and a call on a side stream is ordered:
    its inputs are written on that stream just before and its outputs read on it after."""
    import torch
    dev = torch.device("cuda:0")
    from asp_amd.haloes import halo_profiles
    props = mixed["props"][:2]
    host_count, _ = run(mixed, props)
    pos = torch.from_numpy(mixed["pos"]).to(dev)
    dprops = [torch.from_numpy(p).to(dev) for p in props]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        moved = pos + 0.0   # produced on the side stream: the call must run behind it
        count, sums = halo_profiles(moved, mixed["centres"], mixed["radii"], mixed["edges"],
                                    mixed["L"], dprops, stream=stream)
        total = count.sum()  # consumed on the side stream
    stream.synchronize()
    assert count.is_cuda and count.dtype == torch.int64 and sums.dtype == torch.float64
    assert np.array_equal(count.cpu().numpy(), host_count)
    assert int(total) == int(host_count.sum())
    assert_bar(count.cpu().numpy(), sums.cpu().numpy(), sub(mixed["ref"], (0, 1)))
    # accumulate on the device, no properties
    c2, s2 = halo_profiles(pos, mixed["centres"], mixed["radii"], mixed["edges"], mixed["L"])
    c3, _ = halo_profiles(pos, mixed["centres"], mixed["radii"], mixed["edges"], mixed["L"],
                          accumulate=(c2, s2))
    torch.cuda.synchronize()
    assert c3 is c2 and np.array_equal(c3.cpu().numpy(), 2 * host_count) and s2.shape == (0, 300, 5)


def test_aperture_sums_are_the_first_bin(gpu, mixed):
    from asp_amd.haloes import aperture_sums
    from halo_profile_ref import Ref
    ref = mixed["ref"]
    count, sums = aperture_sums(mixed["pos"], mixed["centres"], mixed["radii"], mixed["L"],
                                mixed["props"][:2], factor=0.25)
    assert count.shape == (300,) and sums.shape == (2, 300)
    first = Ref(ref.count[:, :1], ref.sums[:2, :, :1], ref.sabs[:2, :, :1], ref.gap)
    assert_bar(count[:, None], np.ascontiguousarray(sums[:, :, None]), first)
    # the cumulative profile: inside 2 R
    count, _ = aperture_sums(mixed["pos"], mixed["centres"], mixed["radii"], mixed["L"], factor=2.0)
    assert np.array_equal(count, ref.count[:, :4].sum(axis=1))
