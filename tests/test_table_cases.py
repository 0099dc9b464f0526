"""CPU: the inputs and the reference of the ionisation-table GPU tests (table_cases.py).

* the NumPy restatement the existing GPU tests lean on (pyoracle.table_interp3 /
  table_at_redshift) equals scipy's RegularGridInterpolator bit for bit on every axis kind,
  on every shape of the GPU matrix and on tables with -inf and NaN entries;
* every case of the GPU matrix meets the share condition (>= 50 % finite rows, >= 1 % fill,
  >= 0.5 % NaN) on the reference's output, in every call form and at every fixed-axis value
  inside the table, so that no case hides in fills;
* the dispatch constants the shapes are built around are the ones in csrc/asp_table.hip;
* the reference's evaluate_at_redshift on a 1-D table returns N copies of table(z).
"""
import os
import re

import numpy as np
import pytest

import table_cases as tc
from conftest import PKG_ROOT


def forms(case, free="P2"):
    """(label, reference output, inside) of every call form of a case."""
    t, g = case["table"], case["grids"]
    yield "call", tc.reference(t, g, case["P"]), True
    for zaxis, P in case[free].items():
        for label, z, inside in tc.redshifts(g[zaxis]):
            yield f"zaxis {zaxis} z {label}", tc.reference(t, g, P, zaxis, z), inside


def restated(oracle, case):
    t, g = case["table"], case["grids"]

    def quiet(f, *args, **kw):  # (inf coordinates and 1e300-wide cells overflow, as in scipy)
        with np.errstate(all="ignore"):
            return f(*args, **kw)

    yield quiet(oracle.table_interp3, t, g, case["P"])
    for zaxis, P in case["P2"].items():
        for _, z, _ in tc.redshifts(g[zaxis]):
            yield quiet(oracle.table_at_redshift, t, g, P, float(z), zaxis=zaxis)


@pytest.mark.parametrize("name", list(tc.FORM_CASES) + ["hm01"])
def test_restatement_equals_scipy_and_shares_hold(oracle, name):
    case = tc.form_case(name)
    for (label, want, inside), got in zip(forms(case), restated(oracle, case)):
        tc.assert_same(got, want, f"{name} {label}")
        if inside:
            tc.check_shares(want, f"{name} {label}")
        else:  # a fixed value outside the axis fills (or NaNs) every row
            assert not np.isfinite(want).any(), (name, label)


@pytest.mark.parametrize("name", tc.POISON_CASES)
def test_restatement_equals_scipy_on_nonfinite_tables(oracle, name):
    case, clean = tc.poison_case(name), tc.form_case(name)
    t = case["table"]
    assert abs((t == -np.inf).mean() - 0.05) < 0.002 and abs(np.isnan(t).mean() - 0.01) < 0.001
    for (label, want, inside), got in zip(forms(case), restated(oracle, case)):
        tc.assert_same(got, want, f"{name} {label}")
        if inside:
            tc.check_shares(want, f"{name} {label}")
    # the entries are met: rows that the clean table answers with a number and this one does not
    want = tc.reference(t, case["grids"], case["P"])
    was = tc.reference(clean["table"], clean["grids"], clean["P"])
    assert (np.isfinite(was) & ~np.isfinite(want)).mean() >= 0.05
    assert (np.isfinite(was) & np.isnan(want)).mean() >= 0.02


@pytest.mark.parametrize("name", tc.ND_CASES)
def test_nd_cases_meet_the_share_condition(name):
    case = tc.nd_case(name)
    sizes = [g.size for g in case["grids"]]
    assert min(sizes) >= 2 and max(sizes) <= 5
    if len(sizes) >= 2:
        assert 2 in sizes
    for label, want, inside in forms(case, "P1"):
        if inside:
            tc.check_shares(want, f"nd {name} {label}")


def test_poisoned_4d_case_meets_the_share_condition():
    case = tc.poison_nd_case()
    t = case["table"]
    assert (t == -np.inf).sum() == round(0.05 * t.size) and np.isnan(t).sum() == round(0.01 * t.size)
    for label, want, inside in forms(case, "P1"):
        if inside:
            tc.check_shares(want, f"4-D {label}")
    assert np.isnan(tc.reference(t, case["grids"], case["P"])).mean() >= 0.03


def test_slab_trip_and_tail_points_meet_the_share_condition():
    case = tc.form_case("hm01")
    g = case["grids"]
    P = tc.slab_trip_points(256)  # an MI355X's 256 CUs
    assert P.shape == (2 * 256 * 4096 + 4097, 2)
    tc.check_shares(tc.reference(case["table"], g, P, 2, 0.5 * (g[2][20] + g[2][21])), "slab trip")
    assert case["P"].shape[0] == max(tc.TAIL_COUNTS)


def test_order_variants_take_scipys_paths():
    """What each 2-D table kind is, so that the GPU test compares the order selection on the
    kinds it names; writeable / read-only differ in the last bit somewhere."""
    case = tc.nd_case("2")
    v = {k: tc.order_variant(case["table"], k) for k in tc.ORDER_KINDS}
    assert v["writeable"].flags.writeable and not v["readonly"].flags.writeable
    assert v["float32"].dtype == np.float32 and v["big-endian"].dtype.byteorder == ">"
    assert v["int64"].dtype == np.int64
    assert v["fortran"].flags.f_contiguous and not v["fortran"].flags.c_contiguous
    a = tc.reference(v["writeable"], case["grids"], case["P"])
    b = tc.reference(v["readonly"], case["grids"], case["P"])
    ok = np.isfinite(a)
    assert np.array_equal(ok, np.isfinite(b)) and np.allclose(a[ok], b[ok], rtol=1e-14, atol=0)
    assert (a[ok] != b[ok]).any(), "the two arithmetic orders never differ on this case"


def test_axis_kinds():
    rng = np.random.default_rng(0)
    for kind in ("uniform", "jitter", "log", "log600", "neglog600", "cluster", "far"):
        for n in (2, 3, 40):
            g = tc.axis(kind, n, rng)
            assert g.size == n and np.all(np.diff(g) > 0) and np.all(np.isfinite(g))
    g = tc.axis("cluster", 40, rng)
    assert g[-2] - g[1] <= 1e-6 and g[1] - g[0] > 0.5 and g[-1] - g[-2] > 0.5
    assert tc.axis("far", 40, rng)[0] > 1e9
    assert np.array_equal(tc.axis("subnormal", 4, rng), [0.0, 5e-324, 1e-323, 1.0])


def test_points_recipe():
    rng = np.random.default_rng(1)
    grids = [tc.axis("jitter", 9, rng), tc.axis("log", 30, rng)]
    P = tc.points(grids, 20000, rng)
    for c, g in enumerate(grids):
        x = P[:, c]
        assert 0.10 < np.isin(x, g).mean() < 0.18
        assert 0.005 < np.isin(x, np.nextafter(g, np.inf)).mean() < 0.02
        assert 0.005 < np.isin(x, np.nextafter(g, -np.inf)).mean() < 0.02
        assert (x == np.nextafter(g[-1], np.inf)).any() and (x == np.nextafter(g[0], -np.inf)).any()
    assert np.isnan(P[::97]).any(axis=1).all()
    assert np.isposinf(P).any() and np.isneginf(P).any()


def test_assert_same_tells_bits_apart():
    a = np.array([1.0, -np.inf, np.nan, 0.0])
    tc.assert_same(a.copy(), a)
    tc.assert_same(np.array([1.0, -np.inf, -np.nan, 0.0]), a)  # NaN sign is not compared
    for other in ([np.nextafter(1.0, 2.0), -np.inf, np.nan, 0.0], [1.0, -np.inf, np.nan, -0.0],
                  [1.0, np.nan, np.nan, 0.0], [1.0, np.inf, np.nan, 0.0], [-np.inf, -np.inf, np.nan, 0.0]):
        with pytest.raises(AssertionError):
            tc.assert_same(np.array(other), a)


def test_dispatch_constants_match_the_source():
    with open(os.path.join(PKG_ROOT, "csrc", "asp_table.hip")) as f:
        src = f.read()
    for name, value in (("kTabLdsAxis", 2048), ("kSlabMax", 16384), ("kTabBlock", 256),
                        ("kTabPerThread", 4), ("kSlabBlock", 1024), ("kSlabPerThread", 4),
                        ("kTabMaxDims", 6)):
        found = re.findall(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", src)
        assert found == [str(value)], (name, found)
    # the shapes against the constants: on the edge and one past it
    shape = {k: v[0] for k, v in tc.FORM_CASES.items()}
    assert sum(shape["sum2048"]) == 2048 and sum(shape["sum2049"]) == 2049
    assert shape["slab16384"][0] * shape["slab16384"][1] * 2 == 16384
    assert shape["slab16512"][0] * shape["slab16512"][1] * 2 > 16384
    assert sum(shape["slab16512"]) <= 2048
    assert sum(shape["pair2048"][:2]) == 2048 and sum(shape["pair2049"][:2]) == 2049
    assert shape["pair2049"][0] * shape["pair2049"][1] * 2 <= 16384  # only the axes say no
    assert sum(shape["large"]) > 2048 and shape["large"][0] * shape["large"][1] * 2 > 16384


def test_reference_1d_at_redshift_is_n_copies():
    """IonisationTableBase.evaluate_at_redshift on a 1-D table builds an (N, 1) matrix of the
    redshift: N copies of table(z), fill outside the axis, NaN for a NaN redshift."""
    g = np.array([0.0, 1.0, 2.0])
    t = np.array([1.0, 5.0, 2.0])
    none = np.empty((7, 0))
    assert np.array_equal(tc.reference(t, [g], none, 0, 0.5), np.full(7, 3.0))
    assert np.array_equal(tc.reference(t, [g], none, 0, 2.5), np.full(7, -np.inf))
    assert np.isnan(tc.reference(t, [g], none, 0, np.nan)).all()
    assert tc.reference(t, [g], np.empty((0, 0)), 0, 0.5).shape == (0,)
