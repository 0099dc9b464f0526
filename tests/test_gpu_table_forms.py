"""GPU: the ionisation tables on every kernel form, axis edge and mode (csrc/asp_table.hip).

asp_table_interp3 and asp_table_interp dispatch to k_table<3|2, LDS|global>, k_table_slab
and k_table_nd<1..6> by table shape, fixed axis and column count.  Every comparison here is
BIT-EXACT (table_cases.assert_same: NaN masks, -inf masks, all other elements as uint64
bits) against scipy's RegularGridInterpolator on the same table object
(table_cases.reference), on inputs with rows on the nodes, one ulp either side of them,
outside the table, at +-inf and NaN (table_cases.points); test_table_cases.py holds every
case to the share condition, so none hides in fills.  The one other bar is the fused
10^f of mode 2 on finite rows: rtol 4.5e-16, the project's bar for the device exp10
(test_gpu_table.py), with table values in [-10, 0].

(a) kernel form x shape on both dispatch edges (kTabLdsAxis, kSlabMax) and all axis kinds;
(b) point counts around the block sizes and the slab's second, ragged persistent trip;
(c) -inf and NaN table entries; (d) 1 .. 6 axes with the fixed axis first, middle and last,
3-D through asp_table_interp itself, scipy's 2-D order selection, a 1-D table at a fixed
value; (e) modes 1 and 2 on every kernel form; (f) the error paths of the two entry points.
"""
import ctypes as C

import numpy as np
import pytest

import table_cases as tc

pytestmark = pytest.mark.gpu


def _table(case, zaxis):
    from asp_amd.ionisation import IonisationTable
    return IonisationTable(case["table"], *case["grids"], redshift_input_index=zaxis)


def _check_call(case, what):
    want = tc.reference(case["table"], case["grids"], case["P"])
    tc.assert_same(_table(case, len(case["grids"]) - 1)(case["P"]), want, f"{what} call")


def _check_at_redshift(case, zaxis, P, what):
    tab, g = _table(case, zaxis), case["grids"]
    for label, z, _ in tc.redshifts(g[zaxis]):
        want = tc.reference(case["table"], g, P, zaxis, z)
        tc.assert_same(tab.evaluate_at_redshift(P, float(z)), want, f"{what} zaxis {zaxis} z {label}")


# ---- (a) kernel form x shape ---------------------------------------------------------------

@pytest.mark.parametrize("name", list(tc.FORM_CASES))
def test_forms_call(gpu, name):
    """k_table<3,true> up to 2048 axis nodes in all (s_g full at 2048), <3,false> past it."""
    _check_call(tc.form_case(name), name)


@pytest.mark.parametrize("zaxis", [0, 1, 2])
@pytest.mark.parametrize("name", list(tc.FORM_CASES))
def test_forms_at_redshift(gpu, name, zaxis):
    """zaxis 2: k_table_slab while n0*n1*2 <= 16384 and n0+n1 <= 2048 (s_slab / s_g full on
    the edges, the whole table as the slab at 2x2x2), k_table<2,*> one past either edge;
    zaxis 0 / 1: k_table<2,true|false>.  z on the first, an interior and the last node, one
    ulp below a node, mid-cell, one ulp above the last node, far outside and NaN."""
    case = tc.form_case(name)
    _check_at_redshift(case, zaxis, case["P2"][zaxis], name)


# ---- (b) point counts and tails ------------------------------------------------------------

@pytest.mark.parametrize("form", ["call", "zaxis2", "zaxis0"])
def test_point_counts_and_tails(gpu, form):
    """1024 points per block in k_table, 4096 in k_table_slab: one short, exact, one over."""
    case = tc.form_case("hm01")
    t, g = case["table"], case["grids"]
    if form == "call":
        tab, P, zaxis, z = _table(case, 2), case["P"], None, None
    else:
        zaxis = int(form[-1])
        tab, P, z = _table(case, zaxis), case["P2"][zaxis], float(tc.redshifts(g[zaxis])[3][1])
    want = tc.reference(t, g, P, zaxis, z)
    for n in tc.TAIL_COUNTS:
        got = tab(P[:n]) if zaxis is None else tab.evaluate_at_redshift(P[:n], z)
        tc.assert_same(got, want[:n], f"{form} n {n}")


def test_slab_second_ragged_trip(gpu):
    """2 * CUs * 4096 + 4097 points: k_table_slab runs min(need, 2 * CUs) blocks, so every
    block makes a second trip and the last one is ragged.  Every element is checked."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = tc.form_case("hm01")
    t, g = case["table"], case["grids"]
    P = tc.slab_trip_points(cus)
    assert P.shape[0] == 2 * cus * 4096 + 4097
    z = float(tc.redshifts(g[2])[3][1])
    want = tc.reference(t, g, P, 2, z)
    tc.check_shares(want, "slab trip")
    tc.assert_same(_table(case, 2).evaluate_at_redshift(P, z), want, "slab trip")


# ---- (c) non-finite table entries ----------------------------------------------------------

@pytest.mark.parametrize("name", tc.POISON_CASES)
def test_nonfinite_table_entries(gpu, name):
    """5 % -inf and 1 % NaN entries: scipy's 0 * (-inf) = NaN on the faces of such cells."""
    case = tc.poison_case(name)
    _check_call(case, f"poisoned {name}")
    for zaxis in (0, 1, 2):
        _check_at_redshift(case, zaxis, case["P2"][zaxis], f"poisoned {name}")


def test_nonfinite_table_entries_4d(gpu):
    case = tc.poison_nd_case()
    _check_call(case, "poisoned 4-D")
    for zaxis in case["zaxes"]:
        _check_at_redshift(case, zaxis, case["P1"][zaxis], "poisoned 4-D")


# ---- the C-ABI with device tensors ---------------------------------------------------------

def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


class Abi:
    """One case on the device; ``interp3`` / ``interp`` call the entry points directly."""

    def __init__(self, case):
        self.table = _cuda(case["table"])
        self.axes = [_cuda(g) for g in case["grids"]]
        self.shape = case["table"].shape

    def _io(self, P, a0, a1):
        import torch
        from asp_amd._call import dptr
        P, a0, a1 = _cuda(P), _cuda(a0), _cuda(a1)
        out = torch.full((P.shape[0],), 12345.0, dtype=torch.float64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        return (P, a0, a1, out), dptr, st

    def interp3(self, P, zaxis=0, z=0.0, mode=0, a0=None, a1=None):
        from asp_amd import _lib
        (P, a0, a1, out), d, st = self._io(P, a0, a1)
        _lib.check(_lib.lib().asp_table_interp3(
            d(self.table), *self.shape, *(d(g) for g in self.axes), d(P), P.shape[1], zaxis,
            float(z), P.shape[0], -np.inf, mode, d(a0), d(a1), d(out), 0, st))
        return out.cpu().numpy()

    def interp(self, P, zaxis=0, z=0.0, mode=0, order=0, a0=None, a1=None):
        from asp_amd import _lib
        (P, a0, a1, out), d, st = self._io(P, a0, a1)
        nd = len(self.shape)
        shape = (C.c_int32 * nd)(*self.shape)
        axes = (C.c_void_p * nd)(*(g.data_ptr() for g in self.axes))
        _lib.check(_lib.lib().asp_table_interp(
            d(self.table), nd, shape, axes, d(P), P.shape[1], zaxis, float(z), P.shape[0],
            -np.inf, mode, order, d(a0), d(a1), d(out), 0, st))
        return out.cpu().numpy()


# ---- (d) N-D: asp_table_interp -------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in tc.ND_CASES if n != "3"])
def test_nd_call_and_fixed_axis_anywhere(gpu, name):
    """k_table_nd<1|2|4|5|6> through IonisationTable: 2 .. 5 nodes per axis with a 2-node and
    a clustered axis, the fixed axis first, middle and last."""
    case = tc.nd_case(name)
    _check_call(case, f"nd {name}")
    for zaxis in case["zaxes"]:
        _check_at_redshift(case, zaxis, case["P1"][zaxis], f"nd {name}")


def test_nd_three_axes_through_the_c_abi(gpu):
    """k_table_nd<3> (the class sends 3-D tables to asp_table_interp3): equal to scipy and
    to asp_table_interp3 on the same inputs."""
    case = tc.nd_case("3")
    t, g = case["table"], case["grids"]
    abi = Abi(case)
    want = tc.reference(t, g, case["P"])
    tc.assert_same(abi.interp(case["P"]), want, "nd 3 call")
    tc.assert_same(abi.interp3(case["P"]), want, "interp3 call")
    for zaxis in (0, 1, 2):
        P = case["P1"][zaxis]
        for label, z, _ in tc.redshifts(g[zaxis]):
            want = tc.reference(t, g, P, zaxis, z)
            tc.assert_same(abi.interp(P, zaxis, z), want, f"nd 3 zaxis {zaxis} z {label}")
            tc.assert_same(abi.interp3(P, zaxis, z), want, f"interp3 zaxis {zaxis} z {label}")


@pytest.mark.parametrize("kind", tc.ORDER_KINDS)
def test_2d_order_selection_follows_scipy(gpu, kind):
    """scipy takes its Cython 2-D path (value * w0 * w1) for a writeable native-float64 table
    -- a Fortran-ordered one and the fresh float copy of an integer one included -- and
    _evaluate_linear for read-only, float32 and big-endian ones; the two orders differ in
    the last bit, and scipy runs here on the same object."""
    from asp_amd.ionisation import IonisationTable
    base = tc.nd_case("2")
    t, g = tc.order_variant(base["table"], kind), base["grids"]
    fast = kind in ("writeable", "int64", "fortran")
    for zaxis in (0, 1):
        tab = IonisationTable(t, *g, redshift_input_index=zaxis)
        assert tab._order == int(fast)
        tc.assert_same(tab(base["P"]), tc.reference(t, g, base["P"]), f"{kind} call")
        P = base["P1"][zaxis]
        z = tc.redshifts(g[zaxis])[3][1]
        tc.assert_same(tab.evaluate_at_redshift(P, float(z)), tc.reference(t, g, P, zaxis, z),
                       f"{kind} zaxis {zaxis}")


def test_seven_axes_not_implemented(gpu):
    from asp_amd.ionisation import IonisationTable
    with pytest.raises(NotImplementedError):
        IonisationTable(np.zeros((2,) * 7), *[np.arange(2.0)] * 7)


@pytest.mark.parametrize("name", ["1-two", "1-cluster"])
def test_1d_table_at_fixed_value_is_n_copies(gpu, name):
    """evaluate_at_redshift on a 1-D table: the reference builds an (N, 1) matrix of the
    redshift, so the answer is N copies of table(z) -- -inf for z outside, NaN for NaN."""
    import torch
    case = tc.nd_case(name)
    t, g = case["table"], case["grids"]
    tab = _table(case, 0)
    for n in (7, 1000):
        none = np.empty((n, 0))
        for label, z, inside in tc.redshifts(g[0]):
            got = tab.evaluate_at_redshift(none, float(z))
            tc.assert_same(got, tc.reference(t, g, none, 0, z), f"1-D {name} z {label}")
            assert got.shape == (n,)
            if inside:
                assert np.isfinite(got).all() and (got == got[0]).all()
            elif label == "nan":
                assert np.isnan(got).all()
            else:
                assert (got == -np.inf).all()
    z = float(tc.redshifts(g[0])[3][1])
    dev = tab.evaluate_at_redshift(torch.empty((5, 0), dtype=torch.float64, device="cuda"), z)
    assert dev.is_cuda
    tc.assert_same(dev.cpu().numpy(), tc.reference(t, g, np.empty((5, 0)), 0, z), "device (5, 0)")
    assert tab.evaluate_at_redshift(np.empty((0, 0)), z).shape == (0,)


# ---- (e) modes 1 and 2 on every kernel form ------------------------------------------------

def _check_modes(run, f, what, seed):
    """run(mode, a0, a1) against the reference value f: mode 1 bit-exact (a pure fp64
    product), mode 2 within the exp10 bar on finite rows and exact -- (a0 * a1) * 0.0 for a
    fill row, NaN for a NaN row or product -- on the others."""
    tc.check_shares(f, what)
    a0, a1 = tc.weights(f.size, np.random.default_rng(seed))
    with np.errstate(all="ignore"):
        w = a0 * a1
        want1, want2 = w * f, w * 10.0 ** f
    tc.assert_same(run(1, a0, a1), want1, f"{what} mode 1")
    got2 = run(2, a0, a1)
    fin = np.isfinite(f)
    np.testing.assert_allclose(got2[fin], want2[fin], rtol=4.5e-16, atol=0, err_msg=f"{what} mode 2")
    with np.errstate(invalid="ignore"):  # 10^-inf = +0: (a0 * a1) * 0.0 on a fill row
        assert np.array_equal(want2[f == -np.inf], (w * 0.0)[f == -np.inf], equal_nan=True)
    tc.assert_same(got2[~fin], want2[~fin], f"{what} mode 2, fill and NaN rows")


@pytest.mark.parametrize("form,name", [("<3,true>", "slab16384"), ("<3,false>", "sum2049")])
def test_modes_three_columns(gpu, form, name):
    case = tc.form_case(name)
    abi = Abi(case)
    f = tc.reference(case["table"], case["grids"], case["P"])
    _check_modes(lambda mode, a0, a1: abi.interp3(case["P"], 0, 0.0, mode, a0, a1), f, form, 31)


@pytest.mark.parametrize("form,name,zaxis", [("<2,true>", "slab16384", 0), ("<2,false>", "sum2049", 0),
                                             ("slab", "slab16384", 2)])
def test_modes_ion_masses(gpu, form, name, zaxis):
    """ion_masses reaches the two-column forms: m * X * f and m * X * 10^f."""
    from asp_amd.ionisation import ion_masses
    case = tc.form_case(name)
    tab, P = _table(case, zaxis), case["P2"][zaxis]
    z = float(tc.redshifts(case["grids"][zaxis])[3][1])
    f = tc.reference(case["table"], case["grids"], P, zaxis, z)
    _check_modes(lambda mode, a0, a1: ion_masses(tab, a0, a1, P[:, 0], P[:, 1], z,
                                                 table_is_log10=mode == 2), f, form, 32)


@pytest.mark.parametrize("name,order", [("2", 0), ("2", 1), ("4", 0)])
def test_modes_nd(gpu, name, order):
    """k_table_nd<2> in both arithmetic orders and k_table_nd<4>, all columns and with the
    first axis fixed."""
    case = tc.nd_case(name)
    t = tc.order_variant(case["table"], "writeable" if order else "readonly")
    g = case["grids"]
    abi = Abi(case)
    f = tc.reference(t, g, case["P"])
    _check_modes(lambda mode, a0, a1: abi.interp(case["P"], 0, 0.0, mode, order, a0, a1), f,
                 f"nd {name} order {order}", 33)
    P = case["P1"][0]
    z = float(tc.redshifts(g[0])[3][1])
    f = tc.reference(t, g, P, 0, z)
    _check_modes(lambda mode, a0, a1: abi.interp(P, 0, z, mode, order, a0, a1), f,
                 f"nd {name} order {order} zaxis 0", 34)


# ---- (f) error paths ----------------------------------------------------------------------

def test_error_paths_launch_nothing(gpu):
    """Each bad argument returns its code before any device work: the output keeps its
    sentinel.  n == 0 is OK with NULL pointers."""
    import torch
    from asp_amd import _lib
    from asp_amd._call import dptr as d
    L = _lib.lib()
    INV, UNS, OK = _lib.ASP_ERR_INVALID, _lib.ASP_ERR_UNSUPPORTED, _lib.ASP_OK
    dev = torch.device("cuda:0")
    t = lambda *x: torch.tensor(x, dtype=torch.float64, device=dev)  # noqa: E731
    table, g, pts, w = t(*range(8)), t(0.0, 1.0), t(0.5, 0.5, 0.5), t(1.0)
    out = t(777.0)

    def i3(n0=2, n1=2, n2=2, points=pts, ncol=3, zaxis=0, n=1, mode=0, a0=None, a1=None, o=out):
        return L.asp_table_interp3(d(table), n0, n1, n2, d(g), d(g), d(g), d(points), ncol, zaxis,
                                   0.5, n, -np.inf, mode, d(a0), d(a1), d(o), 0, None)

    def nd(ndim=3, shape=(2, 2, 2), points=pts, ncol=3, zaxis=0, n=1, mode=0, order=0, a0=None,
           a1=None, o=out, tab=table):
        sh = (C.c_int32 * len(shape))(*shape)
        ax = (C.c_void_p * len(shape))(*([g.data_ptr()] * len(shape)))
        return L.asp_table_interp(d(tab), ndim, sh, ax, d(points), ncol, zaxis, 0.5, n, -np.inf,
                                  mode, order, d(a0), d(a1), d(o), 0, None)

    assert i3() == OK and nd() == OK  # the calls are sound before each is broken
    torch.cuda.synchronize()
    assert out.item() == 3.5
    out.fill_(777.0)
    for axis1 in ({"n0": 1}, {"n1": 1}, {"n2": 1}):
        assert i3(**axis1) == INV
    for shape in ((1, 2, 2), (2, 1, 2), (2, 2, 1)):
        assert nd(shape=shape) == INV
    for ncol in (0, 1, 4):
        assert i3(ncol=ncol) == INV and nd(ncol=ncol) == INV
    for zaxis in (-1, 3):
        assert i3(ncol=2, zaxis=zaxis) == INV and nd(ncol=2, zaxis=zaxis) == INV
    for mode in (-1, 3):
        assert i3(mode=mode, a0=w, a1=w) == INV and nd(mode=mode, a0=w, a1=w) == INV
    for order in (-1, 2):
        assert nd(order=order) == INV
    assert i3(n=-1) == INV and nd(n=-1) == INV
    for mode in (1, 2):
        assert i3(mode=mode, a0=None, a1=w) == INV and nd(mode=mode, a0=None, a1=w) == INV
        assert i3(mode=mode, a0=w, a1=None) == INV and nd(mode=mode, a0=w, a1=None) == INV
    assert i3(points=None) == INV and nd(points=None) == INV  # NULL points with columns
    assert nd(ndim=0, shape=(2,)) == UNS and nd(ndim=7, shape=(2,) * 7) == UNS
    assert L.asp_last_error()
    # n == 0: OK with NULL pointers
    assert L.asp_table_interp3(None, 2, 2, 2, None, None, None, None, 3, 0, 0.0, 0, -np.inf, 0,
                               None, None, None, 0, None) == OK
    assert nd(points=None, n=0, o=None, tab=None) == OK
    torch.cuda.synchronize()
    assert out.item() == 777.0
