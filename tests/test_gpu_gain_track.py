"""GPU tier: the gain applied between two solves in one launch (cmpc_gain_track).  No solver: gains, solutions, records and
measured states are drawn with numpy; the reference is the same sums in numpy.longdouble.

Bound per output word: 32 * 2^-53 * (|base| + sum_c |G_rc| |dx_c|).  A 21-term fp64 sum -- the twenty products and the base --
in any order, fused or not, is within gamma_21 = 21 u / (1 - 21 u) of that magnitude (u = 2^-53; each product and dx itself
add one rounding more: 23 u); the rest of the 32 is slack for the reference's own rounding.  Derived, not measured."""
import ctypes

import numpy as np
import pytest
import torch

from cmpc_amd import capi
from cmpc_amd.problem import ProblemSpec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 2
COLUMNS = (0xFFF, 0xFFFFF, 0, 0x1C0)
HELD = {5: "a NaN in the first word of the block", 100: "an Inf in the last", 256: "a NaN in a selected word of x_meas"}
_cache = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _draw(nv, B):
    """(spec, records, XU, G, x_meas) of a draw, once per shape and never modified; rows of G scaled over e^-3 .. e^3.
    B = 257: the planted holds of HELD."""
    if (nv, B) not in _cache:
        spec = ProblemSpec(N=N, nv=nv)
        rng = np.random.default_rng(1000 * nv + B)
        rec = rng.normal(size=(B, spec.nrec))
        XU = rng.normal(size=(B, spec.nsol))
        G = rng.normal(size=(B, 20 + spec.nu, 20)) * np.exp(rng.uniform(-3, 3, size=(B, 20 + spec.nu, 1)))
        xm = rec[:, :20] + rng.normal(scale=0.05, size=(B, 20))
        if B == 257:
            G[5, 0, 0] = np.nan
            G[100, -1, -1] = np.inf
            xm[256, 7] = np.nan                                  # word 7: bit 7 is set in 0xFFF, 0xFFFFF and 0x1C0
        _cache[(nv, B)] = (spec, rec, XU, G, xm)
    return _cache[(nv, B)]


def _solver(spec):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")
    from cmpc_amd.solver import BatchedCentroidalMPC
    return BatchedCentroidalMPC(spec, device=DEV)


def _reference(spec, rec, XU, G, xm, columns):
    """(values, bounds, X[:,1] and U[:,0], hold): rows x_1 then u_0, in longdouble; hold by the rule of include/cmpc.h."""
    sel = np.array([(columns >> c) & 1 for c in range(20)], dtype=bool)
    ld = np.longdouble
    dx = np.where(sel[None, :], xm.astype(ld) - rec[:, :20].astype(ld), ld(0))
    hold = ~np.isfinite(G).all(axis=(1, 2)) | ~np.isfinite(np.where(sel[None, :], xm, 0.0)).all(axis=1) \
        | ~np.isfinite(np.where(sel[None, :], rec[:, :20], 0.0)).all(axis=1)
    n1 = 20 * (N + 1)
    base = np.concatenate([XU[:, 20:40], XU[:, n1:n1 + spec.nu]], axis=1)
    with np.errstate(invalid="ignore"):
        Gl = np.where(np.isfinite(G), G, 0.0).astype(ld)
        dxl = np.where(np.isfinite(dx), dx, ld(0))
        val = base.astype(ld) + np.einsum("brc,bc->br", Gl, dxl)
        mag = np.abs(base).astype(ld) + np.einsum("brc,bc->br", np.abs(Gl), np.abs(dxl))
    bound = 32 * ld(2.0) ** -53 * mag
    return val, bound, base, hold


@pytest.mark.parametrize("columns", COLUMNS, ids=[hex(c) for c in COLUMNS])
@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("nv", [4, 8])
def test_track_matches_the_longdouble_sums_and_holds_where_it_must(nv, B, columns):
    spec, rec, XU, G, xm = _draw(nv, B)
    s = _solver(spec)
    x1, u0, used = s.track(_t(rec), _t(XU), _t(G), _t(xm), columns=columns)
    torch.cuda.synchronize()
    s.close()
    got = np.concatenate([x1.cpu().numpy(), u0.cpu().numpy()], axis=1)
    used = used.cpu().numpy()
    val, bound, base, hold = _reference(spec, rec, XU, G, xm, columns)
    if B == 257:
        want = np.zeros(B, bool)
        want[[b for b, what in HELD.items() if "x_meas" not in what]] = True
        want[256] = columns != 0                                           # (x_meas is not read where nothing is selected)
        assert np.array_equal(hold, want)
    else:
        assert not hold.any()
    assert used.dtype == np.bool_ and np.array_equal(used, ~hold)
    # held: X[:,1] and U[:,0] bit for bit
    assert np.array_equal(got[hold].view(np.int64), base[hold].view(np.int64))
    err = np.abs(got[~hold].astype(np.longdouble) - val[~hold])
    worst = float((err / bound[~hold]).max()) if (~hold).any() else 0.0
    print(f"nv {nv} B {B} columns {columns:#x}: worst error / bound {worst:.3f}, held {int(hold.sum())}")
    assert (err <= bound[~hold]).all()
    if columns == 0:                                                           # nothing selected: dx = 0
        assert np.array_equal(got[~hold], base[~hold])


@pytest.mark.parametrize("nv", [4, 8])
def test_unselected_nan_does_not_hold_and_the_measured_x0_returns_the_solution(nv):
    spec, rec, XU, G, xm = _draw(nv, 3)
    s = _solver(spec)
    xm2 = xm.copy()
    xm2[1, 15] = np.nan                                                        # a foot word: outside 0xFFF
    x1, u0, used = s.track(_t(rec), _t(XU), _t(G), _t(xm2), columns=0xFFF)
    y1, v0, _ = s.track(_t(rec), _t(XU), _t(G), _t(xm), columns=0xFFF)
    torch.cuda.synchronize()
    assert used.all().item()
    assert np.array_equal(x1.cpu().numpy(), y1.cpu().numpy()) and np.array_equal(u0.cpu().numpy(), v0.cpu().numpy())
    # x_meas = x0: X[:,1] and U[:,0] exactly, with every column selected
    x1, u0, used = s.track(_t(rec), _t(XU), _t(G), _t(rec[:, :20]), columns=0xFFFFF)
    torch.cuda.synchronize()
    s.close()
    n1 = 20 * (N + 1)
    assert used.all().item()
    assert np.array_equal(x1.cpu().numpy(), XU[:, 20:40]) and np.array_equal(u0.cpu().numpy(), XU[:, n1:n1 + spec.nu])


def test_columns_beyond_the_state_are_refused_and_a_side_stream_works():
    spec, rec, XU, G, xm = _draw(4, 3)
    s = _solver(spec)
    args = [_t(a) for a in (rec, XU, G, xm)]
    with pytest.raises(ValueError):
        s.track(*args, columns=1 << 20)
    # the C entry point itself
    lib = capi.load()
    x1 = torch.empty((3, 20), dtype=torch.float64, device=DEV)
    u0 = torch.empty((3, spec.nu), dtype=torch.float64, device=DEV)
    used = torch.zeros(3, dtype=torch.bool, device=DEV)
    ptrs = [a.data_ptr() for a in args]
    rc = lib.cmpc_gain_track(N, 4, 3, *ptrs, ctypes.c_uint32((1 << 20) | 0xFFF), x1.data_ptr(), u0.data_ptr(), used.data_ptr(), None)
    assert rc != 0 and "columns" in lib.cmpc_last_error(None).decode()
    rc = lib.cmpc_gain_track(N, 5, 3, *ptrs, ctypes.c_uint32(0xFFF), x1.data_ptr(), u0.data_ptr(), used.data_ptr(), None)
    assert rc != 0 and "cmpc_gain_track" in lib.cmpc_last_error(None).decode()
    ref = s.track(*args)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = s.track(*args, x1_out=x1, u0_out=u0)
    side.synchronize()
    torch.cuda.synchronize()
    s.close()
    assert got[0] is x1 and got[1] is u0
    for a, b in zip(got, ref):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
