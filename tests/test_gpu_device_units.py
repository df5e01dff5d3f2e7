"""GPU-tier unit tests of the seven device-only pieces the host emulation replaces by plain C++ (tests/emu):
the Newton pivot square root on v_rsq_f64, the inline-asm LDS batch-read helpers, the fp64 MFMA tile with the
lane layout the blocked Cholesky feeds it, and the wave primitives -- cmpc_pair_of<M> (the butterfly exchange of every
wave-wide reduction of the solvers and of the whole-body QP kernel), cmpc_bcast, cmpc_uniform_d and CMPC_RELANE.  Each
is run in isolation (tests/gpu_unit/cmpc_device_unit.hip) against values computed on the host."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import build as _b

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unit():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    lib = ctypes.CDLL(_b.build_device_unit())
    vp = ctypes.c_void_p
    lib.unit_pivot_sqrt.argtypes = [vp, vp, vp, ctypes.c_int]
    lib.unit_lds_helpers.argtypes = [vp]
    lib.unit_mfma_tile.argtypes = [vp, vp, vp]
    lib.unit_pair_of.argtypes = [vp, vp, vp]
    lib.unit_reduce.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int]
    lib.unit_bcast.argtypes = [vp, vp]
    lib.unit_uniform_d.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int]
    lib.unit_relane.argtypes = [vp]
    return lib


def test_pivot_sqrt_matches_ieee_sqrt(unit):
    """Pivots range from the 1e-8 acceptance floor to barrier-inflated 1e+15: sqrt to 1 ulp, 1/sqrt to 2 ulp."""
    rng = np.random.default_rng(0)
    p = np.concatenate([10.0 ** rng.uniform(-8, 15, size=200000), [1e-8, 1.0, 4.0, 2.0 ** 52, 1e15, 3e-7]])
    d_p = torch.from_numpy(p).to("cuda:0")
    d_s, d_i = torch.empty_like(d_p), torch.empty_like(d_p)
    assert unit.unit_pivot_sqrt(d_p.data_ptr(), d_s.data_ptr(), d_i.data_ptr(), p.size) == 0
    s, inv = d_s.cpu().numpy(), d_i.cpu().numpy()
    ref = np.sqrt(p)
    assert (np.abs(s - ref) <= np.spacing(ref)).all()
    assert (np.abs(inv - 1.0 / ref) <= 2 * np.spacing(1.0 / ref)).all()
    assert np.abs(s * inv - 1.0).max() < 1e-15


def test_lds_batch_read_helpers(unit):
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    assert unit.unit_lds_helpers(bad.data_ptr()) == 0
    assert int(bad.item()) == 0


def test_mfma_f64_tile_layout(unit):
    rng = np.random.default_rng(1)
    A, B = rng.normal(size=(16, 16)), rng.normal(size=(16, 16))
    d_a, d_b = torch.from_numpy(A).to("cuda:0"), torch.from_numpy(B).to("cuda:0")
    d_d = torch.zeros((16, 16), dtype=torch.float64, device="cuda:0")
    assert unit.unit_mfma_tile(d_a.data_ptr(), d_b.data_ptr(), d_d.data_ptr()) == 0
    want = A @ B.T
    assert np.abs(d_d.cpu().numpy() - want).max() < 1e-13


def _random_bits(rng, n):
    """n finite doubles with random bits in both 32-bit halves (sign, exponent and all 52 mantissa bits)."""
    while True:
        v = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64).view(np.float64)
        if np.isfinite(v).all() and np.unique(v.view(np.uint64) >> 32).size == n and np.unique(v.view(np.uint32)[::2]).size == n:
            return v


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _pair_of(unit, v):
    d_v = torch.from_numpy(v).to("cuda:0")
    d_a = torch.zeros((6, 64), dtype=torch.float64, device="cuda:0")
    d_b = torch.zeros_like(d_a)
    assert unit.unit_pair_of(d_v.data_ptr(), d_a.data_ptr(), d_b.data_ptr()) == 0
    return _bits(d_a.cpu().numpy()), _bits(d_b.cpu().numpy())


def test_pair_of_hands_each_lane_its_own_and_its_partners_word(unit):
    """The two 32-bit halves of a double travel separately: every word of the input differs from every other in both
    halves, so a hi / lo mix-up or a wrong partner cannot go unseen.  Compared bit for bit."""
    rng = np.random.default_rng(2)
    lane = np.arange(64)
    for _ in range(4):
        v = _random_bits(rng, 64)
        a, b = _pair_of(unit, v)
        vb = _bits(v)
        for row, M in enumerate((32, 16, 8, 4, 2, 1)):
            if M == 4:      # row_ror:4 reaches lane ^ 4 or lane ^ 12 (which one differs by lane): good enough after the step of 8
                assert (a[row] == vb).all() and ((b[row] == vb[lane ^ 4]) | (b[row] == vb[lane ^ 12])).all()
            else:           # {a, b} = {own, partner's} as a multiset
                own_first = (a[row] == vb) & (b[row] == vb[lane ^ M])
                own_second = (b[row] == vb) & (a[row] == vb[lane ^ M])
                assert (own_first | own_second).all(), M
    # ... and where lanes 8 apart agree, as they do when the steps run from 32 down, the rotate by 4 IS the exchange
    v = _random_bits(rng, 64)
    v[lane | 8] = v[lane & ~8]
    a, b = _pair_of(unit, v)
    assert (a[3] == _bits(v)).all() and (b[3] == _bits(v)[lane ^ 4]).all()


def _host_butterfly(op, v):
    """The emulation's definition of the six-step reduction (tests/emu: v = op(v, v of lane ^ M), M = 32 .. 1), fp64."""
    v = v.copy()
    lane = np.arange(64)
    for M in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, lane ^ M])
    return v


def test_six_step_reductions_match_the_host_butterfly(unit):
    """Solver::wave_sum and the bfly_max / bfly_min chains of red_max / red_min over vectors of magnitudes 1e-300 .. 1e300:
    every lane holds the bits of the host butterfly, which is what the CPU tier runs.  Maxima and minima also see
    +-inf and NaN (the kernels rely on fmax / fmin dropping a NaN: np.fmax / np.fmin); the sums see no NaN and neither
    sees a zero (the sign of fmax(+0, -0) and of a sum of mixed-sign zeros is not what is under test)."""
    rng = np.random.default_rng(3)
    n = 300
    mag = lambda: 10.0 ** rng.uniform(-300, 300, size=(n, 64)) * rng.choice([-1.0, 1.0], size=(n, 64))
    vs, vm = mag(), mag()
    vs[: n // 2] = 10.0 ** rng.uniform(-3, 3, size=(n // 2, 64)) * rng.choice([-1.0, 1.0], size=(n // 2, 64))   # (sums that round)
    special = rng.uniform(size=(n, 64))
    vm[special < 0.10] = np.nan
    vm[(special >= 0.10) & (special < 0.13)] = np.inf
    vm[(special >= 0.13) & (special < 0.16)] = -np.inf
    vm[0, 1:] = np.nan                                            # one survivor
    vm[1, :] = np.nan; vm[1, 37] = -np.inf
    assert not np.isnan(vm).all(axis=1).any()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_vs, d_vm = d(vs), d(vm)
    d_sum, d_max, d_min = torch.zeros_like(d_vs), torch.zeros_like(d_vs), torch.zeros_like(d_vs)
    assert unit.unit_reduce(d_vs.data_ptr(), d_vm.data_ptr(), d_sum.data_ptr(), d_max.data_ptr(), d_min.data_ptr(), n) == 0
    with np.errstate(over="ignore", invalid="ignore"):
        want = [_host_butterfly(np.add, vs), _host_butterfly(np.fmax, vm), _host_butterfly(np.fmin, vm)]
    assert np.isfinite(want[0]).all() and not np.isnan(want[1]).any() and not np.isnan(want[2]).any()
    assert (want[1] == np.nanmax(vm, axis=1, keepdims=True)).all() and (want[2] == np.nanmin(vm, axis=1, keepdims=True)).all()
    for got, ref in zip((d_sum, d_max, d_min), want):
        got = got.cpu().numpy()
        assert (_bits(got) == _bits(got[:, :1])).all()            # every lane the same bits
        assert (_bits(got) == _bits(ref)).all()


def test_bcast_from_every_source_lane(unit):
    v = _random_bits(np.random.default_rng(4), 64)
    d_v = torch.from_numpy(v).to("cuda:0")
    d_o = torch.zeros((64, 64), dtype=torch.float64, device="cuda:0")
    assert unit.unit_bcast(d_v.data_ptr(), d_o.data_ptr()) == 0
    assert (_bits(d_o.cpu().numpy()) == _bits(v)[:, None]).all()    # row src: 64 copies of v[src]


def test_uniform_d_between_a_vector_producer_and_a_vector_consumer(unit):
    """cmpc_uniform_d is inline asm: the wait states between the vector-ALU write, the v_readfirstlane and the vector-ALU
    read are s_nop counted by hand, which the compiler neither checks nor pads.  No host emulation or static check can
    see that hazard -- running the sequence with its producer (a vector FMA) right in front and its consumer (a
    vector multiply) right behind, for values that change from one turn of the loop to the next, is the only check there
    is.  A stale read would return the previous turn's value (or half of it)."""
    rng = np.random.default_rng(5)
    n = 64
    x, y, z = _random_bits(rng, n), 10.0 ** rng.uniform(-3, 3, size=n), np.empty(n)
    x = np.ldexp(np.frexp(x)[0], rng.integers(-20, 20, size=n))      # random mantissas, products that neither overflow nor vanish
    z[:] = -x * y * (1.0 + rng.uniform(-1e-3, 1e-3, size=n))       # cancellation: the FMA's single rounding matters
    fac = _random_bits(rng, 64)
    fac = np.ldexp(np.frexp(fac)[0], rng.integers(-8, 8, size=64))
    rep = lambda a: torch.from_numpy(np.ascontiguousarray(np.repeat(a[:, None], 64, axis=1))).to("cuda:0")
    d_x, d_y, d_z, d_f = rep(x), rep(y), rep(z), torch.from_numpy(fac).to("cuda:0")
    d_o = torch.zeros((n, 64), dtype=torch.float64, device="cuda:0")
    assert unit.unit_uniform_d(d_x.data_ptr(), d_y.data_ptr(), d_z.data_ptr(), d_f.data_ptr(), d_o.data_ptr(), n) == 0
    u = np.array([float(Fraction(a) * Fraction(b) + Fraction(c)) for a, b, c in zip(x, y, z)])   # exact, rounded once: the FMA
    assert np.unique(u).size == n and (u != 0).all()
    assert (_bits(d_o.cpu().numpy()) == _bits(u[:, None] * fac[None, :])).all()


def test_relane_in_a_two_wave_workgroup(unit):
    d_o = torch.full((128,), -7, dtype=torch.int32, device="cuda:0")
    assert unit.unit_relane(d_o.data_ptr()) == 0
    assert d_o.cpu().tolist() == list(range(128))
