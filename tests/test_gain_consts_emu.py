"""CPU tier: the solver with a gain AND per-instance constants (Solver<..., GAIN, CONSTS>, cmpc_solve_batch_gain_consts) as the
host emulation of the device source runs it (tests/emu/cmpc_emu_gain_consts.cpp).  The reference throughout is code that was
there before: the gain emulation on a spec of its own (tests/emu/cmpc_emu_gain.cpp) and tests/gain_reference.py.  Rows that say
what the spec says give that emulation's bits; every instance of a mixed batch is its group's own gain solve; drawn rows
against the independent gain on each instance's own spec; a refused row has no gain and disturbs nobody, the next instance
on its slot included.  Small cases: the harness runs 64 OS threads per instance."""
import ctypes
import os

import numpy as np
import pytest

import build as _b
import gain_reference as gr
from consts_common import drawn_specs, uniform_rows
from test_gain_emu import LEVEL
from cmpc_amd import problem, workloads as wl
from cmpc_amd.problem import to_cspec

#: the inputs of test_gain_emu.py::test_gain_matches_reference that show a status-0 instance with a finite gain each
GROUPS = {"perturbed": dict(N=10, B=3, scale=0.25), "payload": dict(N=10, B=3), "randomized": dict(N=10, B=3, rate=10)}
_ref = {}


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_b.build_emu_gain_consts())


@pytest.fixture(scope="module")
def gain_emu():
    return ctypes.CDLL(_b.build_emu_gain())


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _solve(lib, spec, rec, rows=None, pair=False, fail_iter=None, fill=None):
    """(out, status, iters, kkt, state_out, G) of the emulated gain solve: on the spec (rows None, the gain emulation) or with
    the rows (the GAIN + CONSTS variant).  Every output starts from a value the solver never writes."""
    env = dict(CMPC_EMU_PAIR="1" if pair else "0")
    if fail_iter is not None:
        env["CMPC_EMU_FAIL_ITER"] = str(fail_iter)
    if fill is not None:
        env["CMPC_EMU_FILL"] = fill
    os.environ.update(env)
    try:
        cs = to_cspec(spec)
        rec = np.ascontiguousarray(rec, dtype=np.float64)
        B = rec.shape[0]
        out, so = np.full((B, spec.nsol), 7.0), np.full((B, spec.nstate), 7.0)
        st, it, kk = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.full(B, 7.0)
        G = np.full((B, 20 + spec.nu, 20), 7.0)
        if rows is None:
            rc = lib.cmpc_emu_solve_batch_gain(ctypes.byref(cs), B, _p(rec), None, None, _p(out), _p(so), _p(st), _p(it), _p(kk), _p(G))
        else:
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            assert rows.shape == (B, problem.NCONST)
            rc = lib.cmpc_emu_solve_batch_gain_consts(ctypes.byref(cs), B, _p(rec), _p(rows), None, None, _p(out), _p(so), _p(st),
                                                      _p(it), _p(kk), _p(G))
        assert rc == 0
        return out, st, it, kk, so, G
    finally:
        for k in env:
            os.environ.pop(k, None)


def _group(gain_emu, name, pair):
    """(spec, records, the gain emulation's own solve of them), computed once per group and kernel shape."""
    if (name, pair) not in _ref:
        spec, rec = wl.make_workload(name, **GROUPS[name])
        _ref[(name, pair)] = (spec, rec, _solve(gain_emu, spec, rec, pair=pair))
    return _ref[(name, pair)]


def _same(a, b, ia=slice(None), ib=slice(None)):
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        assert np.array_equal(x[ia], y[ib], equal_nan=True)


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_rows_of_the_spec_are_bitwise_the_gain_solve(emu, gain_emu, name, pair):
    spec, rec, ref = _group(gain_emu, name, pair)
    ok = ref[1] == 0
    assert ok.any() and np.isfinite(ref[5][ok]).all()                      # (a gain to compare, not only NaNs)
    _same(_solve(emu, spec, rec, rows=uniform_rows(spec, rec.shape[0]), pair=pair), ref)


def test_mixed_batch_is_bitwise_the_groups_own_gain_solves(emu, gain_emu, pair=False):
    """(The single wave; the pair is covered on every group above and takes the refusal below.)
    The nine instances of the three groups (nominal 4 / 0.1; payload 7 / 1; mpc_rate 10: 5 / 0.2, delta 0.1, no force-rate
    cost) interleaved in one batch, each with its own row: solution, verdict, state and gain of its group's own solve."""
    names = sorted(GROUPS)
    groups = [_group(gain_emu, n, pair) for n in names]
    assert len({(g[0].delta, g[0].k1, g[0].k2) for g in groups}) == 3
    order = [(g, i) for i in range(3) for g in range(3)]                       # (group, instance of the group)
    rec = np.stack([groups[g][1][i] for g, i in order])
    rows = problem.consts_rows([groups[g][0] for g, _ in order])
    # the handle's own constants are none of the groups': only the rows count
    handle = wl.make_workload("perturbed", B=1, N=10)[0]
    handle.k1, handle.k2, handle.w_hw = 6.0, 0.5, 500.0
    mixed = _solve(emu, handle, rec, rows=rows, pair=pair)
    n_gain = 0
    for j, (g, i) in enumerate(order):
        _same(mixed, groups[g][2], j, i)
        n_gain += int(np.isfinite(mixed[5][j]).all())
    assert n_gain >= 3


def test_drawn_rows_match_the_reference_gain_on_each_instances_own_spec(emu):
    """Level: test_gain_emu.py's LEVEL[1].  Weakly active instances are counted and printed, as that test does."""
    spec, rec = wl.make_workload("perturbed", B=3, N=10, scale=0.25)
    _, specs = drawn_specs(spec, 3)
    out, st, _, _, _, G = _solve(emu, spec, rec, rows=problem.consts_rows(specs))
    worst, skipped, n = 0.0, 0, 0
    for b in range(3):
        if st[b] != 0:
            continue
        n += 1
        assert np.isfinite(G[b]).all(), f"instance {b}: status 0 without a finite gain"
        Gr, weak, _ = gr.gain(to_cspec(specs[b]), rec[b], out[b])
        if weak:
            skipped += 1
            continue
        e = gr.rel_err_groups(G[b], Gr, spec.nv)
        print(f"instance {b}: {e}")
        worst = max(worst, max(e.values()))
        assert max(e.values()) <= LEVEL[1], f"instance {b}: {e}"
        # the row matters: the gain on the shared spec at the same point is another one
        e0 = gr.rel_err_groups(G[b], gr.gain(to_cspec(spec), rec[b], out[b])[0], spec.nv)
        assert max(e0.values()) > LEVEL[1], e0
    print(f"drawn rows: worst {worst:.2e}, weakly active {skipped}/{n}, statuses {st.tolist()}")
    assert n - skipped >= 1


@pytest.mark.parametrize("field,value,pair", [("k2", float("nan"), False), ("delta", 0.0, True)], ids=["k2-nan-single", "delta-0-pair"])
def test_a_refused_row_has_no_gain_and_its_neighbours_are_untouched(emu, gain_emu, field, value, pair):
    spec, rec, good = _group(gain_emu, "perturbed", pair)
    rows = uniform_rows(spec, 3)
    rows[1, problem.CONST_FIELDS.index(field)] = value
    got = _solve(emu, spec, rec, rows=rows, pair=pair)
    out, st, it, kk, so, G = got
    assert st[1] == 2 and it[1] == 0 and kk[1] == np.inf and np.isnan(out[1]).all()
    assert np.isnan(G[1]).all()                                                # every word of the block
    assert so[1, spec.nstate - 8 - 2 * (spec.N + 1)] == 0.0                    # no solver state
    _same(got, good, [0, 2], [0, 2])


def test_a_refused_first_instance_leaves_the_slots_saved_iterate_clean(emu, gain_emu):
    """One slot: the emulation runs the batch in order on one saved iterate.  The refused instance comes first; the next one
    fails its last factorisation and returns -- and takes its gain at -- the point it saved, through that saved iterate.  Slab,
    LDS and saved iterate start as NaN: what the refused instance leaves is what the next one finds."""
    spec, rec = wl.make_workload("randomized", B=2, N=3)
    it0 = _solve(gain_emu, spec, rec[:1])[2]
    fail = int(it0[0]) - 1
    alone = _solve(gain_emu, spec, rec[:1], fail_iter=fail, fill="nan")
    assert alone[1][0] == 3 and np.isfinite(alone[5][0]).all()                 # (the saved point, with a gain)
    rows = uniform_rows(spec, 2)
    rows[0, problem.CONST_FIELDS.index("k2")] = float("nan")
    got = _solve(emu, spec, rec[[0, 0]], rows=rows, fail_iter=fail, fill="nan")
    assert got[1][0] == 2 and got[2][0] == 0 and np.isnan(got[5][0]).all() and np.isnan(got[0][0]).all()
    _same(got, alone, [1], [0])
