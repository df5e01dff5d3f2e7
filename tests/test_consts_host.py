"""CPU tier: the host side of the per-instance constants (cmpc_solve_batch_consts) -- the row layout in Python, in the
header and in the library's cmpc_spec_consts agree.  Needs the built library, not a device."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

from consts_common import drawn_specs, header_const_fields
from cmpc_amd import capi, problem
from cmpc_amd.problem import CSpec, ProblemSpec, to_cspec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cmpc.h")


@pytest.fixture(scope="module")
def lib():
    # (plain CDLL: capi.load() would do as well, this keeps the test to the one symbol it is about)
    so = ctypes.CDLL(capi.LIB_PATH)
    so.cmpc_spec_consts.argtypes = [ctypes.POINTER(CSpec), ctypes.POINTER(ctypes.c_double)]
    so.cmpc_spec_consts.restype = None
    return so


def _c_row(lib, spec):
    row = (ctypes.c_double * problem.NCONST)()
    lib.cmpc_spec_consts(ctypes.byref(to_cspec(spec)), row)
    return np.array(row[:])


def test_symbols_are_listed():
    assert "cmpc_solve_batch_consts" in capi.SYMBOLS and "cmpc_spec_consts" in capi.SYMBOLS


def test_consts_row_is_the_librarys_row(lib):
    base = ProblemSpec(N=10)
    specs = [base, dataclasses.replace(base, delta=0.1, k1=5.0, k2=0.2, w_rate=0.0), dataclasses.replace(base, k1=7.0, k2=1.0)]
    specs += drawn_specs(base, 5)[1]
    # every field distinct, so that a swapped pair of entries cannot pass
    specs.append(dataclasses.replace(base, **{f: 1.0 + i for i, f in enumerate(
        ("delta", "g", "k1", "k2", "w_rate", "w_hw", "w_cxy", "w_cz_const", "w_foot", "w_force", "cz_max"))},
        box=(12.0, 13.0, 14.0), foot_length=15.0, foot_width=16.0, prox=17.0, relax=18.0))
    for s in specs:
        row = s.consts_row()
        assert row.shape == (18,) and row.dtype == np.float64
        assert np.array_equal(row, _c_row(lib, s)), (row, _c_row(lib, s))
    assert np.array_equal(specs[-1].consts_row(), np.arange(1.0, 19.0))


def test_const_fields_match_the_header():
    assert problem.NCONST == 18 and len(problem.CONST_FIELDS) == 18
    text = open(HEADER).read()
    assert int(re.search(r"#define CMPC_NCONST (\d+)", text).group(1)) == problem.NCONST
    assert header_const_fields(HEADER) == problem.CONST_FIELDS
    # ... and the documented row is the field order of the struct itself, from delta to relax
    body = text[text.index("typedef struct cmpc_spec {"):text.index("} cmpc_spec;")]
    fields = []
    for m in re.finditer(r"^\s*double\s+([^;]+);", body, re.M):
        for name in m.group(1).split(","):
            name = name.strip()
            mm = re.match(r"(\w+)\[(\d+)\]$", name)
            fields += [f"{mm.group(1)}[{j}]" for j in range(int(mm.group(2)))] if mm else [name]
    i = fields.index("delta")
    assert tuple(fields[i:i + problem.NCONST]) == problem.CONST_FIELDS
    assert fields[i + problem.NCONST:] == ["tol", "acc_tol"]
    # the ctypes mirror has the same order
    mirror = []
    for name, typ in CSpec._fields_:
        if typ is ctypes.c_double:
            mirror.append(name)
        elif name == "box":
            mirror += ["box[0]", "box[1]", "box[2]"]
    assert tuple(mirror[:problem.NCONST]) == problem.CONST_FIELDS


def test_consts_rows_stacks_and_refuses_mixed_shared_fields():
    base = ProblemSpec(N=10)
    over, specs = drawn_specs(base, 4)
    rows = problem.consts_rows(specs)
    assert rows.shape == (4, 18) and rows.dtype == np.float64 and rows.flags["C_CONTIGUOUS"]
    for r, s, o in zip(rows, specs, over):
        assert np.array_equal(r, s.consts_row())
        assert r[problem.CONST_FIELDS.index("k1")] == o["k1"] and r[problem.CONST_FIELDS.index("box[1]")] == o["box"][1]
        assert r[problem.CONST_FIELDS.index("delta")] == base.delta          # not drawn
    assert problem.consts_rows([]).shape == (0, 18)
    for field, value in (("N", 20), ("tol", 1e-6), ("nv", 8), ("max_iter", 50), ("acc_tol", 1e-3)):
        with pytest.raises(ValueError, match=field):
            problem.consts_rows([base, dataclasses.replace(base, **{field: value})])
    # what may differ, does: the three variants of the reference share a launch
    problem.consts_rows([base, dataclasses.replace(base, delta=0.1, k1=5.0, k2=0.2, w_rate=0.0), dataclasses.replace(base, k1=7.0, k2=1.0)])
