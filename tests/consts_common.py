"""Shared by the tests of the per-instance constants (cmpc_solve_batch_consts): the draw of the rows and small helpers.
Not a test module."""
import dataclasses

import numpy as np

DRAW_SEED = 4711


def draw_overrides(spec, B, seed=DRAW_SEED):
    """One dict of spec overrides per instance (numpy.random.default_rng(seed), drawn instance by instance):
    k1 in [3, 7], k2 in [0.1, 1]; the six weights, each the spec's value times [0.5, 2]; cz_max in [0.76, 0.80];
    foot_length, foot_width, each the spec's times [0.8, 1.2]; box, the spec's times one factor in [0.5, 2];
    g in [9.78, 9.83].  delta, prox and relax are not drawn."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(B):
        o = dict(k1=rng.uniform(3.0, 7.0), k2=rng.uniform(0.1, 1.0))
        for w in ("w_hw", "w_cxy", "w_cz_const", "w_foot", "w_force", "w_rate"):
            o[w] = getattr(spec, w) * rng.uniform(0.5, 2.0)
        o["cz_max"] = rng.uniform(0.76, 0.80)
        o["foot_length"] = spec.foot_length * rng.uniform(0.8, 1.2)
        o["foot_width"] = spec.foot_width * rng.uniform(0.8, 1.2)
        f = rng.uniform(0.5, 2.0)
        o["box"] = tuple(float(b) * f for b in spec.box)
        o["g"] = rng.uniform(9.78, 9.83)
        rows.append({k: (v if k == "box" else float(v)) for k, v in o.items()})
    return rows


def drawn_specs(spec, B, seed=DRAW_SEED):
    """(overrides, specs): the draw, and the ProblemSpec of every instance."""
    over = draw_overrides(spec, B, seed)
    return over, [dataclasses.replace(spec, **o) for o in over]


def uniform_rows(spec, B):
    return np.ascontiguousarray(np.tile(spec.consts_row(), (B, 1)))


def header_const_fields(path):
    """The row layout as include/cmpc.h documents it: the `[i] name` entries of the cmpc_solve_batch_consts comment."""
    import re
    text = open(path).read()
    block = text[text.index("consts  [B][CMPC_NCONST]"):text.index("#define CMPC_NCONST")]
    names = []
    for m in re.finditer(r"\[(\d+)(?:\.\.(\d+))?\]\s+([a-z_0-9]+)(\[3\])?", block):
        lo, hi, name = int(m.group(1)), m.group(2), m.group(3)
        if hi is None:
            names.append((lo, name))
        else:
            names += [(lo + j, f"{name}[{j}]") for j in range(int(hi) - lo + 1)]
    names.sort()
    assert [i for i, _ in names] == list(range(len(names))), names
    return tuple(n for _, n in names)
