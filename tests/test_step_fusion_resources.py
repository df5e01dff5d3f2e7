"""CPU tier, cross-compiled ISA: the one-wave 4-vertex kernels (plain and per-instance constants) that apply the Newton step
where the matrix sweep loads the iterate (Solver::STEP_FUSED, csrc/cmpc_kernel.hpp), against the same source built with
-DCMPC_SEPARATE_STEP (the step in a pass of its own, apply_step -- the kernels as they were).

  * registers, scratch and LDS are where the other resource tests pin them: the step lengths and the pending flag live in LDS
    words the map had to spare;
  * the stage loop of the matrix sweep (the innermost loop that holds the MFMA trailing update; loop nesting read from the
    compiler's loop comments) carries the step: at most five more global loads (dx, lam+, du, ds, dz of the stage's nodes) and
    five more stores (x, lam, u, s, z) than the separate build's -- and not one more full drain: the `s_waitcnt vmcnt(0)` of
    the loop are no more than the separate build has there.  (vmcnt counts stores too on gfx950: a load behind the five
    stores that waited for an empty queue would wait for them.)
  * and, local to the stage load: from the first of the five stores on, along every path of the kernel's control flow, no
    `s_waitcnt vmcnt(n)` of any n stands before the stage's next global loads are in flight -- a counted wait there waits
    for the stores' acknowledgements alone, one round trip after another.  The one full wait the fused build adds stands in
    front of the stores (CMPC_VM_LANDED), where the LDS commit has consumed every load and nothing is outstanding;
  * the separate pass is gone from the kernel: fewer global loads over the whole kernel than the separate build."""
import os
import re
import subprocess

import pytest

import build as _b

KERNELS = {"plain": "cmpc_solve_kernelILi4ELi1EEEvN4cmpc5KArgsEPiPKi", "consts": "cmpc_solve_consts_kernelILi4ELi1EEEvN4cmpc5KArgsEPKdPiPKi"}
STEP_WORDS = 5
NOTE = "cmpc: the step's stores"


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """(ISA of the default build, its resource remarks, ISA of the -DCMPC_SEPARATE_STEP build); the two compiles run side by side."""
    d = tmp_path_factory.mktemp("step_isa")
    src = os.path.join(_b.PKG, "csrc", "cmpc_hip.hip")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    jobs = [subprocess.Popen(cmd + flags + ["-o", str(d / name), src], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
            for name, flags in (("fused.s", []), ("separate.s", ["-DCMPC_SEPARATE_STEP"]))]
    errs = [j.communicate()[1] for j in jobs]
    for j, e in zip(jobs, errs):
        assert j.returncode == 0, e[-2000:]
    res, cur = {}, None
    for ln in errs[0].splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return (d / "fused.s").read_text(), res, (d / "separate.s").read_text()


def _body(isa, mangled):
    name = next(m for m in re.findall(r"^(\S*" + mangled + r"):", isa, flags=re.M))
    body = isa[isa.index(name + ":"):]
    return body[:body.index("s_endpgm")]


def _loops(body):
    """({loop header: parent loop header}, {innermost loop header or None: instructions}) from the compiler's loop comments."""
    return _loops_and_lines(body)[:2]


def _loops_and_lines(body):
    """_loops, and for every line of the body the header of the innermost loop it stands in (or None)."""
    parent, ins, cur, label, chain, where = {}, {}, None, None, [], []
    for ln in body.splitlines():
        where.append(None)
        m = re.match(r"^\.L(BB\d+_\d+):(.*)$", ln)
        if m:
            label, chain = m.group(1), []
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", m.group(2))
            cur = h.group(1) if h else None
        c = re.search(r";\s+Parent Loop (BB\d+_\d+) Depth=\d+", ln)
        if c:
            chain.append(c.group(1))
        if re.search(r"This (?:Inner )?Loop Header: Depth=\d+", ln):
            parent[label] = chain[-1] if chain else None
            cur = label
        s = ln.strip()
        if s and not s.startswith((";", ".")) and not re.match(r"^\S+:", ln):
            ins.setdefault(cur, []).append(re.sub(r"\s*;.*", "", s))
        where[-1] = cur
    return parent, ins, where


def _mfma_loop(parent, ins):
    """Header of the matrix sweep's stage loop: the innermost loop that holds the MFMA trailing update."""
    holders = {l for l, v in ins.items() if any(x.startswith("v_mfma") for x in v)}
    assert len(holders) == 1 and None not in holders, holders
    return holders.pop()


def _inside(l, top, parent):
    while l is not None and l != top:
        l = parent.get(l)
    return l == top


def _stage_loop(body):
    """Instructions of the matrix sweep's stage loop, nested loops included: the innermost loop that holds the MFMA update."""
    parent, ins = _loops(body)
    top = _mfma_loop(parent, ins)
    out = []
    for l, v in ins.items():
        if _inside(l, top, parent):
            out += v
    return out


def _n(lines, what):
    return sum(1 for x in lines if what in x)


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_registers_scratch_and_lds_are_where_they_were(builds, which):
    _, res, _ = builds
    r = next(v for k, v in res.items() if KERNELS[which] in k)
    print(which, r)
    assert r["ScratchSize"] == 0 and r["LDS Size"] == 22936 and r["AGPRs"] == 0
    assert r["VGPRs"] == 256 if which == "plain" else r["VGPRs"] <= 256


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_the_stage_loop_carries_the_step_without_a_new_full_drain(builds, which):
    fused, _, separate = builds
    new, old = _stage_loop(_body(fused, KERNELS[which])), _stage_loop(_body(separate, KERNELS[which]))
    count = {k: (_n(new, k), _n(old, k)) for k in ("global_load", "global_store", "vmcnt(0)", "scratch_")}
    print(which, "stage loop of the matrix sweep, fused / separate:", count)
    assert 0 < count["global_load"][0] - count["global_load"][1] <= STEP_WORDS
    assert 0 < count["global_store"][0] - count["global_store"][1] <= STEP_WORDS
    assert count["vmcnt(0)"][0] <= count["vmcnt(0)"][1]
    assert count["scratch_"] == (0, 0)


def _behind_the_step_stores(body):
    """Walks the kernel's control flow from the note the source leaves at the top of the step's stores (CMPC_ASM_NOTE in
    load_stage), along every path, to the first wait on the vector-memory counter -- or to where the path leaves the stage
    loop, or reaches a sixth store, which belongs to the code behind the loader.  Returns (the waits reached before any
    global load was issued -- each would wait for stores alone --, the most stores a path issues before its first load)."""
    lines = body.splitlines()
    label_at = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label_at[m.group(1)] = i
    # (the loader is inlined twice: in the stage loop of the matrix sweep, which is meant, and in finish_step, the rare exit
    # of an attempt whose factorisation has failed for good, which ends with a full fence)
    parent, ins, where = _loops_and_lines(body)
    top = _mfma_loop(parent, ins)
    starts = [i for i, ln in enumerate(lines) if NOTE in ln and _inside(where[i], top, parent)]
    assert len(starts) == 1, starts
    bad, most, seen, todo = [], 0, set(), [(starts[0] + 1, 0, False)]
    while todo:
        i, stores, loaded = todo.pop()
        while i < len(lines) and (i, stores, loaded) not in seen:
            seen.add((i, stores, loaded))
            if not _inside(where[i], top, parent):                # (the sweep is left: a factorisation that failed)
                break
            s = re.sub(r"\s*;.*", "", lines[i]).strip()
            i += 1
            if s.startswith("s_waitcnt") and "vmcnt(" in s:
                if not loaded:
                    bad.append("line %d of the kernel: %s" % (i, s))
                break
            if s.startswith("global_load"):
                loaded = True
            elif s.startswith("global_store") and not loaded:
                if stores == STEP_WORDS:                          # (a store of the code behind the loader: the five are long out)
                    break
                stores += 1
                most = max(most, stores)
            elif s.startswith("s_cbranch") or s.startswith("s_branch"):
                to = label_at.get(s.split()[-1])
                if s.startswith("s_branch"):
                    if to is None:
                        break
                    i = to
                elif to is not None:
                    todo.append((to, stores, loaded))
            elif s.startswith(("s_endpgm", "s_setpc", "s_swappc")):
                break
    return sorted(set(bad)), most


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_nothing_waits_for_the_step_stores_alone(builds, which):
    """vmcnt counts stores too on gfx950, and the compiler plans its waits for a counter that runs in order: a counted wait
    between the five stores, or behind them before the stage's next loads are in flight, waits at run time for the stores'
    acknowledgements -- round trips in the stage's serial path.  From the first store on, along every path of the kernel's
    control flow, the first `s_waitcnt vmcnt(n)`, whatever n, comes behind a global load: it is that load's wait, and the
    stores ride along with it.  (The `s_waitcnt vmcnt(0)` the source puts in front of the stores, CMPC_VM_LANDED, is ahead
    of this walk: it stands where the LDS commit has consumed every load, and is what lets the compiler plan so.)"""
    fused, _, _ = builds
    bad, most = _behind_the_step_stores(_body(fused, KERNELS[which]))
    print(which, "stores issued back to back:", most, "waits for stores alone:", bad)
    assert most == STEP_WORDS
    assert bad == []


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_the_separate_pass_is_gone_from_the_kernel(builds, which):
    fused, _, separate = builds
    new, old = _body(fused, KERNELS[which]), _body(separate, KERNELS[which])
    n_new, n_old = (sum(ln.strip().startswith("global_load") for ln in b.splitlines()) for b in (new, old))
    print(which, "global loads", n_new, "with the separate pass", n_old)
    assert n_new < n_old
