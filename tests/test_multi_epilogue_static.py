"""CPU tests of the set reductions of the shared sweep (sweep_body_multi, csrc/csmp_kernels.hpp) on tests/xsum_twin.py, the symbolic
twin of the lane moves: a set of four / of two leaves in the lanes of row q / half q EXACTLY wave_xsum's tree of additions over the
64 lanes of input q (so every c keeps the bits of the one-column bodies) and nothing of another input; the assignment of
(member, column) to the slots of the sets is pinned, and read out of the kernel's source; the kernels of the code object are the
frozen list of tests/test_sweep_plan_static.py (nothing added, nothing taken away), and the new code sits in the k_sweep_multi /
k_sweep_wide families alone.  The Float64 body (sweep_body_multi_w4) keeps its one wave_xsum per member: it has no set to check."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xsum_twin as xt  # noqa: E402
import test_sweep_plan_static as static  # noqa: E402

KERNELS = os.path.join(ROOT, "compressedsensing.jl_amd", "csrc", "csmp_kernels.hpp")


def source():
    with open(KERNELS) as f:
        return f.read()


def region(text, start, end):
    a = text.index(start)
    return text[a:text.index(end, a)]


def multi_body(text):
    """the shared Float32 pair body and its two kernels"""
    return region(text, "// Shared sweep: ONE pass over the dictionary", "// The shared sweep of round 7")


def test_twin_wave_xsum_is_the_xor_butterfly():
    """the twin's moves: wave_xsum is v += xor 32, 16, 8, 4, 2, 1, and every lane ends with the same tree"""
    v = xt.leaves("a")
    ref = list(v)
    for s in (32, 16, 8, 4, 2, 1):
        ref = [xt.add(ref[l], ref[l ^ s]) for l in range(xt.WAVE)]
    got = xt.wave_xsum(v)
    assert got == ref
    assert len(set(got)) == 1


def test_xs_steps_keep_their_inputs_apart():
    x, y = xt.leaves("x"), xt.leaves("y")
    a = xt.xs32(x, y)
    assert all(a[l] == xt.add(x[l], x[l + 32]) for l in range(32)) and all(a[l] == xt.add(y[l - 32], y[l]) for l in range(32, 64))
    b = xt.xs16(x, y)
    for l in range(64):
        v = (x, y)[(l >> 4) & 1]  # rows 0 and 2 keep x's pairs, rows 1 and 3 y's
        assert b[l] == xt.add(v[l & ~16], v[l | 16]), l


@pytest.mark.parametrize("nslots", [4, 2])
def test_a_set_leaves_wave_xsums_tree_of_slot_q_where_slot_q_ends(nslots):
    names = ["v%d" % q for q in range(nslots)]
    ins = [xt.leaves(n) for n in names]
    got = xt.set_of_four(*ins) if nslots == 4 else xt.set_of_two(*ins)
    want = [xt.wave_xsum(v)[0] for v in ins]  # (every lane of wave_xsum holds the same tree)
    for lane in range(xt.WAVE):
        q = xt.lane_slot(nslots, lane)
        assert got[lane] == want[q], (nslots, lane)
        assert xt.inputs_of(got[lane]) == {names[q]}, (nslots, lane)
    # a set fed ONE value four times / twice is the plain wave_xsum
    v = xt.leaves("a")
    assert (xt.set_of_four(v, v, v, v) if nslots == 4 else xt.set_of_two(v, v)) == xt.wave_xsum(v)


def test_slot_assignment_is_the_written_down_one():
    assert xt.set_slots(1) == [[(0, 0), (0, 1)]]
    assert xt.set_slots(2) == [[(0, 0), (0, 1), (1, 0), (1, 1)]]
    assert xt.set_slots(3) == [[(0, 0), (0, 1), (1, 0), (1, 1)], [(2, 0), (2, 1)]]
    assert xt.set_slots(4) == [[(0, 0), (0, 1), (1, 0), (1, 1)], [(2, 0), (2, 1), (3, 0), (3, 1)]]
    for R in (1, 2, 3, 4):  # every (member, column) once
        flat = [mc for s in xt.set_slots(R) for mc in s]
        assert sorted(flat) == [(i, j) for i in range(R) for j in (0, 1)]
    # ... and it is the one the body's expressions use: xs16(xs32(v0, v2), xs32(v1, v3)) and xs32(v0, v1) on acc[column][member]
    body = multi_body(source())
    acc = r"acc\[(\d)\]\[([^\]]+)\]"
    m = re.search(r"row_xsum\(xs16\(xs32\(%s, %s\), xs32\(%s, %s\)\)\)" % (acc, acc, acc, acc), body)
    assert m, "the set of four"
    g = m.groups()
    v0, v2, v1, v3 = [(g[2 * i + 1], int(g[2 * i])) for i in range(4)]
    assert [v0, v1, v2, v3] == [("2 * s", 0), ("2 * s", 1), ("2 * s + 1", 0), ("2 * s + 1", 1)]
    m = re.search(r"v = xs32\(%s, %s\);\s*v = row_xsum\(xs16\(v, v\)\);" % (acc, acc), body)
    assert m, "the set of two"
    assert [(m.group(2), int(m.group(1))), (m.group(4), int(m.group(3)))] == [("R - 1", 0), ("R - 1", 1)]
    # where slot q ends: the parity of the lane's column and the member whose c pointer a lane of a set of four takes
    assert "col = c0 + ((lane >> 4) & 1);" in body and "col = c0 + (lane >> 5);" in body
    assert "(lane & 32) ? cv(2 * s + 1) : cv(2 * s)" in body


def test_only_the_shared_float32_pass_changed_its_kernels():
    text = source()
    body = multi_body(text)
    rest = text.replace(body, "")
    # the set butterfly on accumulators, the unclamped loads and the instantiation flag are the shared Float32 body's alone
    for token in ("whole_base", "WHOLE", "cslot & 15"):
        assert token not in rest, token
    assert body.count("sweep_body_multi<TA, U, 2, R, ") == 4  # two instantiations under each of k_sweep_multi and k_sweep_wide
    assert body.count("__global__") == 2
    # the Float64 body keeps one wave_xsum per member and CStage, and CStage its two store forms
    w4 = region(text, "// The shared sweep of round 7", "// The append stages of two groups in ONE launch")
    assert "const double c = wave_xsum(acc[i]);" in w4 and "CStage<R> cs;" in w4
    cstage = region(text, "struct CStage {", "// ------")
    assert cstage.count("void flush(") == 2 and cstage.count("void put(") == 2
    # the code object: the frozen list of sweep-family kernels, no name more and none less
    lib = os.path.join(ROOT, "compressedsensing.jl_amd", "csrc", "libcsmp.so")
    if os.path.exists(lib) and shutil.which("nm"):
        out = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
        assert set(static.NAME.findall(out)) == static.frozen_names()
