"""CPU tests of tests/sweep_plan.py, the Python twin of the host dispatch of the product sweeps.

Config check: the twin gives the phases and the documented unit choices test_gpu_shapes.py asserts on its SWEEP_SHAPES.
Coverage check: the kernels the case tables of tests/test_gpu_sweep_matrix.py reach, per the twin, against the sweep-family kernel
NAMES of the code object (names only, no instructions).  The name list is frozen HERE (frozen_names(): 104 names, written out as
the explicit instantiations of csmp_kernels.hpp / csmp_forward.hpp and checked once against `nm -C libcsmp.so` and against the
per-kernel lines of profiles/r12_sweep_parts.txt); where the built library and binutils' nm are at hand the test also checks the list
against the library's own symbols, so a kernel added to or taken from the code object fails it."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_plan as sp  # noqa: E402
import test_gpu_shapes as shapes  # noqa: E402
import test_gpu_sweep_matrix as matrix  # noqa: E402

FAMILIES = ("k_sweep_gen", "k_sweep_short", "k_sweep_ph", "k_sweep_dyn", "k_sweep_multi", "k_sweep_multi_w4", "k_sweep_wide", "k_tick",
            "k_fr_sweep", "k_tick_fr")
NAME = re.compile(r"csmp::((?:%s)<[^>]*>)" % "|".join(FAMILIES))

# kernels of the code object that no case table reaches, each with the reason (checkable in the host code)
UNREACHED = {}
for _r in (1, 2, 3, 4):
    UNREACHED["k_sweep_wide<float, 4, %d, true>" % _r] = (
        "nontemporal ring loads: the scheduler runs kWideNt = false (host/omp.hpp:201); only csmp_bench_sweep's variants launch NT = true")
for _r in (1, 2):
    UNREACHED["k_sweep_wide<float, 4, %d, false>" % _r] = (
        "a wide pass serves 5 .. 8 members and R is its larger half, (size + 1) / 2 >= 3 (multi_members, host/omp.hpp:211-213); "
        "R = 1, 2 are launched by csmp_bench_sweep alone")


def frozen_names():
    """the 104 sweep-family kernels of the code object, family by family"""
    tas, units, tf = ("float", "double"), (4, 8, 16), ("false", "true")
    names = []
    for ta in tas:
        for fam in ("k_sweep_gen", "k_sweep_dyn"):  # <TA, U, NB>: a ring of 32 chunks
            names += ["%s<%s, %d, %d>" % (fam, ta, u, 32 // u) for u in units]
        names += ["k_sweep_short<%s, %s>" % (ta, nch_cpu) for nch_cpu in ("1, 4", "2, 4", "4, 2")]  # <TA, NCH, CPU>
        names.append("k_sweep_ph<%s, 8, 4>" % ta)
        # k_tick<TA, U, PH, STEADY, DYN>: every unit static and dynamic, phases on 8-load units and never dynamic
        names += ["k_tick<%s, %d, false, %s, %s>" % (ta, u, steady, dyn) for u in units for steady in tf for dyn in tf]
        names += ["k_tick<%s, 8, true, %s, false>" % (ta, steady) for steady in tf]
        names += ["k_fr_sweep<%s, %s, %d>" % (ta, blk, nq) for blk in ("16, true", "8, true", "4, false") for nq in (-1, 0, 1, 2)]
        names += ["k_tick_fr<%s, %d, %d>" % (ta, u, nq) for u in (8, 16) for nq in (-1, 1)]
    names += ["k_sweep_multi<float, 4, %d>" % r for r in (1, 2, 3, 4)]
    names += ["k_sweep_multi_w4<double, %d, %d>" % (u, r) for u in units for r in (1, 2, 3, 4)]
    names += ["k_sweep_wide<float, 4, %d, %s>" % (r, nt) for r in (1, 2, 3, 4) for nt in tf]
    assert len(names) == len(set(names))
    return set(names)


def test_twin_reproduces_the_documented_configurations():
    for M, N in shapes.SWEEP_SHAPES:
        for dtype in (np.float32, np.float64):
            cfg = sp.plan(M, N, dtype, 256).config()
            assert cfg["phases"] == (1 if M <= 20000 else 2 if M <= 36000 else 3), (M, N, dtype, cfg)
    # the documented unit choices (host/dictionary.hpp:139-141: the unit that pads the column's chunks least, the larger on a tie)
    assert sp.plan(4352, 260, np.float32, 256).sweep_U == 4   # 17 chunks: 20 under 4-load units, 24 under 8, 32 under 16
    assert sp.plan(4096, 130, np.float32, 256).sweep_U == 16  # 16 chunks: no padding under any unit, the largest wins
    assert sp.plan(4096, 130, np.float64, 256).sweep_U == 16
    assert sp.plan(3000, 515, np.float32, 256).sweep_U == 4   # 12 chunks: 12 / 16 / 16
    # the bodies: short columns, phases, the dynamic split on request only
    assert sp.plan(256, 4096, np.float32, 256).sweep() == ("k_sweep_short", "float", 1, 4)
    assert sp.plan(512, 2048, np.float32, 256).sweep() == ("k_sweep_short", "float", 2, 4)
    assert sp.plan(200, 1021, np.float64, 256).sweep() == ("k_sweep_short", "double", 2, 4)
    assert sp.plan(1000, 700, np.float32, 256).sweep() == ("k_sweep_short", "float", 4, 2)
    assert sp.plan(32, 48, np.float32, 256, {"sweep_short": 1}).sweep()[0] == "k_sweep_gen"
    assert sp.plan(32, 5, np.float32, 256).sweep()[0] == "k_sweep_gen"  # (fewer than eight columns: never short)
    assert sp.plan(32768, 96, np.float32, 256).sweep() == ("k_sweep_ph", "float", 8, 4)
    assert sp.plan(4096, 130, np.float32, 256, {"sweep_dyn": 1}).sweep() == ("k_sweep_dyn", "float", 16, 2)
    # groups: four images at 4096 rows, wide groups on Float32 only
    assert sp.plan(4096, 6000, np.float32, 256).config()["group_wide"] == 8
    assert sp.plan(4096, 6000, np.float64, 256).config()["group_wide"] == 4
    assert sp.plan(32768, 96, np.float32, 256).sweep_group == 0


def test_column_maps_partition_the_columns():
    for body, nch in (("gen", 0), ("multi", 0), ("multi_w4", 0), ("short", 1), ("short", 2), ("short", 4)):
        for N in (1, 3, 5, 257, 259, 1033):
            for nblk in (1, 2, 3):
                waves = 8 if body == "multi" else 4
                seen = []
                for b in range(nblk):
                    for w in range(waves):
                        cols = sp.wave_columns(body, b, w, N, nblk, nch)
                        assert cols == sorted(cols)
                        for pos, c in enumerate(cols):
                            assert sp.column_owner(body, c, nblk, nch)[:3] == (b, w, pos), (body, nch, N, nblk, c)
                        seen += cols
                assert sorted(seen) == list(range(N)), (body, nch, N, nblk)


def test_case_tables_reach_every_sweep_kernel():
    names = frozen_names()
    assert len(names) == 104
    lib = os.path.join(ROOT, "compressedsensing.jl_amd", "csrc", "libcsmp.so")
    if os.path.exists(lib) and shutil.which("nm"):
        out = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
        assert set(NAME.findall(out)) == names
    got = matrix.reached()
    assert got <= names, sorted(got - names)
    assert not (set(UNREACHED) & got), sorted(set(UNREACHED) & got)
    assert set(UNREACHED) <= names, sorted(set(UNREACHED) - names)
    missing = names - got - set(UNREACHED)
    assert not missing, sorted(missing)
    assert all(len(reason) > 20 for reason in UNREACHED.values())
