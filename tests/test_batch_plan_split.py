"""The split rule of the grouped schedule (host/batch_plan.hpp: narrow_last_groups, batch_plan) against a Python restatement: a small
program of its own, built from the header alone under AddressSanitizer and UBSan, prints every plan of 1 .. 64 signals for passes of
1, 2, 3, 4 and 8 members, with the rule (group_split 0) and with the even split (group_split 1)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compressedsensing.jl_amd", "csrc")
RS = (1, 2, 3, 4, 8)
NARROW = 4   # kGroupMax: the members of a narrow pass, a half of a wide one
KSLOTS = 24  # kSlots (host/ctx.hpp): member m of group g is solver slot g + 3 m

PROGRAM = r"""
#include "host/batch_plan.hpp"
#include <cstdio>
int main() {
    const int Rs[] = {1, 2, 3, 4, 8};
    for (int R : Rs)
        for (int split = 0; split < 2; ++split)
            for (long nsig = 1; nsig <= 64; ++nsig) {
                const std::vector<PlanRound> plan = batch_plan(nsig, BatchSchedule::Grouped, R, false, 4, split);
                for (size_t j = 0; j < plan.size(); ++j)
                    for (int i = 0; i < 6; ++i) {  // the order the groups are dealt in: A, B, A, B, ...
                        const PlanGroup& g = plan[j].g[i % 2][i / 2];
                        if (g.size > 0) std::printf("%d %d %ld %zu %d %d %ld %d\n", R, split, nsig, j, i % 2, i / 2, (long)g.first, g.size);
                    }
            }
    const std::vector<PlanGroup> e = even_groups(18, 8), n = narrow_last_groups(18, 8, 4);
    std::printf("even18 %d %d %d narrow18 %d %d %d\n", e[0].size, e[1].size, e[2].size, n[0].size, n[1].size, n[2].size);
    return 0;
}
"""


def even(nsig, R):
    p = -(-nsig // R)
    return [nsig // p + (1 if i < nsig % p else 0) for i in range(p)]


def rule(nsig, R, split):
    """the sizes of the groups: R <= 4 and group_split 1 the even split; else a last group of four where that takes no pass more"""
    p = -(-nsig // R)
    if R <= NARROW or split == 1 or p < 2 or nsig > R * (p - 1) + NARROW:
        return even(nsig, R)
    rest = nsig - NARROW
    return [R] * (rest // R) + ([rest % R] if rest % R else []) + [NARROW]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the plan printer"
    d = tmp_path_factory.mktemp("plan")
    src, exe = d / "plan_print.cpp", d / "plan_print"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {}
    for line in out[:-1]:
        R, split, nsig, rnd, pipe, grp, first, size = (int(x) for x in line.split())
        got.setdefault((R, split, nsig), []).append((rnd, pipe, grp, first, size))
    return got, out[-1]


def test_python_rule_gives_the_named_sizes():
    assert rule(9, 8, 0) == [5, 4] and rule(10, 8, 0) == [6, 4] and rule(12, 8, 0) == [8, 4]
    assert rule(17, 8, 0) == [8, 5, 4] and rule(18, 8, 0) == [8, 6, 4] and rule(20, 8, 0) == [8, 8, 4]
    for nsig in (13, 14, 16, 21, 24):
        assert rule(nsig, 8, 0) == even(nsig, 8), nsig
    for nsig in range(5, 9):
        assert rule(nsig, 8, 0) == [nsig]
    assert rule(18, 8, 1) == [6, 6, 6] and rule(20, 8, 1) == [7, 7, 6]


def test_every_plan(plans):
    got, last = plans
    assert last == "even18 6 6 6 narrow18 8 6 4"
    for R in RS:
        for split in (0, 1):
            for nsig in range(1, 65):
                groups = got[(R, split, nsig)]
                want = rule(nsig, R, split)
                assert [g[4] for g in groups] == want, (R, split, nsig)
                assert len(groups) == -(-nsig // R)                      # the fewest passes
                at = 0
                for i, (rnd, pipe, grp, first, size) in enumerate(groups):
                    assert first == at and 1 <= size <= R                # consecutive runs, every signal once, none above R
                    assert (rnd, pipe, grp) == (i // 6, i % 2, (i % 6) // 2)  # dealt six to a round, A, B, A, B, ...
                    assert grp + 3 * (size - 1) < KSLOTS
                    at += size
                assert at == nsig
                assert all(a >= b for a, b in zip(want, want[1:]))       # the larger first
                if R <= NARROW or split == 1:
                    assert want == even(nsig, R)
                elif want != even(nsig, R):                              # the rule: a narrow pass last, wide ones before it
                    assert want[-1] == NARROW and all(s > NARROW for s in want[:-1])
