"""The lockstep schedule of csmp_bp_batch (host/bp_batch_plan.hpp: bp_lockstep) against a Python restatement of its rules: a small
program of its own, built from the header alone under AddressSanitizer and UBSan, prints every entry, every step's member list, every
check and every retirement for groups of 1, 2, 3, 4 and 8 slots, 1 .. 20 signals, check_every 1, 7, 32 and maxiter 0, 50, 96, 100.
Signal s converges at its check number MULT[s] (iteration MULT[s] * check_every), or never."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compressedsensing.jl_amd", "csrc")
RS = (1, 2, 3, 4, 8)
NSIGS = range(1, 21)
CHECKS = (1, 7, 32)
MAXITERS = (0, 50, 96, 100)
MULT = (1, 3, 0, 2, 1, 5, 2, 0, 4, 1, 3, 3, 1, 0, 2, 6, 1, 2, 4, 1)  # 0: never

PROGRAM = r"""
#include "host/bp_batch_plan.hpp"
#include <cstdio>
static const int MULT[20] = {%s};
struct Hooks {
    long ce;
    long sig[kBpPlanMaxMembers], it[kBpPlanMaxMembers];
    int enter(int slot, int64_t s) { sig[slot] = (long)s; it[slot] = 0; std::printf("E %%d %%ld\n", slot, (long)s); return 0; }
    int step(const int* slots, int n) {
        std::printf("S");
        for (int i = 0; i < n; ++i) { std::printf(" %%d", slots[i]); it[slots[i]] += 1; }
        std::printf("\n");
        return 0;
    }
    int check(const int* slots, int n, bool* conv) {
        std::printf("C");
        for (int i = 0; i < n; ++i) {
            const long T = MULT[sig[slots[i]]] * ce;
            conv[i] = T > 0 && it[slots[i]] == T;
            std::printf(" %%d:%%ld", slots[i], it[slots[i]]);
        }
        std::printf("\n");
        return 0;
    }
    int retire(const BpPlanRetired* who, int n) {
        for (int i = 0; i < n; ++i) std::printf("R %%d %%ld %%ld %%d\n", who[i].slot, (long)who[i].sig, (long)who[i].iterations, who[i].converged ? 1 : 0);
        return 0;
    }
};
int main() {
    const int Rs[] = {%s};
    const long ces[] = {%s}, mis[] = {%s};
    for (int R : Rs)
        for (long nsig = 1; nsig <= 20; ++nsig)
            for (long ce : ces)
                for (long mi : mis) {
                    std::printf("P %%d %%ld %%ld %%ld\n", R, nsig, ce, mi);
                    Hooks h{};
                    h.ce = ce;
                    if (bp_lockstep(R, nsig, mi, ce, h) != 0) return 1;
                }
    Hooks h{};
    h.ce = 1;
    if (bp_lockstep(0, 1, 1, 1, h) != -1 || bp_lockstep(kBpPlanMaxMembers + 1, 1, 1, 1, h) != -1 || bp_lockstep(1, 1, 1, 0, h) != -1) return 2;
    return 0;
}
""" % (", ".join(map(str, MULT)), ", ".join(map(str, RS)), ", ".join(map(str, CHECKS)), ", ".join(map(str, MAXITERS)))


def rules(R, nsig, ce, maxiter):
    """section 2 of the issue, restated: the lines the program prints for one plan"""
    out = []
    slot = [None] * R  # [signal, iterations]
    nxt = done = 0
    while done < nsig:
        for m in range(R):                       # signals enter the lowest free slot in ascending order
            if slot[m] is None and nxt < nsig:
                slot[m] = [nxt, 0]
                out.append(f"E {m} {nxt}")
                nxt += 1
        cnt = [None if s is None else min(ce, maxiter - s[1]) for s in slot]
        for j in range(max(c for c in cnt if c is not None)):
            out.append("S" + "".join(f" {m}" for m in range(R) if cnt[m] is not None and cnt[m] > j))
        conv = [False] * R
        checked = []
        for m in range(R):
            if slot[m] is not None:
                slot[m][1] += cnt[m]
                if cnt[m] == ce:                 # a member that reaches maxiter inside an interval is not checked
                    checked.append(m)
        if checked:
            out.append("C" + "".join(f" {m}:{slot[m][1]}" for m in checked))
            for m in checked:
                conv[m] = MULT[slot[m][0]] > 0 and slot[m][1] == MULT[slot[m][0]] * ce
        for m in range(R):
            if slot[m] is not None and (conv[m] or slot[m][1] >= maxiter):
                out.append(f"R {m} {slot[m][0]} {slot[m][1]} {int(conv[m])}")
                slot[m] = None
                done += 1
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the plan printer"
    d = tmp_path_factory.mktemp("bp_plan")
    src, exe = d / "bp_plan_print.cpp", d / "bp_plan_print"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got, cur = {}, None
    for line in out:
        if line[0] == "P":
            cur = got.setdefault(tuple(int(x) for x in line.split()[1:]), [])
        else:
            cur.append(line)
    return got


def test_the_header_is_plain_cxx():
    src = open(os.path.join(CSRC, "host", "bp_batch_plan.hpp")).read()
    assert [ln for ln in src.splitlines() if ln.startswith("#include")] == ["#include <cstdint>"]
    assert "__global__" not in src and "hipLaunch" not in src and "hipStream" not in src


def test_every_plan_line_by_line(printed):
    assert len(printed) == len(RS) * len(NSIGS) * len(CHECKS) * len(MAXITERS)
    for key, lines in printed.items():
        assert lines == rules(*key), key


def test_properties_of_every_plan(printed):
    for (R, nsig, ce, maxiter), lines in printed.items():
        key = (R, nsig, ce, maxiter)
        slot = {}            # slot -> signal
        its = {}             # signal -> iterations run
        entered, retired = [], {}
        for line in lines:
            kind, rest = line[0], line[1:].split()
            if kind == "E":
                m, s = int(rest[0]), int(rest[1])
                assert m not in slot, key                          # a slot never holds two signals
                assert m == min(set(range(R)) - set(slot)), key    # the lowest free slot
                slot[m] = s
                its[s] = 0
                entered.append(s)
            elif kind == "S":
                live = [int(x) for x in rest]
                assert live == sorted(live) and 1 <= len(live) <= R and all(m in slot for m in live), key
                for m in live:
                    its[slot[m]] += 1
            elif kind == "C":
                for item in rest:
                    m, it = (int(x) for x in item.split(":"))
                    assert its[slot[m]] == it and it % ce == 0 and it > 0, key   # checks at multiples of check_every of its own count
            else:
                m, s, it, conv = (int(x) for x in rest)
                assert slot.pop(m) == s and its[s] == it, key
                retired[s] = (it, conv)
            assert len(slot) <= R, key
        assert entered == list(range(nsig)), key                   # ascending order, every signal once
        assert not slot and sorted(retired) == list(range(nsig)), key
        for s, (it, conv) in retired.items():
            T = MULT[s] * ce if MULT[s] > 0 else None
            reach = T is not None and T <= maxiter
            assert it == (T if reach else maxiter) and conv == int(reach), (key, s)   # exactly min(T_s, maxiter) iterations
