// host/bp_batch_plan.hpp -- the lockstep schedule of csmp_bp_batch (host/bp_batch.hpp) as one loop over callbacks.  Plain C++, no
// HIP: included by csmp.hip (the library) and, alone, by the program tests/test_bp_batch_plan.py builds, which prints every launch list
// and every retirement of the schedules a batch can get.
//
// Up to R members -- solves of csmp_bp that end at different iterations -- share their launches:
//   entry      the signals enter the LOWEST free slot in ascending order, at interval boundaries only
//   interval   member m runs cnt_m = min(check_every, maxiter - it_m) iterations
//   step j     of an interval launches the members with cnt_m > j, in slot order (ONE call of step)
//   check      at the interval's end the members with cnt_m == check_every are checked together (ONE call of check): a member's checks
//              fall on the multiples of check_every of its OWN count, as csmp_bp's do; a member that reaches maxiter inside an
//              interval is not checked, as bp_iterate's loop ends
//   retire     a member that converged or has reached maxiter leaves (ONE call of retire for all of an interval); its slot is free
//              for the next signal.  maxiter == 0: every signal enters, runs nothing and retires unconverged.
// Nothing here knows what an iteration is: csmp_bpd's or any other ADMM loop with a periodic test fits the same callbacks.
#pragma once
#include <cstdint>

constexpr int kBpPlanMaxMembers = 8;  // slots of a group (kWideMax, csmp_kernels.hpp: the members one wide pass serves)

struct BpPlanMember {
    int64_t sig = -1;  // the signal in the slot, -1: free
    int64_t it = 0;    // iterations it has run
    int64_t cnt = 0;   // ... and runs in the current interval
};
struct BpPlanRetired {
    int slot;
    int64_t sig, iterations;
    bool converged;
};

// H: int enter(int slot, int64_t sig);  int step(const int* slots, int n);  int check(const int* slots, int n, bool* converged);
//    int retire(const BpPlanRetired* who, int n).  A non-zero return ends the loop and is returned.  -1: R out of range.
template <typename H>
static int bp_lockstep(int R, int64_t nsig, int64_t maxiter, int64_t check_every, H& h) {
    if (R < 1 || R > kBpPlanMaxMembers || check_every < 1 || maxiter < 0) return -1;
    BpPlanMember mem[kBpPlanMaxMembers];
    int64_t next = 0, done = 0;
    while (done < nsig) {
        for (int m = 0; m < R && next < nsig; ++m)
            if (mem[m].sig < 0) {
                mem[m].sig = next++;
                mem[m].it = 0;
                const int rc = h.enter(m, mem[m].sig);
                if (rc != 0) return rc;
            }
        int64_t steps = 0;
        for (int m = 0; m < R; ++m) {
            if (mem[m].sig < 0) continue;
            mem[m].cnt = maxiter - mem[m].it < check_every ? maxiter - mem[m].it : check_every;
            if (mem[m].cnt > steps) steps = mem[m].cnt;
        }
        int list[kBpPlanMaxMembers];
        for (int64_t j = 0; j < steps; ++j) {
            int n = 0;
            for (int m = 0; m < R; ++m)
                if (mem[m].sig >= 0 && mem[m].cnt > j) list[n++] = m;
            const int rc = h.step(list, n);
            if (rc != 0) return rc;
        }
        bool conv[kBpPlanMaxMembers] = {};
        int nchk = 0;
        for (int m = 0; m < R; ++m) {
            if (mem[m].sig < 0) continue;
            mem[m].it += mem[m].cnt;
            if (mem[m].cnt == check_every) list[nchk++] = m;
        }
        if (nchk > 0) {
            bool got[kBpPlanMaxMembers] = {};
            const int rc = h.check(list, nchk, got);
            if (rc != 0) return rc;
            for (int i = 0; i < nchk; ++i) conv[list[i]] = got[i];
        }
        BpPlanRetired out[kBpPlanMaxMembers];
        int nret = 0;
        for (int m = 0; m < R; ++m)
            if (mem[m].sig >= 0 && (conv[m] || mem[m].it >= maxiter)) out[nret++] = {m, mem[m].sig, mem[m].it, conv[m]};
        if (nret > 0) {
            const int rc = h.retire(out, nret);
            if (rc != 0) return rc;
            for (int i = 0; i < nret; ++i) mem[out[i].slot] = BpPlanMember();
            done += nret;
        }
    }
    return 0;
}
