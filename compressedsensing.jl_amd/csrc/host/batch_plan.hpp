// host/batch_plan.hpp -- the schedules of csmp_omp_batch / csmp_fr_batch as data: the stage rotation of a tick pipeline and the
// rounds a batch runs in (host/forward.hpp: batch_impl).  Plain C++, no HIP: included by csmp.hip (the library) and, alone, by
// tools/sanitize/hostonly_driver.cpp, which checks every plan a batch of up to 64 signals can get.
#pragma once
#include <cstdint>
#include <vector>

// A pipeline holds three groups of signals (a group of the grouped schedule has up to sweep_group members -- with wide groups up to
// group_wide = 2 * sweep_group, swept as two halves --, every other schedule's one or none).  At tick n group n % 3 sweeps, group (n + 2) % 3 runs its k_qr1 stage and group (n + 1) % 3 its k_qr2 stage: every
// signal's chain -- sweep, qr1, qr2 in three consecutive ticks -- takes one step in three ticks, k steps in 3k + 2 ticks.
struct TickStages {
    int z, y, x;       // the sweep, qr1 and qr2 groups
    bool az, ay, ax;   // ... whether each is live (a group of size 0 never is)
    int64_t tz;        // the sweep's step
};
static TickStages tick_stages(int64_t n, int64_t k, const int size[3]) {
    TickStages t;
    t.z = (int)(n % 3);
    t.y = (int)((n + 2) % 3);
    t.x = (int)((n + 1) % 3);
    t.tz = (n - t.z) / 3;
    t.az = size[t.z] > 0 && t.tz < k;
    t.ay = size[t.y] > 0 && n >= 1 + t.y && (n - 1 - t.y) / 3 < k;
    t.ax = size[t.x] > 0 && n >= 2 + t.x && (n - 2 - t.x) / 3 < k;
    return t;
}

enum class BatchSchedule {
    Signals,  // no pipeline: one signal after the other
    One,      // one pipeline of three signals
    Pairs,    // two pipelines side by side, the second on a twin context
    Grouped,  // two pipelines of three groups whose members share one sweep
};
enum class RoundForm { One, Pair, Grouped };  // how a round's ticks are launched
struct PlanGroup {
    int64_t first = 0;  // the group's first signal; its members are the signals first .. first + size - 1
    int size = 0;
};
struct PlanRound {
    RoundForm form = RoundForm::One;
    PlanGroup g[2][3];  // [pipeline: 0 = A, the caller's context; 1 = B, the twin][group]; member m of group g is solver slot g + 3 m
};

// The fewest shared passes for nsig signals, R to a pass at the most: ceil(nsig / R) groups of consecutive signals, their sizes as
// even as possible, the larger ones first
static std::vector<PlanGroup> even_groups(int64_t nsig, int R) {
    std::vector<PlanGroup> groups;
    if (nsig < 1 || R < 1) return groups;
    const int64_t ngroups = (nsig + R - 1) / R, base = nsig / ngroups, extra = nsig % ngroups;
    int64_t at = 0;
    for (int64_t i = 0; i < ngroups; ++i) {
        groups.push_back({at, (int)(base + (i < extra ? 1 : 0))});
        at += groups.back().size;
    }
    return groups;
}

// The rounds of a batch of nsig signals (R: the members a shared pass serves, ctx->sweep_group or ctx->group_wide).  Pairs: rounds of 3 + 3 while six or
// more signals remain, then 1 + 1, then a lone signal in the one-pipeline form.  Grouped: the fewest shared passes (even_groups)
// dealt six to a round, even offsets to A and odd ones to B; a last round may leave B with no group and keeps the pair form.
static std::vector<PlanRound> batch_plan(int64_t nsig, BatchSchedule sched, int R, bool one_pipe = false) {
    std::vector<PlanRound> rounds;
    auto round = [&](RoundForm form) -> PlanRound& {
        rounds.emplace_back();
        rounds.back().form = form;
        return rounds.back();
    };
    int64_t at = 0;
    switch (sched) {
        case BatchSchedule::Signals: break;
        case BatchSchedule::One:
            for (; at < nsig; at += 3) {
                PlanRound& r = round(RoundForm::One);
                for (int g = 0; g < 3 && at + g < nsig; ++g) r.g[0][g] = {at + g, 1};
            }
            break;
        case BatchSchedule::Pairs:
            // measured on the 1-GiB dictionary, atoms/s of a whole batch -- 3 + 3: 6680, 1 + 1: 6690, 2 + 2: 6486, and the rounds whose
            // pipelines hold different numbers 3 + 2: 6340, 2 + 1: 6332 (one pipeline of three: 6306, a lone signal: 5830;
            // tools/probes/few_signals.sh).  Two streams with a sweep ready each keep the HBM busy; what costs is a round in which one
            // stream's ticks have sweeps the other's have not.
            for (; nsig - at >= 6; at += 6) {
                PlanRound& r = round(RoundForm::Pair);
                for (int g = 0; g < 3; ++g) {
                    r.g[0][g] = {at + g, 1};
                    r.g[1][g] = {at + 3 + g, 1};
                }
            }
            for (; nsig - at >= 2; at += 2) {
                PlanRound& r = round(RoundForm::Pair);
                r.g[0][0] = {at, 1};
                r.g[1][0] = {at + 1, 1};
            }
            if (at < nsig) round(RoundForm::One).g[0][0] = {at, 1};
            break;
        case BatchSchedule::Grouped: {
            const std::vector<PlanGroup> groups = even_groups(nsig, R);
            for (size_t i = 0; i < groups.size(); ++i) {
                const size_t per = one_pipe ? 3 : 6;  // (one_pipe, a measurement: three groups to a round, all on A; B stays empty)
                if (i % per == 0) round(RoundForm::Grouped);
                if (one_pipe) rounds.back().g[0][i % 3] = groups[i];
                else rounds.back().g[i % 2][(i % 6) / 2] = groups[i];
            }
            break;
        }
    }
    return rounds;
}

// The rounds of csmp_mp_batch (host/mp_batch.hpp): a round is ONE group per pipeline -- MP has no append stages to rotate, a step of
// a group is its shared pass and one short launch --, up to 2 R signals (R: the members a pass serves).  The fewest passes
// (even_groups), dealt two to a round, A then B.  one_pipe: every
// round holds one group, on A.  split_lone: a round that would hold a single group of two or more signals on A -- a batch of up to R
// signals, the last round of an odd number of groups -- is cut into two halves, A's the larger, so that each half's short launch
// falls under the other's pass (one pass more; kMpSplitLone, host/mp_batch.hpp, says which was faster).
struct MpRound {
    PlanGroup g[2];  // [pipeline: 0 = A, the caller's context; 1 = B, the twin]; member m of a group is solver slot 3 m
};
static std::vector<MpRound> mp_batch_plan(int64_t nsig, int R, bool one_pipe, bool split_lone) {
    std::vector<MpRound> rounds;
    const std::vector<PlanGroup> groups = even_groups(nsig, R);
    for (size_t i = 0; i < groups.size(); ++i) {
        const PlanGroup& g = groups[i];
        if (one_pipe || i % 2 == 0) rounds.emplace_back();
        MpRound& r = rounds.back();
        if (!one_pipe && split_lone && i % 2 == 0 && i + 1 == groups.size() && g.size >= 2) {
            r.g[0] = {g.first, (g.size + 1) / 2};
            r.g[1] = {g.first + (g.size + 1) / 2, g.size / 2};
        } else {
            r.g[one_pipe ? 0 : i % 2] = g;
        }
    }
    return rounds;
}
