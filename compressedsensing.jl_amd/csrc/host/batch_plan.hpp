// host/batch_plan.hpp -- the schedules of csmp_omp_batch / csmp_fr_batch as data: the stage rotation of a tick pipeline and the
// rounds a batch runs in (host/forward.hpp: batch_impl).  Plain C++, no HIP: included by csmp.hip (the library) and, alone, by
// tools/sanitize/hostonly_driver.cpp, which checks every plan a batch of up to 64 signals can get.
#pragma once
#include <cstddef>
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

// The groups of WIDE passes (R members in two halves of up to `narrow`, R >= 2 narrow: every group before the last stays wide): ceil(nsig / R) groups as even_groups has them,
// consecutive signals, the larger first -- but where the last group can be cut to `narrow` signals without another pass it is, and
// runs the narrow pass, which costs 35-45 us less than a wide one at 4096 x 65536 f32 whatever the wide one's halves hold (DESIGN.md
// section 0.3, rounds 15 and 17); the other groups take the rest, full ones first, then one group with what is left:
//   p = ceil(nsig / R) >= 2 and nsig <= R (p - 1) + narrow:  R, ..., R, nsig - narrow - R (p - 2), narrow    (the rest is even: even_groups)
//   R = 8, narrow = 4:  9: 5 + 4   10: 6 + 4   12: 8 + 4   17: 8 + 5 + 4   18: 8 + 6 + 4   20: 8 + 8 + 4;  13 .. 16, 21 .. 24: even
// split: 0 this rule; 1 even_groups (the A/B switch, csmp_tune group_split); 2 and 3 are measurements of the rule's neighbours where it
// applies -- 2: the groups before the narrow one even (18: 7 + 7 + 4), 3: full groups, then what is left (18: 8 + 8 + 2).
// Measured on the benchmark (4096 x 65536 f32, k = 256), atoms/s of a whole call, medians, this rule / even: 18 signals 29 352 / 28 162
// (8 + 8 + 2: 29 109, 7 + 7 + 4: 28 717, one reading each), 20: 32 655 / 30 909, 10: 27 374 / 24 540, 12: 31 554 / 29 180,
// 17: 28 422 / 27 260, 25: 31 059 / 30 078.  The narrow group on B instead (A: 8, 6; B: 4) read x 1.007 / 1.005 at
// 18 / 20 signals, about the parent's run-to-run spread: not adopted.  Not measured: every other size.
static std::vector<PlanGroup> narrow_last_groups(int64_t nsig, int R, int narrow, int split = 0) {
    if (nsig < 1 || R < 1) return {};
    const int64_t p = (nsig + R - 1) / R;
    if (split == 1 || narrow < 1 || 2 * narrow > R || p < 2 || nsig > (int64_t)R * (p - 1) + narrow) return even_groups(nsig, R);
    std::vector<PlanGroup> groups;
    if (split == 2) {
        groups = even_groups(nsig - narrow, R);
    } else {
        const int64_t last = split == 3 ? nsig - (int64_t)R * (p - 1) : narrow;
        for (int64_t at = 0, left = nsig - last; left > 0; at += R, left -= R) groups.push_back({at, (int)(left < R ? left : R)});
        if (split == 3) narrow = (int)last;
    }
    groups.push_back({nsig - narrow, narrow});
    return groups;
}

// The rounds of a batch of nsig signals (R: the members a shared pass serves, ctx->sweep_group or ctx->group_wide).  Pairs: rounds of 3 + 3 while six or
// more signals remain, then 1 + 1, then a lone signal in the one-pipeline form.  Grouped: the fewest shared passes (even_groups; wide
// groups, narrow > 0: narrow_last_groups with that half and split)
// dealt six to a round, even offsets to A and odd ones to B; a last round may leave B with no group and keeps the pair form.
static std::vector<PlanRound> batch_plan(int64_t nsig, BatchSchedule sched, int R, bool one_pipe = false, int narrow = 0, int split = 0) {
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
            const std::vector<PlanGroup> groups = narrow > 0 ? narrow_last_groups(nsig, R, narrow, split) : even_groups(nsig, R);
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
