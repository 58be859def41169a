// tools/sanitize/hostonly_driver.cpp -- drives the context-free exports of include/csmp.h (host/hostonly.hpp: dictionary files, the
// sharded gather's wire layout) and the round plans of the batch drivers (host/batch_plan.hpp) under gcc's AddressSanitizer +
// UndefinedBehaviorSanitizer.  CPU only: no HIP, no GPU.
// Built and run by tools/sanitize_cpu.sh; argv[1] = tests/golden (the committed dictionary files), argv[2] = a scratch directory.
#include "../../compressedsensing.jl_amd/csrc/host/hostonly.hpp"
#include "../../compressedsensing.jl_amd/csrc/host/batch_plan.hpp"
#include <cstdlib>
#include <string>
#include <vector>

static int fails = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                        \
        }                                                                   \
    } while (0)

static std::vector<char> slurp(const std::string& p) {
    std::vector<char> v;
    if (FILE* f = std::fopen(p.c_str(), "rb")) {
        char buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
        std::fclose(f);
    }
    return v;
}
static void spit(const std::string& p, const std::vector<char>& v, size_t n) {
    FILE* f = std::fopen(p.c_str(), "wb");
    if (!f) { ++fails; return; }
    if (n && std::fwrite(v.data(), 1, n, f) != n) ++fails;
    std::fclose(f);
}

static void dictionary_files(const std::string& golden, const std::string& tmp) {
    struct Case { const char* name; int64_t M, N; int dtype; } cases[] = {{"dict_3x4_f64.csmp", 3, 4, CSMP_F64}, {"dict_5x3_f32.csmp", 5, 3, CSMP_F32}};
    for (const Case& c : cases) {
        const std::string path = golden + "/" + c.name;
        int64_t M = -1, N = -1;
        int dt = -1;
        EXPECT(csmp_dictionary_file_info(path.c_str(), &M, &N, &dt) == CSMP_OK);
        EXPECT(M == c.M && N == c.N && dt == c.dtype);
        EXPECT(csmp_dictionary_file_info(path.c_str(), nullptr, nullptr, nullptr) == CSMP_OK);  // every out pointer is optional
        // the committed file, column by column, through the writer again: the same bytes (leading dimension = the file's, then a
        // caller's array with a LARGER leading dimension)
        const std::vector<char> bytes = slurp(path);
        const size_t es = c.dtype == CSMP_F32 ? 4 : 8;
        const int64_t vec = 16 / (int64_t)es, ld = ((c.M + vec - 1) / vec) * vec;
        EXPECT(bytes.size() == 64 + (size_t)ld * (size_t)c.N * es);
        if (bytes.size() != 64 + (size_t)ld * (size_t)c.N * es) continue;
        const std::string out = tmp + "/rewrite_" + c.name;
        EXPECT(csmp_dictionary_file_write(out.c_str(), bytes.data() + 64, c.M, c.N, ld, c.dtype) == CSMP_OK);
        EXPECT(slurp(out) == bytes);
        const int64_t ld2 = ld + 5;
        std::vector<char> wide((size_t)ld2 * (size_t)c.N * es, (char)0x5a);  // (poison between the columns: it must not reach the file)
        for (int64_t j = 0; j < c.N; ++j) std::memcpy(wide.data() + (size_t)j * ld2 * es, bytes.data() + 64 + (size_t)j * ld * es, (size_t)c.M * es);
        EXPECT(csmp_dictionary_file_write(out.c_str(), wide.data(), c.M, c.N, ld2, c.dtype) == CSMP_OK);
        EXPECT(slurp(out) == bytes);
        // an exactly-sized caller array (ldA == M): the writer must not read past its end (ASan sees it if it does)
        std::vector<char> tight((size_t)c.M * (size_t)c.N * es);
        for (int64_t j = 0; j < c.N; ++j) std::memcpy(tight.data() + (size_t)j * c.M * es, bytes.data() + 64 + (size_t)j * ld * es, (size_t)c.M * es);
        EXPECT(csmp_dictionary_file_write(out.c_str(), tight.data(), c.M, c.N, c.M, c.dtype) == CSMP_OK);
        EXPECT(slurp(out) == bytes);
        // damaged files: every truncation of the header, a wrong magic, a wrong version, a leading dimension that is not M rounded up
        for (size_t cut : {(size_t)0, (size_t)7, (size_t)8, (size_t)40, (size_t)63}) {
            const std::string bad = tmp + "/cut.csmp";
            spit(bad, bytes, cut);
            EXPECT(csmp_dictionary_file_info(bad.c_str(), &M, &N, &dt) == CSMP_EIO);
        }
        for (size_t off : {(size_t)0, (size_t)8, (size_t)12, (size_t)16, (size_t)24, (size_t)32}) {  // magic, version, dtype, M, N, ld
            std::vector<char> bad = bytes;
            bad[off] = (char)(bad[off] ^ 0x7f);
            const std::string bp = tmp + "/bad.csmp";
            spit(bp, bad, bad.size());
            const int rc = csmp_dictionary_file_info(bp.c_str(), &M, &N, &dt);
            EXPECT(rc == CSMP_EIO || (off == 24 && rc == CSMP_OK));  // (N is not cross-checked against the file's length by the header reader)
        }
    }
    int64_t M = 0, N = 0;
    int dt = 0;
    EXPECT(csmp_dictionary_file_info(nullptr, &M, &N, &dt) == CSMP_EINVAL);
    EXPECT(csmp_dictionary_file_info((tmp + "/does_not_exist.csmp").c_str(), &M, &N, &dt) == CSMP_EIO);
    const double a[6] = {1, 2, 3, 4, 5, 6};
    const std::string out = tmp + "/args.csmp";
    EXPECT(csmp_dictionary_file_write(nullptr, a, 3, 2, 3, CSMP_F64) == CSMP_EINVAL);
    EXPECT(csmp_dictionary_file_write(out.c_str(), nullptr, 3, 2, 3, CSMP_F64) == CSMP_EINVAL);
    EXPECT(csmp_dictionary_file_write(out.c_str(), a, 0, 2, 3, CSMP_F64) == CSMP_EINVAL);
    EXPECT(csmp_dictionary_file_write(out.c_str(), a, 3, 0, 3, CSMP_F64) == CSMP_EINVAL);
    EXPECT(csmp_dictionary_file_write(out.c_str(), a, 3, 2, 2, CSMP_F64) == CSMP_EINVAL);   // ldA < M
    EXPECT(csmp_dictionary_file_write(out.c_str(), a, 3, 2, 3, 7) == CSMP_EINVAL);          // no such element type
    EXPECT(csmp_dictionary_file_write((tmp + "/no/such/dir/x.csmp").c_str(), a, 3, 2, 3, CSMP_F64) == CSMP_EIO);
    EXPECT(csmp_dictionary_file_write(out.c_str(), a, 3, 2, 3, CSMP_F64) == CSMP_OK);
    EXPECT(csmp_dictionary_file_info(out.c_str(), &M, &N, &dt) == CSMP_OK && M == 3 && N == 2 && dt == CSMP_F64);
}

static void shard_ranges() {
    for (int64_t nsig = 0; nsig <= 67; ++nsig)
        for (int world = 1; world <= 9; ++world) {
            int64_t expect_lo = 0, smallest = nsig, largest = 0;
            for (int r = 0; r < world; ++r) {
                int64_t lo = -1, hi = -1;
                EXPECT(csmp_shard_range(nsig, r, world, &lo, &hi) == CSMP_OK);
                EXPECT(lo == expect_lo && hi >= lo);
                expect_lo = hi;
                smallest = std::min(smallest, hi - lo);
                largest = std::max(largest, hi - lo);
            }
            EXPECT(expect_lo == nsig);          // contiguous blocks that cover 0 .. nsig
            EXPECT(largest - smallest <= 1);    // sizes differ by at most one
        }
    int64_t lo, hi;
    EXPECT(csmp_shard_range(-1, 0, 1, &lo, &hi) == CSMP_EINVAL);
    EXPECT(csmp_shard_range(4, 0, 0, &lo, &hi) == CSMP_EINVAL);
    EXPECT(csmp_shard_range(4, -1, 2, &lo, &hi) == CSMP_EINVAL);
    EXPECT(csmp_shard_range(4, 2, 2, &lo, &hi) == CSMP_EINVAL);
    EXPECT(csmp_shard_range(4, 0, 2, nullptr, &hi) == CSMP_EINVAL);
    EXPECT(csmp_shard_range(4, 0, 2, &lo, nullptr) == CSMP_EINVAL);
}

static void wire_layout() {
    for (int64_t k : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)128})
        for (int64_t nsig : {(int64_t)0, (int64_t)1, (int64_t)7}) {
            // exactly-sized arrays (std::vector: heap, so that ASan sees one element too far)
            std::vector<int64_t> idx((size_t)(k * nsig)), nnz((size_t)nsig), idx2((size_t)(k * nsig), -7), nnz2((size_t)nsig, -7);
            std::vector<double> val((size_t)(k * nsig)), val2((size_t)(k * nsig), -7.0), packed((size_t)((2 * k + 1) * nsig), -1.0);
            uint64_t sd = 0x243F6A8885A308D3ull + (uint64_t)k * 977 + (uint64_t)nsig;
            auto rnd = [&]() { sd = sd * 6364136223846793005ull + 1442695040888963407ull; return sd >> 11; };
            for (int64_t s = 0; s < nsig; ++s) {
                nnz[(size_t)s] = k ? (int64_t)(rnd() % (uint64_t)(k + 1)) : 0;
                for (int64_t t = 0; t < k; ++t) {
                    idx[(size_t)(s * k + t)] = t < nnz[(size_t)s] ? (int64_t)(rnd() % ((uint64_t)1 << 52)) : -1;  // (exact in Float64 below 2^53)
                    val[(size_t)(s * k + t)] = (double)(int64_t)(rnd() % 2000001) / 1e3 - 1000.0;
                }
            }
            // (data() of an empty vector may be null: the functions take that as a missing argument, so hand them a valid address)
            int64_t di = 0;
            double dd = 0.0;
            auto P = [&](std::vector<int64_t>& v) { return v.empty() ? &di : v.data(); };
            auto Pd = [&](std::vector<double>& v) { return v.empty() ? &dd : v.data(); };
            EXPECT(csmp_pack_results(P(idx), Pd(val), P(nnz), k, nsig, Pd(packed)) == CSMP_OK);
            EXPECT(csmp_unpack_results(Pd(packed), k, nsig, P(idx2), Pd(val2), P(nnz2)) == CSMP_OK);
            EXPECT(idx == idx2 && val == val2 && nnz == nnz2);
            for (int64_t s = 0; s < nsig; ++s) EXPECT(packed[(size_t)(s * (2 * k + 1) + 2 * k)] == (double)nnz[(size_t)s]);
        }
    int64_t i1 = 0, n1 = 0;
    double v1 = 0, p3[3] = {0, 0, 0};
    EXPECT(csmp_pack_results(nullptr, &v1, &n1, 1, 1, p3) == CSMP_EINVAL);
    EXPECT(csmp_pack_results(&i1, nullptr, &n1, 1, 1, p3) == CSMP_EINVAL);
    EXPECT(csmp_pack_results(&i1, &v1, nullptr, 1, 1, p3) == CSMP_EINVAL);
    EXPECT(csmp_pack_results(&i1, &v1, &n1, 1, 1, nullptr) == CSMP_EINVAL);
    EXPECT(csmp_pack_results(&i1, &v1, &n1, -1, 1, p3) == CSMP_EINVAL);
    EXPECT(csmp_pack_results(&i1, &v1, &n1, 1, -1, p3) == CSMP_EINVAL);
    EXPECT(csmp_unpack_results(nullptr, 1, 1, &i1, &v1, &n1) == CSMP_EINVAL);
    EXPECT(csmp_unpack_results(p3, 1, 1, nullptr, &v1, &n1) == CSMP_EINVAL);
    EXPECT(csmp_unpack_results(p3, -1, 1, &i1, &v1, &n1) == CSMP_EINVAL);
}

// the stage rotation: group g's step t sweeps at tick 3t + g, runs its qr1 stage at 3t + g + 1 and its qr2 stage at 3t + g + 2, all
// of it inside the 3k + 2 ticks of a round, and a group of size 0 is never live
static void tick_rotation() {
    for (int64_t k = 1; k <= 5; ++k)
        for (int mask = 0; mask < 8; ++mask) {
            const int size[3] = {mask & 1, (mask >> 1) & 1, 2 * ((mask >> 2) & 1)};
            int stages[3][3] = {};  // [group][sweep, qr1, qr2]: live ticks
            for (int64_t n = 0; n < 3 * k + 2; ++n) {
                const TickStages t = tick_stages(n, k, size);
                EXPECT(t.z == n % 3 && t.y == (n + 2) % 3 && t.x == (n + 1) % 3);
                if (t.az) { EXPECT(n == 3 * t.tz + t.z && t.tz < k); stages[t.z][0] += 1; }
                if (t.ay) stages[t.y][1] += 1;
                if (t.ax) stages[t.x][2] += 1;
                EXPECT(!t.ay || (n - 1 - t.y) % 3 == 0);
                EXPECT(!t.ax || (n - 2 - t.x) % 3 == 0);
            }
            for (int g = 0; g < 3; ++g)
                for (int st = 0; st < 3; ++st) EXPECT(stages[g][st] == (size[g] > 0 ? (int)k : 0));
        }
}

// every plan of nsig 1..64 signals: each signal in exactly one (round, pipeline, group, member), the members of a group consecutive,
// no solver slot at or above 3 * kWideMax (= kSlots, host/ctx.hpp), and the round shapes of each schedule.  R: the members of a
// pass, up to 8 with wide groups (two halves of up to four).
static void batch_plans() {
    const int kSlots = 3 * 8;
    for (int64_t nsig = 1; nsig <= 64; ++nsig)
        for (int R = 1; R <= 8; ++R)
            for (BatchSchedule sched : {BatchSchedule::Signals, BatchSchedule::One, BatchSchedule::Pairs, BatchSchedule::Grouped})
              // the grouped schedule's split (narrow_last_groups): narrow 0 and split 1 are the even split, as is every R < 2 narrow; split 0
              // the rule, 2 and 3 its measured neighbours
              for (int mode = 0; mode < (sched == BatchSchedule::Grouped ? 5 : 1); ++mode) {
                const int narrow = mode == 0 ? 0 : 4, split = mode == 0 ? 0 : mode - 1;
                const std::vector<PlanRound> plan = batch_plan(nsig, sched, R, false, narrow, split);
                if (sched == BatchSchedule::Signals) {
                    EXPECT(plan.empty());
                    continue;
                }
                std::vector<int> seen((size_t)nsig, 0);
                int64_t next = 0;  // signals are dealt in order: A's groups, then B's, within a round
                int prev_size = 0;
                const int64_t ngroups = (nsig + R - 1) / R;
                for (size_t j = 0; j < plan.size(); ++j) {
                    const PlanRound& r = plan[j];
                    int count[2] = {0, 0}, live[2] = {0, 0};
                    for (int p = 0; p < 2; ++p)
                        for (int g = 0; g < 3; ++g) {
                            const PlanGroup& G = r.g[p][g];
                            EXPECT(G.size >= 0);
                            if (G.size == 0) continue;
                            EXPECT(g + 3 * (G.size - 1) < kSlots);
                            for (int m = 0; m < G.size; ++m) {
                                EXPECT(G.first + m >= 0 && G.first + m < nsig);
                                if (G.first + m >= 0 && G.first + m < nsig) seen[(size_t)(G.first + m)] += 1;
                            }
                            count[p] += G.size;
                            live[p] += 1;
                        }
                    if (sched == BatchSchedule::One) {
                        // rounds of three consecutive signals on A, the last one 1 or 2 when nsig is not a multiple of three
                        EXPECT(r.form == RoundForm::One && count[1] == 0);
                        EXPECT(count[0] == (int)std::min<int64_t>(3, nsig - 3 * (int64_t)j));
                        for (int g = 0; g < count[0]; ++g) EXPECT(r.g[0][g].first == next + g && r.g[0][g].size == 1);
                    } else if (sched == BatchSchedule::Pairs) {
                        const int64_t left = nsig - next;
                        if (left >= 6) {
                            EXPECT(r.form == RoundForm::Pair && count[0] == 3 && count[1] == 3);
                            for (int g = 0; g < 3; ++g) EXPECT(r.g[0][g].first == next + g && r.g[1][g].first == next + 3 + g);
                        } else if (left >= 2) {
                            EXPECT(r.form == RoundForm::Pair && count[0] == 1 && count[1] == 1);
                            EXPECT(r.g[0][0].first == next && r.g[1][0].first == next + 1);
                        } else {  // the lone last signal: the one-pipeline form
                            EXPECT(j + 1 == plan.size() && r.form == RoundForm::One && count[0] == 1 && count[1] == 0);
                            EXPECT(r.g[0][0].first == next);
                        }
                    } else {
                        // six groups to a round (fewer in the last), dealt A, B, A, B, ... in slot order; a last round with no group on B
                        // keeps the pair form
                        EXPECT(r.form == RoundForm::Grouped);
                        const int64_t in_round = std::min<int64_t>(6, ngroups - 6 * (int64_t)j);
                        EXPECT(live[0] == (int)(in_round + 1) / 2 && live[1] == (int)in_round / 2);
                        // the rule applies to wide groups where the last one can be cut to `narrow` signals without another pass; then
                        // every group before the last is a wide one (more than `narrow` members), split 0: full groups, one with the
                        // rest, and `narrow`; split 2: the groups before the last within one of each other; split 3: full groups, the rest
                        const bool ruled = narrow > 0 && R >= 2 * narrow && split != 1 && ngroups >= 2 && nsig <= (int64_t)R * (ngroups - 1) + narrow;
                        for (int64_t i = 0; i < in_round; ++i) {
                            const PlanGroup& G = r.g[i % 2][i / 2];
                            const int64_t gi = 6 * (int64_t)j + i;
                            int want = (int)(nsig / ngroups + (gi < nsig % ngroups ? 1 : 0));
                            if (ruled) {
                                const int64_t last = split == 3 ? nsig - (int64_t)R * (ngroups - 1) : narrow, rest = nsig - last;
                                const int64_t before = ngroups - 1;
                                if (gi == before) want = (int)last;
                                else if (split == 2) want = (int)(rest / before + (gi < rest % before ? 1 : 0));
                                else want = (int)std::min<int64_t>(R, rest - R * gi);
                                if (gi < before) EXPECT(G.size > narrow);
                            }
                            EXPECT(G.first == next && G.size == want && G.size >= 1 && G.size <= R);
                            if (gi > 0) EXPECT(G.size <= prev_size);  // the larger first
                            prev_size = G.size;
                            next += G.size;
                        }
                        continue;
                    }
                    next += count[0] + count[1];
                }
                EXPECT(next == nsig);
                if (sched == BatchSchedule::Grouped) EXPECT((int64_t)plan.size() == (ngroups + 5) / 6);
                for (int64_t s = 0; s < nsig; ++s) EXPECT(seen[(size_t)s] == 1);
              }
    const int want18[3] = {8, 6, 4}, want20[3] = {8, 8, 4};
    const std::vector<PlanGroup> g18 = narrow_last_groups(18, 8, 4), g20 = narrow_last_groups(20, 8, 4);
    EXPECT(g18.size() == 3 && g20.size() == 3);
    for (size_t i = 0; i < 3 && g18.size() == 3 && g20.size() == 3; ++i) EXPECT(g18[i].size == want18[i] && g20[i].size == want20[i]);
}

// every plan csmp_mp_batch can get for nsig 1..64 (host/batch_plan.hpp: mp_batch_plan): each signal in exactly one group, the groups
// consecutive and in order (A's, then B's, round by round), none above its cap R, the fewest passes unless a lone group is split,
// B empty on one pipeline, and no round of two pipelines with a group on B only
static void mp_batch_plans() {
    for (int64_t nsig = 1; nsig <= 64; ++nsig)
        for (int R = 1; R <= 8; ++R)
            for (int mode = 0; mode < 4; ++mode) {
                const bool one_pipe = (mode & 1) != 0, split = (mode & 2) != 0;
                const std::vector<MpRound> plan = mp_batch_plan(nsig, R, one_pipe, split);
                std::vector<int> seen((size_t)nsig, 0);
                const int64_t ngroups = (nsig + R - 1) / R;
                int64_t next = 0, groups = 0;
                for (size_t j = 0; j < plan.size(); ++j) {
                    const MpRound& r = plan[j];
                    EXPECT(r.g[0].size >= 1);  // (a round always has a group on A)
                    if (one_pipe) EXPECT(r.g[1].size == 0);
                    for (int p = 0; p < 2; ++p) {
                        const PlanGroup& G = r.g[p];
                        EXPECT(G.size >= 0 && G.size <= R && 3 * (G.size - 1) < 3 * 8);
                        if (G.size == 0) continue;
                        EXPECT(G.first == next);
                        for (int m = 0; m < G.size; ++m)
                            if (G.first + m >= 0 && G.first + m < nsig) seen[(size_t)(G.first + m)] += 1;
                        next += G.size;
                        groups += 1;
                    }
                    if (!one_pipe && j + 1 < plan.size()) EXPECT(r.g[1].size >= 1);  // (only the last round may leave B idle)
                    if (!one_pipe && r.g[1].size > 0) EXPECT(r.g[0].size - r.g[1].size >= 0 && r.g[0].size - r.g[1].size <= 1);
                }
                EXPECT(next == nsig);
                for (int64_t s = 0; s < nsig; ++s) EXPECT(seen[(size_t)s] == 1);
                const bool was_split = !one_pipe && split && ngroups % 2 == 1 && (nsig / ngroups) >= 2;
                EXPECT(groups == ngroups + (was_split ? 1 : 0));
                EXPECT((int64_t)plan.size() == (one_pipe ? ngroups : (ngroups + 1) / 2));
            }
    EXPECT(mp_batch_plan(0, 8, false, false).empty() && mp_batch_plan(5, 0, false, false).empty());
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <tests/golden> <scratch directory>\n", argv[0]);
        return 2;
    }
    dictionary_files(argv[1], argv[2]);
    shard_ranges();
    wire_layout();
    tick_rotation();
    batch_plans();
    mp_batch_plans();
    std::printf("hostonly_driver: %s (%d failed expectation(s))\n", fails ? "FAILED" : "ok", fails);
    return fails ? 1 : 0;
}
