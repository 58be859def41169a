// csmp_analysis.hpp -- gfx950 kernels of the dictionary analysis: colnorms (src/util.jl:2) and coherence / babel / cumbabel
// (src/util.jl:96-115) on the resident dictionary, in Float64 on the exactly promoted values.
//
// cumbabel(A, k) is N product sweeps whose "residuals" are the columns of A themselves, i.e. the GEMM A'A with a top-k epilogue
// per row.  The N x N matrix is never held: the host walks over strips of 128 query columns,
//   k_gram_strip    the 128 x N strip |a_q' a_j| (times 1 / (|a_q| |a_j|) under normalize, exactly 0.0 at j = q) on the Float64
//                   matrix cores -- k_fr_rebuild_lds's inner loop with the directions read from A itself
//   k_babel_rows    one workgroup per query row: the k largest entries in descending order, their running sums, and the row's
//                   largest entry off the diagonal with the lowest atom index among equals
//   k_babel_fold    mu[m] = max(mu[m], the strip's running sums), and the running best pair (i < j)
// No kernel waits for another workgroup and none uses a floating-point atomic: the k largest of a row are found by a radix
// selection on the bit patterns (integer LDS counters, whose order does not reach the result), sorted, and added in that order,
// so two runs give the same bits.
#pragma once
#include "csmp_kernels.hpp"
#include "csmp_forward.hpp"

namespace csmp {

constexpr int kGramQ = kRbDirs;        // query columns of a strip (the 128 directions k_fr_rebuild_lds stages)
constexpr int kBabelThreads = 256;
constexpr int kBabelCap = 1024;        // entries k_babel_rows sorts in the LDS: CSMP_BABEL_KMAX
struct BabelBest {                     // the running best pair of a call (device memory, written by k_babel_fold only)
    double val;
    long long i, j;
};

// s[j] = |a_j| (mode 0) or 1 / |a_j|, 0 for a zero column (mode 1), from the sums of squares k_fr_colnorm2 left in s
__global__ __launch_bounds__(256) void k_an_root(double* __restrict__ s, int64_t N, int mode) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const double n = sqrt(s[j]);
    s[j] = mode == 0 ? n : (n > 0.0 ? 1.0 / n : 0.0);
}

// strip[q][atom] = |a_{q0+q}' a_atom| * (scale[q0+q] * scale[atom]) for q < min(128, N - q0), atom < N; exactly 0.0 where
// atom == q0 + q.  scale == nullptr: no factor.  Grid: ceil(N / 128) workgroups of 256 threads (a wave owns 2 x 16 atoms),
// fr_rebuild_lds_bytes() of dynamic LDS.  The 128 x 64 block of the query columns a row block needs is read ONCE per workgroup
// at the dictionary's stride and element type, promoted, and double-buffered in the LDS at the 66-double row stride; the next
// block (queries and atoms) is fetched into registers while the matrix cores work on the current one.  Every steady row block
// is loaded unguarded; the last one clamps its row indices into the column and masks what lies beyond M.  Queries past N are
// staged as zeros, atoms past N are clamped for the loads and not stored.
template <typename TA, bool VEC>
__global__ __launch_bounds__(256) void k_gram_strip(const TA* __restrict__ A, int64_t ld, int M, int64_t N, int64_t q0,
                                                    const double* __restrict__ scale, double* __restrict__ strip, int64_t lds) {
    typedef double d4 __attribute__((ext_vector_type(4)));
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef TA ta4 __attribute__((ext_vector_type(16 / sizeof(TA))));
    typedef TA ta2 __attribute__((ext_vector_type(2)));
    constexpr int NA = 2, NT = kRbDirs / 16, PERV = 16 / (int)sizeof(TA), NV = 16 / PERV;
    extern __shared__ double qlds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int nd = (int)(N - q0 < kRbDirs ? N - q0 : kRbDirs);
    const int64_t a0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * NA);
    const TA* acol[NA];
#pragma unroll
    for (int h = 0; h < NA; ++h) {
        const int64_t atom = a0 + h * 16 + fr < N ? a0 + h * 16 + fr : N - 1;
        acol[h] = A + atom * ld + fq * 16;
    }
    // loader: thread -> row pair tid % 32 of query tid / 32 + 8 j (32 threads cover the 64 rows of a query's block)
    const int lrp = tid & 31, ldir = tid >> 5;
    const TA* qsrc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int dir = ldir + 8 * j;
        qsrc[j] = A + (q0 + (dir < nd ? dir : 0)) * ld;
    }
    ta2 stage[16];
    TA raw[NA][16];
    d4 acc[NA][NT];
#pragma unroll
    for (int h = 0; h < NA; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[h][t] = d4{0.0, 0.0, 0.0, 0.0};
    const int nrb = (M + kRbRows - 1) / kRbRows;

    auto fetch_q_full = [&](int rb) {
        const int r = rb * kRbRows + lrp * 2;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (VEC) {
                stage[j] = *reinterpret_cast<const ta2*>(qsrc[j] + r);
            } else {
                stage[j][0] = qsrc[j][r];
                stage[j][1] = qsrc[j][r + 1];
            }
        }
    };
    auto fetch_q_last = [&](int rb) {  // rows clamped into the column, and zero beyond M
        const int r = rb * kRbRows + lrp * 2;
#pragma unroll
        for (int j = 0; j < 16; ++j)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const TA x = qsrc[j][r + c < M ? r + c : M - 1];
                stage[j][c] = r + c < M ? x : (TA)0;
            }
    };
    auto store_q = [&](int buf) {
        double* dst = qlds + (size_t)buf * kRbDirs * kRbStride + lrp * 2;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int dir = ldir + 8 * j;
            *reinterpret_cast<d2*>(dst + dir * kRbStride) = dir < nd ? d2{(double)stage[j][0], (double)stage[j][1]} : d2{0.0, 0.0};
        }
    };
    auto fetch_a_full = [&](int rb) {
#pragma unroll
        for (int h = 0; h < NA; ++h) {
            if (VEC) {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const ta4 x = *(reinterpret_cast<const ta4*>(acol[h] + (int64_t)rb * kRbRows) + v);
#pragma unroll
                    for (int c = 0; c < PERV; ++c) raw[h][v * PERV + c] = x[c];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) raw[h][e] = acol[h][(int64_t)rb * kRbRows + e];
            }
        }
    };
    auto fetch_a_last = [&](int rb) {  // row indices clamped into the column; the operand is masked below
        const int r0 = rb * kRbRows + fq * 16;
#pragma unroll
        for (int h = 0; h < NA; ++h)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = r0 + e < M ? r0 + e : M - 1;
                raw[h][e] = acol[h][row - fq * 16];
            }
    };
    auto compute = [&](int buf, const double (&bv)[NA][16]) {
        const double* src = qlds + (size_t)buf * kRbDirs * kRbStride + fq * 16;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            double qv[16];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const d2 x = *reinterpret_cast<const d2*>(src + (t * 16 + fr) * kRbStride + 2 * e);
                qv[2 * e] = x[0];
                qv[2 * e + 1] = x[1];
            }
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
#pragma unroll
                for (int h = 0; h < NA; ++h) acc[h][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[kk], bv[h][kk], acc[h][t], 0, 0, 0);
        }
    };

    if (nrb > 1) {
        fetch_q_full(0);
        fetch_a_full(0);
    } else {
        fetch_q_last(0);
        fetch_a_last(0);
    }
    store_q(0);
    __syncthreads();
    int buf = 0;
    for (int rb = 0; rb + 1 < nrb; ++rb) {
        double bv[NA][16];
#pragma unroll
        for (int h = 0; h < NA; ++h)
#pragma unroll
            for (int e = 0; e < 16; ++e) bv[h][e] = (double)raw[h][e];
        if (rb + 2 < nrb) {
            fetch_q_full(rb + 1);
            fetch_a_full(rb + 1);
        } else {
            fetch_q_last(rb + 1);
            fetch_a_last(rb + 1);
        }
        compute(buf, bv);
        store_q(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    {
        double bv[NA][16];
        const int r0 = (nrb - 1) * kRbRows + fq * 16;
#pragma unroll
        for (int h = 0; h < NA; ++h)
#pragma unroll
            for (int e = 0; e < 16; ++e) bv[h][e] = r0 + e < M ? (double)raw[h][e] : 0.0;
        compute(buf, bv);
    }
    // the queries' factors through the LDS (every workgroup is done with the staged blocks)
    __syncthreads();
    if (tid < kRbDirs) qlds[tid] = scale ? (tid < nd ? scale[q0 + tid] : 0.0) : 1.0;
    __syncthreads();
    if (a0 >= N) return;
    // C/D layout: col = lane & 15 (atom), row = (lane >> 4) + 4 reg (query within the tile): for a fixed query the 16 lanes of a
    // quarter store 16 consecutive atoms, 128 contiguous bytes
#pragma unroll
    for (int h = 0; h < NA; ++h) {
        const int64_t atom = a0 + h * 16 + fr;
        if (atom >= N) continue;
        const double sa = scale ? scale[atom] : 1.0;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int q = t * 16 + fq + 4 * reg;
                if (q >= nd) continue;
                const double v = fabs(acc[h][t][reg]) * (qlds[q] * sa);  // (the factor is symmetric in the pair, and 1.0 without normalize)
                strip[(int64_t)q * lds + atom] = q0 + q == atom ? 0.0 : v;
            }
    }
}

// One workgroup per query row of a strip (row blockIdx.x is query q0 + blockIdx.x): the k largest of the row's N entries, sorted
// in descending order, their running sums added in that order -> rowcum[row][0..k); the row's largest entry off the diagonal and
// the lowest atom index that holds it -> rowtop / rowarg (rowarg = -1 when N = 1).
// The entries are non-negative, so their bit patterns order like the values.  Selection: passes over the row from the most
// significant byte down; each counts the keys that share the prefix found so far by their next byte (integer LDS counters) and
// picks the byte that holds the k-th largest.  As soon as the keys at or above the chosen prefix number at most kBabelCap they
// are collected and sorted in the LDS; when all eight bytes are fixed and more than that remain (many equal values) the keys
// ABOVE the k-th largest are collected and the rest of the k are copies of it.  Which of several equal entries is taken does
// not reach the sums; the reported index is found by comparison, not by the selection.
__global__ __launch_bounds__(kBabelThreads) void k_babel_rows(const double* __restrict__ strip, int64_t lds, int64_t N, int64_t q0, int k,
                                                              double* __restrict__ rowcum, double* __restrict__ rowtop,
                                                              long long* __restrict__ rowarg) {
    typedef unsigned long long u64;
    typedef u64 u64x2 __attribute__((ext_vector_type(2)));
    __shared__ unsigned hist[256];
    __shared__ u64 buf[kBabelCap];
    __shared__ u64 sv[kBabelThreads];
    __shared__ long long si[kBabelThreads];
    __shared__ u64 s_prefix;
    __shared__ unsigned s_above, s_inb, s_cnt;
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    const u64* row = reinterpret_cast<const u64*>(strip + (int64_t)blockIdx.x * lds);
    const int64_t self = q0 + blockIdx.x;
    if (tid == 0) {
        s_prefix = 0;
        s_above = 0;
        s_cnt = 0;
        s_stop = 0;
    }
    u64 bestk = 0;
    long long besti = -1;
    int pass = 0;
    for (; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        const u64 prefix = s_prefix;
        // (the rows of the strip start on 128-byte boundaries: pairs of entries, the second masked at an odd N's end)
        for (int64_t i = (int64_t)tid * 2; i < N; i += 2 * kBabelThreads) {
            const u64x2 x = *reinterpret_cast<const u64x2*>(row + i);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (i + c >= N) continue;
                const u64 key = x[c];
                if (pass == 0) {
                    atomicAdd(&hist[(unsigned)(key >> 56)], 1u);
                    if (i + c != self && (besti < 0 || key > bestk)) {  // (ascending i per thread: '>' keeps the first maximum)
                        bestk = key;
                        besti = i + c;
                    }
                } else if ((key >> (shift + 8)) == (prefix >> (shift + 8))) {
                    atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned need = (unsigned)k - s_above;  // >= 1: fewer than k keys lie above the prefix
            unsigned cum = 0;
            int b = 255;
            for (; b > 0; --b) {
                if (cum + hist[b] >= need) break;
                cum += hist[b];
            }
            s_prefix = prefix | ((u64)b << shift);
            s_above += cum;
            s_inb = hist[b];
            s_stop = s_above + hist[b] <= (unsigned)kBabelCap;
        }
        __syncthreads();
        if (s_stop) break;
    }
    // pass == 8: every byte is fixed, s_prefix IS the k-th largest key and more than kBabelCap keys are at or above it
    const bool exact = pass == 8;
    const u64 low = s_prefix;
    const unsigned above = s_above;
    const int n = exact ? k : (int)(above + s_inb);  // entries to sort: >= k
    for (int64_t i = (int64_t)tid * 2; i < N; i += 2 * kBabelThreads) {
        const u64x2 x = *reinterpret_cast<const u64x2*>(row + i);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (i + c >= N) continue;
            const u64 key = x[c];
            if (exact ? key > low : key >= low) {
                const unsigned pos = atomicAdd(&s_cnt, 1u);
                if (pos < (unsigned)kBabelCap) buf[pos] = key;
            }
        }
    }
    int P = 1;
    while (P < n) P <<= 1;
    __syncthreads();
    for (int t = tid; t < P; t += kBabelThreads)
        if (t >= (int)(exact ? above : (unsigned)n)) buf[t] = t < n ? low : 0;  // (copies of the k-th largest; zeros up to the power of two)
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += kBabelThreads) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const u64 a = buf[lo], b = buf[hi];
                const bool desc = (lo & size) == 0;
                if ((a < b) == desc && a != b) {
                    buf[lo] = b;
                    buf[hi] = a;
                }
            }
            __syncthreads();
        }
    if (tid == 0) {  // the running sums, added in descending order of the entries
        double c = 0.0;
        for (int m = 0; m < k; ++m) {
            c += __longlong_as_double((long long)buf[m]);
            buf[m] = (u64)__double_as_longlong(c);
        }
    }
    // the row's largest entry off the diagonal, the lowest index among equals
    sv[tid] = bestk;
    si[tid] = besti;
    __syncthreads();
    for (int s = kBabelThreads / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            const u64 ov = sv[tid + s];
            const long long oi = si[tid + s];
            const long long mi = si[tid];
            if (oi >= 0 && (mi < 0 || ov > sv[tid] || (ov == sv[tid] && oi < mi))) {
                sv[tid] = ov;
                si[tid] = oi;
            }
        }
        __syncthreads();
    }
    for (int m = tid; m < k; m += kBabelThreads) rowcum[(int64_t)blockIdx.x * kBabelCap + m] = __longlong_as_double((long long)buf[m]);
    if (tid == 0) {
        rowtop[blockIdx.x] = __longlong_as_double((long long)sv[0]);
        rowarg[blockIdx.x] = si[0];
    }
}

// start of a call: mu = 0, no pair
__global__ __launch_bounds__(256) void k_babel_init(double* __restrict__ mu, BabelBest* __restrict__ best) {
    for (int m = threadIdx.x; m < kBabelCap; m += 256) mu[m] = 0.0;
    if (threadIdx.x == 0) *best = BabelBest{-1.0, -1, -1};
}

// One workgroup per strip: mu[m] = max(mu[m], rowcum[q][m]) over the strip's nq queries, and the running best pair -- the largest
// entry, among equals the lowest i, then the lowest j, with i < j ((i, j) and (j, i) carry the same value).
__global__ __launch_bounds__(256) void k_babel_fold(const double* __restrict__ rowcum, const double* __restrict__ rowtop,
                                                    const long long* __restrict__ rowarg, int nq, int64_t q0, int k,
                                                    double* __restrict__ mu, BabelBest* __restrict__ best) {
    for (int m = threadIdx.x; m < k; m += 256) {
        double v = mu[m];
        for (int q = 0; q < nq; ++q) v = fmax(v, rowcum[(int64_t)q * kBabelCap + m]);
        mu[m] = v;
    }
    if (threadIdx.x == 0) {
        BabelBest b = *best;
        for (int q = 0; q < nq; ++q) {
            const long long a = rowarg[q];
            if (a < 0) continue;
            const double v = rowtop[q];
            const long long i = a < q0 + q ? a : q0 + q, j = a < q0 + q ? q0 + q : a;
            if (v > b.val || (v == b.val && (i < b.i || (i == b.i && j < b.j)))) b = BabelBest{v, i, j};
        }
        *best = b;
    }
}

}  // namespace csmp
