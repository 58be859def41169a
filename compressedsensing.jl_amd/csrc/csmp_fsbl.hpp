// csmp_fsbl.hpp -- gfx950 kernels of the greedy forms of sparse Bayesian learning, fsbl(A, b, sigma2) and rmps(A, b, sigma2)
// (src/sbl.jl:57-437), for a scalar noise variance (include/csmp.h, csmp_fsbl / csmp_rmps).  The state is alpha (N prior precisions,
// +inf = inactive), Ci = C^-1 (M x M, exactly symmetric), S_j = a_j' C^-1 a_j and Q_j = a_j' C^-1 b.  One step changes ONE alpha_i:
//     v = C^-1 a_i;  den = 1 / gam + S_i;  C^-1 -= v v' / den;  w = A'v;  S -= w^2 / den;  Q -= w Q_i / den
//   k_fsbl_score   the N-pass: first the pending S / Q update of the previous step (w, den and Q_i from the device record), then the
//                  value of every atom for a mode and the partials (best value, lowest index) of every workgroup
//   k_fsbl_pick    one workgroup: the partials folded in index order, the action decided, alpha_i written, the decision record
//   k_fsbl_col     column i (read from the record) of A as doubles
//   k_bp_gemv      (csmp_bp.hpp, BP_FULL, unchanged) v = C^-1 a_i
//   k_fsbl_rank1   C^-1 -= v v' / den, streaming, every element from the same two operands in the same order
//   the product sweep (csmp_kernels.hpp, unchanged) w = A'v
//   k_fsbl_x       x_j = Q_j / alpha_j on the active atoms, 0 elsewhere
//   k_fsbl_score_group, k_fsbl_pick_group, k_fsbl_col_group, k_fsbl_gemv_group, k_fsbl_rank1_group
//                  the same work for every member of a lockstep group of csmp_fsbl_batch / csmp_rmps_batch in ONE launch each: the
//                  single kernels' bodies (fsbl_*_body) on the member's own buffers, the member on the grid's third axis
//
// Determinism: no atomics, no workgroup waits for another, every fold has a fixed order: the same bits on every run.
#pragma once
#include "csmp_bp.hpp"

namespace csmp {

constexpr int kFsblParts = 256;  // most workgroups (and partials) of k_fsbl_score: one per thread of k_fsbl_pick
enum : int { FSBL_MODE_NONE = 0, FSBL_MODE_ALL = 1, FSBL_MODE_ADD = 2, FSBL_MODE_RMP_DEL = 3, FSBL_MODE_UPD = 4 };
enum : int { FSBL_ACT_NONE = 0, FSBL_ACT_ADD = 1, FSBL_ACT_DEL = 2, FSBL_ACT_UPD = 3 };

// the decision record of a step: written by k_fsbl_pick, read by the step's kernels, the next k_fsbl_score and the host
struct FsblRec {
    double value;      // the picked atom's value (the maximum; the minimum in FSBL_MODE_RMP_DEL)
    double alpha_new;  // alpha_i after the action (+inf: deleted)
    double gamma;      // the change of 1 / alpha_i the rank-one step applies
    double den;        // 1 / gamma + S_i
    double Qi;         // Q_i before the step
    long long i;       // the picked atom
    int action;        // FSBL_ACT_*
    int bad;           // 1: a value that is not finite (NaN; an infinite maximum)
    int pending;       // 1: w, den and Qi describe an S / Q update the next N-pass has to apply
    int pad;
};

struct FsblSq {
    double f, s, q;
    bool active, relevant;
};
__device__ __forceinline__ FsblSq fsbl_sq(double a, double S, double Q) {
    FsblSq r;
    r.active = a < __builtin_inf();
    r.f = r.active ? a / (a - S) : 1.0;
    r.s = S * r.f;
    r.q = Q * r.f;
    r.relevant = r.s < r.q * r.q;
    return r;
}
__device__ __forceinline__ double fsbl_opt_alpha(const FsblSq& t) { return t.relevant ? t.s * t.s / (t.q * t.q - t.s) : __builtin_inf(); }
__device__ __forceinline__ double fsbl_d_add(double S, double Q) { return (Q * Q - S) / S + log(S) - log(Q * Q); }
__device__ __forceinline__ double fsbl_d_del(double S, double Q, double a) { return Q * Q / (S - a) - log(1.0 - S / a); }
__device__ __forceinline__ double fsbl_d_upd(double S, double Q, double a, double an) {
    const double d = 1.0 / an - 1.0 / a;
    return Q * Q / (S + 1.0 / d) - log(fmax(1.0 + S * d, 0.0));
}
// the value of one atom: delta of fsbl (FSBL_MODE_ALL), sbl_acquisition_value, rmp_deletion_value (lower is better), sbl_update_value
__device__ __forceinline__ double fsbl_value(int mode, double a, double S, double Q) {
    const FsblSq t = fsbl_sq(a, S, Q);
    if (mode == FSBL_MODE_RMP_DEL) return (t.active && !t.relevant) ? t.q * t.q / t.s : __builtin_inf();
    if (!t.active) return (t.relevant && mode != FSBL_MODE_UPD) ? fsbl_d_add(S, Q) : 0.0;
    if (t.relevant) return mode != FSBL_MODE_ADD ? fsbl_d_upd(S, Q, a, fsbl_opt_alpha(t)) : 0.0;
    return mode == FSBL_MODE_ALL ? fsbl_d_del(S, Q, a) : 0.0;
}
// (v, i) beats (bv, bi): the larger value (the smaller where MIN), the lower index on a tie -- Julia's argmax / findmin
__device__ __forceinline__ bool fsbl_better(bool MIN, double v, long long i, double bv, long long bi) {
    return (MIN ? v < bv : v > bv) || (v == bv && i < bi);
}

// Workgroup g owns the atoms [g per, (g + 1) per), per a multiple of 256.  rec->pending: S_j -= w_j^2 / den and Q_j -= w_j Qi / den come
// first and are stored.  Then the atom's value (vals, where not NULL, receives it), thread bests in index order, the wave's and the
// workgroup's by fsbl_better.  pval[g] / pidx[g]: the workgroup's best; pidx[g] = -1 where a value is NaN or an infinite maximum.
// FSBL_MODE_NONE: the pending update alone.
// blk: the workgroup's index g.
__device__ __forceinline__ void fsbl_score_body(const int blk, const double* __restrict__ alpha, double* __restrict__ S, double* __restrict__ Q,
                                                const double* __restrict__ w, const FsblRec* __restrict__ rec, int64_t N, int64_t per, int mode,
                                                double* __restrict__ vals, double* __restrict__ pval, long long* __restrict__ pidx) {
    __shared__ double sv[4];
    __shared__ long long si[4];
    const bool pend = rec->pending != 0;
    const double den = rec->den, Qi = rec->Qi;
    const bool MIN = mode == FSBL_MODE_RMP_DEL;
    const int64_t j0 = (int64_t)blk * per, j1 = j0 + per < N ? j0 + per : N;
    double bv = MIN ? __builtin_inf() : -__builtin_inf();
    long long bi = 0x7fffffffffffffffLL;
    int bad = 0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        double Sj = S[j], Qj = Q[j];
        if (pend) {
            const double wj = w[j];
            Sj = Sj - wj * wj / den;
            Qj = Qj - wj * Qi / den;
            S[j] = Sj;
            Q[j] = Qj;
        }
        if (mode == FSBL_MODE_NONE) continue;
        const double v = fsbl_value(mode, alpha[j], Sj, Qj);
        if (vals) vals[j] = v;
        if (v != v || (!MIN && !(fabs(v) < __builtin_inf()))) bad = 1;
        if (fsbl_better(MIN, v, j, bv, bi)) {
            bv = v;
            bi = j;
        }
    }
    if (mode == FSBL_MODE_NONE) return;
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = shx(bv, s);
        const long long oi = __shfl_xor(bi, s, kWave);
        if (fsbl_better(MIN, ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    const int anybad = __syncthreads_or(bad);
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = bv;
        si[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k)
            if (fsbl_better(MIN, sv[k], si[k], bv, bi)) {
                bv = sv[k];
                bi = si[k];
            }
        pval[blk] = bv;
        pidx[blk] = anybad ? -1 : bi;
    }
}
__global__ __launch_bounds__(256) void k_fsbl_score(const double* __restrict__ alpha, double* __restrict__ S, double* __restrict__ Q,
                                                    const double* __restrict__ w, const FsblRec* __restrict__ rec, int64_t N, int64_t per, int mode,
                                                    double* __restrict__ vals, double* __restrict__ pval, long long* __restrict__ pidx) {
    fsbl_score_body((int)blockIdx.x, alpha, S, Q, w, rec, N, per, mode, vals, pval, pidx);
}

// One workgroup.  force_i < 0: the nparts partials folded (thread t holds partial t; a workgroup's atoms lie below the next one's, so the
// lowest index of the best value wins), then the action of the mode on the picked atom i -- add where the value is > 0 (FSBL_MODE_ADD),
// delete where the minimum is < 1 (FSBL_MODE_RMP_DEL), re-estimate where it is > 0 (FSBL_MODE_UPD), whichever of the three matches the
// atom where it is > 0 (FSBL_MODE_ALL) -- with alpha_i written and the record filled.  force_i >= 0: the rank-one step of atom force_i
// with the given gamma, alpha untouched (the warm start's replay, the measurement hooks).
__device__ __forceinline__ void fsbl_pick_body(const double* __restrict__ pval, const long long* __restrict__ pidx, int nparts, int mode,
                                               double* __restrict__ alpha, const double* __restrict__ S, const double* __restrict__ Q,
                                               long long force_i, double force_gamma, FsblRec* __restrict__ rec) {
    __shared__ double sv[4];
    __shared__ long long si[4];
    FsblRec r;
    r.pad = 0;
    r.bad = 0;
    if (force_i >= 0) {
        if (threadIdx.x != 0) return;
        r.value = 0.0;
        r.i = force_i;
        r.alpha_new = alpha[force_i];
        r.gamma = force_gamma;
        r.den = 1.0 / force_gamma + S[force_i];
        r.Qi = Q[force_i];
        r.action = FSBL_ACT_ADD;
        r.pending = 1;
        *rec = r;
        return;
    }
    const bool MIN = mode == FSBL_MODE_RMP_DEL;
    double bv = MIN ? __builtin_inf() : -__builtin_inf();
    long long bi = 0x7fffffffffffffffLL;
    int bad = 0;
    if ((int)threadIdx.x < nparts) {
        bv = pval[threadIdx.x];
        bi = pidx[threadIdx.x];
        if (bi < 0) {
            bad = 1;
            bi = 0x7fffffffffffffffLL;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = shx(bv, s);
        const long long oi = __shfl_xor(bi, s, kWave);
        if (fsbl_better(MIN, ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    const int anybad = __syncthreads_or(bad);
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = bv;
        si[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < 4; ++k)
        if (fsbl_better(MIN, sv[k], si[k], bv, bi)) {
            bv = sv[k];
            bi = si[k];
        }
    r.value = bv;
    r.i = bi;
    r.action = FSBL_ACT_NONE;
    r.alpha_new = r.gamma = r.den = r.Qi = 0.0;
    r.bad = anybad;
    if (!anybad && bi != 0x7fffffffffffffffLL) {
        const double a = alpha[bi], Si = S[bi], Qv = Q[bi];
        const FsblSq t = fsbl_sq(a, Si, Qv);
        const double an = fsbl_opt_alpha(t);
        int act = FSBL_ACT_NONE;
        if (MIN) {
            if (bv < 1.0) act = FSBL_ACT_DEL;
        } else if (bv > 0.0) {
            if (!t.active && t.relevant && (mode == FSBL_MODE_ALL || mode == FSBL_MODE_ADD)) act = FSBL_ACT_ADD;
            else if (t.active && !t.relevant && mode == FSBL_MODE_ALL) act = FSBL_ACT_DEL;
            else if (t.active && t.relevant && (mode == FSBL_MODE_ALL || mode == FSBL_MODE_UPD)) act = FSBL_ACT_UPD;
        }
        if (act != FSBL_ACT_NONE) {
            r.alpha_new = act == FSBL_ACT_DEL ? __builtin_inf() : an;
            r.gamma = act == FSBL_ACT_ADD ? 1.0 / an : act == FSBL_ACT_DEL ? -1.0 / a : 1.0 / an - 1.0 / a;
            r.den = 1.0 / r.gamma + Si;
            r.Qi = Qv;
            r.action = act;
            if (!(fabs(r.den) < __builtin_inf()) || r.den == 0.0 || r.alpha_new != r.alpha_new) {
                r.bad = 1;
                r.action = FSBL_ACT_NONE;
            } else {
                alpha[bi] = r.alpha_new;
            }
        }
    }
    r.pending = r.action != FSBL_ACT_NONE ? 1 : 0;
    *rec = r;
}
__global__ __launch_bounds__(256) void k_fsbl_pick(const double* __restrict__ pval, const long long* __restrict__ pidx, int nparts, int mode,
                                                   double* __restrict__ alpha, const double* __restrict__ S, const double* __restrict__ Q,
                                                   long long force_i, double force_gamma, FsblRec* __restrict__ rec) {
    fsbl_pick_body(pval, pidx, nparts, mode, alpha, S, Q, force_i, force_gamma, rec);
}

// col[r] = A[r, i] as a double for r < M, i = rec->i (what lies beyond M in col is zero and stays so).  VEC: the columns of A start on
// 16-byte boundaries -- 16-byte loads over the whole vectors of the column, the rest by elements.
template <typename TA, bool VEC>
__device__ __forceinline__ void fsbl_col_body(const int blk, const TA* __restrict__ A, int64_t ld, int M, const FsblRec* __restrict__ rec,
                                              double* __restrict__ col) {
    constexpr int PERV = 16 / (int)sizeof(TA);
    typedef TA tav __attribute__((ext_vector_type(PERV)));
    const TA* a = A + rec->i * ld;
    const int t = blk * 256 + threadIdx.x;
    if (VEC) {
        const int r0 = t * PERV;
        if (r0 + PERV <= M) {
            const tav x = *reinterpret_cast<const tav*>(a + r0);
#pragma unroll
            for (int c = 0; c < PERV; ++c) col[r0 + c] = (double)x[c];
        } else {
            for (int r = r0; r < M; ++r) col[r] = (double)a[r];
        }
    } else {
#pragma unroll
        for (int c = 0; c < PERV; ++c) {
            const int r = blk * 256 * PERV + c * 256 + threadIdx.x;
            if (r < M) col[r] = (double)a[r];
        }
    }
}
template <typename TA, bool VEC>
__global__ __launch_bounds__(256) void k_fsbl_col(const TA* __restrict__ A, int64_t ld, int M, const FsblRec* __restrict__ rec,
                                                  double* __restrict__ col) {
    fsbl_col_body<TA, VEC>((int)blockIdx.x, A, ld, M, rec, col);
}

// Ci[r, c] -= v[r] v[c] / den (den = rec->den), Ci with the even leading dimension ldc >= M: workgroup (c, y) takes the rows
// 512 y .. 512 y + 511 of column c, a thread two of them with one 16-byte load and store.  The product is rounded (commutative: the
// element (c, r) forms the same), divided, subtracted -- no contraction -- so the matrix stays exactly symmetric.  v is zero from M on.
__device__ __forceinline__ void fsbl_rank1_body(const int64_t c, const int by, double* __restrict__ Ci, int64_t ldc, const double* __restrict__ v,
                                                const FsblRec* __restrict__ rec) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const int64_t r = ((int64_t)by * 256 + threadIdx.x) * 2;
    if (r >= ldc) return;
    const double den = rec->den, vc = v[c];
    const d2 vr = *reinterpret_cast<const d2*>(v + r);
    d2* p = reinterpret_cast<d2*>(Ci + c * ldc + r);
    d2 x = *p;
    x[0] = __dsub_rn(x[0], __ddiv_rn(__dmul_rn(vr[0], vc), den));
    x[1] = __dsub_rn(x[1], __ddiv_rn(__dmul_rn(vr[1], vc), den));
    *p = x;
}
__global__ __launch_bounds__(256) void k_fsbl_rank1(double* __restrict__ Ci, int64_t ldc, const double* __restrict__ v,
                                                    const FsblRec* __restrict__ rec) {
    fsbl_rank1_body((int64_t)blockIdx.x, (int)blockIdx.y, Ci, ldc, v, rec);
}

// Ci = I / sigma2 over the M x M block, zero in the padding rows
__global__ __launch_bounds__(256) void k_fsbl_eye(double* __restrict__ Ci, int64_t ldc, int M, double sigma2) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ldc * M) return;
    Ci[e] = (e % ldc) == (e / ldc) ? 1.0 / sigma2 : 0.0;
}
// S = |a_j|^2 / sigma2 (in place, from k_fr_colnorm2's sums of squares) and Q = (A'b)_j / sigma2
__global__ __launch_bounds__(256) void k_fsbl_scale(double* __restrict__ S, double* __restrict__ Q, int64_t N, double sigma2) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    S[j] = S[j] / sigma2;
    Q[j] = Q[j] / sigma2;
}
__global__ __launch_bounds__(256) void k_fsbl_fill(double* __restrict__ a, int64_t N, double v) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < N) a[j] = v;
}
// the posterior mean on the active atoms: x_j = Q_j / alpha_j (mu = Gamma A' C^-1 b), 0 on the others
__global__ __launch_bounds__(256) void k_fsbl_x(const double* __restrict__ alpha, const double* __restrict__ Q, int64_t N, double* __restrict__ x) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const double a = alpha[j];
    x[j] = a < __builtin_inf() ? Q[j] / a : 0.0;
}

// ---------------------------------------------------------------------------------------------
// The group forms of csmp_fsbl_batch / csmp_rmps_batch (host/fsbl_batch.hpp): ONE launch does a kernel's work for every member of a
// lockstep group that takes part in the tick.  The member is the grid's third axis; its pointers, the mode of its N-pass and a forced
// (atom, gamma) come from this kernel-argument struct, by value.  Every member's workgroups run the single kernels' bodies above on the
// member's own buffers: per member the arithmetic and its order are the single solve's.  turn[m] = 0: the member takes the N-pass only
// (the pending update of a member that is finishing) and leaves k_fsbl_pick_group and the step's kernels at once; the step's kernels
// -- k_fsbl_col_group, k_fsbl_gemv_group, k_fsbl_rank1_group -- also leave where the member's device record holds no action, so a
// tick's launches go out without the host reading a record in between.
struct FsblGroup {
    int n;
    int mode[kBpGroupMax];              // FSBL_MODE_* of the member's N-pass
    int turn[kBpGroupMax];              // 1: the member picks and, where its record says so, steps
    long long force_i[kBpGroupMax];     // >= 0: the forced record of the warm start's replay
    double force_gamma[kBpGroupMax];
    double *alpha[kBpGroupMax], *S[kBpGroupMax], *Q[kBpGroupMax], *w[kBpGroupMax], *pval[kBpGroupMax];
    long long* pidx[kBpGroupMax];
    FsblRec* rec[kBpGroupMax];
    double *Ci[kBpGroupMax], *col[kBpGroupMax], *v[kBpGroupMax];  // C^-1, a_i and v = C^-1 a_i
};
static_assert(sizeof(FsblGroup) <= 4096, "kernel arguments");
__global__ __launch_bounds__(256) void k_fsbl_score_group(const FsblGroup G, int64_t N, int64_t per) {
    const int m = (int)blockIdx.z;
    if (m >= G.n) return;
    fsbl_score_body((int)blockIdx.x, G.alpha[m], G.S[m], G.Q[m], G.w[m], G.rec[m], N, per, G.mode[m], nullptr, G.pval[m], G.pidx[m]);
}
__global__ __launch_bounds__(256) void k_fsbl_pick_group(const FsblGroup G, int nparts) {
    const int m = (int)blockIdx.z;
    if (m >= G.n || !G.turn[m]) return;
    fsbl_pick_body(G.pval[m], G.pidx[m], nparts, G.mode[m], G.alpha[m], G.S[m], G.Q[m], G.force_i[m], G.force_gamma[m], G.rec[m]);
}
template <typename TA, bool VEC>
__global__ __launch_bounds__(256) void k_fsbl_col_group(const TA* __restrict__ A, int64_t ld, int M, const FsblGroup G) {
    const int m = (int)blockIdx.z;
    if (m >= G.n || !G.turn[m] || !G.rec[m]->pending) return;
    fsbl_col_body<TA, VEC>((int)blockIdx.x, A, ld, M, G.rec[m], G.col[m]);
}
// v_m = C_m^-1 a_m: k_bp_gemv's BP_FULL arithmetic for every member, one matrix per member -- a wave per output, the lane partials over
// t = lane in steps of 128 on the chains a0 and a1, the tail into a0, a0 + a1, the butterfly 32 .. 1.
__global__ __launch_bounds__(256) void k_fsbl_gemv_group(int64_t ldc, int M, const FsblGroup G) {
    const int m = (int)blockIdx.z;
    if (m >= G.n || !G.turn[m] || !G.rec[m]->pending) return;
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= M) return;
    const double* __restrict__ col = G.Ci[m] + (int64_t)c * ldc;
    const double* __restrict__ x = G.col[m];
    double a0 = 0.0, a1 = 0.0;
    int t = lane;
    for (; t + 64 < M; t += 128) {
        a0 = fma(col[t], x[t], a0);
        a1 = fma(col[t + 64], x[t + 64], a1);
    }
    if (t < M) a0 = fma(col[t], x[t], a0);
    double a = a0 + a1;
    for (int s = 32; s >= 1; s >>= 1) a += shx(a, s);
    if (lane == 0) G.v[m][c] = a;
}
__global__ __launch_bounds__(256) void k_fsbl_rank1_group(int64_t ldc, const FsblGroup G) {
    const int m = (int)blockIdx.z;
    if (m >= G.n || !G.turn[m] || !G.rec[m]->pending) return;
    fsbl_rank1_body((int64_t)blockIdx.x, (int)blockIdx.y, G.Ci[m], ldc, G.v[m], G.rec[m]);
}

}  // namespace csmp
