// csmp_somp.hpp -- kernels of csmp_somp (host/somp.hpp): simultaneous OMP for the columns of B that share ONE support (S-OMP, Tropp,
// Gilbert and Strauss 2006).  A step is omp's with the residual matrix R in place of r:
//     the passes        c_l = A'r_l and ||r_l||^2 for every column (the shared pass, or one sweep per column)
//     k_somp_pick       s_j = sum_l |c_l[j]|^p, the arg-max partials where k_qr1 (mode 1) takes them, ||R||_F and the eps decision
//     k_qr1 -> k_qr2 -> k_qr3   ONE append of the atom to ONE factorisation (csmp_kernels.hpp, unchanged)
//     k_somp_project    z_l[j] = q'r_l,  r_l -= q z_l[j] for every column, q the new direction
// and at the end k_somp_solve back-substitutes R_fac X = Z for all columns.  The append chain runs on the solver slot with a ZERO
// residual of its own: it serves no column, so every column's z and r come from the same expressions and equal columns of B stay
// equal bit for bit.  No floating-point atomics, every sum in a fixed order: the same bits on every run.
#pragma once
#include "csmp_kernels.hpp"

namespace csmp {

// the columns of one call, in the call's own arrays
struct SompCols {
    int nsig;
    double* R; int64_t ldr;  // residuals: column l from l * ldr, ldr doubles (rows past size(A,1) zero)
    double* C; int64_t ldc;  // c_l = A'r_l of the step's passes: column l from l * ldc
    DevState* st;            // the passes' control blocks, one per column: rnorm2 (written by the pass), done (read by it)
    double* Z; int kcap;     // z_l = Q'b_l: column l from l * kcap
};

// B -> R, the passes' control blocks reset.  Column l owns the wgs = ldr / 256 workgroups from l * wgs
template <typename TB>
__global__ __launch_bounds__(256) void k_somp_init(const TB* __restrict__ B, int64_t ldB, int M, const SompCols g, int wgs) {
    const int l = (int)(blockIdx.x / (unsigned)wgs), i = (int)(blockIdx.x % (unsigned)wgs) * 256 + (int)threadIdx.x;
    if (l >= g.nsig) return;
    if (i < g.ldr) g.R[(int64_t)l * g.ldr + i] = i < M ? (double)B[(int64_t)l * ldB + i] : 0.0;
    if (i == 0) {
        DevState* st = g.st + l;
        st->nsel = 0; st->j = 0; st->cand = -1; st->go = 0; st->done = 0; st->steps = 0; st->go2 = 0; st->pcount = 0;
        st->rnorm2 = 0.0; st->cval = 0.0; st->uncertain = 0; st->rstep = 0.f;
    }
}

// The joint pick.  Workgroup w scores the atoms w * 256 + tid, stepping by the grid: s_j = sum over l = 0, 1, ... of |c_l[j]|
// (P == 1) or c_l[j]^2 (P == 2) -- the c values are the passes' bits, added in COLUMN order, so the score does not depend on how the
// columns were cut into passes -- and leaves its arg-max in better()'s order in pval[w] / pidx[w]: the solver slot's partials, which
// k_qr1 in mode 1 folds with the same order and guards (nblk = this grid).  Workgroup 0 first adds the columns' ||r_l||^2 in column
// order and takes omp's test (src/matchingpursuit.jl:79): below eps the solve is done, and the flag goes to every column's control
// block so that the passes of later steps return at once.  A workgroup that finds the solve done (at entry; the test's flag of
// this very launch included -- what it then does not write, k_qr1 does not read: it sees the same flag) writes nothing.
// nrun: steps whose passes ran (the host's count of passes).
template <int P>
__global__ __launch_bounds__(256) void k_somp_pick(const SompCols g, int64_t N, DevState* st0, double* __restrict__ pval,
                                                  int* __restrict__ pidx, double eps, int check_eps, int skipmask, int* nrun) {
    __shared__ double sv[256];
    __shared__ int si[256];
    __shared__ int stop;
    const int tid = threadIdx.x, w = blockIdx.x, nsig = g.nsig;
    const int done = st0->done;
    if (done & skipmask) {  // (k_qr1's guards ended the solve: STOP_STAG, STOP_FULL)
        if (w == 0)
            for (int l = tid; l < nsig; l += 256) g.st[l].done = done;
        return;
    }
    if (w == 0) {
        if (tid == 0) {
            double f2 = 0.0;
            for (int l = 0; l < nsig; ++l) f2 += g.st[l].rnorm2;
            stop = check_eps && !(sqrt(f2) >= eps);
            *nrun += 1;
        }
        __syncthreads();
        if (stop) {
            for (int l = tid; l < nsig; l += 256) g.st[l].done = done | STOP_EPS;
            if (tid == 0) st0->done = done | STOP_EPS;
            return;
        }
    }
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int64_t j = (int64_t)w * 256 + tid; j < N; j += (int64_t)gridDim.x * 256) {
        const double* __restrict__ c = g.C + j;
        double s = 0.0;
        int l = 0;
        for (; l + 8 <= nsig; l += 8) {  // (eight loads in flight, added in order)
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = c[(int64_t)(l + q) * g.ldc];
#pragma unroll
            for (int q = 0; q < 8; ++q) s = P == 1 ? s + fabs(v[q]) : fma(v[q], v[q], s);
        }
        for (; l < nsig; ++l) {
            const double v = c[(int64_t)l * g.ldc];
            s = P == 1 ? s + fabs(v) : fma(v, v, s);
        }
        if (better(s, (int)j, bv, bi)) {
            bv = s;
            bi = (int)j;
        }
    }
    block_argmax(bv, bi, sv, si);
    if (tid == 0) {
        pval[w] = bv;
        pidx[w] = bi;
    }
}

// Every residual off the direction the append chain committed: workgroup l takes column l, z_l[j] = q'r_l with thread t adding the
// rows t, t + 256, ... in turn and block_sum256 over the threads, then r_l -= q z_l[j].  q = Q[:, j], zero past size(A,1).
// Nothing where the step appended nothing (st0->go == 0: a guard failed, or the solve is done).
__global__ __launch_bounds__(256) void k_somp_project(const SompCols g, const DevState* st0, const double* __restrict__ Q, int64_t ldq) {
    __shared__ double sc[4];
    if (!st0->go) return;
    const int l = blockIdx.x, tid = threadIdx.x, j = st0->j;
    if (l >= g.nsig || j < 0 || j >= g.kcap) return;
    const double* __restrict__ q = Q + (int64_t)j * ldq;
    double* __restrict__ r = g.R + (int64_t)l * g.ldr;
    const int rows = (int)(ldq < g.ldr ? ldq : g.ldr);
    double d = 0.0;
    for (int i = tid; i < rows; i += 256) d = fma(q[i], r[i], d);
    d = block_sum256(d, sc);
    if (tid == 0) g.Z[(int64_t)l * g.kcap + j] = d;
    for (int i = tid; i < rows; i += 256) r[i] = fma(-q[i], d, r[i]);
}

// The end of a solve.  Workgroup l back-substitutes R_fac x = z_l in place (column-oriented, from the last row up: x_i by the
// thread that owns entry i, handed over in LDS; every entry of the vector is touched by its owner alone), so any support length
// is served -- the finish kernels of the single solvers change scheme at 256 columns, this one does not.  Then it writes its
// column of the coefficient block in ASCENDING atom order (row i of val belongs to idx[i]; entries that are exactly zero stay) and
// ||r_l||; workgroup 0 also writes idx, the selection order and the count.  Unused tails: idx, order -1, val 0.
__global__ __launch_bounds__(256) void k_somp_solve(const SompCols g, const DevState* st0, const double* __restrict__ Rf,
                                                   const int* __restrict__ sel, int M, int64_t* __restrict__ idx,
                                                   double* __restrict__ val, int64_t ldval, int64_t* __restrict__ nnz,
                                                   int64_t* __restrict__ order, double* __restrict__ resnorm, int outk) {
    __shared__ double sc[4];
    __shared__ double sx;
    const int l = blockIdx.x, tid = threadIdx.x, kcap = g.kcap;
    if (l >= g.nsig) return;
    const int n = min(min(st0->nsel, kcap), outk);
    double* y = g.Z + (int64_t)l * kcap;
    for (int i = n - 1; i >= 0; --i) {
        const double* __restrict__ col = Rf + (int64_t)i * kcap;
        if (tid == (i & 255)) {
            sx = y[i] / col[i];
            y[i] = sx;
        }
        __syncthreads();
        const double xi = sx;
        for (int c = tid; c < i; c += 256) y[c] = fma(-col[c], xi, y[c]);
        __syncthreads();
    }
    double* __restrict__ v = val + (int64_t)l * ldval;
    for (int t = tid; t < outk; t += 256) {
        if (t >= n) {
            v[t] = 0.0;
            if (l == 0) {
                idx[t] = -1;
                if (order) order[t] = -1;
            }
        }
    }
    for (int t = tid; t < n; t += 256) {
        const int me = sel[t];
        int rank = 0;
        for (int u = 0; u < n; ++u) rank += (int)(sel[u] < me);
        v[rank] = y[t];
        if (l == 0) {
            idx[rank] = me;
            if (order) order[t] = me;
        }
    }
    if (l == 0 && tid == 0) *nnz = n;
    if (resnorm) {
        const double* __restrict__ r = g.R + (int64_t)l * g.ldr;
        double d = 0.0;
        for (int i = tid; i < M; i += 256) d = fma(r[i], r[i], d);
        d = block_sum256(d, sc);
        if (tid == 0) resnorm[l] = sqrt(d);
    }
}

}  // namespace csmp
